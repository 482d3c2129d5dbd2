// The column skeleton of the loss nodes that put a ray potential on grid_wh: cost(ray) = sum_k p_k psi_k over the
// ray-termination probabilities.  One lane per (y, x) ray, the z column in registers: D pass + occupancy scale/clamp + the
// DRC recurrence forward, the division-free adjoint recurrence + the adjoint D pass backward, ds handed over inside the
// launch.  What a loss brings is its potential, a small struct uniform per launch (DepthPot in dpc_depth.hip, MaskPot in
// dpc_drc_loss.hip); the kernels are thin __global__ shells around the four bodies below.  Design notes: DESIGN.md section 4.
//
// A potential Pot supplies
//   struct Fwd                                   a ray's forward state, zero for a ray outside the image
//   fwd_read(f, P, b, prow, pcol)                what the ray reads before its column is loaded
//   fwd_add(f, z, D, e_eps, y, A)                voxel z: clamped occupancy y, A = prod_{j<z} (1 - y_j)
//   fwd_close(f, P, e_eps, A)                    the background term, A = A_D
//   fwd_epilogue(f, P, bk, ray, live, tiles)     the whole block: outputs, this tile's share of the loss
//   struct Bwd                                   what the ray reads before its column is loaded (bwd_read)
//   bwd_start(r, P, e_eps)                       R_{D-1}, in the form the potential carries R
//   bwd_term(r, P, m, D, e_eps)                  E_m psi_m in the same form (E_0 = e^eps, else 1)
//   bwd_grad(r, P, R)                            the gradient arriving at the ray, from the final R = R_{-1}
// in its own arithmetic, operation for operation: the skeleton never asks which loss it serves.
#pragma once
#include <type_traits>

#include "dpc_kernels.h"

namespace dpck {

// ------------------------------------------------------------------------------------------------------
// Forward: D pass + scale/clamp + DRC recurrence + the potential's sums.            grid (ceil(HW/256) * B)
//   p_0 = e^eps y_0, p_k = y_k A_k, p_D = e^eps A_D, A_k = prod_{j<k} (1 - y_j)   (k_drc_fwd, dpc_stages.hip)
// ------------------------------------------------------------------------------------------------------
template <class Pot, int DD, int RB>
__device__ __forceinline__ void ray_column_fwd(const DpcParams& P, const RayHost& rh, double e_eps,
                                               const float* __restrict__ grid_wh, const float* __restrict__ s,
                                               const TapsT<RB>& taps_arg, const Pot& pot, float* __restrict__ loss_tiles) {
  const TapsT<RB> taps = resolve_taps<RB>(taps_arg, P.dev_taps_z, P.taps_z, false);
  const int HW = P.H * P.W;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const bool live = ray < HW;
  const RayConst rc = ray_const(rh, s, b);
  typename Pot::Fwd f;
  if (live) {
    pot.fwd_read(f, P, b, P.H - 1 - ray / P.W, ray % P.W);   // before the column is loaded
    float c[DD];
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grid_wh + (size_t)b * DD * HW), 0, DD * HW * 4, 0x00020000);
#pragma unroll
    for (int z = 0; z < DD; ++z) c[z] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, ray * 4, z * HW * 4, 0));  // one lane offset, plane offsets in SGPRs
    double A = 1.0;
#pragma unroll
    for (int z = 0; z < DD; ++z) {
      float v2 = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * RB + 1; ++k) {
        const int zz = z + k - RB;
        if (zz >= 0 && zz < DD) v2 = fmaf(taps.w[k], c[zz], v2);
      }
      const double y = (double)drc_clamp(rc, occupancy(rc, v2));
      pot.fwd_add(f, z, DD, e_eps, y, A);
      A *= 1.0 - y;
      if ((z & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    pot.fwd_close(f, P, e_eps, A);
  }
  pot.fwd_epilogue(f, P, bk, ray, live, loss_tiles);
}

// Generic depth / tap count: same arithmetic, column re-read from global (L1/L2 serve the re-reads).
template <class Pot>
__device__ __forceinline__ void ray_column_fwd_dyn(const DpcParams& P, const RayHost& rh, double e_eps,
                                                   const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                   const TapsDyn& taps, const Pot& pot, float* __restrict__ loss_tiles) {
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const bool live = ray < HW;
  const RayConst rc = ray_const(rh, s, b);
  typename Pot::Fwd f;
  if (live) {
    pot.fwd_read(f, P, b, P.H - 1 - ray / P.W, ray % P.W);
    const float* col = grid_wh + (size_t)b * D * HW + ray;
    const int R = taps.n > 0 ? (taps.n - 1) / 2 : 0;
    double A = 1.0;
    for (int z = 0; z < D; ++z) {
      float v2;
      if (taps.n == 0) {
        v2 = col[(size_t)z * HW];
      } else {
        v2 = 0.f;
        for (int k = 0; k < taps.n; ++k) {
          const int zz = z + k - R;
          if (zz >= 0 && zz < D) v2 = fmaf(dyn_tap(taps, P.dev_taps_z, k), col[(size_t)zz * HW], v2);
        }
      }
      const double y = (double)drc_clamp(rc, occupancy(rc, v2));
      pot.fwd_add(f, z, D, e_eps, y, A);
      A *= 1.0 - y;
    }
    pot.fwd_close(f, P, e_eps, A);
  }
  pot.fwd_epilogue(f, P, bk, ray, live, loss_tiles);
}

// ------------------------------------------------------------------------------------------------------
// Backward: d cost -> DRC adjoint -> clamp masks -> adjoint D pass.                 grid (ceil(HW/256) * B)
//
// With R_m = (sum_{k>m} psi_k p_k) / A_{m+1}, the potential of what lies behind voxel m given that the ray got there,
//   R_{D-1} = e^eps psi_D,   R_{m-1} = R_m + y_m (E_m psi_m - R_m),   cost = R_{-1}            (E_0 = e^eps, else 1)
//   d cost / d y_m = A_m (E_m psi_m - R_m)
// which is k_drc_bwd's formula (E_m psi_m A_m - suffix_m / (1 - y_m)) with the division taken out: suffix_m / (1 - y_m) =
// R_m A_m.  One pass down the ray leaves q_m = E_m psi_m - R_m and the cost, one pass up multiplies by the prefix products
// and the gradient arriving at the ray, with the adjoint D pass RB voxels behind it.  A voxel keeps two registers: its
// clamped occupancy y (negated where a clamp acted: no gradient) and q.
// ------------------------------------------------------------------------------------------------------
template <class Pot, int DD, int RB>
__device__ __forceinline__ void ray_column_bwd(const DpcParams& P, const RayHost& rh, double e_eps,
                                               const float* __restrict__ grid_wh, const float* __restrict__ s,
                                               const TapsT<RB>& taps_arg, const TapsT<RB>& taps_adj_arg, const Pot& pot,
                                               float* __restrict__ dgrid, float* __restrict__ ds_part,
                                               unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  const TapsT<RB> taps = resolve_taps<RB>(taps_arg, P.dev_taps_z, P.taps_z, false);
  const TapsT<RB> taps_adj = resolve_taps<RB>(taps_adj_arg, P.dev_taps_z, P.taps_z, true);
  const int HW = P.H * P.W;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float ds_acc = 0.f;
  if (ray < HW) {
    // everything the ray needs besides its column, read before the column is loaded
    const int yrow = ray / P.W, xcol = ray - yrow * P.W;
    const typename Pot::Bwd r = pot.bwd_read(P, b, P.H - 1 - yrow, xcol);
    float y[DD], q[DD];
    {
      float c[DD];
      const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grid_wh + (size_t)b * DD * HW), 0, DD * HW * 4, 0x00020000);
#pragma unroll
      for (int z = 0; z < DD; ++z) c[z] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, ray * 4, z * HW * 4, 0));  // one lane offset, plane offsets in SGPRs
#pragma unroll
      for (int z = 0; z < DD; ++z) {
        float v2 = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * RB + 1; ++k) {
          const int zz = z + k - RB;
          if (zz >= 0 && zz < DD) v2 = fmaf(taps.w[k], c[zz], v2);
        }
        // y = med3(s v2, eps, 1-eps) [= clamp(clamp(s v2, 0, 1), eps, 1-eps)]; the clamps let the gradient through <=> y == s v2
        const float x = v2 * rc.s;   // s = 1 when there is no scale input
        const float yc = __builtin_amdgcn_fmed3f(x, rc.eps, rc.hi);
        y[z] = (yc == x) ? yc : -yc;
        if ((z & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
    double R = pot.bwd_start(r, P, e_eps);
#pragma unroll
    for (int m = DD - 1; m >= 0; --m) {
      const double qd = pot.bwd_term(r, P, m, DD, e_eps) - R;
      q[m] = (float)qd;
      R = fma((double)fabsf(y[m]), qd, R);
      if ((m & 3) == 0) __builtin_amdgcn_sched_barrier(0);
    }
    const float gd = pot.bwd_grad(r, P, R);
    const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(dgrid + (size_t)b * DD * HW, 0, DD * HW * 4, 0x00020000);
    double A = 1.0;
    float dsum = 0.f;
#pragma unroll
    for (int z = 0; z < DD + RB; ++z) {
      if (z < DD) {
        float yv = y[z];
        asm("" : "+v"(yv));   // opaque: or the pass above's (double)|y| is kept alive for this one, two more registers per voxel
        const float ya = fabsf(yv);
        const float e = yv > 0.f ? gd * (float)A * q[z] : 0.f;
        dsum = fmaf(ya, e, dsum);
        q[z] = e;   // q[z] carries dL/dv3 for the adjoint window from here on
        A *= 1.0 - (double)ya;
      }
      if (z >= RB) {
        const int zo = z - RB;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 2 * RB + 1; ++i) {
          const int k = tap_edge_first<RB>(i), zz = zo + k - RB;   // adjoint D pass: edges first, centre last (dpc_common.h)
          if (zz >= 0 && zz < DD) acc = fmaf(taps_adj.w[k], q[zz], acc);
        }
        acc *= rc.s;   // d grid_wh = s * adj(dL/dv3); s = 1 when there is no scale input
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, acc), dst, ray * 4, zo * HW * 4, kAuxThrough);
      }
      if ((z & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    ds_acc = (rc.has_s && rc.s != 0.f) ? dsum / rc.s : 0.f;   // inside the clamps v2 = y / s
  }
  if (ds != nullptr) depth_ds_publish(ds_acc, bk, ds_part, ds_count, ds);   // block-uniform
}

// Generic depth / tap count: the column is re-read from global, q and dL/dv3 are parked in a grid-sized scratch `dv`
// (every lane reads back only what it wrote itself).
template <class Pot>
__device__ __forceinline__ void ray_column_bwd_dyn(const DpcParams& P, const RayHost& rh, double e_eps,
                                                   const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                   const TapsDyn& taps, const Pot& pot, float* __restrict__ dgrid, float* dv_grid,
                                                   float* __restrict__ ds_part, unsigned int* __restrict__ ds_count,
                                                   float* __restrict__ ds) {   // the adjoint is `taps` read backwards
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float ds_acc = 0.f;
  if (ray < HW) {
    const int yrow = ray / P.W, xcol = ray - yrow * P.W;
    const typename Pot::Bwd r = pot.bwd_read(P, b, P.H - 1 - yrow, xcol);
    const float* col = grid_wh + (size_t)b * D * HW + ray;
    float* dv = dv_grid + (size_t)b * D * HW + ray;
    float* out = dgrid + (size_t)b * D * HW + ray;
    const int Rt = taps.n > 0 ? (taps.n - 1) / 2 : 0;
    auto x_at = [&](int z) -> float {  // forward D pass at depth z, scaled
      if (taps.n == 0) return col[(size_t)z * HW] * rc.s;
      float v2 = 0.f;
      for (int k = 0; k < taps.n; ++k) {
        const int zz = z + k - Rt;
        if (zz >= 0 && zz < D) v2 = fmaf(dyn_tap(taps, P.dev_taps_z, k), col[(size_t)zz * HW], v2);
      }
      return v2 * rc.s;
    };
    double R = pot.bwd_start(r, P, e_eps);
    for (int m = D - 1; m >= 0; --m) {
      const float x = x_at(m), yc = __builtin_amdgcn_fmed3f(x, rc.eps, rc.hi);
      const double qd = pot.bwd_term(r, P, m, D, e_eps) - R;
      dv[(size_t)m * HW] = (yc == x) ? (float)qd : 0.f;
      R = fma((double)yc, qd, R);
    }
    const float gd = pot.bwd_grad(r, P, R);
    double A = 1.0;
    float dsum = 0.f;
    for (int z = 0; z < D; ++z) {
      const float yc = __builtin_amdgcn_fmed3f(x_at(z), rc.eps, rc.hi);
      const float e = gd * (float)A * dv[(size_t)z * HW];
      dsum = fmaf(yc, e, dsum);
      dv[(size_t)z * HW] = e;
      A *= 1.0 - (double)yc;
    }
    for (int z = 0; z < D; ++z) {
      float acc;
      if (taps.n == 0) {
        acc = dv[(size_t)z * HW];
      } else {
        acc = 0.f;
        for (int k = 0; k < taps.n; ++k) {
          const int zz = z + k - Rt;
          if (zz >= 0 && zz < D) acc = fmaf(dyn_tap(taps, P.dev_taps_z, taps.n - 1 - k), dv[(size_t)zz * HW], acc);
        }
      }
      out[(size_t)z * HW] = rc.s * acc;
    }
    ds_acc = (rc.has_s && rc.s != 0.f) ? dsum / rc.s : 0.f;
  }
  if (ds != nullptr) depth_ds_publish(ds_acc, bk, ds_part, ds_count, ds);
}

// ground truth of the image pixel (prow, pcol): gt[s, f*prow, f*pcol], gt [S, f*H, f*W] in image orientation, S = B (TF-1's
// nearest neighbour / resize_images without align_corners samples exactly there for an integer factor)
__device__ inline float column_gt(const float* gt, int f, const DpcParams& P, int b, int prow, int pcol) {
  const size_t Wd = (size_t)f * P.W;
  return gt[((size_t)b * P.H * f + (size_t)prow * f) * Wd + (size_t)pcol * f];
}

// ------------------------------------------------------------------------------------------------------
// Host side.  Workspace of the backwards (dpc_depth_workspace_bytes, dpc_drc_workspace_bytes):
// [tickets B][ds partials B x ntile][dv grid, generic kernel].  The tickets come first: they are the part the caller hands
// over zeroed (the first 4 B bytes, dpc_render.h).
// ------------------------------------------------------------------------------------------------------
inline bool column_depth(const DpcParams* p) { return p->D == 32 || p->D == 64 || p->D == 128; }
// the generic backward may be needed: another depth, or a z kernel that can be longer than the largest compiled window
inline bool may_need_dv(const DpcParams* p) { return !column_depth(p) || p->taps_z > 2 * 15 + 1; }
inline size_t ws_ds_bytes(const DpcParams* p) { return ws_round((size_t)p->B * col_tiles(p) * sizeof(float)); }
inline size_t ws_count_bytes(const DpcParams* p) { return ws_round((size_t)p->B * sizeof(unsigned int)); }

inline size_t column_workspace_bytes(const DpcParams* p) {
  if (validate(p) != DPC_OK) return 0;
  return ws_ds_bytes(p) + ws_count_bytes(p) + (may_need_dv(p) ? ws_grid_bytes(p) : 0);
}

struct ColumnWorkspace {
  unsigned int* ds_count;
  float* ds_part;
  float* dv;
};
inline ColumnWorkspace column_workspace(const DpcParams* p, void* workspace) {
  char* base = static_cast<char*>(workspace);
  return ColumnWorkspace{reinterpret_cast<unsigned int*>(base), reinterpret_cast<float*>(base + ws_count_bytes(p)),
                         reinterpret_cast<float*>(base + ws_ds_bytes(p) + ws_count_bytes(p))};
}

struct ColumnCall {
  TapPlan pz;
  RayHost rh;
  double e_eps;
  float inv_S;
};

// argument checks shared by the entry points; DPC_OK with p->B == 0 means "nothing to launch"
inline int column_check(const DpcParams* p, const float* grid_wh, const float* host_kern_z, const float* gt, bool need_gt,
                        int gt_factor, ColumnCall& call) {
  const int rc = validate(p);
  if (rc != DPC_OK) return rc;
  if (gt_factor < 1 || (long long)gt_factor * p->H > 1024 || (long long)gt_factor * p->W > 1024) return DPC_ERR_SHAPE;
  if (p->B == 0) return DPC_OK;
  if (!grid_wh || (need_gt && !gt) || (p->taps_z > 0 && !host_kern_z)) return DPC_ERR_NULL;
  call.pz = plan_taps(host_kern_z, p->taps_z);
  call.rh = ray_host(p);
  call.e_eps = exp((double)p->clip_val);
  call.inv_S = 1.0f / (float)p->B;
  return DPC_OK;
}

// The compiled instantiations: D in {32, 64, 128} x the tap buckets of plan_taps.  launch(D, RB), both as integral constants,
// is called for the one that serves the call and `done` set; not done: another depth or a longer z kernel, the generic
// kernel's case.  DPC_ERR_TAPS for a bucket nobody compiled.
template <int RB, class Launch>
bool column_depths(int D, Launch& launch) {
  const std::integral_constant<int, RB> rb;
  if (D == 32) launch(std::integral_constant<int, 32>{}, rb);
  else if (D == 64) launch(std::integral_constant<int, 64>{}, rb);
  else if (D == 128) launch(std::integral_constant<int, 128>{}, rb);
  else return false;
  return true;
}
template <class Launch>
int column_dispatch(const DpcParams* p, const TapPlan& pz, bool& done, Launch launch) {
  int rc = DPC_OK;
  done = false;
#define DPC_COLUMN_RB(RB) done = column_depths<RB>(p->D, launch);
  if (pz.bucket >= 0) { DPC_FOR_BUCKET(pz.bucket, DPC_COLUMN_RB) }
#undef DPC_COLUMN_RB
  return rc;
}

}  // namespace dpck
