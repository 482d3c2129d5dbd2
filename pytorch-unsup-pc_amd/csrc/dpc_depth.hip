// Expected-depth column kernels: one lane per (y, x) ray, the z column in registers.  D pass + occupancy scale/clamp + the DRC
// recurrence + expected depth sum_k p_k psi_k and its squared-error loss against a ground-truth depth map (k_depth_fwd), the
// loss's one-block finalize (k_depth_loss_finalize) and the hand-written backward down to grid_wh and the occupancy scale
// (k_depth_bwd).  Reference: add_proj_depth_loss (dpc/util/losses.py:113-136) on drc_depth_projection (dpc/util/drc.py:145-160).
// Design notes: DESIGN.md section 4.
#include "dpc_kernels.h"

namespace dpck {
namespace {

// psi_k = k/D - 1/2 + camera_distance, psi_D = max_depth (dpc/util/drc.py:145-149; the formula of dpc_stages.hip), split into
// the part all voxels share and k/D, a compile-time constant of the unrolled kernels: the sums below carry k/D alone and the
// shared part is added once per ray (sum_{k<D} p_k psi_k = sum p_k k/D + psi_base sum p_k) -- one register for the whole
// column instead of a double per voxel.
__device__ inline double psi_base(const DpcParams& P) { return (double)P.camera_distance - 0.5; }

// The loss's ground truth and weights (uniform per launch).  gt [S, f*H, f*W] depth maps in image orientation, S = B.
struct DepthLoss {
  const float* gt;        // nullptr: projection only
  int f;                  // gt is f times the depth map's size; pixel (y, x) reads gt[f*y, f*x] (TF-1 nearest neighbour)
  float max_dataset_depth;  // the dataset's background value, replaced by P.max_depth where the two differ
  const float* weights;   // [S] | nullptr = 1
  float inv_S;
};

__device__ inline float depth_gt(const DepthLoss& dl, const DpcParams& P, int b, int prow, int pcol) {
  const size_t Wd = (size_t)dl.f * P.W;
  const float g = dl.gt[((size_t)b * P.H * dl.f + (size_t)prow * dl.f) * Wd + (size_t)pcol * dl.f];
  return (g == dl.max_dataset_depth && dl.max_dataset_depth != P.max_depth) ? P.max_depth : g;
}

// Epilogue of the forward kernels: the depth at the row-flipped pixel, this tile's squared error.
__device__ inline void depth_fwd_epilogue(const DpcParams& P, const Blk& bk, int ray, bool live, double d, float g,
                                          const DepthLoss& dl, float* __restrict__ depth, float* __restrict__ loss_tiles) {
  float sq = 0.f;
  if (live) {
    const int yrow = ray / P.W, x = ray - yrow * P.W;
    const float df = (float)d;
    if (depth != nullptr) depth[(size_t)bk.y * P.H * P.W + (P.H - 1 - yrow) * P.W + x] = df;
    const float diff = g - df;
    sq = diff * diff;
  }
  if (dl.gt != nullptr) {  // block-uniform
    const float tot = tile_sum(sq);
    if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
  }
}

// ------------------------------------------------------------------------------------------------------
// Forward: D pass + scale/clamp + DRC recurrence + expected depth.                 grid (ceil(HW/256), B)
//   p_0 = e^eps y_0, p_k = y_k A_k, p_D = e^eps A_D, A_k = prod_{j<k} (1 - y_j)   (k_drc_fwd, dpc_stages.hip)
// ------------------------------------------------------------------------------------------------------
template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 64 ? 4 : 2)) void k_depth_fwd(DpcParams P, RayHost rh, double e_eps,
                                                                             const float* __restrict__ grid_wh,
                                                                             const float* __restrict__ s, TapsT<RB> taps_arg,
                                                                             DepthLoss dl, float* __restrict__ depth,
                                                                             float* __restrict__ loss_tiles) {
  const TapsT<RB> taps = resolve_taps<RB>(taps_arg, P.dev_taps_z, P.taps_z, false);
  const int HW = P.H * P.W;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const bool live = ray < HW;
  const RayConst rc = ray_const(rh, s, b);
  double d = 0.0;
  float g = 0.f;
  if (live) {
    if (dl.gt != nullptr) g = depth_gt(dl, P, b, P.H - 1 - ray / P.W, ray % P.W);   // before the column is loaded
    float c[DD];
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grid_wh + (size_t)b * DD * HW), 0, DD * HW * 4, 0x00020000);
#pragma unroll
    for (int z = 0; z < DD; ++z) c[z] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, ray * 4, z * HW * 4, 0));  // one lane offset, plane offsets in SGPRs
    double A = 1.0, dsum = 0.0, psum = 0.0;
#pragma unroll
    for (int z = 0; z < DD; ++z) {
      float v2 = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * RB + 1; ++k) {
        const int zz = z + k - RB;
        if (zz >= 0 && zz < DD) v2 = fmaf(taps.w[k], c[zz], v2);
      }
      const double y = (double)drc_clamp(rc, occupancy(rc, v2));
      const double pk = (z == 0 ? e_eps * y : y) * A;
      psum += pk;
      dsum = fma(pk, (double)z / (double)DD, dsum);
      A *= 1.0 - y;
      if ((z & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    d = fma(psi_base(P), psum, dsum) + e_eps * A * (double)P.max_depth;
  }
  depth_fwd_epilogue(P, bk, ray, live, d, g, dl, depth, loss_tiles);
}

// Generic depth / tap count: same arithmetic, column re-read from global (L1/L2 serve the re-reads).
__global__ __launch_bounds__(kColThreads) void k_depth_fwd_dyn(DpcParams P, RayHost rh, double e_eps,
                                                               const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                               TapsDyn taps_arg, DepthLoss dl, float* __restrict__ depth,
                                                               float* __restrict__ loss_tiles) {
  const TapsDyn& taps = taps_arg;
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const bool live = ray < HW;
  const RayConst rc = ray_const(rh, s, b);
  double d = 0.0;
  float g = 0.f;
  if (live) {
    if (dl.gt != nullptr) g = depth_gt(dl, P, b, P.H - 1 - ray / P.W, ray % P.W);
    const float* col = grid_wh + (size_t)b * D * HW + ray;
    const int R = taps.n > 0 ? (taps.n - 1) / 2 : 0;
    double A = 1.0, dsum = 0.0, psum = 0.0;
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
      const double pk = (z == 0 ? e_eps * y : y) * A;
      psum += pk;
      dsum = fma(pk, (double)z / (double)D, dsum);
      A *= 1.0 - y;
    }
    d = fma(psi_base(P), psum, dsum) + e_eps * A * (double)P.max_depth;
  }
  depth_fwd_epilogue(P, bk, ray, live, d, g, dl, depth, loss_tiles);
}

// loss = (1/2) sum_s w_s^2 (sum of the sample's tiles, in tile order) / S.  One block; the same bits on every run.
__global__ __launch_bounds__(256) void k_depth_loss_finalize(const float* __restrict__ loss_tiles, int ntile, int S, float half_inv_S,
                                                             const float* __restrict__ weights, float* __restrict__ loss) {
  __shared__ float red[256 / DPC_WAVE];
  float acc = 0.f;
  for (int smp = threadIdx.x; smp < S; smp += blockDim.x) {
    float v = 0.f;
    for (int i = 0; i < ntile; ++i) v += loss_tiles[(size_t)smp * ntile + i];
    acc += v * ::sample_weight2(weights, smp);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < 256 / DPC_WAVE; ++i) tot += red[i];
    *loss = tot * half_inv_S;
  }
}

// ------------------------------------------------------------------------------------------------------
// Backward: d depth -> DRC adjoint (depth term) -> clamp masks -> adjoint D pass.  grid (ceil(HW/256), B)
//
// With R_m = (sum_{k>m} psi_k p_k) / A_{m+1}, the expected depth of what lies behind voxel m given that the ray got there,
//   R_{D-1} = e^eps psi_D,   R_{m-1} = R_m + y_m (E_m psi_m - R_m),   depth = R_{-1}            (E_0 = e^eps, else 1)
//   d depth / d y_m = A_m (E_m psi_m - R_m)
// which is k_drc_bwd's formula (E_m psi_m A_m - suffix_m / (1 - y_m)) with the division taken out: suffix_m / (1 - y_m) =
// R_m A_m.  One pass down the ray leaves q_m = E_m psi_m - R_m and the depth, one pass up multiplies by the prefix products
// and the gradient arriving at the depth, with the adjoint D pass RB voxels behind it.  A voxel keeps two registers: its
// clamped occupancy y (negated where a clamp acted: no gradient) and q.
// ------------------------------------------------------------------------------------------------------
// gradient arriving at this ray's depth: from the loss, (1/2) w^2 (g - depth)^2 / S times dloss, plus the caller's own
__device__ inline float depth_grad(const DepthLoss& dl, float w2, float up, float g, float gin, float d) {
  return dl.gt != nullptr ? fmaf(up * w2 * dl.inv_S, d - g, gin) : gin;
}

template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 32 ? 4 : (DD <= 64 ? 2 : 1)))
void k_depth_bwd(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh, const float* __restrict__ s,
                 TapsT<RB> taps_arg, TapsT<RB> taps_adj_arg, DepthLoss dl, const float* __restrict__ dloss,
                 const float* __restrict__ ddepth, float* __restrict__ dgrid, float* __restrict__ ds_part,
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
    const int yrow = ray / P.W, xcol = ray - yrow * P.W, prow = P.H - 1 - yrow;
    const float g = dl.gt != nullptr ? depth_gt(dl, P, b, prow, xcol) : 0.f;
    const float w2 = ::sample_weight2(dl.weights, b);
    const float up = dloss != nullptr ? *dloss : 1.0f;
    const float gin = ddepth != nullptr ? ddepth[(size_t)b * HW + prow * P.W + xcol] : 0.f;
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
    // R is carried as R - psi_base: then E_m psi_m - R_m = m/D - R_m for m > 0 (a compile-time constant minus the carry)
    const double base = psi_base(P);
    double R = e_eps * (double)P.max_depth - base;
#pragma unroll
    for (int m = DD - 1; m >= 0; --m) {
      const double qd = (m == 0 ? (e_eps - 1.0) * base : (double)m / (double)DD) - R;
      q[m] = (float)qd;
      R = fma((double)fabsf(y[m]), qd, R);
      if ((m & 3) == 0) __builtin_amdgcn_sched_barrier(0);
    }
    const float gd = depth_grad(dl, w2, up, g, gin, (float)(R + base));
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
__global__ __launch_bounds__(kColThreads) void k_depth_bwd_dyn(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh,
                                                               const float* __restrict__ s, TapsDyn taps_arg,
                                                               DepthLoss dl, const float* __restrict__ dloss,
                                                               const float* __restrict__ ddepth, float* __restrict__ dgrid,
                                                               float* dv_grid, float* __restrict__ ds_part,
                                                               unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  const TapsDyn& taps = taps_arg;   // the adjoint is the same table read backwards
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float ds_acc = 0.f;
  if (ray < HW) {
    const int yrow = ray / P.W, xcol = ray - yrow * P.W, prow = P.H - 1 - yrow;
    const float g = dl.gt != nullptr ? depth_gt(dl, P, b, prow, xcol) : 0.f;
    const float w2 = ::sample_weight2(dl.weights, b);
    const float up = dloss != nullptr ? *dloss : 1.0f;
    const float gin = ddepth != nullptr ? ddepth[(size_t)b * HW + prow * P.W + xcol] : 0.f;
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
    const double base = psi_base(P);
    double R = e_eps * (double)P.max_depth - base;   // carried as R - psi_base, as in k_depth_bwd
    for (int m = D - 1; m >= 0; --m) {
      const float x = x_at(m), yc = __builtin_amdgcn_fmed3f(x, rc.eps, rc.hi);
      const double qd = (m == 0 ? (e_eps - 1.0) * base : (double)m / (double)D) - R;
      dv[(size_t)m * HW] = (yc == x) ? (float)qd : 0.f;
      R = fma((double)yc, qd, R);
    }
    const float gd = depth_grad(dl, w2, up, g, gin, (float)(R + base));
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

// ------------------------------------------------------------------------------------------------------
// Host side.  Workspace of the backward (dpc_depth_workspace_bytes): [tickets B][ds partials B x ntile][dv grid, generic kernel]
// The tickets come first: they are the part the caller hands over zeroed (the first 4 B bytes, dpc_render.h).
// ------------------------------------------------------------------------------------------------------
struct DepthCall {
  TapPlan pz;
  DepthLoss dl;
  RayHost rh;
  double e_eps;
};

// argument checks shared by the two entry points; DPC_OK with p->B == 0 means "nothing to launch"
int depth_check(const DpcParams* p, const float* grid_wh, const float* host_kern_z, const float* gt, int gt_factor,
                float max_dataset_depth, const float* weights, DepthCall& call) {
  const int rc = validate(p);
  if (rc != DPC_OK) return rc;
  if (gt_factor < 1 || (long long)gt_factor * p->H > 1024 || (long long)gt_factor * p->W > 1024) return DPC_ERR_SHAPE;
  if (p->B == 0) return DPC_OK;
  if (!grid_wh || (p->taps_z > 0 && !host_kern_z)) return DPC_ERR_NULL;
  call.pz = plan_taps(host_kern_z, p->taps_z);
  call.dl = DepthLoss{gt, gt_factor, max_dataset_depth, weights, 1.0f / (float)p->B};
  call.rh = ray_host(p);
  call.e_eps = exp((double)p->clip_val);
  return DPC_OK;
}

}  // namespace
}  // namespace dpck

using namespace dpck;

extern "C" {

size_t dpc_depth_workspace_bytes(const DpcParams* p) {
  if (validate(p) != DPC_OK) return 0;
  return ws_ds_bytes(p) + ws_count_bytes(p) + (may_need_dv(p) ? ws_grid_bytes(p) : 0);
}

int dpc_depth_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_depth,
                       int gt_factor, float max_dataset_depth, const float* weights, float* depth, float* loss_tiles, float* loss,
                       void* stream) {
  if (p && ((gt_depth && (!loss || !loss_tiles)) || (!gt_depth && !depth))) return DPC_ERR_SHAPE;  // a loss nobody can receive / nothing asked for
  DepthCall c;
  int rc = depth_check(p, grid_wh, host_kern_z, gt_depth, gt_factor, max_dataset_depth, weights, c);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  const dim3 gcol(col_tiles(p) * p->B);
  bool done = false;
#define DPC_DFWD(RB)                                                                                               \
  {                                                                                                                \
    const TapsT<RB> tz = make_taps<RB>(host_kern_z, c.pz, false);                                                  \
    if (p->D == 32) { DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd", 32, RB), (k_depth_fwd<32, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.dl, depth, loss_tiles); done = true; } \
    else if (p->D == 64) { DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd", 64, RB), (k_depth_fwd<64, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.dl, depth, loss_tiles); done = true; } \
    else if (p->D == 128) { DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd", 128, RB), (k_depth_fwd<128, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.dl, depth, loss_tiles); done = true; } \
  }
  if (c.pz.bucket >= 0) { DPC_FOR_BUCKET(c.pz.bucket, DPC_DFWD) }
#undef DPC_DFWD
  if (rc != DPC_OK) return rc;
  if (!done)  // other depths / longer kernels: same arithmetic, column re-read from global
    DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd_dyn"), k_depth_fwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s,
               make_taps_dyn(host_kern_z, p->taps_z, false), c.dl, depth, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  if (!gt_depth) return DPC_OK;
  DPC_LAUNCH("k_depth_loss_finalize", dpc_kid("k_depth_loss_finalize"), k_depth_loss_finalize, dim3(1), dim3(256), 0, st, loss_tiles,
             col_tiles(p), p->B, 0.5f * c.dl.inv_S, weights, loss);
  return launch_ok();
}

int dpc_depth_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_depth,
                       int gt_factor, float max_dataset_depth, const float* weights, const float* dloss, const float* ddepth,
                       float* dgrid_wh, float* ds, void* workspace, void* stream) {
  if (p && !gt_depth && !ddepth) return DPC_ERR_SHAPE;   // no gradient arrives anywhere
  DepthCall c;
  int rc = depth_check(p, grid_wh, host_kern_z, gt_depth, gt_factor, max_dataset_depth, weights, c);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dgrid_wh || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(workspace);
  unsigned int* ds_count = reinterpret_cast<unsigned int*>(base);
  float* ds_part = reinterpret_cast<float*>(base + ws_count_bytes(p));
  float* dv = reinterpret_cast<float*>(base + ws_ds_bytes(p) + ws_count_bytes(p));
  const dim3 gcol(col_tiles(p) * p->B);
  bool done = false;
#define DPC_DBWD(RB)                                                                                               \
  {                                                                                                                \
    const TapsT<RB> tzf = make_taps<RB>(host_kern_z, c.pz, false), tza = make_taps<RB>(host_kern_z, c.pz, true);   \
    if (p->D == 32) { DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd", 32, RB), (k_depth_bwd<32, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.dl, dloss, ddepth, dgrid_wh, ds_part, ds_count, ds); done = true; } \
    else if (p->D == 64) { DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd", 64, RB), (k_depth_bwd<64, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.dl, dloss, ddepth, dgrid_wh, ds_part, ds_count, ds); done = true; } \
    else if (p->D == 128) { DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd", 128, RB), (k_depth_bwd<128, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.dl, dloss, ddepth, dgrid_wh, ds_part, ds_count, ds); done = true; } \
  }
  if (c.pz.bucket >= 0) { DPC_FOR_BUCKET(c.pz.bucket, DPC_DBWD) }
#undef DPC_DBWD
  if (rc != DPC_OK) return rc;
  if (!done) {
    if (!may_need_dv(p)) return DPC_ERR_TAPS;   // cannot happen: a kernel of <= 31 taps has a compiled window
    DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd_dyn"), k_depth_bwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s,
               make_taps_dyn(host_kern_z, p->taps_z, false), c.dl, dloss, ddepth, dgrid_wh, dv, ds_part, ds_count, ds);
  }
  return launch_ok();
}

}  // extern "C"
