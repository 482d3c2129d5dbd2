// Ray-consistency (DRC) losses as ray potentials sum_k p_k psi_k over the ray-termination probabilities, fused with their
// hand-written backwards: the mask loss on grid_wh (k_drcmask_fwd / k_drcmask_bwd, the structure of k_depth_* in
// dpc_depth.hip: one lane per (y, x) ray, the z column in registers) and the colour loss on the renderer's voxels and colour
// grid (k_drcrgb_fwd / k_drcrgb_bwd, the inputs and options of k_rgb_* in dpc_rgb.hip), and their one-block finalize.
// Reference (TF-1 originals): drc_loss, drc_rgb_loss, add_drc_loss, add_drc_rgb_loss (dpc/util/losses.py:23-66, 93-110) on
// drc_event_probabilities (dpc/util/drc.py:48-106) and the flip of pointcloud_project_fast (dpc/util/point_cloud.py:269-276).
// Design notes: DESIGN.md section 4.  The tile sum, the ds hand-off, the tap lookup, the images' reads and the colour value are
// those of dpc_depth.hip and dpc_rgb.hip (dpc_kernels.h).
#include "dpc_kernels.h"

namespace dpck {
namespace {

// loss = sum_s w_s^2 (sum of the sample's tiles, in tile order) / S: no 1/2 (losses.py:29, 46, 62, 106).  One block; the same
// bits on every run.
__global__ __launch_bounds__(256) void k_drc_loss_finalize(const float* __restrict__ loss_tiles, int ntile, int S, float inv_S,
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
    *loss = tot * inv_S;
  }
}

// ------------------------------------------------------------------------------------------------------
// Mask loss.  Ray cost (1 - g) sum_{k<D} p_k + g p_D with g the mask at the ray's pixel (drc_loss, losses.py:23-29: psi is
// 1 - g for the D voxels and g for the background).  sum_{k<D} p_k is summed, not taken as 1 - p_D: with the e^eps factors
// the probabilities do not add up to one.
// ------------------------------------------------------------------------------------------------------
struct MaskLoss {
  const float* gt;        // [S, f*H, f*W] masks in image orientation, S = B
  int f;                  // pixel (y, x) reads gt[f*y, f*x] (TF-1 resize_images without align_corners, integer factor)
  const float* weights;   // [S] | nullptr = 1
  float inv_S;
};

__device__ inline float mask_gt(const MaskLoss& ml, const DpcParams& P, int b, int prow, int pcol) {
  const size_t Wd = (size_t)ml.f * P.W;
  return ml.gt[((size_t)b * P.H * ml.f + (size_t)prow * ml.f) * Wd + (size_t)pcol * ml.f];
}

__device__ inline void mask_fwd_epilogue(const Blk& bk, float cost, float* __restrict__ loss_tiles) {
  const float tot = tile_sum(cost);
  if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
}

// Forward: D pass + scale/clamp + DRC recurrence + ray cost.                        grid (ceil(HW/256) * B)
//   p_0 = e^eps y_0, p_k = y_k A_k, p_D = e^eps A_D, A_k = prod_{j<k} (1 - y_j)   (k_drc_fwd, dpc_stages.hip)
template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 64 ? 4 : 2)) void k_drcmask_fwd(DpcParams P, RayHost rh, double e_eps,
                                                                               const float* __restrict__ grid_wh,
                                                                               const float* __restrict__ s, TapsT<RB> taps_arg,
                                                                               MaskLoss ml, float* __restrict__ loss_tiles) {
  const TapsT<RB> taps = resolve_taps<RB>(taps_arg, P.dev_taps_z, P.taps_z, false);
  const int HW = P.H * P.W;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float cost = 0.f;
  if (ray < HW) {
    const double g = (double)mask_gt(ml, P, b, P.H - 1 - ray / P.W, ray % P.W);   // before the column is loaded
    float c[DD];
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grid_wh + (size_t)b * DD * HW), 0, DD * HW * 4, 0x00020000);
#pragma unroll
    for (int z = 0; z < DD; ++z) c[z] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, ray * 4, z * HW * 4, 0));  // one lane offset, plane offsets in SGPRs
    double A = 1.0, psum = 0.0;
#pragma unroll
    for (int z = 0; z < DD; ++z) {
      float v2 = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * RB + 1; ++k) {
        const int zz = z + k - RB;
        if (zz >= 0 && zz < DD) v2 = fmaf(taps.w[k], c[zz], v2);
      }
      const double y = (double)drc_clamp(rc, occupancy(rc, v2));
      psum = fma(z == 0 ? e_eps * y : y, A, psum);
      A *= 1.0 - y;
      if ((z & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    cost = (float)fma(1.0 - g, psum, g * e_eps * A);
  }
  mask_fwd_epilogue(bk, cost, loss_tiles);
}

// Generic depth / tap count: same arithmetic, column re-read from global (L1/L2 serve the re-reads).
__global__ __launch_bounds__(kColThreads) void k_drcmask_fwd_dyn(DpcParams P, RayHost rh, double e_eps,
                                                                 const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                                 TapsDyn taps_arg, MaskLoss ml, float* __restrict__ loss_tiles) {
  const TapsDyn& taps = taps_arg;
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float cost = 0.f;
  if (ray < HW) {
    const double g = (double)mask_gt(ml, P, b, P.H - 1 - ray / P.W, ray % P.W);
    const float* col = grid_wh + (size_t)b * D * HW + ray;
    const int R = taps.n > 0 ? (taps.n - 1) / 2 : 0;
    double A = 1.0, psum = 0.0;
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
      psum = fma(z == 0 ? e_eps * y : y, A, psum);
      A *= 1.0 - y;
    }
    cost = (float)fma(1.0 - g, psum, g * e_eps * A);
  }
  mask_fwd_epilogue(bk, cost, loss_tiles);
}

// Backward: d cost -> DRC adjoint -> clamp masks -> adjoint D pass.                 grid (ceil(HW/256) * B)
//
// k_depth_bwd's division-free recurrence with psi_m = 1 - g, psi_D = g.  With R_m = (sum_{k>m} psi_k p_k) / A_{m+1},
//   R_{D-1} = e^eps g,   R_{m-1} = R_m + y_m (E_m (1 - g) - R_m),   d cost / d y_m = A_m (E_m (1 - g) - R_m)     (E_0 = e^eps, else 1)
// The cost is linear in the probabilities, so the gradient arriving at a ray is dloss w_s^2 / S whatever the forward gave.
// One pass down the ray leaves q_m = E_m (1 - g) - R_m, one pass up multiplies by the prefix products, with the adjoint D
// pass RB voxels behind it.  A voxel keeps two registers: its clamped occupancy y (negated where a clamp acted) and q.
template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 32 ? 4 : (DD <= 64 ? 2 : 1)))
void k_drcmask_bwd(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh, const float* __restrict__ s,
                   TapsT<RB> taps_arg, TapsT<RB> taps_adj_arg, MaskLoss ml, const float* __restrict__ dloss,
                   float* __restrict__ dgrid, float* __restrict__ ds_part, unsigned int* __restrict__ ds_count,
                   float* __restrict__ ds) {
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
    const double fg = 1.0 - (double)mask_gt(ml, P, b, P.H - 1 - yrow, xcol);
    const float gd = (dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(ml.weights, b) * ml.inv_S;
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
    double R = e_eps * (1.0 - fg);
#pragma unroll
    for (int m = DD - 1; m >= 0; --m) {
      const double qd = (m == 0 ? e_eps * fg : fg) - R;
      q[m] = (float)qd;
      R = fma((double)fabsf(y[m]), qd, R);
      if ((m & 3) == 0) __builtin_amdgcn_sched_barrier(0);
    }
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
__global__ __launch_bounds__(kColThreads) void k_drcmask_bwd_dyn(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh,
                                                                 const float* __restrict__ s, TapsDyn taps_arg, MaskLoss ml,
                                                                 const float* __restrict__ dloss, float* __restrict__ dgrid,
                                                                 float* dv_grid, float* __restrict__ ds_part,
                                                                 unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  const TapsDyn& taps = taps_arg;   // the adjoint is the same table read backwards
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const RayConst rc = ray_const(rh, s, b);
  float ds_acc = 0.f;
  if (ray < HW) {
    const int yrow = ray / P.W, xcol = ray - yrow * P.W;
    const double fg = 1.0 - (double)mask_gt(ml, P, b, P.H - 1 - yrow, xcol);
    const float gd = (dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(ml.weights, b) * ml.inv_S;
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
    double R = e_eps * (1.0 - fg);
    for (int m = D - 1; m >= 0; --m) {
      const float x = x_at(m), yc = __builtin_amdgcn_fmed3f(x, rc.eps, rc.hi);
      const double qd = (m == 0 ? e_eps * fg : fg) - R;
      dv[(size_t)m * HW] = (yc == x) ? (float)qd : 0.f;
      R = fma((double)yc, qd, R);
    }
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
// Colour loss.  Ray cost sum_{k<D} p_k psi_k + p_D psi_D with psi_k = sum_c (g_c - C^_{c,k})^2 the squared distance of the
// voxel's colour from the pixel's and psi_D = sum_c (g_c - 1)^2 for the white background (drc_rgb_loss, losses.py:32-46).
// C^ is the colour k_rgb_fwd's integral sees: C / (div + eps) when div is given, clamped when clip_after.
// ------------------------------------------------------------------------------------------------------
__device__ inline float white_psi(const float (&g)[3]) {
  float psi = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) psi = fmaf(g[c] - 1.0f, g[c] - 1.0f, psi);
  return psi;
}

// Forward: any D, one lane per ray, one read of vox, C and div.                     grid (ceil(HW/256) * B)
__global__ __launch_bounds__(kColThreads) void k_drcrgb_fwd(DpcParams P, double e_eps, const float* __restrict__ vox,
                                                            const float* __restrict__ C, RgbArgs a, float* __restrict__ loss_tiles) {
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const float eps = P.clip_val, hi = (float)(1.0 - (double)P.clip_val);
  float cost = 0.f;
  if (ray < HW) {
    const int yrow = ray / P.W, x = ray - yrow * P.W;
    float g[3];
    rgb_gt(a, P, b, P.H - 1 - yrow, x, g);
    const size_t plane = (size_t)D * HW;
    const float* col = vox + (size_t)b * plane + ray;
    const float* ccol = C + (size_t)b * 3 * plane + ray;
    const float* dcol = a.div != nullptr ? a.div + (size_t)b * plane + ray : nullptr;
    double A = 1.0, acc = 0.0;
    for (int k = 0; k < D; ++k) {
      const size_t at = (size_t)k * HW;
      const float y = fminf(fmaxf(col[at], eps), hi);
      const double pk = (k == 0 ? e_eps : 1.0) * (double)y * A;
      const float dv = dcol != nullptr ? dcol[at] : 0.f;
      float psi = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float scale;
        const float d = g[c] - rgb_value(a, ccol[c * plane + at], dv, scale);
        psi = fmaf(d, d, psi);
      }
      acc = fma(pk, (double)psi, acc);
      A *= 1.0 - (double)y;
    }
    cost = (float)fma(e_eps * A, (double)white_psi(g), acc);
  }
  const float tot = tile_sum(cost);
  if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
}

// Backward.  With r = dloss w_s^2 / S:
//   dC^_{c,k} = 2 r p_k (C^_{c,k} - g_c), times rgb_value's scale;
//   dL/dy_m   = r (psi_m E_m A_m - (sum_{k>m} psi_k p_k) / (1 - y_m)), zero where the clamp acted   (k_drc_bwd's formula).
// Pass 1 runs over vox alone and leaves y (negated where the clamp acted) and the prefix products A_m in registers; pass 2
// walks down the ray with the suffix sum, reads C and div once and writes dC and dvox once: the bytes moved are vox + C
// (+ div) in and dvox + dC out, nothing per-voxel is parked in global memory.
template <int DD>
__global__ __launch_bounds__(kColThreads, (DD <= 32 ? 4 : 2)) void k_drcrgb_bwd(DpcParams P, double e_eps,
                                                                              const float* __restrict__ vox,
                                                                              const float* __restrict__ C, RgbArgs a,
                                                                              const float* __restrict__ dloss,
                                                                              float* __restrict__ dvox, float* __restrict__ dC) {
  const int HW = P.H * P.W;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const float eps = P.clip_val, hi = (float)(1.0 - (double)P.clip_val);
  if (ray >= HW) return;
  const int yrow = ray / P.W, x = ray - yrow * P.W;
  float g[3];
  rgb_gt(a, P, b, P.H - 1 - yrow, x, g);
  const double r = (double)((dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(a.weights, b) * a.inv_S);
  float y[DD], Af[DD];
  const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(vox + (size_t)b * DD * HW), 0, DD * HW * 4, 0x00020000);
#pragma unroll
  for (int z = 0; z < DD; ++z) y[z] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, ray * 4, z * HW * 4, 0));
  double A = 1.0;
#pragma unroll
  for (int z = 0; z < DD; ++z) {
    const float v = y[z], yc = __builtin_amdgcn_fmed3f(v, eps, hi);
    float af = (float)A, ys = (yc == v) ? yc : -yc;
    asm("" : "+v"(af), "+v"(ys));   // opaque: or pass 2 is fed from v, yc and the fp64 product, four registers per voxel and spills
    Af[z] = af;
    y[z] = ys;
    A *= 1.0 - (double)yc;
  }
  const size_t plane = (size_t)DD * HW;
  const float* ccol = C + (size_t)b * 3 * plane + ray;
  const float* dcol = a.div != nullptr ? a.div + (size_t)b * plane + ray : nullptr;
  float* gv = dvox + (size_t)b * plane + ray;
  float* gc = dC + (size_t)b * 3 * plane + ray;
  double suffix = (double)white_psi(g) * e_eps * A;   // sum_{k>m} psi_k p_k, starting from the background
#pragma unroll
  for (int m = DD - 1; m >= 0; --m) {
    const size_t at = (size_t)m * HW;
    const float yv = y[m], ya = fabsf(yv);
    const double EA = (m == 0 ? e_eps : 1.0) * (double)Af[m];
    const double pm = EA * (double)ya;
    const float dv = dcol != nullptr ? dcol[at] : 0.f;
    const float k2 = (float)(2.0 * r * pm);
    float psi = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float scale;
      const float d = rgb_value(a, ccol[c * plane + at], dv, scale) - g[c];
      psi = fmaf(d, d, psi);
      gc[c * plane + at] = k2 * d * scale;
    }
    const double dy = r * ((double)psi * EA - suffix / (1.0 - (double)ya));
    gv[at] = yv > 0.f ? (float)dy : 0.f;
    suffix = fma((double)psi, pm, suffix);
    if ((m & 3) == 0) __builtin_amdgcn_sched_barrier(0);   // four voxels' loads in flight, not the whole column's: no spills
  }
}

// Generic depth: pass 1 parks the prefix products A_m in dvox (fp32), pass 2 overwrites them, as k_rgb_bwd does.
__global__ __launch_bounds__(kColThreads) void k_drcrgb_bwd_dyn(DpcParams P, double e_eps, const float* __restrict__ vox,
                                                                const float* __restrict__ C, RgbArgs a,
                                                                const float* __restrict__ dloss, float* __restrict__ dvox,
                                                                float* __restrict__ dC) {
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const float eps = P.clip_val, hi = (float)(1.0 - (double)P.clip_val);
  if (ray >= HW) return;
  const int yrow = ray / P.W, x = ray - yrow * P.W;
  float g[3];
  rgb_gt(a, P, b, P.H - 1 - yrow, x, g);
  const double r = (double)((dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(a.weights, b) * a.inv_S);
  const size_t plane = (size_t)D * HW;
  const float* col = vox + (size_t)b * plane + ray;
  const float* ccol = C + (size_t)b * 3 * plane + ray;
  const float* dcol = a.div != nullptr ? a.div + (size_t)b * plane + ray : nullptr;
  float* gv = dvox + (size_t)b * plane + ray;
  float* gc = dC + (size_t)b * 3 * plane + ray;
  double A = 1.0;
  for (int k = 0; k < D; ++k) {
    const size_t at = (size_t)k * HW;
    gv[at] = (float)A;
    A *= 1.0 - (double)fminf(fmaxf(col[at], eps), hi);
  }
  double suffix = (double)white_psi(g) * e_eps * A;
  for (int m = D - 1; m >= 0; --m) {
    const size_t at = (size_t)m * HW;
    const float v = col[at];
    const float ya = fminf(fmaxf(v, eps), hi);
    const double EA = (m == 0 ? e_eps : 1.0) * (double)gv[at];
    const double pm = EA * (double)ya;
    const float dv = dcol != nullptr ? dcol[at] : 0.f;
    const float k2 = (float)(2.0 * r * pm);
    float psi = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float scale;
      const float d = rgb_value(a, ccol[c * plane + at], dv, scale) - g[c];
      psi = fmaf(d, d, psi);
      gc[c * plane + at] = k2 * d * scale;
    }
    const double dy = r * ((double)psi * EA - suffix / (1.0 - (double)ya));
    gv[at] = (v >= eps && v <= hi) ? (float)dy : 0.f;
    suffix = fma((double)psi, pm, suffix);
  }
}

// ------------------------------------------------------------------------------------------------------
// Host side.  Workspace of the mask backward (dpc_drc_workspace_bytes): the layout of dpc_depth_workspace_bytes
// (dpc_kernels.h).  The tickets come first: the part the caller hands over zeroed.
// ------------------------------------------------------------------------------------------------------
struct MaskCall {
  TapPlan pz;
  MaskLoss ml;
  RayHost rh;
  double e_eps;
};

// argument checks shared by the two mask entry points (depth_check's); DPC_OK with p->B == 0 means "nothing to launch"
int mask_check(const DpcParams* p, const float* grid_wh, const float* host_kern_z, const float* gt, int gt_factor,
               const float* weights, MaskCall& call) {
  const int rc = validate(p);
  if (rc != DPC_OK) return rc;
  if (gt_factor < 1 || (long long)gt_factor * p->H > 1024 || (long long)gt_factor * p->W > 1024) return DPC_ERR_SHAPE;
  if (p->B == 0) return DPC_OK;
  if (!grid_wh || !gt || (p->taps_z > 0 && !host_kern_z)) return DPC_ERR_NULL;
  call.pz = plan_taps(host_kern_z, p->taps_z);
  call.ml = MaskLoss{gt, gt_factor, weights, 1.0f / (float)p->B};
  call.rh = ray_host(p);
  call.e_eps = exp((double)p->clip_val);
  return DPC_OK;
}

int finalize(const DpcParams* p, const float* loss_tiles, const float* weights, float* loss, hipStream_t st) {
  DPC_LAUNCH("k_drc_loss_finalize", dpc_kid("k_drc_loss_finalize"), k_drc_loss_finalize, dim3(1), dim3(256), 0, st, loss_tiles,
             col_tiles(p), p->B, 1.0f / (float)p->B, weights, loss);
  return launch_ok();
}

}  // namespace
}  // namespace dpck

using namespace dpck;

extern "C" {

size_t dpc_drc_workspace_bytes(const DpcParams* p) {
  if (validate(p) != DPC_OK) return 0;
  return ws_ds_bytes(p) + ws_count_bytes(p) + (may_need_dv(p) ? ws_grid_bytes(p) : 0);
}

int dpc_drc_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, float* loss_tiles, float* loss, void* stream) {
  if (p && gt_mask && (!loss || !loss_tiles)) return DPC_ERR_SHAPE;   // a loss nobody can receive
  MaskCall c;
  int rc = mask_check(p, grid_wh, host_kern_z, gt_mask, gt_factor, weights, c);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  const dim3 gcol(col_tiles(p) * p->B);
  bool done = false;
#define DPC_MFWD(RB)                                                                                               \
  {                                                                                                                \
    const TapsT<RB> tz = make_taps<RB>(host_kern_z, c.pz, false);                                                  \
    if (p->D == 32) { DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd", 32, RB), (k_drcmask_fwd<32, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.ml, loss_tiles); done = true; } \
    else if (p->D == 64) { DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd", 64, RB), (k_drcmask_fwd<64, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.ml, loss_tiles); done = true; } \
    else if (p->D == 128) { DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd", 128, RB), (k_drcmask_fwd<128, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tz, c.ml, loss_tiles); done = true; } \
  }
  if (c.pz.bucket >= 0) { DPC_FOR_BUCKET(c.pz.bucket, DPC_MFWD) }
#undef DPC_MFWD
  if (rc != DPC_OK) return rc;
  if (!done)  // other depths / longer kernels: same arithmetic, column re-read from global
    DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd_dyn"), k_drcmask_fwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps_dyn(host_kern_z, p->taps_z, false), c.ml, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  return finalize(p, loss_tiles, weights, loss, st);
}

int dpc_drc_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, const float* dloss, float* dgrid_wh, float* ds, void* workspace,
                     void* stream) {
  MaskCall c;
  int rc = mask_check(p, grid_wh, host_kern_z, gt_mask, gt_factor, weights, c);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dgrid_wh || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(workspace);
  unsigned int* ds_count = reinterpret_cast<unsigned int*>(base);
  float* ds_part = reinterpret_cast<float*>(base + ws_count_bytes(p));
  float* dv = reinterpret_cast<float*>(base + ws_ds_bytes(p) + ws_count_bytes(p));
  const dim3 gcol(col_tiles(p) * p->B);
  bool done = false;
#define DPC_MBWD(RB)                                                                                               \
  {                                                                                                                \
    const TapsT<RB> tzf = make_taps<RB>(host_kern_z, c.pz, false), tza = make_taps<RB>(host_kern_z, c.pz, true);   \
    if (p->D == 32) { DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd", 32, RB), (k_drcmask_bwd<32, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.ml, dloss, dgrid_wh, ds_part, ds_count, ds); done = true; } \
    else if (p->D == 64) { DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd", 64, RB), (k_drcmask_bwd<64, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.ml, dloss, dgrid_wh, ds_part, ds_count, ds); done = true; } \
    else if (p->D == 128) { DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd", 128, RB), (k_drcmask_bwd<128, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s, tzf, tza, c.ml, dloss, dgrid_wh, ds_part, ds_count, ds); done = true; } \
  }
  if (c.pz.bucket >= 0) { DPC_FOR_BUCKET(c.pz.bucket, DPC_MBWD) }
#undef DPC_MBWD
  if (rc != DPC_OK) return rc;
  if (!done) {
    if (!may_need_dv(p)) return DPC_ERR_TAPS;   // cannot happen: a kernel of <= 31 taps has a compiled window
    DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd_dyn"), k_drcmask_bwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps_dyn(host_kern_z, p->taps_z, false), c.ml, dloss, dgrid_wh, dv, ds_part, ds_count, ds);
  }
  return launch_ok();
}

int dpc_drc_rgb_loss_fwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, float* loss_tiles, float* loss,
                         void* stream) {
  if (p && gt && (!loss || !loss_tiles)) return DPC_ERR_SHAPE;   // a loss nobody can receive
  const int rc = rgb_check(p, gt_factor);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  if (!vox || !C || !gt) return DPC_ERR_NULL;
  const RgbArgs a{div, div_eps, clip_after != 0, gt, gt_factor, gt_planar != 0, weights, 1.0f / (float)p->B};
  DPC_LAUNCH("k_drcrgb_fwd", dpc_kid("k_drcrgb_fwd"), k_drcrgb_fwd, dim3(col_tiles(p) * p->B), dim3(kColThreads), 0, st, *p,
             exp((double)p->clip_val), vox, C, a, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  return finalize(p, loss_tiles, weights, loss, st);
}

int dpc_drc_rgb_loss_bwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, const float* dloss, float* dvox,
                         float* dC, void* stream) {
  const int rc = rgb_check(p, gt_factor);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!vox || !C || !gt || !dvox || !dC) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  const RgbArgs a{div, div_eps, clip_after != 0, gt, gt_factor, gt_planar != 0, weights, 1.0f / (float)p->B};
  const dim3 gcol(col_tiles(p) * p->B);
  const double e_eps = exp((double)p->clip_val);
  if (p->D == 32)
    DPC_LAUNCH("k_drcrgb_bwd", dpc_kid("k_drcrgb_bwd", 32), (k_drcrgb_bwd<32>), gcol, dim3(kColThreads), 0, st, *p, e_eps, vox, C, a, dloss, dvox, dC);
  else if (p->D == 64)
    DPC_LAUNCH("k_drcrgb_bwd", dpc_kid("k_drcrgb_bwd", 64), (k_drcrgb_bwd<64>), gcol, dim3(kColThreads), 0, st, *p, e_eps, vox, C, a, dloss, dvox, dC);
  else
    DPC_LAUNCH("k_drcrgb_bwd", dpc_kid("k_drcrgb_bwd_dyn"), k_drcrgb_bwd_dyn, gcol, dim3(kColThreads), 0, st, *p, e_eps, vox, C, a, dloss, dvox, dC);
  return launch_ok();
}

}  // extern "C"
