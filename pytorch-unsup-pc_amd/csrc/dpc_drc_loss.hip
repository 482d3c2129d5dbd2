// Ray-consistency (DRC) losses as ray potentials sum_k p_k psi_k over the ray-termination probabilities, fused with their
// hand-written backwards: the mask loss on grid_wh, a potential on the column skeleton of dpc_ray_column.h (MaskPot;
// k_drcmask_fwd / k_drcmask_bwd are shells around the skeleton, as k_depth_* in dpc_depth.hip are), and the colour loss on the
// renderer's voxels and colour grid (k_drcrgb_fwd / k_drcrgb_bwd, the inputs and options of k_rgb_* in dpc_rgb.hip).
// Reference (TF-1 originals): drc_loss, drc_rgb_loss, add_drc_loss, add_drc_rgb_loss (dpc/util/losses.py:23-66, 93-110) on
// drc_event_probabilities (dpc/util/drc.py:48-106) and the flip of pointcloud_project_fast (dpc/util/point_cloud.py:269-276).
// Design notes: DESIGN.md section 4.  The tile sum and the finalize are those of dpc_depth.hip and dpc_rgb.hip (dpc_kernels.h), the
// images' reads, the colour value and the entries' checks those of dpc_rgb.hip (dpc_colour_column.h); loss = sum_s w_s^2 (the sample's tiles) / S: no 1/2 (losses.py:29, 46, 62, 106).
#include "dpc_colour_column.h"
#include "dpc_ray_column.h"

namespace dpck {
namespace {

// ------------------------------------------------------------------------------------------------------
// Mask loss.  Ray cost (1 - g) sum_{k<D} p_k + g p_D with g the mask at the ray's pixel (drc_loss, losses.py:23-29: psi is
// 1 - g for the D voxels and g for the background).  sum_{k<D} p_k is summed, not taken as 1 - p_D: with the e^eps factors
// the probabilities do not add up to one.
// ------------------------------------------------------------------------------------------------------
struct MaskPot {
  const float* gt;        // [S, f*H, f*W] masks in image orientation, S = B
  int f;                  // pixel (y, x) reads gt[f*y, f*x] (TF-1 resize_images without align_corners, integer factor)
  const float* weights;   // [S] | nullptr = 1
  float inv_S;
  const float* dloss;     // backward: device scalar, the gradient arriving at the loss | nullptr = 1

  struct Fwd {
    double g = 0.0, psum = 0.0;
    float cost = 0.f;
  };
  __device__ __forceinline__ void fwd_read(Fwd& a, const DpcParams& P, int b, int prow, int pcol) const {
    a.g = (double)column_gt(gt, f, P, b, prow, pcol);
  }
  __device__ __forceinline__ void fwd_add(Fwd& a, int z, int, double e_eps, double y, double A) const {
    a.psum = fma(z == 0 ? e_eps * y : y, A, a.psum);
  }
  __device__ __forceinline__ void fwd_close(Fwd& a, const DpcParams&, double e_eps, double A) const {
    a.cost = (float)fma(1.0 - a.g, a.psum, a.g * e_eps * A);
  }
  __device__ __forceinline__ void fwd_epilogue(const Fwd& a, const DpcParams&, const Blk& bk, int, bool,
                                               float* __restrict__ loss_tiles) const {
    const float tot = tile_sum(a.cost);
    if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
  }

  // Backward: psi_m = 1 - g, psi_D = g.  The cost is linear in the probabilities, so the gradient arriving at a ray is
  // dloss w_s^2 / S whatever the forward gave.
  struct Bwd {
    double fg;   // 1 - g
    float gd;
  };
  __device__ __forceinline__ Bwd bwd_read(const DpcParams& P, int b, int prow, int pcol) const {
    Bwd r;
    r.fg = 1.0 - (double)column_gt(gt, f, P, b, prow, pcol);
    r.gd = (dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(weights, b) * inv_S;
    return r;
  }
  __device__ __forceinline__ double bwd_start(const Bwd& r, const DpcParams&, double e_eps) const { return e_eps * (1.0 - r.fg); }
  __device__ __forceinline__ double bwd_term(const Bwd& r, const DpcParams&, int m, int, double e_eps) const {
    return m == 0 ? e_eps * r.fg : r.fg;
  }
  __device__ __forceinline__ float bwd_grad(const Bwd& r, const DpcParams&, double) const { return r.gd; }
};

template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 64 ? 4 : 2)) void k_drcmask_fwd(DpcParams P, RayHost rh, double e_eps,
                                                                               const float* __restrict__ grid_wh,
                                                                               const float* __restrict__ s, TapsT<RB> taps,
                                                                               MaskPot pot, float* __restrict__ loss_tiles) {
  ray_column_fwd<MaskPot, DD, RB>(P, rh, e_eps, grid_wh, s, taps, pot, loss_tiles);
}

__global__ __launch_bounds__(kColThreads) void k_drcmask_fwd_dyn(DpcParams P, RayHost rh, double e_eps,
                                                                 const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                                 TapsDyn taps, MaskPot pot, float* __restrict__ loss_tiles) {
  ray_column_fwd_dyn(P, rh, e_eps, grid_wh, s, taps, pot, loss_tiles);
}

template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 32 ? 4 : (DD <= 64 ? 2 : 1)))
void k_drcmask_bwd(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh, const float* __restrict__ s,
                   TapsT<RB> taps, TapsT<RB> taps_adj, MaskPot pot, float* __restrict__ dgrid, float* __restrict__ ds_part,
                   unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  ray_column_bwd<MaskPot, DD, RB>(P, rh, e_eps, grid_wh, s, taps, taps_adj, pot, dgrid, ds_part, ds_count, ds);
}

__global__ __launch_bounds__(kColThreads) void k_drcmask_bwd_dyn(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh,
                                                                 const float* __restrict__ s, TapsDyn taps, MaskPot pot,
                                                                 float* __restrict__ dgrid, float* dv_grid,
                                                                 float* __restrict__ ds_part, unsigned int* __restrict__ ds_count,
                                                                 float* __restrict__ ds) {
  ray_column_bwd_dyn(P, rh, e_eps, grid_wh, s, taps, pot, dgrid, dv_grid, ds_part, ds_count, ds);
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

}  // namespace
}  // namespace dpck

using namespace dpck;

extern "C" {

size_t dpc_drc_workspace_bytes(const DpcParams* p) { return column_workspace_bytes(p); }

int dpc_drc_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, float* loss_tiles, float* loss, void* stream) {
  if (p && gt_mask && (!loss || !loss_tiles)) return DPC_ERR_SHAPE;   // a loss nobody can receive
  ColumnCall c;
  int rc = column_check(p, grid_wh, host_kern_z, gt_mask, true, gt_factor, c);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  const MaskPot pot{gt_mask, gt_factor, weights, c.inv_S, nullptr};
  const dim3 gcol(col_tiles(p) * p->B);
  bool done;
  rc = column_dispatch(p, c.pz, done, [&](auto dd, auto rb) {
    constexpr int DD = decltype(dd)::value, RB = decltype(rb)::value;
    DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd", DD, RB), (k_drcmask_fwd<DD, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh,
               c.e_eps, grid_wh, s, make_taps<RB>(host_kern_z, c.pz, false), pot, loss_tiles);
  });
  if (rc != DPC_OK) return rc;
  if (!done)  // other depths / longer kernels: same arithmetic, column re-read from global
    DPC_LAUNCH("k_drcmask_fwd", dpc_kid("k_drcmask_fwd_dyn"), k_drcmask_fwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps_dyn(host_kern_z, p->taps_z, false), pot, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  return launch_tile_loss_finalize(p, loss_tiles, c.inv_S, weights, loss, st);
}

int dpc_drc_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_mask,
                     int gt_factor, const float* weights, const float* dloss, float* dgrid_wh, float* ds, void* workspace,
                     void* stream) {
  ColumnCall c;
  int rc = column_check(p, grid_wh, host_kern_z, gt_mask, true, gt_factor, c);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dgrid_wh || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  const ColumnWorkspace w = column_workspace(p, workspace);
  const MaskPot pot{gt_mask, gt_factor, weights, c.inv_S, dloss};
  const dim3 gcol(col_tiles(p) * p->B);
  bool done;
  rc = column_dispatch(p, c.pz, done, [&](auto dd, auto rb) {
    constexpr int DD = decltype(dd)::value, RB = decltype(rb)::value;
    DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd", DD, RB), (k_drcmask_bwd<DD, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh,
               c.e_eps, grid_wh, s, make_taps<RB>(host_kern_z, c.pz, false), make_taps<RB>(host_kern_z, c.pz, true), pot, dgrid_wh,
               w.ds_part, w.ds_count, ds);
  });
  if (rc != DPC_OK) return rc;
  if (!done) {
    if (!may_need_dv(p)) return DPC_ERR_TAPS;   // cannot happen: a kernel of <= 31 taps has a compiled window
    DPC_LAUNCH("k_drcmask_bwd", dpc_kid("k_drcmask_bwd_dyn"), k_drcmask_bwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps_dyn(host_kern_z, p->taps_z, false), pot, dgrid_wh, w.dv, w.ds_part, w.ds_count, ds);
  }
  return launch_ok();
}

int dpc_drc_rgb_loss_fwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, float* loss_tiles, float* loss,
                         void* stream) {
  if (p && gt && (!loss || !loss_tiles)) return DPC_ERR_SHAPE;   // a loss nobody can receive
  RgbArgs a;
  const int rc = colour_check(p, vox, C, div, div_eps, clip_after, gt, ColourGt::required, gt_factor, gt_planar, weights, a);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  DPC_LAUNCH("k_drcrgb_fwd", dpc_kid("k_drcrgb_fwd"), k_drcrgb_fwd, dim3(col_tiles(p) * p->B), dim3(kColThreads), 0, st, *p,
             exp((double)p->clip_val), vox, C, a, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  return launch_tile_loss_finalize(p, loss_tiles, a.inv_S, weights, loss, st);
}

int dpc_drc_rgb_loss_bwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                         const float* gt, int gt_factor, int gt_planar, const float* weights, const float* dloss, float* dvox,
                         float* dC, void* stream) {
  RgbArgs a;
  const int rc = colour_check(p, vox, C, div, div_eps, clip_after, gt, ColourGt::required, gt_factor, gt_planar, weights, a);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dvox || !dC) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
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
