// Colour projection and loss: column kernels that integrate the colour grid of the splat (dpc_rgb_splat.hip) along each ray
// with the ray-termination probabilities over a white background, with the squared-error loss against the input image
// (k_rgb_fwd, the hand-written backward k_rgb_bwd; the tile sum and the loss's one-block finalize are the loss nodes' shared
// ones, dpc_kernels.h).
// Reference (TF-1 originals): the clips, the division by the occupancies and the flip of pointcloud_project_fast
// (dpc/util/point_cloud.py:244-262, 275-277), project_volume_rgb_integral (dpc/util/drc.py:132-142), add_proj_rgb_loss
// (dpc/util/losses.py:69-90).  Design notes: DESIGN.md section 4.
#include "dpc_colour_column.h"

namespace dpck {
namespace {

// ------------------------------------------------------------------------------------------------------
// Column kernels.  One thread per ray (b, y, x), x fastest: every plane read and write is coalesced.
// ------------------------------------------------------------------------------------------------------
// Forward: p_0 = e^eps y_0, p_k = y_k A_k, p_D = e^eps A_D (k_drc_fwd, dpc_stages.hip);
//   proj_rgb[b, H-1-y, x, c] = sum_{k<D} p_k C[b,c,k,y,x] + p_D * 1                 grid (ceil(HW/256) * B)
__global__ __launch_bounds__(kColThreads) void k_rgb_fwd(DpcParams P, double e_eps, const float* __restrict__ vox,
                                                         const float* __restrict__ C, RgbArgs a, float* __restrict__ proj_rgb,
                                                         float* __restrict__ loss_tiles) {
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const float eps = P.clip_val, hi = (float)(1.0 - (double)P.clip_val);
  float sq = 0.f;
  if (ray < HW) {
    const int yrow = ray / P.W, x = ray - yrow * P.W, prow = P.H - 1 - yrow;
    float g[3] = {0.f, 0.f, 0.f};
    if (a.gt != nullptr) rgb_gt(a, P, b, prow, x, g);
    const size_t plane = (size_t)D * HW;
    const float* col = vox + (size_t)b * plane + ray;
    const float* ccol = C + (size_t)b * 3 * plane + ray;
    const float* dcol = a.div != nullptr ? a.div + (size_t)b * plane + ray : nullptr;
    double A = 1.0, acc[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < D; ++k) {
      const size_t at = (size_t)k * HW;
      const float y = fminf(fmaxf(col[at], eps), hi);
      const double pk = (k == 0 ? e_eps : 1.0) * (double)y * A;
      const float dv = dcol != nullptr ? dcol[at] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float scale;
        acc[c] = fma(pk, (double)rgb_value(a, ccol[c * plane + at], dv, scale), acc[c]);
      }
      A *= 1.0 - (double)y;
    }
    const double pD = e_eps * A;   // the white background
    float* o = proj_rgb != nullptr ? proj_rgb + (((size_t)b * P.H + prow) * P.W + x) * 3 : nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = (float)(acc[c] + pD);
      if (o != nullptr) o[c] = v;
      const float diff = g[c] - v;
      sq = fmaf(diff, diff, sq);
    }
  }
  if (a.gt != nullptr) {   // block-uniform
    const float tot = tile_sum(sq);
    if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
  }
}

// Backward.  Residual of a ray r_c = dloss w_s^2 (proj_c - g_c) / S + dproj_rgb_c;  dC_{c,k} = p_k r_c (times 1/(div+eps) and
// the after-clip mask);  the occupancies see the DRC backward of k_drc_bwd (dpc_stages.hip) with gp_k = a_k = sum_c r_c C_{c,k},
// gp_D = a_D = sum_c r_c:   dL/dy_m = a_m E_m A_m - (sum_{k>m} a_k p_k) / (1 - y_m).
// Pass 1 parks the prefix products A_m in dvox (fp32), pass 2 walks the ray backwards with the suffix sum and overwrites them.
__global__ __launch_bounds__(kColThreads) void k_rgb_bwd(DpcParams P, double e_eps, const float* __restrict__ vox,
                                                         const float* __restrict__ C, RgbArgs a, const float* __restrict__ proj_rgb,
                                                         const float* __restrict__ dloss, const float* __restrict__ dproj_rgb,
                                                         float* __restrict__ dvox, float* __restrict__ dC) {
  const int HW = P.H * P.W, D = P.D;
  const Blk bk = block_coords(P.B);
  const int b = bk.y, ray = bk.x * kColThreads + threadIdx.x;
  const float eps = P.clip_val, hi = (float)(1.0 - (double)P.clip_val);
  if (ray >= HW) return;
  const int yrow = ray / P.W, x = ray - yrow * P.W, prow = P.H - 1 - yrow;
  const size_t pix = (((size_t)b * P.H + prow) * P.W + x) * 3;
  float r[3] = {0.f, 0.f, 0.f};
  if (a.gt != nullptr) {
    float g[3];
    rgb_gt(a, P, b, prow, x, g);
    const float k = (dloss != nullptr ? *dloss : 1.0f) * ::sample_weight2(a.weights, b) * a.inv_S;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = k * (proj_rgb[pix + c] - g[c]);
  }
  if (dproj_rgb != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] += dproj_rgb[pix + c];
  }
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
  double suffix = ((double)r[0] + (double)r[1] + (double)r[2]) * e_eps * A;   // sum_{k>m} a_k p_k, starting from the background
  for (int m = D - 1; m >= 0; --m) {
    const size_t at = (size_t)m * HW;
    const float v = col[at];
    const float y = fminf(fmaxf(v, eps), hi);
    const double EA = (m == 0 ? e_eps : 1.0) * (double)gv[at];
    const double pm = EA * (double)y;
    const float dv = dcol != nullptr ? dcol[at] : 0.f;
    double am = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float scale;
      const float cv = rgb_value(a, ccol[c * plane + at], dv, scale);
      am = fma((double)r[c], (double)cv, am);
      gc[c * plane + at] = (float)(pm * (double)r[c]) * scale;
    }
    const double dy = am * EA - suffix / (1.0 - (double)y);
    gv[at] = (v >= eps && v <= hi) ? (float)dy : 0.f;
    suffix = fma(am, pm, suffix);
  }
}

}  // namespace
}  // namespace dpck

using namespace dpck;

extern "C" {

int dpc_rgb_loss_fwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                     const float* gt, int gt_factor, int gt_planar, const float* weights, float* proj_rgb, float* loss_tiles,
                     float* loss, void* stream) {
  if (p && ((gt && (!loss || !loss_tiles)) || (!gt && !proj_rgb))) return DPC_ERR_SHAPE;  // a loss nobody can receive / nothing asked for
  RgbArgs a;
  const int rc = colour_check(p, vox, C, div, div_eps, clip_after, gt, ColourGt::optional, gt_factor, gt_planar, weights, a);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  DPC_LAUNCH("k_rgb_fwd", dpc_kid("k_rgb_fwd"), k_rgb_fwd, dim3(col_tiles(p) * p->B), dim3(kColThreads), 0, st, *p,
             exp((double)p->clip_val), vox, C, a, proj_rgb, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  if (!gt) return DPC_OK;
  return launch_tile_loss_finalize(p, loss_tiles, 0.5f * a.inv_S, weights, loss, st);
}

int dpc_rgb_loss_bwd(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                     const float* gt, int gt_factor, int gt_planar, const float* weights, const float* proj_rgb,
                     const float* dloss, const float* dproj_rgb, float* dvox, float* dC, void* stream) {
  if (p && !gt && !dproj_rgb) return DPC_ERR_SHAPE;   // no gradient arrives anywhere
  RgbArgs a;
  const int rc = colour_check(p, vox, C, div, div_eps, clip_after, gt, ColourGt::optional, gt_factor, gt_planar, weights, a);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dvox || !dC || (gt && !proj_rgb)) return DPC_ERR_NULL;
  DPC_LAUNCH("k_rgb_bwd", dpc_kid("k_rgb_bwd"), k_rgb_bwd, dim3(col_tiles(p) * p->B), dim3(kColThreads), 0, (hipStream_t)stream, *p,
             exp((double)p->clip_val), vox, C, a, proj_rgb, dloss, dproj_rgb, dvox, dC);
  return launch_ok();
}

}  // extern "C"
