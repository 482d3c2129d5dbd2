// What the colour column kernels of dpc_rgb.hip (k_rgb_fwd / k_rgb_bwd) and dpc_drc_loss.hip (k_drcrgb_*) share: their
// per-launch arguments, the ground-truth read, the colour the integral sees, and the entry points' argument checks.
#pragma once
#include "dpc_kernels.h"

namespace dpck {

// What the colour column kernels need besides the grids (uniform per launch).
struct RgbArgs {
  const float* div;      // [B,D,H,W] smoothed raw occupancies | nullptr: no division (point_cloud.py:255-259)
  float div_eps;
  int clip_after;        // clamp(C, 0, 1) after the division (:261-262)
  const float* gt;       // images [S,f*H,f*W,3], or [S,3,f*H,f*W] when planar | nullptr: projection only
  int f, planar;
  const float* weights;  // [S] | nullptr = 1
  float inv_S;
};

// ground truth of the image pixel (prow, pcol): images[s, f*prow, f*pcol, :] -- TF-1's bilinear resize_images without
// align_corners samples exactly there for an integer factor (losses.py:74-77)
__device__ inline void rgb_gt(const RgbArgs& a, const DpcParams& P, int b, int prow, int pcol, float (&g)[3]) {
  const size_t Hi = (size_t)a.f * P.H, Wi = (size_t)a.f * P.W, y = (size_t)prow * a.f, x = (size_t)pcol * a.f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    g[c] = a.planar ? a.gt[(((size_t)b * 3 + c) * Hi + y) * Wi + x] : a.gt[(((size_t)b * Hi + y) * Wi + x) * 3 + c];
}

// the colour the integral sees at one voxel: C / (div + eps), clamped when clip_after; `scale` = d value / d C
__device__ inline float rgb_value(const RgbArgs& a, float c, float dv, float& scale) {
  scale = 1.0f;
  if (a.div != nullptr) {
    scale = 1.0f / (dv + a.div_eps);
    c *= scale;
  }
  if (a.clip_after) {
    if (!(c >= 0.f && c <= 1.f)) scale = 0.f;   // torch.clamp's backward: the gradient passes inside [0, 1]
    c = fminf(fmaxf(c, 0.f), 1.f);
  }
  return c;
}

// Host side: argument checks shared by the colour entry points
inline int rgb_validate(const DpcParams* p) {
  const int rc = validate(p);
  if (rc != DPC_OK) return rc;
  if (p->point_replicas > 1 || p->point_index != nullptr) return DPC_ERR_SHAPE;   // one row of points and colours per cloud
  return DPC_OK;
}

inline int rgb_check(const DpcParams* p, int gt_factor) {
  const int rc = rgb_validate(p);
  if (rc != DPC_OK) return rc;
  if (gt_factor < 1 || (long long)gt_factor * p->H > 1024 || (long long)gt_factor * p->W > 1024) return DPC_ERR_SHAPE;
  return DPC_OK;
}

// the four loss entries' checks and the kernels' RgbArgs.  DPC_OK with p->B == 0 means "nothing to launch": `a` is then not set
enum class ColourGt { optional, required };
inline int colour_check(const DpcParams* p, const float* vox, const float* C, const float* div, float div_eps, int clip_after,
                        const float* gt, ColourGt need, int gt_factor, int gt_planar, const float* weights, RgbArgs& a) {
  const int rc = rgb_check(p, gt_factor);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!vox || !C || (need == ColourGt::required && !gt)) return DPC_ERR_NULL;
  a = RgbArgs{div, div_eps, clip_after != 0, gt, gt_factor, gt_planar != 0, weights, 1.0f / (float)p->B};
  return DPC_OK;
}

}  // namespace dpck
