// Colour node of the projection: per-point RGB splatted with the points' trilinear weights (k_rgb_splat, its gather
// backward k_rgb_splat_bwd), and column kernels that integrate the colour grid along each ray with the ray-termination
// probabilities over a white background, with the squared-error loss against the input image (k_rgb_fwd, the hand-written
// backward k_rgb_bwd; the tile sum and the loss's one-block finalize are the loss nodes' shared ones, dpc_kernels.h).
// Reference (TF-1 originals): pointcloud2voxels3d_fast's rgb half (dpc/util/point_cloud.py:98-134), the clips, the division
// by the occupancies and the flip of pointcloud_project_fast (:244-262, 275-277), project_volume_rgb_integral
// (dpc/util/drc.py:132-142), add_proj_rgb_loss (dpc/util/losses.py:69-90).  Design notes: DESIGN.md section 4.
#include "dpc_colour_column.h"

namespace dpck {
namespace {

constexpr int kRgbThreads = 256;

inline unsigned rgb_blocks(size_t total) {
  const size_t b = (total + kRgbThreads - 1) / kRgbThreads;
  return (unsigned)(b < 1 ? 1 : (b > 1048576 ? 1048576 : b));
}

// ------------------------------------------------------------------------------------------------------
// Colour splat: C_raw[b, c, iz+k, iy+j, ix+i] += wz[k] wy[j] wx[i] rgb[b,n,c]        point_cloud.py:98-118
// Two neighbouring lanes per (cloud, channel, point), the point index next fastest: the pair owns the two x corners, which
// are neighbours in memory, so each of a wave's four atomic instructions leaves as 32 two-float requests instead of 64
// one-float ones (scattered float atomics are bound by requests, MI355X_MICROARCH.md "Global float atomics").  The cell
// and the weights are those of the occupancy splat (make_record / cell_from_record, corners past the grid dropped).
// fp32 hardware atomics into a zeroed grid: the sums depend on the order the adds arrive in, so the grid is not
// bit-reproducible from run to run.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRgbThreads) void k_rgb_splat(DpcParams P, const float* __restrict__ tr,
                                                           const float* __restrict__ rgb, float* __restrict__ out) {
  const int D = P.D, H = P.H, W = P.W;
  const size_t total = (size_t)P.B * 3 * P.N * 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 1);
    const size_t h = i >> 1;
    const int n = (int)(h % P.N);
    const size_t bc = h / P.N;
    const int c = (int)(bc % 3);
    const size_t pt = (bc / 3) * P.N + n;
    const Cell cl = cell_from_record(make_record((double)tr[3 * pt], (double)tr[3 * pt + 1], (double)tr[3 * pt + 2], D, H, W));
    if (!cl.valid || cl.ix + e >= W) continue;
    const float wc = (e ? cl.wx[1] : cl.wx[0]) * rgb[3 * pt + c];
    float* plane = out + bc * D * H * W + cl.ix + e;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool ok = (cl.iz + k < D) && (cl.iy + j < H);
        if (ok) atomicAdd(plane + ((size_t)(cl.iz + k) * H + cl.iy + j) * W, cl.wz[k] * cl.wy[j] * wc);
      }
  }
}

// Backward of the splat: one thread per point gathers its 8 corners from the three planes.
//   drgb_c = sum_corners w dC_c;   dtr = k_splat_bwd's formula (dpc_stages.hip) on g[corner] = sum_c rgb_c dC_c[corner]
// dtr == nullptr: pc_rgb_stop_points_gradient (point_cloud.py:112-113).  Points outside the cube get exact zeros.
__global__ __launch_bounds__(kRgbThreads) void k_rgb_splat_bwd(DpcParams P, const float* __restrict__ tr,
                                                               const float* __restrict__ rgb, const float* __restrict__ dC,
                                                               float* __restrict__ drgb, float* __restrict__ dtr) {
  const int D = P.D, H = P.H, W = P.W;
  const size_t total = (size_t)P.B * P.N, plane = (size_t)D * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / P.N;
    const Cell c = cell_from_record(make_record((double)tr[3 * i], (double)tr[3 * i + 1], (double)tr[3 * i + 2], D, H, W));
    float dcol[3] = {0.f, 0.f, 0.f};
    float dZ = 0.f, dY = 0.f, dX = 0.f;
    if (c.valid) {
      const float col[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
      const float* gb = dC + b * 3 * plane;
      float cv[2][2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const bool ok = (c.iz + k < D) && (c.iy + j < H) && (c.ix + e < W);
            const size_t at = ((size_t)(c.iz + k) * H + c.iy + j) * W + c.ix + e;
            const float w = c.wz[k] * c.wy[j] * c.wx[e];
            float g = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float d = ok ? gb[ch * plane + at] : 0.f;
              dcol[ch] = fmaf(w, d, dcol[ch]);
              g = fmaf(col[ch], d, g);
            }
            cv[k][j][e] = g;
          }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          dZ += (cv[1][a][e] - cv[0][a][e]) * c.wy[a] * c.wx[e];
          dY += (cv[a][1][e] - cv[a][0][e]) * c.wz[a] * c.wx[e];
          dX += (cv[a][e][1] - cv[a][e][0]) * c.wz[a] * c.wy[e];
        }
      dZ *= (float)(D - 1); dY *= (float)(H - 1); dX *= (float)(W - 1);
    }
    drgb[3 * i] = dcol[0]; drgb[3 * i + 1] = dcol[1]; drgb[3 * i + 2] = dcol[2];
    if (dtr != nullptr) { dtr[3 * i] = dZ; dtr[3 * i + 1] = dY; dtr[3 * i + 2] = dX; }
  }
}

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

int dpc_rgb_splat_fwd(const DpcParams* p, const float* tr, const float* rgb, float* out, void* stream) {
  const int rc = rgb_validate(p);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!out || (p->N > 0 && (!tr || !rgb))) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (!zero_words_async(out, (size_t)p->B * 3 * p->D * p->H * p->W, st)) return DPC_ERR_LAUNCH;
  if (p->N == 0) return DPC_OK;
  DPC_LAUNCH("k_rgb_splat", dpc_kid("k_rgb_splat"), k_rgb_splat, dim3(rgb_blocks((size_t)p->B * 3 * p->N * 2)), dim3(kRgbThreads), 0, st,
             *p, tr, rgb, out);
  return launch_ok();
}

int dpc_rgb_splat_bwd(const DpcParams* p, const float* tr, const float* rgb, const float* dC, float* drgb, float* dtr,
                      void* stream) {
  const int rc = rgb_validate(p);
  if (rc != DPC_OK || p->B == 0 || p->N == 0) return rc;
  if (!tr || !rgb || !dC || !drgb) return DPC_ERR_NULL;
  DPC_LAUNCH("k_rgb_splat_bwd", dpc_kid("k_rgb_splat_bwd"), k_rgb_splat_bwd, dim3(rgb_blocks((size_t)p->B * p->N)), dim3(kRgbThreads),
             0, (hipStream_t)stream, *p, tr, rgb, dC, drgb, dtr);
  return launch_ok();
}

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
