// Expected depth as a ray potential on the column skeleton of dpc_ray_column.h: psi_k = k/D - 1/2 + camera_distance for the
// voxels, max_depth for the background, the squared-error loss against a ground-truth depth map and the gradient arriving at
// the depth map itself (DepthPot; k_depth_fwd / k_depth_bwd are shells around the skeleton), and the one-block finalize all
// the loss nodes share (k_tile_loss_finalize).
// Reference: add_proj_depth_loss (dpc/util/losses.py:113-136) on drc_depth_projection (dpc/util/drc.py:145-160).
// Design notes: DESIGN.md section 4.
#include "dpc_ray_column.h"

namespace dpck {
namespace {

// psi_k = k/D - 1/2 + camera_distance, psi_D = max_depth (dpc/util/drc.py:145-149; the formula of dpc_stages.hip), split into
// the part all voxels share and k/D, a compile-time constant of the unrolled kernels: the sums below carry k/D alone and the
// shared part is added once per ray (sum_{k<D} p_k psi_k = sum p_k k/D + psi_base sum p_k) -- one register for the whole
// column instead of a double per voxel.
__device__ inline double psi_base(const DpcParams& P) { return (double)P.camera_distance - 0.5; }

// The depth potential with its loss (uniform per launch).  gt [S, f*H, f*W] depth maps in image orientation, S = B.
struct DepthPot {
  const float* gt;          // nullptr: projection only
  int f;                    // gt is f times the depth map's size; pixel (y, x) reads gt[f*y, f*x] (TF-1 nearest neighbour)
  float max_dataset_depth;  // the dataset's background value, replaced by P.max_depth where the two differ
  const float* weights;     // [S] | nullptr = 1
  float inv_S;
  float* depth;             // forward: the depth map [B,H,W], rows flipped | nullptr
  const float* dloss;       // backward: device scalar, the gradient arriving at the loss | nullptr = 1
  const float* ddepth;      // backward: the caller's own gradient at the depth map [B,H,W] | nullptr

  __device__ __forceinline__ float gt_at(const DpcParams& P, int b, int prow, int pcol) const {
    const float g = column_gt(gt, f, P, b, prow, pcol);
    return (g == max_dataset_depth && max_dataset_depth != P.max_depth) ? P.max_depth : g;
  }

  // Forward: sum p_k and sum p_k k/D; depth = psi_base sum p_k + sum p_k k/D + p_D max_depth.
  struct Fwd {
    float g = 0.f;
    double psum = 0.0, dsum = 0.0, d = 0.0;
  };
  __device__ __forceinline__ void fwd_read(Fwd& a, const DpcParams& P, int b, int prow, int pcol) const {
    if (gt != nullptr) a.g = gt_at(P, b, prow, pcol);
  }
  __device__ __forceinline__ void fwd_add(Fwd& a, int z, int D, double e_eps, double y, double A) const {
    const double pk = (z == 0 ? e_eps * y : y) * A;
    a.psum += pk;
    a.dsum = fma(pk, (double)z / (double)D, a.dsum);
  }
  __device__ __forceinline__ void fwd_close(Fwd& a, const DpcParams& P, double e_eps, double A) const {
    a.d = fma(psi_base(P), a.psum, a.dsum) + e_eps * A * (double)P.max_depth;
  }
  // the depth at the row-flipped pixel, this tile's squared error
  __device__ __forceinline__ void fwd_epilogue(const Fwd& a, const DpcParams& P, const Blk& bk, int ray, bool live,
                                               float* __restrict__ loss_tiles) const {
    float sq = 0.f;
    if (live) {
      const int yrow = ray / P.W, x = ray - yrow * P.W;
      const float df = (float)a.d;
      if (depth != nullptr) depth[(size_t)bk.y * P.H * P.W + (P.H - 1 - yrow) * P.W + x] = df;
      const float diff = a.g - df;
      sq = diff * diff;
    }
    if (gt != nullptr) {  // block-uniform
      const float tot = tile_sum(sq);
      if (threadIdx.x == 0) loss_tiles[(size_t)bk.y * bk.nx + bk.x] = tot;
    }
  }

  // Backward.  R is carried as R - psi_base: then E_m psi_m - R_m = m/D - R_m for m > 0 (a compile-time constant minus the
  // carry).  The gradient arriving at the ray's depth: from the loss, (1/2) w^2 (g - depth)^2 / S times dloss, plus the
  // caller's own.
  struct Bwd {
    float g, w2, up, gin;
    double base;   // psi_base, formed once per ray: formed anew at each use below, k_depth_bwd<32, 2> needs 128 VGPRs and spills (84)
  };
  __device__ __forceinline__ Bwd bwd_read(const DpcParams& P, int b, int prow, int pcol) const {
    Bwd r;
    r.g = gt != nullptr ? gt_at(P, b, prow, pcol) : 0.f;
    r.w2 = ::sample_weight2(weights, b);
    r.up = dloss != nullptr ? *dloss : 1.0f;
    r.gin = ddepth != nullptr ? ddepth[(size_t)b * (P.H * P.W) + prow * P.W + pcol] : 0.f;
    r.base = psi_base(P);
    return r;
  }
  __device__ __forceinline__ double bwd_start(const Bwd& r, const DpcParams& P, double e_eps) const {
    return e_eps * (double)P.max_depth - r.base;
  }
  __device__ __forceinline__ double bwd_term(const Bwd& r, const DpcParams&, int m, int D, double e_eps) const {
    return m == 0 ? (e_eps - 1.0) * r.base : (double)m / (double)D;
  }
  __device__ __forceinline__ float bwd_grad(const Bwd& r, const DpcParams&, double R) const {
    return gt != nullptr ? fmaf(r.up * r.w2 * inv_S, (float)(R + r.base) - r.g, r.gin) : r.gin;
  }
};

template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 64 ? 4 : 2)) void k_depth_fwd(DpcParams P, RayHost rh, double e_eps,
                                                                             const float* __restrict__ grid_wh,
                                                                             const float* __restrict__ s, TapsT<RB> taps,
                                                                             DepthPot pot, float* __restrict__ loss_tiles) {
  ray_column_fwd<DepthPot, DD, RB>(P, rh, e_eps, grid_wh, s, taps, pot, loss_tiles);
}

__global__ __launch_bounds__(kColThreads) void k_depth_fwd_dyn(DpcParams P, RayHost rh, double e_eps,
                                                               const float* __restrict__ grid_wh, const float* __restrict__ s,
                                                               TapsDyn taps, DepthPot pot, float* __restrict__ loss_tiles) {
  ray_column_fwd_dyn(P, rh, e_eps, grid_wh, s, taps, pot, loss_tiles);
}

template <int DD, int RB>
__global__ __launch_bounds__(kColThreads, (DD <= 32 ? 4 : (DD <= 64 ? 2 : 1)))
void k_depth_bwd(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh, const float* __restrict__ s,
                 TapsT<RB> taps, TapsT<RB> taps_adj, DepthPot pot, float* __restrict__ dgrid, float* __restrict__ ds_part,
                 unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  ray_column_bwd<DepthPot, DD, RB>(P, rh, e_eps, grid_wh, s, taps, taps_adj, pot, dgrid, ds_part, ds_count, ds);
}

__global__ __launch_bounds__(kColThreads) void k_depth_bwd_dyn(DpcParams P, RayHost rh, double e_eps, const float* __restrict__ grid_wh,
                                                               const float* __restrict__ s, TapsDyn taps, DepthPot pot,
                                                               float* __restrict__ dgrid, float* dv_grid, float* __restrict__ ds_part,
                                                               unsigned int* __restrict__ ds_count, float* __restrict__ ds) {
  ray_column_bwd_dyn(P, rh, e_eps, grid_wh, s, taps, pot, dgrid, dv_grid, ds_part, ds_count, ds);
}

// loss = scale sum_s w_s^2 (sum of the sample's tiles, in tile order), scale = 1/(2S) for the squared-error losses and 1/S for
// the ray-consistency ones.  One block; the same bits on every run.
__global__ __launch_bounds__(256) void k_tile_loss_finalize(const float* __restrict__ loss_tiles, int ntile, int S, float scale,
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
    *loss = tot * scale;
  }
}

}  // namespace

int launch_tile_loss_finalize(const DpcParams* p, const float* loss_tiles, float scale, const float* weights, float* loss,
                              hipStream_t st) {
  DPC_LAUNCH("k_tile_loss_finalize", dpc_kid("k_tile_loss_finalize"), k_tile_loss_finalize, dim3(1), dim3(256), 0, st, loss_tiles,
             col_tiles(p), p->B, scale, weights, loss);
  return launch_ok();
}

}  // namespace dpck

using namespace dpck;

extern "C" {

size_t dpc_depth_workspace_bytes(const DpcParams* p) { return column_workspace_bytes(p); }

int dpc_depth_loss_fwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_depth,
                       int gt_factor, float max_dataset_depth, const float* weights, float* depth, float* loss_tiles, float* loss,
                       void* stream) {
  if (p && ((gt_depth && (!loss || !loss_tiles)) || (!gt_depth && !depth))) return DPC_ERR_SHAPE;  // a loss nobody can receive / nothing asked for
  ColumnCall c;
  int rc = column_check(p, grid_wh, host_kern_z, gt_depth, false, gt_factor, c);
  if (rc != DPC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->B == 0) return (!loss || zero_words_async(loss, 1, st)) ? DPC_OK : DPC_ERR_LAUNCH;  // the loss of nothing is 0
  const DepthPot pot{gt_depth, gt_factor, max_dataset_depth, weights, c.inv_S, depth, nullptr, nullptr};
  const dim3 gcol(col_tiles(p) * p->B);
  bool done;
  rc = column_dispatch(p, c.pz, done, [&](auto dd, auto rb) {
    constexpr int DD = decltype(dd)::value, RB = decltype(rb)::value;
    DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd", DD, RB), (k_depth_fwd<DD, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps<RB>(host_kern_z, c.pz, false), pot, loss_tiles);
  });
  if (rc != DPC_OK) return rc;
  if (!done)  // other depths / longer kernels: same arithmetic, column re-read from global
    DPC_LAUNCH("k_depth_fwd", dpc_kid("k_depth_fwd_dyn"), k_depth_fwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s,
               make_taps_dyn(host_kern_z, p->taps_z, false), pot, loss_tiles);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  if (!gt_depth) return DPC_OK;
  return launch_tile_loss_finalize(p, loss_tiles, 0.5f * c.inv_S, weights, loss, st);
}

int dpc_depth_loss_bwd(const DpcParams* p, const float* grid_wh, const float* s, const float* host_kern_z, const float* gt_depth,
                       int gt_factor, float max_dataset_depth, const float* weights, const float* dloss, const float* ddepth,
                       float* dgrid_wh, float* ds, void* workspace, void* stream) {
  if (p && !gt_depth && !ddepth) return DPC_ERR_SHAPE;   // no gradient arrives anywhere
  ColumnCall c;
  int rc = column_check(p, grid_wh, host_kern_z, gt_depth, false, gt_factor, c);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!dgrid_wh || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  const ColumnWorkspace w = column_workspace(p, workspace);
  const DepthPot pot{gt_depth, gt_factor, max_dataset_depth, weights, c.inv_S, nullptr, dloss, ddepth};
  const dim3 gcol(col_tiles(p) * p->B);
  bool done;
  rc = column_dispatch(p, c.pz, done, [&](auto dd, auto rb) {
    constexpr int DD = decltype(dd)::value, RB = decltype(rb)::value;
    DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd", DD, RB), (k_depth_bwd<DD, RB>), gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps,
               grid_wh, s, make_taps<RB>(host_kern_z, c.pz, false), make_taps<RB>(host_kern_z, c.pz, true), pot, dgrid_wh, w.ds_part,
               w.ds_count, ds);
  });
  if (rc != DPC_OK) return rc;
  if (!done) {
    if (!may_need_dv(p)) return DPC_ERR_TAPS;   // cannot happen: a kernel of <= 31 taps has a compiled window
    DPC_LAUNCH("k_depth_bwd", dpc_kid("k_depth_bwd_dyn"), k_depth_bwd_dyn, gcol, dim3(kColThreads), 0, st, *p, c.rh, c.e_eps, grid_wh, s,
               make_taps_dyn(host_kern_z, p->taps_z, false), pot, dgrid_wh, w.dv, w.ds_part, w.ds_count, ds);
  }
  return launch_ok();
}

}  // extern "C"
