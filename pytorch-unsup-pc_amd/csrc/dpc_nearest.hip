// Nearest target point of every source point: point_cloud_distance (dpc/util/point_cloud_distance.py:25-40), the
// kernel of the reference's Chamfer evaluation (dpc/run/eval_chamfer_to.py:24-44, 119-123).  SURVEY.md 8(f) rank 4.
//
// The reference materialises [Ns,Nt,3] differences, takes sqrt(sum(diff^2, 2)) and torch.argmin (first minimum) over
// the targets.  Here nothing is materialised: one lane owns one source point, the targets stream through LDS, and the
// targets are also split over blockIdx.y so that small source clouds still fill the chip; a second, tiny kernel merges
// the per-slice winners in slice order.  The scan itself -- the reference's arithmetic op for op in the input's precision,
// and its first-minimum rule including near ties -- is nearest_scan in dpc_nearest.h, shared with the batched Chamfer
// kernels of dpc_chamfer.hip.
// Compute-bound on the fp32 / fp64 vector pipe (about a dozen instructions per pair); HBM traffic is negligible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_nearest.h"
#include "dpc_launch.h"

namespace {

constexpr int kNnThreads = 256;
constexpr int kNnTile = 1024;  // targets staged per LDS tile (12 KiB fp32, 24 KiB fp64)

template <class T>
__global__ __launch_bounds__(kNnThreads) void k_nearest_partial(const T* __restrict__ vs, const T* __restrict__ vt, int ns,
                                                                int nt, int slice, T* __restrict__ part_dist,
                                                                int* __restrict__ part_idx) {
  __shared__ T tx[kNnTile], ty[kNnTile], tz[kNnTile];
  const int i = blockIdx.x * kNnThreads + threadIdx.x;
  const bool live = i < ns;
  const int j0 = blockIdx.y * slice, j1 = min(nt, j0 + slice);
  T sx = 0, sy = 0, sz = 0;
  if (live) {
    sx = vs[3 * (size_t)i + 0]; sy = vs[3 * (size_t)i + 1]; sz = vs[3 * (size_t)i + 2];
  }
  T best_d2;
  int best;
  nearest_scan<T, kNnThreads, kNnTile>(vt, j0, j1, sx, sy, sz, tx, ty, tz, best_d2, best);
  if (live) {
    part_dist[(size_t)blockIdx.y * ns + i] = sqrt(best_d2);
    part_idx[(size_t)blockIdx.y * ns + i] = best;
  }
}

template <class T>
__global__ __launch_bounds__(kNnThreads) void k_nearest_merge(const T* __restrict__ vt, int ns, int nslice,
                                                              const T* __restrict__ part_dist,
                                                              const int* __restrict__ part_idx, T* __restrict__ proj,
                                                              T* __restrict__ min_dist, int64_t* __restrict__ idx) {
  const int i = blockIdx.x * kNnThreads + threadIdx.x;
  if (i >= ns) return;
  T best_dist = part_dist[i];
  int best = part_idx[i];
  for (int s = 1; s < nslice; ++s) {  // slices hold increasing target indices: strict < keeps the first minimum
    const T d = part_dist[(size_t)s * ns + i];
    if (d < best_dist) {
      best_dist = d; best = part_idx[(size_t)s * ns + i];
    }
  }
  if (min_dist != nullptr) min_dist[i] = best_dist;
  if (idx != nullptr) idx[i] = best;
  if (proj != nullptr) {
    const T* p = vt + 3 * (size_t)best;
    proj[3 * (size_t)i + 0] = p[0]; proj[3 * (size_t)i + 1] = p[1]; proj[3 * (size_t)i + 2] = p[2];
  }
}

// targets per slice (nearest_slice in dpc_nearest.h); returns the number of slices
int nearest_slices(int ns, int nt, int* slice_out) {
  const int64_t slice = nearest_slice((ns + (int64_t)kNnThreads - 1) / kNnThreads, nt);
  *slice_out = (int)slice;
  return (int)((nt + slice - 1) / slice);
}

template <class T>
int nearest_impl(const T* vs, const T* vt, int ns, int nt, T* proj, T* min_dist, int64_t* idx, void* workspace,
                 hipStream_t st) {
  int slice;
  const int nslice = nearest_slices(ns, nt, &slice);
  T* part_dist = static_cast<T*>(workspace);
  int* part_idx = reinterpret_cast<int*>(part_dist + (size_t)nslice * ns);
  const dim3 grid((ns + kNnThreads - 1) / kNnThreads, nslice);
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  DPC_LAUNCH("k_nearest_partial", dpc_kid(kIsF64 ? "k_nearest_partial<double>" : "k_nearest_partial<float>"), k_nearest_partial<T>, grid, dim3(kNnThreads), 0, st, vs, vt, ns, nt, slice, part_dist, part_idx);
  DPC_LAUNCH("k_nearest_merge", dpc_kid(kIsF64 ? "k_nearest_merge<double>" : "k_nearest_merge<float>"), k_nearest_merge<T>, dim3(grid.x), dim3(kNnThreads), 0, st, vt, ns, nslice,
             (const T*)part_dist, (const int*)part_idx, proj, min_dist, idx);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_nearest_workspace_bytes(int ns, int nt, int is_f64) {
  if (ns <= 0 || nt <= 0) return 0;
  int slice;
  const size_t nslice = (size_t)nearest_slices(ns, nt, &slice);
  return nslice * (size_t)ns * ((is_f64 ? 8 : 4) + 4) + 16;
}

int dpc_point_cloud_distance(const void* vs, const void* vt, int ns, int nt, int is_f64, void* proj, void* min_dist,
                             int64_t* idx, void* workspace, void* stream) {
  if (ns < 0 || nt < 0) return DPC_ERR_SHAPE;
  if (ns == 0) return DPC_OK;
  if (nt == 0) return DPC_ERR_SHAPE;  // argmin over an empty set: the reference raises as well
  if (!vs || !vt || !workspace) return DPC_ERR_NULL;
  if (is_f64)
    return nearest_impl<double>(static_cast<const double*>(vs), static_cast<const double*>(vt), ns, nt,
                                static_cast<double*>(proj), static_cast<double*>(min_dist), idx, workspace, (hipStream_t)stream);
  return nearest_impl<float>(static_cast<const float*>(vs), static_cast<const float*>(vt), ns, nt,
                             static_cast<float*>(proj), static_cast<float*>(min_dist), idx, workspace, (hipStream_t)stream);
}

}  // extern "C"
