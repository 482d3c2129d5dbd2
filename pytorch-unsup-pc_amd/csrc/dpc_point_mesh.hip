// Exact point-to-mesh distance: the squared Euclidean distance from every point of a row to the nearest point of the
// union of the row's triangles, for a ragged batch of (cloud, mesh) rows in one call.  The contract (the rules for
// zero-area and non-finite faces, the table, the guards) is in include/dpc_render.h (dpc_point_mesh_distance); all
// arithmetic is fp64, fp32 inputs widen exactly first.  Brute force: every point of a row meets every face of it.
//
// k_pm_scan   one block: checks the device table's rows and builds the per-row prefixes of work items and output points.
// k_pm_fill   d2 = +inf everywhere.
// k_pm_dist<fp64 points, fp64 vertices>   one workgroup of DPC_PM_BLOCK lanes per work item (row, block of points, chunk
//     of faces), found by binary search in the work prefix; a lane owns one point.  Per round the workgroup stages
//     DPC_PM_FACE_TILE faces in LDS, one lane per face: the vertices rotated so that the longest edge lies opposite
//     vertex A (the normal then comes from the two shortest edges), A, the edges E0 = B - A, E1 = C - A, E2 = C - B, the
//     normal N = E0 x E1, and the quotients a lane would otherwise form per face (1 / N.N, the Gram entries over N.N,
//     the reciprocal edge lengths squared): 22 doubles, computed once per face.  Then every lane walks the tile; all lanes
//     read the same record, an LDS broadcast.  Per face and point, branch-free:
//         D = P - A, d0 = D.E0, d1 = D.E1
//         s = (c d0 - b d1) / N.N, t = (a d1 - b d0) / N.N      barycentric coordinates of the plane foot point
//         inside = s >= 0 && t >= 0 && s + t <= 1              false for a zero-area face, whose quotients are NaN
//         plane  = (D.N)^2 / N.N
//         edge_k = |R - clamp(R.E / E.E, 0, 1) E|^2             for (R, E) = (D, E0), (D, E1), (D - E0, E2)
//         d2     = inside ? plane : min(edge_0, edge_1, edge_2)
//     80 fp64 operations (an fma counted as two, a min / max as one, compares and selects not counted).  A skipped face is
//     staged as NaNs, which the running fmin drops.  The lane's minimum over its chunk goes to d2 with one 64-bit unsigned
//     atomic min: a non-negative double orders like its bit pattern, min is exact and order-free, so the result does not
//     depend on how the faces were split or on which workgroup arrives first.
// A row with few points and many faces is split over chunks of faces so that the call fills the device (pm_geometry).
// The decomposition is dpc_point_mesh.h's, which dpc_closest.hip and dpc_winding.hip use through pm_item (the prologue)
// and pm_walk (the tile loop).  k_pm_dist keeps both written out, to be kept in step with them: over the two helpers it
// came out at 80 VGPRs for 81, so 6 waves per SIMD for 5, and 0.9 to 1.3 % slower on large batches (LAB_NOTES.md, 21).
// Every index is checked against the device table before it becomes an address; every loop is bounded by a checked count.
#include <hip/hip_runtime.h>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_point_mesh.h"
#include "dpc_launch.h"

namespace {

size_t pm_workspace(int pairs, char* base, PmWork* w) {
  Carver c{base};
  const PmWork t = pm_carve<0>(c, pairs);
  if (w) *w = t;
  return c.off + 16;
}

__global__ __launch_bounds__(256) void k_pm_fill(double* __restrict__ d2, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) d2[i] = std::numeric_limits<double>::infinity();
}

template <int PF64, int VF64>
__global__ __launch_bounds__(kPmBlock) void k_pm_dist(const void* __restrict__ pts_, int n_pts, const void* __restrict__ verts,
                                                      int n_verts, const int32_t* __restrict__ faces, int n_faces,
                                                      const int32_t* __restrict__ desc, int pairs, int chunk, PmWork pre, int n_out,
                                                      double* __restrict__ d2, int32_t* __restrict__ status) {
  using T = std::conditional_t<PF64 != 0, double, float>;
  __shared__ double2 tile[kPmTile * kPmRec];
  const int t = threadIdx.x;
  const int item = blockIdx.x;
  if (item >= pre.work[pairs]) return;
  const int p = owner(pre.work, pairs, item);
  PmRow r;
  if (!pm_row(desc, p, n_pts, n_verts, n_faces, &r)) return;   // k_pm_scan has reported it
  const int nb = pm_blocks(r.np), nc = pm_chunks(r.np, r.nf, chunk);
  const int local = item - pre.work[p];
  if (local < 0 || (int64_t)local >= (int64_t)nb * nc) return;
  const int b = local % nb, c = local / nb;   // the point blocks of one chunk are adjacent: they read the same faces
  const int i = b * kPmBlock + t;
  const bool live = i < r.np;
  const int f0 = c * chunk;                                    // < nf
  const int f1 = r.nf - f0 < chunk ? r.nf : f0 + chunk;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) {
    const T* q = static_cast<const T*>(pts_) + 3 * ((size_t)r.ps + i);
    px = (double)q[0]; py = (double)q[1]; pz = (double)q[2];
  }
  int flags = 0;
  const bool finite = fabs(px) < DPC_MESH_VOXEL_MAX_COORD && fabs(py) < DPC_MESH_VOXEL_MAX_COORD && fabs(pz) < DPC_MESH_VOXEL_MAX_COORD;
  if (!finite) {
    flags = kPmNonFinite;
    px = py = pz = 0.0;
  }
  double best = std::numeric_limits<double>::infinity();
  for (int base = f0; base < f1; base += kPmTile) {   // the same trip count in every thread: barriers inside
    const int n = f1 - base < kPmTile ? f1 - base : kPmTile;
    __syncthreads();
    if (t < n) flags |= pm_stage<VF64>(verts, faces, r, base + t, tile + t * kPmRec);
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < n; ++k) best = fmin(best, pm_d2(tile + k * kPmRec, px, py, pz));
  }
  if (!finite) best = std::numeric_limits<double>::infinity();
  const int o = pre.out[p] + i;
  if (live && (unsigned)o < (unsigned)n_out)
    atomicMin(reinterpret_cast<unsigned long long*>(d2 + o), (unsigned long long)__double_as_longlong(best));
  pm_report(flags, status);
}

template <int PF64, int VF64>
int pm_launch(const void* pts, int n_pts, const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc,
              int pairs, const PmGeom& g, const PmWork& w, double* d2, int32_t* status, hipStream_t st) {
  DPC_LAUNCH("k_pm_dist", dpc_kid("k_pm_dist", PF64, VF64), (k_pm_dist<PF64, VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, pts,
             n_pts, verts, n_verts, faces, n_faces, desc, pairs, g.chunk, w, (int)g.points, d2, status);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_point_mesh_workspace_bytes(int n_pairs) { return n_pairs > 0 ? pm_workspace(n_pairs, nullptr, nullptr) : 0; }

int dpc_point_mesh_distance(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                            const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                            double* d2, void* workspace, int32_t* status, void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0 || n_pairs < 0) return DPC_ERR_SHAPE;
  if (n_pairs == 0) return DPC_OK;
  if (!host_pair_desc) return DPC_ERR_NULL;
  int64_t total = 0;
  const int rc = pm_check(n_pairs, host_pair_desc, n_points, n_verts, n_faces, &total);
  if (rc != DPC_OK) return rc;
  const PmGeom g = pm_geometry(n_pairs, host_pair_desc);
  if (g.work > INT32_MAX) return DPC_ERR_SHAPE;
  if (total == 0) return DPC_OK;
  if (!points || !verts || !faces || !pair_desc || !d2 || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  PmWork w;
  pm_workspace(n_pairs, static_cast<char*>(workspace), &w);
  DPC_LAUNCH("k_pm_scan", dpc_kid("k_pm_scan", 0), (k_pm_scan<0>), dim3(1), dim3(kPmScanThreads), 0, st, pair_desc, n_pairs, n_points,
             n_verts, n_faces, g.chunk, w.work, w.out, w.slot, status);
  DPC_LAUNCH("k_pm_fill", dpc_kid("k_pm_fill"), k_pm_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d2, (int)total);
  return pm_dispatch(points_f64, verts_f64, [&](auto pf, auto vf) {
    return pm_launch<decltype(pf)::value, decltype(vf)::value>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w,
                                                               d2, status, st);
  });
}

}  // extern "C"
