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
// Every index is checked against the device table before it becomes an address; every loop is bounded by a checked count.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_profile.h"

namespace {

constexpr int kPmBlock = DPC_PM_BLOCK;
constexpr int kPmTile = DPC_PM_FACE_TILE;
constexpr int kPmRec = 12;                  // double2 per staged face
constexpr int kPmScanThreads = 1024;
constexpr int64_t kPmFill = 8 * 256;        // workgroups a call should have at least: 8 per CU
static_assert(kPmTile <= kPmBlock, "a lane stages at most one face per round");
static_assert(kPmBlock % 64 == 0 && kPmTile * kPmRec * 16 <= 64 * 1024, "whole waves; the tile fits the default LDS limit");

__host__ __device__ inline int pm_blocks(int np) { return (np + kPmBlock - 1) / kPmBlock; }
__host__ __device__ inline int pm_chunks(int np, int nf, int chunk) { return np > 0 ? (nf + chunk - 1) / chunk : 0; }

struct PmGeom {
  int64_t blocks, work, points;
  int chunk;
};

// Faces per chunk: one chunk per row when the point blocks alone fill the device, else the largest face range is cut into
// as many chunks as it takes to reach kPmFill workgroups, each a whole number of tiles and at least DPC_PM_CHUNK_TILES.
PmGeom pm_geometry(int pairs, const int32_t* desc) {
  PmGeom g{0, 0, 0, kPmTile * DPC_PM_CHUNK_TILES};
  int max_nf = 0;
  for (int p = 0; p < pairs; ++p) {
    const int np = desc[6 * p + 1], nf = desc[6 * p + 5];
    g.blocks += pm_blocks(np);
    g.points += np;
    if (np > 0 && nf > max_nf) max_nf = nf;
  }
  if (g.blocks > 0) {
    const int64_t want = (kPmFill + g.blocks - 1) / g.blocks;
    const int64_t per = (max_nf + want - 1) / want;
    const int64_t tiles = (per + kPmTile - 1) / kPmTile;
    g.chunk = kPmTile * (int)(tiles > DPC_PM_CHUNK_TILES ? tiles : DPC_PM_CHUNK_TILES);   // <= max_nf + kPmTile: fits an int
  }
  for (int p = 0; p < pairs; ++p)
    g.work += (int64_t)pm_blocks(desc[6 * p + 1]) * pm_chunks(desc[6 * p + 1], desc[6 * p + 5], g.chunk);
  return g;
}

struct PmWork {
  int32_t* work;   // [pairs + 1] exclusive prefix of work items
  int32_t* out;    // [pairs + 1] exclusive prefix of output points
};

size_t pm_carve(int pairs, char* base, PmWork* w) {
  Carver c{base};
  PmWork t;
  t.work = c.take<int32_t>((size_t)pairs + 1);
  t.out = c.take<int32_t>((size_t)pairs + 1);
  if (w) *w = t;
  return c.off + 16;
}

struct PmRow {
  int ps, np, vs, nv, fs, nf;
};

// the table row of a pair; false when it does not lie inside the packed arrays (nothing of it is then used)
__device__ inline bool pm_row(const int32_t* __restrict__ desc, int p, int n_pts, int n_verts, int n_faces, PmRow* r) {
  const int32_t* d = desc + 6 * (size_t)p;
  r->ps = d[0]; r->np = d[1]; r->vs = d[2]; r->nv = d[3]; r->fs = d[4]; r->nf = d[5];
  return r->ps >= 0 && r->np >= 0 && (int64_t)r->ps + r->np <= n_pts && r->vs >= 0 && r->nv >= 0 &&
         (int64_t)r->vs + r->nv <= n_verts && r->fs >= 0 && r->nf >= 0 && (int64_t)r->fs + r->nf <= n_faces;
}

__global__ __launch_bounds__(kPmScanThreads) void k_pm_scan(const int32_t* __restrict__ desc, int pairs, int n_pts, int n_verts,
                                                            int n_faces, int chunk, PmWork pre, int32_t* __restrict__ status) {
  __shared__ int32_t scratch[kPmScanThreads / 64 + 1];
  const int t = threadIdx.x;
  const int seg = (pairs + kPmScanThreads - 1) / kPmScanThreads;
  const int p0 = min(pairs, t * seg), p1 = min(pairs, p0 + seg);
  int32_t loc[2] = {0, 0};
  bool bad = false;
  for (int p = p0; p < p1; ++p) {
    PmRow r;
    if (pm_row(desc, p, n_pts, n_verts, n_faces, &r)) {
      loc[0] += pm_blocks(r.np) * pm_chunks(r.np, r.nf, chunk);
      loc[1] += r.np;
    } else {
      bad = true;
    }
  }
  if (bad && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
  int32_t run[2], total[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) total[k] = block_scan<kPmScanThreads>(loc[k], &run[k], scratch);
  for (int p = p0; p < p1; ++p) {
    pre.work[p] = run[0]; pre.out[p] = run[1];
    PmRow r;
    if (pm_row(desc, p, n_pts, n_verts, n_faces, &r)) {
      run[0] += pm_blocks(r.np) * pm_chunks(r.np, r.nf, chunk);
      run[1] += r.np;
    }
  }
  if (t == 0) { pre.work[pairs] = total[0]; pre.out[pairs] = total[1]; }
}

__global__ __launch_bounds__(256) void k_pm_fill(double* __restrict__ d2, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) d2[i] = std::numeric_limits<double>::infinity();
}

__device__ inline double pm_dot(double ax, double ay, double az, double bx, double by, double bz) { return ax * bx + ay * by + az * bz; }
__device__ inline double pm_clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }   // a NaN gives 0

constexpr int kPmBadIndex = 1, kPmNonFinite = 2;

// Stages face i of the row into rec[0 .. kPmRec); returns the flags of the face.  A face that is skipped is staged as
// NaNs.  An index outside the mesh never becomes an address.
template <int VF64>
__device__ inline int pm_stage(const void* __restrict__ verts_, const int32_t* __restrict__ faces, const PmRow& r, int i, double2* rec) {
  using T = std::conditional_t<VF64 != 0, double, float>;
  const T* __restrict__ verts = static_cast<const T*>(verts_);
  const int32_t* f = faces + 3 * ((size_t)r.fs + i);
  const int idx[3] = {f[0], f[1], f[2]};
  int flags = 0;
  double v[3][3];
  if ((unsigned)idx[0] >= (unsigned)r.nv || (unsigned)idx[1] >= (unsigned)r.nv || (unsigned)idx[2] >= (unsigned)r.nv) {
    flags = kPmBadIndex;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const T* q = verts + 3 * ((size_t)r.vs + idx[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[k][c] = (double)q[c];
        if (!(fabs(v[k][c]) < DPC_MESH_VOXEL_MAX_COORD)) flags = kPmNonFinite;   // a NaN too
      }
    }
  }
  if (flags) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
#pragma unroll
    for (int j = 0; j < kPmRec; ++j) rec[j] = make_double2(nan, nan);
    return flags;
  }
  // the longest edge goes opposite A; the first of equals in the order (12, 20, 01)
  double l[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i0 = (k + 1) % 3, i1 = (k + 2) % 3;   // l[k]: the edge opposite vertex k
    l[k] = pm_dot(v[i1][0] - v[i0][0], v[i1][1] - v[i0][1], v[i1][2] - v[i0][2], v[i1][0] - v[i0][0], v[i1][1] - v[i0][1],
                  v[i1][2] - v[i0][2]);
  }
  const int ia = (l[0] >= l[1] && l[0] >= l[2]) ? 0 : (l[1] >= l[2] ? 1 : 2);
  double A[3], B[3], C[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A[c] = ia == 0 ? v[0][c] : ia == 1 ? v[1][c] : v[2][c];
    B[c] = ia == 0 ? v[1][c] : ia == 1 ? v[2][c] : v[0][c];
    C[c] = ia == 0 ? v[2][c] : ia == 1 ? v[0][c] : v[1][c];
  }
  double E0[3], E1[3], E2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { E0[c] = B[c] - A[c]; E1[c] = C[c] - A[c]; E2[c] = C[c] - B[c]; }
  const double a = pm_dot(E0[0], E0[1], E0[2], E0[0], E0[1], E0[2]);
  const double b = pm_dot(E0[0], E0[1], E0[2], E1[0], E1[1], E1[2]);
  const double c = pm_dot(E1[0], E1[1], E1[2], E1[0], E1[1], E1[2]);
  const double e = pm_dot(E2[0], E2[1], E2[2], E2[0], E2[1], E2[2]);
  const double N[3] = {E0[1] * E1[2] - E0[2] * E1[1], E0[2] * E1[0] - E0[0] * E1[2], E0[0] * E1[1] - E0[1] * E1[0]};
  const double nn = pm_dot(N[0], N[1], N[2], N[0], N[1], N[2]);   // the determinant a c - b^2, without its cancellation
  const bool area = nn > 0.0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  rec[0] = make_double2(A[0], A[1]);
  rec[1] = make_double2(A[2], E0[0]);
  rec[2] = make_double2(E0[1], E0[2]);
  rec[3] = make_double2(E1[0], E1[1]);
  rec[4] = make_double2(E1[2], E2[0]);
  rec[5] = make_double2(E2[1], E2[2]);
  rec[6] = make_double2(N[0], N[1]);
  rec[7] = make_double2(N[2], area ? 1.0 / nn : 0.0);
  rec[8] = make_double2(area ? c / nn : nan, area ? b / nn : nan);
  rec[9] = make_double2(area ? a / nn : nan, a > 0.0 ? 1.0 / a : 0.0);
  rec[10] = make_double2(c > 0.0 ? 1.0 / c : 0.0, e > 0.0 ? 1.0 / e : 0.0);
  rec[11] = make_double2(0.0, 0.0);
  return 0;
}

// the squared distance from P to the staged face
__device__ inline double pm_d2(const double2* __restrict__ rec, double px, double py, double pz) {
  const double2 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4], q5 = rec[5], q6 = rec[6], q7 = rec[7], q8 = rec[8],
                q9 = rec[9], q10 = rec[10];
  const double dx = px - q0.x, dy = py - q0.y, dz = pz - q1.x;
  const double e0x = q1.y, e0y = q2.x, e0z = q2.y, e1x = q3.x, e1y = q3.y, e1z = q4.x, e2x = q4.y, e2y = q5.x, e2z = q5.y;
  const double d0 = pm_dot(dx, dy, dz, e0x, e0y, e0z), d1 = pm_dot(dx, dy, dz, e1x, e1y, e1z);
  const double s = q8.x * d0 - q8.y * d1, t = q9.x * d1 - q8.y * d0;
  const bool inside = s >= 0.0 && t >= 0.0 && s + t <= 1.0;
  const double dn = pm_dot(dx, dy, dz, q6.x, q6.y, q7.x);
  const double plane = dn * dn * q7.y;
  const double t0 = pm_clamp01(d0 * q9.y);
  const double r0x = dx - t0 * e0x, r0y = dy - t0 * e0y, r0z = dz - t0 * e0z;
  const double t1 = pm_clamp01(d1 * q10.x);
  const double r1x = dx - t1 * e1x, r1y = dy - t1 * e1y, r1z = dz - t1 * e1z;
  const double gx = dx - e0x, gy = dy - e0y, gz = dz - e0z;
  const double t2 = pm_clamp01(pm_dot(gx, gy, gz, e2x, e2y, e2z) * q10.y);
  const double r2x = gx - t2 * e2x, r2y = gy - t2 * e2y, r2z = gz - t2 * e2z;
  const double edge = fmin(fmin(pm_dot(r0x, r0y, r0z, r0x, r0y, r0z), pm_dot(r1x, r1y, r1z, r1x, r1y, r1z)),
                           pm_dot(r2x, r2y, r2z, r2x, r2y, r2z));
  return inside ? plane : edge;
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
  if (flags && status) atomicOr(status, (flags & kPmBadIndex ? (int)DPC_STATUS_BAD_INDEX : 0) | (flags & kPmNonFinite ? (int)DPC_STATUS_NONFINITE : 0));
}

int pm_check(int pairs, const int32_t* desc, int64_t n_pts, int64_t n_verts, int64_t n_faces, int64_t* total) {
  const int64_t len[3] = {n_pts, n_verts, n_faces};
  return check_desc<6, 3>(desc, pairs, len, INT32_MAX, total, [](const int32_t* d) {
    return !(d[5] == 0 && d[1] > 0);   // the minimum over an empty set of faces
  });
}

template <int PF64, int VF64>
int pm_launch(const void* pts, int n_pts, const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc,
              int pairs, const PmGeom& g, const PmWork& w, double* d2, int32_t* status, hipStream_t st) {
  DPC_LAUNCH("k_pm_dist", dpc_kid("k_pm_dist", PF64, VF64), (k_pm_dist<PF64, VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, pts,
             n_pts, verts, n_verts, faces, n_faces, desc, pairs, g.chunk, w, (int)g.points, d2, status);
  return hipGetLastError() == hipSuccess ? DPC_OK : DPC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t dpc_point_mesh_workspace_bytes(int n_pairs) { return n_pairs > 0 ? pm_carve(n_pairs, nullptr, nullptr) : 0; }

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
  pm_carve(n_pairs, static_cast<char*>(workspace), &w);
  DPC_LAUNCH("k_pm_scan", dpc_kid("k_pm_scan"), k_pm_scan, dim3(1), dim3(kPmScanThreads), 0, st, pair_desc, n_pairs, n_points, n_verts,
             n_faces, g.chunk, w, status);
  DPC_LAUNCH("k_pm_fill", dpc_kid("k_pm_fill"), k_pm_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d2, (int)total);
  if (points_f64)
    return verts_f64 ? pm_launch<1, 1>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w, d2, status, st)
                     : pm_launch<1, 0>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w, d2, status, st);
  return verts_f64 ? pm_launch<0, 1>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w, d2, status, st)
                   : pm_launch<0, 0>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w, d2, status, st);
}

}  // extern "C"
