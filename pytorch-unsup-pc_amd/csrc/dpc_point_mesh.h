// What the brute-force "every point of a row meets every face of its mesh" pipelines share -- dpc_point_mesh.hip (the
// distance), dpc_closest.hip (the nearest face, the closest point, its weights and the face normal), dpc_winding.hip
// (the winding number of points and of grid nodes) and dpc_raycast.hip (the first hit and the hit count of rays, whose
// origins are "the points").  One decomposition: a work item is (row, block of points, chunk of
// faces), a lane owns a point, the workgroup stages a tile of faces in LDS and every lane walks it.
//   host     pm_check, pm_geometry (pm_chunk: the chunk-size rule), pm_slots and pm_plan (the checks of an entry point
//            with workspace slots; empty_ok: rows with points and no faces pass, for the rays, which then all miss), PmWork / pm_carve (the prefix arrays of the workspace), pm_dispatch (the dtypes)
//   device   pm_row (the checked table row), k_pm_scan (the prefixes), pm_item (the prologue of a work item), pm_walk (the
//            tile loop with its barriers), pm_fetch (a face's checked indices and widened vertices), pm_slot (the guarded
//            slot index), pm_out (the prologue of an output point), pm_report (the status word)
//   faces    pm_stage forms the distance's record of a face once, pm_d2 is the squared distance from a point to a staged
//            face: the distance and the closest kernels inline the same two, so they compute the same d2 for the same
//            (point, face).  The winding's record and term are in dpc_winding.hip, the ray's in dpc_raycast.hip.
//            pm_normal is the unit normal of a face in the caller's winding, which closest and raycast report.
// The contract is in include/dpc_render.h (dpc_point_mesh_distance); the formulation is described at the head of
// dpc_point_mesh.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"

namespace {

constexpr int kPmBlock = DPC_PM_BLOCK;
constexpr int kPmTile = DPC_PM_FACE_TILE;
constexpr int kPmRec = 12;                  // double2 per staged face
constexpr int64_t kPmFill = 8 * 256;        // workgroups a call should have at least: 8 per CU
static_assert(kPmTile <= kPmBlock, "a lane stages at most one face per round");
static_assert(kPmBlock % 64 == 0 && kPmTile * kPmRec * 16 <= 64 * 1024, "whole waves; the tile fits the default LDS limit");

__host__ __device__ inline int pm_blocks(int np) { return (np + kPmBlock - 1) / kPmBlock; }
__host__ __device__ inline int pm_chunks(int np, int nf, int chunk) { return np > 0 ? (nf + chunk - 1) / chunk : 0; }

struct PmGeom {
  int64_t blocks, work, points;
  int chunk;
};

// Faces per chunk for `blocks` > 0 blocks of points and a largest face range of max_nf: one chunk per row when the point
// blocks alone fill the device, else the largest face range is cut into as many chunks as it takes to reach kPmFill
// workgroups, each a whole number of tiles and at least DPC_PM_CHUNK_TILES.
inline int pm_chunk(int64_t blocks, int max_nf) {
  const int64_t want = (kPmFill + blocks - 1) / blocks;
  const int64_t per = (max_nf + want - 1) / want;
  const int64_t tiles = (per + kPmTile - 1) / kPmTile;
  return kPmTile * (int)(tiles > DPC_PM_CHUNK_TILES ? tiles : DPC_PM_CHUNK_TILES);   // <= max_nf + kPmTile: fits an int
}

inline PmGeom pm_geometry(int pairs, const int32_t* desc) {
  PmGeom g{0, 0, 0, kPmTile * DPC_PM_CHUNK_TILES};
  int max_nf = 0;
  for (int p = 0; p < pairs; ++p) {
    const int np = desc[6 * p + 1], nf = desc[6 * p + 5];
    g.blocks += pm_blocks(np);
    g.points += np;
    if (np > 0 && nf > max_nf) max_nf = nf;
  }
  if (g.blocks > 0) g.chunk = pm_chunk(g.blocks, max_nf);
  for (int p = 0; p < pairs; ++p)
    g.work += (int64_t)pm_blocks(desc[6 * p + 1]) * pm_chunks(desc[6 * p + 1], desc[6 * p + 5], g.chunk);
  return g;
}

// workspace slots of a host table that pm_check has accepted: a row has chunks * points of them
inline int64_t pm_slots(int pairs, const int32_t* desc, int chunk) {
  int64_t n = 0;
  for (int p = 0; p < pairs; ++p) n += (int64_t)desc[6 * p + 1] * pm_chunks(desc[6 * p + 1], desc[6 * p + 5], chunk);
  return n;
}

// The prefix arrays at the head of an entry point's workspace, which k_pm_scan builds.
struct PmWork {
  int32_t* work;   // [pairs + 1] exclusive prefix of work items
  int32_t* out;    // [pairs + 1] exclusive prefix of output points
  int32_t* slot;   // [pairs + 1] exclusive prefix of workspace slots; nullptr for an entry point without slots
};

template <int SLOTS>
inline PmWork pm_carve(Carver& c, int pairs) {
  PmWork w{c.take<int32_t>((size_t)pairs + 1), c.take<int32_t>((size_t)pairs + 1), nullptr};
  if (SLOTS) w.slot = c.take<int32_t>((size_t)pairs + 1);
  return w;
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

constexpr int kPmScanThreads = 1024;

// One block: checks the device table's rows (a row outside the packed arrays sets DPC_STATUS_BAD_INDEX and counts nothing)
// and builds the per-row exclusive prefixes, [pairs + 1] each, of work items and of output points; with SLOTS also of
// workspace slots, chunks * points per row (dpc_closest.hip, dpc_winding.hip).
template <int SLOTS>
__global__ __launch_bounds__(kPmScanThreads) void k_pm_scan(const int32_t* __restrict__ desc, int pairs, int n_pts, int n_verts,
                                                            int n_faces, int chunk, int32_t* __restrict__ work,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ slot,
                                                            int32_t* __restrict__ status) {
  constexpr int N = SLOTS ? 3 : 2;
  __shared__ int32_t scratch[kPmScanThreads / 64 + 1];
  const int t = threadIdx.x;
  const int seg = (pairs + kPmScanThreads - 1) / kPmScanThreads;
  const int p0 = min(pairs, t * seg), p1 = min(pairs, p0 + seg);
  int32_t loc[3] = {0, 0, 0};
  bool bad = false;
  for (int p = p0; p < p1; ++p) {
    PmRow r;
    if (pm_row(desc, p, n_pts, n_verts, n_faces, &r)) {
      const int nc = pm_chunks(r.np, r.nf, chunk);
      loc[0] += pm_blocks(r.np) * nc;
      loc[1] += r.np;
      loc[2] += r.np * nc;
    } else {
      bad = true;
    }
  }
  if (bad && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
  int32_t run[3] = {0, 0, 0}, total[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < N; ++k) total[k] = block_scan<kPmScanThreads>(loc[k], &run[k], scratch);
  for (int p = p0; p < p1; ++p) {
    work[p] = run[0]; out[p] = run[1];
    if (SLOTS) slot[p] = run[2];
    PmRow r;
    if (pm_row(desc, p, n_pts, n_verts, n_faces, &r)) {
      const int nc = pm_chunks(r.np, r.nf, chunk);
      run[0] += pm_blocks(r.np) * nc;
      run[1] += r.np;
      run[2] += r.np * nc;
    }
  }
  if (t == 0) {
    work[pairs] = total[0]; out[pairs] = total[1];
    if (SLOTS) slot[pairs] = total[2];
  }
}

__device__ inline double pm_dot(double ax, double ay, double az, double bx, double by, double bz) { return ax * bx + ay * by + az * bz; }
__device__ inline double pm_clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }   // a NaN gives 0

constexpr int kPmBadIndex = 1, kPmNonFinite = 2;

__device__ inline void pm_report(int flags, int32_t* status) {
  if (flags && status) atomicOr(status, (flags & kPmBadIndex ? (int)DPC_STATUS_BAD_INDEX : 0) | (flags & kPmNonFinite ? (int)DPC_STATUS_NONFINITE : 0));
}

// What a lane of a work item (row, block of points, chunk of faces) knows before it meets a face.
struct PmItem {
  PmRow r;
  int p, i, c;          // the row, the lane's point of it, the chunk
  int f0, f1;           // the chunk's faces
  bool live, finite;    // the point exists; its coordinates are usable
  double px, py, pz;    // the point, widened; zeros unless live and finite
  int flags;
};

// The prologue of a work-item kernel: finds the block's item by binary search in the work prefix and loads the lane's
// point.  False where the whole workgroup has nothing to do: past the last item, or in a row outside the packed arrays.
template <int PF64>
__device__ inline bool pm_item(const void* __restrict__ pts_, int n_pts, int n_verts, int n_faces, const int32_t* __restrict__ desc,
                               int pairs, int chunk, const PmWork& pre, PmItem* it) {
  using T = std::conditional_t<PF64 != 0, double, float>;
  const int item = blockIdx.x;
  if (item >= pre.work[pairs]) return false;
  const int p = owner(pre.work, pairs, item);
  PmRow r;
  if (!pm_row(desc, p, n_pts, n_verts, n_faces, &r)) return false;   // k_pm_scan has reported it
  const int nb = pm_blocks(r.np), nc = pm_chunks(r.np, r.nf, chunk);
  const int local = item - pre.work[p];
  if (local < 0 || (int64_t)local >= (int64_t)nb * nc) return false;
  const int b = local % nb, c = local / nb;   // the point blocks of one chunk are adjacent: they read the same faces
  const int i = b * kPmBlock + threadIdx.x;
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
  *it = PmItem{r, p, i, c, f0, f1, live, finite, px, py, pz, flags};
  return true;
}

// The walk over faces f0 .. f1 - 1 in tiles of kPmTile records of REC double2 each.  Per tile, lane t < n stages face
// base + t: stage(face, rec) writes the record and returns the face's flags, which are or-ed into *flags; then every lane
// calls visit(face, rec) for the tile's faces in ascending order -- all lanes read the same record, an LDS broadcast.
// Every thread of the workgroup calls it with the same (f0, f1): barriers inside.
template <int REC, class Stage, class Visit>
__device__ __forceinline__ void pm_walk(int f0, int f1, double2* tile, int* flags, Stage stage, Visit visit) {
  const int t = threadIdx.x;
  for (int base = f0; base < f1; base += kPmTile) {   // the same trip count in every thread
    const int n = f1 - base < kPmTile ? f1 - base : kPmTile;
    __syncthreads();
    if (t < n) *flags |= stage(base + t, tile + t * REC);
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < n; ++k) visit(base + k, tile + k * REC);
  }
}

// The workspace slot [chunk c][point i] of row p, whose np points the caller has checked; -1 when it does not lie inside
// the n_slots the host has carved.
__device__ inline int64_t pm_slot(const PmWork& pre, int p, int np, int c, int i, int n_slots) {
  const int64_t s = (int64_t)pre.slot[p] + (int64_t)c * np + i;
  return s >= 0 && s < n_slots ? s : -1;
}

constexpr int kPmOutBlock = 256;

struct PmOut {
  PmRow r;
  int o, p, i, nc;   // the output point, its row, its index in the row, the row's chunks
};

// The prologue of a kernel with one lane of kPmOutBlock per output point: false for a lane without one.
__device__ inline bool pm_out(int n_pts, int n_verts, int n_faces, const int32_t* __restrict__ desc, int pairs, int chunk,
                              const PmWork& pre, int n_out, PmOut* q) {
  const int64_t o64 = (int64_t)blockIdx.x * kPmOutBlock + threadIdx.x;
  if (o64 >= n_out || o64 >= pre.out[pairs]) return false;
  q->o = (int)o64;
  q->p = owner(pre.out, pairs, q->o);
  if (!pm_row(desc, q->p, n_pts, n_verts, n_faces, &q->r)) return false;
  q->i = q->o - pre.out[q->p];
  if (q->i < 0 || q->i >= q->r.np) return false;
  q->nc = pm_chunks(q->r.np, q->r.nf, chunk);   // <= nf
  return true;
}

// The caller's three vertices of face i of the row, widened, in v; returns the flags of the face.  A face that is skipped
// (v is then not to be used) is staged as NaNs in rec[0 .. REC).  An index outside the mesh never becomes an address.
template <int VF64, int REC>
__device__ inline int pm_fetch(const void* __restrict__ verts_, const int32_t* __restrict__ faces, const PmRow& r, int i,
                               double (&v)[3][3], double2* rec) {
  using T = std::conditional_t<VF64 != 0, double, float>;
  const T* __restrict__ verts = static_cast<const T*>(verts_);
  const int32_t* f = faces + 3 * ((size_t)r.fs + i);
  const int idx[3] = {f[0], f[1], f[2]};
  int flags = 0;
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
    for (int j = 0; j < REC; ++j) rec[j] = make_double2(nan, nan);
  }
  return flags;
}

// The distance's record rec[0 .. kPmRec) of a face with the finite vertices v.  rot (optional): which of the caller's
// three vertices became A -- the staged (A, B, C) are the caller's vertices (rot, rot + 1, rot + 2) mod 3.
__device__ inline void pm_record(const double (&v)[3][3], double2* rec, int* rot = nullptr) {
  // the longest edge goes opposite A; the first of equals in the order (12, 20, 01)
  double l[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i0 = (k + 1) % 3, i1 = (k + 2) % 3;   // l[k]: the edge opposite vertex k
    l[k] = pm_dot(v[i1][0] - v[i0][0], v[i1][1] - v[i0][1], v[i1][2] - v[i0][2], v[i1][0] - v[i0][0], v[i1][1] - v[i0][1],
                  v[i1][2] - v[i0][2]);
  }
  const int ia = (l[0] >= l[1] && l[0] >= l[2]) ? 0 : (l[1] >= l[2] ? 1 : 2);
  if (rot) *rot = ia;
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
}

// Stages face i of the row into rec[0 .. kPmRec); returns the flags of the face (pm_fetch's rules).
template <int VF64>
__device__ inline int pm_stage(const void* __restrict__ verts, const int32_t* __restrict__ faces, const PmRow& r, int i, double2* rec) {
  double v[3][3];
  const int flags = pm_fetch<VF64, kPmRec>(verts, faces, r, i, v, rec);
  if (!flags) pm_record(v, rec);
  return flags;
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

// The unit normal of (v0, v1, v2) in that winding, (v1 - v0) x (v2 - v0) over its length, each operation rounded on its
// own as numpy's elementwise arithmetic rounds it (nothing fused: a contracted cross product of a sliver differs from the
// plain one by far more than an ulp); zeros when the cross product has no length.
__device__ inline void pm_normal(const double (&v)[3][3], double* n) {
#pragma clang fp contract(off)
  const double ax = v[1][0] - v[0][0], ay = v[1][1] - v[0][1], az = v[1][2] - v[0][2];
  const double bx = v[2][0] - v[0][0], by = v[2][1] - v[0][1], bz = v[2][2] - v[0][2];
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double len = sqrt((cx * cx + cy * cy) + cz * cz);
  const bool area = len > 0.0;
  n[0] = area ? cx / len : 0.0;
  n[1] = area ? cy / len : 0.0;
  n[2] = area ? cz / len : 0.0;
}

// the host check of a pair table: DPC_ERR_SHAPE, or DPC_OK with the number of output points in *total.  empty_ok: a row
// with points and no faces is accepted (an entry point whose answer over an empty set of faces is defined)
inline int pm_check(int pairs, const int32_t* desc, int64_t n_pts, int64_t n_verts, int64_t n_faces, int64_t* total,
                    bool empty_ok = false) {
  const int64_t len[3] = {n_pts, n_verts, n_faces};
  return check_desc<6, 3>(desc, pairs, len, INT32_MAX, total, [empty_ok](const int32_t* d) {
    return empty_ok || !(d[5] == 0 && d[1] > 0);   // the minimum over an empty set of faces
  });
}

// The checks of a pair entry point with workspace slots, and of its workspace size: DPC_OK with the geometry, the slot
// count and the number of output points, or the code to return.  max_faces: the most faces a row may have.
inline int pm_plan(int n_points, int n_verts, int n_faces, const int32_t* host_pair_desc, int n_pairs, int max_faces, PmGeom* g,
                   int64_t* slots, int64_t* total, bool empty_ok = false) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0 || n_pairs < 0) return DPC_ERR_SHAPE;
  *g = PmGeom{0, 0, 0, kPmTile * DPC_PM_CHUNK_TILES};
  *slots = *total = 0;
  if (n_pairs == 0) return DPC_OK;
  if (!host_pair_desc) return DPC_ERR_NULL;
  const int rc = pm_check(n_pairs, host_pair_desc, n_points, n_verts, n_faces, total, empty_ok);
  if (rc != DPC_OK) return rc;
  for (int p = 0; p < n_pairs; ++p)
    if (host_pair_desc[6 * p + 5] > max_faces) return DPC_ERR_SHAPE;
  *g = pm_geometry(n_pairs, host_pair_desc);
  *slots = pm_slots(n_pairs, host_pair_desc, g->chunk);
  return g->work > INT32_MAX || *slots > INT32_MAX ? DPC_ERR_SHAPE : DPC_OK;
}

// f(points are fp64, vertices are fp64) with the two runtime flags as std::integral_constant<int, 0 or 1>
template <class F>
inline int pm_dispatch(int points_f64, int verts_f64, F f) {
  const std::integral_constant<int, 0> no;
  const std::integral_constant<int, 1> yes;
  if (points_f64) return verts_f64 ? f(yes, yes) : f(yes, no);
  return verts_f64 ? f(no, yes) : f(no, no);
}

}  // namespace
