// Generalized winding numbers: w(P) = (1 / 4 pi) sum over the faces of the signed solid angle of the face seen from P, for
// every point of a ragged batch of (cloud, mesh) rows (dpc_mesh_winding) or for the node centres of one grid per mesh
// (dpc_mesh_winding_voxels).  The contract (the rule for one face, the fixed-point sum, the guards) is in
// include/dpc_render.h (dpc_mesh_winding); all arithmetic is fp64, fp32 inputs widen exactly first.  Brute force: every
// point of a row meets every face of it.
//
// k_pm_scan<1>   the distance's scan (dpc_point_mesh.h): checks the device table's rows and builds the per-row prefixes of
//     work items, output points and workspace slots.
// k_wn_sum<fp64 points, fp64 vertices>   k_pm_dist's decomposition, from pm_item, pm_walk and pm_fetch of
//     dpc_point_mesh.h: one workgroup of DPC_PM_BLOCK lanes per work item (row, block of points, chunk of faces), a lane
//     owns one point.  Per round the workgroup stages DPC_PM_FACE_TILE faces in LDS, one lane per face: the three
//     vertices in the caller's order, nine doubles widened once (a skipped face as NaNs, whose term is 0).  Then every
//     lane walks the tile; all lanes read the same record, an LDS broadcast.  Per face and point, branch-free:
//         a = V0 - P, b = V1 - P, c = V2 - P
//         det = a . (b x c),  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|
//         q = det != 0 ? rint(atan2(det, den) / (2 pi) * 2^40) : 0          an int64
//     and the lane adds q to its int64 sum.  The sum of its chunk goes to the workspace slot [chunk][point] of its row,
//     which no other lane writes: there is no atomic, and no slot is read before the kernel has ended.
// k_wn_finish<fp64 points>   one lane per output point: adds the point's slots and writes the sum and w = sum 2^-40 (NaN
//     for a point that is not finite).
// k_wn_vox<fp64 vertices>   the same walk with a lane owning a grid node, whose centre it forms itself: work item (mesh,
//     block of nodes, chunk of faces), slot [mesh][chunk][node].
// k_wn_vox_finish   one lane per node: adds the node's slots, compares with the threshold in integers and packs the
//     wave's 64 answers into two words of the bit grid with a ballot.
// Integer addition is associative, so a result depends on neither the chunk size, nor the batching, nor the order in which
// workgroups run.  Every index is checked against the device table before it becomes an address; every loop is bounded by
// a checked count.
#include <hip/hip_runtime.h>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_point_mesh.h"
#include "dpc_launch.h"
#include "dpc_voxel_bits.h"

namespace {

constexpr int kWnRec = 5;                                  // double2 per staged face: V0, V1, V2 and one pad
constexpr double kWnScale = (double)(1ll << DPC_WINDING_FRAC_BITS);
constexpr int kWnMaxFaces = 1 << 22;                       // |q| <= 2^39: 2^22 terms stay inside an int64
static_assert(DPC_WINDING_FRAC_BITS - 1 + 22 < 63 && DPC_WINDING_FRAC_BITS < 51, "the sum cannot wrap; wn_term's rounding is exact");
static_assert(kPmTile * kWnRec * 16 <= 64 * 1024, "the tile fits the default LDS limit");

struct WnWork : PmWork {   // a row has chunks * points slots
  int64_t* part;           // [slots]
};

size_t wn_carve(int pairs, int64_t slots, char* base, WnWork* w) {
  Carver c{base};
  WnWork t;
  static_cast<PmWork&>(t) = pm_carve<1>(c, pairs);
  t.part = c.take<int64_t>((size_t)slots);
  if (w) *w = t;
  return c.off + 16;
}

// Stages face i of the row into rec[0 .. kWnRec): the caller's three vertices; returns the flags of the face (pm_fetch's
// rules).
template <int VF64>
__device__ inline int wn_stage(const void* __restrict__ verts, const int32_t* __restrict__ faces, const PmRow& r, int i, double2* rec) {
  double v[3][3];
  const int flags = pm_fetch<VF64, kWnRec>(verts, faces, r, i, v, rec);
  if (flags) return flags;
  rec[0] = make_double2(v[0][0], v[0][1]);
  rec[1] = make_double2(v[0][2], v[1][0]);
  rec[2] = make_double2(v[1][1], v[1][2]);
  rec[3] = make_double2(v[2][0], v[2][1]);
  rec[4] = make_double2(v[2][2], 0.0);
  return 0;
}

// the quantised term of the staged face seen from P: rint(Omega / 4 pi * 2^40)
__device__ inline int64_t wn_term(const double2* __restrict__ rec, double px, double py, double pz) {
  const double2 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4];
  const double ax = q0.x - px, ay = q0.y - py, az = q1.x - pz;
  const double bx = q1.y - px, by = q2.x - py, bz = q2.y - pz;
  const double cx = q3.x - px, cy = q3.y - py, cz = q4.x - pz;
  const double la = sqrt(pm_dot(ax, ay, az, ax, ay, az)), lb = sqrt(pm_dot(bx, by, bz, bx, by, bz)),
               lc = sqrt(pm_dot(cx, cy, cz, cx, cy, cz));
  const double det = pm_dot(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
  const double den = la * lb * lc + pm_dot(ax, ay, az, bx, by, bz) * lc + pm_dot(bx, by, bz, cx, cy, cz) * la +
                     pm_dot(cx, cy, cz, ax, ay, az) * lb;
  const double t = atan2(det, den) / 6.283185307179586476925286766559;
  // |t 2^40| <= 2^39: adding 1.5 2^52 rounds it to the nearest integer, ties to even, and leaves that integer in the low
  // bits of the sum -- llrint without the 64-bit conversion
  const double magic = 6755399441055744.0;
  const int64_t q = __double_as_longlong(t * kWnScale + magic) - __double_as_longlong(magic);
  return fabs(det) > 0.0 ? q : 0;   // false for the NaN of a skipped face; never asks for the sign of a zero
}

// The sum of the terms of faces f0 .. f1 - 1 of the row seen from P.  Every thread of the workgroup calls it with the same
// (r, f0, f1): barriers inside.
template <int VF64>
__device__ inline int64_t wn_walk(const void* __restrict__ verts, const int32_t* __restrict__ faces, const PmRow& r, int f0, int f1,
                                  double px, double py, double pz, double2* tile, int* flags) {
  int64_t sum = 0;
  pm_walk<kWnRec>(
      f0, f1, tile, flags, [&](int f, double2* rec) { return wn_stage<VF64>(verts, faces, r, f, rec); },
      [&](int, const double2* rec) { sum += wn_term(rec, px, py, pz); });
  return sum;
}

template <int PF64, int VF64>
__global__ __launch_bounds__(kPmBlock) void k_wn_sum(const void* __restrict__ pts_, int n_pts, const void* __restrict__ verts,
                                                     int n_verts, const int32_t* __restrict__ faces, int n_faces,
                                                     const int32_t* __restrict__ desc, int pairs, int chunk, WnWork pre, int n_slots,
                                                     int32_t* __restrict__ status) {
  __shared__ double2 tile[kPmTile * kWnRec];
  PmItem it;
  if (!pm_item<PF64>(pts_, n_pts, n_verts, n_faces, desc, pairs, chunk, pre, &it)) return;
  int64_t sum = wn_walk<VF64>(verts, faces, it.r, it.f0, it.f1, it.px, it.py, it.pz, tile, &it.flags);
  if (!it.finite) sum = 0;
  const int64_t s = pm_slot(pre, it.p, it.r.np, it.c, it.i, n_slots);
  if (it.live && s >= 0) pre.part[s] = sum;
  pm_report(it.flags, status);
}

template <int PF64>
__global__ __launch_bounds__(kPmOutBlock) void k_wn_finish(const void* __restrict__ pts_, int n_pts, int n_verts, int n_faces,
                                                           const int32_t* __restrict__ desc, int pairs, int chunk, WnWork pre,
                                                           int n_slots, int n_out, int64_t* __restrict__ sums,
                                                           double* __restrict__ winding) {
  using T = std::conditional_t<PF64 != 0, double, float>;
  PmOut out;
  if (!pm_out(n_pts, n_verts, n_faces, desc, pairs, chunk, pre, n_out, &out)) return;
  const int o = out.o;
  int64_t sum = 0;
  for (int c = 0; c < out.nc; ++c) {
    const int64_t s = pm_slot(pre, out.p, out.r.np, c, out.i, n_slots);
    if (s >= 0) sum += pre.part[s];
  }
  const T* q = static_cast<const T*>(pts_) + 3 * ((size_t)out.r.ps + out.i);
  const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
  const bool finite = fabs(px) < DPC_MESH_VOXEL_MAX_COORD && fabs(py) < DPC_MESH_VOXEL_MAX_COORD && fabs(pz) < DPC_MESH_VOXEL_MAX_COORD;
  if (sums) sums[o] = finite ? sum : 0;
  if (winding) winding[o] = finite ? (double)sum * (1.0 / kWnScale) : std::numeric_limits<double>::quiet_NaN();
}

template <int PF64, int VF64>
int wn_launch(const void* pts, int n_pts, const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc,
              int pairs, const PmGeom& g, const WnWork& w, int64_t slots, int64_t* sums, double* winding, int32_t* status,
              hipStream_t st) {
  DPC_LAUNCH("k_wn_sum", dpc_kid("k_wn_sum", PF64, VF64), (k_wn_sum<PF64, VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, pts,
             n_pts, verts, n_verts, faces, n_faces, desc, pairs, g.chunk, w, (int)slots, status);
  DPC_LAUNCH("k_wn_finish", dpc_kid("k_wn_finish", PF64), (k_wn_finish<PF64>), dim3((unsigned)((g.points + kPmOutBlock - 1) / kPmOutBlock)),
             dim3(kPmOutBlock), 0, st, pts, n_pts, n_verts, n_faces, desc, pairs, g.chunk, w, (int)slots, (int)g.points, sums, winding);
  return launch_ok();
}

// ---------------------------------------------------------------------------------------------------------------------
// grids
struct WvGeom : VoxelGrid {
  int nb;           // blocks of nodes of one grid
  int chunk, ncmax; // faces per chunk, chunks of the mesh with the most faces
  int64_t work, slots;
};

// the checks of both grid entry points: DPC_OK with the geometry, or the code to return
int wv_plan(int n_verts, int n_faces, const int32_t* host_mesh_desc, int meshes, int D, int H, int W, WvGeom* g) {
  if (n_verts < 0 || n_faces < 0 || meshes < 0) return DPC_ERR_SHAPE;
  VoxelGrid v;
  if (!voxel_grid(D, H, W, 2, &v)) return DPC_ERR_SHAPE;
  *g = WvGeom{v, pm_blocks(v.V), kPmTile * DPC_PM_CHUNK_TILES, 0, 0, 0};
  if (meshes == 0) return DPC_OK;
  if (!host_mesh_desc) return DPC_ERR_NULL;
  const int64_t len[2] = {n_verts, n_faces};
  const int rc = check_desc<4, 2>(host_mesh_desc, meshes, len, INT32_MAX, nullptr, [](const int32_t* d) { return d[3] <= kWnMaxFaces; });
  if (rc != DPC_OK) return rc;
  int max_nf = 0;
  for (int m = 0; m < meshes; ++m) max_nf = host_mesh_desc[4 * m + 3] > max_nf ? host_mesh_desc[4 * m + 3] : max_nf;
  const int64_t blocks = (int64_t)meshes * g->nb;   // > 0
  g->chunk = pm_chunk(blocks, max_nf);
  g->ncmax = (max_nf + g->chunk - 1) / g->chunk;
  g->work = blocks * g->ncmax;
  g->slots = (int64_t)meshes * g->ncmax * g->V;
  return g->work > INT32_MAX || g->slots > INT32_MAX || (int64_t)meshes * g->words > INT32_MAX ? DPC_ERR_SHAPE : DPC_OK;
}

// the table row of a mesh as a row of V nodes; false when it does not lie inside the packed arrays
__device__ inline bool wv_row(const int32_t* __restrict__ desc, int mesh, int n_verts, int n_faces, int V, PmRow* r) {
  const int32_t* d = desc + 4 * (size_t)mesh;
  r->ps = 0; r->np = V; r->vs = d[0]; r->nv = d[1]; r->fs = d[2]; r->nf = d[3];
  return r->vs >= 0 && r->nv >= 0 && (int64_t)r->vs + r->nv <= n_verts && r->fs >= 0 && r->nf >= 0 && (int64_t)r->fs + r->nf <= n_faces;
}

template <int VF64>
__global__ __launch_bounds__(kPmBlock) void k_wn_vox(const void* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces,
                                                     int n_faces, const int32_t* __restrict__ desc, int meshes, int D, int H, int W, int nb,
                                                     int chunk, int ncmax, int64_t* __restrict__ part, int32_t* __restrict__ status) {
  __shared__ double2 tile[kPmTile * kWnRec];
  const int t = threadIdx.x;
  const int per = nb * ncmax;
  const int mesh = blockIdx.x / per, local = blockIdx.x - mesh * per;
  if (mesh >= meshes) return;
  const int V = D * H * W;
  PmRow r;
  if (!wv_row(desc, mesh, n_verts, n_faces, V, &r)) return;    // k_wn_vox_finish reports it
  const int b = local % nb, c = local / nb;
  if (c >= pm_chunks(V, r.nf, chunk)) return;                  // a mesh with fewer chunks than the largest
  const int i = b * kPmBlock + t;
  const bool live = i < V;
  const int f0 = c * chunk;
  const int f1 = r.nf - f0 < chunk ? r.nf : f0 + chunk;
  const int n = live ? i : 0;
  const int n0 = n / (H * W), n1 = (n / W) % H, n2 = n % W;
  // the node centres of dpc_voxelise_meshes' frame, a division and a subtraction each
  const double px = (double)n0 / (double)(D - 1) - 0.5, py = (double)n1 / (double)(H - 1) - 0.5, pz = (double)n2 / (double)(W - 1) - 0.5;
  int flags = 0;
  const int64_t sum = wn_walk<VF64>(verts, faces, r, f0, f1, px, py, pz, tile, &flags);
  if (live) part[((int64_t)mesh * ncmax + c) * V + i] = sum;
  pm_report(flags, status);
}

__global__ __launch_bounds__(kPmBlock) void k_wn_vox_finish(const int32_t* __restrict__ desc, int n_verts, int n_faces, int meshes, int V,
                                                           int words, int nb, int chunk, int ncmax, const int64_t* __restrict__ part,
                                                           int64_t threshold_q, uint32_t* __restrict__ bits, int32_t* __restrict__ status) {
  const int t = threadIdx.x;
  const int mesh = blockIdx.x / nb, b = blockIdx.x - mesh * nb;
  if (mesh >= meshes) return;
  PmRow r;
  if (!wv_row(desc, mesh, n_verts, n_faces, V, &r)) {
    if (b == 0 && t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  const int i = b * kPmBlock + t;
  const int nc = pm_chunks(V, r.nf, chunk);   // <= ncmax for the table the host has checked; bounded here for any other
  int64_t sum = 0;
  if (i < V)
    for (int c = 0; c < nc && c < ncmax; ++c) sum += part[((int64_t)mesh * ncmax + c) * V + i];
  const bool in = i < V && r.nf > 0 && sum > threshold_q;     // a mesh without faces gives an empty grid
  const unsigned long long mask = __ballot(in);
  const int w = (b * kPmBlock + (t & ~63)) >> 5;                // the first of the wave's two words
  if ((t & 63) == 0 && w < words) bits[(size_t)mesh * words + w] = (uint32_t)mask;
  if ((t & 63) == 32 && w + 1 < words) bits[(size_t)mesh * words + w + 1] = (uint32_t)(mask >> 32);
}

template <int VF64>
int wv_launch(const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc, int meshes, const WvGeom& g,
              int64_t threshold_q, uint32_t* bits, int64_t* part, int32_t* status, hipStream_t st) {
  if (g.work > 0)
    DPC_LAUNCH("k_wn_vox", dpc_kid("k_wn_vox", VF64), (k_wn_vox<VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, verts, n_verts,
               faces, n_faces, desc, meshes, g.D, g.H, g.W, g.nb, g.chunk, g.ncmax, part, status);
  DPC_LAUNCH("k_wn_vox_finish", dpc_kid("k_wn_vox_finish"), k_wn_vox_finish, dim3((unsigned)(meshes * g.nb)), dim3(kPmBlock), 0, st, desc,
             n_verts, n_faces, meshes, g.V, g.words, g.nb, g.chunk, g.ncmax, part, threshold_q, bits, status);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_mesh_winding_workspace_bytes(const int32_t* host_pair_desc, int n_pairs) {
  if (n_pairs <= 0 || !host_pair_desc) return 0;
  PmGeom g;
  int64_t slots, total;
  if (pm_plan(INT32_MAX, INT32_MAX, INT32_MAX, host_pair_desc, n_pairs, kWnMaxFaces, &g, &slots, &total) != DPC_OK) return 0;
  return wn_carve(n_pairs, slots, nullptr, nullptr);
}

int dpc_mesh_winding(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                     const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                     int64_t* sums, double* winding, void* workspace, int32_t* status, void* stream) {
  PmGeom g;
  int64_t slots, total;
  const int rc = pm_plan(n_points, n_verts, n_faces, host_pair_desc, n_pairs, kWnMaxFaces, &g, &slots, &total);
  if (rc != DPC_OK) return rc;
  if (n_pairs == 0 || total == 0) return DPC_OK;
  if (!points || !verts || !faces || !pair_desc || (!sums && !winding) || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  WnWork w;
  wn_carve(n_pairs, slots, static_cast<char*>(workspace), &w);
  DPC_LAUNCH("k_pm_scan", dpc_kid("k_pm_scan", 1), (k_pm_scan<1>), dim3(1), dim3(kPmScanThreads), 0, st, pair_desc, n_pairs, n_points,
             n_verts, n_faces, g.chunk, w.work, w.out, w.slot, status);
  return pm_dispatch(points_f64, verts_f64, [&](auto pf, auto vf) {
    return wn_launch<decltype(pf)::value, decltype(vf)::value>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w,
                                                               slots, sums, winding, status, st);
  });
}

size_t dpc_mesh_winding_voxels_workspace_bytes(const int32_t* host_mesh_desc, int meshes, int D, int H, int W) {
  if (meshes <= 0 || !host_mesh_desc) return 0;
  WvGeom g;
  if (wv_plan(INT32_MAX, INT32_MAX, host_mesh_desc, meshes, D, H, W, &g) != DPC_OK) return 0;
  return (size_t)g.slots * sizeof(int64_t) + 16;
}

int dpc_mesh_winding_voxels(const void* verts, int n_verts, int is_f64, const int32_t* faces, int n_faces, const int32_t* mesh_desc,
                            const int32_t* host_mesh_desc, int meshes, int D, int H, int W, int64_t threshold_q, uint32_t* bits,
                            void* workspace, int32_t* status, void* stream) {
  WvGeom g;
  const int rc = wv_plan(n_verts, n_faces, host_mesh_desc, meshes, D, H, W, &g);
  if (rc != DPC_OK) return rc;
  if (meshes == 0) return DPC_OK;
  if ((!verts && n_verts > 0) || (!faces && n_faces > 0) || !mesh_desc || !bits || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  int64_t* part = static_cast<int64_t*>(workspace);
  return is_f64 ? wv_launch<1>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, threshold_q, bits, part, status, st)
                : wv_launch<0>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, threshold_q, bits, part, status, st);
}

}  // extern "C"
