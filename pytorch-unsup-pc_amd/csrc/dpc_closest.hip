// Closest points on meshes: for every point of a ragged batch of (cloud, mesh) rows, the nearest face of the row's mesh,
// the closest point Q of that face, Q's weights on the face's three vertices and the face's unit normal.  The contract is
// in include/dpc_render.h (dpc_point_mesh_closest); the per-face squared distance is dpc_point_mesh_distance's, pm_stage
// and pm_d2 of dpc_point_mesh.h, so d2 here equals d2 there.
//
// k_pm_scan<1>   the distance's scan (dpc_point_mesh.h), which here also builds the per-row prefix of workspace slots.
// k_pc_arg<fp64 points, fp64 vertices>   k_pm_dist's decomposition, from pm_item and pm_walk of dpc_point_mesh.h: one
//     workgroup of DPC_PM_BLOCK lanes per work item (row, block of points, chunk of faces), a lane owns one point,
//     DPC_PM_FACE_TILE faces staged in LDS per round and read by every lane as a broadcast.  A lane walks its chunk's
//     faces in ascending order and keeps (best, arg) with a strict <: one compare and two selects on top of pm_d2's 80
//     operations, the lowest index among equal d2, and a NaN (a skipped face) never wins.  The lane's pair goes to the
//     workspace slot [chunk][point] of its row, which no other lane writes: there is no atomic, and no slot is read
//     before the kernel has ended.
// k_pc_finish<fp64 points, fp64 vertices>   one lane per output point: reduces the point's slots in ascending chunk order
//     with a strict < (so the lowest face index among equal d2 wins whatever the chunk size), fetches the winning face's
//     vertices once (pm_fetch) for its record and its normal, decides its region with pm_d2's own terms and writes d2,
//     face, Q, the weights in the caller's vertex order and the normal.
// The result depends on neither the chunk size, nor the batching, nor the order in which workgroups run.
// Every index is checked against the device table before it becomes an address; every loop is bounded by a checked count.
#include <hip/hip_runtime.h>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_point_mesh.h"
#include "dpc_launch.h"

namespace {

struct PcWork : PmWork {   // a row has chunks * points slots
  double* best;            // [slots]
  int32_t* arg;            // [slots]
};

size_t pc_carve(int pairs, int64_t slots, char* base, PcWork* w) {
  Carver c{base};
  PcWork t;
  static_cast<PmWork&>(t) = pm_carve<1>(c, pairs);
  t.best = c.take<double>((size_t)slots);
  t.arg = c.take<int32_t>((size_t)slots);
  if (w) *w = t;
  return c.off + 16;
}

template <int PF64, int VF64>
__global__ __launch_bounds__(kPmBlock) void k_pc_arg(const void* __restrict__ pts_, int n_pts, const void* __restrict__ verts,
                                                     int n_verts, const int32_t* __restrict__ faces, int n_faces,
                                                     const int32_t* __restrict__ desc, int pairs, int chunk, PcWork pre, int n_slots,
                                                     int32_t* __restrict__ status) {
  __shared__ double2 tile[kPmTile * kPmRec];
  PmItem it;
  if (!pm_item<PF64>(pts_, n_pts, n_verts, n_faces, desc, pairs, chunk, pre, &it)) return;
  double best = std::numeric_limits<double>::infinity();
  int arg = -1;
  pm_walk<kPmRec>(
      it.f0, it.f1, tile, &it.flags, [&](int f, double2* rec) { return pm_stage<VF64>(verts, faces, it.r, f, rec); },
      [&](int f, const double2* rec) {
        const double d = pm_d2(rec, it.px, it.py, it.pz);
        const bool wins = d < best;   // false for a NaN and for an equal d2: the lower index stays
        best = wins ? d : best;
        arg = wins ? f : arg;
      });
  if (!it.finite) {
    best = std::numeric_limits<double>::infinity();
    arg = -1;
  }
  const int64_t s = pm_slot(pre, it.p, it.r.np, it.c, it.i, n_slots);
  if (it.live && s >= 0) {
    pre.best[s] = best;
    pre.arg[s] = arg;
  }
  pm_report(it.flags, status);
}

// Q on the staged face (A, B, C) and its weights on (A, B, C), from pm_d2's own terms: the foot point of the plane in the
// inside region, else the point of the nearest of the three segments (the first of equals in the order AB, AC, BC; where
// two tie, at a vertex, they name the same point).
__device__ inline void pc_closest(const double2* __restrict__ rec, const double* B, double px, double py, double pz, double* q, double* w) {
  const double2 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4], q5 = rec[5], q6 = rec[6], q7 = rec[7], q8 = rec[8],
                q9 = rec[9], q10 = rec[10];
  const double dx = px - q0.x, dy = py - q0.y, dz = pz - q1.x;
  const double e0x = q1.y, e0y = q2.x, e0z = q2.y, e1x = q3.x, e1y = q3.y, e1z = q4.x, e2x = q4.y, e2y = q5.x, e2z = q5.y;
  const double d0 = pm_dot(dx, dy, dz, e0x, e0y, e0z), d1 = pm_dot(dx, dy, dz, e1x, e1y, e1z);
  const double s = q8.x * d0 - q8.y * d1, t = q9.x * d1 - q8.y * d0;
  const double u = s + t;
  const bool inside = s >= 0.0 && t >= 0.0 && u <= 1.0;
  if (inside) {
    const double k = pm_dot(dx, dy, dz, q6.x, q6.y, q7.x) * q7.y;   // D.N / N.N
    q[0] = px - k * q6.x; q[1] = py - k * q6.y; q[2] = pz - k * q7.x;
    w[0] = 1.0 - u; w[1] = s; w[2] = t;
    return;
  }
  const double t0 = pm_clamp01(d0 * q9.y);
  const double r0x = dx - t0 * e0x, r0y = dy - t0 * e0y, r0z = dz - t0 * e0z;
  const double t1 = pm_clamp01(d1 * q10.x);
  const double r1x = dx - t1 * e1x, r1y = dy - t1 * e1y, r1z = dz - t1 * e1z;
  const double gx = dx - e0x, gy = dy - e0y, gz = dz - e0z;
  const double t2 = pm_clamp01(pm_dot(gx, gy, gz, e2x, e2y, e2z) * q10.y);
  const double r2x = gx - t2 * e2x, r2y = gy - t2 * e2y, r2z = gz - t2 * e2z;
  const double m0 = pm_dot(r0x, r0y, r0z, r0x, r0y, r0z), m1 = pm_dot(r1x, r1y, r1z, r1x, r1y, r1z),
               m2 = pm_dot(r2x, r2y, r2z, r2x, r2y, r2z);
  // the first endpoint plus t E (at t = 1 the caller puts the far vertex itself, which endpoint + E only approximates)
  if (m0 <= m1 && m0 <= m2) {
    q[0] = q0.x + t0 * e0x; q[1] = q0.y + t0 * e0y; q[2] = q1.x + t0 * e0z;
    w[0] = 1.0 - t0; w[1] = t0; w[2] = 0.0;
  } else if (m1 <= m2) {
    q[0] = q0.x + t1 * e1x; q[1] = q0.y + t1 * e1y; q[2] = q1.x + t1 * e1z;
    w[0] = 1.0 - t1; w[1] = 0.0; w[2] = t1;
  } else {
    q[0] = B[0] + t2 * e2x; q[1] = B[1] + t2 * e2y; q[2] = B[2] + t2 * e2z;
    w[0] = 0.0; w[1] = 1.0 - t2; w[2] = t2;
  }
}

template <int PF64, int VF64>
__global__ __launch_bounds__(kPmOutBlock) void k_pc_finish(const void* __restrict__ pts_, int n_pts, const void* __restrict__ verts,
                                                           int n_verts, const int32_t* __restrict__ faces, int n_faces,
                                                           const int32_t* __restrict__ desc, int pairs, int chunk, PcWork pre,
                                                           int n_slots, int n_out, double* __restrict__ d2, int32_t* __restrict__ face,
                                                           double* __restrict__ closest, double* __restrict__ weights,
                                                           double* __restrict__ normal) {
  using T = std::conditional_t<PF64 != 0, double, float>;
  PmOut out;
  if (!pm_out(n_pts, n_verts, n_faces, desc, pairs, chunk, pre, n_out, &out)) return;
  const PmRow& r = out.r;
  const int o = out.o, i = out.i;
  double best = std::numeric_limits<double>::infinity();
  int arg = -1;
  for (int c = 0; c < out.nc; ++c) {   // ascending chunks hold ascending faces: strict < keeps the lowest index
    const int64_t s = pm_slot(pre, out.p, r.np, c, i, n_slots);
    if (s < 0) continue;
    const double b = pre.best[s];
    const int a = pre.arg[s];
    const bool wins = b < best;
    best = wins ? b : best;
    arg = wins ? a : arg;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double q[3] = {nan, nan, nan}, w[3] = {nan, nan, nan}, n[3] = {0.0, 0.0, 0.0};
  double2 rec[kPmRec];   // for a skipped face only pm_fetch's NaN target: nothing reads it then
  double v[3][3];
  if ((unsigned)arg < (unsigned)r.nf && pm_fetch<VF64, kPmRec>(verts, faces, r, arg, v, rec) == 0) {
    int rot = 0;
    pm_record(v, rec, &rot);
    const T* x = static_cast<const T*>(pts_) + 3 * ((size_t)r.ps + i);
    const int ib = rot == 0 ? 1 : rot == 1 ? 2 : 0;
    double B[3], ws[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) B[c] = ib == 0 ? v[0][c] : ib == 1 ? v[1][c] : v[2][c];
    pc_closest(rec, B, (double)x[0], (double)x[1], (double)x[2], q, ws);
    // (A, B, C) are the caller's vertices (rot, rot + 1, rot + 2) mod 3
    w[0] = rot == 0 ? ws[0] : rot == 1 ? ws[2] : ws[1];
    w[1] = rot == 0 ? ws[1] : rot == 1 ? ws[0] : ws[2];
    w[2] = rot == 0 ? ws[2] : rot == 1 ? ws[1] : ws[0];
#pragma unroll
    for (int k = 0; k < 3; ++k)   // a weight of exactly 1: Q is that vertex itself, on whichever segment it was reached
      if (w[k] == 1.0) { q[0] = v[k][0]; q[1] = v[k][1]; q[2] = v[k][2]; }
    pm_normal(v, n);
  } else {
    best = std::numeric_limits<double>::infinity();
    arg = -1;
  }
  d2[o] = best;
  face[o] = arg;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    closest[3 * (size_t)o + c] = q[c];
    weights[3 * (size_t)o + c] = w[c];
    if (normal) normal[3 * (size_t)o + c] = n[c];
  }
}

template <int PF64, int VF64>
int pc_launch(const void* pts, int n_pts, const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc,
              int pairs, const PmGeom& g, const PcWork& w, int64_t slots, double* d2, int32_t* face, double* closest, double* weights,
              double* normal, int32_t* status, hipStream_t st) {
  DPC_LAUNCH("k_pc_arg", dpc_kid("k_pc_arg", PF64, VF64), (k_pc_arg<PF64, VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, pts,
             n_pts, verts, n_verts, faces, n_faces, desc, pairs, g.chunk, w, (int)slots, status);
  DPC_LAUNCH("k_pc_finish", dpc_kid("k_pc_finish", PF64, VF64), (k_pc_finish<PF64, VF64>),
             dim3((unsigned)((g.points + kPmOutBlock - 1) / kPmOutBlock)), dim3(kPmOutBlock), 0, st, pts, n_pts, verts, n_verts, faces,
             n_faces, desc, pairs, g.chunk, w, (int)slots, (int)g.points, d2, face, closest, weights, normal);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_point_mesh_closest_workspace_bytes(const int32_t* host_pair_desc, int n_pairs) {
  if (n_pairs <= 0 || !host_pair_desc) return 0;
  PmGeom g;
  int64_t slots, total;
  if (pm_plan(INT32_MAX, INT32_MAX, INT32_MAX, host_pair_desc, n_pairs, INT32_MAX, &g, &slots, &total) != DPC_OK) return 0;
  return pc_carve(n_pairs, slots, nullptr, nullptr);
}

int dpc_point_mesh_closest(const void* points, int n_points, int points_f64, const void* verts, int n_verts, int verts_f64,
                           const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc, int n_pairs,
                           double* d2, int32_t* face, double* closest, double* weights, double* normal, void* workspace,
                           int32_t* status, void* stream) {
  PmGeom g;
  int64_t slots, total;
  const int rc = pm_plan(n_points, n_verts, n_faces, host_pair_desc, n_pairs, INT32_MAX, &g, &slots, &total);
  if (rc != DPC_OK) return rc;
  if (n_pairs == 0 || total == 0) return DPC_OK;
  if (!points || !verts || !faces || !pair_desc || !d2 || !face || !closest || !weights || !workspace) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  PcWork w;
  pc_carve(n_pairs, slots, static_cast<char*>(workspace), &w);
  DPC_LAUNCH("k_pm_scan", dpc_kid("k_pm_scan", 1), (k_pm_scan<1>), dim3(1), dim3(kPmScanThreads), 0, st, pair_desc, n_pairs, n_points,
             n_verts, n_faces, g.chunk, w.work, w.out, w.slot, status);
  return pm_dispatch(points_f64, verts_f64, [&](auto pf, auto vf) {
    return pc_launch<decltype(pf)::value, decltype(vf)::value>(points, n_points, verts, n_verts, faces, n_faces, pair_desc, n_pairs, g, w,
                                                               slots, d2, face, closest, weights, normal, status, st);
  });
}

}  // extern "C"
