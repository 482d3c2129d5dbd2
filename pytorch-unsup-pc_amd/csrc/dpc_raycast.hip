// Ray-mesh intersection: for every ray O + t D of a ragged batch of (ray bundle, mesh) rows, the first face of the row's
// mesh it hits (the smallest t in [t_min, t_max]), that hit's weights on the face's vertices, the face's unit normal and
// the number of faces hit.  The contract (the rule for one ray and one face, the tie rule, the guards) is in
// include/dpc_render.h (dpc_ray_mesh_intersect); tests/raycast_oracle.py restates it in numpy.  All arithmetic is fp64,
// fp32 inputs widen exactly first, and nothing is fused: this file is built with -ffp-contract=off.  Brute force: every
// ray of a row meets every face of it.
//
// k_pm_scan<1>   the distance's scan (dpc_point_mesh.h): checks the device table's rows and builds the per-row prefixes of
//     work items, output rays and workspace slots.
// k_rc_hit<fp64 rays, fp64 vertices>   k_pc_arg's decomposition, from pm_item, pm_walk and pm_fetch of dpc_point_mesh.h:
//     one workgroup of DPC_PM_BLOCK lanes per work item (row, block of rays, chunk of faces), a lane owns one ray --
//     pm_item loads its origin as "the point", the lane loads its direction from the second array at the same index.  Per
//     round the workgroup stages DPC_PM_FACE_TILE faces in LDS, one lane per face, as (V0, E1, E2): nine doubles widened
//     and subtracted once (a skipped face as NaNs, which no ray hits).  Then every lane walks the tile; all lanes read the
//     same record, an LDS broadcast.  Per face and ray the Moeller-Trumbore test of rc_terms: two cross products and three
//     dot products decide inside or outside by products alone; the division t = (E2 . Q) / det runs only under the branch
//     of a face the ray is inside of, so the common miss pays for none.  A lane keeps (best t, its face, the count) in
//     registers, the best under a strict < while the faces ascend: the lowest index among bit-equal t.  Its triple goes
//     to the workspace slot [chunk][ray] of its row, which no other lane writes: there is no atomic, and no slot is read
//     before the kernel has ended.
// k_rc_finish<fp64 rays, fp64 vertices>   one lane per output ray: reduces the ray's slots in ascending chunk order with a
//     strict < (the lowest face index among equal t whatever the chunk size), adds the counts (integers: any order), stages
//     the winning face alone, recomputes u and v with rc_terms' own expressions and the normal with pm_normal, and writes
//     t, face, weights, hits and the normal.  It also reports a ray that is not finite, so a row without faces reports too.
// The result depends on neither the chunk size, nor the batching, nor the order in which workgroups run.
// Every index is checked against the device table before it becomes an address; every loop is bounded by a checked count.
#include <hip/hip_runtime.h>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_point_mesh.h"
#include "dpc_launch.h"

namespace {

constexpr int kRcRec = 5;   // double2 per staged face: V0, E1, E2 and one pad
static_assert(kPmTile * kRcRec * 16 == DPC_RAY_LDS_BYTES && DPC_RAY_LDS_BYTES <= 64 * 1024, "the tile fits the default LDS limit");

struct RcWork : PmWork {   // a row has chunks * rays slots, 16 bytes each
  double* t;               // [slots] the smallest hit t of the chunk, +inf without one
  int32_t* face;           // [slots] its face, -1 without one
  int32_t* hits;           // [slots] the faces of the chunk the ray hits
};

size_t rc_carve(int pairs, int64_t slots, char* base, RcWork* w) {
  Carver c{base};
  RcWork r;
  static_cast<PmWork&>(r) = pm_carve<1>(c, pairs);
  r.t = c.take<double>((size_t)slots);
  r.face = c.take<int32_t>((size_t)slots);
  r.hits = c.take<int32_t>((size_t)slots);
  if (w) *w = r;
  return c.off + 16;
}

// the checks of the entry point and of its workspace size; a row with rays and no faces is accepted: every ray misses
int rc_plan(int n_rays, int n_verts, int n_faces, const int32_t* host_pair_desc, int n_pairs, PmGeom* g, int64_t* slots, int64_t* total) {
  return pm_plan(n_rays, n_verts, n_faces, host_pair_desc, n_pairs, INT32_MAX, g, slots, total, true);
}

struct RcRay {
  double ox, oy, oz, dx, dy, dz;
};

// Element i of a packed [.,3] array, widened, in x; false (and zeros) when a component is NaN, infinite or
// >= DPC_MESH_VOXEL_MAX_COORD in magnitude.
template <int F64>
__device__ inline bool rc_vec3(const void* __restrict__ a_, size_t i, double* x) {
  using T = std::conditional_t<F64 != 0, double, float>;
  const T* q = static_cast<const T*>(a_) + 3 * i;
  x[0] = (double)q[0]; x[1] = (double)q[1]; x[2] = (double)q[2];
  const bool finite = fabs(x[0]) < DPC_MESH_VOXEL_MAX_COORD && fabs(x[1]) < DPC_MESH_VOXEL_MAX_COORD && fabs(x[2]) < DPC_MESH_VOXEL_MAX_COORD;
  if (!finite) x[0] = x[1] = x[2] = 0.0;
  return finite;
}

__device__ inline double rc_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// Stages face i of the row into rec[0 .. kRcRec) as (V0, E1 = V1 - V0, E2 = V2 - V0), the caller's vertices in v; returns
// the flags of the face (pm_fetch's rules).
template <int VF64>
__device__ inline int rc_stage(const void* __restrict__ verts, const int32_t* __restrict__ faces, const PmRow& r, int i, double (&v)[3][3],
                               double2* rec) {
  const int flags = pm_fetch<VF64, kRcRec>(verts, faces, r, i, v, rec);
  if (flags) return flags;
  rec[0] = make_double2(v[0][0], v[0][1]);
  rec[1] = make_double2(v[0][2], v[1][0] - v[0][0]);
  rec[2] = make_double2(v[1][1] - v[0][1], v[1][2] - v[0][2]);
  rec[3] = make_double2(v[2][0] - v[0][0], v[2][1] - v[0][1]);
  rec[4] = make_double2(v[2][2] - v[0][2], 0.0);
  return 0;
}

// The terms of the staged face and the ray that need no division: det = E1 . (D x E2), a = T . (D x E2) and b = D . Q for
// T = O - V0 and Q = T x E1, and whether the ray's line meets the closed triangle (u = a / det >= 0, v = b / det >= 0,
// u + v <= 1, decided on the products).  False for the NaNs of a skipped face, a parallel or zero-area face and a zero D.
struct RcTerms {
  double det, a, b, qx, qy, qz;
  bool inside;
};

__device__ __forceinline__ RcTerms rc_terms(const double2* __restrict__ rec, const RcRay& r) {
  const double2 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4];
  const double e1x = q1.y, e1y = q2.x, e1z = q2.y, e2x = q3.x, e2y = q3.y, e2z = q4.x;
  const double pvx = r.dy * e2z - r.dz * e2y, pvy = r.dz * e2x - r.dx * e2z, pvz = r.dx * e2y - r.dy * e2x;
  RcTerms m;
  m.det = rc_dot(e1x, e1y, e1z, pvx, pvy, pvz);
  const double tx = r.ox - q0.x, ty = r.oy - q0.y, tz = r.oz - q1.x;
  m.a = rc_dot(tx, ty, tz, pvx, pvy, pvz);
  m.qx = ty * e1z - tz * e1y; m.qy = tz * e1x - tx * e1z; m.qz = tx * e1y - ty * e1x;
  m.b = rc_dot(r.dx, r.dy, r.dz, m.qx, m.qy, m.qz);
  const double s = m.det > 0.0 ? 1.0 : -1.0;
  const double as = s * m.a, bs = s * m.b, mag = fabs(m.det);
  m.inside = mag > 0.0 && as >= 0.0 && bs >= 0.0 && as + bs <= mag;
  return m;
}

// t of a face the ray's line is inside of: (E2 . Q) / det
__device__ __forceinline__ double rc_t(const double2* __restrict__ rec, const RcTerms& m) {
  const double2 q3 = rec[3], q4 = rec[4];
  return rc_dot(q3.x, q3.y, q4.x, m.qx, m.qy, m.qz) / m.det;
}

template <int RF64, int VF64>
__global__ __launch_bounds__(kPmBlock) void k_rc_hit(const void* __restrict__ org, const void* __restrict__ dir, int n_rays,
                                                     const void* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces,
                                                     int n_faces, const int32_t* __restrict__ desc, int pairs, int chunk, RcWork pre,
                                                     int n_slots, double t_min, double t_max, int cull, int32_t* __restrict__ status) {
  __shared__ double2 tile[kPmTile * kRcRec];
  PmItem it;
  if (!pm_item<RF64>(org, n_rays, n_verts, n_faces, desc, pairs, chunk, pre, &it)) return;
  double d[3] = {0.0, 0.0, 0.0};
  if (it.live && !rc_vec3<RF64>(dir, (size_t)it.r.ps + it.i, d)) it.finite = false;   // k_rc_finish reports it, and answers
  if (!it.finite) d[0] = d[1] = d[2] = 0.0;                                             // det == 0: it hits nothing
  const RcRay ray{it.px, it.py, it.pz, d[0], d[1], d[2]};
  double best = std::numeric_limits<double>::infinity();
  int arg = -1, count = 0;
  pm_walk<kRcRec>(
      it.f0, it.f1, tile, &it.flags,
      [&](int f, double2* rec) {
        double v[3][3];
        return rc_stage<VF64>(verts, faces, it.r, f, v, rec);
      },
      [&](int f, const double2* rec) {
        const RcTerms m = rc_terms(rec, ray);
        if (m.inside && !(cull && m.det < 0.0)) {   // the division stays out of the common path
          const double t = rc_t(rec, m);
          const bool hit = t >= t_min && t <= t_max;   // false for a NaN
          const bool wins = hit && t < best;           // an equal t: the lower index stays
          count += hit ? 1 : 0;
          best = wins ? t : best;
          arg = wins ? f : arg;
        }
      });
  const int64_t s = pm_slot(pre, it.p, it.r.np, it.c, it.i, n_slots);
  if (it.live && s >= 0) {
    pre.t[s] = best;
    pre.face[s] = arg;
    pre.hits[s] = count;
  }
  pm_report(it.flags, status);
}

template <int RF64, int VF64>
__global__ __launch_bounds__(kPmOutBlock) void k_rc_finish(const void* __restrict__ org, const void* __restrict__ dir, int n_rays,
                                                           const void* __restrict__ verts, int n_verts,
                                                           const int32_t* __restrict__ faces, int n_faces,
                                                           const int32_t* __restrict__ desc, int pairs, int chunk, RcWork pre,
                                                           int n_slots, int n_out, double* __restrict__ t_out,
                                                           int32_t* __restrict__ face, double* __restrict__ weights,
                                                           int32_t* __restrict__ hits, double* __restrict__ normal,
                                                           int32_t* __restrict__ status) {
  PmOut out;
  if (!pm_out(n_rays, n_verts, n_faces, desc, pairs, chunk, pre, n_out, &out)) return;
  const PmRow& r = out.r;
  const int o = out.o, i = out.i;
  double best = std::numeric_limits<double>::infinity();
  int arg = -1, count = 0;
  for (int c = 0; c < out.nc; ++c) {   // ascending chunks hold ascending faces: strict < keeps the lowest index
    const int64_t s = pm_slot(pre, out.p, r.np, c, i, n_slots);
    if (s < 0) continue;
    const double b = pre.t[s];
    const int a = pre.face[s];
    const bool wins = b < best;
    best = wins ? b : best;
    arg = wins ? a : arg;
    count += pre.hits[s];
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double w[3] = {nan, nan, nan}, n[3] = {0.0, 0.0, 0.0};
  double O[3], D[3];
  const bool o_ok = rc_vec3<RF64>(org, (size_t)r.ps + i, O), d_ok = rc_vec3<RF64>(dir, (size_t)r.ps + i, D);
  const bool finite = o_ok && d_ok;
  double2 rec[kRcRec];
  double v[3][3];
  if (!finite) {
    best = nan;
    arg = -1;
    count = 0;
    pm_report(kPmNonFinite, status);
  } else if ((unsigned)arg < (unsigned)r.nf && rc_stage<VF64>(verts, faces, r, arg, v, rec) == 0) {
    const RcTerms m = rc_terms(rec, RcRay{O[0], O[1], O[2], D[0], D[1], D[2]});
    const double u = m.a / m.det, vv = m.b / m.det;
    w[0] = (1.0 - u) - vv; w[1] = u; w[2] = vv;
    pm_normal(v, n);
  } else {
    best = std::numeric_limits<double>::infinity();
    arg = -1;
  }
  t_out[o] = best;
  face[o] = arg;
  if (hits) hits[o] = count;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    weights[3 * (size_t)o + c] = w[c];
    if (normal) normal[3 * (size_t)o + c] = n[c];
  }
}

template <int RF64, int VF64>
int rc_launch(const void* org, const void* dir, int n_rays, const void* verts, int n_verts, const int32_t* faces, int n_faces,
              const int32_t* desc, int pairs, const PmGeom& g, const RcWork& w, int64_t slots, double t_min, double t_max, int cull,
              double* t, int32_t* face, double* weights, int32_t* hits, double* normal, int32_t* status, hipStream_t st) {
  if (g.work > 0)   // no work item when no row with rays has a face
    DPC_LAUNCH("k_rc_hit", dpc_kid("k_rc_hit", RF64, VF64), (k_rc_hit<RF64, VF64>), dim3((unsigned)g.work), dim3(kPmBlock), 0, st, org, dir,
               n_rays, verts, n_verts, faces, n_faces, desc, pairs, g.chunk, w, (int)slots, t_min, t_max, cull, status);
  DPC_LAUNCH("k_rc_finish", dpc_kid("k_rc_finish", RF64, VF64), (k_rc_finish<RF64, VF64>),
             dim3((unsigned)((g.points + kPmOutBlock - 1) / kPmOutBlock)), dim3(kPmOutBlock), 0, st, org, dir, n_rays, verts, n_verts, faces,
             n_faces, desc, pairs, g.chunk, w, (int)slots, (int)g.points, t, face, weights, hits, normal, status);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_ray_mesh_workspace_bytes(const int32_t* host_pair_desc, int n_pairs) {
  if (n_pairs <= 0 || !host_pair_desc) return 0;
  PmGeom g;
  int64_t slots, total;
  if (rc_plan(INT32_MAX, INT32_MAX, INT32_MAX, host_pair_desc, n_pairs, &g, &slots, &total) != DPC_OK) return 0;
  return rc_carve(n_pairs, slots, nullptr, nullptr);
}

int dpc_ray_mesh_intersect(const void* origins, const void* directions, int n_rays, int rays_f64, const void* verts, int n_verts,
                           int verts_f64, const int32_t* faces, int n_faces, const int32_t* pair_desc, const int32_t* host_pair_desc,
                           int n_pairs, double t_min, double t_max, int cull_backfaces, double* t, int32_t* face, double* weights,
                           int32_t* hits, double* normal, void* workspace, int32_t* status, void* stream) {
  PmGeom g;
  int64_t slots, total;
  const int rc = rc_plan(n_rays, n_verts, n_faces, host_pair_desc, n_pairs, &g, &slots, &total);
  if (rc != DPC_OK) return rc;
  if (!(t_min <= t_max)) return DPC_ERR_SHAPE;   // a NaN too
  if (n_pairs == 0 || total == 0) return DPC_OK;
  if (!origins || !directions || (!verts && n_verts > 0) || (!faces && n_faces > 0) || !pair_desc || !t || !face || !weights || !workspace)
    return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  RcWork w;
  rc_carve(n_pairs, slots, static_cast<char*>(workspace), &w);
  DPC_LAUNCH("k_pm_scan", dpc_kid("k_pm_scan", 1), (k_pm_scan<1>), dim3(1), dim3(kPmScanThreads), 0, st, pair_desc, n_pairs, n_rays,
             n_verts, n_faces, g.chunk, w.work, w.out, w.slot, status);
  return pm_dispatch(rays_f64, verts_f64, [&](auto rf, auto vf) {
    return rc_launch<decltype(rf)::value, decltype(vf)::value>(origins, directions, n_rays, verts, n_verts, faces, n_faces, pair_desc,
                                                               n_pairs, g, w, slots, t_min, t_max, cull_backfaces != 0, t, face, weights,
                                                               hits, normal, status, st);
  });
}

}  // extern "C"
