// Batched mesh densification of ground-truth models: the reference's densify/densify_single.py (utils.densify applied
// densifyN times after parseObj and removeWeirdDuplicate) for many ragged models in one call, in fp64.  Semantics in
// include/dpc_render.h (dpc_densify); the ordering argument in DESIGN.md.
//
// The reference pops edges by (length descending, creation index ascending).  Every edge a split creates is at most
// sqrt(3)/2 of its parent, so with Lmax the longest live edge, the live edges longer than kDnBand * Lmax are exactly the
// next pops, in sorted order, and nothing created meanwhile comes between them.  One "round" splits that whole band
// (cut at the model's remaining budget):
//   k_dn_plan    one block: every model's region offsets (output rows, edges, faces, slots) from the descriptors;
//   k_dn_init    one block per model: copies the vertices to the output, checks the mesh, counts every edge's faces,
//                lays out the edge -> face slot lists in ascending face order (the reference's pushEtoFandFtoE);
//   k_dn_round   one block per model: Lmax, the band compacted in edge order, a stable LSD radix sort of the band in
//                global memory (key Lmax bits - length bits: descending length, ties in edge order), then per split its
//                midpoint, halves and the id prefixes (2 + deg edges, 2 deg faces, 4 deg slots);
//   k_dn_faces   one lane per (split, slot) whose face is owned by it (the face's lowest-rank split): replays the face's
//                1 - 3 splits in rank order, writes the medians, the final sub-faces and every slot they occupy.
// Each slot of each edge belongs to exactly one face, so no slot is written twice and no atomics order any result.
// Built with -ffp-contract=off: the only fused operations are the explicit fma of dn_length.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kDnThreads = 256;
constexpr int kDnWaves = kDnThreads / 64;
constexpr int kDnRadix = 256;
constexpr int kDnPlanThreads = 1024;
constexpr int kDnFaceBlocks = 32;   // k_dn_faces blocks per model
constexpr double kDnBand = 0.87;    // >= sqrt(3)/2 plus a margin for rounding

struct DnModel {
  int64_t vbase, ebase, fbase, sbase;  // first output row, edge, face and slot of the model's regions
  int32_t nV, nE, nF, nS;              // live counts (vertices, edges, faces, slots)
  int32_t left;                        // splits still to do; 0: the model is done (or was refused)
  int32_t sel, v0, fb0;                // this round: splits, the first new vertex, the first new face
  double lmax;                         // this round's longest live edge
};

struct DnWork {
  DnModel* model;  // [models]
  int32_t* lo;     // [Ecap] first vertex of the edge (the reference's E[e][0]), model-local
  int32_t* hi;     // [Ecap]
  double* len;     // [Ecap] np.linalg.norm(V[lo] - V[hi]); -1 once split
  int32_t* deg;    // [Ecap] faces on the edge
  int32_t* soff;   // [Ecap] first slot of its face list, model-local
  int32_t* srank;  // [Ecap] rank of the edge's split in the current round, else -1 (a cursor during k_dn_init)
  int32_t* fv;     // [Fcap, 3] face vertices, model-local, in the reference's order
  int32_t* fe;     // [Fcap, 3] the edge opposite vertex j
  int32_t* fp;     // [Fcap, 3] the face's slot in that edge's face list
  int32_t* slots;  // [Scap] face lists, model-local face ids
  uint64_t* keys[2];  // [Ecap] band sort keys
  int32_t* rows[2];   // [Ecap] band sort payload: the edge
  int32_t* sp_e;   // [Ecap] split r of the round: its edge
  int32_t* sp_eb;  // [Ecap] its first new edge (h1 = eb, h2 = eb + 1, median k = eb + 2 + k)
  int32_t* sp_fb;  // [Ecap] its first new face (slot k: fb + 2k on lo's side, fb + 2k + 1 on hi's side)
  int32_t* sp_sb;  // [Ecap] its first new slot (h1: sb, h2: sb + deg, median k: sb + 2 deg + 2k)
};

size_t dn_carve(int models, int64_t ecap, int64_t fcap, int64_t scap, char* base, DnWork* w) {
  Carver c{base};
  const size_t E = (size_t)ecap, F = (size_t)fcap, S = (size_t)scap;
  DnWork t;
  t.model = c.take<DnModel>(models);
  t.lo = c.take<int32_t>(E);
  t.hi = c.take<int32_t>(E);
  t.len = c.take<double>(E);
  t.deg = c.take<int32_t>(E);
  t.soff = c.take<int32_t>(E);
  t.srank = c.take<int32_t>(E);
  t.fv = c.take<int32_t>(3 * F);
  t.fe = c.take<int32_t>(3 * F);
  t.fp = c.take<int32_t>(3 * F);
  t.slots = c.take<int32_t>(S);
  for (int k = 0; k < 2; ++k) t.keys[k] = c.take<uint64_t>(E);
  for (int k = 0; k < 2; ++k) t.rows[k] = c.take<int32_t>(E);
  t.sp_e = c.take<int32_t>(E);
  t.sp_eb = c.take<int32_t>(E);
  t.sp_fb = c.take<int32_t>(E);
  t.sp_sb = c.take<int32_t>(E);
  if (w) *w = t;
  return c.off;
}

// Per-model capacities: a split adds 2 + deg edges, 2 deg faces and 4 deg slots, deg <= D = max(2, max_face_count).
__host__ __device__ inline int64_t dn_ecap(int64_t e, int64_t n, int64_t D) { return e + n * (2 + D); }
__host__ __device__ inline int64_t dn_fcap(int64_t f, int64_t n, int64_t D) { return f + 2 * n * D; }
__host__ __device__ inline int64_t dn_scap(int64_t f, int64_t n, int64_t D) { return 3 * f + 4 * n * D; }

// np.linalg.norm(a - b) as numpy computes it: sqrt(x.dot(x)), the dot an fma chain (OpenBLAS ddot).
__device__ inline double dn_length(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
}

// desc row: v_start, v_count, e_start, e_count, f_start, f_count, budget
constexpr int kDnDesc = 7;

__global__ __launch_bounds__(kDnPlanThreads) void k_dn_plan(const int32_t* __restrict__ desc, int models, int D, DnWork w) {
  __shared__ int64_t scratch[kDnPlanThreads / 64 + 1];
  const int t = threadIdx.x;
  const int seg = (models + kDnPlanThreads - 1) / kDnPlanThreads;
  const int m0 = min(models, t * seg), m1 = min(models, m0 + seg);
  int64_t s[4] = {0, 0, 0, 0};
  for (int m = m0; m < m1; ++m) {
    const int32_t* d = desc + kDnDesc * m;
    s[0] += (int64_t)d[1] + d[6];
    s[1] += dn_ecap(d[3], d[6], D);
    s[2] += dn_fcap(d[5], d[6], D);
    s[3] += dn_scap(d[5], d[6], D);
  }
  int64_t b[4];
  for (int k = 0; k < 4; ++k) block_scan<kDnPlanThreads>(s[k], &b[k], scratch);
  for (int m = m0; m < m1; ++m) {
    const int32_t* d = desc + kDnDesc * m;
    DnModel& M = w.model[m];
    M.vbase = b[0]; M.ebase = b[1]; M.fbase = b[2]; M.sbase = b[3];
    b[0] += (int64_t)d[1] + d[6];
    b[1] += dn_ecap(d[3], d[6], D);
    b[2] += dn_fcap(d[5], d[6], D);
    b[3] += dn_scap(d[5], d[6], D);
  }
}

__global__ __launch_bounds__(kDnThreads) void k_dn_init(const double* __restrict__ verts, const int32_t* __restrict__ edges,
                                                        const int32_t* __restrict__ faces,
                                                        const int32_t* __restrict__ face_edges,
                                                        const int32_t* __restrict__ desc, int D, DnWork w,
                                                        double* __restrict__ out, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ active) {
  __shared__ int bad;
  __shared__ int scratch[kDnWaves + 1];
  const int m = blockIdx.x, t = threadIdx.x;
  const int32_t* d = desc + kDnDesc * m;
  const int v0 = d[0], nv = d[1], e0 = d[2], ne = d[3], f0 = d[4], nf = d[5], budget = d[6];
  DnModel M = w.model[m];
  if (t == 0) bad = 0;
  __syncthreads();
  int flags = 0;
  for (int i = t; i < nv; i += kDnThreads) {
    const double* p = verts + 3 * ((int64_t)v0 + i);
    double* q = out + 3 * (M.vbase + i);
    for (int k = 0; k < 3; ++k) {
      flags |= isfinite(p[k]) ? 0 : DPC_STATUS_NONFINITE;
      q[k] = p[k];
    }
  }
  int32_t* lo = w.lo + M.ebase;
  int32_t* hi = w.hi + M.ebase;
  double* len = w.len + M.ebase;
  int32_t* deg = w.deg + M.ebase;
  int32_t* soff = w.soff + M.ebase;
  int32_t* cur = w.srank + M.ebase;
  for (int i = t; i < ne; i += kDnThreads) {
    const int a = edges[2 * ((int64_t)e0 + i)], b = edges[2 * ((int64_t)e0 + i) + 1];
    double L = -1.0;
    if (a < 0 || a >= nv || b < 0 || b >= nv || a == b) {
      flags |= DPC_STATUS_BAD_INDEX;
    } else {
      L = dn_length(verts + 3 * ((int64_t)v0 + a), verts + 3 * ((int64_t)v0 + b));
      if (!(L <= 1.7976931348623157e308)) flags |= DPC_STATUS_NONFINITE;
    }
    lo[i] = a;
    hi[i] = b;
    len[i] = L;
    deg[i] = 0;
    cur[i] = 0;
  }
  __syncthreads();
  for (int f = t; f < nf; f += kDnThreads) {
    int v[3], e[3];
    for (int j = 0; j < 3; ++j) {
      v[j] = faces[3 * ((int64_t)f0 + f) + j];
      e[j] = face_edges[3 * ((int64_t)f0 + f) + j];
    }
    bool ok = true;
    for (int j = 0; j < 3; ++j) ok = ok && v[j] >= 0 && v[j] < nv && e[j] >= 0 && e[j] < ne;
    for (int j = 0; ok && j < 3; ++j) {  // edge j joins the two other vertices
      const int a = v[(j + 1) % 3], b = v[(j + 2) % 3];
      ok = (lo[e[j]] == a && hi[e[j]] == b) || (lo[e[j]] == b && hi[e[j]] == a);
    }
    if (!ok) {
      flags |= DPC_STATUS_BAD_INDEX;
      continue;
    }
    for (int j = 0; j < 3; ++j) atomicAdd(&deg[e[j]], 1);  // a count: the order of the adds does not matter
  }
  if (flags) atomicOr(&bad, flags);
  __syncthreads();
  // slot offsets: exclusive prefix of the face counts, in edge order
  int run = 0;
  for (int c0 = 0; c0 < ne; c0 += kDnThreads) {
    const int i = c0 + t;
    const int g = i < ne ? deg[i] : 0;
    if (g > D) flags |= DPC_STATUS_BAD_INDEX;  // more faces on an edge than the caller's max_face_count
    int excl;
    const int total = block_scan<kDnThreads>(g, &excl, scratch);
    if (i < ne) soff[i] = run + excl;
    run += total;
  }
  if (flags) atomicOr(&bad, flags);
  __syncthreads();
  const int fail = bad;
  if (fail) {
    if (t == 0) {
      if (status) atomicOr(status, fail);
      M.nV = nv; M.nE = ne; M.nF = nf; M.nS = 3 * nf;
      M.left = 0; M.sel = 0; M.v0 = nv; M.fb0 = nf; M.lmax = 0.0;
      w.model[m] = M;
    }
    return;
  }
  int32_t* slots = w.slots + M.sbase;
  for (int f = t; f < nf; f += kDnThreads)
    for (int j = 0; j < 3; ++j) {
      const int e = face_edges[3 * ((int64_t)f0 + f) + j];
      slots[soff[e] + atomicAdd(&cur[e], 1)] = f;  // any order: sorted below
    }
  __syncthreads();
  for (int i = t; i < ne; i += kDnThreads) {  // each face list in ascending face order (pushEtoFandFtoE's order)
    int32_t* s = slots + soff[i];
    for (int a = 1; a < deg[i]; ++a) {
      const int x = s[a];
      int b = a - 1;
      while (b >= 0 && s[b] > x) { s[b + 1] = s[b]; --b; }
      s[b + 1] = x;
    }
    cur[i] = -1;
  }
  __syncthreads();
  for (int f = t; f < nf; f += kDnThreads)
    for (int j = 0; j < 3; ++j) {
      const int64_t src = 3 * ((int64_t)f0 + f) + j, dst = 3 * (M.fbase + f) + j;
      const int e = face_edges[src];
      int p = 0;
      while (slots[soff[e] + p] != f) ++p;
      w.fv[dst] = faces[src];
      w.fe[dst] = e;
      w.fp[dst] = p;
    }
  if (t == 0) {
    M.nV = nv; M.nE = ne; M.nF = nf; M.nS = 3 * nf;
    M.left = budget; M.sel = 0; M.v0 = nv; M.fb0 = nf; M.lmax = 0.0;
    w.model[m] = M;
    if (budget > 0) atomicAdd(active, 1);
  }
}

__device__ inline uint64_t dn_bits(double x) { return (uint64_t)__double_as_longlong(x); }

__global__ __launch_bounds__(kDnThreads) void k_dn_round(DnWork w, double* __restrict__ out, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ active) {
  __shared__ double smax[kDnThreads];
  __shared__ uint64_t skey[kDnThreads];
  __shared__ int scratch[kDnWaves + 1];
  __shared__ int hist[kDnRadix];
  __shared__ int wcnt[kDnWaves][kDnRadix];
  __shared__ int sflags;
  const int m = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  DnModel M = w.model[m];
  if (M.left <= 0) {
    if (t == 0 && M.sel != 0) { w.model[m].sel = 0; }  // k_dn_faces of a finished model returns at once
    return;
  }
  if (t == 0) sflags = 0;
  const int32_t* lo = w.lo + M.ebase;
  const int32_t* hi = w.hi + M.ebase;
  double* len = w.len + M.ebase;
  // 1. Lmax over the live edges (split edges hold -1)
  double mx = -1.0;
  for (int i = t; i < M.nE; i += kDnThreads) mx = fmax(mx, len[i]);
  smax[t] = mx;
  __syncthreads();
  for (int s = kDnThreads / 2; s > 0; s >>= 1) {
    if (t < s) smax[t] = fmax(smax[t], smax[t + s]);
    __syncthreads();
  }
  const double lmax = smax[0];
  const double thr = kDnBand * lmax;
  const uint64_t lbits = dn_bits(lmax);
  // 2. the band, compacted in edge order: len > c Lmax (and len == Lmax, for an all-zero Lmax)
  uint64_t* kin = w.keys[0] + M.ebase;
  int32_t* rin = w.rows[0] + M.ebase;
  int B = 0;
  uint64_t kmax = 0;
  for (int c0 = 0; c0 < M.nE; c0 += kDnThreads) {
    const int i = c0 + t;
    const double L = i < M.nE ? len[i] : -1.0;
    const bool in = L > thr || (L >= lmax && L >= 0.0);
    int excl;
    const int total = block_scan<kDnThreads>(in ? 1 : 0, &excl, scratch);
    if (in) {
      const uint64_t key = lbits - dn_bits(L);  // both positive: descending length is ascending key
      kin[B + excl] = key;
      rin[B + excl] = i;
      kmax = key > kmax ? key : kmax;
    }
    B += total;
  }
  skey[t] = kmax;
  __syncthreads();
  for (int s = kDnThreads / 2; s > 0; s >>= 1) {
    if (t < s) skey[t] = skey[t] > skey[t + s] ? skey[t] : skey[t + s];
    __syncthreads();
  }
  int passes = 0;
  while (passes < 8 && (skey[0] >> (8 * passes)) != 0) ++passes;
  // 3. stable LSD radix sort of the band, 8 bits per pass, one 256-member chunk at a time
  const uint64_t below = (1ull << lane) - 1;
  for (int pass = 0; pass < passes; ++pass) {
    const uint64_t* ks = w.keys[pass & 1] + M.ebase;
    const int32_t* rs = w.rows[pass & 1] + M.ebase;
    uint64_t* kd = w.keys[(pass + 1) & 1] + M.ebase;
    int32_t* rd = w.rows[(pass + 1) & 1] + M.ebase;
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < B; i += kDnThreads) atomicAdd(&hist[(int)((ks[i] >> (8 * pass)) & 0xff)], 1);
    __syncthreads();
    int base;
    block_scan<kDnThreads>(hist[t], &base, scratch);  // digit t starts at base
    for (int c0 = 0; c0 < B; c0 += kDnThreads) {
      const int i = c0 + t;
      const bool live = i < B;
      const uint64_t key = live ? ks[i] : 0;
      const int row = live ? rs[i] : 0;
      const int dg = (int)((key >> (8 * pass)) & 0xff);
      uint64_t same = __ballot(live);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const uint64_t ones = __ballot((dg >> b) & 1);
        same &= ((dg >> b) & 1) ? ones : ~ones;
      }
      for (int v = 0; v < kDnWaves; ++v) wcnt[v][t] = 0;
      __syncthreads();
      if (live && (same & below) == 0) wcnt[wave][dg] = __popcll(same);  // the group's lowest lane
      __syncthreads();
      {  // digit t: the waves' counts prefixed in wave order after the digit's running base
        int r = base;
        for (int v = 0; v < kDnWaves; ++v) { const int n = wcnt[v][t]; wcnt[v][t] = r; r += n; }
        base = r;
      }
      __syncthreads();
      if (live) {
        const int dst = wcnt[wave][dg] + __popcll(same & below);
        kd[dst] = key;
        rd[dst] = row;
      }
      __syncthreads();
    }
  }
  const int32_t* order = w.rows[passes & 1] + M.ebase;
  // 4. the splits: rank r < sel takes order[r]
  const int sel = min(B, M.left);
  int32_t* deg = w.deg + M.ebase;
  int32_t* soff = w.soff + M.ebase;
  int32_t* srank = w.srank + M.ebase;
  double* V = out + 3 * M.vbase;
  int re = 0, rf = 0, rs = 0;
  int flags = 0;
  for (int c0 = 0; c0 < sel; c0 += kDnThreads) {
    const int r = c0 + t;
    const bool live = r < sel;
    const int e = live ? order[r] : 0;
    const int g = live ? deg[e] : 0;
    int xe, xf, xs;
    const int te = block_scan<kDnThreads>(live ? 2 + g : 0, &xe, scratch);
    const int tf = block_scan<kDnThreads>(2 * g, &xf, scratch);
    const int ts = block_scan<kDnThreads>(4 * g, &xs, scratch);
    if (live) {
      const int eb = M.nE + re + xe, fb = M.nF + rf + xf, sb = M.nS + rs + xs;
      w.sp_e[M.ebase + r] = e;
      w.sp_eb[M.ebase + r] = eb;
      w.sp_fb[M.ebase + r] = fb;
      w.sp_sb[M.ebase + r] = sb;
      srank[e] = r;
      const int a = lo[e], b = hi[e], vn = M.nV + r;
      double* p = V + 3 * (int64_t)vn;
      for (int k = 0; k < 3; ++k) {
        p[k] = (V[3 * (int64_t)a + k] + V[3 * (int64_t)b + k]) / 2.0;
        flags |= isfinite(p[k]) ? 0 : DPC_STATUS_NONFINITE;
      }
      const int ends[2] = {a, b};
      for (int h = 0; h < 2; ++h) {  // halves: [lo, new] then [hi, new], the parent's face count and slot order
        const double L = dn_length(V + 3 * (int64_t)ends[h], p);
        if (L > thr) flags |= DPC_STATUS_DENSIFY_ORDER;
        w.lo[M.ebase + eb + h] = ends[h];
        w.hi[M.ebase + eb + h] = vn;
        len[eb + h] = L;
        deg[eb + h] = g;
        soff[eb + h] = sb + h * g;
        srank[eb + h] = -1;
      }
      len[e] = -1.0;  // split: no longer live
    }
    re += te;
    rf += tf;
    rs += ts;
  }
  if (flags) atomicOr(&sflags, flags);
  __syncthreads();
  if (t == 0) {
    if (sflags && status) atomicOr(status, sflags);
    M.v0 = M.nV;
    M.fb0 = M.nF;
    M.sel = sel;
    M.lmax = lmax;
    M.nV += sel;
    M.nE += re;
    M.nF += rf;
    M.nS += rs;
    M.left -= sel;
    if (sflags & DPC_STATUS_NONFINITE) M.left = 0;  // stop: the lengths are meaningless from here
    w.model[m] = M;
    if (M.left == 0) atomicSub(active, 1);
  }
}

// One lane per (split r, slot k): face g = the slot's face.  The lane of g's lowest-rank split this round replays g's
// splits in rank order on up to four local sub-faces, then writes the medians, the final sub-faces and their slots.
__global__ __launch_bounds__(kDnThreads) void k_dn_faces(DnWork w, const double* __restrict__ out,
                                                         int32_t* __restrict__ status) {
  const int m = blockIdx.y;
  const DnModel M = w.model[m];
  if (M.sel <= 0) return;
  const int32_t* sp_e = w.sp_e + M.ebase;
  const int32_t* sp_eb = w.sp_eb + M.ebase;
  const int32_t* sp_fb = w.sp_fb + M.ebase;
  const int32_t* sp_sb = w.sp_sb + M.ebase;
  const int items = (M.nF - M.fb0) / 2;
  const double thr = kDnBand * M.lmax;
  const double* V = out + 3 * M.vbase;
  int flags = 0;
  for (int i = blockIdx.x * kDnThreads + threadIdx.x; i < items; i += gridDim.x * kDnThreads) {
    int a = 0, b = M.sel - 1;  // the last split whose first face item is <= i
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if ((sp_fb[mid] - M.fb0) / 2 <= i) a = mid; else b = mid - 1;
    }
    const int r = a, e = sp_e[r], k = i - (sp_fb[r] - M.fb0) / 2;
    const int g = w.slots[M.sbase + w.soff[M.ebase + e] + k];
    int fv[4][3], fe[4][3], fp[4][3], fid[4];
    int rk[3], rmin = INT32_MAX;
    for (int j = 0; j < 3; ++j) {
      const int64_t x = 3 * (M.fbase + g) + j;
      fv[0][j] = w.fv[x];
      fe[0][j] = w.fe[x];
      fp[0][j] = w.fp[x];
      rk[j] = w.srank[M.ebase + fe[0][j]];
      if (rk[j] >= 0) rmin = min(rmin, rk[j]);
    }
    if (rmin != r) continue;  // another split of this round owns the face
    fid[0] = g;
    int nf = 1;
    for (int step = 0; step < 3; ++step) {  // the face's splits in rank order
      int js = -1;
      for (int j = 0; j < 3; ++j)
        if (rk[j] >= 0 && (js < 0 || rk[j] < rk[js])) js = j;
      if (js < 0) break;
      const int rt = rk[js];
      rk[js] = -1;
      const int et = sp_e[rt];
      int q = 0, j = 0;  // the sub-face holding the edge, and its position there
      for (int u = 0; u < nf; ++u)
        for (int x = 0; x < 3; ++x)
          if (fe[u][x] == et) { q = u; j = x; }
      const int kt = fp[q][j], dg = w.deg[M.ebase + et];
      const int vi1 = w.lo[M.ebase + et], vi2 = w.hi[M.ebase + et], vio = fv[q][j];
      const int vn = M.v0 + rt, eb = sp_eb[rt], fb = sp_fb[rt], sb = sp_sb[rt], med = eb + 2 + kt;
      int i1 = 0, i2 = 0;
      for (int x = 0; x < 3; ++x) {
        if (fv[q][x] == vi1) i1 = x;
        if (fv[q][x] == vi2) i2 = x;
      }
      const double L = dn_length(V + 3 * (int64_t)vio, V + 3 * (int64_t)vn);
      if (L > thr) flags |= DPC_STATUS_DENSIFY_ORDER;
      w.lo[M.ebase + med] = vio;  // the median [vio, new], faces [lo's side, hi's side]
      w.hi[M.ebase + med] = vn;
      w.len[M.ebase + med] = L;
      w.deg[M.ebase + med] = 2;
      w.soff[M.ebase + med] = sb + 2 * dg + 2 * kt;
      w.srank[M.ebase + med] = -1;
      for (int x = 0; x < 3; ++x) { fv[nf][x] = fv[q][x]; fe[nf][x] = fe[q][x]; fp[nf][x] = fp[q][x]; }
      // lo's side (f_new1: hi -> new) keeps the edge from vio to lo; hi's side (f_new2: lo -> new) the one to hi
      fv[q][i2] = vn; fe[q][i1] = med; fp[q][i1] = 0; fe[q][j] = eb; fp[q][j] = kt; fid[q] = fb + 2 * kt;
      fv[nf][i1] = vn; fe[nf][i2] = med; fp[nf][i2] = 1; fe[nf][j] = eb + 1; fp[nf][j] = kt; fid[nf] = fb + 2 * kt + 1;
      ++nf;
    }
    for (int u = 0; u < nf; ++u)
      for (int x = 0; x < 3; ++x) {
        const int64_t dst = 3 * (M.fbase + fid[u]) + x;
        w.fv[dst] = fv[u][x];
        w.fe[dst] = fe[u][x];
        w.fp[dst] = fp[u][x];
        w.slots[M.sbase + w.soff[M.ebase + fe[u][x]] + fp[u][x]] = fid[u];
      }
  }
  if (flags && status) atomicOr(status, flags);
}

struct DnTotals {
  int64_t rows, edges, faces, splits;
};

inline int dn_maxdeg(int max_face_count) { return max_face_count > 2 ? max_face_count : 2; }

}  // namespace

extern "C" {

size_t dpc_densify_workspace_bytes(int models, int64_t edges, int64_t faces, int64_t splits, int max_face_count) {
  if (models <= 0 || edges < 0 || faces < 0 || splits < 0 || max_face_count < 0 || max_face_count > (1 << 20)) return 0;
  const int64_t D = dn_maxdeg(max_face_count);
  return dn_carve(models, dn_ecap(edges, splits, D), dn_fcap(faces, splits, D), dn_scap(faces, splits, D), nullptr,
                  nullptr);
}

int dpc_densify(const double* verts, int n_verts, const int32_t* edges, int n_edges, const int32_t* faces,
                const int32_t* face_edges, int n_faces, const int32_t* model_desc, const int32_t* host_model_desc,
                int models, int max_face_count, int begin, int rounds, double* out, int32_t* status, int32_t* active,
                void* workspace, void* stream) {
  if (models < 0 || n_verts < 0 || n_edges < 0 || n_faces < 0 || rounds < 0 || max_face_count < 0 ||
      max_face_count > (1 << 20))
    return DPC_ERR_SHAPE;
  if (models == 0) return DPC_OK;
  if (!host_model_desc) return DPC_ERR_NULL;
  const int D = dn_maxdeg(max_face_count);
  const int rc = check_desc<kDnDesc>(
      host_model_desc, models, {(int64_t)n_verts, (int64_t)n_edges, (int64_t)n_faces}, INT64_MAX, nullptr,
      [D](const int32_t* d) {
        const int64_t nv = d[1], ne = d[3], nf = d[5], n = d[6];
        if (n < 0 || (n > 0 && ne == 0)) return false;  // a budget, and with one something to split
        // every model-local id (output rows, edges, 3 x faces, slots) must fit an int32
        return nv + n <= INT32_MAX && dn_ecap(ne, n, D) <= INT32_MAX && 3 * dn_fcap(nf, n, D) <= INT32_MAX &&
               dn_scap(nf, n, D) <= INT32_MAX;
      });
  if (rc != DPC_OK) return rc;
  DnTotals tot{0, 0, 0, 0};
  for (int m = 0; m < models; ++m) {
    const int32_t* d = host_model_desc + (int64_t)kDnDesc * m;
    tot.rows += (int64_t)d[1] + d[6];
    tot.edges += d[3];
    tot.faces += d[5];
    tot.splits += d[6];
  }
  if (!model_desc || !out || !active || !workspace) return DPC_ERR_NULL;
  if (begin && ((tot.rows > 0 && !verts) || (tot.edges > 0 && !edges) || (tot.faces > 0 && (!faces || !face_edges))))
    return DPC_ERR_NULL;
  DnWork w;
  dn_carve(models, dn_ecap(tot.edges, tot.splits, D), dn_fcap(tot.faces, tot.splits, D),
           dn_scap(tot.faces, tot.splits, D), static_cast<char*>(workspace), &w);
  hipStream_t st = (hipStream_t)stream;
  if (begin) {
    DPC_LAUNCH("k_dn_plan", dpc_kid("k_dn_plan"), k_dn_plan, dim3(1), dim3(kDnPlanThreads), 0, st, model_desc, models, D,
               w);
    DPC_LAUNCH("k_dn_init", dpc_kid("k_dn_init"), k_dn_init, dim3(models), dim3(kDnThreads), 0, st, verts, edges, faces,
               face_edges, model_desc, D, w, out, status, active);
  }
  for (int r = 0; r < rounds; ++r) {  // the number of rounds a model needs is on the device: done models return at once
    DPC_LAUNCH("k_dn_round", dpc_kid("k_dn_round"), k_dn_round, dim3(models), dim3(kDnThreads), 0, st, w, out, status,
               active);
    DPC_LAUNCH("k_dn_faces", dpc_kid("k_dn_faces"), k_dn_faces, dim3(kDnFaceBlocks, models), dim3(kDnThreads), 0, st, w,
               out, status);
  }
  return launch_ok();
}

}  // extern "C"
