// The backward of dpc_nearest_batched (dpc_chamfer.hip): the gradient of sum_p gmean[p] * mean[p] + sum_i gdist[i] * v[i]
// with respect to every packed point, v = the distances or (squared mode) their squares.  Semantics, the d = 0 rule and
// the summation order in include/dpc_render.h (dpc_nearest_batched_bwd).
//
// The forward's idx says which target each source point chose; the gradient follows it.  Four launches, no atomics:
//   k_chamfer_bwd_scan     one block: per-pair prefixes of source points, target points and their 256-point blocks, built
//                          on the device from pair_desc (no host -> device copy: the call stays capture-safe);
//   k_chamfer_bwd_terms    one lane per source point: its weight w (fp64, rounded once), and the term c = w * (t - s) / d
//                          (squared mode: (2 w) * (t - s)) that its target receives; the source itself receives -c;
//   k_chamfer_bwd_targets  one lane per (pair, target): the pair's idx values stream through LDS tiles and the lane adds,
//                          in ascending source order onto 0.0, the terms of the sources that chose it.  Eight idx values per
//                          step, and a wave-uniform ballot skips the steps in which no lane of the wave is hit (nearly
//                          all of them: every source hits one lane of one wave);
//   k_chamfer_bwd_gather   one lane per packed point: walks the pair table (LDS tiles) in pair order and adds, onto 0.0,
//                          its source-role term and then its target-role sum of each pair whose ranges hold it; a block
//                          skips the pairs whose ranges miss its 256 points.
// Cost: k_chamfer_bwd_targets makes sum over pairs of src_count x tgt_count integer compares, the pair count of the
// forward's k_chamfer_partial at about one vector instruction each; the other three are linear in the points.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kBwThreads = 256;      // points per block, in all three point kernels
constexpr int kBwTile = 2048;        // idx values staged per LDS tile (8 KiB)
constexpr int kBwPairTile = 512;     // pair-table rows staged per LDS tile in the gather (12 KiB)
constexpr int kBwScanThreads = 1024;

// Prefix arrays, each [P + 1], exclusive: pre[0] = 0, pre[P] = total.
struct BwPrefix {
  int32_t* out;   // source points (the packing of min_dist / idx / gdist)
  int32_t* tgt;   // target points (the packing of the per-pair target sums)
  int32_t* sblk;  // 256-point source blocks
  int32_t* tblk;  // 256-point target blocks
};

struct BwGeom {
  int64_t src, tgt, sblk, tblk;
};

__host__ __device__ inline int bw_blocks(int n) { return (n + kBwThreads - 1) / kBwThreads; }

BwGeom bwd_geometry(int pairs, const int32_t* desc) {
  BwGeom g{0, 0, 0, 0};
  for (int p = 0; p < pairs; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    g.src += ns; g.tgt += nt;
    g.sblk += bw_blocks(ns); g.tblk += bw_blocks(nt);
  }
  return g;
}

struct BwWork {
  BwPrefix pre;
  void* term;  // [src, 3] in T: what each source point's target receives
  void* tsum;  // [tgt, 3] in T: per pair and target, the sum of the terms it received
};

size_t bwd_carve(const BwGeom& g, int pairs, size_t tsize, char* base, BwWork* w) {
  Carver c{base};
  BwWork t;
  const size_t np1 = (size_t)pairs + 1;
  t.pre.out = c.take<int32_t>(np1);
  t.pre.tgt = c.take<int32_t>(np1);
  t.pre.sblk = c.take<int32_t>(np1);
  t.pre.tblk = c.take<int32_t>(np1);
  t.term = c.take<char>((size_t)g.src * 3 * tsize);
  t.tsum = c.take<char>((size_t)g.tgt * 3 * tsize);
  if (w) *w = t;
  return c.off + 16;
}

// dpc_nearest_batched's table rules, and the target points of all pairs, which index tsum, must fit int32 as well
int bwd_check(int pairs, const int32_t* desc, int64_t n_pts) {
  const int rc = check_desc<4>(desc, pairs, {n_pts, n_pts}, INT32_MAX, nullptr, [](const int32_t* d) {
    return !(d[3] == 0 && d[1] > 0);
  });
  if (rc != DPC_OK) return rc;
  const BwGeom g = bwd_geometry(pairs, desc);
  return g.tgt > INT32_MAX || g.tblk > INT32_MAX || g.sblk > INT32_MAX ? DPC_ERR_SHAPE : DPC_OK;
}

__global__ __launch_bounds__(kBwScanThreads) void k_chamfer_bwd_scan(const int32_t* __restrict__ desc, int pairs,
                                                                     BwPrefix pre) {
  __shared__ int32_t scratch[kBwScanThreads / 64 + 1];
  const int t = threadIdx.x;
  const int seg = (pairs + kBwScanThreads - 1) / kBwScanThreads;
  const int p0 = min(pairs, t * seg), p1 = min(pairs, p0 + seg);
  int32_t loc[4] = {0, 0, 0, 0};
  for (int p = p0; p < p1; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    loc[0] += ns; loc[1] += nt; loc[2] += bw_blocks(ns); loc[3] += bw_blocks(nt);
  }
  int32_t run[4], total[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) total[k] = block_scan<kBwScanThreads>(loc[k], &run[k], scratch);
  for (int p = p0; p < p1; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    pre.out[p] = run[0]; pre.tgt[p] = run[1]; pre.sblk[p] = run[2]; pre.tblk[p] = run[3];
    run[0] += ns; run[1] += nt; run[2] += bw_blocks(ns); run[3] += bw_blocks(nt);
  }
  if (t == 0) {
    pre.out[pairs] = total[0]; pre.tgt[pairs] = total[1]; pre.sblk[pairs] = total[2]; pre.tblk[pairs] = total[3];
  }
}

// The term of source point i of pair p, in T, op for op:  w = T(gdist[i] + gmean[p] / n_p) (formed in fp64);
//   distance mode  c = ((t - s) / d) * w per component, exactly 0 when d == 0 (the reference's autograd gives NaN there);
//   squared mode   c = (2 w) * (t - s).
// No contraction: each difference, divide and multiply rounds once.  An idx outside the pair's targets (never the
// forward's own) reads nothing and gives NaN.
template <class T>
__global__ __launch_bounds__(kBwThreads) void k_chamfer_bwd_terms(const T* __restrict__ pts, const int32_t* __restrict__ desc,
                                                                  int pairs, BwPrefix pre, const T* __restrict__ min_dist,
                                                                  const int64_t* __restrict__ idx,
                                                                  const double* __restrict__ gmean,
                                                                  const T* __restrict__ gdist, int squared,
                                                                  T* __restrict__ term) {
#pragma clang fp contract(off)
  const int p = owner(pre.sblk, pairs, blockIdx.x);
  const int s0 = desc[4 * p], ns = desc[4 * p + 1], t0 = desc[4 * p + 2], nt = desc[4 * p + 3];
  const int i = (blockIdx.x - pre.sblk[p]) * kBwThreads + threadIdx.x;
  if (i >= ns) return;
  const size_t o = (size_t)pre.out[p] + i;
  double w64 = gdist != nullptr ? (double)gdist[o] : 0.0;
  if (gmean != nullptr) w64 += gmean[p] / (double)ns;
  const T w = (T)w64;
  const int64_t j = idx[o];
  T cx, cy, cz;
  if (j < 0 || j >= nt) {
    cx = cy = cz = std::numeric_limits<T>::quiet_NaN();
  } else {
    const T* s = pts + 3 * ((size_t)s0 + i);
    const T* t = pts + 3 * ((size_t)t0 + (size_t)j);
    const T dx = t[0] - s[0], dy = t[1] - s[1], dz = t[2] - s[2];
    if (squared) {
      const T w2 = (T)2 * w;
      cx = w2 * dx; cy = w2 * dy; cz = w2 * dz;
    } else {
      const T d = min_dist[o];
      if (d == (T)0) {
        cx = cy = cz = (T)0;
      } else {
        cx = (dx / d) * w; cy = (dy / d) * w; cz = (dz / d) * w;
      }
    }
  }
  T* c = term + 3 * o;
  c[0] = cx; c[1] = cy; c[2] = cz;
}

template <class T>
__global__ __launch_bounds__(kBwThreads) void k_chamfer_bwd_targets(const int32_t* __restrict__ desc, int pairs, BwPrefix pre,
                                                                    const int64_t* __restrict__ idx,
                                                                    const T* __restrict__ term, T* __restrict__ tsum) {
  __shared__ __attribute__((aligned(16))) int tile[kBwTile];
  const int p = owner(pre.tblk, pairs, blockIdx.x);
  const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
  const int j = (blockIdx.x - pre.tblk[p]) * kBwThreads + threadIdx.x;  // idx < nt: a lane past the targets is never hit
  const size_t o = (size_t)pre.out[p];
  T ax = 0, ay = 0, az = 0;
  for (int base = 0; base < ns; base += kBwTile) {
    const int n = min(kBwTile, ns - base);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kBwThreads) tile[k] = (int)idx[o + base + k];
    __syncthreads();
    const T* c0 = term + 3 * (o + base);
    auto take = [&](int v, int k) {
      if (v == j) { ax += c0[3 * k]; ay += c0[3 * k + 1]; az += c0[3 * k + 2]; }
    };
    int k = 0;
    for (; k + 8 <= n; k += 8) {  // two 16-byte LDS reads in flight per step
      const int4 q = *reinterpret_cast<const int4*>(&tile[k]);
      const int4 r = *reinterpret_cast<const int4*>(&tile[k + 4]);
      const bool hit = (q.x == j) | (q.y == j) | (q.z == j) | (q.w == j) | (r.x == j) | (r.y == j) | (r.z == j) | (r.w == j);
      if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
        take(q.x, k); take(q.y, k + 1); take(q.z, k + 2); take(q.w, k + 3);
        take(r.x, k + 4); take(r.y, k + 5); take(r.z, k + 6); take(r.w, k + 7);
      }
    }
    for (; k < n; ++k) take(tile[k], k);
  }
  if (j < nt) {  // a target that nobody chose gets +0.0
    T* g = tsum + 3 * ((size_t)pre.tgt[p] + j);
    g[0] = ax; g[1] = ay; g[2] = az;
  }
}

template <class T>
__global__ __launch_bounds__(kBwThreads) void k_chamfer_bwd_gather(const int32_t* __restrict__ desc, int pairs, BwPrefix pre,
                                                                   int n_pts, const T* __restrict__ term,
                                                                   const T* __restrict__ tsum, T* __restrict__ dpts) {
  __shared__ int32_t tab[kBwPairTile][6];
  const int64_t b0 = (int64_t)blockIdx.x * kBwThreads, b1 = b0 + kBwThreads;
  const int64_t x = b0 + threadIdx.x;
  T ax = 0, ay = 0, az = 0;
  for (int base = 0; base < pairs; base += kBwPairTile) {
    const int n = min(kBwPairTile, pairs - base);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kBwThreads) {
      const int p = base + k;
#pragma unroll
      for (int c = 0; c < 4; ++c) tab[k][c] = desc[4 * p + c];
      tab[k][4] = pre.out[p];
      tab[k][5] = pre.tgt[p];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int64_t s0 = tab[k][0], s1 = s0 + tab[k][1], t0 = tab[k][2], t1 = t0 + tab[k][3];
      if (!((s0 < b1 && s1 > b0) || (t0 < b1 && t1 > b0))) continue;  // the same for the whole block
      if (x >= s0 && x < s1) {
        const T* c = term + 3 * ((size_t)tab[k][4] + (size_t)(x - s0));
        ax -= c[0]; ay -= c[1]; az -= c[2];
      }
      if (x >= t0 && x < t1) {
        const T* g = tsum + 3 * ((size_t)tab[k][5] + (size_t)(x - t0));
        ax += g[0]; ay += g[1]; az += g[2];
      }
    }
  }
  if (x < n_pts) {
    T* g = dpts + 3 * (size_t)x;
    g[0] = ax; g[1] = ay; g[2] = az;
  }
}

template <class T>
int bwd_impl(const T* pts, int n_pts, const int32_t* desc, const BwGeom& g, int pairs, const T* min_dist, const int64_t* idx,
             const double* gmean, const T* gdist, int squared, T* dpts, void* workspace, hipStream_t st) {
  BwWork w;
  bwd_carve(g, pairs, sizeof(T), static_cast<char*>(workspace), &w);
  T* term = static_cast<T*>(w.term);
  T* tsum = static_cast<T*>(w.tsum);
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  if (pairs > 0)
    DPC_LAUNCH("k_chamfer_bwd_scan", dpc_kid("k_chamfer_bwd_scan"), k_chamfer_bwd_scan, dim3(1), dim3(kBwScanThreads), 0, st,
               desc, pairs, w.pre);
  if (g.sblk > 0)
    DPC_LAUNCH("k_chamfer_bwd_terms", dpc_kid(kIsF64 ? "k_chamfer_bwd_terms<double>" : "k_chamfer_bwd_terms<float>"),
               k_chamfer_bwd_terms<T>, dim3((unsigned)g.sblk), dim3(kBwThreads), 0, st, pts, desc, pairs, w.pre, min_dist, idx,
               gmean, gdist, squared, term);
  if (g.tblk > 0)
    DPC_LAUNCH("k_chamfer_bwd_targets", dpc_kid(kIsF64 ? "k_chamfer_bwd_targets<double>" : "k_chamfer_bwd_targets<float>"),
               k_chamfer_bwd_targets<T>, dim3((unsigned)g.tblk), dim3(kBwThreads), 0, st, desc, pairs, w.pre, idx,
               (const T*)term, tsum);
  DPC_LAUNCH("k_chamfer_bwd_gather", dpc_kid(kIsF64 ? "k_chamfer_bwd_gather<double>" : "k_chamfer_bwd_gather<float>"),
             k_chamfer_bwd_gather<T>, dim3((unsigned)bw_blocks(n_pts)), dim3(kBwThreads), 0, st, desc, pairs, w.pre, n_pts,
             (const T*)term, (const T*)tsum, dpts);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_chamfer_bwd_workspace_bytes(int pairs, const int32_t* host_pair_desc, int is_f64) {
  if (pairs <= 0 || !host_pair_desc || bwd_check(pairs, host_pair_desc, -1) != DPC_OK) return 0;
  const BwGeom g = bwd_geometry(pairs, host_pair_desc);
  return bwd_carve(g, pairs, is_f64 ? sizeof(double) : sizeof(float), nullptr, nullptr);
}

int dpc_nearest_batched_bwd(const void* pts, int n_pts, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc,
                            int pairs, const void* min_dist, const int64_t* idx, const double* gmean, const void* gdist,
                            int squared, void* dpts, void* workspace, void* stream) {
  if (pairs < 0 || n_pts < 0) return DPC_ERR_SHAPE;
  if (pairs > 0) {
    if (!host_pair_desc) return DPC_ERR_NULL;
    const int rc = bwd_check(pairs, host_pair_desc, n_pts);
    if (rc != DPC_OK) return rc;
  }
  if (n_pts == 0) return DPC_OK;  // every count is 0: there is no row of dpts to write
  if (!dpts || !workspace || (pairs > 0 && (!pair_desc || !pts))) return DPC_ERR_NULL;
  const BwGeom g = bwd_geometry(pairs, host_pair_desc);
  if (g.src > 0 && (!idx || (!squared && !min_dist))) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return bwd_impl<double>(static_cast<const double*>(pts), n_pts, pair_desc, g, pairs, static_cast<const double*>(min_dist),
                            idx, gmean, static_cast<const double*>(gdist), squared, static_cast<double*>(dpts), workspace, st);
  return bwd_impl<float>(static_cast<const float*>(pts), n_pts, pair_desc, g, pairs, static_cast<const float*>(min_dist), idx,
                         gmean, static_cast<const float*>(gdist), squared, static_cast<float*>(dpts), workspace, st);
}

}  // extern "C"
