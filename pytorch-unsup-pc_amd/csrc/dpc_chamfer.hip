// Batched nearest-target distances with per-pair means: the Chamfer half of the reference's evaluation
// (dpc/run/eval_chamfer_to.py:88-145: compute_distance in both directions per view, then np.mean) for a whole split in
// one call.  Semantics in include/dpc_render.h (dpc_nearest_batched).
//
// All clouds live in one packed buffer; P directed pairs (src_start, src_count, tgt_start, tgt_count) index it, so
// "pred -> GT" and "GT -> pred" are two pairs and the views of one model share one GT copy.  Four launches, no atomics:
//   k_chamfer_scan     one block: per-pair prefixes of source blocks, work items, output points and 8192-point chunks,
//                      built on the device from pair_desc (the call makes no host -> device copy and stays capture-safe);
//   k_chamfer_partial  one block per work item (pair, 256-point source block, target slice), found by binary search in
//                      the work prefix: nearest_scan (dpc_nearest.h, shared with k_nearest_partial) over the slice;
//   k_chamfer_merge    one block per (pair, source block): merges the slices in slice order with a strict <, writes the
//                      distance and the index of every source point into the packed outputs;
//   k_chamfer_chunks   one wave per (pair, 8192-point chunk): the chunk's float64 sum in numpy's pairwise order;
//   k_chamfer_mean     one lane per pair: adds the chunk sums in order onto 0.0 and divides by src_count in fp64.
// The last two reproduce np.mean of the float64 distances bit for bit (numpy 2.x's np.add.reduce: buffers of 8192
// elements summed with pairwise_sum, buffer sums added left to right; tests/test_chamfer_host.py pins that order).
// dpc_chamfer_pair_means runs the scan and the last two alone over values the caller packed (the squared distances of the
// Chamfer loss, whose backward is dpc_chamfer_bwd.hip).
// Compute-bound on the fp32 / fp64 vector pipe in k_chamfer_partial: sum over pairs of src_count x tgt_count d2s.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_nearest.h"
#include "dpc_launch.h"

namespace {

constexpr int kChThreads = 256;   // source points per block
constexpr int kChTile = 1024;     // targets staged per LDS tile (12 KiB fp32, 24 KiB fp64), as k_nearest_partial
constexpr int kChChunk = 8192;    // numpy's reduction buffer (NPY_BUFSIZE elements)
constexpr int kChLeaf = 128;      // pairwise_sum's unrolled block
constexpr int kChMaxLeaves = 2 * kChChunk / kChLeaf;  // leaves hold at least 64 elements
constexpr int kChScanThreads = 1024;

// Prefix arrays, each [P + 1], exclusive: pre[0] = 0, pre[P] = total.
struct ChPrefix {
  int32_t* blk;    // 256-point source blocks
  int32_t* work;   // (source block, target slice) items
  int32_t* out;    // output points (sum of src_count)
  int32_t* chunk;  // 8192-point chunks of the mean
};

struct ChGeom {
  int64_t blocks, work, points, chunks;
  int slice, max_nt;
};

__host__ __device__ inline int ch_src_blocks(int ns) { return (ns + kChThreads - 1) / kChThreads; }
__host__ __device__ inline int ch_slices(int ns, int nt, int slice) { return ns > 0 ? (nt + slice - 1) / slice : 0; }
__host__ __device__ inline int ch_chunks(int ns) { return (ns + kChChunk - 1) / kChChunk; }

// Host side of the geometry, from a validated host table.  Target slices by nearest_slice (dpc_nearest.h) over the
// batch's source blocks and its largest target; a split-sized batch runs with one slice.
ChGeom chamfer_geometry(int pairs, const int32_t* desc) {
  ChGeom g{0, 0, 0, 0, 256, 0};
  for (int p = 0; p < pairs; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    g.blocks += ch_src_blocks(ns);
    g.points += ns;
    g.chunks += ch_chunks(ns);
    if (ns > 0 && nt > g.max_nt) g.max_nt = nt;
  }
  if (g.max_nt > 0) g.slice = (int)nearest_slice(g.blocks, g.max_nt);
  for (int p = 0; p < pairs; ++p)
    g.work += (int64_t)ch_src_blocks(desc[4 * p + 1]) * ch_slices(desc[4 * p + 1], desc[4 * p + 3], g.slice);
  return g;
}

struct ChWork {
  ChPrefix pre;
  double* chunk_sum;  // [chunks]
  void* dist;         // [points] in T: the distances the mean reads when the caller wants none
  void* part_dist;    // [work * 256] in T
  int* part_idx;      // [work * 256]
};

size_t chamfer_carve(const ChGeom& g, int pairs, size_t tsize, char* base, ChWork* w) {
  Carver c{base};
  ChWork t;
  const size_t np1 = (size_t)pairs + 1;
  t.pre.blk = c.take<int32_t>(np1);
  t.pre.work = c.take<int32_t>(np1);
  t.pre.out = c.take<int32_t>(np1);
  t.pre.chunk = c.take<int32_t>(np1);
  t.chunk_sum = c.take<double>(g.chunks);
  t.dist = c.take<char>((size_t)g.points * tsize);
  t.part_dist = c.take<char>((size_t)g.work * kChThreads * tsize);
  t.part_idx = c.take<int>((size_t)g.work * kChThreads);
  if (w) *w = t;
  return c.off + 16;
}

__global__ __launch_bounds__(kChScanThreads) void k_chamfer_scan(const int32_t* __restrict__ desc, int pairs, int slice,
                                                                 ChPrefix pre) {
  __shared__ int32_t scratch[kChScanThreads / 64 + 1];
  const int t = threadIdx.x;
  const int seg = (pairs + kChScanThreads - 1) / kChScanThreads;
  const int p0 = min(pairs, t * seg), p1 = min(pairs, p0 + seg);
  int32_t loc[4] = {0, 0, 0, 0};
  for (int p = p0; p < p1; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    loc[0] += ch_src_blocks(ns);
    loc[1] += ch_src_blocks(ns) * ch_slices(ns, nt, slice);
    loc[2] += ns;
    loc[3] += ch_chunks(ns);
  }
  int32_t run[4], total[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) total[k] = block_scan<kChScanThreads>(loc[k], &run[k], scratch);
  for (int p = p0; p < p1; ++p) {
    const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
    pre.blk[p] = run[0]; pre.work[p] = run[1]; pre.out[p] = run[2]; pre.chunk[p] = run[3];
    run[0] += ch_src_blocks(ns);
    run[1] += ch_src_blocks(ns) * ch_slices(ns, nt, slice);
    run[2] += ns;
    run[3] += ch_chunks(ns);
  }
  if (t == 0) {
    pre.blk[pairs] = total[0]; pre.work[pairs] = total[1]; pre.out[pairs] = total[2]; pre.chunk[pairs] = total[3];
  }
}

template <class T>
__global__ __launch_bounds__(kChThreads) void k_chamfer_partial(const T* __restrict__ pts, const int32_t* __restrict__ desc,
                                                                int pairs, int slice, const int32_t* __restrict__ work_pre,
                                                                T* __restrict__ part_dist, int* __restrict__ part_idx) {
  __shared__ T tx[kChTile], ty[kChTile], tz[kChTile];
  const int item = blockIdx.x;
  const int p = owner(work_pre, pairs, item);
  const int s0 = desc[4 * p], ns = desc[4 * p + 1], t0 = desc[4 * p + 2], nt = desc[4 * p + 3];
  const int sb = ch_src_blocks(ns);
  const int local = item - work_pre[p];
  const int b = local % sb, s = local / sb;  // the source blocks of one slice are adjacent: they read the same targets
  const int i = b * kChThreads + threadIdx.x;
  const bool live = i < ns;
  const int j0 = s * slice, j1 = min(nt, j0 + slice);
  T sx = 0, sy = 0, sz = 0;
  if (live) {
    const T* q = pts + 3 * ((size_t)s0 + i);
    sx = q[0]; sy = q[1]; sz = q[2];
  }
  T best_d2;
  int best;
  nearest_scan<T, kChThreads, kChTile>(pts + 3 * (size_t)t0, j0, j1, sx, sy, sz, tx, ty, tz, best_d2, best);
  part_dist[(size_t)item * kChThreads + threadIdx.x] = sqrt(best_d2);
  part_idx[(size_t)item * kChThreads + threadIdx.x] = best;
}

template <class T>
__global__ __launch_bounds__(kChThreads) void k_chamfer_merge(const int32_t* __restrict__ desc, int pairs, int slice,
                                                              ChPrefix pre, const T* __restrict__ part_dist,
                                                              const int* __restrict__ part_idx, T* __restrict__ dist,
                                                              int64_t* __restrict__ idx) {
  const int p = owner(pre.blk, pairs, blockIdx.x);
  const int ns = desc[4 * p + 1], nt = desc[4 * p + 3];
  const int b = blockIdx.x - pre.blk[p];
  const int i = b * kChThreads + threadIdx.x;
  if (i >= ns) return;
  const int sb = ch_src_blocks(ns), nsl = ch_slices(ns, nt, slice);
  size_t o = ((size_t)pre.work[p] + b) * kChThreads + threadIdx.x;
  T best_dist = part_dist[o];
  int best = part_idx[o];
  for (int s = 1; s < nsl; ++s) {  // slices hold increasing target indices: strict < keeps the first minimum
    o += (size_t)sb * kChThreads;
    const T d = part_dist[o];
    if (d < best_dist) { best_dist = d; best = part_idx[o]; }
  }
  const size_t out = (size_t)pre.out[p] + i;
  dist[out] = best_dist;
  if (idx != nullptr) idx[out] = best;
}

// numpy's pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) of one buffer, n <= 8192 elements, in float64:
//   n < 8     sequential from zero;
//   n <= 128  eight accumulators r[j] = a[j], r[j] += a[i + j] per full group of 8, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//             then the n % 8 tail sequentially;
//   else      n2 = n/2 - (n/2) % 8, pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2).
// Lane 0 walks the split tree (an LDS stack, no scratch) to list the leaves left to right, every lane sums leaves, and
// lane 0 walks the tree again adding the leaf sums in the recursion's order.
__device__ inline int ch_split(int n) { return n / 2 - (n / 2) % 8; }

template <class T>
__device__ double ch_leaf_sum(const T* __restrict__ a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += (double)a[i];
    return r;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += (double)a[i]; r1 += (double)a[i + 1]; r2 += (double)a[i + 2]; r3 += (double)a[i + 3];
    r4 += (double)a[i + 4]; r5 += (double)a[i + 5]; r6 += (double)a[i + 6]; r7 += (double)a[i + 7];
  }
  double r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) r += (double)a[i];
  return r;
}

template <class T>
__global__ __launch_bounds__(64) void k_chamfer_chunks(int pairs, ChPrefix pre, const T* __restrict__ dist,
                                                       double* __restrict__ chunk_sum) {
  __shared__ int leaf_start[kChMaxLeaves], leaf_n[kChMaxLeaves];
  __shared__ double leaf_sum[kChMaxLeaves];
  __shared__ int stk_a[16], stk_n[16], stk_stage[16];
  __shared__ double stk_val[16];
  __shared__ int n_leaves;
  const int c = blockIdx.x;
  const int p = owner(pre.chunk, pairs, c);
  const int k = c - pre.chunk[p];
  const int ns = pre.out[p + 1] - pre.out[p];
  const int n = min(kChChunk, ns - k * kChChunk);
  const T* a = dist + (size_t)pre.out[p] + (size_t)k * kChChunk;
  if (threadIdx.x == 0) {  // leaves, left to right (depth <= 8 for n <= 8192)
    int sp = 0, nl = 0;
    stk_a[0] = 0; stk_n[0] = n; sp = 1;
    while (sp > 0) {
      --sp;
      const int s = stk_a[sp], m = stk_n[sp];
      if (m <= kChLeaf) {
        leaf_start[nl] = s; leaf_n[nl] = m; ++nl;
      } else {
        const int m2 = ch_split(m);
        stk_a[sp] = s + m2; stk_n[sp] = m - m2; ++sp;  // right first: the left half is popped next
        stk_a[sp] = s; stk_n[sp] = m2; ++sp;
      }
    }
    n_leaves = nl;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < n_leaves; l += 64) leaf_sum[l] = ch_leaf_sum(a + leaf_start[l], leaf_n[l]);
  __syncthreads();
  if (threadIdx.x == 0) {  // the same tree, post-order: stage 0 descends left, 1 holds the left sum, 2 adds the right
#pragma clang fp contract(off)
    int sp = 1, leaf = 0;
    double ret = 0.0;
    stk_n[0] = n; stk_stage[0] = 0;
    while (sp > 0) {
      const int f = sp - 1, m = stk_n[f];
      if (m <= kChLeaf) {
        ret = leaf_sum[leaf++];
        --sp;
      } else if (stk_stage[f] == 0) {
        stk_stage[f] = 1;
        stk_n[sp] = ch_split(m); stk_stage[sp] = 0; ++sp;
      } else if (stk_stage[f] == 1) {
        stk_val[f] = ret;
        stk_stage[f] = 2;
        stk_n[sp] = m - ch_split(m); stk_stage[sp] = 0; ++sp;
      } else {
        ret = stk_val[f] + ret;
        --sp;
      }
    }
    chunk_sum[c] = ret;
  }
}

// np.add.reduce over the buffers: 0.0 + S_0 + S_1 + ..., left to right; np.mean = sum / n (an empty pair: 0 / 0 = NaN)
__global__ __launch_bounds__(64) void k_chamfer_mean(int pairs, ChPrefix pre, const double* __restrict__ chunk_sum,
                                                     double* __restrict__ mean) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= pairs) return;
  double s = 0.0;
  for (int c = pre.chunk[p]; c < pre.chunk[p + 1]; ++c) s += chunk_sum[c];
  mean[p] = s / (double)(pre.out[p + 1] - pre.out[p]);
}

// DPC_ERR_SHAPE for a table the reference could not evaluate or the kernels cannot index (the output points, the sum of
// src_count, are indexed by int32); DPC_OK otherwise.  n_pts < 0: the length is not known yet.
int chamfer_check(int pairs, const int32_t* desc, int64_t n_pts) {
  return check_desc<4>(desc, pairs, {n_pts, n_pts}, INT32_MAX, nullptr, [](const int32_t* d) {
    return !(d[3] == 0 && d[1] > 0);  // argmin over an empty set: the reference raises
  });
}

template <class T>
int chamfer_impl(const T* pts, const int32_t* desc, const ChGeom& g, int pairs, double* mean, T* min_dist, int64_t* idx,
                 void* workspace, hipStream_t st) {
  ChWork w;
  chamfer_carve(g, pairs, sizeof(T), static_cast<char*>(workspace), &w);
  T* dist = min_dist != nullptr ? min_dist : static_cast<T*>(w.dist);
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  DPC_LAUNCH("k_chamfer_scan", dpc_kid("k_chamfer_scan"), k_chamfer_scan, dim3(1), dim3(kChScanThreads), 0, st, desc, pairs,
             g.slice, w.pre);
  if (g.work > 0) {
    DPC_LAUNCH("k_chamfer_partial", dpc_kid(kIsF64 ? "k_chamfer_partial<double>" : "k_chamfer_partial<float>"),
               k_chamfer_partial<T>, dim3((unsigned)g.work), dim3(kChThreads), 0, st, pts, desc, pairs, g.slice,
               (const int32_t*)w.pre.work, static_cast<T*>(w.part_dist), w.part_idx);
    DPC_LAUNCH("k_chamfer_merge", dpc_kid(kIsF64 ? "k_chamfer_merge<double>" : "k_chamfer_merge<float>"), k_chamfer_merge<T>,
               dim3((unsigned)g.blocks), dim3(kChThreads), 0, st, desc, pairs, g.slice, w.pre,
               (const T*)w.part_dist, (const int*)w.part_idx, dist, idx);
    DPC_LAUNCH("k_chamfer_chunks", dpc_kid(kIsF64 ? "k_chamfer_chunks<double>" : "k_chamfer_chunks<float>"),
               k_chamfer_chunks<T>, dim3((unsigned)g.chunks), dim3(64), 0, st, pairs, w.pre, (const T*)dist, w.chunk_sum);
  }
  DPC_LAUNCH("k_chamfer_mean", dpc_kid("k_chamfer_mean"), k_chamfer_mean, dim3((pairs + 63) / 64), dim3(64), 0, st, pairs,
             w.pre, (const double*)w.chunk_sum, mean);
  return launch_ok();
}

// The mean stage alone, over values the caller packed in pair order (the squared distances of the Chamfer loss).
template <class T>
int chamfer_means_impl(const T* values, const int32_t* desc, const ChGeom& g, int pairs, double* mean, void* workspace,
                       hipStream_t st) {
  ChWork w;
  chamfer_carve(g, pairs, sizeof(T), static_cast<char*>(workspace), &w);
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  DPC_LAUNCH("k_chamfer_scan", dpc_kid("k_chamfer_scan"), k_chamfer_scan, dim3(1), dim3(kChScanThreads), 0, st, desc, pairs,
             g.slice, w.pre);
  if (g.chunks > 0)
    DPC_LAUNCH("k_chamfer_chunks", dpc_kid(kIsF64 ? "k_chamfer_chunks<double>" : "k_chamfer_chunks<float>"),
               k_chamfer_chunks<T>, dim3((unsigned)g.chunks), dim3(64), 0, st, pairs, w.pre, values, w.chunk_sum);
  DPC_LAUNCH("k_chamfer_mean", dpc_kid("k_chamfer_mean"), k_chamfer_mean, dim3((pairs + 63) / 64), dim3(64), 0, st, pairs,
             w.pre, (const double*)w.chunk_sum, mean);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_chamfer_workspace_bytes(int pairs, const int32_t* host_pair_desc, int is_f64) {
  if (pairs <= 0 || !host_pair_desc || chamfer_check(pairs, host_pair_desc, -1) != DPC_OK) return 0;
  const ChGeom g = chamfer_geometry(pairs, host_pair_desc);
  return chamfer_carve(g, pairs, is_f64 ? sizeof(double) : sizeof(float), nullptr, nullptr);
}

int dpc_nearest_batched(const void* pts, int n_pts, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc,
                        int pairs, double* mean, void* min_dist, int64_t* idx, void* workspace, void* stream) {
  if (pairs < 0 || n_pts < 0) return DPC_ERR_SHAPE;
  if (pairs == 0) return DPC_OK;
  if (!host_pair_desc) return DPC_ERR_NULL;
  const int rc = chamfer_check(pairs, host_pair_desc, n_pts);
  if (rc != DPC_OK) return rc;
  if (!pair_desc || !mean || !workspace || (n_pts > 0 && !pts)) return DPC_ERR_NULL;
  const ChGeom g = chamfer_geometry(pairs, host_pair_desc);
  if (g.work > INT32_MAX || g.blocks > INT32_MAX) return DPC_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return chamfer_impl<double>(static_cast<const double*>(pts), pair_desc, g, pairs, mean, static_cast<double*>(min_dist),
                                idx, workspace, st);
  return chamfer_impl<float>(static_cast<const float*>(pts), pair_desc, g, pairs, mean, static_cast<float*>(min_dist), idx,
                             workspace, st);
}

int dpc_chamfer_pair_means(const void* values, int is_f64, const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs,
                           double* mean, void* workspace, void* stream) {
  if (pairs < 0) return DPC_ERR_SHAPE;
  if (pairs == 0) return DPC_OK;
  if (!host_pair_desc) return DPC_ERR_NULL;
  const int rc = chamfer_check(pairs, host_pair_desc, -1);
  if (rc != DPC_OK) return rc;
  const ChGeom g = chamfer_geometry(pairs, host_pair_desc);
  if (!pair_desc || !mean || !workspace || (g.points > 0 && !values)) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) return chamfer_means_impl<double>(static_cast<const double*>(values), pair_desc, g, pairs, mean, workspace, st);
  return chamfer_means_impl<float>(static_cast<const float*>(values), pair_desc, g, pairs, mean, workspace, st);
}

}  // extern "C"
