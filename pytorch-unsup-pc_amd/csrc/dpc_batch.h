// The ragged-batch plumbing shared by the fp64 evaluation pipelines (dpc_icp.hip, dpc_chamfer.hip, dpc_downsample.hip,
// dpc_densify.hip).  Items (clouds, pairs of clouds, meshes) are (start, count) ranges of packed buffers, listed in a
// host int32 descriptor table with a device copy.  The host checks the table (check_desc) and carves one
// caller-allocated workspace (Carver); the device builds per-item prefixes (block_scan), and each block finds its item
// by binary search in them (owner).  The voxel files share check_pairs and block_sum as well.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/dpc_render.h"

// Hands out the pieces of one workspace in order, each rounded up to 16 bytes.  With base == nullptr it only counts:
// `off` is then the bytes the pieces span.  dpc_downsample_workspace_bytes and dpc_densify_workspace_bytes report off,
// which is at most
//   downsample  56 C + 28 M + 2056 ceil(M / 4096) + 1056 + 14 * 15 bytes  (C clouds, M members),
//   densify     72 models + 68 Ecap + 36 Fcap + 4 Scap + 19 * 15 bytes     (the capacities dn_ecap, dn_fcap, dn_scap);
// dpc_chamfer_workspace_bytes and dpc_icp_workspace_bytes report off + 16.
struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (n * sizeof(T) + 15) & ~(size_t)15;
    return p;
  }
};

// Host check of a descriptor table of `rows` rows of W int32.  Columns (2k, 2k + 1), k < K, are (start, count) ranges
// of an array of len[k] elements (len[k] < 0: no length is known, only the signs are checked).  The counts of column 1
// are summed, and the table is refused once that sum passes `limit`.  row_ok(row) holds an entry point's own rules.
// Returns DPC_ERR_SHAPE, or DPC_OK with the sum in *total.
template <int W, int K, class RowOk>
int check_desc(const int32_t* desc, int rows, const int64_t (&len)[K], int64_t limit, int64_t* total, RowOk row_ok) {
  int64_t sum = 0;
  for (int r = 0; r < rows; ++r) {
    const int32_t* d = desc + (int64_t)W * r;
    for (int k = 0; k < K; ++k) {
      const int64_t s = d[2 * k], n = d[2 * k + 1];
      if (s < 0 || n < 0 || (len[k] >= 0 && s + n > len[k])) return DPC_ERR_SHAPE;
    }
    if (!row_ok(d)) return DPC_ERR_SHAPE;
    sum += d[1];
    if (sum > limit) return DPC_ERR_SHAPE;
  }
  if (total) *total = sum;
  return DPC_OK;
}

// Host check of a table of `pairs` rows (i, j) of int32: items i of n_a and j of n_b.
inline int check_pairs(const int32_t* host_pairs, int pairs, int n_a, int n_b) {
  for (int p = 0; p < pairs; ++p) {
    const int32_t i = host_pairs[2 * (int64_t)p], j = host_pairs[2 * (int64_t)p + 1];
    if (i < 0 || i >= n_a || j < 0 || j >= n_b) return DPC_ERR_SHAPE;
  }
  return DPC_OK;
}

// The largest i < n with pre[i] <= x, for an exclusive prefix pre[0..n]: items without work share their prefix with the
// next item that has some, so the search always lands on the item that owns work unit x.
__device__ inline int owner(const int32_t* __restrict__ pre, int n, int x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Exclusive scan of one T per thread over a block of N threads (N a multiple of 64, <= 1024); returns the block total.
// scratch holds N / 64 + 1 T in LDS.  Every thread of the block must call it.
template <int N, class T>
__device__ inline T block_scan(T v, T* excl, T* scratch) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  T x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) scratch[wave] = x;
  __syncthreads();
  if (t == 0) {
    T run = 0;
    for (int w = 0; w < N / 64; ++w) { const T s = scratch[w]; scratch[w] = run; run += s; }
    scratch[N / 64] = run;
  }
  __syncthreads();
  *excl = scratch[wave] + x - v;
  const T total = scratch[N / 64];
  __syncthreads();
  return total;
}

// The sum of one T per thread over a block of THREADS threads, in thread 0 alone (0 elsewhere): wave sums in T by
// shuffles, then thread 0 adds the waves in wave order in Acc.  scratch holds THREADS / 64 T in LDS.  Every thread of
// the block must call it.
template <int THREADS, class Acc, class T>
__device__ inline Acc block_sum(T v, T* scratch) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  Acc s = 0;
  if (t == 0)
    for (int w = 0; w < THREADS / 64; ++w) s += scratch[w];
  __syncthreads();
  return s;
}
