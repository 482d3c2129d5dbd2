// Batched voxel-grid downsampling of ground-truth clouds: open3d's PointCloud::VoxelDownSample (0.7 - 0.9), as the
// reference's densify/downsample_gt.py:47-57 calls it, for many clouds in one call, in fp64.  Semantics and the one
// deliberate divergence (output order) in include/dpc_render.h (dpc_voxel_downsample).
//
// Clouds are (start, count) ranges of one packed buffer; their members (M = sum of counts) are keyed
// slot | kx | ky | kz, stably sorted, cut into voxels and averaged.  No host synchronisation and no floating-point
// atomics; the only atomics are integer LDS adds of the radix histograms.
//   k_ds_bounds    one block per cloud: fp64 min / max (any tree is exact), lo = min - vs * 0.5, open3d's "too small" test,
//                  the largest key per axis (floor((max - lo) / vs): the key is monotonic in the coordinate), non-finite;
//   k_ds_plan      one block: member prefix per cloud, batch-wide key field widths, the number of 8-bit digit passes
//                  (0 .. 8) and the abort flag that later kernels obey; status bits;
//   k_ds_keys      one lane per member: key and input row;
//   k_ds_hist      per pass and 4096-member tile: digit histogram, stored digit-major;
//   k_ds_digits    per pass, one block per digit: exclusive scan of that digit's tile counts, the digit's total;
//   k_ds_scatter   per pass and tile: stable rank inside the tile (8 ballots per wave, waves in order), then the move;
//   k_ds_heads     per tile: voxels starting in it (a key differs from its predecessor);
//   k_ds_tiles     one block: exclusive scan of those counts, the voxel count V;
//   k_ds_voxels    per tile: the first sorted position of every voxel;
//   k_ds_average   one lane per voxel: its members added one at a time in input order onto 0.0, one fp64 division;
//   k_ds_clouds    one lane per cloud: output count and offset (binary search of the voxel starts).
// Every digit pass is enqueued (8); a pass beyond the plan's count returns at once.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kDsThreads = 256;
constexpr int kDsItems = 16;                       // members per lane in a tile
constexpr int kDsTile = kDsThreads * kDsItems;     // 4096
constexpr int kDsWaves = kDsThreads / 64;
constexpr int kDsRadix = 256;
constexpr int kDsMaxPasses = 8;
constexpr int kDsScanThreads = 1024;
constexpr double kDsIntMax = 2147483647.0;

struct DsPlan {
  int32_t abort;    // a status bit was set: later kernels do nothing
  int32_t passes;   // 8-bit digit passes the keys need
  int32_t bx, by, bz;
  int32_t voxels;   // V, written by k_ds_tiles
};

struct DsWork {
  int32_t* mpre;       // [C + 1] member prefix
  double* lo;          // [C, 3]
  double* kmax;        // [C, 3] largest key per axis, as a double (floor value)
  int32_t* flags;      // [C] DPC_STATUS_* bits of the cloud
  DsPlan* plan;
  uint64_t* keys[2];   // [M]
  int32_t* rows[2];    // [M] input row of the member
  int32_t* hist;       // [256, tiles] digit counts per tile
  int32_t* hist_off;   // [256, tiles] their exclusive scan along the tiles
  int32_t* digit_total;  // [256]
  int32_t* tile_heads;   // [tiles] voxels starting in the tile
  int32_t* tile_off;     // [tiles] their exclusive scan
  int32_t* vstart;       // [M + 1] first sorted position of each voxel, vstart[V] = M
};

inline int64_t ds_tiles(int64_t members) { return (members + kDsTile - 1) / kDsTile; }

size_t ds_carve(int clouds, int64_t members, char* base, DsWork* w) {
  Carver c{base};
  const size_t C = (size_t)clouds, M = (size_t)members, T = (size_t)ds_tiles(members);
  DsWork t;
  t.mpre = c.take<int32_t>(C + 1);
  t.lo = c.take<double>(3 * C);
  t.kmax = c.take<double>(3 * C);
  t.flags = c.take<int32_t>(C);
  t.plan = c.take<DsPlan>(1);
  for (int k = 0; k < 2; ++k) t.keys[k] = c.take<uint64_t>(M);
  for (int k = 0; k < 2; ++k) t.rows[k] = c.take<int32_t>(M);
  t.hist = c.take<int32_t>((size_t)kDsRadix * T);
  t.hist_off = c.take<int32_t>((size_t)kDsRadix * T);
  t.digit_total = c.take<int32_t>(kDsRadix);
  t.tile_heads = c.take<int32_t>(T);
  t.tile_off = c.take<int32_t>(T);
  t.vstart = c.take<int32_t>(M + 1);
  if (w) *w = t;
  return c.off;
}

__device__ inline int ds_bits(double v) {  // bits to hold the integer v in [0, 2^31)
  int b = 0;
  while (b < 31 && (double)(1u << b) <= v) ++b;
  return b;
}

template <class T>
__global__ __launch_bounds__(kDsThreads) void k_ds_bounds(const T* __restrict__ pts, const int32_t* __restrict__ desc,
                                                          double vs, DsWork w) {
  __shared__ double smin[3][kDsThreads], smax[3][kDsThreads];
  __shared__ int sbad[kDsThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  const int start = desc[2 * c], count = desc[2 * c + 1];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int i = t; i < count; i += kDsThreads) {
    const T* p = pts + 3 * ((size_t)start + i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = (double)p[k];
      bad |= !isfinite(x);
      mn[k] = fmin(mn[k], x);
      mx[k] = fmax(mx[k], x);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { smin[k][t] = mn[k]; smax[k][t] = mx[k]; }
  sbad[t] = bad;
  __syncthreads();
  for (int s = kDsThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        smin[k][t] = fmin(smin[k][t], smin[k][t + s]);
        smax[k][t] = fmax(smax[k][t], smax[k][t + s]);
      }
      sbad[t] |= sbad[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  int flags = sbad[0] ? DPC_STATUS_NONFINITE : 0;
  double range = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double lo_k = count > 0 ? smin[k][0] : 0.0, hi_k = count > 0 ? smax[k][0] : 0.0;  // empty: bounds are 0
    const double lo = lo_k - vs * 0.5, hi = hi_k + vs * 0.5;
    range = fmax(range, hi - lo);
    w.lo[3 * c + k] = lo;
    w.kmax[3 * c + k] = count > 0 ? floor((hi_k - lo) / vs) : 0.0;
  }
  if (vs * kDsIntMax < range) flags |= DPC_STATUS_VOXEL_TOO_SMALL;  // open3d: "voxel_size is too small"
  w.flags[c] = flags;
}

__global__ __launch_bounds__(kDsScanThreads) void k_ds_plan(const int32_t* __restrict__ desc, int clouds, DsWork w,
                                                            int32_t* __restrict__ status) {
  __shared__ int scratch[kDsScanThreads / 64 + 1];
  __shared__ double smax[3][kDsScanThreads];
  __shared__ int sflags[kDsScanThreads];
  const int t = threadIdx.x;
  const int seg = (clouds + kDsScanThreads - 1) / kDsScanThreads;
  const int c0 = min(clouds, t * seg), c1 = min(clouds, c0 + seg);
  int loc = 0, fl = 0;
  double km[3] = {0.0, 0.0, 0.0};
  for (int c = c0; c < c1; ++c) {
    loc += desc[2 * c + 1];
    fl |= w.flags[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) km[k] = fmax(km[k], w.kmax[3 * c + k]);  // NaN (a non-finite cloud) is dropped
  }
  int run;
  const int total = block_scan<kDsScanThreads>(loc, &run, scratch);
  for (int c = c0; c < c1; ++c) { w.mpre[c] = run; run += desc[2 * c + 1]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) smax[k][t] = km[k];
  sflags[t] = fl;
  __syncthreads();
  for (int s = kDsScanThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) smax[k][t] = fmax(smax[k][t], smax[k][t + s]);
      sflags[t] |= sflags[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  w.mpre[clouds] = total;
  int flags = sflags[0];
  DsPlan plan{0, 0, 0, 0, 0, 0};
  if (!flags && (smax[0][0] > kDsIntMax || smax[1][0] > kDsIntMax || smax[2][0] > kDsIntMax))
    flags |= DPC_STATUS_KEY_OVERFLOW;  // open3d's int(floor(...)) would overflow
  if (!flags) {
    plan.bx = ds_bits(smax[0][0]);
    plan.by = ds_bits(smax[1][0]);
    plan.bz = ds_bits(smax[2][0]);
    const int bits = ds_bits((double)(clouds - 1)) + plan.bx + plan.by + plan.bz;
    if (bits > 64) flags |= DPC_STATUS_KEY_OVERFLOW;
    plan.passes = (bits + 7) / 8;
  }
  if (flags) {
    plan.abort = 1;
    plan.passes = 0;
    if (status) atomicOr(status, flags);
  }
  *w.plan = plan;
}

template <class T>
__global__ __launch_bounds__(kDsThreads) void k_ds_keys(const T* __restrict__ pts, const int32_t* __restrict__ desc,
                                                        int clouds, int members, double vs, DsWork w) {
  const DsPlan plan = *w.plan;
  if (plan.abort) return;
  for (int m = blockIdx.x * kDsThreads + threadIdx.x; m < members; m += gridDim.x * kDsThreads) {
    const int c = owner(w.mpre, clouds, m);
    const int row = desc[2 * c] + (m - w.mpre[c]);
    const T* p = pts + 3 * (size_t)row;
    uint64_t key = (uint64_t)c;
    const int bits[3] = {plan.bx, plan.by, plan.bz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double q = floor(((double)p[k] - w.lo[3 * c + k]) / vs);  // subtract, then an IEEE division
      key = (key << bits[k]) | (uint64_t)(uint32_t)q;                  // 0 <= q <= kmax < 2^bits (monotonic)
    }
    w.keys[0][m] = key;
    w.rows[0][m] = row;
  }
}

__device__ inline int ds_digit(uint64_t key, int pass) { return (int)((key >> (8 * pass)) & 0xff); }

__global__ __launch_bounds__(kDsThreads) void k_ds_hist(int members, int pass, DsWork w) {
  __shared__ int h[kDsRadix];
  const DsPlan* plan = w.plan;
  if (pass >= plan->passes) return;
  const uint64_t* __restrict__ keys = w.keys[pass & 1];
  const int t = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x;
  h[t] = 0;
  __syncthreads();
  const int64_t base = (int64_t)tile * kDsTile;
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = base + j * kDsThreads + t;
    if (i < members) atomicAdd(&h[ds_digit(keys[i], pass)], 1);
  }
  __syncthreads();
  w.hist[(size_t)t * tiles + tile] = h[t];
}

// One block per digit: the exclusive scan of its row of tile counts, and the digit's total.
__global__ __launch_bounds__(kDsScanThreads) void k_ds_digits(int tiles, int pass, DsWork w) {
  __shared__ int scratch[kDsScanThreads / 64 + 1];
  if (pass >= w.plan->passes) return;
  const int32_t* row = w.hist + (size_t)blockIdx.x * tiles;
  int32_t* off = w.hist_off + (size_t)blockIdx.x * tiles;
  int run = 0;
  for (int b0 = 0; b0 < tiles; b0 += kDsScanThreads) {
    const int b = b0 + threadIdx.x;
    const int v = b < tiles ? row[b] : 0;
    int excl;
    const int total = block_scan<kDsScanThreads>(v, &excl, scratch);
    if (b < tiles) off[b] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) w.digit_total[blockIdx.x] = run;
}

// Stable scatter of one tile.  Wave v owns members [v * 1024, (v + 1) * 1024) of the tile and walks them 64 at a time:
// the lanes holding the same digit are found with 8 ballots, a lane's rank is the wave's running count of its digit plus
// the lower lanes of its group.  The waves' counts are then prefixed in wave order, so ranks follow member order.
__global__ __launch_bounds__(kDsThreads) void k_ds_scatter(int members, int pass, DsWork w) {
  __shared__ int wcnt[kDsWaves][kDsRadix];
  __shared__ int base[kDsRadix];
  __shared__ int scratch[kDsThreads / 64 + 1];
  if (pass >= w.plan->passes) return;
  const uint64_t* __restrict__ kin = w.keys[pass & 1];
  const int32_t* __restrict__ rin = w.rows[pass & 1];
  uint64_t* __restrict__ kout = w.keys[(pass + 1) & 1];
  int32_t* __restrict__ rout = w.rows[(pass + 1) & 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, tile = blockIdx.x, tiles = gridDim.x;
  for (int v = 0; v < kDsWaves; ++v) wcnt[v][t] = 0;
  // digit d starts at (members of smaller digits) + (members of digit d in earlier tiles)
  const int total_d = w.digit_total[t];
  int excl;
  block_scan<kDsThreads>(total_d, &excl, scratch);
  base[t] = excl + w.hist_off[(size_t)t * tiles + tile];
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1;
  uint64_t key[kDsItems];
  int32_t row[kDsItems];
  int rank[kDsItems];
  const int64_t first = (int64_t)tile * kDsTile + wave * (kDsItems * 64);
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = first + j * 64 + lane;
    const bool live = i < members;
    key[j] = live ? kin[i] : 0;
    row[j] = live ? rin[i] : 0;
    const int d = ds_digit(key[j], pass);
    uint64_t same = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t ones = __ballot((d >> b) & 1);
      same &= ((d >> b) & 1) ? ones : ~ones;
    }
    int r = 0;
    if (live) r = wcnt[wave][d] + __popcll(same & below);
    __builtin_amdgcn_wave_barrier();
    if (live && (same & below) == 0) wcnt[wave][d] += __popcll(same);  // the group's lowest lane counts it
    __builtin_amdgcn_wave_barrier();
    rank[j] = r;
  }
  __syncthreads();
  {  // digit t: the waves' counts prefixed in wave order
    int run = base[t];
    for (int v = 0; v < kDsWaves; ++v) { const int n = wcnt[v][t]; wcnt[v][t] = run; run += n; }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = first + j * 64 + lane;
    if (i < members) {
      const int dst = wcnt[wave][ds_digit(key[j], pass)] + rank[j];
      kout[dst] = key[j];
      rout[dst] = row[j];
    }
  }
}

__device__ inline bool ds_head(const uint64_t* __restrict__ keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

__global__ __launch_bounds__(kDsThreads) void k_ds_heads(int members, DsWork w) {
  __shared__ int scratch[kDsThreads / 64 + 1];
  const DsPlan plan = *w.plan;
  if (plan.abort) return;
  const uint64_t* __restrict__ keys = w.keys[plan.passes & 1];
  const int64_t first = (int64_t)blockIdx.x * kDsTile + threadIdx.x * kDsItems;
  int n = 0;
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = first + j;
    if (i < members) n += ds_head(keys, i);
  }
  int excl;
  const int total = block_scan<kDsThreads>(n, &excl, scratch);
  if (threadIdx.x == 0) w.tile_heads[blockIdx.x] = total;
}

__global__ __launch_bounds__(kDsScanThreads) void k_ds_tiles(int tiles, int members, DsWork w) {
  __shared__ int scratch[kDsScanThreads / 64 + 1];
  if (w.plan->abort) return;
  int run = 0;
  for (int b0 = 0; b0 < tiles; b0 += kDsScanThreads) {
    const int b = b0 + threadIdx.x;
    const int v = b < tiles ? w.tile_heads[b] : 0;
    int excl;
    const int total = block_scan<kDsScanThreads>(v, &excl, scratch);
    if (b < tiles) w.tile_off[b] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) {
    w.plan->voxels = run;
    w.vstart[run] = members;
  }
}

__global__ __launch_bounds__(kDsThreads) void k_ds_voxels(int members, DsWork w) {
  __shared__ int scratch[kDsThreads / 64 + 1];
  const DsPlan plan = *w.plan;
  if (plan.abort) return;
  const uint64_t* __restrict__ keys = w.keys[plan.passes & 1];
  const int64_t first = (int64_t)blockIdx.x * kDsTile + threadIdx.x * kDsItems;
  int n = 0;
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = first + j;
    if (i < members) n += ds_head(keys, i);
  }
  int excl;
  block_scan<kDsThreads>(n, &excl, scratch);
  int v = w.tile_off[blockIdx.x] + excl;
  for (int j = 0; j < kDsItems; ++j) {
    const int64_t i = first + j;
    if (i < members && ds_head(keys, i)) w.vstart[v++] = (int32_t)i;
  }
}

// acc = 0; acc += p for each member in input order (AccumulatedPoint::AddPoint); out = acc / double(n).  One lane runs
// a voxel's whole chain: splitting it would change the order of the adds.  The loads of 8 members are issued before
// their adds, so a long chain waits on memory once per 8 members, not once per member.
constexpr int kDsBatch = 8;

template <class T>
__global__ __launch_bounds__(kDsThreads) void k_ds_average(const T* __restrict__ pts, DsWork w, double* __restrict__ out) {
  const DsPlan plan = *w.plan;
  if (plan.abort) return;
  const int32_t* __restrict__ rows = w.rows[plan.passes & 1];
  for (int v = blockIdx.x * kDsThreads + threadIdx.x; v < plan.voxels; v += gridDim.x * kDsThreads) {
    const int i0 = w.vstart[v], i1 = w.vstart[v + 1];
    double ax = 0.0, ay = 0.0, az = 0.0;
    int i = i0;
    for (; i + kDsBatch <= i1; i += kDsBatch) {
      T x[kDsBatch], y[kDsBatch], z[kDsBatch];
#pragma unroll
      for (int k = 0; k < kDsBatch; ++k) {
        const T* p = pts + 3 * (size_t)rows[i + k];
        x[k] = p[0]; y[k] = p[1]; z[k] = p[2];
      }
#pragma unroll
      for (int k = 0; k < kDsBatch; ++k) { ax += (double)x[k]; ay += (double)y[k]; az += (double)z[k]; }
    }
    for (; i < i1; ++i) {
      const T* p = pts + 3 * (size_t)rows[i];
      ax += (double)p[0];
      ay += (double)p[1];
      az += (double)p[2];
    }
    const double n = (double)(i1 - i0);
    out[3 * (size_t)v] = ax / n;
    out[3 * (size_t)v + 1] = ay / n;
    out[3 * (size_t)v + 2] = az / n;
  }
}

__device__ inline int ds_lower_bound(const int32_t* __restrict__ a, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kDsThreads) void k_ds_clouds(int clouds, DsWork w, int32_t* __restrict__ out_count,
                                                          int32_t* __restrict__ out_offset) {
  const int c = blockIdx.x * kDsThreads + threadIdx.x;
  if (c >= clouds) return;
  const DsPlan plan = *w.plan;
  if (plan.abort) {
    out_count[c] = 0;
    out_offset[c] = 0;
    return;
  }
  // a cloud's members are contiguous in the sorted order (the slot is the key's top field), its first one a voxel start
  const int a = ds_lower_bound(w.vstart, plan.voxels, w.mpre[c]);
  const int b = ds_lower_bound(w.vstart, plan.voxels, w.mpre[c + 1]);
  out_offset[c] = a;
  out_count[c] = b - a;
}

inline unsigned ds_grid(int64_t members) {
  const int64_t b = (members + kDsThreads - 1) / kDsThreads;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

template <class T>
int ds_impl(const T* pts, const int32_t* desc, int clouds, int members, double vs, double* out, int32_t* out_count,
            int32_t* out_offset, int32_t* status, void* workspace, hipStream_t st) {
  DsWork w;
  ds_carve(clouds, members, static_cast<char*>(workspace), &w);
  constexpr bool kF64 = sizeof(T) == sizeof(double);
  const int tiles = (int)ds_tiles(members);
  DPC_LAUNCH("k_ds_bounds", dpc_kid(kF64 ? "k_ds_bounds<double>" : "k_ds_bounds<float>"), k_ds_bounds<T>, dim3(clouds),
             dim3(kDsThreads), 0, st, pts, desc, vs, w);
  DPC_LAUNCH("k_ds_plan", dpc_kid("k_ds_plan"), k_ds_plan, dim3(1), dim3(kDsScanThreads), 0, st, desc, clouds, w, status);
  if (members > 0) {
    DPC_LAUNCH("k_ds_keys", dpc_kid(kF64 ? "k_ds_keys<double>" : "k_ds_keys<float>"), k_ds_keys<T>, dim3(ds_grid(members)),
               dim3(kDsThreads), 0, st, pts, desc, clouds, members, vs, w);
    for (int pass = 0; pass < kDsMaxPasses; ++pass) {  // the plan's count is on the device: surplus passes return at once
      DPC_LAUNCH("k_ds_hist", dpc_kid("k_ds_hist"), k_ds_hist, dim3(tiles), dim3(kDsThreads), 0, st, members, pass, w);
      DPC_LAUNCH("k_ds_digits", dpc_kid("k_ds_digits"), k_ds_digits, dim3(kDsRadix), dim3(kDsScanThreads), 0, st, tiles,
                 pass, w);
      DPC_LAUNCH("k_ds_scatter", dpc_kid("k_ds_scatter"), k_ds_scatter, dim3(tiles), dim3(kDsThreads), 0, st, members,
                 pass, w);
    }
    DPC_LAUNCH("k_ds_heads", dpc_kid("k_ds_heads"), k_ds_heads, dim3(tiles), dim3(kDsThreads), 0, st, members, w);
    DPC_LAUNCH("k_ds_tiles", dpc_kid("k_ds_tiles"), k_ds_tiles, dim3(1), dim3(kDsScanThreads), 0, st, tiles, members, w);
    DPC_LAUNCH("k_ds_voxels", dpc_kid("k_ds_voxels"), k_ds_voxels, dim3(tiles), dim3(kDsThreads), 0, st, members, w);
    DPC_LAUNCH("k_ds_average", dpc_kid(kF64 ? "k_ds_average<double>" : "k_ds_average<float>"), k_ds_average<T>,
               dim3(ds_grid(members)), dim3(kDsThreads), 0, st, pts, w, out);
  }
  DPC_LAUNCH("k_ds_clouds", dpc_kid("k_ds_clouds"), k_ds_clouds, dim3((clouds + kDsThreads - 1) / kDsThreads),
             dim3(kDsThreads), 0, st, clouds, w, out_count, out_offset);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_downsample_workspace_bytes(int clouds, int members) {
  if (clouds <= 0 || members < 0 || members > INT32_MAX - 1) return 0;
  return ds_carve(clouds, members, nullptr, nullptr);
}

int dpc_voxel_downsample(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc,
                         const int32_t* host_cloud_desc, int clouds, double voxel_size, double* out, int32_t* out_count,
                         int32_t* out_offset, int32_t* status, void* workspace, void* stream) {
  if (clouds < 0 || n_pts < 0 || !(voxel_size > 0.0) || !std::isfinite(voxel_size)) return DPC_ERR_SHAPE;
  if (clouds == 0) return DPC_OK;
  if (!host_cloud_desc) return DPC_ERR_NULL;
  int64_t members = 0;
  // members are indexed by int32, and vstart holds M + 1 of them
  const int rc = check_desc<2>(host_cloud_desc, clouds, {(int64_t)n_pts}, INT32_MAX - 1, &members,
                               [](const int32_t*) { return true; });
  if (rc != DPC_OK) return rc;
  if (!cloud_desc || !out_count || !out_offset || !workspace || (members > 0 && (!pts || !out))) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return ds_impl<double>(static_cast<const double*>(pts), cloud_desc, clouds, (int)members, voxel_size, out, out_count,
                           out_offset, status, workspace, st);
  return ds_impl<float>(static_cast<const float*>(pts), cloud_desc, clouds, (int)members, voxel_size, out, out_count,
                        out_offset, status, workspace, st);
}

}  // extern "C"
