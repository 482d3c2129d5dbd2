// Voxel-grid evaluation: clouds and float grids to bit grids, the five counts of evaluate_voxel_prediction per pair of
// bit grids, and bit grids back to points (voxel2pc).  The contract (grid layout, the nearest-node rule, the bit layout,
// the thresholds, the counts, voxel2pc's axis order and coordinates, guards) is in include/dpc_render.h (dpc_voxelise).
// Everything is integer- or bit-exact: bit-OR and popcount do not depend on order, the fp64 arithmetic is elementwise.
//
// k_voxelise<F64, WORDS, THREADS>   a workgroup owns WORDS consecutive words of one cloud's bit grid (the whole grid in
//     classes 0 and 1; in class 2 a slab of 16384 words = 2^19 voxels, i.e. 32 z-planes of a 128^3 grid, and a cloud has
//     ceil(words / 16384) workgroups).  It zeroes the words in LDS, reads every point of the cloud, ORs the bits that
//     fall into its words with LDS atomics and writes the finished words with plain coalesced stores: no word of the
//     output belongs to two workgroups, so there is no global atomic but the OR into the status word.  Slab 0 of a
//     cloud counts the points it dropped and reports a non-finite coordinate.
//       class   words of the grid     LDS per workgroup   threads   largest cubic grid
//         0        1 .. 1024            4 KiB + 16 B        256        32^3
//         1     1025 .. 8192           32 KiB + 16 B        512        64^3
//         2     8193 .. 65536          64 KiB + 16 B       1024       128^3 (4 slabs); 2 workgroups share a CU
// k_voxel_threshold<DT>   one wave per 64 consecutive voxels of a grid: a coalesced load, the compare in the grid's own
//     dtype, one ballot = two words.  DT 0 fp32, 1 fp64, 2 uint8 (occupied = non-zero: bool grids).
// k_voxel_unpack          bit grids to one byte per voxel (the bool tensors of the Python layer), four voxels a thread.
// k_voxel_stats           one workgroup per (pred, gt) pair: popcounts of p & g, p & ~g, ~p & g summed per thread, then
//     per wave by shuffles, then over the waves by thread 0 in wave order (integers: any order gives the same sums).
// k_voxel_count           one workgroup per grid: its number of set bits.
// k_voxel2pc              one workgroup per grid: 256 words a round, block_scan of their popcounts gives every word its
//     place, each thread writes the points of its word in ascending bit order: ascending flat index overall.
// Nothing waits on another workgroup; every loop is bounded by a host-checked size or a checked table entry.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"
#include "dpc_voxel_bits.h"

namespace {

constexpr int kVxClasses = 3;
constexpr int kVxWords[kVxClasses] = {1024, 8192, 16384};     // words of a workgroup
constexpr int kVxThreads[kVxClasses] = {256, 512, 1024};
constexpr int kVxExtra = 4;                                   // ints behind the words: dropped, non-finite (+ 2 pad)
static_assert((int64_t)DPC_VOXEL_MAX_SIDE * DPC_VOXEL_MAX_SIDE * DPC_VOXEL_MAX_SIDE <= INT32_MAX, "a flat voxel index is an int");

constexpr int vx_class(int64_t words) { return words <= kVxWords[0] ? 0 : words <= kVxWords[1] ? 1 : 2; }
static_assert(vx_class(32 * 32 * 32 / 32) == 0 && vx_class(32 * 32 * 32 / 32 + 1) == 1 && vx_class(64 * 64 * 64 / 32) == 1 &&
                  vx_class(64 * 64 * 64 / 32 + 1) == 2, "32^3 is the largest grid of class 0, 64^3 of class 1");

// the node of coordinate a on an axis of G nodes; a is inside [-0.5, 0.5]
__device__ inline int vx_node(double a, int G) {
  const double t = (a + 0.5) * (double)(G - 1);
  const int i = (int)floor(t + 0.5);
  return i < 0 ? 0 : i > G - 1 ? G - 1 : i;  // cannot change a result: 0 <= t <= G - 1 for a valid point
}

template <int F64, int WORDS, int THREADS>
__global__ __launch_bounds__(THREADS) void k_voxelise(const void* __restrict__ pts_, int n_pts, const int32_t* __restrict__ desc,
                                                      int slabs, int D, int H, int W, int words, uint32_t* __restrict__ bits,
                                                      int32_t* __restrict__ dropped, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  using T = std::conditional_t<F64 != 0, double, float>;
  extern __shared__ __attribute__((aligned(16))) uint32_t vx_smem[];  // [WORDS] bits, then dropped, non-finite
  int* const extra = reinterpret_cast<int*>(vx_smem + WORDS);
  const T* __restrict__ pts = static_cast<const T*>(pts_);
  const int t = threadIdx.x;
  const int cloud = blockIdx.x / slabs, slab = blockIdx.x - cloud * slabs;
  const int w0 = slab * WORDS;
  const int nw = words - w0 < WORDS ? words - w0 : WORDS;

  const int start = desc[2 * (size_t)cloud], count = desc[2 * (size_t)cloud + 1];
  // nothing of the device table becomes an address or a loop bound before it passed this
  if (!(start >= 0 && count >= 0 && (int64_t)start + count <= n_pts)) {
    if (slab == 0 && t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  for (int j = t; j < nw; j += THREADS) vx_smem[j] = 0u;
  if (t < kVxExtra) extra[t] = 0;
  __syncthreads();

  int drop = 0;
  bool bad = false;
  for (int i = t; i < count; i += THREADS) {
    const T* p = pts + 3 * ((size_t)start + i);
    const double a = (double)p[0], b = (double)p[1], c = (double)p[2];
    bad |= !(__builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c));
    // false for a NaN: an index is never formed from an invalid point
    const bool in = a >= -0.5 && a <= 0.5 && b >= -0.5 && b <= 0.5 && c >= -0.5 && c <= 0.5;
    if (in) {
      const int f = (vx_node(a, D) * H + vx_node(b, H)) * W + vx_node(c, W);
      const int w = (f >> 5) - w0;
      if ((unsigned)w < (unsigned)nw) atomicOr(&vx_smem[w], 1u << (f & 31));
    } else {
      ++drop;
    }
  }
  if (slab == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) drop += __shfl_down(drop, off, 64);
    if ((t & 63) == 0 && drop) atomicAdd(&extra[0], drop);
    if (bad) extra[1] = 1;
  }
  __syncthreads();
  uint32_t* out = bits + (size_t)cloud * words + w0;
  for (int j = t; j < nw; j += THREADS) out[j] = vx_smem[j];
  if (slab == 0 && t == 0) {
    dropped[cloud] = extra[0];
    if (extra[1] && status) atomicOr(status, (int)DPC_STATUS_NONFINITE);
  }
}

constexpr int kVxChunks = 4;  // chunks of 64 voxels a wave has in flight

template <int DT>
__global__ __launch_bounds__(256) void k_voxel_threshold(const void* __restrict__ grids_, int B, int V, int words, double threshold,
                                                         int inclusive, uint32_t* __restrict__ bits) {
  using T = std::conditional_t<DT == 0, float, std::conditional_t<DT == 1, double, uint8_t>>;
  const T* __restrict__ grids = static_cast<const T*>(grids_);
  const T thr = DT == 2 ? (T)0 : (T)threshold;  // the threshold rounded to the grid's dtype (none for uint8)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = (V + 63) / 64;
  const int c0 = (blockIdx.x * 4 + wave) * kVxChunks;
  if (c0 >= nchunk) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const T* g = grids + (size_t)b * V;
    uint32_t* out = bits + (size_t)b * words;
    T v[kVxChunks];
#pragma unroll
    for (int k = 0; k < kVxChunks; ++k) {
      const int vox = (c0 + k) * 64 + lane;
      v[k] = vox < V ? g[vox] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kVxChunks; ++k) {
      const int vox = (c0 + k) * 64 + lane;
      bool occ;
      if (DT == 2) occ = v[k] != (T)0;
      else occ = inclusive ? v[k] >= thr : v[k] > thr;  // false for a NaN voxel, and for a NaN threshold
      const unsigned long long m = __ballot(occ && vox < V);
      const int j = 2 * (c0 + k) + lane;  // lanes 0 and 1 store the two words
      if (lane < 2 && j < words) out[j] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
  }
}

__global__ __launch_bounds__(256) void k_voxel_unpack(const uint32_t* __restrict__ bits, int B, int V, int words,
                                                      uint8_t* __restrict__ out) {
  const int vox = 4 * (blockIdx.x * 256 + threadIdx.x);  // four voxels a thread: bits vox & 31 .. + 3 of one word
  if (vox >= V) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const uint32_t nib = bits[(size_t)b * words + (vox >> 5)] >> (vox & 31);
    uint8_t* o = out + (size_t)b * V + vox;
    if ((V & 3) == 0) {  // every grid starts on a multiple of four bytes: one store
      *reinterpret_cast<uint32_t*>(o) = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
    } else {
      for (int k = 0; k < 4 && vox + k < V; ++k) o[k] = (uint8_t)((nib >> k) & 1u);
    }
  }
}

__global__ __launch_bounds__(256) void k_voxel_stats(const uint32_t* __restrict__ pred, int n_pred, const uint32_t* __restrict__ gt,
                                                     int n_gt, int V, int words, const int32_t* __restrict__ pair_desc,
                                                     long long* __restrict__ stats, int32_t* __restrict__ status) {
  __shared__ int scratch[4];
  const int t = threadIdx.x;
  const int pi = pair_desc[2 * (size_t)blockIdx.x], gi = pair_desc[2 * (size_t)blockIdx.x + 1];
  if (!(pi >= 0 && pi < n_pred && gi >= 0 && gi < n_gt)) {  // not read, its row left as it was
    if (t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  const uint32_t* p = pred + (size_t)pi * words;
  const uint32_t* g = gt + (size_t)gi * words;
  int both = 0, fp = 0, fn = 0;
#pragma unroll 4
  for (int j = t; j < words; j += 256) {
    const uint32_t a = voxel_word(p, j, words, V), b = voxel_word(g, j, words, V);
    both += __popc(a & b);
    fp += __popc(a & ~b);
    fn += __popc(~a & b);
  }
  const long long s_both = block_sum<256, long long>(both, scratch);
  const long long s_fp = block_sum<256, long long>(fp, scratch);
  const long long s_fn = block_sum<256, long long>(fn, scratch);
  if (t == 0) {
    long long* row = stats + 5 * (size_t)blockIdx.x;
    row[0] = s_fp + s_fn;           // diff = popcount(p ^ g)
    row[1] = s_both;                // intersection
    row[2] = s_both + s_fp + s_fn;  // union
    row[3] = s_fp;
    row[4] = s_fn;
  }
}

__global__ __launch_bounds__(256) void k_voxel_count(const uint32_t* __restrict__ bits, int V, int words, int32_t* __restrict__ counts) {
  __shared__ int scratch[4];
  const uint32_t* w = bits + (size_t)blockIdx.x * words;
  int n = 0;
#pragma unroll 4
  for (int j = threadIdx.x; j < words; j += 256) n += __popc(voxel_word(w, j, words, V));
  const long long s = block_sum<256, long long>(n, scratch);
  if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)s;
}

__global__ __launch_bounds__(256) void k_voxel2pc(const uint32_t* __restrict__ bits, int G, int V, int words,
                                                  const int32_t* __restrict__ out_desc, int n_out, double* __restrict__ xyz,
                                                  int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ int scratch[256 / 64 + 1];
  const int t = threadIdx.x;
  const int start = out_desc[2 * (size_t)blockIdx.x], count = out_desc[2 * (size_t)blockIdx.x + 1];
  if (!(start >= 0 && count >= 0 && (int64_t)start + count <= n_out)) {
    if (t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  const uint32_t* w = bits + (size_t)blockIdx.x * words;
  const double step = 1.0 / (double)(G - 1);
  int base = 0;
  for (int j0 = 0; j0 < words; j0 += 256) {  // the same trip count in every thread: block_scan has barriers
    const int j = j0 + t;
    uint32_t m = j < words ? voxel_word(w, j, words, V) : 0u;
    int excl;
    const int total = block_scan<256>((int)__popc(m), &excl, scratch);
    int o = base + excl;
    while (m) {
      const int f = j * 32 + __builtin_ctz(m);
      m &= m - 1u;
      if (o < count) {  // a point beyond the range the table gives this grid is not written
        const int k = f % G, q = f / G;
        const int jj = q % G, i = q / G;
        double* p = xyz + 3 * ((size_t)start + o);
        // np.linspace(-0.5, 0.5, G): arange(G) * step + start, the last one set to the stop; 'xy' meshgrid: (x[j], x[i], x[k])
        p[0] = jj == G - 1 ? 0.5 : (double)jj * step + (-0.5);
        p[1] = i == G - 1 ? 0.5 : (double)i * step + (-0.5);
        p[2] = k == G - 1 ? 0.5 : (double)k * step + (-0.5);
      }
      ++o;
    }
    base += total;
  }
  if (t == 0 && base != count && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);  // the table is not this grid's count
}

template <int F64, int CLS>
int vx_launch(const void* pts, int n_pts, const int32_t* desc, int clouds, const VoxelGrid& g, uint32_t* bits, int32_t* dropped,
              int32_t* status, hipStream_t st) {
  constexpr int WORDS = kVxWords[CLS], THREADS = kVxThreads[CLS];
  constexpr size_t lds = sizeof(uint32_t) * (WORDS + kVxExtra);
  static_assert(lds <= 80 * 1024, "two workgroups share the CU's 160 KiB of LDS");
  static LdsLimit limit;
  const int rc = set_lds(k_voxelise<F64, WORDS, THREADS>, lds, limit);
  if (rc != DPC_OK) return rc;
  const int slabs = (g.words + WORDS - 1) / WORDS;
  DPC_LAUNCH("k_voxelise", dpc_kid("k_voxelise", F64, WORDS, THREADS), (k_voxelise<F64, WORDS, THREADS>),
             dim3((unsigned)clouds * (unsigned)slabs), dim3(THREADS), lds, st, pts, n_pts, desc, slabs, g.D, g.H, g.W, g.words, bits,
             dropped, status);
  return launch_ok();
}

template <int F64>
int vx_run(const void* pts, int n_pts, const int32_t* desc, int clouds, const VoxelGrid& g, uint32_t* bits, int32_t* dropped,
           int32_t* status, hipStream_t st) {
  switch (vx_class(g.words)) {
    case 0: return vx_launch<F64, 0>(pts, n_pts, desc, clouds, g, bits, dropped, status, st);
    case 1: return vx_launch<F64, 1>(pts, n_pts, desc, clouds, g, bits, dropped, status, st);
    default: return vx_launch<F64, 2>(pts, n_pts, desc, clouds, g, bits, dropped, status, st);
  }
}

template <int DT>
int vx_threshold(const void* grids, int B, const VoxelGrid& g, double threshold, int inclusive, uint32_t* bits, hipStream_t st) {
  const int nchunk = (g.V + 63) / 64;
  const dim3 grid((unsigned)((nchunk + 4 * kVxChunks - 1) / (4 * kVxChunks)), (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_voxel_threshold", dpc_kid("k_voxel_threshold", DT), (k_voxel_threshold<DT>), grid, dim3(256), 0, st, grids, B, g.V,
             g.words, threshold, inclusive, bits);
  return launch_ok();
}

}  // namespace

extern "C" {

int dpc_voxelise(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc, const int32_t* host_cloud_desc, int clouds,
                 int D, int H, int W, uint32_t* bits, int32_t* dropped, int32_t* status, void* stream) {
  VoxelGrid g;
  if (n_pts < 0 || clouds < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (clouds > 0 && !host_cloud_desc) return DPC_ERR_NULL;
  const int64_t len[1] = {n_pts};
  const int rc = check_desc<2, 1>(host_cloud_desc, clouds, len, INT32_MAX, nullptr, [](const int32_t*) { return true; });
  if (rc != DPC_OK) return rc;
  const int64_t slabs = (g.words + kVxWords[vx_class(g.words)] - 1) / kVxWords[vx_class(g.words)];
  if (clouds * slabs > INT32_MAX) return DPC_ERR_SHAPE;
  if (clouds == 0) return DPC_OK;
  if ((!pts && n_pts > 0) || !cloud_desc || !bits || !dropped) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  return is_f64 ? vx_run<1>(pts, n_pts, cloud_desc, clouds, g, bits, dropped, status, st)
                : vx_run<0>(pts, n_pts, cloud_desc, clouds, g, bits, dropped, status, st);
}

int dpc_voxel_threshold(const void* grids, int dtype, int B, int D, int H, int W, double threshold, int inclusive, uint32_t* bits,
                        void* stream) {
  VoxelGrid g;
  if (B < 0 || dtype < 0 || dtype > 2 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!grids || !bits) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  return dtype == 0 ? vx_threshold<0>(grids, B, g, threshold, inclusive != 0, bits, st)
       : dtype == 1 ? vx_threshold<1>(grids, B, g, threshold, inclusive != 0, bits, st)
                    : vx_threshold<2>(grids, B, g, threshold, inclusive != 0, bits, st);
}

int dpc_voxel_unpack(const uint32_t* bits, int B, int D, int H, int W, uint8_t* out, void* stream) {
  VoxelGrid g;
  if (B < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!bits || !out) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return DPC_ERR_SHAPE;  // the four-voxel stores need it
  const dim3 grid((unsigned)((g.V + 1023) / 1024), (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_voxel_unpack", dpc_kid("k_voxel_unpack"), k_voxel_unpack, grid, dim3(256), 0, st, bits, B, g.V, g.words, out);
  return launch_ok();
}

int dpc_voxel_stats(const uint32_t* pred_bits, int n_pred, const uint32_t* gt_bits, int n_gt, int D, int H, int W,
                    const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs, int64_t* stats, int32_t* status,
                    void* stream) {
  VoxelGrid g;
  if (n_pred < 0 || n_gt < 0 || pairs < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (pairs > 0 && !host_pair_desc) return DPC_ERR_NULL;
  const int rc = check_pairs(host_pair_desc, pairs, n_pred, n_gt);
  if (rc != DPC_OK) return rc;
  if (pairs == 0) return DPC_OK;
  if (!pred_bits || !gt_bits || !pair_desc || !stats) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_voxel_stats", dpc_kid("k_voxel_stats"), k_voxel_stats, dim3((unsigned)pairs), dim3(256), 0, st, pred_bits, n_pred,
             gt_bits, n_gt, g.V, g.words, pair_desc, reinterpret_cast<long long*>(stats), status);
  return launch_ok();
}

int dpc_voxel_count(const uint32_t* bits, int B, int D, int H, int W, int32_t* counts, void* stream) {
  VoxelGrid g;
  if (B < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!bits || !counts) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_voxel_count", dpc_kid("k_voxel_count"), k_voxel_count, dim3((unsigned)B), dim3(256), 0, st, bits, g.V, g.words, counts);
  return launch_ok();
}

int dpc_voxel2pc(const uint32_t* bits, int B, int G, const int32_t* out_desc, const int32_t* host_out_desc, int n_out, double* xyz,
                 int32_t* status, void* stream) {
  VoxelGrid g;
  if (B < 0 || n_out < 0 || G < 2 || !voxel_grid(G, G, G, 1, &g)) return DPC_ERR_SHAPE;  // linspace over one node divides by zero
  if (B > 0 && !host_out_desc) return DPC_ERR_NULL;
  int64_t end = 0;
  for (int b = 0; b < B; ++b) {  // output ranges ascend without overlap, inside [0, n_out), none longer than a grid
    const int64_t start = host_out_desc[2 * (int64_t)b], count = host_out_desc[2 * (int64_t)b + 1];
    if (start < end || count < 0 || count > g.V || start + count > n_out) return DPC_ERR_SHAPE;
    end = start + count;
  }
  if (B == 0) return DPC_OK;
  if (!bits || !out_desc || (!xyz && n_out > 0)) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_voxel2pc", dpc_kid("k_voxel2pc"), k_voxel2pc, dim3((unsigned)B), dim3(256), 0, st, bits, G, g.V, g.words, out_desc,
             n_out, xyz, status);
  return launch_ok();
}

}  // extern "C"
