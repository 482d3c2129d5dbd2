// Exact squared Euclidean distance transforms of bit grids, their surface shells, and the sums and counts a voxel F-score
// needs.  The contract (seeds, the value without a seed, padding bits, the stats columns, guards and check order) is in
// include/dpc_render.h (dpc_voxel_edt).  Everything is an integer: min and + over squared index distances have one right
// answer, int64 sums do not depend on order.
//
// The transform is min-plus in three separable passes, each the plain minimum over all candidates of a line (sides are at
// most 128): g1(w) = the squared distance along W to the nearest seed of the row, g2(h) = min_j g1(j) + (h - j)^2 along H,
// sq(d) = min_k g2(k) + (d - k)^2 along D.  A line without a seed carries kEdtInf = 2^28: two added squares (at most
// 2 * 127^2) cannot wrap it, and anything >= kEdtInf is "no seed".
//
// k_edt_plane<S, THREADS>   one workgroup per (grid, d-plane), H, W <= S.  The rows' bits are cut out of the grid's words
//     into row-aligned words in LDS; g1 of every voxel comes from them by count-leading / trailing-zeros and is kept in LDS
//     as int32 [H][S], lanes along w.  The H pass is register-blocked: a thread owns one w and a strip of S / (THREADS / S)
//     outputs, so one LDS read of g1(j, w) serves the whole strip; the reads of a wave are consecutive words (no bank
//     conflict) and the stores of g2 to sq are coalesced.  From S = 64 a wave shares one strip, so (h - j)^2 is scalar
//     arithmetic and a candidate costs one add and one min.
//       S     threads   strip   LDS (g1 + row words)
//       32      256        4      4 KiB + 128 B
//       64      256       16     16 KiB + 512 B
//      128      512       32     64 KiB + 2 KiB
// k_edt_depth<S>            one workgroup of 256 threads per (grid, 64 consecutive (h, w) columns), D <= S: it reads all D
//     values of its columns into LDS (int32 [D][64]) before it writes any of them, which is what lets it run in place on
//     sq; a thread owns one column and a strip of S / 4 outputs along d.  It writes DPC_VOXEL_EDT_NONE where the minimum
//     is still infinite.
// k_voxel_shell             one thread per output word: the six neighbour words are 32-bit windows of the grid at f -+ 1,
//     f -+ W and f -+ H W; a neighbour outside the grid counts as clear.
// k_voxel_edt_stats         one workgroup per (field, bit grid) pair.  A wave reads 64 words of the grid a round, a word a
//     lane, and visits only the runs of 16 words that have a bit set (a ballot: much of a shell's grid is zero words); in a
//     visited run the lanes lie along the 64 voxels of two words at a time, so the field loads the set bits select are
//     consecutive, and the eight loads of a run are in flight together (a lane without a bit reads voxel 0).  Counts and
//     the int64 sum go per thread, per wave by shuffles, over the waves by thread 0, which alone writes the pair's row.
// Nothing waits on another workgroup; every loop is bounded by a host-checked size.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"
#include "dpc_voxel_bits.h"

namespace {

constexpr int kEdtInf = 1 << 28;
static_assert(DPC_VOXEL_MAX_SIDE <= 128, "the size classes end at 128");
static_assert((int64_t)kEdtInf + 2 * (DPC_VOXEL_MAX_SIDE - 1) * (DPC_VOXEL_MAX_SIDE - 1) <= INT32_MAX, "an infinite line plus two squares");
static_assert(3 * (DPC_VOXEL_MAX_SIDE - 1) * (DPC_VOXEL_MAX_SIDE - 1) < kEdtInf, "every finite distance is below the infinite value");
static_assert(DPC_VOXEL_EDT_NONE == INT32_MAX, "the value of a grid without a seed");

constexpr int edt_class(int side) { return side <= 32 ? 32 : side <= 64 ? 64 : 128; }

template <int S, int THREADS>
__global__ __launch_bounds__(THREADS) void k_edt_plane(const uint32_t* __restrict__ bits, int D, int H, int W, int words, int of_clear,
                                                       int32_t* __restrict__ sq) {
  constexpr int K = S / 32;        // row-aligned words of a row
  constexpr int NQ = THREADS / S;  // strips of the H pass
  constexpr int R = S / NQ;        // outputs of a strip
  static_assert(THREADS % S == 0 && S % NQ == 0, "whole strips");
  __shared__ int g1[S * S];
  __shared__ uint32_t rows[S * K];
  const int t = threadIdx.x;
  const int b = blockIdx.x / D, d = blockIdx.x - b * D;
  const uint32_t* __restrict__ grid = bits + (size_t)b * words;
  const int f0 = d * H * W;  // the plane's first voxel

  // the seeds of row h as words of its own: bit i of word k is voxel (h, 32 k + i); nothing beyond W, so neither the next
  // row nor the padding bits of the grid's last word can be a seed
  for (int i = t; i < H * K; i += THREADS) {
    const int h = i / K, k = i - h * K;
    const int left = W - 32 * k;  // bits of this word inside the row
    uint32_t m = 0u;
    if (left > 0) {
      m = voxel_window(grid, words, f0 + h * W + 32 * k);
      if (of_clear) m = ~m;
      if (left < 32) m &= (1u << left) - 1u;
    }
    rows[i] = m;
  }
  __syncthreads();

  // g1: the squared distance along the row to its nearest seed
  for (int i = t; i < H * S; i += THREADS) {
    const int h = i / S, w = i - h * S;
    int best = kEdtInf;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t m = rows[h * K + k];
      const int rel = w - 32 * k;
      const uint32_t lo = rel < 0 ? 0u : rel >= 31 ? m : m & ((2u << rel) - 1u);   // seeds at or before w
      const uint32_t hi = rel <= 0 ? m : rel >= 32 ? 0u : m & ~((1u << rel) - 1u);  // seeds at or after w
      if (lo) best = min(best, rel - (31 - (int)__clz(lo)));
      if (hi) best = min(best, (int)__builtin_ctz(hi) - rel);
    }
    g1[i] = best < kEdtInf ? best * best : kEdtInf;
  }
  __syncthreads();

  // g2(h, w) = min_j g1(j, w) + (h - j)^2
  const int w = t % S;
  const int q = S >= 64 ? __builtin_amdgcn_readfirstlane(t / S) : t / S;  // from 64 lanes a row, a wave has one strip
  int acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = kEdtInf;
  for (int j = 0; j < H; ++j) {
    const int g = g1[j * S + w];
    const int e = q * R - j;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = min(acc[r], g + (e + r) * (e + r));
  }
  if (w < W) {
    int32_t* __restrict__ out = sq + (size_t)b * D * H * W + f0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int h = q * R + r;
      if (h < H) out[h * W + w] = acc[r] < kEdtInf ? acc[r] : kEdtInf;
    }
  }
}

constexpr int kEdtCols = 64;  // (h, w) columns of a depth workgroup: one wave wide

template <int S>
__global__ __launch_bounds__(256) void k_edt_depth(int D, int HW, int tiles, int32_t* __restrict__ sq) {
  constexpr int NQ = 256 / kEdtCols;
  constexpr int R = S / NQ;
  __shared__ int g2[S * kEdtCols];
  const int t = threadIdx.x;
  const int c = t & (kEdtCols - 1);
  const int q = __builtin_amdgcn_readfirstlane(t / kEdtCols);
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int col = tile * kEdtCols + c;
  int32_t* __restrict__ field = sq + (size_t)b * D * HW;
  const bool live = col < HW;

  // every value of the workgroup's columns is read before any is written: the pass runs in place
  for (int k = q; k < D; k += NQ) g2[k * kEdtCols + c] = live ? field[(size_t)k * HW + col] : kEdtInf;
  __syncthreads();

  int acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = kEdtInf;
  for (int k = 0; k < D; ++k) {
    const int g = g2[k * kEdtCols + c];
    const int e = q * R - k;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = min(acc[r], g + (e + r) * (e + r));
  }
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int d = q * R + r;
      if (d < D) field[(size_t)d * HW + col] = acc[r] < kEdtInf ? acc[r] : (int32_t)DPC_VOXEL_EDT_NONE;
    }
  }
}

__global__ __launch_bounds__(256) void k_voxel_shell(const uint32_t* __restrict__ bits, int B, int D, int H, int W, int V, int words,
                                                     uint32_t* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= words) return;
  // which of the word's voxels have a neighbour inside the grid on each side: walk the 32 voxels from the first one's
  // coordinates
  const int f0 = 32 * j;
  int w = f0 % W, h = (f0 / W) % H, d = f0 / (W * H);
  uint32_t valid = 0u, w_lo = 0u, w_hi = 0u, h_lo = 0u, h_hi = 0u, d_lo = 0u, d_hi = 0u;
  for (int i = 0; i < 32 && f0 + i < V; ++i) {
    const uint32_t bit = 1u << i;
    valid |= bit;
    if (w > 0) w_lo |= bit;
    if (w < W - 1) w_hi |= bit;
    if (h > 0) h_lo |= bit;
    if (h < H - 1) h_hi |= bit;
    if (d > 0) d_lo |= bit;
    if (d < D - 1) d_hi |= bit;
    if (++w == W) {
      w = 0;
      if (++h == H) { h = 0; ++d; }
    }
  }
  const int HW = H * W;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const uint32_t* __restrict__ g = bits + (size_t)b * words;
    // a neighbour counts only where it lies inside the grid, so no padding bit is ever looked at
    const uint32_t inner = (voxel_window(g, words, f0 - 1) & w_lo) & (voxel_window(g, words, f0 + 1) & w_hi) &
                           (voxel_window(g, words, f0 - W) & h_lo) & (voxel_window(g, words, f0 + W) & h_hi) &
                           (voxel_window(g, words, f0 - HW) & d_lo) & (voxel_window(g, words, f0 + HW) & d_hi);
    out[(size_t)b * words + j] = g[j] & valid & ~inner;
  }
}

constexpr int kEdtStatsBurst = 8;  // pairs of words whose field loads k_voxel_edt_stats has in flight together
static_assert(32 % kEdtStatsBurst == 0, "whole bursts in a round of 64 words");

struct EdtThresholds {
  int32_t t[DPC_VOXEL_EDT_MAX_THRESHOLDS];
};

__global__ __launch_bounds__(256) void k_voxel_edt_stats(const int32_t* __restrict__ sq, int n_fields, const uint32_t* __restrict__ bits,
                                                         int n_grids, int V, int words, const int32_t* __restrict__ pair_desc,
                                                         EdtThresholds thr, int K, long long* __restrict__ out,
                                                         int32_t* __restrict__ status) {
  constexpr int KMAX = DPC_VOXEL_EDT_MAX_THRESHOLDS;
  __shared__ long long scratch[4];
  const int t = threadIdx.x;
  const int fi = pair_desc[2 * (size_t)blockIdx.x], gi = pair_desc[2 * (size_t)blockIdx.x + 1];
  if (!(fi >= 0 && fi < n_fields && gi >= 0 && gi < n_grids)) {  // not read, its row left as it was
    if (t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  const int32_t* __restrict__ field = sq + (size_t)fi * V;
  const uint32_t* __restrict__ g = bits + (size_t)gi * words;
  int n = 0, reached = 0, within[KMAX];
  long long sum = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) within[k] = 0;
  const int lane = t & 63, wave = t >> 6;
  for (int j0 = 64 * wave; j0 < words; j0 += 256) {  // a wave takes 64 words a round, a word a lane: the same trips in every lane
    const int j = j0 + lane;
    const uint32_t mine = voxel_clear_padding(j < words ? g[j] : 0u, j, words, V);  // a padding bit is not a voxel
    n += __popc(mine);
    const unsigned long long some = __ballot(mine != 0u);
    for (int i0 = 0; i0 < 32; i0 += kEdtStatsBurst) {  // words 2 i and 2 i + 1 of the round are 64 consecutive voxels, a lane each
      if (((some >> (2 * i0)) & ((1ull << (2 * kEdtStatsBurst)) - 1ull)) == 0ull) continue;  // the same in every lane: nothing set
      int32_t v[kEdtStatsBurst];
#pragma unroll
      for (int u = 0; u < kEdtStatsBurst; ++u) {  // branch-free, so the loads of a burst are in flight together
        const uint32_t m = (uint32_t)__shfl((int)mine, 2 * (i0 + u) + (lane >> 5), 64);
        const bool set = (m >> (lane & 31)) & 1u;  // a set bit lies in a word of the grid and below V
        v[u] = field[set ? (size_t)(j0 + 2 * (i0 + u)) * 32 + lane : (size_t)0];
        if (!set) v[u] = (int32_t)DPC_VOXEL_EDT_NONE;
      }
#pragma unroll
      for (int u = 0; u < kEdtStatsBurst; ++u) {
        const bool hit = v[u] != (int32_t)DPC_VOXEL_EDT_NONE;
        reached += hit ? 1 : 0;
        sum += hit ? v[u] : 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) within[k] += (k < K && v[u] <= thr.t[k]) ? 1 : 0;  // t_k < NONE: never for a voxel not reached
      }
    }
  }
  long long* row = out + (size_t)(3 + K) * blockIdx.x;
  const long long s_n = block_sum<256, long long>((long long)n, scratch), s_reached = block_sum<256, long long>((long long)reached, scratch),
                  s_sum = block_sum<256, long long>(sum, scratch);
  if (t == 0) {
    row[0] = s_n;
    row[1] = s_reached;
    row[2] = s_sum;
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {  // the same in every thread: block_sum has barriers
      const long long s = block_sum<256, long long>((long long)within[k], scratch);
      if (t == 0) row[3 + k] = s;
    }
  }
}

template <int S, int THREADS>
int edt_plane(const uint32_t* bits, int B, const VoxelGrid& g, int of_clear, int32_t* sq, hipStream_t st) {
  DPC_LAUNCH("k_edt_plane", dpc_kid("k_edt_plane", S, THREADS), (k_edt_plane<S, THREADS>), dim3((unsigned)B * (unsigned)g.D),
             dim3(THREADS), 0, st, bits, g.D, g.H, g.W, g.words, of_clear, sq);
  return launch_ok();
}

template <int S>
int edt_depth(int B, const VoxelGrid& g, int tiles, int32_t* sq, hipStream_t st) {
  DPC_LAUNCH("k_edt_depth", dpc_kid("k_edt_depth", S), (k_edt_depth<S>), dim3((unsigned)B * (unsigned)tiles), dim3(256), 0, st, g.D,
             g.H * g.W, tiles, sq);
  return launch_ok();
}

}  // namespace

extern "C" {

int dpc_voxel_edt(const uint32_t* bits, int B, int D, int H, int W, int of_clear, int32_t* sq, void* stream) {
  VoxelGrid g;
  if (B < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  const int tiles = (g.H * g.W + kEdtCols - 1) / kEdtCols;
  if ((int64_t)B * g.D > INT32_MAX || (int64_t)B * tiles > INT32_MAX) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!bits || !sq) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (edt_class(g.H > g.W ? g.H : g.W)) {
    case 32: rc = edt_plane<32, 256>(bits, B, g, of_clear != 0, sq, st); break;
    case 64: rc = edt_plane<64, 256>(bits, B, g, of_clear != 0, sq, st); break;
    default: rc = edt_plane<128, 512>(bits, B, g, of_clear != 0, sq, st); break;
  }
  if (rc != DPC_OK) return rc;
  switch (edt_class(g.D)) {
    case 32: return edt_depth<32>(B, g, tiles, sq, st);
    case 64: return edt_depth<64>(B, g, tiles, sq, st);
    default: return edt_depth<128>(B, g, tiles, sq, st);
  }
}

int dpc_voxel_shell(const uint32_t* bits, int B, int D, int H, int W, uint32_t* out, void* stream) {
  VoxelGrid g;
  if (B < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!bits || !out) return DPC_ERR_NULL;
  if (out == bits) return DPC_ERR_SHAPE;  // a word's neighbours are read after other words have been written
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((g.words + 255) / 256), (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_voxel_shell", dpc_kid("k_voxel_shell"), k_voxel_shell, grid, dim3(256), 0, st, bits, B, g.D, g.H, g.W, g.V, g.words, out);
  return launch_ok();
}

int dpc_voxel_edt_stats(const int32_t* sq, int n_fields, const uint32_t* bits, int n_grids, int D, int H, int W,
                        const int32_t* pair_desc, const int32_t* host_pair_desc, int pairs, const int32_t* host_thresholds_sq, int K,
                        int64_t* out, int32_t* status, void* stream) {
  VoxelGrid g;
  if (n_fields < 0 || n_grids < 0 || pairs < 0 || !voxel_grid(D, H, W, 1, &g)) return DPC_ERR_SHAPE;
  if (K < 0 || K > DPC_VOXEL_EDT_MAX_THRESHOLDS) return DPC_ERR_SHAPE;
  if ((K > 0 && !host_thresholds_sq) || (pairs > 0 && !host_pair_desc)) return DPC_ERR_NULL;
  EdtThresholds thr = {};
  for (int k = 0; k < K; ++k) {
    if (host_thresholds_sq[k] < 0 || host_thresholds_sq[k] >= DPC_VOXEL_EDT_NONE) return DPC_ERR_SHAPE;
    thr.t[k] = host_thresholds_sq[k];
  }
  const int rc = check_pairs(host_pair_desc, pairs, n_fields, n_grids);
  if (rc != DPC_OK) return rc;
  if (pairs == 0) return DPC_OK;
  if (!sq || !bits || !pair_desc || !out) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_voxel_edt_stats", dpc_kid("k_voxel_edt_stats"), k_voxel_edt_stats, dim3((unsigned)pairs), dim3(256), 0, st, sq, n_fields,
             bits, n_grids, g.V, g.words, pair_desc, thr, K, reinterpret_cast<long long*>(out), status);
  return launch_ok();
}

}  // extern "C"
