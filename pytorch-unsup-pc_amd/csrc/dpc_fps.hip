// Batched farthest-point sampling: one workgroup per cloud, the cloud resident on chip, two barriers per round.
// The contract (distance expression, state, tie rule, outputs, guards) is in include/dpc_render.h (dpc_fps).
//
// k_fps<F64, THREADS, PPT>: F64 = the input is fp64, THREADS threads per workgroup, PPT points per thread; a cloud of
// count <= THREADS * PPT points.  Point i belongs to thread i % THREADS, slot i / THREADS, so a thread meets its points
// in ascending index and a strict compare keeps the lowest index of a tie.  Per point a thread keeps x, y, z and
// dist = the squared distance to the nearest pick so far (+inf at the start, -1 once the point is taken or for a slot
// past the end of the cloud: below every distance, and min(-1, d2) stays -1).  Storage per instantiation:
//   fp32 input, PPT <= 8    x y z widened once to fp64 in registers, dist in registers              8 registers per point
//   fp32 input, PPT = 16    x y z as fp32 in registers, widened in every round (exact), dist in registers      5
//   fp64 input, PPT <= 8    x y z and dist in registers                                                          8
//   fp64 input, PPT = 16    x y z in registers, dist in LDS (128 KiB): 1024 threads have 128 registers each      6
// A round, with the pick `cur` known to every thread:
//   thread 0 stores indices[k] = cur and radius2[k] = dist[cur]; the thread that owns cur writes its coordinates to LDS
//   and sets its dist to -1;                                                                              barrier
//   every thread reads the coordinates (wave-uniform, kept in scalar registers), lowers the dist of its points and
//   keeps the largest (dist bits as a signed integer, lowest index); DPP-modified moves merge the 64 lanes' keys and
//   lane 63 of each wave writes the wave's key to LDS;                                                     barrier
//   lane l reads the key of wave l % waves and a DPP butterfly over 4 or 16 lanes selects the winner: the next cur.
// The key is a total order, so the merge tree cannot change a result; there are no atomics on the way.  Nothing waits on
// another workgroup, and every loop is bounded by samples <= count <= DPC_FPS_MAX_POINTS.
//
// A call launches one grid of `clouds` workgroups per size class its host table uses; a workgroup whose cloud is of
// another class leaves at once.  A device row that fails the bounds checks, or whose class no launch of the call runs
// (the host table said otherwise), is flagged DPC_STATUS_BAD_INDEX by the first launch and not run.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kFpClasses = 4;
// size classes: (threads, points per thread); class c takes counts in (cap(c - 1), cap(c)]
constexpr int kFpThreads[kFpClasses] = {256, 1024, 1024, 1024};
constexpr int kFpPpt[kFpClasses] = {4, 4, 8, 16};
constexpr int fp_cap(int c) { return kFpThreads[c] * kFpPpt[c]; }
static_assert(fp_cap(kFpClasses - 1) == DPC_FPS_MAX_POINTS, "the largest class holds DPC_FPS_MAX_POINTS points");

__host__ __device__ constexpr int fp_class(int count) {
  return count <= 1024 ? 0 : count <= 4096 ? 1 : count <= 8192 ? 2 : count <= 16384 ? 3 : -1;
}
static_assert(fp_class(fp_cap(0)) == 0 && fp_class(fp_cap(0) + 1) == 1 && fp_class(fp_cap(1)) == 1 && fp_class(fp_cap(1) + 1) == 2 &&
                  fp_class(fp_cap(2)) == 2 && fp_class(fp_cap(2) + 1) == 3 && fp_class(fp_cap(3)) == 3 && fp_class(fp_cap(3) + 1) == -1,
              "fp_class restates the class table");

constexpr long long kFpInfBits = 0x7ff0000000000000ll;

// a wave-uniform value into scalar registers
__device__ inline int fp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline long long fp_uniform(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ inline double fp_uniform(double v) { return __longlong_as_double(fp_uniform(__double_as_longlong(v))); }

// (dist bits, index) a beats b: the larger dist, then the lower index
__device__ inline bool fp_better(long long ab, int ai, long long bb, int bi) { return ab > bb || (ab == bb && ai < bi); }

// One butterfly step on DPP-modified moves (no LDS traffic, unlike __shfl_xor = ds_bpermute): the key of the lane that
// CTRL names is merged into this lane's; a lane without a source merges its own key, which changes nothing.
template <int CTRL>
__device__ inline void fp_merge(long long& bb, int& bi) {
  const int lo = (int)(unsigned)(unsigned long long)bb, hi = (int)(unsigned)((unsigned long long)bb >> 32);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, 0xf, 0xf, false);
  const long long ob = (long long)(((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo);
  if (fp_better(ob, oi, bb, bi)) { bb = ob; bi = oi; }
}
// the best key of every aligned group of 4 / 16 lanes, in each of its lanes
__device__ inline void fp_merge_quad(long long& bb, int& bi) {
  fp_merge<0xb1>(bb, bi);  // quad_perm:[1,0,3,2]
  fp_merge<0x4e>(bb, bi);  // quad_perm:[2,3,0,1]
}
__device__ inline void fp_merge_row(long long& bb, int& bi) {
  fp_merge_quad(bb, bi);
  fp_merge<0x124>(bb, bi);  // row_ror:4
  fp_merge<0x128>(bb, bi);  // row_ror:8
}

template <int THREADS, int PPT, bool DIST_LDS>
struct FpLds {
  static constexpr int kWaves = THREADS / 64;
  static constexpr size_t kDist = DIST_LDS ? sizeof(double) * THREADS * PPT : 0;  // a multiple of 16
  static constexpr size_t kBytes = kDist + sizeof(long long) * kWaves + sizeof(double) * 4 + sizeof(int) * kWaves;
  double* dist;
  long long* wbits;  // [kWaves] the waves' keys
  double* c;         // [3] the pick's coordinates (+ 1 pad)
  int* widx;         // [kWaves]
  __device__ explicit FpLds(char* base) {
    dist = reinterpret_cast<double*>(base);
    wbits = reinterpret_cast<long long*>(base + kDist);
    c = reinterpret_cast<double*>(wbits + kWaves);
    widx = reinterpret_cast<int*>(c + 4);
  }
};

template <int F64, int THREADS, int PPT>
__global__ __launch_bounds__(THREADS) void k_fps(const void* __restrict__ pts_, int n_pts, const int32_t* __restrict__ desc,
                                                 int n_out, int class_mask, int flagger, int32_t* __restrict__ indices,
                                                 double* __restrict__ radius2, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  using T = std::conditional_t<F64 != 0, double, float>;
  using S = std::conditional_t<(F64 != 0 || PPT <= 8), double, float>;  // what a coordinate is kept as
  constexpr bool kDistLds = F64 != 0 && PPT > 8;
  constexpr bool kNarrow = sizeof(S) < sizeof(double);
  constexpr int kWaves = THREADS / 64;
  constexpr int kShift = THREADS == 1024 ? 10 : 8;
  static_assert((1 << kShift) == THREADS && (kWaves == 4 || kWaves == 16), "THREADS is 256 or 1024");
  extern __shared__ __attribute__((aligned(16))) char fp_smem[];
  const FpLds<THREADS, PPT, kDistLds> L(fp_smem);
  const T* __restrict__ pts = static_cast<const T*>(pts_);
  const int t = threadIdx.x, lane = t & 63, wave = fp_uniform(t >> 6);
  // the thread's slots are THREADS doubles apart; a DS instruction's offset field reaches 8 of them
  int t_hi = t + 8 * THREADS;
  asm volatile("" : "+v"(t_hi));  // one more base register, not one per slot

  const int32_t* row = desc + 5 * (size_t)blockIdx.x;
  const int start = row[0], count = row[1], first = row[2], out0 = row[3], m = row[4];
  // nothing of the device table becomes an address, or a loop bound, before it passed these
  const bool ok = count >= 1 && count <= DPC_FPS_MAX_POINTS && start >= 0 && (int64_t)start + count <= n_pts && first >= 0 &&
                  first < count && m >= 1 && m <= count && out0 >= 0 && (int64_t)out0 + m <= n_out;
  const int cls = ok ? fp_class(count) : -1;
  if (cls < 0 || !((class_mask >> cls) & 1)) {  // no launch of this call runs the row as the device table has it
    if (flagger && t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  if (cls != fp_class(THREADS * PPT)) return;  // another launch's cloud

  S x[PPT], y[PPT], z[PPT];
  double dist[kDistLds ? 1 : PPT];
  const double kInf = __longlong_as_double(kFpInfBits);
  bool bad = false;
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int i = s * THREADS + t;
    T a = 0, b = 0, c = 0;
    if (i < count) {
      const T* p = pts + 3 * ((size_t)start + i);
      a = p[0]; b = p[1]; c = p[2];
      bad |= !(__builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c));
    }
    x[s] = (S)a; y[s] = (S)b; z[s] = (S)c;
    const double d0 = i < count ? kInf : -1.0;
    if (kDistLds) L.dist[i] = d0;
    else dist[s] = d0;
    if (PPT > 8) __builtin_amdgcn_sched_barrier(0);  // one slot's loads at a time, see the round
  }
  if (__syncthreads_or(bad)) {  // the same answer in every thread
    for (int k = t; k < m; k += THREADS) {
      indices[(size_t)out0 + k] = -1;
      radius2[(size_t)out0 + k] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (t == 0 && status) atomicOr(status, (int)DPC_STATUS_NONFINITE);
    return;
  }

  int cur = first;                // wave-uniform from here on
  long long rbits = kFpInfBits;   // dist[cur] as it stands
  for (int k = 0; k < m; ++k) {
    if (t == 0) {
      indices[(size_t)out0 + k] = cur;
      radius2[(size_t)out0 + k] = __longlong_as_double(rbits);
    }
    if (k == m - 1) break;  // the last pick needs no successor
    // the owner of cur publishes its coordinates and takes the point out
    const int slot = cur >> kShift, owner = cur & (THREADS - 1);
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
      if (slot == s) {  // the same in every thread: a scalar branch
        if (t == owner) {
          L.c[0] = (double)x[s]; L.c[1] = (double)y[s]; L.c[2] = (double)z[s];
          if (kDistLds) L.dist[cur] = -1.0;
          else dist[s] = -1.0;
        }
      }
    }
    __syncthreads();
    const double cx = fp_uniform(L.c[0]), cy = fp_uniform(L.c[1]), cz = fp_uniform(L.c[2]);

    long long bb = LLONG_MIN;
    int bs = 0;  // the slot of the thread's best: its index is bs * THREADS + t
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
      if (kNarrow) asm volatile("" : "+v"(x[s]), "+v"(y[s]), "+v"(z[s]));  // keeps the widening in the round: 3 registers a point, not 6
      const double dx = (double)x[s] - cx, dy = (double)y[s] - cy, dz = (double)z[s] - cz;
      const double d2 = dx * dx + dy * dy + dz * dz;
      double* const dp = L.dist + (s < 8 ? t + s * THREADS : t_hi + (s - 8) * THREADS);
      double d = kDistLds ? *dp : dist[s];
      if (d2 < d) {  // never for a taken point or a slot past the end: their dist is -1
        d = d2;
        if (kDistLds) *dp = d;
        else dist[s] = d;
      }
      const long long bits = __double_as_longlong(d);
      if (bits > bb) { bb = bits; bs = s; }  // ascending index and a strict compare: the lowest index of a tie stays
      if (PPT > 8) {  // one point at a time, its key merged before the next: interleaved points cost registers there are none of
        asm volatile("" : "+v"(bb), "+v"(bs));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    int bi = bs * THREADS + t;
    fp_merge_row(bb, bi);
    fp_merge<0x142>(bb, bi);  // row_bcast:15: rows 1..3 take in the row below them
    fp_merge<0x143>(bb, bi);  // row_bcast:31: rows 2 and 3 take in the lower half; lane 63 holds the wave's key
    if (lane == 63) { L.wbits[wave] = bb; L.widx[wave] = bi; }
    __syncthreads();
    // lane l reads the key of wave l % kWaves: every row of 16 lanes (every quad, with 4 waves) holds them all
    bb = L.wbits[lane & (kWaves - 1)]; bi = L.widx[lane & (kWaves - 1)];
    if (kWaves == 4) fp_merge_quad(bb, bi);
    else fp_merge_row(bb, bi);
    cur = fp_uniform(bi);
    rbits = fp_uniform(bb);
  }
}

// Host check of the table: rows (start, count, first, out_start, samples) with 1 <= samples <= count <=
// DPC_FPS_MAX_POINTS, 0 <= first < count, [start, start + count) inside the buffer and output ranges that ascend
// without overlap.  *n_out = the end of the last output range, *mask = the size classes in use.
int fp_check(int clouds, const int32_t* desc, int64_t n_pts, int* n_out, int* mask) {
  int64_t end = 0;
  int used = 0;
  for (int c = 0; c < clouds; ++c) {
    const int32_t* d = desc + 5 * (int64_t)c;
    const int64_t start = d[0], count = d[1], first = d[2], out0 = d[3], m = d[4];
    if (start < 0 || count < 1 || count > DPC_FPS_MAX_POINTS || start + count > n_pts) return DPC_ERR_SHAPE;
    if (first < 0 || first >= count || m < 1 || m > count) return DPC_ERR_SHAPE;
    if (out0 < end || out0 + m > INT32_MAX) return DPC_ERR_SHAPE;
    end = out0 + m;
    used |= 1 << fp_class((int)count);
  }
  *n_out = (int)end;
  *mask = used;
  return DPC_OK;
}

template <int F64, int CLS>
int fp_launch(const void* pts, int n_pts, const int32_t* desc, int clouds, int n_out, int mask, int flagger, int32_t* indices,
              double* radius2, int32_t* status, hipStream_t st) {
  constexpr int THREADS = kFpThreads[CLS], PPT = kFpPpt[CLS];
  constexpr size_t lds = FpLds<THREADS, PPT, (F64 != 0 && PPT > 8)>::kBytes;
  static_assert(lds <= 160 * 1024, "a cloud's state must fit the CU's 160 KiB of LDS");
  static LdsLimit limit;
  const int rc = set_lds(k_fps<F64, THREADS, PPT>, lds, limit);
  if (rc != DPC_OK) return rc;
  DPC_LAUNCH("k_fps", dpc_kid("k_fps", F64, THREADS, PPT), (k_fps<F64, THREADS, PPT>), dim3((unsigned)clouds), dim3(THREADS), lds,
             st, pts, n_pts, desc, n_out, mask, flagger, indices, radius2, status);
  return launch_ok();
}

template <int F64>
int fp_run(const void* pts, int n_pts, const int32_t* desc, int clouds, int n_out, int mask, int32_t* indices, double* radius2,
           int32_t* status, hipStream_t st) {
  int flagger = 1, rc = DPC_OK;  // the first launch of the call flags the rows that no launch runs
  if (rc == DPC_OK && (mask & 1)) { rc = fp_launch<F64, 0>(pts, n_pts, desc, clouds, n_out, mask, flagger, indices, radius2, status, st); flagger = 0; }
  if (rc == DPC_OK && (mask & 2)) { rc = fp_launch<F64, 1>(pts, n_pts, desc, clouds, n_out, mask, flagger, indices, radius2, status, st); flagger = 0; }
  if (rc == DPC_OK && (mask & 4)) { rc = fp_launch<F64, 2>(pts, n_pts, desc, clouds, n_out, mask, flagger, indices, radius2, status, st); flagger = 0; }
  if (rc == DPC_OK && (mask & 8)) { rc = fp_launch<F64, 3>(pts, n_pts, desc, clouds, n_out, mask, flagger, indices, radius2, status, st); flagger = 0; }
  return rc;
}

}  // namespace

extern "C" {

int dpc_fps(const void* pts, int n_pts, int is_f64, const int32_t* cloud_desc, const int32_t* host_cloud_desc, int clouds,
            int32_t* indices, double* radius2, int32_t* status, void* stream) {
  if (n_pts < 0 || clouds < 0) return DPC_ERR_SHAPE;
  if (clouds > 0 && !host_cloud_desc) return DPC_ERR_NULL;
  int n_out = 0, mask = 0;
  const int rc = fp_check(clouds, host_cloud_desc, n_pts, &n_out, &mask);
  if (rc != DPC_OK) return rc;
  if (clouds == 0) return DPC_OK;
  if (!pts || !cloud_desc || !indices || !radius2) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  return is_f64 ? fp_run<1>(pts, n_pts, cloud_desc, clouds, n_out, mask, indices, radius2, status, st)
                : fp_run<0>(pts, n_pts, cloud_desc, clouds, n_out, mask, indices, radius2, status, st);
}

}  // extern "C"
