// Batched Earth Mover's Distance: a deterministic auction with eps-scaling, one workgroup per pair, everything in LDS.
// The contract (cost expression, schedule, tie rules, outputs) is in include/dpc_render.h (dpc_emd_fwd / dpc_emd_bwd).
//
// k_emd_auction<T>, 1024 threads = 16 waves per pair of n <= DPC_EMD_MAX_POINTS points.  LDS, 76 bytes per point:
//   px py pz gx gy gz   6 x double[n]   both clouds, widened to fp64 once (structure of arrays: a wave's 64 consecutive
//                                       objects are 64 consecutive doubles, conflict-free 8-byte reads)
//   price               double[n]
//   bidmax              uint64[n]       the round's highest bid per object as an order-preserving integer key, 0 = no bid
//   owner assigned win  3 x int32[n]    owner[j] = the bidder holding object j, assigned[i] = the object of bidder i,
//                                       win[j] = the round's lowest bidder among those whose bid is bidmax[j]
// A round is three passes between workgroup barriers; prices and owners change in the third only, so every bid of a
// round reads the same snapshot:
//   1  bid      bidder i = slot * 1024 + thread belongs to the wave of its thread.  A wave takes its unassigned bidders
//               one after the other (a ballot, then the set bits in ascending order): its 64 lanes scan the n objects
//               with a stride of 64, each keeping its best value, the lowest j that has it, and its second best; a
//               butterfly merges the 64 triples.  The bidder's own lane keeps (j*, bid) in registers and raises
//               bidmax[j*] with one 64-bit LDS max.
//   2  claim    every lane whose kept bid equals bidmax[j*] lowers win[j*] to its bidder index (32-bit LDS min).
//   3  resolve  thread t looks at objects t and t + 1024: one with a winner frees its previous owner, takes the winner
//               and the bid as its price, and clears bidmax / win for the next round.
// Integer max / min are order-independent, so the outcome does not depend on how the waves are scheduled.  Costs are
// recomputed in every round: the n x n matrix would be 32 MiB at n = 2048.  There is no communication between
// workgroups, the only loop that is not a fixed count over n is the round loop, bounded by max_rounds, and every
// barrier sits in code whose conditions are the same for all threads (values read from LDS after a barrier, or kernel
// arguments).
//
// k_emd_bwd<T>: one thread per point index of a pair, writing that index's pred row and gt row of the gradient.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kEmThreads = 1024;
constexpr int kEmWaves = kEmThreads / 64;
constexpr int kEmSlots = DPC_EMD_MAX_POINTS / kEmThreads;  // bidders, and objects, per thread
constexpr int kEmNone = INT32_MAX;
constexpr int kEmBwThreads = 256;
constexpr size_t kEmPointBytes = 7 * sizeof(double) + sizeof(uint64_t) + 3 * sizeof(int32_t);  // 76
constexpr size_t kEmScratchBytes = 2 * kEmWaves * sizeof(double) + 16;  // the span reduction, the unassigned count
static_assert(DPC_EMD_MAX_POINTS % kEmThreads == 0, "a thread owns DPC_EMD_MAX_POINTS / 1024 bidders");

// arrays of n elements start 8-byte aligned when n is even
__host__ __device__ inline int em_pad(int n) { return (n + 1) & ~1; }
inline size_t em_lds_bytes(int n) { return kEmPointBytes * (size_t)em_pad(n) + kEmScratchBytes; }
static_assert(kEmPointBytes * DPC_EMD_MAX_POINTS + kEmScratchBytes <= 160 * 1024, "a pair must fit the CU's 160 KiB of LDS");

// c_ij: three differences, three squares, two additions left to right, each rounded once (no contraction); then the
// square root unless the cost is the squared distance
__device__ inline double em_cost(double px, double py, double pz, double gx, double gy, double gz, int squared) {
#pragma clang fp contract(off)
  const double dx = px - gx, dy = py - gy, dz = pz - gz;
  const double d2 = dx * dx + dy * dy + dz * dz;
  return squared ? d2 : sqrt(d2);
}

// doubles as unsigned integers in the same order; no finite double maps to 0
__device__ inline unsigned long long em_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double em_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct EmLds {
  double *px, *py, *pz, *gx, *gy, *gz, *price;
  unsigned long long* bidmax;
  int *owner, *assigned, *win;
  double* red;  // [2 * kEmWaves]
  int* left;    // bidders without an object
};

__device__ inline EmLds em_carve(char* base, int n) {
  const int np = em_pad(n);
  EmLds L;
  L.px = reinterpret_cast<double*>(base);
  L.py = L.px + np; L.pz = L.py + np;
  L.gx = L.pz + np; L.gy = L.gx + np; L.gz = L.gy + np;
  L.price = L.gz + np;
  L.bidmax = reinterpret_cast<unsigned long long*>(L.price + np);
  L.owner = reinterpret_cast<int*>(L.bidmax + np);
  L.assigned = L.owner + np; L.win = L.assigned + np;
  L.red = reinterpret_cast<double*>(L.win + np);
  L.left = reinterpret_cast<int*>(L.red + 2 * kEmWaves);
  return L;
}

template <class T>
__global__ __launch_bounds__(kEmThreads) void k_emd_auction(const T* __restrict__ pred, int n_pred, const T* __restrict__ gt,
                                                            int n_gt, const int32_t* __restrict__ desc, int n_cap, int squared,
                                                            double eps, int max_rounds, double* __restrict__ emd,
                                                            int32_t* __restrict__ assignment, int32_t* __restrict__ inverse,
                                                            int32_t* __restrict__ rounds, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char em_smem[];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = desc[4 * p], n = desc[4 * p + 1], g0 = desc[4 * p + 2];
  // the host checked its copy of the table and sized the LDS for n_cap points; a device table that disagrees is not run
  if (n < 1 || n > n_cap || desc[4 * p + 3] != n || p0 < 0 || g0 < 0 || (int64_t)p0 + n > n_pred || (int64_t)g0 + n > n_gt) {
    if (t == 0) {
      emd[p] = __longlong_as_double(0x7ff8000000000000ll);
      rounds[p] = 0;
      if (status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    }
    return;
  }
  const EmLds L = em_carve(em_smem, n);
  const double kInf = __longlong_as_double(0x7ff0000000000000ll);

  for (int i = t; i < n; i += kEmThreads) {
    const T* a = pred + 3 * ((size_t)p0 + i);
    const T* b = gt + 3 * ((size_t)g0 + i);
    L.px[i] = (double)a[0]; L.py[i] = (double)a[1]; L.pz[i] = (double)a[2];
    L.gx[i] = (double)b[0]; L.gy[i] = (double)b[1]; L.gz[i] = (double)b[2];
    L.price[i] = 0.0;
    L.bidmax[i] = 0ull;
    L.owner[i] = -1; L.assigned[i] = -1; L.win[i] = kEmNone;
  }
  if (t == 0) *L.left = n;
  __syncthreads();

  // span = max c - min c over the pair: wave w takes rows w, w + 16, ...
  {
    double cmax = -kInf, cmin = kInf;
    for (int i = wave; i < n; i += kEmWaves) {
      const double x = L.px[i], y = L.py[i], z = L.pz[i];
      for (int j = lane; j < n; j += 64) {
        const double c = em_cost(x, y, z, L.gx[j], L.gy[j], L.gz[j], squared);
        cmax = fmax(cmax, c); cmin = fmin(cmin, c);
      }
    }
    for (int off = 32; off; off >>= 1) {
      cmax = fmax(cmax, __shfl_xor(cmax, off, 64));
      cmin = fmin(cmin, __shfl_xor(cmin, off, 64));
    }
    if (lane == 0) { L.red[wave] = cmax; L.red[kEmWaves + wave] = cmin; }
  }
  __syncthreads();
  double cmax = -kInf, cmin = kInf;
  for (int w = 0; w < kEmWaves; ++w) { cmax = fmax(cmax, L.red[w]); cmin = fmin(cmin, L.red[kEmWaves + w]); }
  const double span = cmax - cmin;

  double eps_k = fmax(span / 2.0, eps);
  bool done = false;
  int round = 0;
  while (round < max_rounds) {
    ++round;
    // 1: the bids of this thread's bidders, kept in registers by the bidder's own lane
    int myj[kEmSlots];
    double mybid[kEmSlots];
#pragma unroll
    for (int s = 0; s < kEmSlots; ++s) {
      myj[s] = -1; mybid[s] = 0.0;
      const int base = s * kEmThreads + wave * 64;
      if (base >= n) continue;  // the same for the whole wave
      const int i = base + lane;
      unsigned long long todo = __builtin_amdgcn_ballot_w64(i < n && L.assigned[i] < 0);
      while (todo != 0ull) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ib = base + b;
        const double x = L.px[ib], y = L.py[ib], z = L.pz[ib];
        double v1 = -kInf, v2 = -kInf;
        int j1 = kEmNone;
        for (int j = lane; j < n; j += 64) {  // ascending j and a strict compare: the lowest j of a tie stays
          const double v = -em_cost(x, y, z, L.gx[j], L.gy[j], L.gz[j], squared) - L.price[j];
          if (v > v1) { v2 = v1; v1 = v; j1 = j; }
          else if (v > v2) v2 = v;
        }
        for (int off = 32; off; off >>= 1) {
          const double ov1 = __shfl_xor(v1, off, 64), ov2 = __shfl_xor(v2, off, 64);
          const int oj = __shfl_xor(j1, off, 64);
          const bool mine = v1 > ov1 || (v1 == ov1 && j1 < oj);
          // the best of the rest: the winner side's second, or the other side's best
          v2 = mine ? fmax(v2, ov1) : fmax(ov2, v1);
          if (!mine) { v1 = ov1; j1 = oj; }
        }
        if (lane == b && j1 < n) {  // j1 == kEmNone: every value was NaN; no bid, the pair runs into the round cap
          const double w = n == 1 ? v1 : v2;
          const double bid = L.price[j1] + (v1 - w) + eps_k;
          if (bid == bid) {
            myj[s] = j1; mybid[s] = bid;
            atomicMax(&L.bidmax[j1], em_key(bid));
          }
        }
      }
    }
    __syncthreads();
    // 2: of the bidders with an object's highest bid, the lowest index
#pragma unroll
    for (int s = 0; s < kEmSlots; ++s)
      if (myj[s] >= 0 && L.bidmax[myj[s]] == em_key(mybid[s])) atomicMin(&L.win[myj[s]], s * kEmThreads + t);
    __syncthreads();
    // 3: objects change hands.  A previous owner did not bid and a bidder wins at most one object, so no two threads
    // write the same entry of assigned
#pragma unroll
    for (int s = 0; s < kEmSlots; ++s) {
      const int j = s * kEmThreads + t;
      if (j < n) {
        const int w = L.win[j];
        if (w != kEmNone) {
          const int old = L.owner[j];
          if (old >= 0) L.assigned[old] = -1;
          else atomicSub(L.left, 1);
          L.owner[j] = w;
          L.assigned[w] = j;
          L.price[j] = em_unkey(L.bidmax[j]);
          L.bidmax[j] = 0ull;
          L.win[j] = kEmNone;
        }
      }
    }
    __syncthreads();
    if (*L.left == 0) {  // the phase is over
      if (eps_k <= eps) { done = true; break; }
      eps_k = fmax(eps_k / 5.0, eps);
      __syncthreads();  // everybody has read left
      for (int i = t; i < n; i += kEmThreads) { L.owner[i] = -1; L.assigned[i] = -1; }
      if (t == 0) *L.left = n;
      __syncthreads();
    }
  }

  // emd = (sum_i c_{i, pi(i)}) / n: lane l of wave 0 adds terms l, l + 64, ... onto 0.0 in ascending order, then a
  // butterfly over the 64 partial sums (distances 32, 16, ... 1)
  double* cost = reinterpret_cast<double*>(L.bidmax);  // all zero again after the last resolve
  if (done) {
    for (int i = t; i < n; i += kEmThreads) {
      const int j = L.assigned[i];
      cost[i] = em_cost(L.px[i], L.py[i], L.pz[i], L.gx[j], L.gy[j], L.gz[j], squared);
    }
  }
  __syncthreads();
  if (wave == 0) {
    double sum = 0.0;
    if (done) {
      for (int i = lane; i < n; i += 64) sum += cost[i];
      for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off, 64);
    }
    if (lane == 0) {
      emd[p] = done ? sum / (double)n : __longlong_as_double(0x7ff8000000000000ll);
      rounds[p] = round;
      if (!done && status) atomicOr(status, (int)DPC_STATUS_EMD_NOT_CONVERGED);
    }
  }
  for (int i = t; i < n; i += kEmThreads) {
    assignment[(size_t)p0 + i] = L.assigned[i];
    inverse[(size_t)g0 + i] = L.owner[i];
  }
}

// The gradient term of the matched couple (a, b) = (pred point, its gt point), in fp64, op for op:
//   w = up / n;  squared: c = (2 w) * (a - b);  otherwise d = sqrt(d2) as in the forward, c = ((a - b) / d) * w, and
//   exactly zero when d == 0.  The pred point receives c and the gt point -c.
__device__ inline void em_term(const double a[3], const double b[3], double w, int squared, double c[3]) {
#pragma clang fp contract(off)
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  if (squared) {
    const double w2 = 2.0 * w;
    c[0] = w2 * dx; c[1] = w2 * dy; c[2] = w2 * dz;
    return;
  }
  const double d = sqrt(dx * dx + dy * dy + dz * dz);
  if (d == 0.0) { c[0] = c[1] = c[2] = 0.0; return; }
  c[0] = (dx / d) * w; c[1] = (dy / d) * w; c[2] = (dz / d) * w;
}

template <class T>
__global__ __launch_bounds__(kEmBwThreads) void k_emd_bwd(const T* __restrict__ pred, const T* __restrict__ gt,
                                                          const int32_t* __restrict__ desc, int squared,
                                                          const double* __restrict__ emd, const int32_t* __restrict__ assignment,
                                                          const int32_t* __restrict__ inverse, const double* __restrict__ gemd,
                                                          T* __restrict__ dpred, T* __restrict__ dgt) {
#pragma clang fp contract(off)
  const int p = blockIdx.x, i = blockIdx.y * kEmBwThreads + threadIdx.x;
  const int p0 = desc[4 * p], n = desc[4 * p + 1], g0 = desc[4 * p + 2];
  if (i >= n) return;
  const double e = emd[p];
  const bool live = e == e && gemd != nullptr;  // a pair that did not converge has no gradient
  const double w = live ? gemd[p] / (double)n : 0.0;
  auto load = [](const T* q, double out[3]) { out[0] = (double)q[0]; out[1] = (double)q[1]; out[2] = (double)q[2]; };
  double a[3], b[3], c[3];
  if (dpred) {
    const int j = assignment[(size_t)p0 + i];
    c[0] = c[1] = c[2] = 0.0;
    if (live && j >= 0 && j < n) {
      load(pred + 3 * ((size_t)p0 + i), a);
      load(gt + 3 * ((size_t)g0 + j), b);
      em_term(a, b, w, squared, c);
    }
    T* o = dpred + 3 * ((size_t)p0 + i);
    o[0] = (T)c[0]; o[1] = (T)c[1]; o[2] = (T)c[2];
  }
  if (dgt) {
    const int k = inverse[(size_t)g0 + i];
    c[0] = c[1] = c[2] = 0.0;
    if (live && k >= 0 && k < n) {
      load(pred + 3 * ((size_t)p0 + k), a);
      load(gt + 3 * ((size_t)g0 + i), b);
      em_term(a, b, w, squared, c);
    }
    T* o = dgt + 3 * ((size_t)g0 + i);
    o[0] = (T)-c[0]; o[1] = (T)-c[1]; o[2] = (T)-c[2];
  }
}

// Every pair has pred_count == gt_count in [1, DPC_EMD_MAX_POINTS], and the pairs' ranges ascend without overlap in
// both buffers (the outputs are indexed like the inputs); *n_cap = the largest count.
int em_check(int pairs, const int32_t* desc, int64_t n_pred, int64_t n_gt, int* n_cap) {
  if (pairs < 0) return DPC_ERR_SHAPE;
  if (pairs > 0 && !desc) return DPC_ERR_NULL;
  const int rc = check_desc<4>(desc, pairs, {n_pred, n_gt}, INT64_MAX, nullptr, [](const int32_t* d) {
    return d[1] == d[3] && d[1] >= 1 && d[1] <= DPC_EMD_MAX_POINTS;
  });
  if (rc != DPC_OK) return rc;
  int cap = 0;
  for (int p = 0; p < pairs; ++p) {
    const int32_t* d = desc + 4 * (int64_t)p;
    if (p > 0 && ((int64_t)d[-4] + d[-3] > d[0] || (int64_t)d[-2] + d[-1] > d[2])) return DPC_ERR_SHAPE;
    cap = d[1] > cap ? d[1] : cap;
  }
  if (n_cap) *n_cap = cap;
  return DPC_OK;
}

template <class T>
int em_fwd(const T* pred, int n_pred, const T* gt, int n_gt, const int32_t* desc, int pairs, int n_cap, int squared, double eps,
           int max_rounds, double* emd, int32_t* assignment, int32_t* inverse, int32_t* rounds, int32_t* status, hipStream_t st) {
  static LdsLimit limit;  // the largest pair's size, so one driver call per kernel and device
  const int rc = set_lds(k_emd_auction<T>, em_lds_bytes(DPC_EMD_MAX_POINTS), limit);
  if (rc != DPC_OK) return rc;
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  DPC_LAUNCH("k_emd_auction", dpc_kid(kIsF64 ? "k_emd_auction<double>" : "k_emd_auction<float>"), k_emd_auction<T>,
             dim3((unsigned)pairs), dim3(kEmThreads), em_lds_bytes(n_cap), st, pred, n_pred, gt, n_gt, desc, n_cap, squared, eps,
             max_rounds, emd, assignment, inverse, rounds, status);
  return launch_ok();
}

template <class T>
int em_bwd(const T* pred, const T* gt, const int32_t* desc, int pairs, int n_cap, int squared, const double* emd,
           const int32_t* assignment, const int32_t* inverse, const double* gemd, T* dpred, T* dgt, hipStream_t st) {
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  DPC_LAUNCH("k_emd_bwd", dpc_kid(kIsF64 ? "k_emd_bwd<double>" : "k_emd_bwd<float>"), k_emd_bwd<T>,
             dim3((unsigned)pairs, (unsigned)((n_cap + kEmBwThreads - 1) / kEmBwThreads)), dim3(kEmBwThreads), 0, st, pred, gt,
             desc, squared, emd, assignment, inverse, gemd, dpred, dgt);
  return launch_ok();
}

}  // namespace

extern "C" {

size_t dpc_emd_lds_bytes(int n) { return n >= 1 && n <= DPC_EMD_MAX_POINTS ? em_lds_bytes(n) : 0; }

int dpc_emd_fwd(const void* pred, int n_pred, const void* gt, int n_gt, int is_f64, const int32_t* pair_desc,
                const int32_t* host_pair_desc, int pairs, int squared, double eps, int max_rounds, double* emd,
                int32_t* assignment, int32_t* inverse, int32_t* rounds, int32_t* status, void* stream) {
  if (n_pred < 0 || n_gt < 0 || !(eps > 0.0) || !std::isfinite(eps) || max_rounds < 1) return DPC_ERR_SHAPE;
  int n_cap = 0;
  const int rc = em_check(pairs, host_pair_desc, n_pred, n_gt, &n_cap);
  if (rc != DPC_OK) return rc;
  if (pairs == 0) return DPC_OK;
  if (!pred || !gt || !pair_desc || !emd || !assignment || !inverse || !rounds) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return em_fwd<double>(static_cast<const double*>(pred), n_pred, static_cast<const double*>(gt), n_gt, pair_desc, pairs, n_cap,
                          squared, eps, max_rounds, emd, assignment, inverse, rounds, status, st);
  return em_fwd<float>(static_cast<const float*>(pred), n_pred, static_cast<const float*>(gt), n_gt, pair_desc, pairs, n_cap,
                       squared, eps, max_rounds, emd, assignment, inverse, rounds, status, st);
}

int dpc_emd_bwd(const void* pred, int n_pred, const void* gt, int n_gt, int is_f64, const int32_t* pair_desc,
                const int32_t* host_pair_desc, int pairs, int squared, const double* emd, const int32_t* assignment,
                const int32_t* inverse, const double* gemd, void* dpred, void* dgt, void* stream) {
  if (n_pred < 0 || n_gt < 0) return DPC_ERR_SHAPE;
  int n_cap = 0;
  const int rc = em_check(pairs, host_pair_desc, n_pred, n_gt, &n_cap);
  if (rc != DPC_OK) return rc;
  if (pairs == 0) return DPC_OK;
  if (!pred || !gt || !pair_desc || !emd || !assignment || !inverse || (!dpred && !dgt)) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return em_bwd<double>(static_cast<const double*>(pred), static_cast<const double*>(gt), pair_desc, pairs, n_cap, squared, emd,
                          assignment, inverse, gemd, static_cast<double*>(dpred), static_cast<double*>(dgt), st);
  return em_bwd<float>(static_cast<const float*>(pred), static_cast<const float*>(gt), pair_desc, pairs, n_cap, squared, emd,
                       assignment, inverse, gemd, static_cast<float*>(dpred), static_cast<float*>(dgt), st);
}

}  // extern "C"
