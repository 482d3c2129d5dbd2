// The nearest-target scan shared by k_nearest_partial (dpc_nearest.hip) and k_chamfer_partial (dpc_chamfer.hip), so the
// two cannot drift: both are pinned bit for bit against the reference's point_cloud_distance (F11, F16).  Also the rule
// that slices the targets of a search, shared by those two and dpc_icp.hip (nearest_slice).
//
// One lane owns one source point (sx, sy, sz); targets vt[j0, j1) stream through the LDS tiles tx / ty / tz, whole block
// cooperating (every thread of the block must call this with the same j0, j1).  Arithmetic follows the reference op for
// op, in T:  d = Vt - Vs;  d2 = (d0*d0 + d1*d1) + d2*d2 (no FMA contraction);  dist = sqrt(d2) correctly rounded.
// "First minimum of dist" is not the same as "first minimum of d2" when two different d2 round to one sqrt, so near ties
// are decided on the sqrt values themselves (see `consider` below); everything else is decided on d2, sqrt being
// monotone.  On return best_d2 / best hold the winner of the range (best = j0 and best_d2 = inf for an empty range).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

// Targets per slice when the targets of a search are split over workgroups (dpc_point_cloud_distance,
// dpc_nearest_batched, dpc_icp_point_to_point): enough slices that (source blocks x slices) comes close to a multiple of
// four workgroups per CU, slices of whole 256-target groups (every resident block then carries the same load: 800 blocks
// on 256 CUs ran 22 % slower than 992).  src_blocks: the blocks of 256 sources; the callers count them in int, which
// wraps to <= 0 for a source count within 255 of 2^31, and such a count asks for a single slice (never a division by
// it).  max_nt >= 1: the targets in the largest set.  The slice exceeds int32 only for max_nt within 255 of 2^31; the
// callers narrow it to the kernels' int.
inline int64_t nearest_slice(int64_t src_blocks, int64_t max_nt) {
  int64_t want = src_blocks > 0 ? (1024 + src_blocks - 1) / src_blocks : 1;
  const int64_t max_slices = (max_nt + 255) / 256;
  if (want > max_slices) want = max_slices;
  const int64_t slice = (max_nt + want - 1) / want;
  return ((slice + 255) / 256) * 256;
}

template <class T, int kThreads, int kTile>
__device__ __forceinline__ void nearest_scan(const T* __restrict__ vt, int j0, int j1, T sx, T sy, T sz, T* tx, T* ty, T* tz,
                                             T& best_d2_out, int& best_out) {
#pragma clang fp contract(off)
  const T kNearTie = (T)1 - (T)16 * std::numeric_limits<T>::epsilon();
  T best_d2 = std::numeric_limits<T>::infinity();
  int best = j0;
  for (int base = j0; base < j1; base += kTile) {
    const int n = min(kTile, j1 - base);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kThreads) {
      const T* p = vt + 3 * (size_t)(base + k);
      tx[k] = p[0]; ty[k] = p[1]; tz[k] = p[2];
    }
    __syncthreads();
    // Four candidates per step; the sqrt-and-compare runs only when some lane of the wave has a candidate below its
    // incumbent (a wave-uniform branch: left as a per-lane condition the compiler evaluates the sqrt for every pair).
    auto pair_d2 = [&](int k) {
      const T d0 = tx[k] - sx, d1 = ty[k] - sy, d2c = tz[k] - sz;
      return (d0 * d0 + d1 * d1) + d2c * d2c;
    };
    // A candidate whose d2 is below the incumbent's by more than a few ulps has a strictly smaller sqrt: taken without
    // evaluating it.  Within that margin (a near tie, ~1e-6 of the improvements) both square roots are evaluated,
    // correctly rounded, and the candidate wins only if its distance is strictly smaller -- the incumbent, which has the
    // smaller index, keeps ties, exactly like argmin over the sqrt values.
    auto consider = [&](T d2, int j) {
      const bool better = d2 < best_d2;
      const bool near_tie = better && d2 >= best_d2 * kNearTie;
      if (__builtin_amdgcn_ballot_w64(near_tie) != 0ull) {
        const bool wins = better && (!near_tie || sqrt(d2) < sqrt(best_d2));
        if (wins) { best_d2 = d2; best = j; }
      } else if (better) {
        best_d2 = d2; best = j;
      }
    };
    int k = 0;
    for (; k + 4 <= n; k += 4) {
      const T a = pair_d2(k), b = pair_d2(k + 1), c = pair_d2(k + 2), d = pair_d2(k + 3);
      const T m = fmin(fmin(a, b), fmin(c, d));
      if (__builtin_amdgcn_ballot_w64(m < best_d2) != 0ull) {
        consider(a, base + k); consider(b, base + k + 1); consider(c, base + k + 2); consider(d, base + k + 3);
      }
    }
    for (; k < n; ++k) consider(pair_d2(k), base + k);
  }
  best_d2_out = best_d2;
  best_out = best;
}
