// Batched k-nearest-neighbour search and PCA surface normals.  Semantics in include/dpc_render.h (dpc_knn_batched,
// dpc_pca_normals); tests/normals_oracle.py restates them in numpy.
//
// All clouds live in one packed buffer; `rows` rows (q_start, q_count, r_start, r_count) index it.  Two kernels, no
// workspace, no atomics but the status word:
//   k_knn          one block per (row, block of B queries), one lane per query.  The row's references stream through LDS
//                  tiles of kKnnTile points, whole block cooperating, in index order; each lane keeps its k best (d2, j)
//                  sorted in LDS, laid out [slot][lane] (a wave touches one slot at 64 consecutive addresses: no bank
//                  conflict, and no runtime-indexed register array, which would go to scratch), and its k-th best d2 in a
//                  register: a candidate is rejected with one compare, and four candidates at once when no lane of the
//                  wave has one below its threshold.  References arrive in increasing j, so "strictly below the k-th
//                  best, inserted behind its equals" is exactly the order by (d2, j).  B shrinks with k (knn_block) so
//                  that the lists fit; the lists are written out by the whole block, coalesced.
//   k_pca_normals  one lane per query: mean and covariance of its neighbours in two passes, a cyclic Jacobi iteration on
//                  the trace-scaled 3x3 matrix, the sign rule.  All fp64.
// The launch grid is (query blocks of the longest row, rows): a block finds its row by blockIdx.y, leaves at once when
// its row has no such block, and otherwise sums the q_count of the rows before its own (its place in the packed outputs)
// from the device table.  That costs rows / B loads per thread next to a scan of thousands of references, and it is
// what lets the call run without a workspace or a prefix kernel.
// Compute-bound on the fp32 / fp64 vector pipe in k_knn: sum over rows of q_count x r_count d2s of 8 operations each.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kKnnTile = DPC_KNN_TILE;   // references staged per LDS tile (6 KiB fp32, 12 KiB fp64)
constexpr int kPcaBlock = 256;
constexpr int kGridRows = 65535;         // rows per launch (gridDim.y)

// Queries per workgroup.  LDS per workgroup = B k (sizeof(T) + 4) + 3 kKnnTile sizeof(T): at most 60 KiB (fp64 with k at
// the top of its band), 38 KiB in fp32, so a CU's 160 KiB hold two workgroups in fp64 and four in fp32 at every k.
inline int knn_block(int k) { return DPC_KNN_BLOCK(k); }

extern __shared__ double knn_lds[];

struct KnnRow {
  int qs, nq, rs, nr;
  int64_t out0;   // queries of the rows before this one
};

// The row of this block and its place in the packed outputs; false when the block has nothing to do.  Every thread of
// the block calls it (barriers inside; the early returns are block-uniform).  A device row that does not lie inside
// pts, or whose outputs would not lie inside the total_q queries the host counted, sets DPC_STATUS_BAD_INDEX and is
// not run.
template <int B>
__device__ bool knn_row(const int32_t* __restrict__ desc, int r, int n_pts, int total_q, int32_t* status, KnnRow* row) {
  __shared__ int64_t red[B / 64];
  const int t = threadIdx.x;
  const int32_t* d = desc + 4 * (size_t)r;
  const int qs = d[0], nq = d[1], rs = d[2], nr = d[3];
  if (nq <= 0 || (int64_t)blockIdx.x * B >= nq) return false;
  int64_t s = 0;
  bool neg = false;
  for (int i = t; i < r; i += B) {
    const int c = desc[4 * (size_t)i + 1];
    neg |= c < 0;
    s += c;
  }
  if (neg) s = -1 - (int64_t)total_q;   // poisons the sum below: a negative count is a bad table
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  int64_t out0 = 0;
#pragma unroll
  for (int w = 0; w < B / 64; ++w) out0 += red[w];
  const bool ok = qs >= 0 && rs >= 0 && nr >= 0 && (int64_t)qs + nq <= n_pts && (int64_t)rs + nr <= n_pts && out0 >= 0 &&
                  out0 + nq <= total_q;
  if (!ok) {
    if (t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return false;
  }
  *row = KnnRow{qs, nq, rs, nr, out0};
  return true;
}

template <class T>
__device__ __forceinline__ bool knn_finite(T x) { return fabs(x) <= std::numeric_limits<T>::max(); }

template <class T, int B>
__global__ __launch_bounds__(B) void k_knn(const T* __restrict__ pts, int n_pts, const int32_t* __restrict__ desc, int row0,
                                           int k, int total_q, int32_t* __restrict__ idx, T* __restrict__ d2out,
                                           int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  KnnRow row;
  if (!knn_row<B>(desc, row0 + (int)blockIdx.y, n_pts, total_q, status, &row)) return;
  const int t = threadIdx.x;
  T* ld = reinterpret_cast<T*>(knn_lds);                // [k][B] the lists' d2, ascending in the slot
  T* tx = ld + (size_t)k * B;                           // [kKnnTile] x 3: the staged references
  T* ty = tx + kKnnTile;
  T* tz = ty + kKnnTile;
  int* li = reinterpret_cast<int*>(tz + kKnnTile);      // [k][B] the lists' indices
  const T inf = std::numeric_limits<T>::infinity();
  for (int s = 0; s < k; ++s) { ld[s * B + t] = inf; li[s * B + t] = -1; }
  const int q0 = blockIdx.x * B;
  const int i = q0 + t;
  const bool live = i < row.nq;
  T sx = 0, sy = 0, sz = 0;
  if (live) {
    const T* q = pts + 3 * ((size_t)row.qs + i);
    sx = q[0]; sy = q[1]; sz = q[2];
  }
  const bool q_odd = !(knn_finite(sx) && knn_finite(sy) && knn_finite(sz));
  // filled: entries in the list; thr: the k-th best d2 once it is full (a lane without a query takes nothing)
  int filled = live ? 0 : k;
  T thr = live ? inf : -inf;
  bool saw_nan = false;
  const T* ref = pts + 3 * (size_t)row.rs;

  auto insert = [&](T d, int j) {
    int pos = filled < k ? filled : k - 1;
    while (pos > 0) {
      const T prev = ld[(pos - 1) * B + t];
      if (!(prev > d)) break;   // equals stay in front: they have the lower index
      ld[pos * B + t] = prev;
      li[pos * B + t] = li[(pos - 1) * B + t];
      --pos;
    }
    ld[pos * B + t] = d;
    li[pos * B + t] = j;
    if (filled < k) ++filled;
    if (filled == k) thr = ld[(k - 1) * B + t];
  };
  auto pair_d2 = [&](int c) {
    const T d0 = tx[c] - sx, d1 = ty[c] - sy, d2c = tz[c] - sz;
    return (d0 * d0 + d1 * d1) + d2c * d2c;
  };

  for (int base = 0; base < row.nr; base += kKnnTile) {   // the same trip count in every thread: barriers inside
    const int n = min(kKnnTile, row.nr - base);
    __syncthreads();
    int odd = 0;
    for (int c = t; c < n; c += B) {
      const T* p = ref + 3 * (size_t)(base + c);
      const T x = p[0], y = p[1], z = p[2];
      tx[c] = x; ty[c] = y; tz[c] = z;
      odd |= !(knn_finite(x) && knn_finite(y) && knn_finite(z));
    }
    // A d2 of finite coordinates is finite or +inf, never NaN: only a tile with a NaN or infinite coordinate, or a wave
    // with such a query, looks at every candidate for NaN.
    const bool tile_odd = __syncthreads_or(odd) != 0;
    if (tile_odd || __builtin_amdgcn_ballot_w64(q_odd) != 0ull) {
      for (int c = 0; c < n; ++c) {
        const T d = pair_d2(c);
        if (d != d) saw_nan |= live;
        else if (filled < k || d < thr) insert(d, base + c);
      }
      continue;
    }
    int c = 0;
    for (; c + 4 <= n; c += 4) {
      const T a = pair_d2(c), b = pair_d2(c + 1), e = pair_d2(c + 2), f = pair_d2(c + 3);
      const T m = fmin(fmin(a, b), fmin(e, f));
      if (__builtin_amdgcn_ballot_w64(filled < k || m < thr) != 0ull) {
        if (filled < k || a < thr) insert(a, base + c);
        if (filled < k || b < thr) insert(b, base + c + 1);
        if (filled < k || e < thr) insert(e, base + c + 2);
        if (filled < k || f < thr) insert(f, base + c + 3);
      }
    }
    for (; c < n; ++c) {
      const T d = pair_d2(c);
      if (filled < k || d < thr) insert(d, base + c);
    }
  }
  if (saw_nan && status) atomicOr(status, (int)DPC_STATUS_NONFINITE);
  __syncthreads();
  // the block's lists are one contiguous piece of the outputs: written by the whole block in output order
  const int nq = min(B, row.nq - q0);
  const size_t out = ((size_t)row.out0 + q0) * k;
  for (int e = t; e < nq * k; e += B) {
    const int qi = e / k, s = e - qi * k;
    idx[out + e] = li[s * B + qi];
    if (d2out) d2out[out + e] = ld[s * B + qi];
  }
}

// One Jacobi rotation that zeroes a_pq of the symmetric matrix (a_pp, a_qq on the diagonal; a_rp, a_rq the third
// row's entries) and applies it to the columns p, q of the eigenvector matrix.
__device__ __forceinline__ void pca_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (fabs(apq) <= 0x1p-70) {   // the matrix has trace 1: below this the rotation moves nothing by 2^-18 of the tolerance
    apq = 0.0;
    return;
  }
  const double theta = (aqq - app) / (2.0 * apq);
  const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double tn = theta < 0.0 ? -tt : tt;
  const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
  app -= tn * apq;
  aqq += tn * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

template <class T>
__global__ __launch_bounds__(kPcaBlock) void k_pca_normals(const T* __restrict__ pts, int n_pts, const int32_t* __restrict__ desc,
                                                           int row0, int k, int total_q, const int32_t* __restrict__ idx,
                                                           const double* __restrict__ viewpoints, double* __restrict__ normals,
                                                           double* __restrict__ evals, int32_t* __restrict__ status) {
#pragma clang fp contract(fast)
  KnnRow row;
  const int r = row0 + (int)blockIdx.y;
  if (!knn_row<kPcaBlock>(desc, r, n_pts, total_q, status, &row)) return;
  const int i = blockIdx.x * kPcaBlock + threadIdx.x;
  if (i >= row.nq) return;
  const size_t o = (size_t)row.out0 + i;
  const int32_t* my = idx + o * k;
  const T* ref = pts + 3 * (size_t)row.rs;
  int c = 0;
  bool bad = false;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int s = 0; s < k; ++s) {
    const int j = my[s];
    if (j >= 0 && j < row.nr) {
      const T* p = ref + 3 * (size_t)j;
      sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
      ++c;
    } else if (j != -1) {
      bad = true;   // never an address: counted as an invalid slot
    }
  }
  if (bad && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
  const double cn = c > 0 ? (double)c : 1.0;
  const double mx = sx / cn, my_ = sy / cn, mz = sz / cn;
  double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  for (int s = 0; s < k; ++s) {
    const int j = my[s];
    if (j >= 0 && j < row.nr) {
      const T* p = ref + 3 * (size_t)j;
      const double dx = (double)p[0] - mx, dy = (double)p[1] - my_, dz = (double)p[2] - mz;
      cxx += dx * dx; cxy += dx * dy; cxz += dx * dz;
      cyy += dy * dy; cyz += dy * dz; czz += dz * dz;
    }
  }
  cxx /= cn; cxy /= cn; cxz /= cn; cyy /= cn; cyz /= cn; czz /= cn;
  const double tr = (cxx + cyy) + czz;
  const double sc = tr > 0.0 ? tr : 1.0;
  double a00 = cxx / sc, a01 = cxy / sc, a02 = cxz / sc, a11 = cyy / sc, a12 = cyz / sc, a22 = czz / sc;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    pca_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (p, q) = (0, 1), third row 2
    pca_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third row 1
    pca_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third row 0
  }
  // the eigenvector of the smallest eigenvalue (the first of equals), and the eigenvalues in ascending order
  // (selects on purpose: written as three-way branches the compiler builds an indexed array in scratch)
  const bool s1 = a11 < a00;
  const double l01 = s1 ? a11 : a00;
  const bool s2 = a22 < l01;
  double nx = s2 ? v02 : s1 ? v01 : v00, ny = s2 ? v12 : s1 ? v11 : v10, nz = s2 ? v22 : s1 ? v21 : v20;
  const double e0 = fmin(fmin(a00, a11), a22), e2 = fmax(fmax(a00, a11), a22);
  const double e1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
  if (evals) {   // C is positive semi-definite: a rounding below zero is moved onto it
    evals[3 * o] = fmax(e0, 0.0) * sc;
    evals[3 * o + 1] = fmax(e1, 0.0) * sc;
    evals[3 * o + 2] = fmax(e2, 0.0) * sc;
  }
  if (c < 3) {
    nx = ny = nz = 0.0;
  } else {
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= len; ny /= len; nz /= len;
    bool flip;
    if (viewpoints) {
      const T* q = pts + 3 * ((size_t)row.qs + i);
      const double* vp = viewpoints + 3 * (size_t)r;
      flip = nx * (vp[0] - (double)q[0]) + ny * (vp[1] - (double)q[1]) + nz * (vp[2] - (double)q[2]) < 0.0;
    } else {   // the component of largest magnitude is positive; the lowest axis wins equal magnitudes
      const double b01 = fabs(ny) > fabs(nx) ? ny : nx;
      const double big = fabs(nz) > fabs(b01) ? nz : b01;
      flip = big < 0.0;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
  }
  normals[3 * o] = nx; normals[3 * o + 1] = ny; normals[3 * o + 2] = nz;
}

// DPC_ERR_SHAPE, or DPC_OK with the queries of all rows in *total and the longest row's in *max_q.
int knn_check(int rows, const int32_t* desc, int64_t n_pts, int k, int64_t* total, int* max_q) {
  const int64_t len[2] = {n_pts, n_pts};
  int mq = 0;
  const int rc = check_desc<4, 2>(desc, rows, len, INT32_MAX / k, total, [&](const int32_t* d) {
    if (d[1] > mq) mq = d[1];
    return true;
  });
  *max_q = mq;
  return rc;
}

template <class T, int B>
void knn_launch(const T* pts, int n_pts, const int32_t* desc, int rows, int k, int max_q, int total_q, int32_t* idx, T* d2,
                int32_t* status, hipStream_t st) {
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  const size_t lds = (size_t)B * k * (sizeof(T) + sizeof(int)) + 3 * (size_t)kKnnTile * sizeof(T);
  const unsigned gx = (unsigned)((max_q + B - 1) / B);
  for (int row0 = 0; row0 < rows; row0 += kGridRows) {
    const unsigned gy = (unsigned)(rows - row0 < kGridRows ? rows - row0 : kGridRows);
    DPC_LAUNCH("k_knn", dpc_kid("k_knn", kIsF64 ? 1 : 0, B), (k_knn<T, B>), dim3(gx, gy), dim3(B), lds, st, pts, n_pts, desc, row0,
               k, total_q, idx, d2, status);
  }
}

template <class T>
int knn_impl(const void* pts, int n_pts, const int32_t* desc, int rows, int k, int max_q, int total_q, int32_t* idx, void* d2,
             int32_t* status, hipStream_t st) {
  const T* p = static_cast<const T*>(pts);
  T* d = static_cast<T*>(d2);
  switch (knn_block(k)) {
    case 256: knn_launch<T, 256>(p, n_pts, desc, rows, k, max_q, total_q, idx, d, status, st); break;
    case 128: knn_launch<T, 128>(p, n_pts, desc, rows, k, max_q, total_q, idx, d, status, st); break;
    default: knn_launch<T, 64>(p, n_pts, desc, rows, k, max_q, total_q, idx, d, status, st); break;
  }
  return launch_ok();
}

template <class T>
int pca_impl(const void* pts, int n_pts, const int32_t* desc, int rows, int k, int max_q, int total_q, const int32_t* idx,
             const double* viewpoints, double* normals, double* evals, int32_t* status, hipStream_t st) {
  constexpr bool kIsF64 = sizeof(T) == sizeof(double);
  const unsigned gx = (unsigned)((max_q + kPcaBlock - 1) / kPcaBlock);
  for (int row0 = 0; row0 < rows; row0 += kGridRows) {
    const unsigned gy = (unsigned)(rows - row0 < kGridRows ? rows - row0 : kGridRows);
    DPC_LAUNCH("k_pca_normals", dpc_kid("k_pca_normals", kIsF64 ? 1 : 0), k_pca_normals<T>, dim3(gx, gy), dim3(kPcaBlock), 0, st,
               static_cast<const T*>(pts), n_pts, desc, row0, k, total_q, idx, viewpoints, normals, evals, status);
  }
  return launch_ok();
}

}  // namespace

extern "C" {

int dpc_knn_batched(const void* pts, int n_pts, int is_f64, const int32_t* row_desc, const int32_t* host_row_desc, int rows, int k,
                    int32_t* idx, void* d2, int32_t* status, void* stream) {
  if (rows < 0 || n_pts < 0 || k < 1 || k > DPC_KNN_MAX_K) return DPC_ERR_SHAPE;
  if (rows == 0) return DPC_OK;
  if (!host_row_desc) return DPC_ERR_NULL;
  int64_t total = 0;
  int max_q = 0;
  const int rc = knn_check(rows, host_row_desc, n_pts, k, &total, &max_q);
  if (rc != DPC_OK) return rc;
  if (total == 0) return DPC_OK;
  if (!pts || !row_desc || !idx) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) return knn_impl<double>(pts, n_pts, row_desc, rows, k, max_q, (int)total, idx, d2, status, st);
  return knn_impl<float>(pts, n_pts, row_desc, rows, k, max_q, (int)total, idx, d2, status, st);
}

int dpc_pca_normals(const void* pts, int n_pts, int is_f64, const int32_t* row_desc, const int32_t* host_row_desc, int rows, int k,
                    const int32_t* idx, const double* viewpoints, double* normals, double* eigenvalues, int32_t* status,
                    void* stream) {
  if (rows < 0 || n_pts < 0 || k < 1 || k > DPC_KNN_MAX_K) return DPC_ERR_SHAPE;
  if (rows == 0) return DPC_OK;
  if (!host_row_desc) return DPC_ERR_NULL;
  int64_t total = 0;
  int max_q = 0;
  const int rc = knn_check(rows, host_row_desc, n_pts, k, &total, &max_q);
  if (rc != DPC_OK) return rc;
  if (total == 0) return DPC_OK;
  if (!pts || !row_desc || !idx || !normals) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    return pca_impl<double>(pts, n_pts, row_desc, rows, k, max_q, (int)total, idx, viewpoints, normals, eigenvalues, status, st);
  return pca_impl<float>(pts, n_pts, row_desc, rows, k, max_q, (int)total, idx, viewpoints, normals, eigenvalues, status, st);
}

}  // extern "C"
