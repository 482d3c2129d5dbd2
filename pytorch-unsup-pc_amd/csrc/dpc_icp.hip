// Batched point-to-point ICP: open3d 0.9's RegistrationICP with TransformationEstimationPointToPoint(with_scaling=False)
// and the default ICPConvergenceCriteria, the alignment step of the reference's unsupervised evaluation
// (dpc/run/compute_alignment.py:28-127, open3d_icp / alignment_to_ground_truth).  Semantics in include/dpc_render.h.
//
// P (source, target) pairs run in one call, all in fp64.  Per pair the working copy of the source cloud is transformed in
// place and cumulatively, like open3d's pcd.Transform(update).  One round is three launches:
//   k_icp_partial  blocks (256 sources, pair, target slice): the pending update U is applied to the source point on load,
//                  the targets of the slice stream through LDS (24 KiB per tile), nearest by d2, first index on ties;
//   k_icp_merge    blocks (256 sources, pair): merges the slices in slice order, writes the transformed point back, tests
//                  d2 < tau2 and block-reduces the 17 fp64 moments of the inliers into one partial per block;
//   k_icp_solve    one lane per pair: sums the block partials in block order, evaluates fitness / inlier_rmse, tests
//                  convergence, solves the 3x3 alignment (Horn's quaternion eigenproblem, Jacobi) and composes T.
// Nothing is atomic, so results are bit-identical from run to run.  Converged pairs set a flag and their blocks return.
// The host issues max_iter + 1 rounds without synchronising; rounds after every pair is done cost three empty launches.
// Compute-bound on the fp64 vector pipe: pairs x rounds x n_src x n_tgt evaluations of d2 (about a dozen instructions).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_nearest.h"
#include "dpc_launch.h"

namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpTile = 1024;  // targets staged per LDS tile (24 KiB fp64)
constexpr int kIcpMoments = 17;  // n, sum d2, sum p (3), sum q (3), sum q p^T (9), p and q about the pair's anchor
constexpr int kIcpState = 32;    // per pair: U (12: R row-major, then t), T (16), previous fitness, previous rmse

struct IcpGeom {
  int max_ns, max_nt, src_blocks, slice, nslice;
};

// From the source and target count of every pair: src_count[p * stride], tgt_count[p * stride].
IcpGeom icp_geometry(int pairs, const int32_t* src_count, const int32_t* tgt_count, int stride) {
  IcpGeom g{0, 0, 0, 256, 1};
  for (int p = 0; p < pairs; ++p) {
    const int ns = src_count[(size_t)p * stride], nt = tgt_count[(size_t)p * stride];
    g.max_ns = ns > g.max_ns ? ns : g.max_ns;
    g.max_nt = nt > g.max_nt ? nt : g.max_nt;
  }
  g.src_blocks = g.max_ns > 0 ? (g.max_ns + kIcpThreads - 1) / kIcpThreads : 1;
  if (g.max_nt > 0) {  // target slices by nearest_slice (dpc_nearest.h), every pair with the batch's source blocks
    g.slice = (int)nearest_slice((int64_t)pairs * g.src_blocks, g.max_nt);
    g.nslice = (g.max_nt + g.slice - 1) / g.slice;
  }
  return g;
}

struct IcpWork {
  double* cur;      // [P, max_ns, 3] working copy of the source clouds
  double* part_d2;  // [nslice, P, max_ns]
  int* part_idx;    // [nslice, P, max_ns]
  double* mom;      // [P, src_blocks, 17]
  double* state;    // [P, 32]
  int* done;        // [P]
};

size_t icp_carve(const IcpGeom& g, int pairs, char* base, IcpWork* w) {
  const size_t pts = (size_t)pairs * g.max_ns;
  Carver c{base};
  IcpWork t;
  t.cur = c.take<double>(pts * 3);
  t.part_d2 = c.take<double>((size_t)g.nslice * pts);
  t.part_idx = c.take<int>((size_t)g.nslice * pts);
  t.mom = c.take<double>((size_t)pairs * g.src_blocks * kIcpMoments);
  t.state = c.take<double>((size_t)pairs * kIcpState);
  t.done = c.take<int>(pairs);
  if (w) *w = t;
  return c.off + 16;
}

// x' = R x + t, each row summed left to right without FMA contraction (the numpy restatement in the tests does the same)
__device__ inline void apply_rt(const double* __restrict__ u, double x, double y, double z, double* o) {
#pragma clang fp contract(off)
  o[0] = ((u[0] * x + u[1] * y) + u[2] * z) + u[9];
  o[1] = ((u[3] * x + u[4] * y) + u[5] * z) + u[10];
  o[2] = ((u[6] * x + u[7] * y) + u[8] * z) + u[11];
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_init(const double* __restrict__ src, const int32_t* __restrict__ desc,
                                                          const double* __restrict__ init, int max_ns, IcpWork w) {
  const int p = blockIdx.y;
  const int ns = desc[4 * p + 1];
  const int i = blockIdx.x * kIcpThreads + threadIdx.x;
  if (i < ns) {
    const double* s = src + 3 * ((size_t)desc[4 * p] + i);
    double* c = w.cur + 3 * ((size_t)p * max_ns + i);
    c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
  }
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    const int k = threadIdx.x, r = k >> 2, col = k & 3;
    const double v = init[16 * (size_t)p + k];
    double* st = w.state + (size_t)p * kIcpState;
    st[12 + k] = v;                           // T = init
    if (r < 3) st[col < 3 ? 3 * r + col : 9 + r] = v;  // U = the 3x4 top of init (pending for round 0)
    if (k == 0) { st[28] = 0.0; st[29] = 0.0; w.done[p] = 0; }
  }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_partial(const double* __restrict__ tgt, const int32_t* __restrict__ desc,
                                                             int max_ns, int slice, IcpWork w) {
#pragma clang fp contract(off)
  __shared__ double tx[kIcpTile], ty[kIcpTile], tz[kIcpTile];
  const int p = blockIdx.y;
  if (w.done[p]) return;
  const int ns = desc[4 * p + 1], t0 = desc[4 * p + 2], nt = desc[4 * p + 3];
  const int j0 = blockIdx.z * slice;
  if (blockIdx.x * kIcpThreads >= ns || j0 >= nt) return;  // block-uniform
  const int j1 = min(nt, j0 + slice);
  const int i = blockIdx.x * kIcpThreads + threadIdx.x;
  const bool live = i < ns;
  double u[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) u[k] = w.state[(size_t)p * kIcpState + k];
  double s[3] = {0.0, 0.0, 0.0};
  if (live) {
    const double* c = w.cur + 3 * ((size_t)p * max_ns + i);
    apply_rt(u, c[0], c[1], c[2], s);
  }
  const double* vt = tgt + 3 * (size_t)t0;
  double best_d2 = std::numeric_limits<double>::infinity();
  int best = j0;
  for (int base = j0; base < j1; base += kIcpTile) {
    const int n = min(kIcpTile, j1 - base);
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kIcpThreads) {
      const double* q = vt + 3 * (size_t)(base + k);
      tx[k] = q[0]; ty[k] = q[1]; tz[k] = q[2];
    }
    __syncthreads();
    auto pair_d2 = [&](int k) {
      const double d0 = tx[k] - s[0], d1 = ty[k] - s[1], d2 = tz[k] - s[2];
      return (d0 * d0 + d1 * d1) + d2 * d2;
    };
    // strict < keeps the first index among equal d2; the four-candidate compare-and-update runs only when some lane of
    // the wave improves (a wave-uniform branch, as in k_nearest_partial)
    int k = 0;
    for (; k + 4 <= n; k += 4) {
      const double a = pair_d2(k), b = pair_d2(k + 1), c = pair_d2(k + 2), d = pair_d2(k + 3);
      const double m = fmin(fmin(a, b), fmin(c, d));
      if (__builtin_amdgcn_ballot_w64(m < best_d2) != 0ull) {
        if (a < best_d2) { best_d2 = a; best = base + k; }
        if (b < best_d2) { best_d2 = b; best = base + k + 1; }
        if (c < best_d2) { best_d2 = c; best = base + k + 2; }
        if (d < best_d2) { best_d2 = d; best = base + k + 3; }
      }
    }
    for (; k < n; ++k) {
      const double a = pair_d2(k);
      if (a < best_d2) { best_d2 = a; best = base + k; }
    }
  }
  if (live) {
    const size_t o = ((size_t)blockIdx.z * gridDim.y + p) * max_ns + i;
    w.part_d2[o] = best_d2;
    w.part_idx[o] = best;
  }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_merge(const double* __restrict__ tgt, const int32_t* __restrict__ desc,
                                                           int max_ns, int slice, int src_blocks, double tau2, IcpWork w) {
#pragma clang fp contract(off)
  __shared__ double red[kIcpThreads / 64][kIcpMoments];
  const int p = blockIdx.y;
  if (w.done[p]) return;
  const int ns = desc[4 * p + 1], t0 = desc[4 * p + 2], nt = desc[4 * p + 3];
  if (blockIdx.x * kIcpThreads >= ns) return;  // block-uniform
  const int i = blockIdx.x * kIcpThreads + threadIdx.x;
  const size_t P = gridDim.y;
  // moments about a fixed per-pair anchor a = the pair's first target point (one pass; Sigma is recentred in k_icp_solve)
  const double ax = tgt[3 * (size_t)t0], ay = tgt[3 * (size_t)t0 + 1], az = tgt[3 * (size_t)t0 + 2];
  double m[kIcpMoments];
#pragma unroll
  for (int k = 0; k < kIcpMoments; ++k) m[k] = 0.0;
  if (i < ns) {
    const size_t o = (size_t)p * max_ns + i;
    double best_d2 = w.part_d2[o];
    int best = w.part_idx[o];
    const int nslice_p = (nt + slice - 1) / slice;
    for (int s = 1; s < nslice_p; ++s) {  // slices hold increasing target indices: strict < keeps the first minimum
      const double d = w.part_d2[(size_t)s * P * max_ns + o];
      if (d < best_d2) { best_d2 = d; best = w.part_idx[(size_t)s * P * max_ns + o]; }
    }
    double u[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) u[k] = w.state[(size_t)p * kIcpState + k];
    double* c = w.cur + 3 * o;
    double s[3];
    apply_rt(u, c[0], c[1], c[2], s);  // bit-identical to the point k_icp_partial searched with
    c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    if (best_d2 < tau2) {
      const double* q = tgt + 3 * ((size_t)t0 + best);
      const double px = s[0] - ax, py = s[1] - ay, pz = s[2] - az;
      const double qx = q[0] - ax, qy = q[1] - ay, qz = q[2] - az;
      m[0] = 1.0; m[1] = best_d2;
      m[2] = px; m[3] = py; m[4] = pz;
      m[5] = qx; m[6] = qy; m[7] = qz;
      m[8] = qx * px; m[9] = qx * py; m[10] = qx * pz;
      m[11] = qy * px; m[12] = qy * py; m[13] = qy * pz;
      m[14] = qz * px; m[15] = qz * py; m[16] = qz * pz;
    }
  }
  // fixed-order reduction: butterfly inside each wave, then the four wave sums in wave order
#pragma unroll
  for (int k = 0; k < kIcpMoments; ++k) {
    double v = m[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    m[k] = v;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kIcpMoments; ++k) red[wave][k] = m[k];
  }
  __syncthreads();
  if (threadIdx.x < kIcpMoments) {
    const int k = threadIdx.x;
    w.mom[((size_t)p * src_blocks + blockIdx.x) * kIcpMoments + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// One Jacobi rotation of the symmetric 4x4 a, zeroing a[r][c]; v accumulates the eigenvectors (columns).
__device__ inline void jacobi_rotate(double (&a)[4][4], double (&v)[4][4], int r, int c) {
  const double apq = a[r][c];
  if (apq == 0.0) return;
  const double theta = (a[c][c] - a[r][r]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // columns r, c of a * J
    const double akr = a[k][r], akc = a[k][c];
    a[k][r] = cs * akr - sn * akc;
    a[k][c] = sn * akr + cs * akc;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // rows r, c of J^T * (a * J)
    const double ark = a[r][k], ack = a[c][k];
    a[r][k] = cs * ark - sn * ack;
    a[c][k] = sn * ark + cs * ack;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkr = v[k][r], vkc = v[k][c];
    v[k][r] = cs * vkr - sn * vkc;
    v[k][c] = sn * vkr + cs * vkc;
  }
}

// Rotation R maximising tr(R^T S) for S = sum (q - mu_q)(p - mu_p)^T: the unit quaternion of the largest eigenvalue of
// Horn's symmetric 4x4 matrix.  This is Umeyama's U diag(1, 1, det(U)det(V)) V^T whenever the singular values of S are
// distinct; for any S (S = 0 included: n = 1) the quaternion is a unit vector, so R is finite with det +1.
__device__ void horn_rotation(const double (&S)[3][3], double (&R)[3][3]) {
  // Horn's M = sum p q^T = S^T: M_ab = S[b][a]
  const double xx = S[0][0], xy = S[1][0], xz = S[2][0];
  const double yx = S[0][1], yy = S[1][1], yz = S[2][1];
  const double zx = S[0][2], zy = S[1][2], zz = S[2][2];
  double a[4][4] = {{xx + yy + zz, yz - zy, zx - xz, xy - yx},
                    {yz - zy, xx - yy - zz, xy + yx, zx + xz},
                    {zx - xz, xy + yx, -xx + yy - zz, yz + zy},
                    {xy - yx, zx + xz, yz + zy, -xx - yy + zz}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  double scale = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) scale = fmax(scale, fabs(a[r][c]));
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = (fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3])) + (fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]));
    if (!(off > 1e-300 + 1e-18 * scale)) break;
    jacobi_rotate(a, v, 0, 1); jacobi_rotate(a, v, 0, 2); jacobi_rotate(a, v, 0, 3);
    jacobi_rotate(a, v, 1, 2); jacobi_rotate(a, v, 1, 3); jacobi_rotate(a, v, 2, 3);
  }
  int best = 0;
  double bl = a[0][0];
  if (a[1][1] > bl) { bl = a[1][1]; best = 1; }
  if (a[2][2] > bl) { bl = a[2][2]; best = 2; }
  if (a[3][3] > bl) { bl = a[3][3]; best = 3; }
  double q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = best == 0 ? v[k][0] : best == 1 ? v[k][1] : best == 2 ? v[k][2] : v[k][3];
  double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(nrm > 0.0) || !isfinite(nrm)) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; nrm = 1.0; }
  const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
  R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2 * (x * y - w * z); R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z); R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y); R[2][1] = 2 * (y * z + w * x); R[2][2] = w * w - x * x - y * y + z * z;
}

__global__ __launch_bounds__(64) void k_icp_solve(const double* __restrict__ tgt, const int32_t* __restrict__ desc, int pairs,
                                                  int src_blocks, int round, int max_iter, double rel_fitness,
                                                  double rel_rmse, IcpWork w, double* __restrict__ transform,
                                                  double* __restrict__ fitness, double* __restrict__ inlier_rmse,
                                                  int32_t* __restrict__ iterations) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= pairs || w.done[p]) return;
  const int ns = desc[4 * p + 1], t0 = desc[4 * p + 2];
  const int nb = (ns + kIcpThreads - 1) / kIcpThreads;
  double m[kIcpMoments];
#pragma unroll
  for (int k = 0; k < kIcpMoments; ++k) m[k] = 0.0;
  for (int b = 0; b < nb; ++b) {  // block order: the sum is the same every run
    const double* mb = w.mom + ((size_t)p * src_blocks + b) * kIcpMoments;
#pragma unroll
    for (int k = 0; k < kIcpMoments; ++k) m[k] += mb[k];
  }
  const double n = m[0];
  const double fit = n > 0.0 ? n / (double)ns : 0.0;
  const double rmse = n > 0.0 ? sqrt(m[1] / n) : 0.0;
  double* st = w.state + (size_t)p * kIcpState;
  fitness[p] = fit;
  inlier_rmse[p] = rmse;
  iterations[p] = round;
#pragma unroll
  for (int k = 0; k < 16; ++k) transform[16 * (size_t)p + k] = st[12 + k];
  if ((round > 0 && fabs(st[28] - fit) < rel_fitness && fabs(st[29] - rmse) < rel_rmse) || round >= max_iter) {
    w.done[p] = 1;
    return;
  }
  st[28] = fit;
  st[29] = rmse;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  double t[3] = {0.0, 0.0, 0.0};
  if (n > 0.0) {  // no inlier: the identity update, as open3d's estimation returns for an empty correspondence set
    const double ax = tgt[3 * (size_t)t0], ay = tgt[3 * (size_t)t0 + 1], az = tgt[3 * (size_t)t0 + 2];
    const double mp[3] = {m[2] / n, m[3] / n, m[4] / n}, mq[3] = {m[5] / n, m[6] / n, m[7] / n};
    double S[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[r][c] = m[8 + 3 * r + c] / n - mq[r] * mp[c];
    horn_rotation(S, R);
    const double P0 = ax + mp[0], P1 = ay + mp[1], P2 = az + mp[2];
    t[0] = (ax + mq[0]) - (R[0][0] * P0 + R[0][1] * P1 + R[0][2] * P2);
    t[1] = (ay + mq[1]) - (R[1][0] * P0 + R[1][1] * P1 + R[1][2] * P2);
    t[2] = (az + mq[2]) - (R[2][0] * P0 + R[2][1] * P1 + R[2][2] * P2);
  }
  // T = update * T (update = [R t; 0 1]); U = update is applied to the working cloud in the next round
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = st[12 + k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      st[12 + 4 * r + c] = R[r][0] * T[c] + R[r][1] * T[4 + c] + R[r][2] * T[8 + c] + t[r] * T[12 + c];
#pragma unroll
  for (int c = 0; c < 4; ++c) st[24 + c] = T[12 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) st[3 * r + c] = R[r][c];
    st[9 + r] = t[r];
  }
}

}  // namespace

extern "C" {

size_t dpc_icp_workspace_bytes(int pairs, const int32_t* src_count, const int32_t* tgt_count) {
  if (pairs <= 0 || !src_count || !tgt_count) return 0;
  for (int p = 0; p < pairs; ++p)
    if (src_count[p] < 0 || tgt_count[p] < 0) return 0;
  return icp_carve(icp_geometry(pairs, src_count, tgt_count, 1), pairs, nullptr, nullptr);
}

int dpc_icp_point_to_point(const double* src, int n_src, const double* tgt, int n_tgt, const int32_t* pair_desc,
                           const int32_t* host_pair_desc, int pairs, const double* init, double max_dist, int max_iter,
                           double rel_fitness, double rel_rmse, double* transform, double* fitness, double* inlier_rmse,
                           int32_t* iterations, void* workspace, void* stream) {
  if (pairs < 0 || n_src < 0 || n_tgt < 0 || max_iter < 0 || !(max_dist > 0.0) || !std::isfinite(max_dist))
    return DPC_ERR_SHAPE;
  if (pairs == 0) return DPC_OK;
  if (!host_pair_desc) return DPC_ERR_NULL;
  const int rc = check_desc<4>(host_pair_desc, pairs, {(int64_t)n_src, (int64_t)n_tgt}, INT64_MAX, nullptr,
                               [](const int32_t* d) { return !(d[3] == 0 && d[1] > 0); });  // argmin over an empty set
  if (rc != DPC_OK) return rc;
  const IcpGeom g = icp_geometry(pairs, host_pair_desc + 1, host_pair_desc + 3, 4);
  if (!pair_desc || !init || !transform || !fitness || !inlier_rmse || !iterations || !workspace) return DPC_ERR_NULL;
  if ((g.max_ns > 0 && !src) || (g.max_nt > 0 && !tgt)) return DPC_ERR_NULL;
  IcpWork w;
  icp_carve(g, pairs, static_cast<char*>(workspace), &w);
  hipStream_t st = (hipStream_t)stream;
  const double tau2 = max_dist * max_dist;  // formed in fp64
  const int sb = g.src_blocks;
  DPC_LAUNCH("k_icp_init", dpc_kid("k_icp_init"), k_icp_init, dim3(sb, pairs), dim3(kIcpThreads), 0, st, src, pair_desc, init,
             g.max_ns, w);
  for (int round = 0; round <= max_iter; ++round) {
    DPC_LAUNCH("k_icp_partial", dpc_kid("k_icp_partial"), k_icp_partial, dim3(sb, pairs, g.nslice), dim3(kIcpThreads), 0, st,
               tgt, pair_desc, g.max_ns, g.slice, w);
    DPC_LAUNCH("k_icp_merge", dpc_kid("k_icp_merge"), k_icp_merge, dim3(sb, pairs), dim3(kIcpThreads), 0, st, tgt, pair_desc,
               g.max_ns, g.slice, sb, tau2, w);
    DPC_LAUNCH("k_icp_solve", dpc_kid("k_icp_solve"), k_icp_solve, dim3((pairs + 63) / 64), dim3(64), 0, st, tgt, pair_desc,
               pairs, sb, round, max_iter, rel_fitness, rel_rmse, w, transform, fitness, inlier_rmse, iterations);
  }
  return launch_ok();
}

}  // extern "C"
