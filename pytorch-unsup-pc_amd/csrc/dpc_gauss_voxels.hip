// The exact Gaussian occupancy renderer: pointcloud2voxels of the TF-1 original (dpc/util/point_cloud.py:17-57), the
// branch the model takes when cfg.pc_fast is false.  Every point is an isotropic Gaussian evaluated at every voxel centre:
//
//   c_i          = -1 + 2 i / (G-1)                                   tf.linspace(-1, 1, G)
//   e_a[n,i]     = exp(-(tr[n,a] - c_i)^2 / (2 sigma^2)),  a = 0,1,2   (pc_normalise_gauss: divided by S_a[n] = sum_i e_a[n,i])
//   raw[b,z,y,x] = k * sum_n e_0[n,z] e_1[n,y] e_2[n,x]
//   vox          = clip(raw, 0, 1)
//
// The Gaussian is separable, so the grid of a cloud is a rank-N contraction of three [N,G] tables and both directions are
// fp32 matrix products on v_mfma_f32_32x32x2_f32 (the vector FMA rate with one operand register per lane; the result is
// bit for bit a k-ordered fmaf chain).  Nothing larger than the grid is stored.
//
//   forward   D[y,x] += A[y,n] B[n,x] per z plane, A[y,n] = e_0[n,z] e_1[n,y] (one multiply per operand), B[n,x] = e_2[n,x].
//             A workgroup owns a 32 x 32 (y,x) tile of 4*ZPW planes, a wave ZPW of them (16 accumulator registers per plane);
//             every voxel is owned by one lane.  Points are taken in index order in chunks of kChunk, whose three 1-D tables
//             are built in LDS by the whole workgroup: 3 ds_read_b32 + ZPW broadcast reads per 2 points and ZPW MFMAs.
//   backward  with g = dvox * [0 <= raw <= 1] * k, one product over x gives, per point n and grid row m = (z,y),
//             D1[m,n] = sum_x g[m,x] P_2[n,x] and D2[m,n] = sum_x g[m,x] dP_2[n,x]; then
//             dtr[n,0] = sum_m dP_0 P_1 D1, dtr[n,1] = sum_m P_0 dP_1 D1, dtr[n,2] = sum_m P_0 P_1 D2,
//             with dP_a[n,i] = P_a[n,i] (w_i - wbar), w_i = -(tr[n,a] - c_i) / sigma^2 and wbar = sum_i P_a w_i under
//             pc_normalise_gauss (the quotient rule), 0 otherwise.  A wave owns 32 points (the MFMA's columns) and keeps
//             their tables in LDS for the whole launch; the workgroup walks the G^2/32 row tiles of g in order, double
//             buffered in LDS, and every lane adds its 16 rows of every tile to three running sums: one launch, one owner
//             per point, a fixed order, no atomics.  The product over x runs at a compiled width of 32 or 64 (KS = 16 or
//             32 MFMA steps, straight-line code), columns past G zero.
//
// Equal inputs give equal bits on every run, in both directions.
#include <math.h>

#include <algorithm>

#include "dpc_common.h"
#include "dpc_launch.h"

namespace dpcg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DPC_WAVE;
constexpr int kChunk = 128;                 // points per forward chunk
constexpr int kMaxSide = DPC_GAUSS_MAX_SIDE;
constexpr double kMagic = 1.78984352254;    // point_cloud.py:48 (estimate_gauss_normaliser)

// tf.linspace(-1, 1, G)[i], in fp64
__device__ inline double centre(int i, int G) { return G > 1 ? -1.0 + 2.0 * (double)i / (double)(G - 1) : -1.0; }

// exp(-(t - c)^2 / (2 sigma^2) - shift); c2 = -1 / (2 sigma^2).  The argument is formed in fp64 and rounded once.
// shift is 0 except under pc_normalise_gauss, where it is the point's largest argument over the grid: e / sum e does not
// change when every argument moves by the same amount, and a point whose Gaussians all underflow in fp32 (one well outside
// the grid under a narrow sigma) keeps its normalised table, as in fp64, instead of 0 / 0.
__device__ inline double gauss_arg(float t, double c, double c2) {
  const double d = (double)t - c;
  return d * d * c2;
}
__device__ inline float gauss(float t, double c, double c2, double shift = 0.0) { return expf((float)(gauss_arg(t, c, c2) - shift)); }

// row of accumulator register r in lane half h of a 32 x 32 MFMA result (the column is lane & 31)
__device__ inline constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
template <int ZPW>
__global__ __launch_bounds__(kThreads) void k_gauss_voxels_fwd(const float* __restrict__ tr, int N, int G, double c2, float k,
                                                               int per_point, float* __restrict__ raw,
                                                               float* __restrict__ vox) {
  constexpr int ZT = kWaves * ZPW, ROW = ZT + 64;   // a point's row of the chunk table: ZT z entries, 32 y, 32 x
  __shared__ float tab[kChunk * ROW];
  __shared__ float inv[kChunk * 3];                 // pc_normalise_gauss: 1 / S_a[n] of the shifted arguments
  __shared__ double shift[kChunk * 3];              //                     and their shift
  __shared__ double cen[ROW];                       // the centres of the row's entries
  __shared__ double cen_all[kMaxSide];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
  const int xt = (G + 31) / 32;
  const int x0 = ((int)blockIdx.x % xt) * 32, y0 = ((int)blockIdx.x / xt) * 32, z0 = (int)blockIdx.y * ZT, b = blockIdx.z;
  const float* pts = tr + (size_t)b * N * 3;
  auto entry_index = [&](int r) { return r < ZT ? z0 + r : (r < ZT + 32 ? y0 + r - ZT : x0 + r - ZT - 32); };
  if (tid < ROW) cen[tid] = centre(entry_index(tid), G);
  if (per_point && tid < G) cen_all[tid] = centre(tid, G);

  f32x16 acc[ZPW];
#pragma unroll
  for (int q = 0; q < ZPW; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  for (int n0 = 0; n0 < N; n0 += kChunk) {
    const int cn = min(kChunk, N - n0);
    __syncthreads();   // the previous chunk has been consumed (first pass: the centres are written)
    if (per_point) {
      for (int e = tid; e < cn * 3; e += kThreads) {
        const float t = pts[(size_t)n0 * 3 + e];
        double top = gauss_arg(t, cen_all[0], c2), s = 0.0;
        for (int i = 1; i < G; ++i) top = fmax(top, gauss_arg(t, cen_all[i], c2));
        for (int i = 0; i < G; ++i) s += (double)gauss(t, cen_all[i], c2, top);
        inv[e] = (float)(1.0 / s);
        shift[e] = top;
      }
      __syncthreads();
    }
    for (int e = tid; e < kChunk * ROW; e += kThreads) {
      const int n = e / ROW, r = e - n * ROW;
      const int a = r < ZT ? 0 : (r < ZT + 32 ? 1 : 2);
      float v = 0.f;   // dead rows and columns of a partly dead tile, and the tail of the last chunk, add nothing
      if (n < cn && entry_index(r) < G) {
        const float t = pts[(size_t)(n0 + n) * 3 + a];
        v = per_point ? gauss(t, cen[r], c2, shift[n * 3 + a]) * inv[n * 3 + a] : gauss(t, cen[r], c2);
      }
      tab[e] = v;
    }
    __syncthreads();
    const int steps = (cn + 1) / 2;   // two points per MFMA, lane half h takes point 2s + h: index order along the chain
    // kBatch steps' operands are read before their MFMAs are issued, so that the LDS latency is paid once per batch
    constexpr int kBatch = ZPW == 1 ? 4 : 2;
    int s = 0;
    for (; s + kBatch <= steps; s += kBatch) {
      float ay[kBatch], bx[kBatch], az[kBatch][ZPW];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float* row = tab + (2 * (s + u) + h) * ROW;
        ay[u] = row[ZT + j];
        bx[u] = row[ZT + 32 + j];
#pragma unroll
        for (int q = 0; q < ZPW; ++q) az[u][q] = row[wave * ZPW + q];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
#pragma unroll
        for (int q = 0; q < ZPW; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(az[u][q] * ay[u], bx[u], acc[q], 0, 0, 0);
    }
    for (; s < steps; ++s) {
      const float* row = tab + (2 * s + h) * ROW;
      const float ay = row[ZT + j], bx = row[ZT + 32 + j];
#pragma unroll
      for (int q = 0; q < ZPW; ++q)
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[wave * ZPW + q] * ay, bx, acc[q], 0, 0, 0);
    }
  }

  const int x = x0 + j;
#pragma unroll
  for (int q = 0; q < ZPW; ++q) {
    const int z = z0 + wave * ZPW + q;
    if (z >= G || x >= G) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int y = y0 + acc_row(r) + 4 * h;
      if (y >= G) continue;
      const size_t o = (((size_t)b * G + z) * G + y) * G + x;
      const float v = k * acc[q][r];
      if (raw != nullptr) raw[o] = v;
      vox[o] = fminf(fmaxf(v, 0.f), 1.f);
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------
// LDS, in floats: cen[GEc] | tile[2][32][GEc + 1] | per wave z, y, x tables [GEc][32] each; GEc = 2 KS is the compiled width:
// the smallest of 32 and 64 that holds G, rows and columns past G zero
constexpr size_t bwd_lds_bytes(int KS) {
  return ((size_t)2 * KS + 2 * 32 * (2 * KS + 1) + (size_t)kWaves * 3 * 2 * KS * 32) * sizeof(float);
}

template <int KS>   // MFMA steps per tile row: the products over x are straight-line code, so that the next tile's loads, issued
                    // in front of them, are waited for only where they are consumed
__global__ __launch_bounds__(kThreads) void k_gauss_voxels_bwd(const float* __restrict__ tr, int N, int G, double c2, float is2,
                                                               float k, int per_point, const float* __restrict__ raw,
                                                               const float* __restrict__ dvox, float* __restrict__ dtr) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int GEc = 2 * KS, GS = GEc + 1;   // an odd row stride: the 32 rows a half-wave reads lie on 32 banks
  constexpr int PER = 32 * GEc / kThreads;    // tile elements per thread
  float* cen = lds;
  float* tile = cen + GEc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
  float* tz = tile + 2 * 32 * GS + (size_t)wave * 3 * GEc * 32;
  float* ty = tz + GEc * 32;
  float* tx = ty + GEc * 32;
  const int b = blockIdx.y;
  const int n = ((int)blockIdx.x * kWaves + wave) * 32 + j;   // this lane's point: the column of every product
  const bool live = n < N;
  const size_t plane = (size_t)G * G;
  const float* rawb = raw + (size_t)b * plane * G;
  const float* dvb = dvox + (size_t)b * plane * G;

  for (int i = tid; i < GEc; i += kThreads) cen[i] = i < G ? (float)centre(i, G) : 0.f;

  // A tile's loads are issued unconditionally (dead elements read element 0) and consumed only by store_tile, so that they
  // stay in flight under the products in between.  Thread tid moves elements tid + u * kThreads = (row, x) of every tile.
  float rv[PER], dv[PER];
  auto tile_offset = [&](int mt, int u, bool& ok) {
    const int e = tid + u * kThreads, row = e / GEc, x = e % GEc;
    const size_t m = (size_t)mt * 32 + row;
    ok = x < G && m < plane;
    return ok ? m * G + x : (size_t)0;
  };
  auto load_tile = [&](int mt) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      bool ok;
      const size_t o = tile_offset(mt, u, ok);
      rv[u] = rawb[o];
      dv[u] = dvb[o];
    }
  };
  auto store_tile = [&](int mt) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      bool ok;
      (void)tile_offset(mt, u, ok);
      const int e = tid + u * kThreads;
      // the inclusive pass-through set of clamp
      tile[((mt & 1) * 32 + e / GEc) * GS + e % GEc] = (ok && rv[u] >= 0.f && rv[u] <= 1.f) ? dv[u] * k : 0.f;
    }
  };
  const int tiles = (int)((plane + 31) / 32);
  load_tile(0);

  // this wave's tables, and per lane its point's coordinates and (pc_normalise_gauss) the e-weighted means of w
  float t[3] = {0.f, 0.f, 0.f}, wbar[3] = {0.f, 0.f, 0.f}, invs[3] = {1.f, 1.f, 1.f};
  double shift[3] = {0.0, 0.0, 0.0};
  if (live)
    for (int a = 0; a < 3; ++a) t[a] = tr[((size_t)b * N + n) * 3 + a];
  if (per_point && live) {
    for (int a = 0; a < 3; ++a) {
      double s = 0.0, mw = 0.0, top = gauss_arg(t[a], centre(0, G), c2);
      for (int i = 1; i < G; ++i) top = fmax(top, gauss_arg(t[a], centre(i, G), c2));
      shift[a] = top;
      for (int i = 0; i < G; ++i) {
        const double c = centre(i, G);
        const float e = gauss(t[a], c, c2, top);
        s += (double)e;
        mw += (double)e * (double)(((float)c - t[a]) * is2);
      }
      invs[a] = (float)(1.0 / s);
      wbar[a] = (float)(mw / s);
    }
  }
  for (int a = 0; a < 3; ++a) {
    float* tab = a == 0 ? tz : (a == 1 ? ty : tx);
    for (int i = h; i < GEc; i += 2) tab[i * 32 + j] = (live && i < G) ? gauss(t[a], centre(i, G), c2, shift[a]) * invs[a] : 0.f;
  }
  store_tile(0);
  __syncthreads();

  float gz = 0.f, gy = 0.f, gx = 0.f;
  int zb = 0, yb = 4 * h;   // (z, y) of this lane's first row of the current tile
  while (yb >= G) { yb -= G; ++zb; }
  for (int mt = 0; mt < tiles; ++mt) {
    const bool more = mt + 1 < tiles;
    if (more) load_tile(mt + 1);   // in flight under the products
    const float* T = tile + (mt & 1) * 32 * GS + j * GS + h;
    const float* X = tx + h * 32 + j;
    f32x16 d1, d2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { d1[r] = 0.f; d2[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < KS; ++s) {   // x = 2 s + h
      const float a = T[2 * s], p = X[2 * s * 32];
      const float w = fmaf(cen[2 * s + h] - t[2], is2, -wbar[2]);
      d1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p, d1, 0, 0, 0);
      d2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p * w, d2, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int y = yb + acc_row(r), z = zb;
      while (y >= G) { y -= G; ++z; }
      if (z < G) {   // rows past the grid's end are zero rows of g
        const float pz = tz[z * 32 + j], py = ty[y * 32 + j];
        const float wz = fmaf(cen[z] - t[0], is2, -wbar[0]), wy = fmaf(cen[y] - t[1], is2, -wbar[1]);
        const float pp = pz * py, pd = pp * d1[r];
        gz = fmaf(pd, wz, gz);
        gy = fmaf(pd, wy, gy);
        gx = fmaf(pp, d2[r], gx);
      }
    }
    yb += 32;
    while (yb >= G) { yb -= G; ++zb; }
    if (more) store_tile(mt + 1);
    __syncthreads();
  }
  // the two halves hold the sums over their rows: lower half + upper half, then one store per point
  gz += __shfl_down(gz, 32, DPC_WAVE);
  gy += __shfl_down(gy, 32, DPC_WAVE);
  gx += __shfl_down(gx, 32, DPC_WAVE);
  if (h == 0 && live) {
    float* o = dtr + ((size_t)b * N + n) * 3;
    o[0] = gz; o[1] = gy; o[2] = gx;
  }
}

int validate(const DpcParams* p, double sigma, int normalise) {
  if (p == nullptr) return DPC_ERR_NULL;
  if (p->B < 0 || p->N < 0 || p->D < 1 || p->B > 65535 || p->N > DPC_MAX_POINTS) return DPC_ERR_SHAPE;
  if (p->D != p->H || p->H != p->W) return DPC_ERR_SHAPE;   // pointcloud2voxels reads vox_size only
  if (p->point_replicas > 1 || p->point_replicas < 0 || p->point_index != nullptr) return DPC_ERR_SHAPE;
  if (!(sigma > 0.0) || !std::isfinite(sigma)) return DPC_ERR_SHAPE;
  if (normalise != DPC_GAUSS_NORM_NONE && normalise != DPC_GAUSS_NORM_ANALYTICAL && normalise != DPC_GAUSS_NORM_PER_POINT)
    return DPC_ERR_SHAPE;
  if (p->D > kMaxSide) return DPC_ERR_LDS;
  return DPC_OK;
}

float scale_of(int G, double sigma, int normalise) {
  if (normalise != DPC_GAUSS_NORM_ANALYTICAL) return 1.f;
  const double sn = sigma * (double)G;
  return (float)(1.0 / (kMagic * sn * sn * sn));
}

}  // namespace dpcg

extern "C" {

int dpc_gauss_voxels_fwd(const DpcParams* p, const float* tr, double sigma, int normalise, float* raw, float* vox, void* stream) {
  using namespace dpcg;
  int rc = validate(p, sigma, normalise);
  if (rc != DPC_OK) return rc;
  if (p->B == 0) return DPC_OK;
  if (!vox || (!tr && p->N > 0)) return DPC_ERR_NULL;
  const int G = p->D, tiles = (G + 31) / 32;
  const double c2 = -1.0 / (2.0 * sigma * sigma);
  const float k = scale_of(G, sigma, normalise);
  const int per_point = normalise == DPC_GAUSS_NORM_PER_POINT;
  hipStream_t st = (hipStream_t)stream;
  // wide grids: four planes per wave, every table entry feeds four MFMAs; narrow ones: one plane, four times the workgroups
  if (G > 32)
    DPC_LAUNCH("k_gauss_voxels_fwd", dpc_kid("k_gauss_voxels_fwd", 4), k_gauss_voxels_fwd<4>, dim3(tiles * tiles, (G + 15) / 16, p->B),
               dim3(kThreads), 0, st, tr, p->N, G, c2, k, per_point, raw, vox);
  else
    DPC_LAUNCH("k_gauss_voxels_fwd", dpc_kid("k_gauss_voxels_fwd", 1), k_gauss_voxels_fwd<1>, dim3(tiles * tiles, (G + 3) / 4, p->B),
               dim3(kThreads), 0, st, tr, p->N, G, c2, k, per_point, raw, vox);
  return launch_ok();
}

int dpc_gauss_voxels_bwd(const DpcParams* p, const float* tr, double sigma, int normalise, const float* raw, const float* dvox,
                         float* dtr, void* stream) {
  using namespace dpcg;
  int rc = validate(p, sigma, normalise);
  if (rc != DPC_OK) return rc;
  if (p->B == 0 || p->N == 0) return DPC_OK;
  if (!tr || !raw || !dvox || !dtr) return DPC_ERR_NULL;
  const int G = p->D;
  const double c2 = -1.0 / (2.0 * sigma * sigma);
  const float is2 = (float)(1.0 / (sigma * sigma));
  const float k = scale_of(G, sigma, normalise);
  const int per_point = normalise == DPC_GAUSS_NORM_PER_POINT;
  const dim3 grid((p->N + 32 * kWaves - 1) / (32 * kWaves), p->B);
  hipStream_t st = (hipStream_t)stream;
  if (G <= 32)
    DPC_LAUNCH("k_gauss_voxels_bwd", dpc_kid("k_gauss_voxels_bwd", 16), k_gauss_voxels_bwd<16>, grid, dim3(kThreads), bwd_lds_bytes(16),
               st, tr, p->N, G, c2, is2, k, per_point, raw, dvox, dtr);
  else
    DPC_LAUNCH("k_gauss_voxels_bwd", dpc_kid("k_gauss_voxels_bwd", 32), k_gauss_voxels_bwd<32>, grid, dim3(kThreads), bwd_lds_bytes(32),
               st, tr, p->N, G, c2, is2, k, per_point, raw, dvox, dtr);
  return launch_ok();
}

}  // extern "C"
