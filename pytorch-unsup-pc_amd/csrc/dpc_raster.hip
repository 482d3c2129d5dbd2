// Batched rendering of point clouds to shaded images: the reference's render_point_cloud_blender.py (one Blender process
// per model, every point a small sphere) for many ragged clouds in one call, ray-traced in fp64.  Semantics in
// include/dpc_render.h (dpc_render_points); cost model and measurements in DESIGN.md.
//
// One workgroup per (image, 16 x 16-pixel tile), image-major so the blocks of one image share its points in L2:
//   1. the tile's sample keys (16 * 16 * ss^2 uint64, at most 32 KiB) live in LDS, all "background";
//   2. the cloud streams through in chunks of 256 points: each thread checks its point's values and bounds the samples
//      its sphere can cover (rs_box, conservative: correctness comes from the per-sample ray test); the boxes clipped to
//      the tile are prefixed (block_scan), and the threads walk the chunk's (box sample, point) pairs, each hit an LDS
//      64-bit atomicMin of (bits(float(t)) << 32 | point index): the minimum is order-independent;
//   3. one thread per pixel shades its ss^2 samples (the winner's fp64 hit recomputed) and writes the pixel and the ids.
// Built with -ffp-contract=off: every product and sum is rounded on its own, as numpy rounds it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kRsTile = 16;                       // pixels per tile side
constexpr int kRsThreads = kRsTile * kRsTile;     // one thread per tile pixel when shading
constexpr int kRsChunk = kRsThreads;              // points per pass over the tile
constexpr int kRsMaxSS = 4;
constexpr int kRsKeys = kRsThreads * kRsMaxSS * kRsMaxSS;  // 4096 keys, 32 KiB
constexpr uint64_t kRsEmpty = ~0ull;              // background

struct RsFrame {
  double C[3], r[3], u[3], f[3];  // camera position, right, up, forward (the frames row: C, r, u, f)
};

// A point of the current chunk whose box meets the tile: m = C - P, c = m.m - rad^2, its index in the cloud and its box
// clipped to the tile (columns x0 .. x0 + w - 1, rows from y0).
struct RsPoint {
  double m[3];
  double c;
  int k, x0, y0, w;
};

__device__ inline double rs_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The direction of sample (sx, sy) = (j ss + b, i ss + a): D = (f + (x_s / F) r) + (y_s / F) u.
__device__ inline void rs_dir(const RsFrame& fr, int sx, int sy, int ss, double half, double F, double* D) {
  const int j = sx / ss, b = sx - j * ss, i = sy / ss, a = sy - i * ss;
  const double xs = ((double)j + ((double)b + 0.5) / (double)ss) - half;
  const double ys = half - ((double)i + ((double)a + 0.5) / (double)ss);
  const double px = xs / F, py = ys / F;
  for (int k = 0; k < 3; ++k) D[k] = (fr.f[k] + px * fr.r[k]) + py * fr.u[k];
}

// The ray C + t D against the sphere with m = C - P and c = m.m - rad^2: hit when c > 0, disc >= 0 and t > 0.
__device__ inline bool rs_hit(const double* m, double c, const double* D, double* t) {
  const double a = rs_dot(D, D), b = rs_dot(m, D);
  const double disc = b * b - a * c;
  if (!(c > 0.0) || !(disc >= 0.0)) return false;
  *t = (-b - sqrt(disc)) / a;
  return *t > 0.0;
}

__device__ inline int rs_clamp(double x, int lo, int hi) { return x < (double)lo ? lo : (x > (double)hi ? hi : (int)x); }

// Samples [box[0], box[1]] x [box[2], box[3]] (columns, rows; inclusive) outside of which no ray of the image can hit the
// sphere (P, rad); empty (box[0] > box[1]) when no ray can.  In camera coordinates (xc, yc, zc) = (q.r, q.u, q.f) with
// q = P - C, a hit point H has x_s = F ((H - C).r) / ((H - C).f): interval bounds of that quotient over the sphere, the
// radius widened for the rounding of the frame and of the ray test, and one sample more on every side.  A sphere that
// reaches the camera plane gets the whole image, one wholly behind it nothing.
__device__ inline void rs_box(const RsFrame& fr, const double* P, double rad, int n, int ss, double half, double F,
                              int* box) {
  const double q[3] = {P[0] - fr.C[0], P[1] - fr.C[1], P[2] - fr.C[2]};
  const double zc = rs_dot(q, fr.f), xc = rs_dot(q, fr.r), yc = rs_dot(q, fr.u);
  const double R = rad * (1.0 + 1e-6) + 1e-9 * (fabs(zc) + fabs(xc) + fabs(yc));
  if (zc + R < 0.0) {
    box[0] = 1; box[1] = 0; box[2] = 1; box[3] = 0;
    return;
  }
  if (!(zc - R > 1e-6 * (fabs(zc) + R))) {
    box[0] = 0; box[1] = n - 1; box[2] = 0; box[3] = n - 1;
    return;
  }
  const double d1 = zc - R, d2 = zc + R;  // 0 < d1 < d2
  const double xa = xc - R, xb = xc + R, ya = yc - R, yb = yc + R;
  const double xlo = F * (xa / (xa >= 0.0 ? d2 : d1)), xhi = F * (xb / (xb >= 0.0 ? d1 : d2));
  const double ylo = F * (ya / (ya >= 0.0 ? d2 : d1)), yhi = F * (yb / (yb >= 0.0 ? d1 : d2));
  const double s = (double)ss;
  // column sx holds x_s = (sx + 0.5) / ss - S/2, row sy holds y_s = S/2 - (sy + 0.5) / ss
  box[0] = rs_clamp(floor((xlo + half) * s - 0.5) - 1.0, -1, n);
  box[1] = rs_clamp(ceil((xhi + half) * s - 0.5) + 1.0, -1, n);
  box[2] = rs_clamp(floor((half - yhi) * s - 0.5) - 1.0, -1, n);
  box[3] = rs_clamp(ceil((half - ylo) * s - 0.5) + 1.0, -1, n);
}

__global__ __launch_bounds__(kRsThreads) void k_rs_tile(const double* __restrict__ points, const float* __restrict__ colors,
                                                        const double* __restrict__ radii, const int32_t* __restrict__ table,
                                                        const double* __restrict__ frames, int tiles_x, int S, int ss,
                                                        double F, double rad0, float* __restrict__ image,
                                                        int32_t* __restrict__ ids, int32_t* __restrict__ status) {
  __shared__ uint64_t key[kRsKeys];
  __shared__ RsPoint pt[kRsChunk];
  __shared__ int pre[kRsChunk];
  __shared__ int scratch[kRsThreads / 64 + 1];
  __shared__ int bad;
  const int t = threadIdx.x;
  const int tiles = tiles_x * tiles_x;
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int start = table[2 * img], count = table[2 * img + 1];
  RsFrame fr;
  {
    const double* g = frames + 12 * (int64_t)img;
    for (int k = 0; k < 3; ++k) {
      fr.C[k] = g[k];
      fr.r[k] = g[3 + k];
      fr.u[k] = g[6 + k];
      fr.f[k] = g[9 + k];
    }
  }
  const int n = S * ss, ts = kRsTile * ss;  // samples per image side, per tile side
  const int sx0 = tx * ts, sy0 = ty * ts;
  const int sx1 = min(n, sx0 + ts) - 1, sy1 = min(n, sy0 + ts) - 1;  // inclusive
  const double half = (double)S * 0.5;
  for (int i = t; i < ts * ts; i += kRsThreads) key[i] = kRsEmpty;
  if (t == 0) bad = 0;
  __syncthreads();
  for (int c0 = 0; c0 < count; c0 += kRsChunk) {
    const int k = c0 + t;
    int area = 0;
    RsPoint p;
    if (k < count) {
      const int64_t g = (int64_t)start + k;
      const double P[3] = {points[3 * g], points[3 * g + 1], points[3 * g + 2]};
      const double rad = radii ? radii[g] : rad0;
      bool ok = isfinite(P[0]) && isfinite(P[1]) && isfinite(P[2]) && isfinite(rad) && rad > 0.0;
      if (colors) ok = ok && isfinite(colors[3 * g]) && isfinite(colors[3 * g + 1]) && isfinite(colors[3 * g + 2]);
      if (!ok) {
        bad = 1;  // any thread that finds one: the same value from all of them
      } else {
        int box[4];
        rs_box(fr, P, rad, n, ss, half, F, box);
        const int x0 = max(box[0], sx0), x1 = min(box[1], sx1), y0 = max(box[2], sy0), y1 = min(box[3], sy1);
        if (x0 <= x1 && y0 <= y1) {
          area = (x1 - x0 + 1) * (y1 - y0 + 1);
          for (int d = 0; d < 3; ++d) p.m[d] = fr.C[d] - P[d];
          p.c = rs_dot(p.m, p.m) - rad * rad;
          p.k = k;
          p.x0 = x0;
          p.y0 = y0;
          p.w = x1 - x0 + 1;
        }
      }
    }
    int excl;
    const int total = block_scan<kRsThreads>(area, &excl, scratch);
    if (area) pt[t] = p;
    pre[t] = excl;  // points without samples share their prefix with the next one that has some (owner())
    __syncthreads();
    for (int x = t; x < total; x += kRsThreads) {
      const int o = owner(pre, kRsThreads, x);
      const int e = x - pre[o], dy = e / pt[o].w, dx = e - dy * pt[o].w;
      const int sx = pt[o].x0 + dx, sy = pt[o].y0 + dy;
      double D[3], tt;
      rs_dir(fr, sx, sy, ss, half, F, D);
      if (rs_hit(pt[o].m, pt[o].c, D, &tt)) {
        const uint64_t kk = ((uint64_t)__float_as_uint((float)tt) << 32) | (uint32_t)pt[o].k;
        atomicMin(&key[(sy - sy0) * ts + (sx - sx0)], kk);  // integer minimum: the order of the hits does not matter
      }
    }
    __syncthreads();
  }
  const bool blank = bad != 0;
  if (blank && tile == 0 && t == 0 && status) atomicOr(status, DPC_STATUS_NONFINITE);
  const int i = ty * kRsTile + t / kRsTile, j = tx * kRsTile + t % kRsTile;
  if (i >= S || j >= S) return;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < ss; ++a)
    for (int b = 0; b < ss; ++b) {
      const int sy = i * ss + a, sx = j * ss + b;
      const uint64_t kk = blank ? kRsEmpty : key[(sy - sy0) * ts + (sx - sx0)];
      double col[3] = {1.0, 1.0, 1.0};  // the white world
      int id = -1;
      if (kk != kRsEmpty) {
        id = (int)(uint32_t)kk;
        const int64_t g = (int64_t)start + id;
        const double P[3] = {points[3 * g], points[3 * g + 1], points[3 * g + 2]};
        const double rad = radii ? radii[g] : rad0;
        double m[3], D[3], tt = 0.0;
        for (int d = 0; d < 3; ++d) m[d] = fr.C[d] - P[d];
        rs_dir(fr, sx, sy, ss, half, F, D);
        rs_hit(m, rs_dot(m, m) - rad * rad, D, &tt);  // the winner's hit, recomputed with the same operations
        const double nd = sqrt(rs_dot(D, D));
        double nrm[3], v[3];
        for (int d = 0; d < 3; ++d) {
          const double H = fr.C[d] + tt * D[d];
          nrm[d] = (H - P[d]) / rad;
          v[d] = -D[d] / nd;
        }
        const double nv = rs_dot(nrm, v);
        const double shade = 0.4 + 0.6 * (nv > 0.0 ? nv : 0.0);
        for (int d = 0; d < 3; ++d) col[d] = (colors ? (double)colors[3 * g + d] : 0.5) * shade;
      }
      for (int d = 0; d < 3; ++d) acc[d] = acc[d] + col[d];
      if (ids) ids[(int64_t)img * n * n + (int64_t)sy * n + sx] = id;
    }
  float* px = image + (((int64_t)img * S + i) * S + j) * 3;
  for (int d = 0; d < 3; ++d) px[d] = (float)(acc[d] / (double)(ss * ss));
}

}  // namespace

extern "C" {

int dpc_render_points(const double* points, const float* colors, const double* radii, int n_points, const int32_t* table,
                      const int32_t* host_table, int images, const double* frames, int image_size, int supersample,
                      double focal, double radius, float* image, int32_t* ids, int32_t* status, void* stream) {
  const int S = image_size, ss = supersample;
  if (images < 0 || n_points < 0 || (int64_t)n_points * 3 > INT32_MAX || S < 1 || S > 4096 || ss < 1 || ss > kRsMaxSS ||
      !(focal > 0.0 && focal <= DBL_MAX) || !(radius > 0.0 && radius <= DBL_MAX))
    return DPC_ERR_SHAPE;
  const int tiles_x = (S + kRsTile - 1) / kRsTile;
  if ((int64_t)images * tiles_x * tiles_x * kRsThreads > INT32_MAX) return DPC_ERR_SHAPE;
  if (images == 0) return DPC_OK;
  if (!host_table) return DPC_ERR_NULL;
  const int rc = check_desc<2>(host_table, images, {(int64_t)n_points}, INT64_MAX, nullptr,
                               [](const int32_t*) { return true; });
  if (rc != DPC_OK) return rc;
  if (!table || !frames || !image || (n_points > 0 && !points)) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_rs_tile", dpc_kid("k_rs_tile"), k_rs_tile, dim3(images * tiles_x * tiles_x), dim3(kRsThreads), 0, st,
             points, colors, radii, table, frames, tiles_x, S, ss, focal, radius, image, ids, status);
  return launch_ok();
}

}  // extern "C"
