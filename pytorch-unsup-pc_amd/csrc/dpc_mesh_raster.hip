// Batched rendering of triangle meshes to the training views (RGBA, 16-bit depth, face ids): what the reference downloads
// as <synth_set>-renders.tar.gz, made here from the meshes with the camera of the reference's own projection, in fp64.
// Semantics in include/dpc_render.h (dpc_render_meshes); cost model and measurements in DESIGN.md.
//
// Four launches per call, all on the caller's stream:
//   k_mr_offsets  one thread: where each view's projected vertices and face boxes start in the workspace;
//   k_mr_project  one thread per (view, vertex of its mesh): r = R p, d, the image-plane position in pixels, 1 / d;
//   k_mr_setup    one thread per (view, face): the face's checks (indices, material, finite values, the near guard, a
//                 projected area of zero) and the box of samples it can cover, 8 bytes, empty when it covers nothing;
//   k_mr_tile     one workgroup per (view, 16 x 16-pixel tile), view-major: the tile's sample keys (16 * 16 * ss^2 uint64,
//                 at most 32 KiB) in LDS; the view's face boxes stream through in chunks of 256, the boxes clipped to the
//                 tile are prefixed (block_scan) and the threads walk the chunk's (box sample, face) pairs, each covered
//                 sample an LDS 64-bit atomicMin of (bits(float(d)) << 32 | face): the minimum is order-independent.
//                 Then one thread per pixel shades its ss^2 samples and writes the pixel.
// dpc_render_meshes_shaded runs the same four kernels as their <true> instantiations (a mesh row of 12, not 6): k_mr_setup
// also checks the faces' uv, normal and texture indices, and k_mr_tile's last stage interpolates the winning face's uvs and
// normals per sample, perspective-correct, and filters its texture; everything up to the keys is the same code.
// Built with -ffp-contract=off: every product and sum is rounded on its own, as numpy rounds it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#include "dpc_launch.h"

namespace {

constexpr int kMrTile = 16;                       // pixels per tile side
constexpr int kMrThreads = kMrTile * kMrTile;     // one thread per tile pixel when shading
constexpr int kMrChunk = kMrThreads;              // faces per pass over the tile
constexpr int kMrMaxSS = 4;
constexpr int kMrMaxSize = 1024;
constexpr int kMrKeys = kMrThreads * kMrMaxSS * kMrMaxSS;  // 4096 keys, 32 KiB
constexpr uint64_t kMrEmpty = ~0ull;              // background
constexpr int kMrDesc = 6;                        // a mesh row: vertices, faces, materials as (start, count)
constexpr int kMrDescShaded = 12;                 // ... then uvs, normals and textures as (start, count)
constexpr int kMrTexDesc = 3;                     // a texture's int64s: byte offset of its texels, width, height
constexpr int kMrMaxTexSide = 65536;
constexpr int kMrCam = 11;                        // a view's doubles: R (row-major), camera_distance, focal_length
constexpr int kMrMaxViews = 65535;                // the launches' grid.y

// A projected vertex: image-plane position in pixels (column x, row y), 1 / d and d.
struct MrVert {
  double x, y, w, d;
};

// What dpc_render_meshes_shaded adds to the flat entry's arguments (device pointers; a NULL face_uv switches textures off,
// a NULL face_vn smooth normals).  It is the one member of the shaded instantiations' argument pack `attr`; the flat
// instantiations' pack is empty, so their arguments and their code are what they were before there was a shaded entry.
struct MrAttr {
  const double* uv;
  const int32_t* face_uv;
  const double* normals;
  const int32_t* face_vn;
  const int32_t* mat_tex;
  const int64_t* tex;
  const uint8_t* texels;
};

template <bool kShaded>
constexpr int mr_desc() {
  return kShaded ? kMrDescShaded : kMrDesc;
}

// A face of the current chunk whose box meets the tile: its projected vertices, its signed area, its index in the mesh
// and its box clipped to the tile (columns x0 .. x0 + bw - 1, rows from y0).
struct MrFace {
  double x[3], y[3], w[3];
  double area;
  int k, x0, y0, bw;
};

// The edge function of the directed edge a -> b at p, (b - a) x (p - a), evaluated on the lexicographically ordered pair
// and negated when that swaps the ends: the two faces on an edge get the same bits (up to the sign), so no sample between
// them is lost to rounding.
__device__ inline double mr_edge(double ax, double ay, double bx, double by, double px, double py) {
  const bool flip = bx < ax || (bx == ax && by < ay);
  const double cx = flip ? bx : ax, cy = flip ? by : ay, ex = flip ? ax : bx, ey = flip ? ay : by;
  const double g = (ex - cx) * (py - cy) - (ey - cy) * (px - cx);
  return flip ? -g : g;
}

// The position of sample column / row s = pixel * ss + sub-sample.
__device__ inline double mr_pos(int s, int ss) {
  const int j = s / ss, b = s - j * ss;
  return (double)j + ((double)b + 0.5) / (double)ss;
}

// Whether the sample at (px, py) is covered, and its depth: 1 / d interpolated linearly in the image plane.
__device__ inline bool mr_cover(const double* x, const double* y, const double* w, double area, double px, double py,
                                double* d) {
  const double e0 = mr_edge(x[1], y[1], x[2], y[2], px, py);
  const double e1 = mr_edge(x[2], y[2], x[0], y[0], px, py);
  const double e2 = mr_edge(x[0], y[0], x[1], y[1], px, py);
  const bool in = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
  if (!in) return false;
  const double iw = ((e0 / area) * w[0] + (e1 / area) * w[1]) + (e2 / area) * w[2];
  if (!(iw > 0.0)) return false;
  *d = 1.0 / iw;
  return true;
}

__device__ inline int mr_clamp(double x, int lo, int hi) { return x < (double)lo ? lo : (x > (double)hi ? hi : (int)x); }

template <int kDesc>
__global__ void k_mr_offsets(const int32_t* __restrict__ meshes, const int32_t* __restrict__ view_mesh, int views,
                             int64_t* __restrict__ voff, int64_t* __restrict__ foff) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t v = 0, f = 0;
  for (int w = 0; w < views; ++w) {
    const int32_t* m = meshes + kDesc * (int64_t)view_mesh[w];
    voff[w] = v;
    foff[w] = f;
    v += m[1];
    f += m[3];
  }
}

template <int kDesc>
__global__ __launch_bounds__(kMrThreads) void k_mr_project(const double* __restrict__ verts,
                                                           const int32_t* __restrict__ meshes,
                                                           const int32_t* __restrict__ view_mesh,
                                                           const double* __restrict__ view_cam,
                                                           const int64_t* __restrict__ voff, int S,
                                                           MrVert* __restrict__ proj, int32_t* __restrict__ status) {
  const int view = blockIdx.y;
  const int32_t* m = meshes + kDesc * (int64_t)view_mesh[view];
  const int i = blockIdx.x * kMrThreads + threadIdx.x;
  if (i >= m[1]) return;
  const double* cam = view_cam + kMrCam * (int64_t)view;
  const double* p = verts + 3 * ((int64_t)m[0] + i);
  const double p0 = p[0], p1 = p[1], p2 = p[2];
  double r[3];
  for (int k = 0; k < 3; ++k) r[k] = (cam[3 * k] * p0 + cam[3 * k + 1] * p1) + cam[3 * k + 2] * p2;
  const double f = cam[10];
  MrVert o;
  o.d = r[0] + cam[9];
  const double v = (r[1] * f) / o.d, u = (r[2] * f) / o.d;
  o.x = (u + 0.5) * (double)S;
  o.y = (0.5 - v) * (double)S;
  o.w = 1.0 / o.d;
  if (!(isfinite(p0) && isfinite(p1) && isfinite(p2))) {
    o.d = nan("");
    if (status) atomicOr(status, DPC_STATUS_NONFINITE);
  }
  proj[voff[view] + i] = o;
}

// The shaded entry's index guard of face g (row m, material mat checked): a uv, normal or texture index below -1 or
// outside its range.
__device__ inline bool mr_attr_bad(const MrAttr& at, const int32_t* m, int64_t g, int mat) {
  bool bad = false;
  for (int c = 0; c < 3; ++c) {
    if (at.face_uv) {
      const int t = at.face_uv[3 * g + c];
      bad |= t < -1 || t >= m[7];
    }
    if (at.face_vn) {
      const int t = at.face_vn[3 * g + c];
      bad |= t < -1 || t >= m[9];
    }
  }
  if (at.face_uv) {
    const int t = at.mat_tex[(int64_t)m[4] + mat];
    bad |= t < -1 || t >= m[11];
  }
  return bad;
}

// Whether a uv or a normal that face g names (its indices checked by mr_attr_bad) is not finite.
__device__ inline bool mr_attr_nonfinite(const MrAttr& at, const int32_t* m, int64_t g) {
  bool bad = false;
  for (int c = 0; c < 3; ++c) {
    const int t = at.face_uv ? at.face_uv[3 * g + c] : -1;
    if (t >= 0) {
      const double* q = at.uv + 2 * ((int64_t)m[6] + t);
      bad |= !(isfinite(q[0]) && isfinite(q[1]));
    }
    const int n = at.face_vn ? at.face_vn[3 * g + c] : -1;
    if (n >= 0) {
      const double* q = at.normals + 3 * ((int64_t)m[8] + n);
      bad |= !(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]));
    }
  }
  return bad;
}

template <bool kShaded, class... Attr>
__global__ __launch_bounds__(kMrThreads) void k_mr_setup(const int32_t* __restrict__ faces,
                                                         const int32_t* __restrict__ face_mat,
                                                         const int32_t* __restrict__ meshes,
                                                         const int32_t* __restrict__ view_mesh,
                                                         const int64_t* __restrict__ voff,
                                                         const int64_t* __restrict__ foff,
                                                         const MrVert* __restrict__ proj, int S, int ss,
                                                         short4* __restrict__ boxes, int32_t* __restrict__ status,
                                                         Attr... attr) {
  const int view = blockIdx.y;
  const int32_t* m = meshes + mr_desc<kShaded>() * (int64_t)view_mesh[view];
  const int i = blockIdx.x * kMrThreads + threadIdx.x;
  if (i >= m[3]) return;
  const int64_t g = (int64_t)m[2] + i;
  const int vcount = m[1], kcount = m[5];
  const int a = faces[3 * g], b = faces[3 * g + 1], c = faces[3 * g + 2], mat = face_mat[g];
  short4 box = make_short4(1, 0, 1, 0);  // empty
  int bits = 0;
  bool bad = a < 0 || a >= vcount || b < 0 || b >= vcount || c < 0 || c >= vcount || mat < 0 || mat >= kcount;
  if constexpr (kShaded) {
    if (!bad) bad = mr_attr_bad((attr, ...), m, g, mat);
  }
  if (bad) {
    bits = DPC_STATUS_BAD_INDEX;
  } else {
    const MrVert* pv = proj + voff[view];
    const MrVert v[3] = {pv[a], pv[b], pv[c]};
    for (int k = 0; k < 3; ++k) {
      if (!isfinite(v[k].d)) bits |= DPC_STATUS_NONFINITE;
      else if (v[k].d <= DPC_MESH_NEAR) bits |= DPC_STATUS_NEAR;
      else if (!(isfinite(v[k].x) && isfinite(v[k].y))) bits |= DPC_STATUS_NONFINITE;
    }
    if constexpr (kShaded) {
      if (mr_attr_nonfinite((attr, ...), m, g)) bits |= DPC_STATUS_NONFINITE;
    }
    if (!bits && mr_edge(v[0].x, v[0].y, v[1].x, v[1].y, v[2].x, v[2].y) != 0.0) {
      const int n = S * ss;
      const double s = (double)ss;
      const double xlo = fmin(v[0].x, fmin(v[1].x, v[2].x)), xhi = fmax(v[0].x, fmax(v[1].x, v[2].x));
      const double ylo = fmin(v[0].y, fmin(v[1].y, v[2].y)), yhi = fmax(v[0].y, fmax(v[1].y, v[2].y));
      // column sx holds x = (sx + 0.5) / ss: one sample more on every side for the rounding of the positions
      box.x = (short)mr_clamp(floor(xlo * s - 0.5) - 1.0, -1, n);
      box.y = (short)mr_clamp(ceil(xhi * s - 0.5) + 1.0, -1, n);
      box.z = (short)mr_clamp(floor(ylo * s - 0.5) - 1.0, -1, n);
      box.w = (short)mr_clamp(ceil(yhi * s - 0.5) + 1.0, -1, n);
    }
  }
  if (bits && status) atomicOr(status, bits);
  boxes[foff[view] + i] = box;
}

// The projected vertices, the signed area and the material of face k of a view's mesh (k_mr_setup has checked it).
__device__ inline void mr_load(const int32_t* __restrict__ faces, int64_t g, const MrVert* __restrict__ pv, double* x,
                               double* y, double* w, double* area, int* idx) {
  for (int c = 0; c < 3; ++c) {
    idx[c] = faces[3 * g + c];
    const MrVert v = pv[idx[c]];
    x[c] = v.x;
    y[c] = v.y;
    w[c] = v.w;
  }
  *area = mr_edge(x[0], y[0], x[1], y[1], x[2], y[2]);
}

// What the shaded k_mr_tile keeps of the face it is shading: the uvs of its corners and its texture when it is textured,
// its corners' normals in camera space when it is smooth.
struct MrShadeFace {
  double u[3], v[3], n[3][3];
  const uint8_t* texel;  // the texture's first byte
  int tw, th;
  bool textured, smooth;
};

__device__ inline void mr_load_attr(const MrAttr& at, const int32_t* m, int64_t g, int mat, const double* cam,
                                    MrShadeFace* sf) {
  sf->textured = false;
  sf->smooth = false;
  if (at.face_uv) {
    const int tex = at.mat_tex[(int64_t)m[4] + mat];
    const int i0 = at.face_uv[3 * g], i1 = at.face_uv[3 * g + 1], i2 = at.face_uv[3 * g + 2];
    if (tex >= 0 && i0 >= 0 && i1 >= 0 && i2 >= 0) {
      const int idx[3] = {i0, i1, i2};
      for (int c = 0; c < 3; ++c) {
        const double* q = at.uv + 2 * ((int64_t)m[6] + idx[c]);
        sf->u[c] = q[0];
        sf->v[c] = q[1];
      }
      const int64_t* td = at.tex + kMrTexDesc * ((int64_t)m[10] + tex);
      sf->texel = at.texels + td[0];
      sf->tw = (int)td[1];
      sf->th = (int)td[2];
      sf->textured = true;
    }
  }
  if (at.face_vn) {
    const int i0 = at.face_vn[3 * g], i1 = at.face_vn[3 * g + 1], i2 = at.face_vn[3 * g + 2];
    if (i0 >= 0 && i1 >= 0 && i2 >= 0) {
      const int idx[3] = {i0, i1, i2};
      for (int c = 0; c < 3; ++c) {
        const double* q = at.normals + 3 * ((int64_t)m[8] + idx[c]);
        const double p0 = q[0], p1 = q[1], p2 = q[2];
        for (int k = 0; k < 3; ++k) sf->n[c][k] = (cam[3 * k] * p0 + cam[3 * k + 1] * p1) + cam[3 * k + 2] * p2;
      }
      sf->smooth = true;
    }
  }
}

// Index i of a texture axis of n texels, i in [-1, n]: wrapped by repeat; the clamp keeps any other value inside too.
__device__ inline int mr_wrap(int i, int n) {
  i = i < 0 ? i + n : (i >= n ? i - n : i);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// The texture of sf filtered bilinearly at (u, v), both finite: rgb in [0, 1].
__device__ inline void mr_texture(const MrShadeFace& sf, double u, double v, double* rgb) {
  const double fu = u - floor(u), fv = v - floor(v);
  const double x = fu * (double)sf.tw - 0.5, y = (1.0 - fv) * (double)sf.th - 0.5;
  const double xf = floor(x), yf = floor(y);
  const double ax = x - xf, ay = y - yf;
  const double bx = 1.0 - ax, by = 1.0 - ay;
  const int x0 = mr_wrap((int)xf, sf.tw), x1 = mr_wrap((int)xf + 1, sf.tw);
  const int y0 = mr_wrap((int)yf, sf.th), y1 = mr_wrap((int)yf + 1, sf.th);
  const uint8_t* t00 = sf.texel + 3 * ((int64_t)y0 * sf.tw + x0);
  const uint8_t* t01 = sf.texel + 3 * ((int64_t)y0 * sf.tw + x1);
  const uint8_t* t10 = sf.texel + 3 * ((int64_t)y1 * sf.tw + x0);
  const uint8_t* t11 = sf.texel + 3 * ((int64_t)y1 * sf.tw + x1);
  for (int c = 0; c < 3; ++c) {
    const double top = ((double)t00[c] / 255.0) * bx + ((double)t01[c] / 255.0) * ax;
    const double bot = ((double)t10[c] / 255.0) * bx + ((double)t11[c] / 255.0) * ax;
    rgb[c] = top * by + bot * ay;
  }
}

template <bool kShaded, class... Attr>
__global__ __launch_bounds__(kMrThreads) void k_mr_tile(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                        const int32_t* __restrict__ face_mat, const double* __restrict__ kd,
                                                        const int32_t* __restrict__ meshes,
                                                        const int32_t* __restrict__ view_mesh,
                                                        const double* __restrict__ view_cam,
                                                        const int64_t* __restrict__ voff, const int64_t* __restrict__ foff,
                                                        const MrVert* __restrict__ proj, const short4* __restrict__ boxes,
                                                        int tiles_x, int S, int ss, uint8_t* __restrict__ rgba,
                                                        uint16_t* __restrict__ depth, int32_t* __restrict__ face_id,
                                                        Attr... attr) {
  __shared__ uint64_t key[kMrKeys];
  __shared__ MrFace fc[kMrChunk];
  __shared__ int pre[kMrChunk];
  __shared__ int scratch[kMrThreads / 64 + 1];
  const int t = threadIdx.x;
  const int tiles = tiles_x * tiles_x;
  const int view = blockIdx.x / tiles, tile = blockIdx.x - view * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int32_t* m = meshes + mr_desc<kShaded>() * (int64_t)view_mesh[view];
  const int vstart = m[0], fstart = m[2], count = m[3], kstart = m[4];
  const MrVert* pv = proj + voff[view];
  const short4* bx = boxes + foff[view];
  const int n = S * ss, ts = kMrTile * ss;  // samples per image side, per tile side
  const int sx0 = tx * ts, sy0 = ty * ts;
  const int sx1 = min(n, sx0 + ts) - 1, sy1 = min(n, sy0 + ts) - 1;  // inclusive
  for (int i = t; i < ts * ts; i += kMrThreads) key[i] = kMrEmpty;
  __syncthreads();
  for (int c0 = 0; c0 < count; c0 += kMrChunk) {
    const int k = c0 + t;
    int area = 0, x0 = 0, y0 = 0, x1 = 0;
    if (k < count) {
      const short4 b = bx[k];
      x0 = max((int)b.x, sx0);
      x1 = min((int)b.y, sx1);
      y0 = max((int)b.z, sy0);
      const int y1 = min((int)b.w, sy1);
      if (x0 <= x1 && y0 <= y1) area = (x1 - x0 + 1) * (y1 - y0 + 1);
    }
    int excl;
    const int total = block_scan<kMrThreads>(area, &excl, scratch);
    if (total == 0) continue;  // uniform: no face of this chunk meets the tile
    if (area) {
      MrFace f;
      int idx[3];
      mr_load(faces, (int64_t)fstart + k, pv, f.x, f.y, f.w, &f.area, idx);
      f.k = k;
      f.x0 = x0;
      f.y0 = y0;
      f.bw = x1 - x0 + 1;
      fc[t] = f;
    }
    pre[t] = excl;  // faces without samples share their prefix with the next one that has some (owner())
    __syncthreads();
    for (int x = t; x < total; x += kMrThreads) {
      const int o = owner(pre, kMrThreads, x);
      const int e = x - pre[o], dy = e / fc[o].bw, dx = e - dy * fc[o].bw;
      const int sx = fc[o].x0 + dx, sy = fc[o].y0 + dy;
      double d;
      if (mr_cover(fc[o].x, fc[o].y, fc[o].w, fc[o].area, mr_pos(sx, ss), mr_pos(sy, ss), &d)) {
        const uint64_t kk = ((uint64_t)__float_as_uint((float)d) << 32) | (uint32_t)fc[o].k;
        atomicMin(&key[(sy - sy0) * ts + (sx - sx0)], kk);  // integer minimum: the order of the faces does not matter
      }
    }
    __syncthreads();
  }
  const int i = ty * kMrTile + t / kMrTile, j = tx * kMrTile + t % kMrTile;
  if (i >= S || j >= S) return;
  const double* cam = view_cam + kMrCam * (int64_t)view;
  double acc[3] = {0.0, 0.0, 0.0}, col[3] = {0.0, 0.0, 0.0};
  double x[3], y[3], w[3], area = 0.0, best_d = 0.0;
  int covered = 0, last = -1;
  uint64_t best = kMrEmpty;
  [[maybe_unused]] MrShadeFace sf;
  [[maybe_unused]] double flat = 0.0;
  for (int a = 0; a < ss; ++a)
    for (int b = 0; b < ss; ++b) {
      const int sy = i * ss + a, sx = j * ss + b;
      const uint64_t kk = key[(sy - sy0) * ts + (sx - sx0)];
      if (kk == kMrEmpty) continue;
      const int k = (int)(uint32_t)kk;
      if (k != last) {
        last = k;
        const int64_t g = (int64_t)fstart + k;
        int idx[3];
        mr_load(faces, g, pv, x, y, w, &area, idx);
        double r[3][3];  // the face's vertices in camera space
        for (int c = 0; c < 3; ++c) {
          const double* p = verts + 3 * ((int64_t)vstart + idx[c]);
          const double p0 = p[0], p1 = p[1], p2 = p[2];
          for (int q = 0; q < 3; ++q) r[c][q] = (cam[3 * q] * p0 + cam[3 * q + 1] * p1) + cam[3 * q + 2] * p2;
        }
        const double e1[3] = {r[1][0] - r[0][0], r[1][1] - r[0][1], r[1][2] - r[0][2]};
        const double e2[3] = {r[2][0] - r[0][0], r[2][1] - r[0][1], r[2][2] - r[0][2]};
        const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2],
                     n2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        const double cn = nn > 0.0 ? fabs(n0) / nn : 0.0;  // |n . (-1, 0, 0)|: the headlight
        const double shade = DPC_MESH_AMBIENT + DPC_MESH_DIFFUSE * cn;
        const int mat = face_mat[g];
        const double* albedo = kd + 3 * ((int64_t)kstart + mat);
        if constexpr (kShaded) {
          for (int c = 0; c < 3; ++c) col[c] = albedo[c];
          flat = shade;
          mr_load_attr((attr, ...), m, g, mat, cam, &sf);
        } else {
          for (int c = 0; c < 3; ++c) col[c] = albedo[c] * shade;
        }
      }
      if constexpr (kShaded) {
        // the attribute weights c_k = ((e_k / A) w_k) d: mr_cover's own terms, so d is the depth the key was made of
        const double px = mr_pos(sx, ss), py = mr_pos(sy, ss);
        const double e0 = mr_edge(x[1], y[1], x[2], y[2], px, py);
        const double e1 = mr_edge(x[2], y[2], x[0], y[0], px, py);
        const double e2 = mr_edge(x[0], y[0], x[1], y[1], px, py);
        const double g0 = (e0 / area) * w[0], g1 = (e1 / area) * w[1], g2 = (e2 / area) * w[2];
        const double d = 1.0 / ((g0 + g1) + g2);
        const double c0 = g0 * d, c1 = g1 * d, c2 = g2 * d;
        double rgb[3] = {col[0], col[1], col[2]}, shade = flat;
        if (sf.textured) {
          const double u = (c0 * sf.u[0] + c1 * sf.u[1]) + c2 * sf.u[2];
          const double v = (c0 * sf.v[0] + c1 * sf.v[1]) + c2 * sf.v[2];
          if (isfinite(u) && isfinite(v)) mr_texture(sf, u, v, rgb);
        }
        if (sf.smooth) {
          const double n0 = (c0 * sf.n[0][0] + c1 * sf.n[1][0]) + c2 * sf.n[2][0];
          const double n1 = (c0 * sf.n[0][1] + c1 * sf.n[1][1]) + c2 * sf.n[2][1];
          const double n2 = (c0 * sf.n[0][2] + c1 * sf.n[1][2]) + c2 * sf.n[2][2];
          const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
          if (nn > 0.0 && isfinite(nn)) shade = DPC_MESH_AMBIENT + DPC_MESH_DIFFUSE * (fabs(n0) / nn);
        }
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + rgb[c] * shade;
        ++covered;
        if (kk < best) {
          best = kk;
          best_d = d;
        }
      } else {
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + col[c];
        ++covered;
        if (kk < best) {
          best = kk;
          mr_cover(x, y, w, area, mr_pos(sx, ss), mr_pos(sy, ss), &best_d);  // the winner's fp64 depth, recomputed
        }
      }
    }
  const int64_t px = ((int64_t)view * S + i) * S + j;
  uint8_t out[4] = {0, 0, 0, 0};
  uint16_t dq = 65535;
  if (covered) {
    for (int c = 0; c < 3; ++c) {
      double v = acc[c] / (double)covered;
      v = v > 1.0 ? 1.0 : (v >= 0.0 ? v : 0.0);
      out[c] = (uint8_t)floor(255.0 * v + 0.5);
    }
    out[3] = (uint8_t)floor(255.0 * ((double)covered / (double)(ss * ss)) + 0.5);
    const double q = floor(best_d / 10.0 * 65535.0 + 0.5);
    dq = (uint16_t)(q > 65535.0 ? 65535.0 : q);
  }
  *reinterpret_cast<uchar4*>(rgba + 4 * px) = make_uchar4(out[0], out[1], out[2], out[3]);
  depth[px] = dq;
  if (face_id) face_id[px] = covered ? (int32_t)(uint32_t)best : -1;
}

// Host checks shared by the entry points: the mesh table's ranges (K (start, count) pairs per row, against len) and the
// views' mesh indices.  DPC_OK with the views' vertex and face totals and the largest counts of a viewed mesh.
template <int K>
int mr_check(const int32_t* host_meshes, int n_meshes, const int32_t* host_view_mesh, int views, const int64_t (&len)[K],
             int64_t* sum_v, int64_t* sum_f, int* max_v, int* max_f) {
  if (n_meshes < 0 || views < 0 || views > kMrMaxViews) return DPC_ERR_SHAPE;
  if ((n_meshes > 0 && !host_meshes) || (views > 0 && !host_view_mesh)) return DPC_ERR_NULL;
  const int rc = check_desc<2 * K>(host_meshes, n_meshes, len, INT64_MAX, nullptr, [](const int32_t*) { return true; });
  if (rc != DPC_OK) return rc;
  int64_t sv = 0, sf = 0;
  int mv = 0, mf = 0;
  for (int w = 0; w < views; ++w) {
    const int m = host_view_mesh[w];
    if (m < 0 || m >= n_meshes) return DPC_ERR_SHAPE;
    const int32_t* d = host_meshes + 2 * K * (int64_t)m;
    sv += d[1];
    sf += d[3];
    mv = d[1] > mv ? d[1] : mv;
    mf = d[3] > mf ? d[3] : mf;
  }
  *sum_v = sv;
  *sum_f = sf;
  *max_v = mv;
  *max_f = mf;
  return DPC_OK;
}

struct MrSpace {
  int64_t* voff;
  int64_t* foff;
  MrVert* proj;
  short4* boxes;
};

size_t mr_carve(void* workspace, int views, int64_t sum_v, int64_t sum_f, MrSpace* sp) {
  Carver cv{static_cast<char*>(workspace)};
  sp->voff = cv.take<int64_t>((size_t)views);
  sp->foff = cv.take<int64_t>((size_t)views);
  sp->proj = cv.take<MrVert>((size_t)sum_v);
  sp->boxes = cv.take<short4>((size_t)sum_f);
  return cv.off;
}

// The four launches of both entry points.
template <bool kShaded>
int mr_launch(const double* verts, const int32_t* faces, const int32_t* face_mat, const double* kd, const int32_t* meshes,
              const int32_t* view_mesh, const double* view_cam, int views, int64_t sv, int64_t sf, int mv, int mf, int S,
              int ss, uint8_t* rgba, uint16_t* depth, int32_t* face_id, int32_t* status, void* workspace, void* stream,
              const MrAttr& at) {
  constexpr int kDesc = mr_desc<kShaded>();
  const int tiles_x = (S + kMrTile - 1) / kMrTile;
  MrSpace sp;
  mr_carve(workspace, views, sv, sf, &sp);
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_mr_offsets", dpc_kid("k_mr_offsets", kDesc), k_mr_offsets<kDesc>, dim3(1), dim3(64), 0, st, meshes,
             view_mesh, views, sp.voff, sp.foff);
  if (mv > 0)
    DPC_LAUNCH("k_mr_project", dpc_kid("k_mr_project", kDesc), k_mr_project<kDesc>,
               dim3((mv + kMrThreads - 1) / kMrThreads, views), dim3(kMrThreads), 0, st, verts, meshes, view_mesh, view_cam,
               sp.voff, S, sp.proj, status);
  const dim3 setup((mf + kMrThreads - 1) / kMrThreads, views), tile(views * tiles_x * tiles_x);
  if constexpr (kShaded) {
    if (mf > 0)
      DPC_LAUNCH("k_mr_setup", dpc_kid("k_mr_setup", 1), k_mr_setup<true>, setup, dim3(kMrThreads), 0, st, faces, face_mat,
                 meshes, view_mesh, sp.voff, sp.foff, sp.proj, S, ss, sp.boxes, status, at);
    DPC_LAUNCH("k_mr_tile", dpc_kid("k_mr_tile", 1), k_mr_tile<true>, tile, dim3(kMrThreads), 0, st, verts, faces, face_mat,
               kd, meshes, view_mesh, view_cam, sp.voff, sp.foff, sp.proj, sp.boxes, tiles_x, S, ss, rgba, depth, face_id, at);
  } else {
    if (mf > 0)
      DPC_LAUNCH("k_mr_setup", dpc_kid("k_mr_setup", 0), k_mr_setup<false>, setup, dim3(kMrThreads), 0, st, faces, face_mat,
                 meshes, view_mesh, sp.voff, sp.foff, sp.proj, S, ss, sp.boxes, status);
    DPC_LAUNCH("k_mr_tile", dpc_kid("k_mr_tile", 0), k_mr_tile<false>, tile, dim3(kMrThreads), 0, st, verts, faces, face_mat,
               kd, meshes, view_mesh, view_cam, sp.voff, sp.foff, sp.proj, sp.boxes, tiles_x, S, ss, rgba, depth, face_id);
  }
  return launch_ok();
}

// The checks of sizes both entry points make first.
bool mr_sizes_ok(int n_verts, int n_faces, int n_mats, int S, int ss) {
  return !(n_verts < 0 || n_faces < 0 || n_mats < 0 || (int64_t)n_verts * 3 > INT32_MAX || (int64_t)n_faces * 3 > INT32_MAX ||
           (int64_t)n_mats * 3 > INT32_MAX || S < 1 || S > kMrMaxSize || ss < 1 || ss > kMrMaxSS);
}

}  // namespace

extern "C" {

size_t dpc_render_meshes_workspace_bytes(const int32_t* host_meshes, int n_meshes, const int32_t* host_view_mesh,
                                         int views) {
  int64_t sv, sf;
  int mv, mf;
  if (mr_check<3>(host_meshes, n_meshes, host_view_mesh, views, {-1, -1, -1}, &sv, &sf, &mv, &mf) != DPC_OK) return 0;
  MrSpace sp;
  return mr_carve(nullptr, views, sv, sf, &sp);
}

int dpc_render_meshes(const double* verts, int n_verts, const int32_t* faces, const int32_t* face_mat, int n_faces,
                      const double* kd, int n_mats, const int32_t* meshes, const int32_t* host_meshes, int n_meshes,
                      const int32_t* view_mesh, const int32_t* host_view_mesh, const double* view_cam, int views,
                      int image_size, int supersample, uint8_t* rgba, uint16_t* depth, int32_t* face_id,
                      int32_t* status, void* workspace, void* stream) {
  const int S = image_size, ss = supersample;
  if (!mr_sizes_ok(n_verts, n_faces, n_mats, S, ss)) return DPC_ERR_SHAPE;
  int64_t sv, sf;
  int mv, mf;
  const int rc = mr_check<3>(host_meshes, n_meshes, host_view_mesh, views, {n_verts, n_faces, n_mats}, &sv, &sf, &mv, &mf);
  if (rc != DPC_OK) return rc;
  const int tiles_x = (S + kMrTile - 1) / kMrTile;
  if ((int64_t)views * tiles_x * tiles_x * kMrThreads > INT32_MAX) return DPC_ERR_SHAPE;
  if (views == 0) return DPC_OK;
  if (!meshes || !view_mesh || !view_cam || !rgba || !depth || !workspace || (n_verts > 0 && !verts) ||
      (n_faces > 0 && (!faces || !face_mat)) || (n_mats > 0 && !kd))
    return DPC_ERR_NULL;
  return mr_launch<false>(verts, faces, face_mat, kd, meshes, view_mesh, view_cam, views, sv, sf, mv, mf, S, ss, rgba, depth,
                          face_id, status, workspace, stream, MrAttr{});
}

size_t dpc_render_meshes_shaded_workspace_bytes(const int32_t* host_meshes, int n_meshes, const int32_t* host_view_mesh,
                                                int views) {
  int64_t sv, sf;
  int mv, mf;
  if (mr_check<6>(host_meshes, n_meshes, host_view_mesh, views, {-1, -1, -1, -1, -1, -1}, &sv, &sf, &mv, &mf) != DPC_OK)
    return 0;
  MrSpace sp;
  return mr_carve(nullptr, views, sv, sf, &sp);
}

int dpc_render_meshes_shaded(const double* verts, int n_verts, const int32_t* faces, const int32_t* face_mat, int n_faces,
                             const double* kd, int n_mats, const double* uv, int n_uv, const int32_t* face_uv,
                             const double* normals, int n_vn, const int32_t* face_vn, const int32_t* mat_tex,
                             const uint8_t* texels, int64_t n_texel_bytes, const int64_t* tex, const int64_t* host_tex,
                             int n_tex, const int32_t* meshes, const int32_t* host_meshes, int n_meshes,
                             const int32_t* view_mesh, const int32_t* host_view_mesh, const double* view_cam, int views,
                             int image_size, int supersample, uint8_t* rgba, uint16_t* depth, int32_t* face_id,
                             int32_t* status, void* workspace, void* stream) {
  const int S = image_size, ss = supersample;
  if (!mr_sizes_ok(n_verts, n_faces, n_mats, S, ss) || n_uv < 0 || n_vn < 0 || n_tex < 0 || n_texel_bytes < 0 ||
      (int64_t)n_uv * 2 > INT32_MAX || (int64_t)n_vn * 3 > INT32_MAX)
    return DPC_ERR_SHAPE;
  if (n_tex > 0 && !host_tex) return DPC_ERR_NULL;
  for (int t = 0; t < n_tex; ++t) {  // every texture inside the texel buffer: 3 w h bytes from its offset
    const int64_t* d = host_tex + kMrTexDesc * (int64_t)t;
    if (d[0] < 0 || d[1] < 1 || d[1] > kMrMaxTexSide || d[2] < 1 || d[2] > kMrMaxTexSide ||
        d[0] > n_texel_bytes || 3 * d[1] * d[2] > n_texel_bytes - d[0])
      return DPC_ERR_SHAPE;
  }
  int64_t sv, sf;
  int mv, mf;
  const int rc = mr_check<6>(host_meshes, n_meshes, host_view_mesh, views, {n_verts, n_faces, n_mats, n_uv, n_vn, n_tex},
                             &sv, &sf, &mv, &mf);
  if (rc != DPC_OK) return rc;
  const int tiles_x = (S + kMrTile - 1) / kMrTile;
  if ((int64_t)views * tiles_x * tiles_x * kMrThreads > INT32_MAX) return DPC_ERR_SHAPE;
  if (views == 0) return DPC_OK;
  if (!meshes || !view_mesh || !view_cam || !rgba || !depth || !workspace || (n_verts > 0 && !verts) ||
      (n_faces > 0 && (!faces || !face_mat)) || (n_mats > 0 && !kd))
    return DPC_ERR_NULL;
  // the attribute groups are optional: face_uv switches textures on, face_vn smooth normals; a group that is on is whole
  if (face_uv && ((n_mats > 0 && !mat_tex) || (n_uv > 0 && !uv) || (n_tex > 0 && (!tex || !texels)))) return DPC_ERR_NULL;
  if (face_vn && n_vn > 0 && !normals) return DPC_ERR_NULL;
  const MrAttr at{uv, face_uv, normals, face_vn, mat_tex, tex, texels};
  return mr_launch<true>(verts, faces, face_mat, kd, meshes, view_mesh, view_cam, views, sv, sf, mv, mf, S, ss, rgba, depth,
                         face_id, status, workspace, stream, at);
}

}  // extern "C"
