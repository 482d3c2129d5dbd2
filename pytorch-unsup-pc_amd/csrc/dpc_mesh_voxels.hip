// Mesh voxelisation: triangle meshes to solid occupancy bit grids (a stand-in for binvox), and the "carve" fill for any
// bit grid.  The contract (the surface rule, the two fills, the counts, guards) is in include/dpc_render.h
// (dpc_voxelise_meshes); the operation order of every fp64 expression below is the one tests/mesh_voxels_oracle.py
// writes out, nothing is fused, so every output bit has one right answer.  Grid and bit layout are dpc_voxelise's.
//
// k_mv_surface<F64, WORDS, THREADS>   the word classes of k_voxelise (512 threads in the slab class): a workgroup owns WORDS consecutive words of one mesh's
//     bit grid in LDS, zeroes them, walks the mesh's faces THREADS at a time, ORs the nodes whose cube meets the face
//     with LDS atomics and writes the finished words with plain coalesced stores.  A face's candidate nodes are its
//     bounding box widened by 1/2, clipped to the grid and to the z-planes of the slab.  Load balance: a lane tests the
//     candidates of its own face when they are at most kMvLane; a face with more goes to an LDS queue that the waves
//     empty after the chunk, one face per wave, 64 candidates a step; a face with more than kMvWave candidates goes to
//     a second queue that the whole workgroup walks, THREADS candidates a step.  A queue holds at most one entry per
//     thread and chunk, so it cannot overflow.  Slab 0 of a mesh counts the faces with a vertex outside the cube.
// k_mv_parity<F64, THREADS>   a workgroup owns a run of z-planes of one mesh, held in LDS with every row padded to whole
//     words (so a step along axis 1 or 0 is a whole number of words whatever W is).  It walks all faces, finds the
//     columns each crosses (lanes and the wave queue as above, in 2-D) and XORs the toggle of a crossing into its plane,
//     or into one "before" plane when the toggle lies below the slab: the prefix XOR along axis 0 then needs no other
//     workgroup.  Toggles behind the slab go to an "after" plane, which only the count of open columns reads (slab 0).
//     The finished words are (surface | parity), assembled from the padded rows and stored coalesced.
// k_mv_carve<THREADS>         the same slabs of padded rows.  The slab's planes are loaded once; the planes before and
//     behind it are OR-ed into one plane each (LDS atomics), which is all the scan along axis 0 needs of them.  Then
//     prefix-OR & suffix-OR along axis 0 (a thread per word of a plane), along axis 1 (a thread per word column of a
//     plane), and along axis 2 inside the rows (a thread per row: everything from the first to the last set bit).
// When H * W is no multiple of 32 a slab's last word reaches into the next plane: the slab then also computes that one
// plane (a halo), so every output word still has exactly one owner and there is no global atomic but the status OR.
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

constexpr int kMvClasses = 3;
constexpr int kMvWords[kMvClasses] = {1024, 8192, 16384};     // words of a k_mv_surface workgroup: k_voxelise's classes
constexpr int kMvThreads[kMvClasses] = {256, 512, 512};   // 512 in the slab class too: 1024 would spill the fp64 face state
constexpr int kMvExtra = 8;             // ints behind the words: outside faces, flags, 2 pad, the two queue counts of even and odd chunks
constexpr int kMvLane = 64;             // candidates a lane tests on its own
constexpr int kMvWave = 4096;           // candidates a wave tests on its own
constexpr int kMvPadWords = 7680;       // padded words of the planes a k_mv_carve / k_mv_parity workgroup loads
constexpr int kMvPlaneWords = DPC_VOXEL_MAX_SIDE * ((DPC_VOXEL_MAX_SIDE + 31) / 32);   // the largest padded plane
static_assert(2 * kMvPadWords + 2 * kMvPlaneWords <= 16384, "k_mv_carve: two slabs and two planes in 64 KiB");
static_assert(kMvPadWords >= 2 * kMvPlaneWords, "a slab holds a plane and its halo");

constexpr int mv_class(int64_t words) { return words <= kMvWords[0] ? 0 : words <= kMvWords[1] ? 1 : 2; }

struct MvGrid : VoxelGrid {
  int Wp, PW;       // words of a padded row, of a padded plane
  int halo;         // 1: a slab's last word may reach into the next plane
  int zs, slabs;    // planes a slab owns, slabs of a grid
};

bool mv_grid(int D, int H, int W, int min_side, MvGrid* g) {
  if (!voxel_grid(D, H, W, min_side, g)) return false;
  g->Wp = (W + 31) / 32;
  g->PW = H * g->Wp;
  g->halo = (H * W) % 32 != 0;
  const int fit = kMvPadWords / g->PW;             // >= 2
  if (D <= fit) g->halo = 0;                       // one slab holds every plane
  g->zs = D <= fit ? D : fit - g->halo;
  g->slabs = (D + g->zs - 1) / g->zs;
  // a word that starts in a slab's last plane ends in the halo plane at the latest
  return g->slabs == 1 || H * W >= 32;
}

// n <= 32 bits of a flat bit array from bit f on; bits f .. f + n - 1 lie inside the array
__device__ inline uint32_t mv_bits(const uint32_t* __restrict__ w, int f, int n) {
  const int j = f >> 5, s = f & 31;
  uint32_t v = w[j] >> s;
  if (s + n > 32) v |= w[j + 1] << (32 - s);
  return n < 32 ? v & ((1u << n) - 1u) : v;
}

// word k of the padded row (z, y) of a flat bit grid
__device__ inline uint32_t mv_row_word(const uint32_t* __restrict__ bits, int z, int y, int k, int H, int W) {
  const int left = W - 32 * k;
  return mv_bits(bits, (z * H + y) * W + 32 * k, left < 32 ? left : 32);
}

// flat word j of a grid whose planes za .. are held as padded rows in `rows`
__device__ inline uint32_t mv_flat_word(const uint32_t* rows, int j, int za, int H, int W, int Wp, int V) {
  uint32_t out = 0u;
  int b = 0, f = 32 * j;
  while (b < 32 && f < V) {
    const int row = f / W, x = f - row * W;
    const int n = 32 - b < W - x ? 32 - b : W - x;
    const int z = row / H, y = row - z * H;
    out |= mv_bits(rows + ((z - za) * H + y) * Wp, x, n) << b;
    b += n;
    f += n;
  }
  return out;
}

constexpr int kMvBadIndex = 1, kMvNonFinite = 2, kMvOutside = 4;

struct MvMesh {
  int vstart, vcount, fstart, fcount;
};

// the table row of a mesh; false when it does not lie inside the packed arrays (nothing of it is then used)
__device__ inline bool mv_mesh(const int32_t* __restrict__ desc, int mesh, int n_verts, int n_faces, MvMesh* m) {
  const int32_t* d = desc + 4 * (size_t)mesh;
  m->vstart = d[0]; m->vcount = d[1]; m->fstart = d[2]; m->fcount = d[3];
  return m->vstart >= 0 && m->vcount >= 0 && (int64_t)m->vstart + m->vcount <= n_verts && m->fstart >= 0 && m->fcount >= 0 &&
         (int64_t)m->fstart + m->fcount <= n_faces;
}

// Grid coordinates u[v][c] of face i of a mesh; returns the flags of the face, and it is kept iff neither kMvBadIndex
// nor kMvNonFinite is among them.  An index outside the mesh never becomes an address.
template <int F64>
__device__ inline int mv_face(const void* __restrict__ verts_, const int32_t* __restrict__ faces, const MvMesh& m, int i, int D,
                              int H, int W, double (&u)[3][3]) {
#pragma clang fp contract(off)
  using T = std::conditional_t<F64 != 0, double, float>;
  const T* __restrict__ verts = static_cast<const T*>(verts_);
  const int32_t* f = faces + 3 * ((size_t)m.fstart + i);
  const int idx[3] = {f[0], f[1], f[2]};
  if ((unsigned)idx[0] >= (unsigned)m.vcount || (unsigned)idx[1] >= (unsigned)m.vcount || (unsigned)idx[2] >= (unsigned)m.vcount)
    return kMvBadIndex;
  const double g1[3] = {(double)(D - 1), (double)(H - 1), (double)(W - 1)};
  int flags = 0;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const T* p = verts + 3 * ((size_t)m.vstart + idx[v]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = (double)p[c];
      if (!(fabs(a) < DPC_MESH_VOXEL_MAX_COORD)) flags |= kMvNonFinite;   // a NaN too
      if (a < -0.5 || a > 0.5) flags |= kMvOutside;
      u[v][c] = (a + 0.5) * g1[c];
    }
  }
  return flags;
}

__device__ inline double mv_min3(double a, double b, double c) { return fmin(fmin(a, b), c); }
__device__ inline double mv_max3(double a, double b, double c) { return fmax(fmax(a, b), c); }

// nodes a .. b of [lo, hi] clamped to 0 .. G - 1, compared as fp64 before any conversion; false when there is none
__device__ inline bool mv_range(double lo, double hi, int G, int* a, int* b) {
  const double x = lo > 0.0 ? lo : 0.0, y = hi < (double)(G - 1) ? hi : (double)(G - 1);
  if (!(x <= y)) return false;
  *a = (int)x;
  *b = (int)y;
  return true;
}

// The candidate nodes of a face: its bounding box widened by 1/2, clipped to the grid.
struct MvBox {
  int a[3], n[3];
};

__device__ inline bool mv_box(const double (&u)[3][3], int D, int H, int W, MvBox* bx) {
#pragma clang fp contract(off)
  const int G[3] = {D, H, W};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int a, b;
    if (!mv_range(ceil(mv_min3(u[0][c], u[1][c], u[2][c]) - 0.5), floor(mv_max3(u[0][c], u[1][c], u[2][c]) + 0.5), G[c], &a, &b))
      return false;
    bx->a[c] = a;
    bx->n[c] = b - a + 1;
  }
  return true;
}

// The face's own edges and normal (they do not move with the node).
struct MvTri {
  double e[3][3], nr[3];
};

__device__ inline void mv_tri(const double (&u)[3][3], MvTri* t) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t->e[0][c] = u[1][c] - u[0][c];
    t->e[1][c] = u[2][c] - u[1][c];
    t->e[2][c] = u[0][c] - u[2][c];
  }
  t->nr[0] = t->e[0][1] * t->e[1][2] - t->e[0][2] * t->e[1][1];
  t->nr[1] = t->e[0][2] * t->e[1][0] - t->e[0][0] * t->e[1][2];
  t->nr[2] = t->e[0][0] * t->e[1][1] - t->e[0][1] * t->e[1][0];
}

// Does the closed cube of half-size 1/2 round the node meet the closed triangle?  13 separating axes on the vertices
// translated to the node; every comparison is strict, so touching counts as meeting.
__device__ inline bool mv_meets(const double (&u)[3][3], const MvTri& t, int n0, int n1, int n2) {
#pragma clang fp contract(off)
  const double nf[3] = {(double)n0, (double)n1, (double)n2};
  double p[3][3];
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int c = 0; c < 3; ++c) p[v][c] = u[v][c] - nf[c];
  bool sep = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) sep |= mv_min3(p[0][c], p[1][c], p[2][c]) > 0.5 || mv_max3(p[0][c], p[1][c], p[2][c]) < -0.5;
  const double d = (t.nr[0] * p[0][0] + t.nr[1] * p[0][1]) + t.nr[2] * p[0][2];
  const double rad = 0.5 * ((fabs(t.nr[0]) + fabs(t.nr[1])) + fabs(t.nr[2]));
  sep |= d > rad || d < -rad;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
#pragma unroll
    for (int ed = 0; ed < 3; ++ed) {
      const double ei = t.e[ed][i], ej = t.e[ed][j];
      const double q0 = ei * p[0][j] - ej * p[0][i], q1 = ei * p[1][j] - ej * p[1][i], q2 = ei * p[2][j] - ej * p[2][i];
      const double r = 0.5 * (fabs(ei) + fabs(ej));
      sep |= mv_min3(q0, q1, q2) > r || mv_max3(q0, q1, q2) < -r;
    }
  }
  return !sep;
}

// Candidates me, me + step, .. of the box, restricted to the words w0 .. w0 + nw - 1 the workgroup holds.
__device__ inline void mv_mark(const double (&u)[3][3], const MvBox& bx, int me, int step, int H, int W, int w0, int nw,
                               uint32_t* smem) {
  MvTri tri;
  mv_tri(u, &tri);
  const int plane = bx.n[1] * bx.n[2], cnt = bx.n[0] * plane;
  for (int c = me; c < cnt; c += step) {
    const int z = c / plane, r = c - z * plane;
    const int y = r / bx.n[2], x = r - y * bx.n[2];
    const int n0 = bx.a[0] + z, n1 = bx.a[1] + y, n2 = bx.a[2] + x;
    if (mv_meets(u, tri, n0, n1, n2)) {
      const int f = (n0 * H + n1) * W + n2;
      const int w = (f >> 5) - w0;
      if ((unsigned)w < (unsigned)nw) atomicOr(&smem[w], 1u << (f & 31));
    }
  }
}

template <int F64, int WORDS, int THREADS>
__global__ __launch_bounds__(THREADS) void k_mv_surface(const void* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces,
                                                        int n_faces, const int32_t* __restrict__ desc, int slabs, int D, int H, int W,
                                                        int words, uint32_t* __restrict__ bits, int32_t* __restrict__ info,
                                                        int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mv_smem[];  // [WORDS] bits, [kMvExtra] ints, two queues of THREADS faces
  int* const extra = reinterpret_cast<int*>(mv_smem + WORDS);
  int* const wave_q = extra + kMvExtra;
  int* const block_q = wave_q + THREADS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int mesh = blockIdx.x / slabs, slab = blockIdx.x - mesh * slabs;
  const int w0 = slab * WORDS;
  const int nw = words - w0 < WORDS ? words - w0 : WORDS;
  MvMesh m;
  if (!mv_mesh(desc, mesh, n_verts, n_faces, &m)) {
    if (slab == 0 && t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    return;
  }
  for (int j = t; j < nw; j += THREADS) mv_smem[j] = 0u;
  if (t < kMvExtra) extra[t] = 0;
  __syncthreads();

  // the z-planes the slab's words touch: a candidate box is clipped to them
  const int hw = H * W, V = D * hw;
  const int f_end = (w0 + nw) * 32 < V ? (w0 + nw) * 32 : V;
  const int z_lo = (w0 * 32) / hw, z_hi = (f_end - 1) / hw;

  int outside = 0, flags = 0;
  int chunk = 0;
  for (int base = 0; base < m.fcount; base += THREADS, ++chunk) {  // the same trip count in every thread: barriers inside
    int* const counts = extra + 4 + 2 * (chunk & 1);
    const int i = base + t;
    if (i < m.fcount) {
      double u[3][3];
      const int fl = mv_face<F64>(verts, faces, m, i, D, H, W, u);
      flags |= fl & (kMvBadIndex | kMvNonFinite);
      MvBox bx;
      if (!(fl & (kMvBadIndex | kMvNonFinite))) {
        outside += (fl & kMvOutside) != 0;
        if (mv_box(u, D, H, W, &bx)) {
          const int za = bx.a[0] > z_lo ? bx.a[0] : z_lo;
          const int zb = bx.a[0] + bx.n[0] - 1 < z_hi ? bx.a[0] + bx.n[0] - 1 : z_hi;
          if (za <= zb) {
            bx.a[0] = za;
            bx.n[0] = zb - za + 1;
            const int cnt = bx.n[0] * bx.n[1] * bx.n[2];
            if (cnt <= kMvLane) mv_mark(u, bx, 0, 1, H, W, w0, nw, mv_smem);
            else if (cnt <= kMvWave) wave_q[atomicAdd(&counts[0], 1)] = i;
            else block_q[atomicAdd(&counts[1], 1)] = i;
          }
        }
      }
    }
    __syncthreads();
    if (t == 0) { extra[4 + 2 * ((chunk + 1) & 1)] = 0; extra[5 + 2 * ((chunk + 1) & 1)] = 0; }  // the next chunk's counts
    const int n_wave = counts[0], n_block = counts[1];
    for (int q = 0; q < n_wave + n_block; ++q) {
      const bool whole = q >= n_wave;
      if (!whole && q % (THREADS / 64) != wave) continue;
      const int i2 = whole ? block_q[q - n_wave] : wave_q[q];
      double u[3][3];
      mv_face<F64>(verts, faces, m, i2, D, H, W, u);   // a queued face is a kept one
      MvBox bx;
      mv_box(u, D, H, W, &bx);
      const int za = bx.a[0] > z_lo ? bx.a[0] : z_lo;
      const int zb = bx.a[0] + bx.n[0] - 1 < z_hi ? bx.a[0] + bx.n[0] - 1 : z_hi;
      bx.a[0] = za;
      bx.n[0] = zb - za + 1;
      mv_mark(u, bx, whole ? t : lane, whole ? THREADS : 64, H, W, w0, nw, mv_smem);
    }
    __syncthreads();
  }
  if (slab == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) outside += __shfl_down(outside, off, 64);
    if (lane == 0 && outside) atomicAdd(&extra[0], outside);
    if (flags) atomicOr(&extra[1], flags);
  }
  __syncthreads();
  uint32_t* out = bits + (size_t)mesh * words + w0;
  for (int j = t; j < nw; j += THREADS) out[j] = mv_smem[j];
  if (slab == 0 && t == 0) {
    info[2 * (size_t)mesh] = extra[0];
    info[2 * (size_t)mesh + 1] = 0;   // open columns: k_mv_parity's
    if (status && (extra[1] & kMvBadIndex)) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    if (status && (extra[1] & kMvNonFinite)) atomicOr(status, (int)DPC_STATUS_NONFINITE);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// parity
struct MvCols {
  int ya, ny, xa, nx;
};

// The edge function of P -> Q at the column (cy, cx), evaluated from the lexicographically smaller endpoint and negated
// when that is Q: two faces that share the edge see equal or exactly opposite values.
__device__ inline double mv_edge(double py, double px, double qy, double qx, double cy, double cx) {
#pragma clang fp contract(off)
  const bool swap = py > qy || (py == qy && px > qx);
  const double ay = swap ? qy : py, ax = swap ? qx : px, by = swap ? py : qy, bx = swap ? px : qx;
  const double val = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  return swap ? -val : val;
}

// The projected face: false when its projected area is zero or no column lies in its bounding box.
__device__ inline bool mv_cols(const double (&u)[3][3], int H, int W, MvCols* c, bool* neg) {
#pragma clang fp contract(off)
  const double area = mv_edge(u[0][1], u[0][2], u[1][1], u[1][2], u[2][1], u[2][2]);
  if (area == 0.0) return false;
  *neg = area < 0.0;
  int a, b;
  if (!mv_range(ceil(mv_min3(u[0][1], u[1][1], u[2][1])), floor(mv_max3(u[0][1], u[1][1], u[2][1])), H, &a, &b)) return false;
  c->ya = a; c->ny = b - a + 1;
  if (!mv_range(ceil(mv_min3(u[0][2], u[1][2], u[2][2])), floor(mv_max3(u[0][2], u[1][2], u[2][2])), W, &a, &b)) return false;
  c->xa = a; c->nx = b - a + 1;
  return true;
}

// Columns me, me + step, .. of the face's box: a crossing toggles plane ceil(z*) clamped to 0 .. D.
__device__ inline void mv_cross(const double (&u)[3][3], const MvCols& c, bool neg, int me, int step, int D, int Wp, int PW, int za,
                                int ze, uint32_t* rows, uint32_t* before, uint32_t* after) {
#pragma clang fp contract(off)
  const int cnt = c.ny * c.nx;
  bool tl[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // w_k belongs to the edge opposite vertex k
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    double dy = u[b][1] - u[a][1], dx = u[b][2] - u[a][2];
    if (neg) { dy = -dy; dx = -dx; }
    tl[k] = dy > 0.0 || (dy == 0.0 && dx < 0.0);
  }
  for (int i = me; i < cnt; i += step) {
    const int yy = i / c.nx, y = c.ya + yy, x = c.xa + (i - yy * c.nx);
    const double cy = (double)y, cx = (double)x;
    double w[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a = (k + 1) % 3, b = (k + 2) % 3;
      const double val = mv_edge(u[a][1], u[a][2], u[b][1], u[b][2], cy, cx);
      w[k] = neg ? -val : val;
      in = in && (w[k] > 0.0 || (w[k] == 0.0 && tl[k]));
    }
    const double total = (w[0] + w[1]) + w[2];
    if (!in || total == 0.0) continue;
    const double zs = ((w[0] * u[0][0] + w[1] * u[1][0]) + w[2] * u[2][0]) / total;
    double kf = ceil(zs);
    kf = kf > 0.0 ? kf : 0.0;
    kf = kf < (double)D ? kf : (double)D;
    const int k = (int)kf;
    const int pw = y * Wp + (x >> 5);
    const uint32_t bit = 1u << (x & 31);
    if (k < za) atomicXor(&before[pw], bit);
    else if (k < ze) atomicXor(&rows[(k - za) * PW + pw], bit);
    else atomicXor(&after[pw], bit);
  }
}

template <int F64, int THREADS>
__global__ __launch_bounds__(THREADS) void k_mv_parity(const void* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces,
                                                       int n_faces, const int32_t* __restrict__ desc, int slabs, int zs, int halo,
                                                       int D, int H, int W, int words, const uint32_t* surface, uint32_t* bits,
                                                       int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mv_smem[];  // rows [nl * PW], before [PW], after [PW], queue, ints
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int mesh = blockIdx.x / slabs, slab = blockIdx.x - mesh * slabs;
  const int Wp = (W + 31) / 32, PW = H * Wp, V = D * H * W;
  const int za = slab * zs, zb = za + zs < D ? za + zs : D, ze = zb + halo < D ? zb + halo : D;
  const int nl = ze - za;
  uint32_t* const rows = mv_smem;
  uint32_t* const before = rows + (zs + halo) * PW;
  uint32_t* const after = before + PW;
  int* const wave_q = reinterpret_cast<int*>(after + PW);
  int* const extra = wave_q + THREADS;   // [0..1] the queue counts of even and odd chunks, [2..] the sum's scratch
  MvMesh m;
  if (!mv_mesh(desc, mesh, n_verts, n_faces, &m)) return;   // k_mv_surface has reported it
  for (int j = t; j < (zs + halo + 2) * PW; j += THREADS) mv_smem[j] = 0u;
  if (t < 2) extra[t] = 0;
  __syncthreads();

  int chunk = 0;
  for (int base = 0; base < m.fcount; base += THREADS, ++chunk) {
    int* const count = extra + (chunk & 1);
    const int i = base + t;
    if (i < m.fcount) {
      double u[3][3];
      const int fl = mv_face<F64>(verts, faces, m, i, D, H, W, u);
      MvCols c;
      bool neg;
      if (!(fl & (kMvBadIndex | kMvNonFinite)) && mv_cols(u, H, W, &c, &neg)) {
        if (c.ny * c.nx <= kMvLane) mv_cross(u, c, neg, 0, 1, D, Wp, PW, za, ze, rows, before, after);
        else wave_q[atomicAdd(count, 1)] = i;
      }
    }
    __syncthreads();
    if (t == 0) extra[(chunk + 1) & 1] = 0;
    const int n_wave = *count;
    for (int q = wave; q < n_wave; q += THREADS / 64) {
      double u[3][3];
      mv_face<F64>(verts, faces, m, wave_q[q], D, H, W, u);
      MvCols c;
      bool neg;
      mv_cols(u, H, W, &c, &neg);
      mv_cross(u, c, neg, lane, 64, D, Wp, PW, za, ze, rows, before, after);
    }
    __syncthreads();
  }
  // prefix XOR along axis 0; every toggle of a column, the ones at plane D included, tells whether it is open
  int open = 0;
  for (int pw = t; pw < PW; pw += THREADS) {
    uint32_t x = before[pw];
    for (int zl = 0; zl < nl; ++zl) {
      x ^= rows[zl * PW + pw];
      rows[zl * PW + pw] = x;
    }
    open += __popc(x ^ after[pw]);
  }
  __syncthreads();
  const int j0 = (int)(((int64_t)za * H * W + 31) / 32), j1 = zb == D ? words : (int)(((int64_t)zb * H * W + 31) / 32);
  const uint32_t* s = surface + (size_t)mesh * words;
  uint32_t* out = bits + (size_t)mesh * words;
  for (int j = j0 + t; j < j1; j += THREADS) out[j] = s[j] | mv_flat_word(rows, j, za, H, W, Wp, V);
  const int total = block_sum<THREADS, int>(open, extra + 2);
  if (slab == 0 && t == 0) info[2 * (size_t)mesh + 1] = total;
}

// ---------------------------------------------------------------------------------------------------------------------
// carve
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_mv_carve(const uint32_t* __restrict__ in, int slabs, int zs, int halo, int D, int H, int W,
                                                      int words, uint32_t* __restrict__ out_bits) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mv_smem[];  // src [cap * PW], res [cap * PW], before [PW], after [PW]
  const int t = threadIdx.x;
  const int grid = blockIdx.x / slabs, slab = blockIdx.x - grid * slabs;
  const int Wp = (W + 31) / 32, PW = H * Wp, V = D * H * W;
  const int za = slab * zs, zb = za + zs < D ? za + zs : D, ze = zb + halo < D ? zb + halo : D;
  const int nl = ze - za, cap = zs + halo;
  uint32_t* const src = mv_smem;
  uint32_t* const res = src + cap * PW;
  uint32_t* const before = res + cap * PW;
  uint32_t* const after = before + PW;
  const uint32_t* g = in + (size_t)grid * words;

  for (int i = t; i < nl * PW; i += THREADS) {
    const int zl = i / PW, r = i - zl * PW;
    const int y = r / Wp, k = r - y * Wp;
    src[i] = mv_row_word(g, za + zl, y, k, H, W);
  }
  for (int i = t; i < 2 * PW; i += THREADS) before[i] = 0u;
  __syncthreads();
  const int others = (D - nl) * PW;   // the planes before and behind the slab, OR-ed into one plane each
  for (int i = t; i < others; i += THREADS) {
    const int pz = i / PW, r = i - pz * PW;
    const int y = r / Wp, k = r - y * Wp;
    const uint32_t w = mv_row_word(g, pz < za ? pz : ze + (pz - za), y, k, H, W);
    if (w) atomicOr(pz < za ? &before[r] : &after[r], w);
  }
  __syncthreads();
  for (int pw = t; pw < PW; pw += THREADS) {   // axis 0
    uint32_t p = before[pw];
    for (int zl = 0; zl < nl; ++zl) {
      p |= src[zl * PW + pw];
      res[zl * PW + pw] = p;
    }
    uint32_t s = after[pw];
    for (int zl = nl - 1; zl >= 0; --zl) {
      s |= src[zl * PW + pw];
      res[zl * PW + pw] &= s;
    }
  }
  __syncthreads();
  for (int i = t; i < nl * Wp; i += THREADS) {   // axis 1
    const int zl = i / Wp, k = i - zl * Wp;
    const int o = zl * PW + k;
    uint32_t p = 0u;
    for (int y = 0; y < H; ++y) {
      p |= src[o + y * Wp];
      res[o + y * Wp] &= p;
    }
    uint32_t s = 0u;
    for (int y = H - 1; y >= 0; --y) {
      s |= src[o + y * Wp];
      res[o + y * Wp] &= s;
    }
  }
  __syncthreads();
  for (int row = t; row < nl * H; row += THREADS) {   // axis 2: from the row's first set bit to its last
    const int o = row * Wp;
    bool seen = false;
    for (int k = 0; k < Wp; ++k) {
      const uint32_t a = src[o + k];
      res[o + k] &= seen ? ~0u : a ? ~((a & (0u - a)) - 1u) : 0u;
      seen |= a != 0u;
    }
    seen = false;
    for (int k = Wp - 1; k >= 0; --k) {
      const uint32_t a = src[o + k];
      res[o + k] &= seen ? ~0u : a ? (a | (0xffffffffu >> __clz(a))) : 0u;
      seen |= a != 0u;
    }
  }
  __syncthreads();
  const int j0 = (int)(((int64_t)za * H * W + 31) / 32), j1 = zb == D ? words : (int)(((int64_t)zb * H * W + 31) / 32);
  uint32_t* out = out_bits + (size_t)grid * words;
  for (int j = j0 + t; j < j1; j += THREADS) out[j] = mv_flat_word(res, j, za, H, W, Wp, V);
}

template <int F64, int CLS>
int mv_surface_launch(const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc, int meshes,
                      const MvGrid& g, uint32_t* bits, int32_t* info, int32_t* status, hipStream_t st) {
  constexpr int WORDS = kMvWords[CLS], THREADS = kMvThreads[CLS];
  constexpr size_t lds = sizeof(uint32_t) * (WORDS + kMvExtra + 2 * THREADS);
  static_assert(lds <= 80 * 1024, "two workgroups share the CU's 160 KiB of LDS");
  static LdsLimit limit;
  const int rc = set_lds(k_mv_surface<F64, WORDS, THREADS>, lds, limit);
  if (rc != DPC_OK) return rc;
  const int slabs = (g.words + WORDS - 1) / WORDS;
  DPC_LAUNCH("k_mv_surface", dpc_kid("k_mv_surface", F64, WORDS, THREADS), (k_mv_surface<F64, WORDS, THREADS>),
             dim3((unsigned)meshes * (unsigned)slabs), dim3(THREADS), lds, st, verts, n_verts, faces, n_faces, desc, slabs, g.D, g.H,
             g.W, g.words, bits, info, status);
  return launch_ok();
}

template <int F64>
int mv_surface(const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc, int meshes, const MvGrid& g,
               uint32_t* bits, int32_t* info, int32_t* status, hipStream_t st) {
  switch (mv_class(g.words)) {
    case 0: return mv_surface_launch<F64, 0>(verts, n_verts, faces, n_faces, desc, meshes, g, bits, info, status, st);
    case 1: return mv_surface_launch<F64, 1>(verts, n_verts, faces, n_faces, desc, meshes, g, bits, info, status, st);
    default: return mv_surface_launch<F64, 2>(verts, n_verts, faces, n_faces, desc, meshes, g, bits, info, status, st);
  }
}

// 256 threads for a slab of at most 2048 padded words, 1024 above
bool mv_small(const MvGrid& g) { return (g.zs + g.halo) * g.PW <= 2048; }

template <int F64, int THREADS>
int mv_parity_launch(const void* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* desc, int meshes,
                     const MvGrid& g, const uint32_t* surface, uint32_t* bits, int32_t* info, hipStream_t st) {
  const size_t lds = sizeof(uint32_t) * ((size_t)(g.zs + g.halo + 2) * g.PW + THREADS + 2 + THREADS / 64 + 1);
  static LdsLimit limit;
  const int rc = set_lds(k_mv_parity<F64, THREADS>, lds, limit);
  if (rc != DPC_OK) return rc;
  DPC_LAUNCH("k_mv_parity", dpc_kid("k_mv_parity", F64, THREADS), (k_mv_parity<F64, THREADS>),
             dim3((unsigned)meshes * (unsigned)g.slabs), dim3(THREADS), lds, st, verts, n_verts, faces, n_faces, desc, g.slabs, g.zs,
             g.halo, g.D, g.H, g.W, g.words, surface, bits, info);
  return launch_ok();
}

template <int THREADS>
int mv_carve_launch(const uint32_t* in, int B, const MvGrid& g, uint32_t* out, hipStream_t st) {
  const size_t lds = sizeof(uint32_t) * ((size_t)(2 * (g.zs + g.halo) + 2) * g.PW);
  static LdsLimit limit;
  const int rc = set_lds(k_mv_carve<THREADS>, lds, limit);
  if (rc != DPC_OK) return rc;
  DPC_LAUNCH("k_mv_carve", dpc_kid("k_mv_carve", THREADS), (k_mv_carve<THREADS>), dim3((unsigned)B * (unsigned)g.slabs), dim3(THREADS),
             lds, st, in, g.slabs, g.zs, g.halo, g.D, g.H, g.W, g.words, out);
  return launch_ok();
}

int mv_carve(const uint32_t* in, int B, const MvGrid& g, uint32_t* out, hipStream_t st) {
  return mv_small(g) ? mv_carve_launch<256>(in, B, g, out, st) : mv_carve_launch<1024>(in, B, g, out, st);
}

}  // namespace

extern "C" {

int dpc_voxelise_meshes(const void* verts, int n_verts, int is_f64, const int32_t* faces, int n_faces, const int32_t* mesh_desc,
                        const int32_t* host_mesh_desc, int meshes, int D, int H, int W, int fill, uint32_t* bits, uint32_t* scratch,
                        int32_t* info, int32_t* status, void* stream) {
  MvGrid g;
  if (n_verts < 0 || n_faces < 0 || meshes < 0 || !mv_grid(D, H, W, 2, &g)) return DPC_ERR_SHAPE;
  if (fill != DPC_MESH_FILL_NONE && fill != DPC_MESH_FILL_CARVE && fill != DPC_MESH_FILL_PARITY) return DPC_ERR_SHAPE;
  if (meshes > 0 && !host_mesh_desc) return DPC_ERR_NULL;
  const int64_t len[2] = {n_verts, n_faces};
  const int rc = check_desc<4, 2>(host_mesh_desc, meshes, len, INT32_MAX, nullptr, [](const int32_t*) { return true; });
  if (rc != DPC_OK) return rc;
  const int64_t slabs = (g.words + kMvWords[mv_class(g.words)] - 1) / kMvWords[mv_class(g.words)];
  if (meshes * slabs > INT32_MAX || (int64_t)meshes * g.slabs > INT32_MAX) return DPC_ERR_SHAPE;
  if (meshes == 0) return DPC_OK;
  if ((!verts && n_verts > 0) || (!faces && n_faces > 0) || !mesh_desc || !bits || !info ||
      (fill == DPC_MESH_FILL_CARVE && !scratch))
    return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* surface = fill == DPC_MESH_FILL_CARVE ? scratch : bits;
  int r = is_f64 ? mv_surface<1>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, surface, info, status, st)
                 : mv_surface<0>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, surface, info, status, st);
  if (r != DPC_OK || fill == DPC_MESH_FILL_NONE) return r;
  if (fill == DPC_MESH_FILL_CARVE) return mv_carve(surface, meshes, g, bits, st);
  if (mv_small(g))
    return is_f64 ? mv_parity_launch<1, 256>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, bits, bits, info, st)
                  : mv_parity_launch<0, 256>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, bits, bits, info, st);
  return is_f64 ? mv_parity_launch<1, 1024>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, bits, bits, info, st)
                : mv_parity_launch<0, 1024>(verts, n_verts, faces, n_faces, mesh_desc, meshes, g, bits, bits, info, st);
}

int dpc_voxel_carve(const uint32_t* bits, int B, int D, int H, int W, uint32_t* out, void* stream) {
  MvGrid g;
  if (B < 0 || !mv_grid(D, H, W, 1, &g) || (int64_t)B * g.slabs > INT32_MAX) return DPC_ERR_SHAPE;
  if (B == 0) return DPC_OK;
  if (!bits || !out) return DPC_ERR_NULL;
  if (bits == out) return DPC_ERR_SHAPE;   // a slab reads the whole grid while the others write theirs
  return mv_carve(bits, B, g, out, (hipStream_t)stream);
}

}  // extern "C"
