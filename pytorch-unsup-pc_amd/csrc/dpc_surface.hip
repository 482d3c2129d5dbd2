// Iso-surface extraction: occupancy grids to triangle meshes, for a ragged batch of grids in one call.  The rule (which
// nodes are inside, where a vertex lies, the order of vertices and faces, the triangulation of a cell) is in
// include/dpc_render.h (dpc_surface_count); the triangulation table is the generated dpc_surface_table.h.  Everything is
// exact: the vertex coordinate is one fp64 subtraction pair, one division and one addition, nothing fused.
//
// A grid's nodes are cut into tiles of kSfTile consecutive flat indices; vertices (key 3*f + a) and faces (corner 0 at f)
// both come in ascending f, so a tile's outputs are one contiguous range each and an ordered scan over the tiles places
// them.  A workgroup of 256 threads takes its tile in kSfRounds rounds of 256 nodes, thread t node 256*r + t: every load
// of a round is coalesced, and a node's seven neighbours are lines that this or a neighbouring workgroup has just read.
// A neighbour that does not exist is loaded as the node itself (offset 0), so no load sits behind a branch, and
// k_surface_tiles, _verts and _faces issue every load of their tile before the first is used.
//
// k_surface_tiles<F64>   per tile: the crossing edges its nodes own and the table triangles of the cells whose corner 0
//                        they are -> tiles[b][tile] = (vertices, faces)
// k_surface_scan         one workgroup per grid: exclusive scan of its tiles' pairs in place; the totals go to counts[b]
//                        (count pass), or are compared with the grid's out_desc row -> ok[b] (extract pass)
// k_surface_verts<F64>   per tile: block_scan of the nodes' vertex counts, the vertices, and for every node
//                        map[f] = local id of its first vertex << 4 | inside << 3 | its three crossing bits
// k_surface_faces        per tile: the case of each cell from the eight map entries of its corners, block_scan of the
//                        triangle counts, the faces; the vertex of cell edge (a, j) is the map entry of the corner that
//                        owns it: id + popcount(crossing bits below a)
// Nothing waits on another workgroup; every loop is bounded by a host-checked size or a checked table entry.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "../../include/dpc_render.h"
#include "dpc_batch.h"
#undef DPC_LAUNCH_TWICE  // the timing experiment of dpc_profile.h is for idempotent kernels only; k_surface_scan is not one
#include "dpc_launch.h"
#include "dpc_surface_table.h"

namespace {

constexpr int kSfThreads = 256;
constexpr int kSfRounds = 4;
constexpr int kSfTile = kSfThreads * kSfRounds;  // nodes of a workgroup
static_assert((int64_t)DPC_VOXEL_MAX_SIDE * DPC_VOXEL_MAX_SIDE * DPC_VOXEL_MAX_SIDE * 3 < (1 << 27), "a local vertex id fits 27 bits of a map entry");

struct SfGrid {
  int start, D, H, W, V, tiles;
};

// f / n and f % n for 0 <= f < 2^21 and 1 <= n <= DPC_VOXEL_MAX_SIDE without an integer division: the float product is
// within one of the quotient (f is exact in a float, the relative error of rcp and of the product is below 2^-22), and the
// remainder says which way
__device__ inline int sf_div(int f, int n, float rcp, int* rem) {
  int q = (int)((float)f * rcp);
  int r = f - q * n;
  if (r < 0) { --q; r += n; }
  else if (r >= n) { ++q; r -= n; }
  *rem = r;
  return q;
}

// (d, h, w) of the flat index f
__device__ inline void sf_dhw(const SfGrid& g, int f, int* d, int* h, int* w) {
  const int q = sf_div(f, g.W, 1.0f / (float)g.W, w);
  *d = sf_div(q, g.H, 1.0f / (float)g.H, h);
}

// a row (first node, D, H, W) of the grid table against the packed buffer of n_values nodes
__host__ __device__ inline bool sf_grid(const int32_t* row, int n_values, SfGrid* g) {
  const int start = row[0], D = row[1], H = row[2], W = row[3];
  if (start < 0 || D < 1 || H < 1 || W < 1 || D > DPC_VOXEL_MAX_SIDE || H > DPC_VOXEL_MAX_SIDE || W > DPC_VOXEL_MAX_SIDE) return false;
  const int V = D * H * W;
  if ((int64_t)start + V > n_values) return false;
  g->start = start; g->D = D; g->H = H; g->W = W; g->V = V;
  g->tiles = (V + kSfTile - 1) / kSfTile;
  return true;
}

// workspace: tiles[B][max_tiles][2], ok[B], map[n_values]
struct SfWork {
  int32_t* tiles;
  int32_t* ok;
  int32_t* map;
};

size_t sf_carve(char* base, int B, int max_tiles, int n_values, SfWork* w) {
  Carver c{base};
  int32_t* tiles = c.take<int32_t>(2 * (size_t)B * max_tiles);
  int32_t* ok = c.take<int32_t>((size_t)B);
  int32_t* map = c.take<int32_t>((size_t)n_values);
  if (w) *w = SfWork{tiles, ok, map};
  return c.off;
}

// host check of the grid table: DPC_OK with the largest tile count, or DPC_ERR_SHAPE
int sf_check_grids(const int32_t* host_grid_desc, int B, int n_values, int* max_tiles) {
  int mt = 0;
  int64_t end = 0;
  for (int b = 0; b < B; ++b) {  // the grids ascend without overlap: a node has one map entry
    SfGrid g;
    if (!sf_grid(host_grid_desc + 4 * (int64_t)b, n_values, &g) || g.start < end) return DPC_ERR_SHAPE;
    end = (int64_t)g.start + g.V;
    if (g.tiles > mt) mt = g.tiles;
  }
  *max_tiles = mt;
  return DPC_OK;
}

// Where node f sits: its coordinates and the offsets to its successor on each axis, 0 where it has none, so that
// f + (any sum of the offsets) is always a node of the grid and a load from it needs no branch.
struct SfPlace {
  int d, h, w, od, oh, ow;
};
__device__ inline SfPlace sf_place(const SfGrid& g, int f) {
  SfPlace p;
  sf_dhw(g, f, &p.d, &p.h, &p.w);
  p.od = p.d + 1 < g.D ? g.H * g.W : 0;
  p.oh = p.h + 1 < g.H ? g.W : 0;
  p.ow = p.w + 1 < g.W ? 1 : 0;
  return p;
}

template <int F64>
__global__ __launch_bounds__(kSfThreads) void k_surface_tiles(const void* __restrict__ values_, int n_values,
                                                              const int32_t* __restrict__ grid_desc, int B, int max_tiles,
                                                              const double* __restrict__ iso_, int32_t* __restrict__ tiles,
                                                              int32_t* __restrict__ status) {
  using T = std::conditional_t<F64 != 0, double, float>;
  __shared__ int8_t tri_count[256];
  __shared__ int sums[2][kSfThreads / 64];
  const int t = threadIdx.x;
  tri_count[t] = kDpcSurfaceTable[t][0];
  __syncthreads();
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // the same trip count in every thread: the loop has barriers
    SfGrid g;
    // nothing of the device table becomes an address or a loop bound before it passed this
    const bool ok = sf_grid(grid_desc + 4 * (size_t)b, n_values, &g) && g.tiles <= max_tiles;
    if (!ok) {
      if (blockIdx.x == 0 && t == 0 && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
      continue;
    }
    if ((int)blockIdx.x >= g.tiles) continue;
    const T* __restrict__ vals = static_cast<const T*>(values_) + g.start;
    const double iso = iso_[b];
    int nv = 0, nt = 0;
    // every load of the tile is issued before the first is used: the loads of a round do not wait for the round before
    T v[kSfRounds][8];
    SfPlace pl[kSfRounds];
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int f = (int)blockIdx.x * kSfTile + r * kSfThreads + t;
      const int fc = f < g.V ? f : g.V - 1;
      pl[r] = sf_place(g, fc);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[r][k] = vals[fc + (k >> 2) * pl[r].od + (k >> 1 & 1) * pl[r].oh + (k & 1) * pl[r].ow];
    }
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int f = (int)blockIdx.x * kSfTile + r * kSfThreads + t;
      if (f < g.V) {
        int c = 0;  // corner k = 4*dd + 2*dh + dw
#pragma unroll
        for (int k = 0; k < 8; ++k) c |= ((double)v[r][k] > iso) << k;  // false for a NaN
        const int in0 = c & 1;
        nv += (pl[r].od && (c >> 4 & 1) != in0) + (pl[r].oh && (c >> 2 & 1) != in0) + (pl[r].ow && (c >> 1 & 1) != in0);
        if (pl[r].od && pl[r].oh && pl[r].ow) nt += tri_count[c];
      }
    }
    __syncthreads();  // the sums of the previous grid are read
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      nv += __shfl_down(nv, off, 64);
      nt += __shfl_down(nt, off, 64);
    }
    if ((t & 63) == 0) { sums[0][t >> 6] = nv; sums[1][t >> 6] = nt; }
    __syncthreads();
    if (t < 2) {
      int s = 0;
      for (int w = 0; w < kSfThreads / 64; ++w) s += sums[t][w];
      tiles[2 * ((size_t)b * max_tiles + blockIdx.x) + t] = s;
    }
  }
}

// out_desc row (first vertex, vertices, first face, faces) against the output buffers
__host__ __device__ inline bool sf_out_row(const int32_t* row, int n_verts, int n_faces) {
  return row[0] >= 0 && row[1] >= 0 && (int64_t)row[0] + row[1] <= n_verts && row[2] >= 0 && row[3] >= 0 &&
         (int64_t)row[2] + row[3] <= n_faces;
}

// It scans the tile sums in place, so it is not idempotent: launched twice (DPC_LAUNCH_TWICE of dpc_profile.h) it would
// scan the offsets again, which is why this file switches that experiment off above.
__global__ __launch_bounds__(kSfThreads) void k_surface_scan(const int32_t* __restrict__ grid_desc, int n_values, int max_tiles,
                                                             int32_t* __restrict__ tiles, int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ out_desc, int n_verts, int n_faces,
                                                             int32_t* __restrict__ ok, int32_t* __restrict__ status) {
  __shared__ int scratch[kSfThreads / 64 + 1];
  const int t = threadIdx.x, b = blockIdx.x;
  SfGrid g;
  if (!(sf_grid(grid_desc + 4 * (size_t)b, n_values, &g) && g.tiles <= max_tiles)) {  // k_surface_tiles has flagged it
    if (t == 0) {
      if (counts) { counts[2 * (size_t)b] = 0; counts[2 * (size_t)b + 1] = 0; }
      if (ok) ok[b] = 0;
    }
    return;
  }
  int32_t* row = tiles + 2 * (size_t)b * max_tiles;
  int base_v = 0, base_t = 0;
  for (int j0 = 0; j0 < g.tiles; j0 += kSfThreads) {  // the same trip count in every thread: block_scan has barriers
    const int j = j0 + t;
    const int nv = j < g.tiles ? row[2 * j] : 0, nt = j < g.tiles ? row[2 * j + 1] : 0;
    int ev, et;
    const int tv = block_scan<kSfThreads>(nv, &ev, scratch);
    const int tt = block_scan<kSfThreads>(nt, &et, scratch);
    if (j < g.tiles) { row[2 * j] = base_v + ev; row[2 * j + 1] = base_t + et; }
    base_v += tv;
    base_t += tt;
  }
  if (t == 0) {
    if (counts) { counts[2 * (size_t)b] = base_v; counts[2 * (size_t)b + 1] = base_t; }
    if (ok) {
      const int32_t* o = out_desc + 4 * (size_t)b;
      const bool good = sf_out_row(o, n_verts, n_faces) && o[1] == base_v && o[3] == base_t;  // the table is this grid's counts
      ok[b] = good;
      if (!good && status) atomicOr(status, (int)DPC_STATUS_BAD_INDEX);
    }
  }
}

template <int F64>
__global__ __launch_bounds__(kSfThreads) void k_surface_verts(const void* __restrict__ values_, int n_values,
                                                              const int32_t* __restrict__ grid_desc, int B, int max_tiles,
                                                              const double* __restrict__ iso_, const int32_t* __restrict__ tiles,
                                                              const int32_t* __restrict__ ok, const int32_t* __restrict__ out_desc,
                                                              double* __restrict__ verts, int32_t* __restrict__ map,
                                                              int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  using T = std::conditional_t<F64 != 0, double, float>;
  __shared__ int scratch[kSfThreads / 64 + 1];
  const int t = threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // the same trip count in every thread: block_scan has barriers
    SfGrid g;
    if (!ok[b] || !sf_grid(grid_desc + 4 * (size_t)b, n_values, &g) || (int)blockIdx.x >= g.tiles || g.tiles > max_tiles) continue;
    const T* __restrict__ vals = static_cast<const T*>(values_) + g.start;
    int32_t* __restrict__ gmap = map + g.start;
    const double iso = iso_[b];
    const int v_start = out_desc[4 * (size_t)b], v_count = out_desc[4 * (size_t)b + 1];
    int base = tiles[2 * ((size_t)b * max_tiles + blockIdx.x)];
    bool bad = false;
    // every load of the tile is issued before the first is used
    T v[kSfRounds][4];  // the node, then its successors on axes 0, 1, 2 (the node again where there is none)
    SfPlace pl[kSfRounds];
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int f = (int)blockIdx.x * kSfTile + r * kSfThreads + t;
      const int fc = f < g.V ? f : g.V - 1;
      pl[r] = sf_place(g, fc);
      v[r][0] = vals[fc];
      v[r][1] = vals[fc + pl[r].od];
      v[r][2] = vals[fc + pl[r].oh];
      v[r][3] = vals[fc + pl[r].ow];
    }
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int f = (int)blockIdx.x * kSfTile + r * kSfThreads + t;
      const double va = (double)v[r][0];
      const bool in = va > iso;  // false for a NaN
      int m = 0;
      if (f < g.V) {
        m = in ? 8 : 0;
        if (pl[r].od && ((double)v[r][1] > iso) != in) m |= 1;
        if (pl[r].oh && ((double)v[r][2] > iso) != in) m |= 2;
        if (pl[r].ow && ((double)v[r][3] > iso) != in) m |= 4;
      }
      int excl;
      const int total = block_scan<kSfThreads>((int)__popc(m & 7), &excl, scratch);
      int id = base + excl;
      if (f < g.V) gmap[f] = (id << 4) | m;
      if (m & 7) {
        const int d = pl[r].d, h = pl[r].h, w = pl[r].w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (m >> a & 1) {
            const double vb = (double)v[r][1 + a];
            bad |= !(__builtin_isfinite(va) && __builtin_isfinite(vb));
            const double tt = (iso - va) / (vb - va);
            if (id < v_count) {  // a vertex beyond the range the table gives this grid is not written
              double* p = verts + 3 * ((size_t)v_start + id);
              p[0] = a == 0 ? (double)d + tt : (double)d;
              p[1] = a == 1 ? (double)h + tt : (double)h;
              p[2] = a == 2 ? (double)w + tt : (double)w;
            }
            ++id;
          }
        }
      }
      base += total;
    }
    if (bad && status) atomicOr(status, (int)DPC_STATUS_NONFINITE);
  }
}

__global__ __launch_bounds__(kSfThreads) void k_surface_faces(const int32_t* __restrict__ grid_desc, int n_values, int B, int max_tiles,
                                                              const int32_t* __restrict__ tiles, const int32_t* __restrict__ ok,
                                                              const int32_t* __restrict__ out_desc, const int32_t* __restrict__ map,
                                                              int32_t* __restrict__ faces) {
  __shared__ int8_t table[256][16];
  __shared__ int scratch[kSfThreads / 64 + 1];
  const int t = threadIdx.x;
  for (int i = t; i < 256 * 16; i += kSfThreads) (&table[0][0])[i] = (&kDpcSurfaceTable[0][0])[i];
  __syncthreads();
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // the same trip count in every thread: block_scan has barriers
    SfGrid g;
    if (!ok[b] || !sf_grid(grid_desc + 4 * (size_t)b, n_values, &g) || (int)blockIdx.x >= g.tiles || g.tiles > max_tiles) continue;
    if (g.D < 2 || g.H < 2 || g.W < 2) continue;  // no cell
    const int32_t* __restrict__ gmap = map + g.start;
    const int f_start = out_desc[4 * (size_t)b + 2], f_count = out_desc[4 * (size_t)b + 3];
    int base = tiles[2 * ((size_t)b * max_tiles + blockIdx.x) + 1];
    // every load of the tile is issued before the first is used
    int mm[kSfRounds][8];
    bool cell[kSfRounds];
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int f = (int)blockIdx.x * kSfTile + r * kSfThreads + t;
      const int fc = f < g.V ? f : g.V - 1;
      const SfPlace pl = sf_place(g, fc);
      cell[r] = f < g.V && pl.od && pl.oh && pl.ow;
#pragma unroll
      for (int k = 0; k < 8; ++k) mm[r][k] = gmap[fc + (k >> 2) * pl.od + (k >> 1 & 1) * pl.oh + (k & 1) * pl.ow];
    }
#pragma unroll
    for (int r = 0; r < kSfRounds; ++r) {
      const int* m = mm[r];
      int c = 0;
      if (cell[r]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) c |= (m[k] >> 3 & 1) << k;
      }
      const int n = table[c][0];
      int excl;
      const int total = block_scan<kSfThreads>(n, &excl, scratch);
      int o = base + excl;
      for (int i = 0; i < n; ++i, ++o) {
        if (o >= f_count) break;  // a face beyond the range the table gives this grid is not written
        int32_t* p = faces + 3 * ((size_t)f_start + o);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int e = table[c][1 + 3 * i + j];
          const int a = e >> 2, u = e & 3;  // the edge runs along a from the corner at (u & 1, u >> 1) on the other two axes
          const int k = a == 0 ? ((u & 1) << 1 | (u >> 1)) : a == 1 ? ((u & 1) << 2 | (u >> 1)) : ((u & 1) << 2 | (u >> 1) << 1);
          int mk = m[0];
#pragma unroll
          for (int kk = 1; kk < 7; ++kk) mk = k == kk ? m[kk] : mk;  // corner 7 owns no edge of the cell
          p[j] = (mk >> 4) + __popc(mk & ((1 << a) - 1));
        }
      }
      base += total;
    }
  }
}

// the checks both passes share; DPC_OK with B == 0 means there is nothing to do
int sf_check(int n_values, int is_f64, const int32_t* host_grid_desc, int B, int* max_tiles) {
  if (n_values < 0 || B < 0 || (is_f64 != 0 && is_f64 != 1)) return DPC_ERR_SHAPE;
  if (B > 0 && !host_grid_desc) return DPC_ERR_NULL;
  return sf_check_grids(host_grid_desc, B, n_values, max_tiles);
}

template <int F64>
void sf_launch_tiles(const void* values, int n_values, const int32_t* grid_desc, int B, int max_tiles, const double* iso,
                     int32_t* tiles, int32_t* status, hipStream_t st) {
  const dim3 grid((unsigned)max_tiles, (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_surface_tiles", dpc_kid("k_surface_tiles", F64), (k_surface_tiles<F64>), grid, dim3(kSfThreads), 0, st, values,
             n_values, grid_desc, B, max_tiles, iso, tiles, status);
}

template <int F64>
void sf_launch_verts(const void* values, int n_values, const int32_t* grid_desc, int B, int max_tiles, const double* iso,
                     const SfWork& w, const int32_t* out_desc, double* verts, int32_t* status, hipStream_t st) {
  const dim3 grid((unsigned)max_tiles, (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_surface_verts", dpc_kid("k_surface_verts", F64), (k_surface_verts<F64>), grid, dim3(kSfThreads), 0, st, values,
             n_values, grid_desc, B, max_tiles, iso, w.tiles, w.ok, out_desc, verts, w.map, status);
}

}  // namespace

extern "C" {

size_t dpc_surface_workspace_bytes(const int32_t* host_grid_desc, int B, int n_values) {
  int max_tiles = 0;
  if (n_values < 0 || B <= 0 || !host_grid_desc || sf_check_grids(host_grid_desc, B, n_values, &max_tiles) != DPC_OK) return 0;
  return sf_carve(nullptr, B, max_tiles, n_values, nullptr);
}

int dpc_surface_count(const void* values, int n_values, int is_f64, const int32_t* grid_desc, const int32_t* host_grid_desc, int B,
                      const double* iso, int32_t* counts, void* workspace, int32_t* status, void* stream) {
  int max_tiles = 0;
  const int rc = sf_check(n_values, is_f64, host_grid_desc, B, &max_tiles);
  if (rc != DPC_OK) return rc;
  if (B == 0) return DPC_OK;
  if (!values || !grid_desc || !iso || !counts || !workspace) return DPC_ERR_NULL;
  SfWork w;
  sf_carve(static_cast<char*>(workspace), B, max_tiles, n_values, &w);
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) sf_launch_tiles<1>(values, n_values, grid_desc, B, max_tiles, iso, w.tiles, status, st);
  else sf_launch_tiles<0>(values, n_values, grid_desc, B, max_tiles, iso, w.tiles, status, st);
  DPC_LAUNCH("k_surface_scan", dpc_kid("k_surface_scan"), k_surface_scan, dim3((unsigned)B), dim3(kSfThreads), 0, st, grid_desc,
             n_values, max_tiles, w.tiles, counts, (const int32_t*)nullptr, 0, 0, (int32_t*)nullptr, status);
  return launch_ok();
}

int dpc_surface_extract(const void* values, int n_values, int is_f64, const int32_t* grid_desc, const int32_t* host_grid_desc,
                        int B, const double* iso, const int32_t* out_desc, const int32_t* host_out_desc, int n_verts, int n_faces,
                        double* verts, int32_t* faces, void* workspace, int32_t* status, void* stream) {
  int max_tiles = 0;
  const int rc = sf_check(n_values, is_f64, host_grid_desc, B, &max_tiles);
  if (rc != DPC_OK) return rc;
  if (n_verts < 0 || n_faces < 0) return DPC_ERR_SHAPE;
  if (B > 0 && !host_out_desc) return DPC_ERR_NULL;
  int64_t v_end = 0, f_end = 0;
  for (int b = 0; b < B; ++b) {  // output ranges ascend without overlap, inside the buffers, none longer than a grid can fill
    const int32_t* o = host_out_desc + 4 * (int64_t)b;
    const int32_t* gr = host_grid_desc + 4 * (int64_t)b;
    const int64_t V = (int64_t)gr[1] * gr[2] * gr[3], cells = (int64_t)(gr[1] - 1) * (gr[2] - 1) * (gr[3] - 1);
    if (!sf_out_row(o, n_verts, n_faces) || o[0] < v_end || o[2] < f_end || o[1] > 3 * V || o[3] > DPC_SURFACE_MAX_TRIANGLES * cells)
      return DPC_ERR_SHAPE;
    v_end = (int64_t)o[0] + o[1];
    f_end = (int64_t)o[2] + o[3];
  }
  if (B == 0) return DPC_OK;
  if (!values || !grid_desc || !iso || !out_desc || !workspace || (!verts && n_verts > 0) || (!faces && n_faces > 0)) return DPC_ERR_NULL;
  SfWork w;
  sf_carve(static_cast<char*>(workspace), B, max_tiles, n_values, &w);
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) sf_launch_tiles<1>(values, n_values, grid_desc, B, max_tiles, iso, w.tiles, status, st);
  else sf_launch_tiles<0>(values, n_values, grid_desc, B, max_tiles, iso, w.tiles, status, st);
  DPC_LAUNCH("k_surface_scan", dpc_kid("k_surface_scan"), k_surface_scan, dim3((unsigned)B), dim3(kSfThreads), 0, st, grid_desc,
             n_values, max_tiles, w.tiles, (int32_t*)nullptr, out_desc, n_verts, n_faces, w.ok, status);
  if (is_f64) sf_launch_verts<1>(values, n_values, grid_desc, B, max_tiles, iso, w, out_desc, verts, status, st);
  else sf_launch_verts<0>(values, n_values, grid_desc, B, max_tiles, iso, w, out_desc, verts, status, st);
  const dim3 grid((unsigned)max_tiles, (unsigned)(B < 65535 ? B : 65535));
  DPC_LAUNCH("k_surface_faces", dpc_kid("k_surface_faces"), k_surface_faces, grid, dim3(kSfThreads), 0, st, grid_desc, n_values, B,
             max_tiles, w.tiles, w.ok, out_desc, w.map, faces);
  return launch_ok();
}

}  // extern "C"
