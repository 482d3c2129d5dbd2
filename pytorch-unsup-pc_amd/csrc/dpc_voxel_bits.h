// The bit grid shared by the voxel files (dpc_voxels.hip, dpc_mesh_voxels.hip, dpc_voxel_edt.hip, dpc_winding.hip,
// dpc_surface.hip): voxel f = (d * H + h) * W + w of a D x H x W grid is bit f & 31 of word f >> 5, and the last word's
// bits from V & 31 on are padding (the layout is in include/dpc_render.h, dpc_voxelise).  Host: the side check and the
// grid record every entry point that takes (D, H, W) starts from.  Device: the two reads of a grid that do not trust
// what lies outside it.  A read that assumes its bits lie inside (dpc_mesh_voxels.hip's mv_bits) stays with its file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dpc_render.h"

// min_side <= D, H, W <= DPC_VOXEL_MAX_SIDE
__host__ __device__ constexpr bool voxel_sides_ok(int D, int H, int W, int min_side) {
  return !(D < min_side || H < min_side || W < min_side || D > DPC_VOXEL_MAX_SIDE || H > DPC_VOXEL_MAX_SIDE || W > DPC_VOXEL_MAX_SIDE);
}

struct VoxelGrid {
  int D, H, W, V, words;
};

// min_side is 1, or 2 for an entry point that divides by side - 1
inline bool voxel_grid(int D, int H, int W, int min_side, VoxelGrid* g) {
  if (!voxel_sides_ok(D, H, W, min_side)) return false;
  g->D = D; g->H = H; g->W = W;
  g->V = D * H * W;
  g->words = (g->V + 31) / 32;
  return true;
}

// m, read as word j of a bit grid of V voxels, with its padding bits cleared whatever the caller left there
__device__ inline uint32_t voxel_clear_padding(uint32_t m, int j, int words, int V) {
  if (j == words - 1 && (V & 31)) m &= (1u << (V & 31)) - 1u;
  return m;
}

// word j of the grid without its padding bits; 0 <= j < words
__device__ inline uint32_t voxel_word(const uint32_t* __restrict__ w, int j, int words, int V) {
  return voxel_clear_padding(w[j], j, words, V);
}

// the 32 bits of a grid from bit p on (p may be negative or reach past the last word: those bits read as zero)
__device__ inline uint32_t voxel_window(const uint32_t* __restrict__ w, int words, int p) {
  const int j = p >> 5, s = p & 31;
  const uint32_t lo = (j >= 0 && j < words) ? w[j] : 0u;
  const uint32_t hi = (s != 0 && j + 1 >= 0 && j + 1 < words) ? w[j + 1] : 0u;
  return s ? (lo >> s) | (hi << (32 - s)) : lo;
}
