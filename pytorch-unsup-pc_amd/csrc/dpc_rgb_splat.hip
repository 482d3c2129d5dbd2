// Colour splat: per-point RGB splatted with the points' trilinear weights into a planar colour grid, and its gather backward.
//   C_raw[b, c, iz+k, iy+j, ix+i] += wz[k] wy[j] wx[i] colour(b,n)[c]                 point_cloud.py:98-118
// One forward body and one backward body (rgb_splat_body, rgb_splat_bwd_body) serve two routes; a policy says where a
// point's colour lives and how a sum is kept:
//   OwnColours  k_rgb_splat, k_rgb_splat_bwd: rgb [B,N,3], a row per point.  fp32 hardware atomics into a zeroed grid: the
//               sums depend on the order the adds arrive in, so the grid is not bit-reproducible from run to run.
//   ColourSets  k_rgb_splat_fixed, k_rgb_splat_fixed_bwd, the converter k_rgb_fixed_to_float (cfg.pc_rgb_deterministic): the
//               colour of point i of cloud b is rgb[b / R][point_index ? point_index[b][i] : i] (DpcParams.point_replicas /
//               point_index, the occupancy path's convention), so the decoder's [B/R,N_set,3] colours serve every view and
//               every dropout row without a [B,n,3] copy.  Each contribution is rounded once to 64-bit fixed point with 40
//               fractional bits (grad_to_fixed, dpc_kernels.h) and added as an integer.  Integer adds commute, so a voxel's
//               sum is the same bits in whatever order its adds arrive, and with it everything computed from the colour
//               grid; the sets' gradients are summed the same way (the dpc_fixed pattern of dpc_slab_bwd.hip).
// The arithmetic of every contribution and every gradient formula is the bodies': the same in both routes.
// Design notes: DESIGN.md section 4.
#include "dpc_colour_column.h"

namespace dpck {
namespace {

constexpr int kSplatThreads = 256;

inline unsigned splat_blocks(size_t total) {
  const size_t b = (total + kSplatThreads - 1) / kSplatThreads;
  return (unsigned)(b < 1 ? 1 : (b > 1048576 ? 1048576 : b));
}

// Largest colour magnitude the fixed-point splat accepts.  A contribution is w * c with 0 <= w <= 1 (fp32 products of factors
// <= 1 never round upwards past their larger operand), so |contribution| <= kRgbFixMax and its fixed-point value is at most
// kRgbFixMax * 2^40 in magnitude; a voxel receives at most one contribution per point of the cloud, N <= DPC_MAX_POINTS.
constexpr float kRgbFixMax = 8.0f;
static_assert((double)kRgbFixMax * (double)DPC_MAX_POINTS * kGradFixScale < 9223372036854775808.0,
              "8 * (2^20 - 1) * 2^40 < 2^63: no accepted input can wrap a voxel's 64-bit sum");
constexpr float kFixToFloat = 1.0f / 1099511627776.0f;   // 2^-40, exact

// The stored colour row of point n of cloud b (the index inside its colour set), -1 for a point_index entry outside
// [0, n_set): such an entry never becomes an address.
__device__ inline int colour_row(const DpcParams& P, size_t pt, int n, int n_set) {
  if (P.point_index == nullptr) return n;
  const int src = P.point_index[pt];
  return (unsigned)src < (unsigned)n_set ? src : -1;
}

// A lane's first element and its stride in a grid-stride loop.  The shells take them (GRID_LANES), not the bodies: blockDim
// read in a __global__ function is one scalar load; read in a device function it is lowered before the function is inlined,
// without the kernel's uniform-workgroup fold, and costs a vector load, a compare and a select more per kernel.
struct Lanes {
  size_t first, step;
};
#define GRID_LANES Lanes{(size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x}

struct OwnColours {
  static constexpr bool kSets = false;
  const float* __restrict__ rgb;    // [B,N,3]
  float* __restrict__ sums;         // forward: the grid [B,3,D,H,W], zeroed
};

struct ColourSets {
  static constexpr bool kSets = true;
  const float* __restrict__ rgb;                // [B/R,n_set,3]
  unsigned long long* __restrict__ sums;        // zeroed 64-bit sums: the grid's (forward), the sets' gradients' | nullptr (backward)
  unsigned int* __restrict__ poison;            // zeroed words behind them: one per cloud (forward), one per set (backward)
  int n_set, reps;
  __device__ ColourSets(const DpcParams& P, const float* rgb_, int n_set_, unsigned long long* sums_, unsigned int* poison_)
      : rgb(rgb_), sums(sums_), poison(poison_), n_set(n_set_), reps(P.point_replicas > 1 ? P.point_replicas : 1) {}
};

// ------------------------------------------------------------------------------------------------------
// Forward.  Two neighbouring lanes per (cloud, channel, point), the point index next fastest: the pair owns the two x
// corners, which are neighbours in memory (8 bytes of an fp32 plane, 16 of a 64-bit one), so each of a wave's four atomic
// instructions leaves as 32 two-element requests instead of 64 single ones (scattered float atomics are bound by requests,
// MI355X_MICROARCH.md "Global float atomics").  The cell and the weights are those of the occupancy splat (make_record /
// cell_from_record, corners past the grid dropped).
// ColourSets: a colour that is not a finite number of magnitude <= kRgbFixMax, or a point_index entry outside its set, adds
// nothing and sets its cloud's poison word.
// ------------------------------------------------------------------------------------------------------
template <class Colours>
__device__ __forceinline__ void rgb_splat_body(const DpcParams& P, const float* __restrict__ tr, const Colours& cs, const Lanes ln) {
  const int D = P.D, H = P.H, W = P.W;
  const size_t total = (size_t)P.B * 3 * P.N * 2;
  for (size_t i = ln.first; i < total; i += ln.step) {
    const int e = (int)(i & 1);
    const size_t h = i >> 1;
    const int n = (int)(h % P.N);
    const size_t bc = h / P.N;
    const int c = (int)(bc % 3);
    const size_t b = bc / 3;
    const size_t pt = b * P.N + n;
    int src = n;   // the point's row inside its cloud's colours
    if constexpr (Colours::kSets) {
      src = colour_row(P, pt, n, cs.n_set);
      if (src < 0) {   // every lane of the point sees it; one of them reports
        if (c == 0 && e == 0) {
          atomicOr(cs.poison + b, 1u);
          if (P.status != nullptr) atomicOr(P.status, (int)DPC_STATUS_BAD_INDEX);
        }
        continue;
      }
    }
    const Cell cl = cell_from_record(make_record((double)tr[3 * pt], (double)tr[3 * pt + 1], (double)tr[3 * pt + 2], D, H, W));
    if (!cl.valid || cl.ix + e >= W) continue;
    size_t row = pt;
    if constexpr (Colours::kSets) row = (b / cs.reps) * cs.n_set + src;
    const float col = cs.rgb[3 * row + c];
    if constexpr (Colours::kSets) {
      if (!(fabsf(col) <= kRgbFixMax)) {   // too large, Inf, or NaN (which fails the comparison)
        atomicOr(cs.poison + b, 1u);
        continue;
      }
    }
    const float wc = (e ? cl.wx[1] : cl.wx[0]) * col;
    auto* plane = cs.sums + bc * D * H * W + cl.ix + e;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool ok = (cl.iz + k < D) && (cl.iy + j < H);
        if (ok) {
          auto* at = plane + ((size_t)(cl.iz + k) * H + cl.iy + j) * W;
          const float v = cl.wz[k] * cl.wy[j] * wc;
          if constexpr (Colours::kSets) atomicAdd(at, grad_to_fixed(v)); else atomicAdd(at, v);
        }
      }
  }
}

// ------------------------------------------------------------------------------------------------------
// Backward: one lane per (cloud, point) gathers its 8 corners from the three planes of dC.
//   drgb_c = sum_corners w dC_c;   dtr = k_splat_bwd's formula (dpc_stages.hip) on g[corner] = sum_c colour_c dC_c[corner]
// dtr == nullptr: pc_rgb_stop_points_gradient (point_cloud.py:112-113).  Points outside the cube get exact zeros.
// drgb: direct stores when every point owns its colour row (OwnColours, or ColourSets without sums); otherwise 64-bit
// fixed-point adds into sums [B/R,n_set,3] under grad_fits_fixed's bound, a set's poison word for a contribution beyond it
// (or for an index outside the set).  Repeated indices of a point_index row are just more integer adds.
// ------------------------------------------------------------------------------------------------------
template <class Colours>
__device__ __forceinline__ void rgb_splat_bwd_body(const DpcParams& P, const float* __restrict__ tr,
                                                   const float* __restrict__ dC, float* __restrict__ drgb,
                                                   float* __restrict__ dtr, const Colours& cs, const Lanes ln) {
  const int D = P.D, H = P.H, W = P.W;
  const size_t total = (size_t)P.B * P.N, plane = (size_t)D * H * W;
  for (size_t i = ln.first; i < total; i += ln.step) {
    const size_t b = i / P.N;
    size_t row = i;
    int src = 0;
    if constexpr (Colours::kSets) {
      src = colour_row(P, i, (int)(i - b * P.N), cs.n_set);
      row = (b / cs.reps) * cs.n_set + (src < 0 ? 0 : src);
    }
    const Cell c = cell_from_record(make_record((double)tr[3 * i], (double)tr[3 * i + 1], (double)tr[3 * i + 2], D, H, W));
    float dcol[3] = {0.f, 0.f, 0.f};
    float dZ = 0.f, dY = 0.f, dX = 0.f;
    if (c.valid && src >= 0) {
      const float col[3] = {cs.rgb[3 * row], cs.rgb[3 * row + 1], cs.rgb[3 * row + 2]};
      const float* gb = dC + b * 3 * plane;
      float cv[2][2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const bool ok = (c.iz + k < D) && (c.iy + j < H) && (c.ix + e < W);
            const size_t at = ((size_t)(c.iz + k) * H + c.iy + j) * W + c.ix + e;
            const float w = c.wz[k] * c.wy[j] * c.wx[e];
            float g = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float d = ok ? gb[ch * plane + at] : 0.f;
              dcol[ch] = fmaf(w, d, dcol[ch]);
              g = fmaf(col[ch], d, g);
            }
            cv[k][j][e] = g;
          }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          dZ += (cv[1][a][e] - cv[0][a][e]) * c.wy[a] * c.wx[e];
          dY += (cv[a][1][e] - cv[a][0][e]) * c.wz[a] * c.wx[e];
          dX += (cv[a][e][1] - cv[a][e][0]) * c.wz[a] * c.wy[e];
        }
      dZ *= (float)(D - 1); dY *= (float)(H - 1); dX *= (float)(W - 1);
    }
    bool owned = true;   // point i owns row i of drgb
    if constexpr (Colours::kSets) owned = cs.sums == nullptr;   // launch-uniform
    if (owned) {
      drgb[3 * i] = dcol[0]; drgb[3 * i + 1] = dcol[1]; drgb[3 * i + 2] = dcol[2];
    } else if constexpr (Colours::kSets) {
      if (src < 0) {
        atomicOr(cs.poison + b / cs.reps, 1u);
        if (P.status != nullptr) atomicOr(P.status, (int)DPC_STATUS_BAD_INDEX);
      } else if (c.valid) {   // a point outside the cube contributes exact zeros: nothing to add
        if (grad_fits_fixed(dcol[0], dcol[1], dcol[2])) {
          unsigned long long* a = cs.sums + 3 * row;
          atomicAdd(a + 0, grad_to_fixed(dcol[0])); atomicAdd(a + 1, grad_to_fixed(dcol[1])); atomicAdd(a + 2, grad_to_fixed(dcol[2]));
        } else {   // NaN / Inf / out of range: the set's gradient becomes NaN (dpc_kernels.h, grad_fits_fixed)
          atomicOr(cs.poison + b / cs.reps, 1u);
        }
      }
    }
    if (dtr != nullptr) { dtr[3 * i] = dZ; dtr[3 * i + 1] = dY; dtr[3 * i + 2] = dX; }
  }
}

// ------------------------------------------------------------------------------------------------------
// The kernels: shells around the two bodies
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSplatThreads) void k_rgb_splat(DpcParams P, const float* __restrict__ tr,
                                                             const float* __restrict__ rgb, float* __restrict__ out) {
  rgb_splat_body(P, tr, OwnColours{rgb, out}, GRID_LANES);
}

__global__ __launch_bounds__(kSplatThreads) void k_rgb_splat_bwd(DpcParams P, const float* __restrict__ tr,
                                                                 const float* __restrict__ rgb, const float* __restrict__ dC,
                                                                 float* __restrict__ drgb, float* __restrict__ dtr) {
  rgb_splat_bwd_body(P, tr, dC, drgb, dtr, OwnColours{rgb, nullptr}, GRID_LANES);
}

// acc [B,3,D,H,W] zeroed 64-bit sums, poison [B] zeroed words behind them
__global__ __launch_bounds__(kSplatThreads) void k_rgb_splat_fixed(DpcParams P, const float* __restrict__ tr,
                                                                   const float* __restrict__ rgb, int n_set,
                                                                   unsigned long long* __restrict__ acc,
                                                                   unsigned int* __restrict__ poison) {
  rgb_splat_body(P, tr, ColourSets(P, rgb, n_set, acc, poison), GRID_LANES);
}

// acc [B/R,n_set,3] zeroed 64-bit sums with poison [B/R] behind them, or nullptr: no sharing, drgb stored directly
__global__ __launch_bounds__(kSplatThreads) void k_rgb_splat_fixed_bwd(DpcParams P, const float* __restrict__ tr,
                                                                       const float* __restrict__ rgb, int n_set,
                                                                       const float* __restrict__ dC, float* __restrict__ drgb,
                                                                       float* __restrict__ dtr, unsigned long long* __restrict__ acc,
                                                                       unsigned int* __restrict__ poison) {
  rgb_splat_bwd_body(P, tr, dC, drgb, dtr, ColourSets(P, rgb, n_set, acc, poison), GRID_LANES);
}

// 64-bit sums -> fp32, one rounding in all: the integer is converted to fp32 with round-to-nearest (one correctly rounded
// conversion, whatever the sum's width) and scaled by 2^-40, which is exact.  Every element of a poisoned group (a cloud's
// grid, a colour set's gradient) is NaN; the other groups are untouched by it.
__global__ __launch_bounds__(kSplatThreads) void k_rgb_fixed_to_float(const unsigned long long* __restrict__ acc,
                                                                      const unsigned int* __restrict__ poison,
                                                                      float* __restrict__ out, size_t n, size_t per_group) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = poison[i / per_group] != 0u ? __int_as_float(0x7fc00000) : (float)(long long)acc[i] * kFixToFloat;
}

// ------------------------------------------------------------------------------------------------------
// Host side of the fixed-point entries
// ------------------------------------------------------------------------------------------------------
inline size_t fix_sets(const DpcParams* p) { return (size_t)(p->B / (p->point_replicas > 1 ? p->point_replicas : 1)); }
inline size_t fix_grid_elems(const DpcParams* p) { return (size_t)p->B * 3 * p->D * p->H * p->W; }
// the forward's part: the grid's sums, then one poison word per cloud
inline size_t fix_fwd_bytes(const DpcParams* p) { return ws_round(fix_grid_elems(p) * 8 + (size_t)p->B * 4); }
// the backward's part: the colour sets' sums, then one poison word per set; nothing when every point owns its colour row
inline size_t fix_bwd_bytes(const DpcParams* p, int n_set) {
  return shares_points(p) ? ws_round(fix_sets(p) * (size_t)n_set * 3 * 8 + fix_sets(p) * 4) : 0;
}

// checks shared by the three entries: everything that needs no device
inline int fix_validate(const DpcParams* p, int n_set) {
  const int rc = validate(p);
  if (rc != DPC_OK) return rc;
  if (p->n_live != nullptr) return DPC_ERR_SHAPE;   // the colour step is not capturable: no device-side point count
  if (p->point_index != nullptr ? (n_set < 1 || n_set != p->N_src) : n_set != p->N) return DPC_ERR_SHAPE;
  return DPC_OK;
}

}  // namespace
}  // namespace dpck

using namespace dpck;

extern "C" {

int dpc_rgb_splat_fwd(const DpcParams* p, const float* tr, const float* rgb, float* out, void* stream) {
  const int rc = rgb_validate(p);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!out || (p->N > 0 && (!tr || !rgb))) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  if (!zero_words_async(out, (size_t)p->B * 3 * p->D * p->H * p->W, st)) return DPC_ERR_LAUNCH;
  if (p->N == 0) return DPC_OK;
  DPC_LAUNCH("k_rgb_splat", dpc_kid("k_rgb_splat"), k_rgb_splat, dim3(splat_blocks((size_t)p->B * 3 * p->N * 2)), dim3(kSplatThreads),
             0, st, *p, tr, rgb, out);
  return launch_ok();
}

int dpc_rgb_splat_bwd(const DpcParams* p, const float* tr, const float* rgb, const float* dC, float* drgb, float* dtr,
                      void* stream) {
  const int rc = rgb_validate(p);
  if (rc != DPC_OK || p->B == 0 || p->N == 0) return rc;
  if (!tr || !rgb || !dC || !drgb) return DPC_ERR_NULL;
  DPC_LAUNCH("k_rgb_splat_bwd", dpc_kid("k_rgb_splat_bwd"), k_rgb_splat_bwd, dim3(splat_blocks((size_t)p->B * p->N)),
             dim3(kSplatThreads), 0, (hipStream_t)stream, *p, tr, rgb, dC, drgb, dtr);
  return launch_ok();
}

uint64_t dpc_rgb_splat_fixed_workspace_bytes(const DpcParams* p, int32_t n_set) {
  if (fix_validate(p, n_set) != DPC_OK) return 0;
  const size_t f = fix_fwd_bytes(p), b = fix_bwd_bytes(p, n_set);
  return f > b ? f : b;
}

int32_t dpc_rgb_splat_fixed_fwd(const DpcParams* p, const float* tr, const float* rgb_sets, int32_t n_set, float* out,
                                void* workspace, void* stream) {
  const int rc = fix_validate(p, n_set);
  if (rc != DPC_OK || p->B == 0) return rc;
  if (!out || (p->N > 0 && (!tr || !rgb_sets || !workspace))) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = fix_grid_elems(p);
  if (p->N == 0) return zero_words_async(out, n, st) ? DPC_OK : DPC_ERR_LAUNCH;
  unsigned long long* acc = static_cast<unsigned long long*>(workspace);
  unsigned int* poison = reinterpret_cast<unsigned int*>(acc + n);
  if (!zero_words_async(workspace, 2 * n + (size_t)p->B, st)) return DPC_ERR_LAUNCH;
  DPC_LAUNCH("k_rgb_splat_fixed", dpc_kid("k_rgb_splat_fixed"), k_rgb_splat_fixed, dim3(splat_blocks((size_t)p->B * 3 * p->N * 2)),
             dim3(kSplatThreads), 0, st, *p, tr, rgb_sets, n_set, acc, poison);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  DPC_LAUNCH("k_rgb_fixed_to_float", dpc_kid("k_rgb_fixed_to_float"), k_rgb_fixed_to_float, dim3(splat_blocks(n)), dim3(kSplatThreads),
             0, st, acc, poison, out, n, n / (size_t)p->B);
  return launch_ok();
}

int32_t dpc_rgb_splat_fixed_bwd(const DpcParams* p, const float* tr, const float* rgb_sets, int32_t n_set, const float* dC,
                                float* drgb_sets, float* dtr, void* workspace, void* stream) {
  const int rc = fix_validate(p, n_set);
  if (rc != DPC_OK || p->B == 0) return rc;
  const bool shared = shares_points(p);
  const size_t n = fix_sets(p) * (size_t)n_set * 3;   // elements of drgb_sets
  if (p->N == 0 && n == 0) return DPC_OK;              // no points and no colours: nothing to write
  if (!drgb_sets || (p->N > 0 && (!tr || !rgb_sets || !dC)) || (shared && !workspace)) return DPC_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* acc = shared ? static_cast<unsigned long long*>(workspace) : nullptr;
  unsigned int* poison = shared ? reinterpret_cast<unsigned int*>(acc + n) : nullptr;
  if (shared && !zero_words_async(workspace, 2 * n + fix_sets(p), st)) return DPC_ERR_LAUNCH;
  if (p->N > 0) {
    DPC_LAUNCH("k_rgb_splat_fixed_bwd", dpc_kid("k_rgb_splat_fixed_bwd"), k_rgb_splat_fixed_bwd, dim3(splat_blocks((size_t)p->B * p->N)),
               dim3(kSplatThreads), 0, st, *p, tr, rgb_sets, n_set, dC, drgb_sets, dtr, acc, poison);
    if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  }
  if (!shared) return DPC_OK;
  DPC_LAUNCH("k_rgb_fixed_to_float", dpc_kid("k_rgb_fixed_to_float"), k_rgb_fixed_to_float, dim3(splat_blocks(n)), dim3(kSplatThreads),
             0, st, acc, poison, drgb_sets, n, (size_t)n_set * 3);
  return launch_ok();
}

}  // extern "C"
