// Bit-reproducible colour splat that reads shared colour sets in place (k_rgb_splat_fixed, its gather backward
// k_rgb_splat_fixed_bwd, the converter k_rgb_fixed_to_float).  The arithmetic of every contribution is k_rgb_splat's
// (dpc_rgb.hip); what differs is the sum: each contribution is rounded once to 64-bit fixed point with 40 fractional bits
// (grad_to_fixed, dpc_kernels.h) and added as an integer.  Integer adds commute, so a voxel's sum is the same bits in whatever
// order its adds arrive, and with it everything computed from the colour grid.  The colour of point i of cloud b is
// rgb[b / R][point_index ? point_index[b][i] : i] (DpcParams.point_replicas / point_index, the occupancy path's convention):
// the decoder's [B/R,N_set,3] colours serve every view and every dropout row without a [B,n,3] copy, and their gradients are
// summed in fixed point as well (the dpc_fixed pattern of dpc_slab_bwd.hip).  Design notes: DESIGN.md section 4.
#include "dpc_colour_column.h"

namespace dpck {
namespace {

constexpr int kFixThreads = 256;

inline unsigned fix_blocks(size_t total) {
  const size_t b = (total + kFixThreads - 1) / kFixThreads;
  return (unsigned)(b < 1 ? 1 : (b > 1048576 ? 1048576 : b));
}

// Largest colour magnitude the splat accepts.  A contribution is w * c with 0 <= w <= 1 (fp32 products of factors <= 1 never
// round upwards past their larger operand), so |contribution| <= kRgbFixMax and its fixed-point value is at most
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

// ------------------------------------------------------------------------------------------------------
// Forward.  Lanes as in k_rgb_splat: two neighbouring lanes per (cloud, channel, point), the point index next fastest; the
// pair owns the two x corners, 16 contiguous bytes of the 64-bit plane.  acc [B,3,D,H,W] zeroed 64-bit sums, poison [B]
// zeroed words behind them.  A colour that is not a finite number of magnitude <= kRgbFixMax, or a point_index entry
// outside its set, adds nothing and sets its cloud's poison word.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFixThreads) void k_rgb_splat_fixed(DpcParams P, const float* __restrict__ tr,
                                                                 const float* __restrict__ rgb, int n_set,
                                                                 unsigned long long* __restrict__ acc,
                                                                 unsigned int* __restrict__ poison) {
  const int D = P.D, H = P.H, W = P.W;
  const int reps = P.point_replicas > 1 ? P.point_replicas : 1;
  const size_t total = (size_t)P.B * 3 * P.N * 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 1);
    const size_t h = i >> 1;
    const int n = (int)(h % P.N);
    const size_t bc = h / P.N;
    const int c = (int)(bc % 3);
    const size_t b = bc / 3;
    const size_t pt = b * P.N + n;
    const int src = colour_row(P, pt, n, n_set);
    if (src < 0) {   // every lane of the point sees it; one of them reports
      if (c == 0 && e == 0) {
        atomicOr(poison + b, 1u);
        if (P.status != nullptr) atomicOr(P.status, (int)DPC_STATUS_BAD_INDEX);
      }
      continue;
    }
    const Cell cl = cell_from_record(make_record((double)tr[3 * pt], (double)tr[3 * pt + 1], (double)tr[3 * pt + 2], D, H, W));
    if (!cl.valid || cl.ix + e >= W) continue;
    const float col = rgb[((b / reps) * n_set + src) * 3 + c];
    if (!(fabsf(col) <= kRgbFixMax)) {   // too large, Inf, or NaN (which fails the comparison)
      atomicOr(poison + b, 1u);
      continue;
    }
    const float wc = (e ? cl.wx[1] : cl.wx[0]) * col;
    unsigned long long* plane = acc + bc * D * H * W + cl.ix + e;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool ok = (cl.iz + k < D) && (cl.iy + j < H);
        if (ok) atomicAdd(plane + ((size_t)(cl.iz + k) * H + cl.iy + j) * W, grad_to_fixed(cl.wz[k] * cl.wy[j] * wc));
      }
  }
}

// 64-bit sums -> fp32, one rounding in all: the integer is converted to fp32 with round-to-nearest (one correctly rounded
// conversion, whatever the sum's width) and scaled by 2^-40, which is exact.  Every element of a poisoned group (a cloud's
// grid, a colour set's gradient) is NaN; the other groups are untouched by it.
__global__ __launch_bounds__(kFixThreads) void k_rgb_fixed_to_float(const unsigned long long* __restrict__ acc,
                                                                    const unsigned int* __restrict__ poison,
                                                                    float* __restrict__ out, size_t n, size_t per_group) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = poison[i / per_group] != 0u ? __int_as_float(0x7fc00000) : (float)(long long)acc[i] * kFixToFloat;
}

// ------------------------------------------------------------------------------------------------------
// Backward: one lane per (cloud, point), the gathers and formulas of k_rgb_splat_bwd with the colour read through the
// same addressing.  drgb: direct stores when every point owns its colour row (acc == nullptr); otherwise 64-bit fixed-point
// adds into acc [B/R,n_set,3] under grad_fits_fixed's bound, a set's poison word for a contribution beyond it (or for an
// index outside the set).  Repeated indices of a point_index row are just more integer adds.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFixThreads) void k_rgb_splat_fixed_bwd(DpcParams P, const float* __restrict__ tr,
                                                                     const float* __restrict__ rgb, int n_set,
                                                                     const float* __restrict__ dC, float* __restrict__ drgb,
                                                                     float* __restrict__ dtr, unsigned long long* __restrict__ acc,
                                                                     unsigned int* __restrict__ poison) {
  const int D = P.D, H = P.H, W = P.W;
  const int reps = P.point_replicas > 1 ? P.point_replicas : 1;
  const size_t total = (size_t)P.B * P.N, plane = (size_t)D * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / P.N;
    const int src = colour_row(P, i, (int)(i - b * P.N), n_set);
    const size_t row = (b / reps) * n_set + (src < 0 ? 0 : src);
    const Cell c = cell_from_record(make_record((double)tr[3 * i], (double)tr[3 * i + 1], (double)tr[3 * i + 2], D, H, W));
    float dcol[3] = {0.f, 0.f, 0.f};
    float dZ = 0.f, dY = 0.f, dX = 0.f;
    const bool live = c.valid && src >= 0;
    if (live) {
      const float col[3] = {rgb[3 * row], rgb[3 * row + 1], rgb[3 * row + 2]};
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
    if (acc == nullptr) {   // launch-uniform: no sharing, point i owns row i
      drgb[3 * i] = dcol[0]; drgb[3 * i + 1] = dcol[1]; drgb[3 * i + 2] = dcol[2];
    } else if (src < 0) {
      atomicOr(poison + b / reps, 1u);
      if (P.status != nullptr) atomicOr(P.status, (int)DPC_STATUS_BAD_INDEX);
    } else if (c.valid) {   // a point outside the cube contributes exact zeros: nothing to add
      if (grad_fits_fixed(dcol[0], dcol[1], dcol[2])) {
        unsigned long long* a = acc + 3 * row;
        atomicAdd(a + 0, grad_to_fixed(dcol[0])); atomicAdd(a + 1, grad_to_fixed(dcol[1])); atomicAdd(a + 2, grad_to_fixed(dcol[2]));
      } else {   // NaN / Inf / out of range: the set's gradient becomes NaN (dpc_kernels.h, grad_fits_fixed)
        atomicOr(poison + b / reps, 1u);
      }
    }
    if (dtr != nullptr) { dtr[3 * i] = dZ; dtr[3 * i + 1] = dY; dtr[3 * i + 2] = dX; }
  }
}

// ------------------------------------------------------------------------------------------------------
// Host side
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
  DPC_LAUNCH("k_rgb_splat_fixed", dpc_kid("k_rgb_splat_fixed"), k_rgb_splat_fixed, dim3(fix_blocks((size_t)p->B * 3 * p->N * 2)),
             dim3(kFixThreads), 0, st, *p, tr, rgb_sets, n_set, acc, poison);
  if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  DPC_LAUNCH("k_rgb_fixed_to_float", dpc_kid("k_rgb_fixed_to_float"), k_rgb_fixed_to_float, dim3(fix_blocks(n)), dim3(kFixThreads), 0,
             st, acc, poison, out, n, n / (size_t)p->B);
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
    DPC_LAUNCH("k_rgb_splat_fixed_bwd", dpc_kid("k_rgb_splat_fixed_bwd"), k_rgb_splat_fixed_bwd, dim3(fix_blocks((size_t)p->B * p->N)),
               dim3(kFixThreads), 0, st, *p, tr, rgb_sets, n_set, dC, drgb_sets, dtr, acc, poison);
    if (launch_ok() != DPC_OK) return DPC_ERR_LAUNCH;
  }
  if (!shared) return DPC_OK;
  DPC_LAUNCH("k_rgb_fixed_to_float", dpc_kid("k_rgb_fixed_to_float"), k_rgb_fixed_to_float, dim3(fix_blocks(n)), dim3(kFixThreads), 0,
             st, acc, poison, drgb_sets, n, (size_t)n_set * 3);
  return launch_ok();
}

}  // extern "C"
