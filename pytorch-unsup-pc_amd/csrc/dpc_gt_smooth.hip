// Ground truth prepared for the losses in one launch: cfg.pc_gauss_filter_gt / pc_gauss_filter_gt_rgb of the TF-1 original
// (gauss_smoothen_image, dpc/util/gauss_kernel.py:14-24; called from dpc/models/model_pc.py:398-404 for the masks and
// dpc/util/losses.py:78-83, 128-129 for the images and the depth maps).  Per plane (one channel of one sample):
//
//   remap    v = (gt == remap_from) ? remap_to : gt                        add_proj_depth_loss, losses.py:121-124
//   resize   mean:   g[y,x] = (sum of the f x f window, row-major, fp32) / (f*f)   nn.AvgPool2d(f), the bits of pooled_mask
//            sample: g[y,x] = v[f*y, f*x]                                  TF-1's resize for an integer factor
//   blur     r[y,x] = sum_t w[t] g[y, x + t - c]     then     o[y,x] = sum_t w[t] r[y + t - c, x],   c = (ntaps - 1) / 2,
//            zeros outside the H x W plane (tf.nn.depthwise_conv2d, padding "SAME": [1,fsz] first, [fsz,1] second)
//
// Both sums run in tap order 0..ntaps-1 in fp32, the first term a plain product: with one tap of 1.0 the output is the
// resized input bit for bit, and an identity kernel of any length (zeros around a 1.0) gives the resized values.
//
// A workgroup of 256 threads owns a kTH x kTW tile of one plane's output.  It builds the resized tile with a halo of c rows
// and c columns in LDS, runs the row pass over the tile's rows and its halo rows into a second LDS buffer, and the column
// pass out of that to global memory: every global value is read once per tile that needs it, there is no intermediate in
// global memory and no atomic.  LDS is (kTH + 2c) x (2 kTW + 2c) floats, 59 KiB at 63 taps and 21 KiB at 21: planes of any
// size up to the sides the losses accept are tiled, none is refused for its size.
//
// The taps come as a launch argument (a host array) or are read from device memory by the kernel (a DeviceSchedule's
// taps_xy: a captured graph follows sigma).  Equal inputs give equal bits on every run.
#include "dpc_common.h"
#include "dpc_launch.h"

namespace dpcs {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 16;   // output tile: columns, rows
constexpr int kMaxSide = 1024;      // source sides, as in the losses

struct Shape {
  int S, C, Hs, Ws, H, W, f, planar, mode, ntaps, tiles_x, tiles_y;
  float remap_from, remap_to;
};

// the resized plane at (y, x), zero outside it
__device__ inline float resized(const float* __restrict__ gt, const Shape& p, int s, int c, int y, int x) {
  if (y < 0 || y >= p.H || x < 0 || x >= p.W) return 0.f;
  const bool remap = p.remap_from != p.remap_to;
  const int n = p.mode == DPC_GT_RESIZE_MEAN ? p.f : 1;
  // element (yy, xx) of the source plane: planar [S,C,Hs,Ws] or channel-last [S,Hs,Ws,C]
  const size_t row_stride = p.planar ? (size_t)p.Ws : (size_t)p.Ws * p.C;
  const size_t col_stride = p.planar ? (size_t)1 : (size_t)p.C;
  const float* base = p.planar ? gt + ((size_t)s * p.C + c) * p.Hs * p.Ws : gt + (size_t)s * p.Hs * p.Ws * p.C + c;
  base += (size_t)y * p.f * row_stride + (size_t)x * p.f * col_stride;
  float acc = 0.f;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      float v = base[i * row_stride + j * col_stride];
      if (remap && v == p.remap_from) v = p.remap_to;
      if (n == 1) return v;
      acc += v;
    }
  return acc / (float)(n * n);
}

__global__ __launch_bounds__(kThreads) void k_gt_smooth(const float* __restrict__ gt, Shape p, TapsDyn host,
                                                         const float* __restrict__ dev_taps, float* __restrict__ out) {
  extern __shared__ float lds[];
  __shared__ float w[DPC_MAX_TAPS];
  const int tid = threadIdx.x;
  const int n = p.ntaps, c = (n - 1) / 2;
  const int rows = kTH + 2 * c, cols = kTW + 2 * c;
  float* src = lds;                  // [rows][cols]: the resized tile and its halo
  float* mid = lds + rows * cols;    // [rows][kTW]:  after the row pass
  int b = blockIdx.x;
  const int tx = b % p.tiles_x;
  b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  b /= p.tiles_y;
  const int ch = b % p.C, s = b / p.C;
  const int x0 = tx * kTW, y0 = ty * kTH;

  if (tid < n) w[tid] = dev_taps != nullptr ? dev_taps[tid] : host.w[tid];
  for (int e = tid; e < rows * cols; e += kThreads) {
    const int r = e / cols, q = e - r * cols;
    src[e] = resized(gt, p, s, ch, y0 + r - c, x0 + q - c);
  }
  __syncthreads();
  for (int e = tid; e < rows * kTW; e += kThreads) {
    const int r = e / kTW, q = e - r * kTW;
    const float* v = src + r * cols + q;
    float acc = w[0] * v[0];
    for (int t = 1; t < n; ++t) acc = fmaf(w[t], v[t], acc);
    // rows outside the plane are the column pass's zero padding, whatever the row pass would make of them
    const int y = y0 + r - c;
    mid[e] = (y >= 0 && y < p.H) ? acc : 0.f;
  }
  __syncthreads();
  const int q = tid & (kTW - 1), x = x0 + q;
  for (int r = tid / kTW; r < kTH; r += kThreads / kTW) {
    const int y = y0 + r;
    if (y >= p.H || x >= p.W) continue;
    const float* v = mid + r * kTW + q;
    float acc = w[0] * v[0];
    for (int t = 1; t < n; ++t) acc = fmaf(w[t], v[t * kTW], acc);
    out[(((size_t)s * p.H + y) * p.W + x) * p.C + ch] = acc;
  }
}

size_t lds_bytes(int ntaps) {
  const int c = (ntaps - 1) / 2;
  return (size_t)(kTH + 2 * c) * (2 * kTW + 2 * c) * sizeof(float);
}

}  // namespace dpcs

extern "C" {

int dpc_gt_smooth(const float* gt, int S, int C, int Hs, int Ws, int planar, int H, int W, int resize_mode, float remap_from,
                  float remap_to, const float* host_taps, const float* dev_taps, int ntaps, float* out, void* stream) {
  using namespace dpcs;
  if (!gt || !out || (!host_taps && !dev_taps)) return DPC_ERR_NULL;
  if (S <= 0 || (C != 1 && C != 3) || H < 1 || W < 1 || Hs < H || Ws < W || Hs > kMaxSide || Ws > kMaxSide) return DPC_ERR_SHAPE;
  if (Hs % H || Ws % W || Hs / H != Ws / W) return DPC_ERR_SHAPE;
  if (resize_mode != DPC_GT_RESIZE_MEAN && resize_mode != DPC_GT_RESIZE_SAMPLE) return DPC_ERR_SHAPE;
  if (ntaps < 1 || ntaps % 2 == 0 || ntaps > DPC_MAX_TAPS) return DPC_ERR_TAPS;
  Shape p;
  p.S = S; p.C = C; p.Hs = Hs; p.Ws = Ws; p.H = H; p.W = W; p.f = Hs / H; p.planar = planar != 0; p.mode = resize_mode;
  p.ntaps = ntaps; p.tiles_x = (W + kTW - 1) / kTW; p.tiles_y = (H + kTH - 1) / kTH;
  p.remap_from = remap_from; p.remap_to = remap_to;
  const long long blocks = (long long)p.tiles_x * p.tiles_y * C * S;
  if (blocks > 0x7fffffffLL) return DPC_ERR_SHAPE;
  TapsDyn taps;
  taps.n = ntaps;
  for (int i = 0; i < DPC_MAX_TAPS; ++i) taps.w[i] = (host_taps && i < ntaps) ? host_taps[i] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  DPC_LAUNCH("k_gt_smooth", dpc_kid("k_gt_smooth"), k_gt_smooth, dim3((unsigned)blocks), dim3(kThreads), lds_bytes(ntaps), st, gt, p,
             taps, dev_taps, out);
  return launch_ok();
}

}  // extern "C"
