// Per-image comparison of two uint8 NHWC stacks a, b (N,H,W,3): the exact sum of squared differences (what MSE / PSNR are made of) and
// the mean structural similarity of Wang et al. 2004 (11x11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03, data range 255, valid
// positions only: the definition in include/svg_hip.h).  The reference has no counterpart.
//   frame_metrics_tile_kernel    one workgroup per (image, 32x32 tile of the (H-10) x (W-10) map).  Per channel: the tile and its 10-pixel
//                                halo of both images go to LDS as f32 (byte loads: neither a row of 3 W bytes nor an image is 4-byte
//                                aligned in general), the horizontal 11-tap pass of a, b, a^2, b^2, ab goes to LDS, the vertical pass and
//                                the map value stay in registers.  The pixels are taken minus 128 first: variances and the covariance do
//                                not change, and the cancellation in G*a^2 - mu^2 loses two bits less.  Every pixel belongs to exactly one
//                                tile (the last tile of a row / column also owns the 10-pixel margin, which its halo load covers), whose
//                                integer squared differences it sums.  The block's two sums go to a [N][tiles] workspace.
//   frame_metrics_finish_kernel  adds an image's partials in tile order: int64 for the squared differences, double for the map.
// No atomics and a fixed order everywhere: an image gives the same bits alone, repeated, or inside a larger batch.
// An evaluation tool, not the hot path.
#include "kernels.h"

namespace {

constexpr int kTile = 32;                  // map positions per tile side
constexpr int kWin = 11;                   // window taps
constexpr int kReg = kTile + kWin - 1;     // 42: pixels per tile side with the halo
constexpr int kThreads = 256;

struct SsimTaps { float g[kWin]; };

__global__ void __launch_bounds__(kThreads) frame_metrics_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W,
                                                                     int tiles_x, int tiles_y, const SsimTaps taps, double* __restrict__ part_ssim,
                                                                     uint32_t* __restrict__ part_sse, float* __restrict__ map) {
  __shared__ float sa[kReg * kReg], sb[kReg * kReg];       // the region of one channel, pixel - 128
  __shared__ float hp[5][kReg * kTile];                    // horizontal pass: a, b, a^2, b^2, ab at [row][column of the tile]
  __shared__ double red_ssim[kThreads / 64];
  __shared__ uint32_t red_sse[kThreads / 64];
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  const int oy0 = ty * kTile, ox0 = tx * kTile;
  const int th = min(kTile, Ho - oy0), tw = min(kTile, Wo - ox0);     // map positions of this tile
  const int rh = th + kWin - 1, rw = tw + kWin - 1;                   // pixels it reads: rows oy0 .. oy0 + rh <= H, the same for columns
  const int own_h = ty == tiles_y - 1 ? rh : th, own_w = tx == tiles_x - 1 ? rw : tw;   // pixels whose squared differences it sums
  const int64_t img = (int64_t)n * H * W * 3;
  const uint8_t* pa = a + img;
  const uint8_t* pb = b + img;
  uint32_t sse = 0;
  double ssim = 0.0;
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < rh * rw; i += kThreads) {
      const int r = i / rw, x = i % rw;
      const int off = ((oy0 + r) * W + ox0 + x) * 3 + c;              // < H W 3 < 2^31 (checked by the entry point)
      const int va = pa[off], vb = pb[off];
      sa[r * kReg + x] = (float)(va - 128);
      sb[r * kReg + x] = (float)(vb - 128);
      if (r < own_h && x < own_w) sse += (uint32_t)((va - vb) * (va - vb));
    }
    __syncthreads();
    for (int i = tid; i < rh * tw; i += kThreads) {
      const int r = i / tw, x = i % tw;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const float g = taps.g[k], u = sa[r * kReg + x + k], v = sb[r * kReg + x + k];
        s0 += g * u; s1 += g * v; s2 += g * (u * u); s3 += g * (v * v); s4 += g * (u * v);
      }
      const int o = r * kTile + x;
      hp[0][o] = s0; hp[1][o] = s1; hp[2][o] = s2; hp[3][o] = s3; hp[4][o] = s4;
    }
    __syncthreads();
    // (the next channel's region load writes sa / sb only, which nobody reads below; its horizontal pass comes after a barrier)
    for (int i = tid; i < th * tw; i += kThreads) {
      const int y = i / tw, x = i % tw;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const float g = taps.g[k];
        const int o = (y + k) * kTile + x;
        s0 += g * hp[0][o]; s1 += g * hp[1][o]; s2 += g * hp[2][o]; s3 += g * hp[3][o]; s4 += g * hp[4][o];
      }
      const float va = s2 - s0 * s0, vb = s3 - s1 * s1, cab = s4 - s0 * s1;       // shift-invariant
      const float ma = s0 + 128.f, mb = s1 + 128.f;
      const float C1 = 6.5025f, C2 = 58.5225f;
      const float v = ((2.f * ma * mb + C1) * (2.f * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2));
      ssim += (double)v;
      if (map) map[(((int64_t)n * Ho + oy0 + y) * Wo + ox0 + x) * 3 + c] = v;
    }
  }
  // per wave, then per block, both in a fixed order
  for (int d = 32; d >= 1; d >>= 1) {
    ssim += __shfl_down(ssim, d, 64);
    sse += __shfl_down(sse, d, 64);
  }
  if ((tid & 63) == 0) { red_ssim[tid >> 6] = ssim; red_sse[tid >> 6] = sse; }
  __syncthreads();
  if (tid == 0) {
    double s = red_ssim[0];
    uint32_t e = red_sse[0];
    for (int w = 1; w < kThreads / 64; ++w) { s += red_ssim[w]; e += red_sse[w]; }
    part_ssim[blockIdx.x] = s;
    part_sse[blockIdx.x] = e;       // <= 42 * 42 * 3 * 255^2 < 2^32
  }
}

__global__ void frame_metrics_finish_kernel(const double* __restrict__ part_ssim, const uint32_t* __restrict__ part_sse, int N, int tiles,
                                            double positions, int64_t* __restrict__ sse, double* __restrict__ ssim) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  int64_t e = 0;
  for (int t = 0; t < tiles; ++t) {
    s += part_ssim[(int64_t)n * tiles + t];
    e += (int64_t)part_sse[(int64_t)n * tiles + t];
  }
  sse[n] = e;
  ssim[n] = s / positions;
}

}  // namespace

int64_t frame_metrics_tiles(int H, int W) { return (int64_t)cdiv(H - (kWin - 1), kTile) * cdiv(W - (kWin - 1), kTile); }

void frame_metrics(const uint8_t* a, const uint8_t* b, int N, int H, int W, double* part_ssim, uint32_t* part_sse, int64_t* sse, double* ssim,
                   float* ssim_map, hipStream_t s) {
  const int tiles_x = cdiv(W - (kWin - 1), kTile), tiles_y = cdiv(H - (kWin - 1), kTile);
  SsimTaps taps;
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double x = k - kWin / 2;
    g[k] = std::exp(-x * x / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < kWin; ++k) taps.g[k] = (float)(g[k] / sum);
  const int tiles = tiles_x * tiles_y;
  hipLaunchKernelGGL(frame_metrics_tile_kernel, dim3((unsigned)((int64_t)N * tiles)), dim3(kThreads), 0, s, a, b, H, W, tiles_x, tiles_y, taps, part_ssim,
                     part_sse, ssim_map);
  check_launch("frame_metrics_tile");
  const double positions = (double)(H - (kWin - 1)) * (double)(W - (kWin - 1)) * 3.0;
  hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(cdiv(N, 64)), dim3(64), 0, s, part_ssim, part_sse, N, tiles, positions, sse, ssim);
  check_launch("frame_metrics_finish");
}
