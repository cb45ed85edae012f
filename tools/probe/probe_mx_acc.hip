// How exactly does v_mfma_scale_f32_16x16x128_f8f6f4 (OCP e4m3, E8M0 block scales) add its 128 products and the accumulator on gfx950?
// One MFMA per wave on its own (no kernel of the library involved), against the exact sum in double: e4m3 x e4m3 products have 8
// significant bits, so 128 of them and an f32 accumulator add exactly in a double as long as their exponents span less than 2^40.
// Reported per data set: F = max |D - (c + sum_k a_k b_k)| / (128 2^-23 (|c| + sum_k |a_k b_k|)), the factor on the term
// K 2^-23 (|A| |W|^T) of the per-element judge in tests/test_fp8_paths_gpu.py (F <= 1 would be a sequential f32 sum's worst case).
// Build: hipcc --offload-arch=gfx950 -O2 tools/probe/probe_mx_acc.hip -o tools/probe/bin/probe_mx_acc ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define OK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

// operand map of the library's kernels (gemm_fp8.hip): lane (r = lane & 15, q = lane >> 4) supplies the 16-byte chunks q and q + 4 of row
// r's 128 bytes and the scale of block q; D register i of a lane: row 4 (lane >> 4) + i of the first operand times row lane & 15 of the second
__global__ void one_mfma(const uint8_t* A, const uint8_t* B, const uint8_t* sa, const uint8_t* sb, const float* cin, float* out) {
  const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
  const size_t w = blockIdx.x;
  const uint8_t* pa = A + w * 2048 + r * 128;
  const uint8_t* pb = B + w * 2048 + r * 128;
  v8i a, b;
  for (int i = 0; i < 4; ++i) {
    a[i] = ((const int*)(pa + 16 * q))[i]; a[4 + i] = ((const int*)(pa + 64 + 16 * q))[i];
    b[i] = ((const int*)(pb + 16 * q))[i]; b[4 + i] = ((const int*)(pb + 64 + 16 * q))[i];
  }
  const int scale_a = sa[w * 64 + r * 4 + q], scale_b = sb[w * 64 + r * 4 + q];
  f32x4 c;
  for (int i = 0; i < 4; ++i) c[i] = cin[w * 256 + lane * 4 + i];
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, scale_a, 0, scale_b);
  for (int i = 0; i < 4; ++i) out[w * 256 + lane * 4 + i] = c[i];
}

static double e4m3_val(uint8_t b) {
  const int ef = (b >> 3) & 15, mf = b & 7;
  const double m = ef == 0 ? std::ldexp((double)mf, -9) : std::ldexp((double)(8 + mf), ef - 10);
  return (b & 0x80) ? -m : m;
}
// round to nearest even onto the e4m3 grid, saturating at 448
static uint8_t e4m3_enc(double v) {
  const uint8_t s = v < 0 ? 0x80 : 0;
  v = std::fabs(v);
  if (v >= 448) return s | 0x7e;
  int best = 0;
  double bd = v;
  for (int b = 1; b <= 0x7e; ++b) {
    const double d = std::fabs(e4m3_val((uint8_t)b) - v);
    if (d < bd || (d == bd && (b & 1) == 0)) { bd = d; best = b; }
  }
  return s | (uint8_t)best;
}
// MX quantisation of a row of 128 doubles: bytes + 4 scale bytes (as quant_mx_kernel)
static void mx_row(const double* x, uint8_t* q, uint8_t* sc) {
  for (int blk = 0; blk < 4; ++blk) {
    double am = 0;
    for (int j = 0; j < 32; ++j) am = std::max(am, std::fabs(x[blk * 32 + j]));
    int e = am > 0 ? (int)std::floor(std::log2(am)) - 8 : -127;
    e = std::min(126, std::max(-127, e));
    for (int j = 0; j < 32; ++j) q[blk * 32 + j] = e4m3_enc(std::ldexp(x[blk * 32 + j], -e));
    sc[blk] = (uint8_t)(e + 127);
  }
}

int main() {
  const int W = 2048;                                   // waves (= MFMAs) per data set
  std::vector<uint8_t> A((size_t)W * 2048), B((size_t)W * 2048), sa((size_t)W * 64), sb((size_t)W * 64);
  std::vector<float> cin((size_t)W * 256), out((size_t)W * 256);
  uint8_t *dA, *dB, *dsa, *dsb; float *dc, *dout;
  OK(hipMalloc(&dA, A.size())); OK(hipMalloc(&dB, B.size())); OK(hipMalloc(&dsa, sa.size())); OK(hipMalloc(&dsb, sb.size()));
  OK(hipMalloc(&dc, cin.size() * 4)); OK(hipMalloc(&dout, out.size() * 4));
  std::mt19937_64 rng(12345);
  std::normal_distribution<double> nd(0.0, 1.0);
  const char* names[] = {"integers, scales 2^-2..2^2 (must be exact)", "MX-quantised N(0,1) x N(0,1)/sqrt(128), c = 0", "the same, c ~ 2 N(0,1)",
                         "the same, rows scaled by 2^-6..2^6, c ~ N(0,1)", "uniform random e4m3 bytes, all scales 1, c = 0",
                         "N(0,1) x N(0,1)/sqrt(128) with an offset of 4 (products of one sign), c = 0"};
  for (int set = 0; set < 6; ++set) {
    std::vector<double> row(128);
    for (int w = 0; w < W; ++w)
      for (int side = 0; side < 2; ++side)
        for (int r = 0; r < 16; ++r) {
          uint8_t* q = (side ? B : A).data() + (size_t)w * 2048 + r * 128;
          uint8_t* sc = (side ? sb : sa).data() + (size_t)w * 64 + r * 4;
          if (set == 0) {
            for (int k = 0; k < 128; ++k) q[k] = e4m3_enc((double)((int)(rng() % 17) - 8));
            for (int blk = 0; blk < 4; ++blk) sc[blk] = (uint8_t)(125 + rng() % 5);
          } else if (set == 4) {
            for (int k = 0; k < 128; ++k) { uint8_t b = (uint8_t)(rng() & 0xff); if ((b & 0x7f) == 0x7f) b ^= 1; q[k] = b; }
            for (int blk = 0; blk < 4; ++blk) sc[blk] = 127;
          } else {
            const double rs = set == 3 ? std::ldexp(1.0, (int)(rng() % 13) - 6) : 1.0, off = set == 5 ? 4.0 : 0.0;
            for (int k = 0; k < 128; ++k) row[k] = (nd(rng) + off) * rs * (side ? 1.0 / std::sqrt(128.0) : 1.0);
            mx_row(row.data(), q, sc);
          }
        }
    for (auto& v : cin) v = set == 2 ? (float)(2 * nd(rng)) : (set == 3 ? (float)nd(rng) : 0.f);
    OK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice)); OK(hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice));
    OK(hipMemcpy(dsa, sa.data(), sa.size(), hipMemcpyHostToDevice)); OK(hipMemcpy(dsb, sb.data(), sb.size(), hipMemcpyHostToDevice));
    OK(hipMemcpy(dc, cin.data(), cin.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(one_mfma, dim3(W), dim3(64), 0, 0, dA, dB, dsa, dsb, dc, dout);
    OK(hipGetLastError());
    OK(hipDeviceSynchronize());
    OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    double fmax = 0, fsum = 0, rel_ulp_max = 0, signed_sum = 0;
    long n = 0, inexact = 0;
    for (int w = 0; w < W; ++w)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int n_ = lane & 15, m_ = (lane >> 4) * 4 + i;       // A row m_ (first operand) times B row n_ (second operand)
          const uint8_t* pa = A.data() + (size_t)w * 2048 + m_ * 128;
          const uint8_t* pb = B.data() + (size_t)w * 2048 + n_ * 128;
          double dot = 0, mag = 0;
          for (int k = 0; k < 128; ++k) {
            const double p = e4m3_val(pa[k]) * std::ldexp(1.0, sa[(size_t)w * 64 + m_ * 4 + k / 32] - 127) * e4m3_val(pb[k]) *
                             std::ldexp(1.0, sb[(size_t)w * 64 + n_ * 4 + k / 32] - 127);
            dot += p; mag += std::fabs(p);
          }
          const double c = cin[(size_t)w * 256 + lane * 4 + i];
          const double ref = c + dot, got = out[(size_t)w * 256 + lane * 4 + i];
          const double err = got - ref, f = std::fabs(err) / (128 * std::ldexp(1.0, -23) * (std::fabs(c) + mag) + 1e-300);
          if (err != 0 && (double)(float)ref == ref) ++inexact;
          fmax = std::max(fmax, f); fsum += f; signed_sum += err / (std::fabs(c) + mag + 1e-300); ++n;
          if (ref != 0) rel_ulp_max = std::max(rel_ulp_max, std::fabs(err) / std::fabs(ref) * std::ldexp(1.0, 24));
        }
    printf("set %d (%s): %ld dot products, F max %.4f, F mean %.5f, mean signed err / (|c| + sum |a b|) %.3e, max |err| in units of 2^-24 |ref| %.1f, wrong where the exact sum is an f32: %ld\n",
           set, names[set], n, fmax, fsum / n, signed_sum / n, rel_ulp_max, inexact);
  }
  // the alignment window: one product of 2^16 (256 x 256) beside 127 equal products of 2^(16 - s): how much of the small ones arrives?
  for (int s = 0; s <= 36; s += 2) {
    for (int r = 0; r < 16; ++r) {
      for (int k = 0; k < 128; ++k) { A[r * 128 + k] = e4m3_enc(k == 0 ? 256.0 : 1.0); B[r * 128 + k] = e4m3_enc(k == 0 ? 256.0 : 1.0); }
      // block 0 holds the big product at scale 1 and 31 small ones that are made small by their own values; blocks 1-3 by their scales
      for (int k = 1; k < 32; ++k) { A[r * 128 + k] = e4m3_enc(std::ldexp(1.0, -(s / 2 > 9 ? 9 : s / 2))); B[r * 128 + k] = e4m3_enc(std::ldexp(1.0, -(s / 2 > 9 ? 9 : s / 2))); }
      sa[r * 4] = sb[r * 4] = 127;
      for (int blk = 1; blk < 4; ++blk) { sa[r * 4 + blk] = (uint8_t)(127 + 8 - s / 2); sb[r * 4 + blk] = (uint8_t)(127 + 8 - (s - s / 2)); }
    }
    for (int i = 0; i < 256; ++i) cin[i] = 0.f;
    OK(hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice)); OK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    OK(hipMemcpy(dsa, sa.data(), 64, hipMemcpyHostToDevice)); OK(hipMemcpy(dsb, sb.data(), 64, hipMemcpyHostToDevice));
    OK(hipMemcpy(dc, cin.data(), 1024, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(one_mfma, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dc, dout);
    OK(hipGetLastError());
    OK(hipDeviceSynchronize());
    OK(hipMemcpy(out.data(), dout, 1024, hipMemcpyDeviceToHost));
    double small = 0;
    for (int k = 1; k < 128; ++k)
      small += e4m3_val(A[k]) * std::ldexp(1.0, sa[k / 32] - 127) * e4m3_val(B[k]) * std::ldexp(1.0, sb[k / 32] - 127);
    printf("window: 65536 + 127 products summing to %.6g (each about 2^%d): got 65536 + %.6g, exact f32 rounding would give 65536 + %.6g\n", small,
           16 - s, (double)out[0] - 65536.0, (double)(float)(65536.0 + small) - 65536.0);
  }
  return 0;
}
