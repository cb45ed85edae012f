// Element-wise and layout kernels of the sampling path (HBM-bound, vectorised where the layout allows).
#include "kernels.h"

namespace SDNS {


namespace {

#define GRID_STRIDE(idx, total) \
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (total); idx += (int64_t)gridDim.x * blockDim.x)

inline dim3 grid_for(int64_t total) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192))); }

// nearest: src = floor(dst * in / out)  (torch F.interpolate mode='nearest', predict.py:158,178)
__device__ __forceinline__ int nearest_src(int d, int in, int out) {
  int s = (int)floorf((float)d * ((float)in / (float)out));
  return min(s, in - 1);
}

// sd_utils.py:135-138: x/255 -> 2*(x-0.5); channels padded 3 -> 8 with zeros
__global__ void img_to_act_kernel(const uint8_t* __restrict__ img, h16* __restrict__ out, int N, int sh, int sw, int H, int W) {
  const int64_t total = (int64_t)N * H * W;
  GRID_STRIDE(idx, total) {
    const int x = (int)(idx % W);
    const int y = (int)((idx / W) % H);
    const int n = (int)(idx / ((int64_t)W * H));
    const int sy = (sh == H) ? y : nearest_src(y, sh, H);
    const int sx = (sw == W) ? x : nearest_src(x, sw, W);
    const uint8_t* p = img + (((int64_t)n * sh + sy) * sw + sx) * 3;
    h16x8 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float f = (float)p[c] / 255.0f;
      o[c] = (h16)(2.f * (f - 0.5f));
    }
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = (h16)0.f;
    *(h16x8*)(out + idx * 8) = o;
  }
}

// sd_utils.py:164-166: (x/2+.5).clamp(0,1) -> *255 -> round (half to even) -> u8, with nearest resize
__global__ void act_to_img_kernel(const float* __restrict__ x, int ldc, uint8_t* __restrict__ img, float* __restrict__ fout,
                                  int N, int h, int w, int oh, int ow) {
  if (img) {
    const int64_t total = (int64_t)N * oh * ow;
    GRID_STRIDE(idx, total) {
      const int ox = (int)(idx % ow);
      const int oy = (int)((idx / ow) % oh);
      const int n = (int)(idx / ((int64_t)ow * oh));
      const int sy = (oh == h) ? oy : nearest_src(oy, h, oh);
      const int sx = (ow == w) ? ox : nearest_src(ox, w, ow);
      const float* p = x + (((int64_t)n * h + sy) * w + sx) * ldc;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float f = p[c] / 2.f + 0.5f;
        f = fminf(fmaxf(f, 0.f), 1.f);
        img[idx * 3 + c] = (uint8_t)rintf(f * 255.f);
      }
    }
  }
  if (fout) {
    const int64_t total = (int64_t)N * h * w;
    GRID_STRIDE(idx, total) {
      const int px = (int)(idx % ((int64_t)h * w));
      const int n = (int)(idx / ((int64_t)h * w));
      const float* p = x + idx * ldc;
#pragma unroll
      for (int c = 0; c < 3; ++c) fout[((int64_t)n * 3 + c) * h * w + px] = p[c];
    }
  }
}

__global__ void nchw_to_act_kernel(const float* __restrict__ x, h16* __restrict__ out, int N, int C, int hw, int Cpad, float scale) {
  const int64_t total = (int64_t)N * hw;
  GRID_STRIDE(idx, total) {
    const int px = (int)(idx % hw);
    const int n = (int)(idx / hw);
    for (int c = 0; c < Cpad; ++c)
      out[idx * Cpad + c] = (h16)((c < C) ? x[((int64_t)n * C + c) * hw + px] * scale : 0.f);
  }
}

__global__ void nchw_to_actf32_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int C, int hw, float scale) {
  const int64_t total = (int64_t)N * hw;
  GRID_STRIDE(idx, total) {
    const int px = (int)(idx % hw);
    const int n = (int)(idx / hw);
    for (int c = 0; c < C; ++c) out[idx * C + c] = x[((int64_t)n * C + c) * hw + px] * scale;
  }
}
__global__ void actf32_pad_h16_kernel(const float* __restrict__ x, int C, h16* __restrict__ out, int Cpad, int64_t P) {
  GRID_STRIDE(idx, P) {
    for (int c = 0; c < Cpad; ++c) out[idx * Cpad + c] = (h16)((c < C) ? x[idx * C + c] : 0.f);
  }
}

__global__ void actf32_to_nchw_kernel(const float* __restrict__ x, int ld, float* __restrict__ out, int N, int C, int hw) {
  const int64_t total = (int64_t)N * hw;
  GRID_STRIDE(idx, total) {
    const int px = (int)(idx % hw);
    const int n = (int)(idx / hw);
    for (int c = 0; c < C; ++c) out[((int64_t)n * C + c) * hw + px] = x[idx * ld + c];
  }
}

__global__ void pixel_linear_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ b,
                                    float* __restrict__ y, int ldy, int64_t P, int Cin, int Cout) {
  GRID_STRIDE(p, P) {
    float in[8];
    for (int i = 0; i < Cin; ++i) in[i] = x[p * ldx + i];
    for (int o = 0; o < Cout; ++o) {
      float acc = b ? b[o] : 0.f;
      for (int i = 0; i < Cin; ++i) acc += w[o * Cin + i] * in[i];
      y[p * ldy + o] = acc;
    }
  }
}

// DiagonalGaussianDistribution.sample (diffusers vae.py): logvar clamp [-30,20], std = exp(.5 logvar);
// sd_utils.py:142-143: .sample() then *= 0.18215
__global__ void vae_sample_kernel(const float* __restrict__ mom, int ldm, const float* __restrict__ eps, float* __restrict__ z,
                                  float* __restrict__ mom_nchw, int N, int hw) {
  const int64_t total = (int64_t)N * hw;
  GRID_STRIDE(idx, total) {
    const int px = (int)(idx % hw);
    const int n = (int)(idx / hw);
    const float* m = mom + idx * ldm;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float mean = m[c];
      const float lv = fminf(fmaxf(m[4 + c], -30.f), 20.f);
      const int64_t o = ((int64_t)n * 4 + c) * hw + px;
      float v = mean;
      if (eps) v += expf(0.5f * lv) * eps[o];
      z[o] = v * 0.18215f;
      if (mom_nchw) {
        mom_nchw[((int64_t)n * 8 + c) * hw + px] = mean;
        mom_nchw[((int64_t)n * 8 + 4 + c) * hw + px] = m[4 + c];
      }
    }
  }
}

__global__ void concat_kernel(const h16* __restrict__ a, int Ca, const h16* __restrict__ b, int Cb, h16* __restrict__ out, int64_t P) {
  const int CV = (Ca + Cb) / 8;
  const int64_t total = P * CV;
  GRID_STRIDE(idx, total) {
    const int cv = (int)(idx % CV);
    const int64_t p = idx / CV;
    const int c0 = cv * 8;
    h16x8 v = (c0 < Ca) ? *(const h16x8*)(a + p * Ca + c0) : *(const h16x8*)(b + p * Cb + (c0 - Ca));
    *(h16x8*)(out + p * (Ca + Cb) + c0) = v;
  }
}

__global__ void resize_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int N, int sh, int sw, int C, int dh, int dw) {
  const int64_t total = (int64_t)N * dh * dw;
  GRID_STRIDE(idx, total) {
    const int x = (int)(idx % dw);
    const int y = (int)((idx / dw) % dh);
    const int n = (int)(idx / ((int64_t)dw * dh));
    const int sy = nearest_src(y, sh, dh), sx = nearest_src(x, sw, dw);
    for (int c = 0; c < C; ++c) dst[idx * C + c] = src[(((int64_t)n * sh + sy) * sw + sx) * C + c];
  }
}

__global__ void f32_to_h16_kernel(const float* __restrict__ x, h16* __restrict__ y, int64_t n) {
  GRID_STRIDE(i, n) y[i] = (h16)x[i];
}
// the same, 8 elements (two 16-byte loads, one 16-byte store) per thread and trip: the 16-bit copy of the VAE's f32 stream
__global__ void f32_to_h16_x8_kernel(const float* __restrict__ x, h16* __restrict__ y, int64_t n8) {
  GRID_STRIDE(i, n8) {
    const float4 a = ((const float4*)x)[2 * i], b = ((const float4*)x)[2 * i + 1];
    h16x8 o;
    o[0] = (h16)a.x; o[1] = (h16)a.y; o[2] = (h16)a.z; o[3] = (h16)a.w;
    o[4] = (h16)b.x; o[5] = (h16)b.y; o[6] = (h16)b.z; o[7] = (h16)b.w;
    ((h16x8*)y)[i] = o;
  }
}
__global__ void h16_to_f32_kernel(const h16* __restrict__ x, float* __restrict__ y, int64_t n) {
  GRID_STRIDE(i, n) y[i] = (float)x[i];
}
__global__ void silu_kernel(const h16* __restrict__ x, h16* __restrict__ y, int64_t n) {
  GRID_STRIDE(i, n) { float f = (float)x[i]; y[i] = (h16)(f / (1.f + __expf(-f))); }
}

// diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]
__global__ void timestep_embed_kernel(const float* __restrict__ t, h16* __restrict__ out, int N, int dim) {
  const int half = dim / 2;
  const int64_t total = (int64_t)N * half;
  GRID_STRIDE(idx, total) {
    const int i = (int)(idx % half);
    const int n = (int)(idx / half);
    const float freq = expf(-logf(10000.f) * (float)i / (float)half);
    const float a = t[n] * freq;
    out[(int64_t)n * dim + i] = (h16)cosf(a);
    out[(int64_t)n * dim + half + i] = (h16)sinf(a);
  }
}

// DDIMScheduler.step (eta 0, clip_sample) with the classifier-free-guidance combine in front
// (sd_utils.py:256-260)
__global__ void ddim_step_kernel(const float* __restrict__ z, const float* __restrict__ eu, const float* __restrict__ ec, float guidance,
                                 float* __restrict__ zo, int64_t n, float sa, float s1a, float sap, float s1ap) {
  GRID_STRIDE(i, n) {
    float e = eu[i];
    if (ec) e = e + guidance * (ec[i] - e);
    float x0 = (z[i] - s1a * e) / sa;
    x0 = fminf(fmaxf(x0, -1.f), 1.f);
    zo[i] = sap * x0 + s1ap * e;
  }
}
// The same step with its scalars read from a device table row chosen by a device counter, so that a captured graph of one DDIM
// step replays for every timestep without new kernel arguments: tab[i] = {t, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)}
__global__ void ddim_step_tab_kernel(const float* __restrict__ z, const float* __restrict__ eu, const float* __restrict__ ec, float guidance,
                                     float* __restrict__ zo, int64_t n, const float* __restrict__ tab, const int* __restrict__ idx) {
  const float* r = tab + 5 * idx[0];
  const float sa = r[1], s1a = r[2], sap = r[3], s1ap = r[4];
  GRID_STRIDE(i, n) {
    float e = eu[i];
    if (ec) e = e + guidance * (ec[i] - e);
    float x0 = (z[i] - s1a * e) / sa;
    x0 = fminf(fmaxf(x0, -1.f), 1.f);
    zo[i] = sap * x0 + s1ap * e;
  }
}
__global__ void ddim_tvec_kernel(float* __restrict__ tvec, int nb, const float* __restrict__ tab, int row, const int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) tvec[i] = tab[row * idx[0]];
}
// DPM-Solver++(2M) (diffusers DPMSolverMultistepScheduler: dpmsolver++, order 2, midpoint, no thresholding) with the CFG combine in
// front: m = (x - sig_s e) / a_s;  D = m + k (m - m_prev) (k = 1 / 2r, 0 at first order);  x' = last ? m : cx x + cd D;  m_prev <- m.
// x / x_out and m_prev / m_out may alias (in-place loop): every element is read before it is written, by the same thread, so those
// pointers are deliberately not __restrict__.  m_prev is not read at first order (k == 0): it may be null or uninitialised then.
__device__ __forceinline__ void dpmpp_elem(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance,
                                           const float* mp, float* xo, float* mo, int64_t i, float inv_a, float sig, float cx, float cd,
                                           float k, bool last) {
  float e = eu[i];
  if (ec) e = e + guidance * (ec[i] - e);
  const float xi = x[i];
  const float m = (xi - sig * e) * inv_a;
  float d = m;
  if (k != 0.f) d = m + k * (m - mp[i]);
  const float out = last ? m : cx * xi + cd * d;
  if (mo) mo[i] = m;
  xo[i] = out;
}
__global__ void dpmpp_step_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, const float* mp,
                                  float* xo, float* mo, int64_t n, float inv_a, float sig, float cx, float cd, float k, int last) {
  GRID_STRIDE(i, n) dpmpp_elem(x, eu, ec, guidance, mp, xo, mo, i, inv_a, sig, cx, cd, k, last != 0);
}
// the same step with its row read from a device table through the DDIM loop's step counter: tab[i] = kDpmRow floats
// {t, 1/a_s, sig_s, sig_s'/sig_s, a_s'(1 - e^-h), 1/2r, last, 0}
__global__ void dpmpp_step_tab_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, const float* mp,
                                      float* xo, float* mo, int64_t n, const float* __restrict__ tab, const int* __restrict__ idx) {
  const float* r = tab + kDpmRow * idx[0];
  const float inv_a = r[1], sig = r[2], cx = r[3], cd = r[4], k = r[5];
  const bool last = r[6] != 0.f;
  GRID_STRIDE(i, n) dpmpp_elem(x, eu, ec, guidance, mp, xo, mo, i, inv_a, sig, cx, cd, k, last);
}
// LMS (diffusers 0.2.3 LMSDiscreteScheduler.step, order <= 4) with the CFG combine in front.  The derivative of step i is the
// combined eps itself ((x - (x - sigma eps)) / sigma up to f32 rounding); it goes to slot i & 3 of the ring dh (4 x n floats), the
// up to three older ones come from the slots (i-1) & 3 ... (i-3) & 3, never the slot written:  x' = x + sum_k c_k d_{i-k}, k < order.
// W = 4: one 16-byte access per operand, W = 1: the scalar tail.  x / x_out may alias (read before written by the same thread).
// Every product is an explicit fmaf, so that the tabled, the direct, the 16-byte and the scalar form round alike.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int W> struct LmsVec { typedef float T; };
template <> struct LmsVec<4> { typedef f32x4 T; };
template <int W>
__device__ __forceinline__ void lms_elem(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, float* dh,
                                         float* xo, int64_t n, int64_t i, int slot, int order, float c0, float c1, float c2, float c3) {
  typedef typename LmsVec<W>::T V;
  const V xv = *(const V*)(x + i);
  V e = *(const V*)(eu + i);
  if (ec) e = __builtin_elementwise_fma(V(guidance), *(const V*)(ec + i) - e, e);
  *(V*)(dh + (int64_t)slot * n + i) = e;
  V acc = V(c0) * e;
  if (order > 1) acc = __builtin_elementwise_fma(V(c1), *(const V*)(dh + (int64_t)((slot + 3) & 3) * n + i), acc);
  if (order > 2) acc = __builtin_elementwise_fma(V(c2), *(const V*)(dh + (int64_t)((slot + 2) & 3) * n + i), acc);
  if (order > 3) acc = __builtin_elementwise_fma(V(c3), *(const V*)(dh + (int64_t)((slot + 1) & 3) * n + i), acc);
  *(V*)(xo + i) = xv + acc;
}
// nv: the number of 4-float groups taken with 16-byte accesses (0 when n % 4 or a pointer forbids them); the rest is the scalar tail
__global__ void lms_step_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, float* dh, float* xo,
                                int64_t n, int64_t nv, int slot, int order, float c0, float c1, float c2, float c3) {
  GRID_STRIDE(v, nv) lms_elem<4>(x, eu, ec, guidance, dh, xo, n, 4 * v, slot, order, c0, c1, c2, c3);
  GRID_STRIDE(j, n - 4 * nv) lms_elem<1>(x, eu, ec, guidance, dh, xo, n, 4 * nv + j, slot, order, c0, c1, c2, c3);
}
// the same step with its row read from a device table through the loop's step counter: tab[i] = kLmsRow floats
// {t, 1/sqrt(sigma_i^2 + 1), order, i, c0, c1, c2, c3}; the ring slot follows from i, so a replayed graph needs no new arguments
__global__ void lms_step_tab_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, float* dh,
                                    float* xo, int64_t n, int64_t nv, const float* __restrict__ tab, const int* __restrict__ idx) {
  const float* r = tab + kLmsRow * idx[0];
  const int order = (int)r[2], slot = (int)r[3] & 3;
  const float c0 = r[4], c1 = r[5], c2 = r[6], c3 = r[7];
  GRID_STRIDE(v, nv) lms_elem<4>(x, eu, ec, guidance, dh, xo, n, 4 * v, slot, order, c0, c1, c2, c3);
  GRID_STRIDE(j, n - 4 * nv) lms_elem<1>(x, eu, ec, guidance, dh, xo, n, 4 * nv + j, slot, order, c0, c1, c2, c3);
}
// the UNet input of an LMS step: o0 (and o1, the second half of a guided batch) <- x * c, c = 1 / sqrt(sigma_i^2 + 1)
template <int W>
__device__ __forceinline__ void lms_input_elem(const float* x, float* o0, float* o1, int64_t i, float c) {
  typedef typename LmsVec<W>::T V;
  const V v = *(const V*)(x + i) * V(c);
  *(V*)(o0 + i) = v;
  if (o1) *(V*)(o1 + i) = v;
}
__global__ void lms_input_kernel(const float* x, float* o0, float* o1, int64_t n, int64_t nv, float c) {
  GRID_STRIDE(v, nv) lms_input_elem<4>(x, o0, o1, 4 * v, c);
  GRID_STRIDE(j, n - 4 * nv) lms_input_elem<1>(x, o0, o1, 4 * nv + j, c);
}
__global__ void lms_input_tab_kernel(const float* x, float* o0, float* o1, int64_t n, int64_t nv, const float* __restrict__ tab,
                                     const int* __restrict__ idx) {
  const float c = tab[kLmsRow * idx[0] + 1];
  GRID_STRIDE(v, nv) lms_input_elem<4>(x, o0, o1, 4 * v, c);
  GRID_STRIDE(j, n - 4 * nv) lms_input_elem<1>(x, o0, o1, 4 * nv + j, c);
}
__global__ void ddim_bump_kernel(int* __restrict__ idx) { idx[0] += 1; }
__global__ void add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ nz, float* __restrict__ out, int64_t n, float sa, float s1a) {
  GRID_STRIDE(i, n) out[i] = sa * x0[i] + s1a * nz[i];
}

}  // namespace

void img_to_act(const uint8_t* img, h16* out, int N, int sh, int sw, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(img_to_act_kernel, grid_for((int64_t)N * H * W), dim3(256), 0, s, img, out, N, sh, sw, H, W);
  check_launch("img_to_act");
}
void act_to_img(const float* x, int ldc, uint8_t* img, float* fout, int N, int h, int w, int oh, int ow, hipStream_t s) {
  hipLaunchKernelGGL(act_to_img_kernel, grid_for((int64_t)N * std::max(h * w, oh * ow)), dim3(256), 0, s, x, ldc, img, fout, N, h, w, oh, ow);
  check_launch("act_to_img");
}
void nchw_to_act(const float* x, h16* out, int N, int C, int h, int w, int Cpad, float scale, hipStream_t s) {
  hipLaunchKernelGGL(nchw_to_act_kernel, grid_for((int64_t)N * h * w), dim3(256), 0, s, x, out, N, C, h * w, Cpad, scale);
  check_launch("nchw_to_act");
}
void nchw_to_actf32(const float* x, float* out, int N, int C, int h, int w, float scale, hipStream_t s) {
  hipLaunchKernelGGL(nchw_to_actf32_kernel, grid_for((int64_t)N * h * w), dim3(256), 0, s, x, out, N, C, h * w, scale);
  check_launch("nchw_to_actf32");
}
void actf32_pad_h16(const float* x, int C, h16* out, int Cpad, int64_t P, hipStream_t s) {
  hipLaunchKernelGGL(actf32_pad_h16_kernel, grid_for(P), dim3(256), 0, s, x, C, out, Cpad, P);
  check_launch("actf32_pad_h16");
}
void actf32_to_nchw(const float* x, int ld, float* out, int N, int C, int h, int w, hipStream_t s) {
  hipLaunchKernelGGL(actf32_to_nchw_kernel, grid_for((int64_t)N * h * w), dim3(256), 0, s, x, ld, out, N, C, h * w);
  check_launch("actf32_to_nchw");
}
void pixel_linear_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int64_t P, int Cin, int Cout, hipStream_t s) {
  SVG_CHECK(Cin <= 8, "pixel_linear: Cin %d > 8", Cin);
  hipLaunchKernelGGL(pixel_linear_kernel, grid_for(P), dim3(256), 0, s, x, ldx, w, b, y, ldy, P, Cin, Cout);
  check_launch("pixel_linear");
}
void vae_sample(const float* mom, int ldm, const float* eps, float* z, float* mom_nchw, int N, int h, int w, hipStream_t s) {
  hipLaunchKernelGGL(vae_sample_kernel, grid_for((int64_t)N * h * w), dim3(256), 0, s, mom, ldm, eps, z, mom_nchw, N, h * w);
  check_launch("vae_sample");
}
void concat_channels(const h16* a, int Ca, const h16* b, int Cb, h16* out, int64_t P, hipStream_t s) {
  SVG_CHECK(Ca % 8 == 0 && Cb % 8 == 0, "concat: channels must be multiples of 8");
  hipLaunchKernelGGL(concat_kernel, grid_for(P * ((Ca + Cb) / 8)), dim3(256), 0, s, a, Ca, b, Cb, out, P);
  check_launch("concat");
}
// f32 planes (P, h, w) -> (P, oh, ow), bilinear with torch's align_corners=False convention (F.interpolate(mode='bilinear')):
// src = max((dst + 0.5) * in / out - 0.5, 0), the upper neighbour clamped to the last row / column
static __global__ void resize_bilinear_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int P, int h, int w, int oh, int ow) {
  const int64_t total = (int64_t)P * oh * ow;
  const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % ow), y = (int)((i / ow) % oh);
    const int64_t p = i / ((int64_t)ow * oh);
    const float fy = fmaxf(((float)y + 0.5f) * sy - 0.5f, 0.f), fx = fmaxf(((float)x + 0.5f) * sx - 0.5f, 0.f);
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float* s = src + p * h * w;
    const float top = s[y0 * w + x0] * (1.f - lx) + s[y0 * w + x1] * lx;
    const float bot = s[y1 * w + x0] * (1.f - lx) + s[y1 * w + x1] * lx;
    dst[i] = top * (1.f - ly) + bot * ly;
  }
}

void resize_bilinear_f32(const float* src, float* dst, int P, int h, int w, int oh, int ow, hipStream_t s) {
  const int64_t total = (int64_t)P * oh * ow;
  hipLaunchKernelGGL(resize_bilinear_f32_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, src, dst, P, h, w, oh, ow);
  check_launch("resize_bilinear_f32");
}

void resize_nearest_u8(const uint8_t* src, uint8_t* dst, int N, int sh, int sw, int C, int dh, int dw, hipStream_t s) {
  hipLaunchKernelGGL(resize_u8_kernel, grid_for((int64_t)N * dh * dw), dim3(256), 0, s, src, dst, N, sh, sw, C, dh, dw);
  check_launch("resize_u8");
}
void f32_to_h16(const float* x, h16* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_h16_kernel, grid_for(n), dim3(256), 0, s, x, y, n);
  check_launch("f32_to_h16");
}
void f32_to_h16_x8(const float* x, h16* y, int64_t n, hipStream_t s) {
  SVG_CHECK(n % 8 == 0 && ((uintptr_t)x & 31) == 0 && ((uintptr_t)y & 15) == 0, "f32_to_h16_x8: n %% 8 and 32 / 16-byte aligned pointers");
  hipLaunchKernelGGL(f32_to_h16_x8_kernel, grid_for(n / 8), dim3(256), 0, s, x, y, n / 8);
  check_launch("f32_to_h16_x8");
}
void h16_to_f32(const h16* x, float* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(h16_to_f32_kernel, grid_for(n), dim3(256), 0, s, x, y, n);
  check_launch("h16_to_f32");
}
void silu_h16(const h16* x, h16* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(silu_kernel, grid_for(n), dim3(256), 0, s, x, y, n);
  check_launch("silu");
}
void timestep_embed(const float* t, h16* out, int N, int dim, hipStream_t s) {
  hipLaunchKernelGGL(timestep_embed_kernel, grid_for((int64_t)N * dim / 2), dim3(256), 0, s, t, out, N, dim);
  check_launch("timestep_embed");
}
void ddim_step(const float* z, const float* eu, const float* ec, float guidance, float* zo, int64_t n, float sa, float s1a,
               float sap, float s1ap, hipStream_t s) {
  hipLaunchKernelGGL(ddim_step_kernel, grid_for(n), dim3(256), 0, s, z, eu, ec, guidance, zo, n, sa, s1a, sap, s1ap);
  check_launch("ddim_step");
}
void ddim_step_tab(const float* z, const float* eu, const float* ec, float guidance, float* zo, int64_t n, const float* tab, const int* idx,
                   hipStream_t s) {
  hipLaunchKernelGGL(ddim_step_tab_kernel, grid_for(n), dim3(256), 0, s, z, eu, ec, guidance, zo, n, tab, idx);
  check_launch("ddim_step_tab");
}
void ddim_tvec(float* tvec, int nb, const float* tab, const int* idx, hipStream_t s, int row) {
  hipLaunchKernelGGL(ddim_tvec_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, tvec, nb, tab, row, idx);
  check_launch("ddim_tvec");
}
void dpmpp_step(const float* x, const float* eu, const float* ec, float guidance, const float* m_prev, float* x_out, float* m_out, int64_t n,
                const float* row, hipStream_t s) {
  SVG_CHECK(m_prev || row[5] == 0.f, "dpmpp_step: a second-order step needs m_prev");
  hipLaunchKernelGGL(dpmpp_step_kernel, grid_for(n), dim3(256), 0, s, x, eu, ec, guidance, m_prev, x_out, m_out, n, row[1], row[2], row[3],
                     row[4], row[5], row[6] != 0.f ? 1 : 0);
  check_launch("dpmpp_step");
}
void dpmpp_step_tab(const float* x, const float* eu, const float* ec, float guidance, float* m, float* x_out, int64_t n, const float* tab,
                    const int* idx, hipStream_t s) {
  hipLaunchKernelGGL(dpmpp_step_tab_kernel, grid_for(n), dim3(256), 0, s, x, eu, ec, guidance, m, x_out, m, n, tab, idx);
  check_launch("dpmpp_step_tab");
}
namespace {
// 4-float groups an LMS kernel may take with 16-byte accesses: all of them when every pointer it indexes is 16-byte aligned
// (`stride4`: the kernel also indexes p + k * n, so n % 4 must be 0 too), else none
inline int64_t lms_groups(int64_t n, bool stride4, std::initializer_list<const void*> ptrs) {
  if (stride4 && n % 4 != 0) return 0;
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return 0;
  return n / 4;
}
inline dim3 lms_grid(int64_t n, int64_t nv) { return grid_for(std::max<int64_t>(nv, n - 4 * nv)); }
}  // namespace
void lms_input(const float* x, float* o0, float* o1, int64_t n, float c, hipStream_t s) {
  const int64_t nv = lms_groups(n, false, {x, o0, o1});
  hipLaunchKernelGGL(lms_input_kernel, lms_grid(n, nv), dim3(256), 0, s, x, o0, o1, n, nv, c);
  check_launch("lms_input");
}
void lms_input_tab(const float* x, float* o0, float* o1, int64_t n, const float* tab, const int* idx, hipStream_t s) {
  const int64_t nv = lms_groups(n, false, {x, o0, o1});
  hipLaunchKernelGGL(lms_input_tab_kernel, lms_grid(n, nv), dim3(256), 0, s, x, o0, o1, n, nv, tab, idx);
  check_launch("lms_input_tab");
}
void lms_step(const float* x, const float* eu, const float* ec, float guidance, float* dhist, float* x_out, int64_t n, int i, int order,
              const float* c, hipStream_t s) {
  SVG_CHECK(i >= 0 && order >= 1 && order <= 4 && order <= i + 1, "lms_step: order %d at step %d", order, i);
  const int64_t nv = lms_groups(n, true, {x, eu, ec, dhist, x_out});
  hipLaunchKernelGGL(lms_step_kernel, lms_grid(n, nv), dim3(256), 0, s, x, eu, ec, guidance, dhist, x_out, n, nv, i & 3, order, c[0], c[1],
                     c[2], c[3]);
  check_launch("lms_step");
}
void lms_step_tab(const float* x, const float* eu, const float* ec, float guidance, float* dhist, float* x_out, int64_t n, const float* tab,
                  const int* idx, hipStream_t s) {
  const int64_t nv = lms_groups(n, true, {x, eu, ec, dhist, x_out});
  hipLaunchKernelGGL(lms_step_tab_kernel, lms_grid(n, nv), dim3(256), 0, s, x, eu, ec, guidance, dhist, x_out, n, nv, tab, idx);
  check_launch("lms_step_tab");
}
void ddim_bump(int* idx, hipStream_t s) {
  hipLaunchKernelGGL(ddim_bump_kernel, dim3(1), dim3(1), 0, s, idx);
  check_launch("ddim_bump");
}

namespace {
__global__ void fill_f32_kernel(float* __restrict__ p, int64_t n, float v) {
  GRID_STRIDE(i, n) p[i] = v;
}
}  // namespace
void fill_f32(float* p, int64_t n, float v, hipStream_t s) {
  hipLaunchKernelGGL(fill_f32_kernel, grid_for(n), dim3(256), 0, s, p, n, v);
  check_launch("fill_f32");
}
void add_noise(const float* x0, const float* nz, float* out, int64_t n, float sa, float s1a, hipStream_t s) {
  hipLaunchKernelGGL(add_noise_kernel, grid_for(n), dim3(256), 0, s, x0, nz, out, n, sa, s1a);
  check_launch("add_noise");
}

}  // namespace SDNS
