// Update kernels of the sampling loop: one kernel per rule, its scalars one row of the schedule plan (sampler_plan.h).
#include "sampler.h"
#include <algorithm>
#include <initializer_list>

namespace {

#define GRID_STRIDE(idx, total) \
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (total); idx += (int64_t)gridDim.x * blockDim.x)

inline dim3 grid_for(int64_t total) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192))); }

// the row of this launch, selected once before the element loop: the table row under the loop's step counter, or the argument itself
__device__ __forceinline__ SamplerRowArg row_of(SamplerRowArg a) {
  if (a.tab)
    for (int j = 0; j < kSamplerRow; ++j) a.v[j] = a.tab[kSamplerRow * a.idx[0] + j];
  return a;
}

// DDIMScheduler.step (eta 0, clip_sample) with the classifier-free-guidance combine in front
// (sd_utils.py:256-260)
__device__ __forceinline__ void ddim_elem(const float* __restrict__ z, const float* __restrict__ eu, const float* __restrict__ ec, float guidance,
                                          float* __restrict__ zo, int64_t i, float sa, float s1a, float sap, float s1ap) {
  float e = eu[i];
  if (ec) e = e + guidance * (ec[i] - e);
  float x0 = (z[i] - s1a * e) / sa;
  x0 = fminf(fmaxf(x0, -1.f), 1.f);
  zo[i] = sap * x0 + s1ap * e;
}
__global__ void ddim_step_kernel(const float* __restrict__ z, const float* __restrict__ eu, const float* __restrict__ ec, float guidance,
                                 float* __restrict__ zo, int64_t n, const SamplerRowArg row) {
  const SamplerRowArg r = row_of(row);
  const float sa = r.v[1], s1a = r.v[2], sap = r.v[3], s1ap = r.v[4];
  GRID_STRIDE(i, n) ddim_elem(z, eu, ec, guidance, zo, i, sa, s1a, sap, s1ap);
}
__global__ void sampler_tvec_kernel(float* __restrict__ tvec, int nb, const float* __restrict__ tab, const int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) tvec[i] = tab[kSamplerRow * idx[0]];
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
                                  float* xo, float* mo, int64_t n, const SamplerRowArg row) {
  const SamplerRowArg r = row_of(row);
  const float inv_a = r.v[1], sig = r.v[2], cx = r.v[3], cd = r.v[4], k = r.v[5];
  const bool last = r.v[6] != 0.f;
  GRID_STRIDE(i, n) dpmpp_elem(x, eu, ec, guidance, mp, xo, mo, i, inv_a, sig, cx, cd, k, last);
}
// LMS (diffusers 0.2.3 LMSDiscreteScheduler.step, order <= 4) with the CFG combine in front.  The derivative of step i is the
// combined eps itself ((x - (x - sigma eps)) / sigma up to f32 rounding); it goes to slot i & 3 of the ring dh (4 x n floats), the
// up to three older ones come from the slots (i-1) & 3 ... (i-3) & 3, never the slot written:  x' = x + sum_k c_k d_{i-k}, k < order.
// W = 4: one 16-byte access per operand, W = 1: the scalar tail.  x / x_out may alias (read before written by the same thread).
// Every product is an explicit fmaf, so that the 16-byte and the scalar form round alike.
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
// nv: the number of 4-float groups taken with 16-byte accesses (0 when n % 4 or a pointer forbids them); the rest is the scalar tail.
// The ring slot follows from the row's i, so a replayed graph needs no new arguments.
__global__ void lms_step_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float guidance, float* dh, float* xo,
                                int64_t n, int64_t nv, const SamplerRowArg row) {
  const SamplerRowArg r = row_of(row);
  const int order = (int)r.v[2], slot = (int)r.v[3] & 3;
  const float c0 = r.v[4], c1 = r.v[5], c2 = r.v[6], c3 = r.v[7];
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
__global__ void lms_input_kernel(const float* x, float* o0, float* o1, int64_t n, int64_t nv, const SamplerRowArg row) {
  const float c = row_of(row).v[1];
  GRID_STRIDE(v, nv) lms_input_elem<4>(x, o0, o1, 4 * v, c);
  GRID_STRIDE(j, n - 4 * nv) lms_input_elem<1>(x, o0, o1, 4 * nv + j, c);
}
__global__ void sampler_bump_kernel(int* __restrict__ idx) { idx[0] += 1; }
__global__ void add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ nz, float* __restrict__ out, int64_t n, float sa, float s1a) {
  GRID_STRIDE(i, n) out[i] = sa * x0[i] + s1a * nz[i];
}

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

void sampler_tvec(float* tvec, int nb, const float* tab, const int* idx, hipStream_t s) {
  hipLaunchKernelGGL(sampler_tvec_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, tvec, nb, tab, idx);
  check_launch("sampler_tvec");
}
void sampler_bump(int* idx, hipStream_t s) {
  hipLaunchKernelGGL(sampler_bump_kernel, dim3(1), dim3(1), 0, s, idx);
  check_launch("sampler_bump");
}
void ddim_step(const float* z, const float* eu, const float* ec, float guidance, float* zo, int64_t n, const SamplerRowArg& row, hipStream_t s) {
  hipLaunchKernelGGL(ddim_step_kernel, grid_for(n), dim3(256), 0, s, z, eu, ec, guidance, zo, n, row);
  check_launch("ddim_step");
}
void dpmpp_step(const float* x, const float* eu, const float* ec, float guidance, const float* m_prev, float* x_out, float* m_out, int64_t n,
                const SamplerRowArg& row, hipStream_t s) {
  SVG_CHECK(m_prev || row.tab || row.v[5] == 0.f, "dpmpp_step: a second-order step needs m_prev");
  hipLaunchKernelGGL(dpmpp_step_kernel, grid_for(n), dim3(256), 0, s, x, eu, ec, guidance, m_prev, x_out, m_out, n, row);
  check_launch("dpmpp_step");
}
void lms_input(const float* x, float* o0, float* o1, int64_t n, const SamplerRowArg& row, hipStream_t s) {
  const int64_t nv = lms_groups(n, false, {x, o0, o1});
  hipLaunchKernelGGL(lms_input_kernel, lms_grid(n, nv), dim3(256), 0, s, x, o0, o1, n, nv, row);
  check_launch("lms_input");
}
void lms_step(const float* x, const float* eu, const float* ec, float guidance, float* dhist, float* x_out, int64_t n, const SamplerRowArg& row,
              hipStream_t s) {
  if (!row.tab) {
    const int order = (int)row.v[2], i = (int)row.v[3];
    SVG_CHECK(i >= 0 && order >= 1 && order <= 4 && order <= i + 1, "lms_step: order %d at step %d", order, i);
  }
  const int64_t nv = lms_groups(n, true, {x, eu, ec, dhist, x_out});
  hipLaunchKernelGGL(lms_step_kernel, lms_grid(n, nv), dim3(256), 0, s, x, eu, ec, guidance, dhist, x_out, n, nv, row);
  check_launch("lms_step");
}
void sampler_step(int sampler, float* z, const float* eu, const float* ec, float guidance, float* state, int64_t n, const SamplerRowArg& row,
                  hipStream_t s) {
  if (sampler == kSamplerLms) lms_step(z, eu, ec, guidance, state, z, n, row, s);
  else if (sampler == kSamplerDpmpp2m) dpmpp_step(z, eu, ec, guidance, state, z, state, n, row, s);
  else ddim_step(z, eu, ec, guidance, z, n, row, s);
}
void add_noise(const float* x0, const float* nz, float* out, int64_t n, float sa, float s1a, hipStream_t s) {
  hipLaunchKernelGGL(add_noise_kernel, grid_for(n), dim3(256), 0, s, x0, nz, out, n, sa, s1a);
  check_launch("add_noise");
}
