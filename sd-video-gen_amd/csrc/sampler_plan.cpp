// Schedule plan of the sampling loop (sampler_plan.h).  Pure host code: no HIP runtime call, no kernel, no environment lookup.
#include "sampler_plan.h"
#include "common.h"
#include <algorithm>
#include <cmath>

// ---- DDIM table, as diffusers' DDIMScheduler builds it: betas = linspace(sqrt(b0), sqrt(b1), 1000, f32)**2,
// alphas_cumprod = cumprod(1 - betas) in f32
const std::vector<float>& sd_alphas_cumprod() {
  static const std::vector<float> table = [] {
    std::vector<float> alphas_cumprod(1000);
    const double b0 = sqrt(0.00085), b1 = sqrt(0.012);
    float prod = 1.f;
    for (int i = 0; i < 1000; ++i) {
      const double step = (b1 - b0) / 999.0;
      float sb = (float)(i * step + b0);
      if (i == 999) sb = (float)b1;
      float beta = sb * sb;
      float alpha = 1.f - beta;
      prod = prod * alpha;
      alphas_cumprod[i] = prod;
    }
    return alphas_cumprod;
  }();
  return table;
}

void ddim_coefs(int t, int t_prev, float* row) {
  SVG_CHECK(t >= 0 && t < 1000, "ddim: timestep %d out of range", t);
  const std::vector<float>& alphas_cumprod = sd_alphas_cumprod();
  const float a_t = alphas_cumprod[t];
  const float a_p = (t_prev >= 0) ? alphas_cumprod[t_prev] : 1.0f;   // set_alpha_to_one
  for (int j = 0; j < kSamplerRow; ++j) row[j] = 0.f;
  row[0] = (float)t;
  row[1] = sqrtf(a_t); row[2] = sqrtf(1.f - a_t); row[3] = sqrtf(a_p); row[4] = sqrtf(1.f - a_p);
}

// DPM-Solver++(2M) on the DDIM timestep set, in double from the f32 alphas_cumprod: with a = sqrt(abar), sig = sqrt(1 - abar),
// lambda = log a - log sig and h = lambda_s' - lambda_s:  x' = (sig_s'/sig_s) x + a_s'(1 - e^-h) D,  D = m + (m - m_prev) / 2r,
// r = (lambda_s - lambda_last) / h (D = m at first order);  sig_s' == 0 (t_next < 0, set_alpha_to_one) is the final step: x' = m.
void dpmpp_coefs(int t, int t_next, int t_last, float* row) {
  SVG_CHECK(t >= 0 && t < 1000 && t_next < t, "dpmpp: timesteps %d -> %d out of range", t, t_next);
  SVG_CHECK(t_last < 0 || (t_last > t && t_last < 1000), "dpmpp: previous timestep %d is not in (%d, 1000)", t_last, t);
  const std::vector<float>& alphas_cumprod = sd_alphas_cumprod();
  auto lam = [](double ab) { return 0.5 * log(ab) - 0.5 * log1p(-ab); };
  const double ab = alphas_cumprod[t];
  const double a = sqrt(ab), sig = sqrt(1.0 - ab);
  for (int j = 0; j < kSamplerRow; ++j) row[j] = 0.f;
  row[0] = (float)t;
  row[1] = (float)(1.0 / a);
  row[2] = (float)sig;
  if (t_next < 0) {                 // lower_order_final: x' = m
    row[6] = 1.f;
    return;
  }
  const double abn = alphas_cumprod[t_next];
  const double h = lam(abn) - lam(ab);
  row[3] = (float)(sqrt(1.0 - abn) / sig);
  row[4] = (float)(-sqrt(abn) * expm1(-h));
  if (t_last >= 0) {
    const double r = (lam(ab) - lam(alphas_cumprod[t_last])) / h;
    row[5] = (float)(0.5 / r);
  }
}

// The LMS schedule in double from the f32 alphas_cumprod.  The coefficient c_k integrates the Lagrange basis polynomial
// prod_{j != k} (tau - sigma_{i-j}) / (sigma_{i-k} - sigma_{i-j}) (degree <= 3) over [sigma_i, sigma_{i+1}]: expanded in
// u = tau - sigma_i (roots r_j = sigma_{i-j} - sigma_i, so nothing of the size of sigma^4 is subtracted) and integrated term by
// term over [0, sigma_{i+1} - sigma_i] -- exact up to rounding, where diffusers runs scipy.integrate.quad(epsrel = 1e-4).
void lms_coefs(int num_steps, int i, LmsCoef* out) {
  SVG_CHECK(num_steps >= 1 && num_steps <= 1000 && i >= 0 && i < num_steps, "lms: step %d of %d out of range", i, num_steps);
  const std::vector<float>& abar = sd_alphas_cumprod();
  // numpy.linspace(999, 0, n): arange(n) * (-999 / (n - 1)) + 999 with the last element set to 0 (and [999] for n = 1)
  auto timestep = [&](int j) -> double {
    if (num_steps == 1) return 999.0;
    if (j == num_steps - 1) return 0.0;
    const double step = -999.0 / (num_steps - 1);
    volatile double prod = j * step;      // rounded on its own, as numpy does (never a fused multiply-add)
    return prod + 999.0;
  };
  auto sigma_at = [&](int j) -> double {
    if (j >= num_steps) return 0.0;
    const double t = timestep(j);
    const int lo = (int)floor(t), hi = (int)ceil(t);
    const double fr = t - floor(t);
    auto train = [&](int k) { const double a = abar[k]; return sqrt((1.0 - a) / a); };
    return (1.0 - fr) * train(lo) + fr * train(hi);
  };
  out->t = timestep(i);
  out->sigma = sigma_at(i);
  out->sigma_next = sigma_at(i + 1);
  out->order = std::min(i + 1, 4);
  const double h = out->sigma_next - out->sigma;
  double r[4];
  for (int j = 0; j < out->order; ++j) r[j] = sigma_at(i - j) - out->sigma;
  for (int k = 0; k < 4; ++k) out->c[k] = 0.0;
  for (int k = 0; k < out->order; ++k) {
    double p[4] = {1.0, 0.0, 0.0, 0.0};    // prod_{j != k} (u - r_j), ascending powers of u
    int deg = 0;
    double den = 1.0;
    for (int j = 0; j < out->order; ++j) {
      if (j == k) continue;
      for (int m = ++deg; m > 0; --m) p[m] = p[m - 1] - r[j] * p[m];
      p[0] = -r[j] * p[0];
      den *= r[k] - r[j];
    }
    double integral = 0.0;
    for (int m = deg; m >= 0; --m) integral = integral * h + p[m] / (m + 1);   // sum_m p_m h^m / (m + 1)
    out->c[k] = integral * h / den;
  }
}

void lms_row(const LmsCoef& lc, int i, float* r) {
  r[0] = (float)lc.t; r[1] = (float)(1.0 / sqrt(lc.sigma * lc.sigma + 1.0)); r[2] = (float)lc.order; r[3] = (float)i;
  for (int k = 0; k < 4; ++k) r[4 + k] = (float)lc.c[k];
}

SamplerPlan sampler_plan(int sampler, int num_steps, int start_step) {
  SVG_CHECK(sampler == kSamplerDdim || sampler == kSamplerDpmpp2m || sampler == kSamplerLms, "sample_loop: unknown sampler %d", sampler);
  const bool dpm = sampler == kSamplerDpmpp2m, lms = sampler == kSamplerLms;
  SVG_CHECK(num_steps >= 1 && num_steps <= 1000 && start_step >= 0 && start_step <= num_steps, "ddim: bad steps %d/%d", start_step, num_steps);
  SVG_CHECK(!lms || start_step == 0, "lms: start_step must be 0 (got %d): the multistep rule has no history to start from", start_step);
  SamplerPlan p;
  p.sampler = sampler; p.num_steps = num_steps; p.start_step = start_step;
  p.scaled_input = lms;
  p.state_buffers = lms ? 4 : dpm ? 1 : 0;
  p.table.resize((size_t)kSamplerRow * num_steps);
  const int ratio = 1000 / num_steps;
  auto timestep_at = [&](int i) { return (num_steps - 1 - i) * ratio; };   // (arange(n)*ratio)[::-1]
  for (int i = 0; i < num_steps; ++i) {
    float* row = &p.table[(size_t)kSamplerRow * i];
    const int t = timestep_at(i);
    if (lms) {
      LmsCoef lc;
      lms_coefs(num_steps, i, &lc);
      lms_row(lc, i, row);
      if (i == 0) p.z_scale = (float)lc.sigma;
    } else if (dpm) {
      dpmpp_coefs(t, t - ratio, i > start_step ? timestep_at(i - 1) : -1, row);
    } else {
      ddim_coefs(t, t - ratio, row);
    }
  }
  if (start_step > 0 && start_step < num_steps) {
    const float a = sd_alphas_cumprod()[timestep_at(start_step)];
    p.add_noise = true;
    p.noise_sa = sqrtf(a); p.noise_s1a = sqrtf(1.f - a);
  }
  return p;
}
