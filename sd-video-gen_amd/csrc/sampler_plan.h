// The schedule plan of the sampling loop (sampler_plan.cpp: no HIP runtime call, no kernel).  Every scalar a step of DDIM, DPM-Solver++(2M)
// or LMS needs is one row of kSamplerRow floats; sampler_plan() builds the rows of a whole loop once, UnetModel::sample_loop uploads them for
// the replayed step graph and hands the same rows to the direct launches, and the one-shot entry points (svg_ddim_step, svg_dpmpp_step,
// svg_lms_step) build a single row with the same functions.  Pure functions of their arguments, so the rows can be dumped and pinned on a
// machine without a GPU (tools/host_sanitize/sampler_plan_dump.cpp, tests/test_sampler_plan_cpu.py).
#pragma once
#include <vector>

// sampler ids of svg_sample_loop (SVG_SAMPLER_* of include/svg_hip.h)
enum { kSamplerDdim = 0, kSamplerDpmpp2m = 1, kSamplerLms = 2 };

// One row per step, the same width for every rule:
//   DDIM   {t, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev), 0, 0, 0}
//   DPM++  {t, 1/a_s, sig_s, sig_s'/sig_s, a_s'(1 - e^-h), 1/2r (0: first order), last, 0}
//   LMS    {t, 1/sqrt(sigma_i^2 + 1), order, i, c0, c1, c2, c3}
constexpr int kSamplerRow = 8;

// The f32 alphas_cumprod of the scaled-linear schedule (0.00085 .. 0.012, 1000 train steps) as diffusers builds it: one table for
// the DDIM / DPM++ coefficients and for the LMS sigmas.
const std::vector<float>& sd_alphas_cumprod();
// DDIMScheduler.step (eta 0) t -> t_prev (< 0: alpha_bar = 1, set_alpha_to_one), in float
void ddim_coefs(int t, int t_prev, float* row);
// one DPM-Solver++(2M) row for the step t -> t_next (< 0: alpha_bar = 1); t_last < 0: first order
void dpmpp_coefs(int t, int t_next, int t_last, float* row);
// Step i of an n-step LMS schedule (diffusers 0.2.3 LMSDiscreteScheduler): timestep linspace(999, 0, n)[i], sigma_i and sigma_{i+1}
// interpolated between the train sigmas sqrt((1 - abar) / abar) (sigma_n = 0), order min(i + 1, 4), and the integrals over
// [sigma_i, sigma_{i+1}] of the Lagrange basis on sigma_i ... sigma_{i-order+1}, exact in double (c[k] = 0 for k >= order).
struct LmsCoef { double t, sigma, sigma_next; int order; double c[4]; };
void lms_coefs(int num_steps, int i, LmsCoef* out);
void lms_row(const LmsCoef& lc, int i, float* row);

struct SamplerPlan {
  int sampler = kSamplerDdim, num_steps = 0, start_step = 0;
  std::vector<float> table;            // num_steps rows
  const float* row(int i) const { return &table[(size_t)kSamplerRow * i]; }
  float timestep(int i) const { return row(i)[0]; }
  bool add_noise = false;              // 0 < start_step < num_steps: z <- noise_sa z + noise_s1a noise before the first step
  float noise_sa = 1.f, noise_s1a = 0.f;
  float z_scale = 1.f;                 // z <- z_scale z on entry (LMS: sigma_0)
  bool scaled_input = false;           // the UNet input is a scaled copy of z, row[1] z (LMS)
  int state_buffers = 0;               // latent-sized buffers the rule keeps between steps: 0 DDIM, 1 DPM++ (m_prev), 4 LMS (the ring)
};
// DDIM / DPM++ run on the timesteps (arange(n) * (1000 / n))[::-1] from step start_step on (DPM++: the step at start_step is first
// order); LMS has its own schedule and no history to start from, so start_step must be 0.
SamplerPlan sampler_plan(int sampler, int num_steps, int start_step);
