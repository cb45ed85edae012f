// Launchers of the sampling loop's update kernels (sampler.hip): f32 only, independent of the storage type, compiled once.
#pragma once
#include "common.h"
#include "sampler_plan.h"

// Where a kernel finds its row (sampler_plan.h): row idx[0] of a device table, so that a captured graph of one step replays for every
// timestep without new kernel arguments, or the kSamplerRow floats themselves.  Both go through the same kernel, so a replayed graph
// and direct launches cannot round differently.
struct SamplerRowArg { const float* tab; const int* idx; float v[kSamplerRow]; };
inline SamplerRowArg sampler_row_at(const float* tab, const int* idx) { return SamplerRowArg{tab, idx, {}}; }
inline SamplerRowArg sampler_row(const float* r) { return SamplerRowArg{nullptr, nullptr, {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]}}; }
inline SamplerRowArg sampler_scale(float c) { return SamplerRowArg{nullptr, nullptr, {0.f, c}}; }   // for lms_input alone: it reads v[1]

// tvec[i] = row[0] (the timestep) of the table row idx[0];  idx[0] += 1
void sampler_tvec(float* tvec, int nb, const float* tab, const int* idx, hipStream_t s);
void sampler_bump(int* idx, hipStream_t s);
// DDIM: z_out <- step(z, eps) with clip_sample; eps = eps_u + guidance (eps_c - eps_u) (eps_c null: eps_u)
void ddim_step(const float* z, const float* eps_u, const float* eps_c, float guidance, float* z_out, int64_t n, const SamplerRowArg& row,
               hipStream_t s);
// DPM-Solver++(2M): x_out <- step(x, eps); m_out <- the x0 prediction (may be null); m_prev is read only when row[5] != 0.
// x / x_out and m_prev / m_out may be the same buffers.
void dpmpp_step(const float* x, const float* eps_u, const float* eps_c, float guidance, const float* m_prev, float* x_out, float* m_out,
                int64_t n, const SamplerRowArg& row, hipStream_t s);
// LMS: x_out <- x + sum_{k < order} c[k] d_{i-k}, d_i = the CFG-combined eps, stored to slot i & 3 of the ring dhist (4 x n floats);
// the older derivatives are read from the slots (i-1) & 3 ...; x / x_out may be the same buffer
void lms_step(const float* x, const float* eps_u, const float* eps_c, float guidance, float* dhist, float* x_out, int64_t n,
              const SamplerRowArg& row, hipStream_t s);
// the UNet input of an LMS step: o0 (and o1 unless null) <- x * row[1]; x / o0 may be the same buffer
void lms_input(const float* x, float* o0, float* o1, int64_t n, const SamplerRowArg& row, hipStream_t s);
// the step of rule `sampler` (kSampler*) inside the loop, in place: state is m_prev (DPM++) or the ring (LMS)
void sampler_step(int sampler, float* z, const float* eps_u, const float* eps_c, float guidance, float* state, int64_t n,
                  const SamplerRowArg& row, hipStream_t s);
void add_noise(const float* x0, const float* noise, float* out, int64_t n, float sa, float s1a, hipStream_t s);
