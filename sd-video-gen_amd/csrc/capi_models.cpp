// C ABI: model configure / load / finalize dispatch.
#include "models.h"
#include "xf_walk.h"
#include "../../include/svg_hip.h"

// The slot of a model id: the one place that refuses an id the library does not know.
static std::unique_ptr<Model>& slot_of(svg_ctx* ctx, int model) {
  if (model < 0 || model >= svg_ctx::kCtxSlot) throw SvgError("unknown model id " + std::to_string(model));
  return ctx->models[model];
}

// A fresh, unconfigured model for a slot: the one id -> type table (svg_ctx::xf() .. i3d() cast back by it).  Storage type of the SD
// networks: configure key f16=1 -> IEEE half (the reference's autocast arithmetic), default bf16.
static std::unique_ptr<Model> make_model(int model, const char* kv) {
  auto f16 = [&]() {
    auto m = parse_kv(kv);
    return m.count("f16") && m["f16"][0] != 0;
  };
  switch (model) {
    case SVG_TRANSFORMER: return std::make_unique<XfModel>();
    case SVG_VAE: return std::unique_ptr<Model>(f16() ? new_vae_f16() : new_vae_bf16());
    case SVG_UNET: return std::unique_ptr<Model>(f16() ? new_unet_f16() : new_unet_bf16());
    case SVG_CLIP_TEXT: return std::make_unique<ClipTextModel>();
    case SVG_MINILM: return std::make_unique<MiniLmModel>();
    case SVG_I3D: return std::make_unique<I3dModel>();
  }
  throw std::logic_error("make_model: model id " + std::to_string(model) + " has a slot and no type");
}

// What every SD entry point starts with: its model (svg_ctx::vae or ::unet, `name` for the message) is configured, and an earlier
// layer-walking forward that gave up is dealt with (walk off + logged; raised to the Transformer's caller, not to this one).
template <class M>
static M& sd_entry(svg_ctx* ctx, M* (svg_ctx::*slot)() const, const char* name) {
  M* m = ctx ? (ctx->*slot)() : nullptr;
  SVG_CHECK(m, "%s: model not configured", name);
  xf_walk_check(ctx, false);
  return *m;
}

void destroy_models(svg_ctx* ctx) {
  for (std::unique_ptr<Model>& slot : ctx->models) {
    if (!slot) continue;
    slot->weights_changed(true);
    slot->ws.clear();
    slot.reset();
  }
}

extern "C" {

int svg_model_configure(svg_ctx* ctx, int model, const char* kv) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx, "null context");
    // a new configuration starts a fresh model: drop the previous weights and packed buffers
    std::unique_ptr<Model>* slot = nullptr;
    {
      DeviceWideScope lk;             // frees live device memory: not while another thread's stream is capturing
      HIP_OK(hipDeviceSynchronize());
      slot = &slot_of(ctx, model);
      if (*slot) (*slot)->ws.clear();
      for (void* p : ctx->owned[model]) hipFree(p);
      ctx->owned[model].clear();
      if (*slot) (*slot)->weights_changed(true);
    }
    *slot = make_model(model, kv);
    (*slot)->configure(kv);
  });
}

int svg_load_weight(svg_ctx* ctx, int model, const char* name, const float* data, const int64_t* shape, int ndim) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && name && data && shape && ndim >= 1 && ndim <= 5, "svg_load_weight: bad arguments");
    std::unique_ptr<Model>& slot = slot_of(ctx, model);
    if (!slot) slot = make_model(model, nullptr);   // a weight before any svg_model_configure: the model's defaults, bf16
    HIP_OK(hipSetDevice(ctx->device));
    slot->ws.put(ctx, name, data, shape, ndim);
    slot->weights_changed(false);
  });
}

int svg_finalize(svg_ctx* ctx, int model, int64_t* n_params) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx, "null context");
    Model* m = slot_of(ctx, model).get();
    SVG_CHECK(m, "svg_finalize: model %d has no weights", model);
    HIP_OK(hipSetDevice(ctx->device));
    ctx->cur_model = model;
    try {
      m->finalize(ctx, n_params);
    } catch (...) { ctx->cur_model = svg_ctx::kCtxSlot; throw; }
    ctx->cur_model = svg_ctx::kCtxSlot;
    {
      DeviceWideScope lk;
      HIP_OK(hipDeviceSynchronize());
    }
  });
}

/* ---- VAE / UNet / DDIM entry points: dispatch on the storage type the model was configured with ---- */
int svg_vae_encode(svg_ctx* ctx, const uint8_t* img, int N, int srcH, int srcW, int H, int W, const float* eps, float* z_out,
                   float* moments_out, void* stream) {
  return svg_guard(ctx, [&] {
    sd_entry(ctx, &svg_ctx::vae, "vae").encode(ctx, img, N, srcH, srcW, H, W, eps, z_out, moments_out, (hipStream_t)stream);
  });
}
int svg_vae_decode(svg_ctx* ctx, const float* z, int N, int h, int w, uint8_t* img_out, int outH, int outW, float* float_out,
                   void* stream) {
  return svg_guard(ctx, [&] {
    sd_entry(ctx, &svg_ctx::vae, "vae").decode(ctx, z, N, h, w, img_out, outH, outW, float_out, (hipStream_t)stream);
  });
}
int svg_unet_forward(svg_ctx* ctx, const float* x, int N, int h, int w, const float* timesteps, const float* ctx_emb, int ctx_len,
                     float* eps_out, void* stream) {
  return svg_guard(ctx, [&] {
    sd_entry(ctx, &svg_ctx::unet, "unet").forward(ctx, x, N, h, w, timesteps, ctx_emb, ctx_len, eps_out, (hipStream_t)stream);
  });
}
int svg_ddim_loop(svg_ctx* ctx, float* z, int N, int h, int w, const float* text_emb, int ctx_len, int num_steps, int start_step,
                  float guidance, const float* noise, float* hist, void* stream) {
  return svg_guard(ctx, [&] {
    sd_entry(ctx, &svg_ctx::unet, "unet").sample_loop(ctx, kSamplerDdim, z, N, h, w, text_emb, ctx_len, num_steps, start_step, guidance, noise, hist, (hipStream_t)stream);
  });
}
static_assert(SVG_SAMPLER_DDIM == kSamplerDdim && SVG_SAMPLER_DPMPP_2M == kSamplerDpmpp2m && SVG_SAMPLER_LMS == kSamplerLms,
              "sampler ids of svg_hip.h and models.h");
int svg_sample_loop(svg_ctx* ctx, int sampler, float* z, int N, int h, int w, const float* text_emb, int ctx_len, int num_steps,
                    int start_step, float guidance, const float* noise, float* hist, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(sampler == SVG_SAMPLER_DDIM || sampler == SVG_SAMPLER_DPMPP_2M || sampler == SVG_SAMPLER_LMS,
              "svg_sample_loop: unknown sampler %d", sampler);
    sd_entry(ctx, &svg_ctx::unet, "unet").sample_loop(ctx, sampler, z, N, h, w, text_emb, ctx_len, num_steps, start_step, guidance, noise, hist, (hipStream_t)stream);
  });
}
int svg_dpmpp_step(svg_ctx* ctx, const float* x, const float* eps, const float* m_prev, float* x_out, float* m_out, int64_t n, int t,
                   int t_next, int t_last, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->unet() && ctx->unet()->ready, "unet: model not finalized");
    SVG_CHECK(x && eps && x_out && n >= 0, "svg_dpmpp_step: null tensor or negative size");
    SVG_CHECK(!m_prev || t_next < 0 || t_last >= 0, "svg_dpmpp_step: a second-order step needs the previous timestep t_last");
    float row[kSamplerRow];
    dpmpp_coefs(t, t_next, m_prev ? t_last : -1, row);
    dpmpp_step(x, eps, nullptr, 0.f, m_prev, x_out, m_out, n, sampler_row(row), (hipStream_t)stream);
  });
}
int svg_lms_coefs(int num_steps, int i, double* timestep, double* sigma, double* sigma_next, int* order, double* coefs) {
  return svg_guard(nullptr, [&] {
    LmsCoef lc;
    lms_coefs(num_steps, i, &lc);
    if (timestep) *timestep = lc.t;
    if (sigma) *sigma = lc.sigma;
    if (sigma_next) *sigma_next = lc.sigma_next;
    if (order) *order = lc.order;
    if (coefs) for (int k = 0; k < 4; ++k) coefs[k] = lc.c[k];
  });
}
int svg_lms_step(svg_ctx* ctx, const float* x, const float* eps, float* dhist, float* x_out, int64_t n, int num_steps, int i, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx, "null context");
    SVG_CHECK(x && eps && dhist && x_out && n >= 0, "svg_lms_step: null tensor or negative size");
    LmsCoef lc;
    lms_coefs(num_steps, i, &lc);
    float row[kSamplerRow];
    lms_row(lc, i, row);
    lms_step(x, eps, nullptr, 0.f, dhist, x_out, n, sampler_row(row), (hipStream_t)stream);
  });
}
int svg_ddim_step(svg_ctx* ctx, const float* x, const float* eps, float* prev, int64_t n, int t, int t_prev, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->unet() && ctx->unet()->ready, "unet: model not finalized");
    float row[kSamplerRow];
    ddim_coefs(t, t_prev, row);
    ddim_step(x, eps, nullptr, 0.f, prev, n, sampler_row(row), (hipStream_t)stream);
  });
}
/* Has a layer-walking Transformer forward on this device given up since the last Transformer call / status query?  Call it where
 * the forward's result is consumed (after the stream has been synchronised): 0 = no, SVG_ERR_RUNTIME = yes (svg_last_error says what;
 * that forward's output is NaN-filled and must be re-issued: the walk is now off, the per-GEMM kernels serve). */
int svg_transformer_status(svg_ctx* ctx) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx, "null context");
    xf_walk_check(ctx, true);
  });
}
/* "bf16" / "fp16": the storage type of a configured SD model (SVG_VAE, SVG_UNET); "f32" for the Transformer / CLIP; NULL if absent */
const char* svg_model_dtype(svg_ctx* ctx, int model) {
  if (!ctx || model < 0 || model >= svg_ctx::kCtxSlot || !ctx->models[model]) return nullptr;   // a query: nothing is refused, absent is NULL
  return ctx->models[model]->dtype();
}

}  // extern "C"
