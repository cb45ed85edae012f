/*
 * svg_hip.h — C ABI of libsvg_hip.so: the MI355X (gfx950) implementation of the
 * sd-video-gen sampling path.  Plain pointers and sizes only; no torch types.
 *
 * The reference has no FFI: this boundary replaces the third-party numerics its Python
 * calls into.  Each entry point names the reference call site it stands in for
 * (paths relative to the reference repo root):
 *
 *   svg_transformer_forward   models/transformer.py:47-68 (Transformer.forward: embedding*sqrt(d),
 *                             PositionalEncoding by batch index positional_encoding.py:33-35,
 *                             nn.Transformer, out Linear); called from prediction/predict.py:16-42
 *   svg_vae_encode            utils/sd_utils.py:128-145 (encode_img: /255, NHWC->NCHW, 2(x-.5),
 *                             vae.encode(...).sample(), *0.18215) incl. the uint8 nearest resize
 *                             of prediction/predict.py:158,178
 *   svg_vae_decode            utils/sd_utils.py:156-169 (decode_img_latents: /0.18215, vae.decode,
 *                             (x/2+.5).clamp(0,1), *255 round -> uint8 NHWC)
 *   svg_unet_forward          utils/sd_utils.py:253 (self.unet(latent_model_input, t,
 *                             encoder_hidden_states=...)['sample'])
 *   svg_ddim_loop             utils/sd_utils.py:222-267 (gen_i2i_latents: DDIMScheduler(0.00085,
 *                             0.012,'scaled_linear',1000), set_timesteps, add_noise, CFG combine,
 *                             scheduler.step) — the hot loop
 *   svg_sample_loop           the same loop with a DPM-Solver++(2M) update in place of scheduler.step
 *                             (an addition: the reference has only DDIM here), or, with SVG_SAMPLER_LMS,
 *                             utils/sd_utils.py:97-126 (denoise_img_latents: LMSDiscreteScheduler(0.00085, 0.012,
 *                             'scaled_linear', 1000), set_timesteps, sigma scaling, CFG combine, scheduler.step)
 *   svg_lms_coefs / _step     that scheduler's timesteps, sigmas and coefficients (host only) / one update on caller data
 *   svg_clip_text_forward     utils/sd_utils.py:84,91 (self.text_encoder(input_ids)[0]: transformers CLIPTextModel of
 *                             'openai/clip-vit-large-patch14', last_hidden_state) — tokenisation stays on the host
 *   svg_resize_nearest_u8     prediction/predict.py:158,178 (F.interpolate on uint8, mode nearest)
 *   svg_resize_bilinear_f32   evaluation/predict_fvd.py:165 (F.interpolate of the predicted latent, mode bilinear)
 *   svg_load_weight/finalize  utils/sd_utils.py:52-66 + prediction/predict.py:50-51 (from_pretrained /
 *                             load_state_dict: tensors are handed over by their state_dict names)
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (SVG_ERR_INVALID: the arguments / shapes / call order are
 *     not acceptable — the Python facade raises ValueError; SVG_ERR_RUNTIME: a HIP call or kernel launch failed —
 *     RuntimeError); svg_last_error() gives the message.
 *   - all device pointers are caller-owned HBM (e.g. torch tensors); the library owns packed
 *     weights and one workspace arena per context, sized at svg_finalize()/first call; no
 *     allocation in steady state.  The library never frees caller memory.
 *   - `stream` is a hipStream_t (NULL = the null stream); every launch is asynchronous on it;
 *     no entry point synchronises the device except svg_load_weight/svg_finalize/svg_prof_*.
 *   - one context per (process, GPU); calls on a context are serialised by the caller.
 *   - boundary dtypes: f32 latents / embeddings / masks / noise, u8 images (NHWC).
 *     Storage type of the SD networks (activations + packed weights, f32 accumulation everywhere): bf16 by default,
 *     IEEE fp16 when the model is configured with f16=1 — the reference runs the UNet under fp16 autocast
 *     (utils/sd_utils.py:246); both sets of kernels are in the library (same sources compiled per type).
 *     The latent Transformer and the CLIP text tower compute in f32 (f32-input MFMA).
 */
#ifndef SVG_HIP_H
#define SVG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svg_ctx svg_ctx;

enum svg_model { SVG_TRANSFORMER = 0, SVG_VAE = 1, SVG_UNET = 2, SVG_CLIP_TEXT = 3, SVG_MINILM = 4, SVG_I3D = 5 };
enum svg_status { SVG_OK = 0, SVG_ERR_RUNTIME = -1, SVG_ERR_INVALID = -2 };

/* ---- context ------------------------------------------------------------------------------ */
int svg_create(int device_id, svg_ctx** out);
void svg_destroy(svg_ctx* ctx);
const char* svg_last_error(svg_ctx* ctx);            /* ctx may be NULL (creation errors) */
const char* svg_version(void);
/* The library reads its $SVG_* tuning / debugging knobs once per name and caches them (no getenv on a launch path); a process
 * that changes such a variable after the first call (the tests do) calls this to have the next call look it up again. */
void svg_env_refresh(void);

/* ---- models: configure -> load every tensor by state_dict name -> finalize ------------------ */
/* `kv`: "key=v[,v...];key=v" e.g. "block_out=320,640,1280,1280;layers=2;heads=8;ctx_dim=768".
 * Transformer keys: d_lat, d_model, heads, enc_layers, dec_layers, ffn (default 2048), text_dim (0; 384 for the
 *   text-conditioned variant, whose first layer is named project_image_embedding instead of embedding).
 * VAE keys: block_out (128,256,512,512), layers (2), groups (32), latent (4), f16 (0; 1 = fp16 storage instead of bf16),
 *   stream_f32 (0; 1 = the residual stream — conv_in, every resnet's conv2 + residual, the mid-block attention's proj_attn + residual,
 *   the up / down-sampler outputs — is stored in f32, closer to the reference's fp32 VAE; GroupNorm, conv1 and shortcut outputs and
 *   every matrix operand stay 16-bit; works with either storage type).
 * UNet keys: block_out (320,640,1280,1280), layers (2), heads (8), ctx_dim (768), groups (32),
 *            in_ch (4), out_ch (4), attn (1,1,1,0: cross-attention per down block), fp8 (0; 1 = BASELINE configs[4]: the
 *            dense projections with K % 128 == 0 that carry no folded LayerNorm / GEGLU run in MX block-scaled fp8 —
 *            OCP e4m3 + E8M0 per 32 — with activations quantised on the way in; everything else stays 16-bit),
 *            f16 (0; 1 = fp16 storage instead of bf16: utils/sd_utils.py:246 autocast).
 * CLIP text keys: vocab (49408), d_model (768), heads (12), layers (12), ffn (3072), max_pos (77); tensors by their
 *   transformers names without the "text_model." prefix (embeddings.token_embedding.weight, encoder.layers.N.*, ...).
 * MiniLM keys: vocab (30522), d_model (384), heads (12), layers (6), ffn (1536), max_pos (512); tensors by their transformers
 *   BertModel names (embeddings.word_embeddings.weight, encoder.layer.N.attention.self.query.weight, ...; the reference's text
 *   checkpoints carry them as sent_transformer.0.auto_model.<name>).
 * I3D keys: num_classes (400); tensors by the names of evaluation/pytorch_i3d.py's state_dict (Conv3d_1a_7x7.conv3d.weight,
 *   Mixed_3b.b1b.bn.running_var, logits.conv3d.bias, ...; num_batches_tracked entries are accepted and ignored). */
int svg_model_configure(svg_ctx* ctx, int model, const char* kv);
/* data: f32, host or device memory (hipMemcpyDefault); shape/ndim as in the state_dict. */
int svg_load_weight(svg_ctx* ctx, int model, const char* name, const float* data,
                    const int64_t* shape, int ndim);
/* packs fused layouts, checks that every expected tensor arrived (error names the first
 * missing key), returns the model's parameter count through *n_params if non-NULL. */
int svg_finalize(svg_ctx* ctx, int model, int64_t* n_params);
/* storage type of a configured model: "bf16" / "fp16" (SVG_VAE, SVG_UNET), "f32" (SVG_TRANSFORMER, SVG_CLIP_TEXT, SVG_MINILM, SVG_I3D); NULL if absent */
const char* svg_model_dtype(svg_ctx* ctx, int model);

/* ---- latent Transformer -------------------------------------------------------------------- */
/* src (B,Ts,D_lat), tgt (B,Tt,D_lat) batch-first f32; mask (Tt,Tt) additive f32 or NULL;
 * out (Tt,B,D_lat) sequence-first like the reference.  pe_row: NULL -> reference quirk (row b of
 * the batch gets PE(b)); else int32[B] giving the PE row used for each batch row (clip-batched
 * sampling passes zeros so every clip sees PE(0) exactly as at batch 1). */
int svg_transformer_forward(svg_ctx* ctx, const float* src, const float* tgt, int B, int Ts, int Tt,
                            const float* mask, const int32_t* pe_row, float* out, void* stream);

/* text-conditioned variant (models/transformer_text.py:71-111; configure text_dim=384): `text` (B,text_dim) f32 is the
 * class-name embedding (an INPUT: SentenceTransformer('all-MiniLM-L6-v2').encode(cls_list), transformer_text.py:82-83);
 * token = cat(project_image_embedding(x), text[b]) * sqrt(d_model) + PE, d_model = DIM_MODEL + text_dim. */
int svg_transformer_forward_text(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts,
                                 int Tt, const float* mask, const int32_t* pe_row, float* out, void* stream);

/* The same forward with nn.Transformer's key-padding masks (models/transformer.py:64: src_key_padding_mask = src_pad_mask,
 * tgt_key_padding_mask = tgt_pad_mask): src_pad (B,Ts) / tgt_pad (B,Tt) are ADDITIVE f32 biases on the scores of every query and
 * head of batch row b (a bool mask's True is -inf, as torch canonicalises it), applied to the encoder / decoder SELF-attention keys;
 * the cross-attention gets none (the reference passes no memory_key_padding_mask).  Either may be NULL; text as above or NULL. */
int svg_transformer_forward_padded(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                   const float* mask, const float* src_pad, const float* tgt_pad, const int32_t* pe_row,
                                   float* out, void* stream);

/* ---- latent Transformer: training step ------------------------------------------------------- */
/* Replaces the body of trainers/trainer.py:111-190 (train_loop: forward in train mode, criterion, loss.backward(),
 * opt.step()) and :192-260 (validation_loop: the same loss in eval mode) for the latent Transformer; the Stable
 * Diffusion side is frozen there too (encode_batch = svg_vae_encode).  f32 throughout like the reference trainer.
 * criterion() of trainers/trainer.py:65-109 is  w_mse*MSE + w_l1*L1 + w_gdl*GDL(alpha) + w_contrastive*BiPatchNCE(temperature)
 * (models/contrastive_loss.py:7-60) on the last frames_to_predict positions; w_* = use_* x lambda_*. */
typedef struct svg_train_cfg {
  int frames_to_predict;          /* F: loss on pred[-F:] (trainer.py:145) */
  int feat_h, feat_w;             /* FRAME_SIZE / 8: latent (4, feat_h, feat_w) */
  float w_mse, w_l1, w_gdl, gdl_alpha, w_contrastive, temperature;
  float dropout_p;                /* nn.Transformer / PositionalEncoding dropout (train mode only) */
  uint64_t seed;                  /* dropout masks are a pure function of (seed, site, element): pass a new seed every step */
} svg_train_cfg;
/* src (B,Ts,D_lat), tgt (B,Tt,D_lat), expected (B,Tt,D_lat) batch-first f32 (trainer.py:124-131: new_batch, new_batch[:,:-1],
 * new_batch[:,1:]); text (B,text_dim) or NULL; mask (Tt,Tt) additive or NULL.  backward = 0: eval-mode forward + criterion only;
 * 1: train mode (dropout) and the gradient of every parameter (overwriting the previous step's: zero_grad + backward);
 * SVG_BACKWARD_ACCUMULATE (2): as 1, but every parameter gradient is ADDED to what its slot holds (loss.backward() without
 * zero_grad()).  The gradients are zero when the training state is created; 1 starts a new sum and 2 continues it, so the first
 * micro-batch of an optimizer step uses 1, the following ones 2, and there is no separate zero-grad entry point.  The order of
 * the additions inside a call is fixed: the same sequence of calls gives the same bits.  Any other non-zero value behaves as 1.
 * losses: host float[5] = {total, mse, l1, gdl, contrastive} (synchronises the stream), or NULL.  B <= 64, Ts, Tt <= 32. */
#define SVG_BACKWARD_ACCUMULATE 2
int svg_transformer_loss(svg_ctx* ctx, const svg_train_cfg* cfg, const float* src, const float* tgt, const float* expected,
                         const float* text, int B, int Ts, int Tt, const float* mask, int backward, float* losses, void* stream);
/* The train-mode forward on its own (models/transformer.py:47-68 with model.train(): dropout active, same sites and masks as
 * svg_transformer_loss with this seed); out (Tt,B,D_lat).  text: (B,text_dim) for the text-conditioned variant, else NULL. */
int svg_transformer_forward_train(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                  const float* mask, float dropout_p, uint64_t seed, float* out, void* stream);
/* torch.optim.Adam(lr, betas=(beta1, beta2), eps) step on the gradients of the last svg_transformer_loss(backward=1)
 * (trainer.py:365: optim.Adam(model.parameters(), lr=lr) -> betas (0.9, 0.999), eps 1e-8, no weight decay). */
int svg_transformer_adam_step(svg_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream);
/* 2-norm over ALL parameter gradients as they stand (the total_norm of torch.nn.utils.clip_grad_norm_(params, ., 2.0)), reduced on
 * the device: squares and sums in double, in a fixed order (same gradients -> same double).  out: host double; synchronises the
 * stream like `losses` does. */
int svg_transformer_grad_norm(svg_ctx* ctx, double* out, void* stream);
/* The optimizer step with what a Transformer of this size is usually trained with.  With g' = grad_scale * g:
 *   total = ||g'||_2 over all parameters;  coef = min(1, max_grad_norm / (total + 1e-6))  (clip_grad_norm_), the update sees coef * g';
 *   then torch.optim.AdamW (decoupled = 1: p *= 1 - lr * weight_decay, then Adam) or torch.optim.Adam(weight_decay) (decoupled = 0:
 *   g += weight_decay * p), with the arithmetic of svg_transformer_adam_step.
 * Unlike torch's in-place clip the STORED gradients are not modified: svg_transformer_tensor(SVG_TENSOR_GRAD) afterwards still returns
 * the unscaled, unclipped sum.  grad_norm_out (host double, may be NULL) receives `total` and synchronises the stream; with NULL the
 * call only enqueues (the norm never visits the host: the update reads it from device memory).  Advances the same step counter as
 * svg_transformer_adam_step.  SVG_ERR_INVALID: no gradients yet, weight_decay < 0, max_grad_norm < 0, grad_scale <= 0, or the
 * hyper-parameter ranges svg_transformer_adam_step rejects. */
typedef struct svg_optim_cfg {
  float lr, beta1, beta2, eps;
  float weight_decay;     /* 0: none */
  int   decoupled;        /* 1: AdamW (p *= 1 - lr*wd, then Adam); 0: torch.optim.Adam(weight_decay=wd) (g += wd*p) */
  float max_grad_norm;    /* 0: no clipping; else torch.nn.utils.clip_grad_norm_(params, max_grad_norm, 2.0) */
  float grad_scale;       /* gradients are multiplied by this first (1/k after k accumulated micro-batches = loss/k in torch); 1: none */
} svg_optim_cfg;
int svg_transformer_optim_step(svg_ctx* ctx, const svg_optim_cfg* cfg, double* grad_norm_out, void* stream);
/* copies a parameter / its gradient / its Adam moments out (host or device `out`, numel floats; state_dict key names):
 * what torch.save(model.state_dict()) at trainer.py:469-480 needs after steps taken in the library. */
/* SVG_TENSOR_EMA: the averaged weights (below); SVG_ERR_INVALID while none exist. */
enum svg_tensor_kind { SVG_TENSOR_PARAM = 0, SVG_TENSOR_GRAD = 1, SVG_TENSOR_EXP_AVG = 2, SVG_TENSOR_EXP_AVG_SQ = 3, SVG_TENSOR_EMA = 4 };
int svg_transformer_tensor(svg_ctx* ctx, int kind, const char* name, float* out, int64_t numel, void* stream);

/* ---- latent Transformer: continuing a training run ------------------------------------------- */
/* The inverse of svg_transformer_tensor for SVG_TENSOR_EXP_AVG, SVG_TENSOR_EXP_AVG_SQ and SVG_TENSOR_EMA: numel floats from `data`
 * (host or device memory) become that tensor of parameter `name` (state_dict key).  Synchronises the stream.
 * If the context has no training state yet it is created, in the condition it has right after creation (zero gradients, zero
 * moments, step count 0, no gradients to step on until the next svg_transformer_loss(backward != 0)); the first SVG_TENSOR_EMA
 * creates the averaged weights, every tensor a copy of its parameter as it stands, before `name` is overwritten.
 * SVG_TENSOR_PARAM and SVG_TENSOR_GRAD are refused: parameters go through svg_load_weight, which DROPS the training state
 * (moments, step count, averaged weights and their decay).  The order of a resume is therefore
 *   svg_load_weight (every tensor) -> svg_finalize -> svg_transformer_set_tensor (moments, averaged weights)
 *   -> svg_transformer_set_optim_step_count -> svg_transformer_ema_configure -> svg_transformer_loss ...
 * SVG_ERR_INVALID, with nothing changed: a null argument, a kind other than the three, an unknown name, numel other than the
 * parameter's, or a model that is not finalized.  Allocation (first call only) happens under the library's device-wide lock,
 * after a device-wide synchronisation, like every other change of what the training state owns. */
int svg_transformer_set_tensor(svg_ctx* ctx, int kind, const char* name, const float* data, int64_t numel, void* stream);
/* The number of optimizer steps taken: the counter that svg_transformer_adam_step and svg_transformer_optim_step advance by one
 * and take their bias corrections 1 - beta^step from (0 without training state).  Setting it (0 <= step < 2^31; creates the
 * training state if there is none) makes the next step number step + 1. */
int svg_transformer_optim_step_count(svg_ctx* ctx, int64_t* out);
int svg_transformer_set_optim_step_count(svg_ctx* ctx, int64_t step);
/* Exponential moving average of the parameters, kept by the optimizer step itself.  0 < decay < 1 turns it on: from then on every
 * svg_transformer_adam_step / svg_transformer_optim_step also does, per element and in f32, in the launch and the loop that forms
 * the new parameter p_new,
 *       e = e + (p_new - e) * (1.f - decay)
 * (the form of the exp_avg update); p, exp_avg and exp_avg_sq get the bits they get without it.  If no averaged weights exist when
 * it is turned on they are allocated as a copy of the parameters as they stand (device-wide synchronisation, once).  decay == 0
 * turns the updates off and keeps the buffers and their values; any other value is SVG_ERR_INVALID.  Read them with
 * svg_transformer_tensor(SVG_TENSOR_EMA), write them with svg_transformer_set_tensor.  They are part of the training state:
 * svg_load_weight / svg_model_configure / svg_destroy free them and forget the decay. */
int svg_transformer_ema_configure(svg_ctx* ctx, float decay);

/* ---- CLIP text encoder ---------------------------------------------------------------------- */
/* input_ids (B,T) int32 token ids (T <= max_pos; the reference pads to 77); out (B,T,d_model) f32 = last_hidden_state.
 * Causal mask only (the reference passes no attention mask); f32 arithmetic like the reference. */
int svg_clip_text_forward(svg_ctx* ctx, const int32_t* input_ids, int B, int T, float* out, void* stream);

/* ---- MiniLM sentence encoder ------------------------------------------------------------------ */
/* models/transformer_text.py:82-83: txt = self.sent_transformer.encode(cls_list) with SentenceTransformer('all-MiniLM-L6-v2')
 * (:12): BertModel -> attention-mask-weighted mean pooling -> L2 normalisation.  input_ids (B,T) int32: [CLS] tokens [SEP],
 * then padding; lengths (B) int32: tokens of each row that are not padding; out (B,d_model) f32 unit-norm embeddings;
 * hidden (optional, may be NULL): (B,T,d_model) last_hidden_state.  T <= 128.  Tokenisation (WordPiece) stays on the host. */
int svg_minilm_encode(svg_ctx* ctx, const int32_t* input_ids, const int32_t* lengths, int B, int T, float* out, float* hidden,
                      void* stream);

/* ---- FVD evaluation (evaluation/pytorch_i3d.py, evaluation/fvd_2.py; called at the end of prediction/predict_text.py) ---------- */
/* InceptionI3d.forward (pytorch_i3d.py:303-312): x (B,3,T,224,224) f32 in [-1,1] -> logits (B,num_classes) f32 (mean over time). */
int svg_i3d_forward(svg_ctx* ctx, const float* x, int B, int T, int H, int W, float* logits, void* stream);
/* fvd_2.get_fvd_logits (fvd_2.py:16-19): videos (B,T,H,W,3) uint8 -> preprocess (fvd_2.py:7-14,109-136: /255, bilinear resize of the
 * shorter side to 224, centre crop, [-1,1]) -> I3D logits (B,num_classes). */
int svg_fvd_logits(svg_ctx* ctx, const uint8_t* videos, int B, int T, int H, int W, float* logits, void* stream);
/* the preprocessing alone: out (B,3,T,224,224) f32 */
int svg_fvd_preprocess(svg_ctx* ctx, const uint8_t* videos, int B, int T, int H, int W, float* out, void* stream);
/* fvd_2.frechet_distance (fvd_2.py:66-78): x1 (n1,d), x2 (n2,d) f32 device embeddings -> *out (HOST double; synchronises the stream).
 * Means / unbiased covariances in f64, the two symmetric square roots (fvd_2.py:22-33, SVD there) by a Jacobi eigen-decomposition. */
int svg_frechet_distance(svg_ctx* ctx, const float* x1, int n1, const float* x2, int n2, int d, double* out, void* stream);

/* ---- per-frame quality: squared error and SSIM (an addition: the reference measures FVD only and has no counterpart) -------------- */
/* a, b: uint8 NHWC stacks (N,H,W,3), contiguous, any byte alignment.  Per image n:
 *   sse[n]   int64: the exact integer sum of (a - b)^2 over all H*W*3 bytes (MSE = sse / (H*W*3), PSNR = 10 log10(255^2 / MSE) are host
 *            arithmetic on it);
 *   ssim[n]  double: the mean over the (H-10)*(W-10)*3 valid positions of the SSIM map of Wang et al. 2004 — 11x11 Gaussian window G,
 *            sigma 1.5, taps exp(-x^2 / (2 sigma^2)) for x = -5..5 normalised to sum 1, separable; K1 = 0.01, K2 = 0.03, data range 255, so
 *            C1 = 6.5025, C2 = 58.5225; per channel mu = G*a, var_a = G*a^2 - mu_a^2, cov = G*ab - mu_a mu_b and
 *            s = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2))
 *            (skimage structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=255, channel_axis=-1); the
 *            valid-convolution form of tf.image.ssim).  The map is computed in f32, its sum in double.
 *   ssim_map (optional, may be NULL): f32 (N,H-10,W-10,3), every map value; sse and ssim get the same bits with or without it.
 * sse, ssim and ssim_map are device memory; the call only enqueues and does not synchronise.  The sums are taken in a fixed order and
 * without atomics: an image gives the same bits alone, repeated, or inside a larger batch.  The per-tile partial sums live in the
 * context's workspace (the call takes part in svg_plan_begin .. svg_plan_end; a second call of a shape grows nothing).
 * SVG_ERR_INVALID, with nothing launched: a null ctx, a, b, sse or ssim; N < 1; H < 11 or W < 11; H or W > 16384 (image offsets are
 * 32-bit: H*W*3 < 2^31); N * ceil((H-10)/32) * ceil((W-10)/32) >= 2^31 (one workgroup per image and 32x32 map tile). */
int svg_frame_metrics(svg_ctx* ctx, const uint8_t* a, const uint8_t* b, int N, int H, int W, int64_t* sse, double* ssim, float* ssim_map,
                      void* stream);

/* ---- VAE ------------------------------------------------------------------------------------ */
/* img: u8 NHWC (N,srcH,srcW,3); nearest-resized to (H,W) on the fly when they differ.
 * eps: f32 (N,4,H/8,W/8) standard-normal draws for .sample(), or NULL for the distribution mean.
 * z_out: f32 (N,4,H/8,W/8), already multiplied by 0.18215.  moments_out (optional, may be NULL):
 * f32 (N,8,H/8,W/8) = [mean; logvar] before sampling. */
int svg_vae_encode(svg_ctx* ctx, const uint8_t* img, int N, int srcH, int srcW, int H, int W,
                   const float* eps, float* z_out, float* moments_out, void* stream);
/* z: f32 (N,4,h,w) scaled latents (divided by 0.18215 inside).  img_out: u8 NHWC (N,outH,outW,3),
 * nearest-resized from (8h,8w) when they differ.  float_out (optional): f32 NCHW (N,3,8h,8w),
 * the decoder output before the clamp/quantise. */
int svg_vae_decode(svg_ctx* ctx, const float* z, int N, int h, int w, uint8_t* img_out, int outH,
                   int outW, float* float_out, void* stream);

/* ---- UNet / DDIM ---------------------------------------------------------------------------- */
/* x (N,4,h,w) f32; timesteps f32[N]; ctx_emb (N,ctx_len,ctx_dim) f32; eps_out (N,4,h,w) f32. */
int svg_unet_forward(svg_ctx* ctx, const float* x, int N, int h, int w, const float* timesteps,
                     const float* ctx_emb, int ctx_len, float* eps_out, void* stream);
/* DDIM img2img over timesteps[start_step:] of a `num_steps` schedule (1000 train steps,
 * scaled_linear 0.00085..0.012, clip_sample, set_alpha_to_one, eta 0).
 * z (N,4,h,w) f32 in/out.  text_emb (2N,ctx_len,ctx_dim) = [uncond; cond] like encode_text().
 * noise: f32 (N,4,h,w) for add_noise when start_step>0 (required then), else ignored.
 * guidance==0 runs the UNet on the uncond half only (exact: u + 0*(c-u) == u).
 * hist (optional): f32 ((num_steps-start_step+1)*N,4,h,w) latent history incl. the start. */
int svg_ddim_loop(svg_ctx* ctx, float* z, int N, int h, int w, const float* text_emb, int ctx_len,
                  int num_steps, int start_step, float guidance, const float* noise, float* hist,
                  void* stream);
/* one scheduler step on caller data (x, eps -> prev); t = timestep value, t_prev = t - 1000/num_steps */
int svg_ddim_step(svg_ctx* ctx, const float* x, const float* eps, float* prev, int64_t n, int t,
                  int t_prev, void* stream);

/* Samplers of svg_sample_loop. */
#define SVG_SAMPLER_DDIM 0      /* the update of svg_ddim_loop */
#define SVG_SAMPLER_DPMPP_2M 1  /* DPM-Solver++(2M) */
#define SVG_SAMPLER_LMS 2       /* linear multistep, order <= 4: the reference's text-to-image sampler (below) */
/* The img2img loop of svg_ddim_loop under the update rule `sampler`: the same arguments, contract, timesteps
 * t_i = (num_steps-1-i)*1000/num_steps, add_noise at t_start, CFG combine, history and step graph.
 * SVG_SAMPLER_DDIM is exactly svg_ddim_loop.  SVG_SAMPLER_DPMPP_2M is the update of diffusers'
 * DPMSolverMultistepScheduler(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint",
 * lower_order_final=True, thresholding=False) on this timestep set: with abar from the DDIM schedule
 * (abar = 1 below t = 0), a = sqrt(abar), sig = sqrt(1-abar), lambda = log a - log sig, step s -> s':
 *   m = (x - sig_s eps) / a_s (no clipping);  h = lambda_s' - lambda_s;
 *   D = m at the loop's first step, else m + (m - m_prev) / 2r with r = (lambda_s - lambda_prev) / h;
 *   x' = (sig_s'/sig_s) x + a_s' (1 - e^-h) D, and x' = m at the last step (sig_s' = 0).
 * Unlike diffusers, a run of fewer than 15 steps does not also fall back to first order at its
 * second-to-last step.  One extra latent-sized buffer (m_prev) in the workspace.
 * An unknown sampler returns SVG_ERR_INVALID. */
int svg_sample_loop(svg_ctx* ctx, int sampler, float* z, int N, int h, int w, const float* text_emb,
                    int ctx_len, int num_steps, int start_step, float guidance, const float* noise,
                    float* hist, void* stream);
/* One DPM-Solver++(2M) step of svg_sample_loop on caller data (f32, n elements, no CFG combine):
 * x_out = step(x, eps), m_out = the x0 prediction m (m_out may be NULL).  t -> t_next (t_next < 0:
 * abar = 1, the final first-order step x_out = m).  m_prev = the previous step's m at timestep t_last
 * (> t); m_prev NULL: a first-order step, t_last ignored.  x / x_out and m_prev / m_out may alias. */
int svg_dpmpp_step(svg_ctx* ctx, const float* x, const float* eps, const float* m_prev, float* x_out,
                   float* m_out, int64_t n, int t, int t_next, int t_last, void* stream);

/* SVG_SAMPLER_LMS runs diffusers 0.2.3's LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, 'scaled_linear', 1000) inside
 * svg_sample_loop.  Its contract differs from the other two samplers:
 *   - z holds unit-normal draws on entry; the loop scales them by sigma_0 (14.6146 at any step count) before the first step;
 *   - start_step must be 0 (SVG_ERR_INVALID otherwise: the reference has no LMS img2img, and the rule is not well defined when
 *     the history is shorter than the order); noise is ignored;
 *   - the timesteps are t_i = linspace(999, 0, num_steps)[i], fractional, handed to the UNet as f32.
 * With abar the f32 alphas_cumprod of the schedule and everything after it in double: sigma_i interpolates the train sigmas
 * sqrt((1 - abar) / abar) linearly between floor(t_i) and ceil(t_i), sigma_num_steps = 0.  Step i: the UNet input is
 * x / sqrt(sigma_i^2 + 1); d_i = eps_i after the CFG combine (the reference computes (x - (x - sigma_i eps_i)) / sigma_i, the same
 * number up to f32 rounding); order = min(i + 1, 4);
 *   c_k = integral over [sigma_i, sigma_{i+1}] of prod_{j != k} (tau - sigma_{i-j}) / (sigma_{i-k} - sigma_{i-j}),  k, j < order
 * (a polynomial of degree <= 3, integrated exactly: no quadrature);  x <- x + sum_k c_k d_{i-k}.
 * As for the other samplers, guidance == 0 runs the uncond half only, hist (num_steps + 1 latents, the first one the scaled
 * draws) is filled on the direct-launch path, and the second step is captured and replayed.  Workspace: one table and a ring of
 * four latent-sized derivative buffers.
 *
 * svg_lms_coefs: step i of a num_steps schedule, on the host (no context, no device): the timestep, sigma_i, sigma_{i+1}, the
 * order and coefs[4] (zero beyond the order); any output pointer may be NULL.  SVG_ERR_INVALID outside 1 <= num_steps <= 1000,
 * 0 <= i < num_steps. */
int svg_lms_coefs(int num_steps, int i, double* timestep, double* sigma, double* sigma_next, int* order,
                  double* coefs);
/* One LMS update of that schedule on caller data (f32, n elements, no CFG combine): eps is stored to slot i & 3 of the caller's
 * ring dhist (4 * n floats, which must hold the eps of the steps i-1 ... i-3 in their slots when the order asks for them), and
 * x_out = x + sum_k c_k dhist[(i - k) & 3].  x / x_out may alias. */
int svg_lms_step(svg_ctx* ctx, const float* x, const float* eps, float* dhist, float* x_out, int64_t n,
                 int num_steps, int i, void* stream);

int svg_resize_nearest_u8(svg_ctx* ctx, const uint8_t* src, int N, int sh, int sw, int C,
                          uint8_t* dst, int dh, int dw, void* stream);
/* evaluation/predict_fvd.py:165 (nn.functional.interpolate(latent, (64, 64), mode='bilinear'), align_corners=False):
 * `planes` f32 images of h x w -> oh x ow (NCHW latents: planes = N * 4). */
int svg_resize_bilinear_f32(svg_ctx* ctx, const float* src, int planes, int h, int w, float* dst, int oh, int ow, void* stream);

/* ---- operator level (the kernels the graphs are made of; used by the parity tests) ---------- */
/* 16-bit buffers are passed as uint16_t bit patterns: bf16 for svg_op_<name>, IEEE fp16 for the svg_op_<name>_f16 twin
 * declared at the end of this section (same arguments, the fp16 build of the same kernel).  NHWC activations, weights
 * [N][K] K-contiguous. */
/* C[M,N] = act(A[M,K] * W[N,K]^T + bias[N] + residual[M,N]);  out_f32: C is f32 instead of bf16.
 * act: 0 none, 1 SiLU, 2 GELU(erf), 3 GEGLU (W rows = [h;gate] halves of 2*N_out, C is [M,N/2]). */
int svg_op_gemm(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias,
                const uint16_t* residual, void* C, int M, int N, int K, int act, int out_f32,
                void* stream);
/* 3x3 convolution on NHWC bf16: x (B,H,W,Cin), w f32 OIHW (packed inside, cached by pointer is NOT
 * done: the packed copy is rebuilt per call — test hook).  mode: 0 stride1 pad1, 1 stride2 pad1,
 * 2 stride2 pad (0,1,0,1), 3 nearest-2x upsample then stride1 pad1.  out (B,Ho,Wo,Cout) bf16. */
int svg_op_conv3x3(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias,
                   uint16_t* out, int B, int H, int W, int Cin, int Cout, int mode, void* stream);
/* stride-1 3x3 conv whose tile epilogue leaves the GroupNorm column sums of its output, then the GroupNorm (+SiLU) that
 * consumes them (no statistics pass over the tensor).  *used_epilogue_stats: 1 when that path ran (images >= 32 x 32 without
 * split-K), 0 when the GroupNorm fell back to its own statistics pass.  Cin % 64 == 0, Cout % 4 == 0. */
int svg_op_conv3x3_gn(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const float* gamma,
                      const float* beta, uint16_t* conv_out, uint16_t* gn_out, int B, int H, int W, int Cin, int Cout,
                      int groups, float eps, int silu, int* used_epilogue_stats, void* stream);
/* 3x3 conv of the VAE's f32 residual stream (model key stream_f32): x (B,H,W,Cin) 16-bit, out (B,Ho,Wo,Cout) f32 = conv + bias + residual
 * (residual: 16-bit, residual_f32: f32, or neither).  gn_out non-NULL: then the GroupNorm (+SiLU) of out into gn_out (16-bit), from the
 * conv epilogue's column sums of the stored f32 values when that path ran (*used_epilogue_stats = 1: images >= 32 x 32 without split-K).
 * *halo_width: 128 / 160 = the halo kernel ran with that channel tile, 0 = the implicit GEMM.  mode 0: stride 1 pad 1 (Cin 8: the
 * small-Cin conv), 2: stride 2 pad (0,1,0,1), 3: nearest-2x upsample then stride 1 pad 1.  Cin % 64 == 0 (or 8), Cout % 4 == 0. */
int svg_op_conv3x3_f32s(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual,
                        const float* residual_f32, float* out, const float* gamma, const float* beta, uint16_t* gn_out, int B, int H,
                        int W, int Cin, int Cout, int mode, int groups, float eps, int silu, int* halo_width, int* used_epilogue_stats,
                        void* stream);
/* GroupNorm (+SiLU) on NHWC f32, 16-bit output (the GroupNorms that read the VAE's f32 residual stream). */
int svg_op_groupnorm_f32(svg_ctx* ctx, const float* x, const float* gamma, const float* beta, uint16_t* out, int B, int HW, int C,
                         int groups, float eps, int silu, void* stream);
/* stride-1 3x3 conv in OCP MX block-scaled fp8 (BASELINE configs[4], conv_halo_fp8.hip): x (B,H,W,Cin) 16-bit and the f32 OIHW weights
 * are quantised on the device (e4m3 + one E8M0 scale per 32 input channels), the products run on v_mfma_scale_f32_16x16x128_f8f6f4
 * with f32 accumulation; out (B,H,W,Cout) 16-bit = conv + bias (+ residual).  q_out ((B*H*W, Cp) bytes, Cp = Cin rounded up to 128)
 * and s_out ((B*H*W, Cp/32) bytes) optionally receive the quantised activations.  Cin % 64 == 0, Cout % 4 == 0 and >= 128,
 * H % 16 == W % 16 == 0 (of the output), at least 192 (16 x 16 pixel block, channel tile) pairs.  mode 0: stride 1 pad 1; mode 3: nearest-2x
 * upsample fused in front (out (B,2H,2W,Cout)), the UNet's Upsample2D.  Replaces F.conv2d of the resnets' convs under
 * the fp8 = 1 model key (reference call sites: the conv1 / conv2 of diffusers' ResnetBlock2D behind utils/sd_utils.py:253). */
int svg_op_conv3x3_mx(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual,
                      uint16_t* out, uint8_t* q_out, uint8_t* s_out, int B, int H, int W, int Cin, int Cout, int mode, void* stream);
/* The same conv on a descriptor, with every operand the UNet gives it and the packed weights read back (test hook; nothing is added to
 * the kernels).  With Npad = Cout rounded up to 4, (Ho, Wo) the output image and Cp = Cin rounded up to 128:
 *   out[b][y][x][n] = conv[b][y][x][n] + bias[n] + bias_bn[b * ld + n] + residual[b][y][x][n],   ld = bias_bn_ld, or Npad when that is 0
 * x (B,H,W,Cin) 16-bit; w_oihw (Cout,Cin,3,3) f32 and bias (Cout, or NULL) f32 in host or device memory; bias_bn (device f32, or NULL):
 * one row per sample, the time-embedding row of a resnet's conv1; residual (or NULL) and out: (B,Ho,Wo,Npad) 16-bit, the columns
 * Cout .. Npad - 1 come from zero weights and a zero bias.  mode 0: stride 1; 3: nearest-2x upsample in front (Ho = 2H, Wo = 2W).
 * gn_part (device f32, or NULL): (B * Ho/16 * Wo/16) * Npad * 2 floats, the GroupNorm column sums with svg_gemm_desc::gn_part's contract
 * for conv_halo: gn_part[(tile_m * Npad + n) * 2 + {0,1}], tile_m = (b * Ho/16 + y/16) * Wo/16 + x/16.
 * Read-backs (device, each may be NULL): q_out (B*H*W, Cp) and s_out (B*H*W, Cp/32) as svg_op_conv3x3_mx; w8_out: the packed weights,
 * e4m3 [Npad][tap = 3 ky + kx][Cp]; w8s_out: their scales, E8M0 [tap][Cp/128][Npad][4] (byte i: channels 32 i .. 32 i + 31 of the
 * 128-channel chunk).  Padding (channels >= Cin, rows >= Cout, and any all-zero block): zero bytes with scale byte 127.
 * path (int[3], or NULL) receives what the launcher used: {column tile (128 / 160), tn_major, workgroups}.  A shape conv_halo_fp8 does
 * not take (see svg_op_conv3x3_mx) returns an error without launching anything. */
typedef struct svg_conv_mx_desc {
  const uint16_t* x;
  const float *w_oihw, *bias;
  const float* bias_bn;
  int bias_bn_ld;
  const uint16_t* residual;
  uint16_t* out;
  int B, H, W, Cin, Cout, mode;
  float* gn_part;
  uint8_t *q_out, *s_out, *w8_out, *w8s_out;
} svg_conv_mx_desc;
int svg_op_conv3x3_mx_ex(svg_ctx* ctx, const svg_conv_mx_desc* desc, int* path, void* stream);
/* C[M,N] = [A | A2] * W[N,K]^T + bias with the A operand given as two tensors (A: M x k_split, A2: M x (K - k_split)): the
 * torch.cat([hidden, skip], dim=1) in front of a resnet's 1x1 shortcut, never materialised.  k_split % 64 == 0. */
/* C[batch*M,N] = A W^T + bias + residual, and the LayerNorm statistics of its rows (rs = rstd, rm = rstd * mean, eps 1e-5) as the
 * transformer blocks of the UNet get them: from row partials the GEMM epilogue emits (*used = column tiles that emitted, 0 = fallback pass) */
int svg_op_gemm_lnstats(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, uint16_t* C, int M,
                        int N, int K, int batch, float* rs, float* rm, int* used, void* stream);
int svg_op_gemm_cat(svg_ctx* ctx, const uint16_t* A, const uint16_t* A2, const uint16_t* W, const float* bias, uint16_t* C,
                    int M, int N, int K, int k_split, void* stream);
/* One GEMM / implicit-GEMM conv with the whole epilogue contract the models use (test hook): the fields mirror the library's own
 * launch descriptor and reach the kernel selection unchanged (no packing, no folding here).  Per batch z:
 *   C[z][m][n] = act( LN( alpha * A[z] W[z]^T )[m][n] + bias[z][n or m] + bias_bn[m / rows_per_batch][n] + residual[z][m][n] )
 * with LN(x) = x (ln_rs NULL), rs[m] x - rm[m] s[n] (normal) or rs[t] x - rm[t] s[m], t = z * ln_zstride + n (ln_swapped; tokens
 * n >= n_valid count as rs = rm = 0).  A[z] = A + z * sA, W[z] = Wt + z * sB, C[z] = C + z * sC, residual[z] = residual + z * sC,
 * bias[z] = bias + z * bias_zs.  amode 0: dense A (row stride lda); 1: 3x3 stride-1 conv of NHWC A (B, H, W, Cin), 4: 3x3 conv
 * of its nearest-2x upsample, (Ho, Wo) the output image, M = B * Ho * Wo, K = 9 * Cin, Wt packed [N][9][Cin] (tap-major).  Rows
 * n >= n_valid of Wt read as zero.  act: 0 none, 1 SiLU, 2 GELU (erf), 3 GEGLU (Wt in 16-row h / gate tiles).  out_f32: C is f32.  vt_out: the fused q | k | V^T write
 * (columns >= vt_n0 go transposed to vt_out[m / vt_rows][n - vt_n0][m % vt_rows], row stride vt_ld, sample stride vt_bs).
 * path (int[3], or NULL) receives what ran: {kernel family (0 tiled igemm, 1 conv_halo, 2 gemm_pp, 3 gemm_ws), column tile, split-K}.
 * Combinations no kernel honours per batch (bias_bn or a normal LayerNorm fold with batch > 1, bias_zs with GEGLU) and a V^T write
 * of a partial last sample (M % vt_rows != 0) return an error without launching anything. */
typedef struct svg_gemm_desc {
  int amode, H, W, Cin, Ho, Wo;
  const uint16_t* A;
  int lda;
  const uint16_t* Wt;
  int ldb, n_valid;
  void* C;
  int ldc, M, N, K, batch;
  int64_t sA, sB, sC;
  float alpha;
  const float* bias;
  int bias_row;
  int64_t bias_zs;
  const float* bias_bn;
  int rows_per_batch, bias_bn_ld;
  const uint16_t* residual;
  int ldr, act, out_f32;
  const float *ln_rs, *ln_rm, *ln_s;
  int ln_swapped;
  int64_t ln_zstride;
  uint16_t* vt_out;
  int vt_n0, vt_rows, vt_ld;
  int64_t vt_bs;
  /* appended (the offsets above stay put); all zero = none of it */
  const uint16_t* A2;       /* dense two-source A = [A | A2]: K columns >= k_split (a multiple of 64) come from A2, row stride lda2; tiled igemm only */
  int lda2, k_split;
  float* gn_part;           /* GroupNorm column sums the tile epilogue leaves: gn_part[(tile_m * N + n) * 2 + {0,1}] = sum, sum of squares of the
                             * STORED values of column n over the rows of row tile tile_m (plan[3] rows; conv_halo: one 16 x 16 pixel block,
                             * tile_m = (b * Ho / 16 + y / 16) * Wo / 16 + x / 16) */
  float* ln_part;           /* LayerNorm row partials: ln_part[((z * M + m) * ln_tiles + tile_n) * 2 + {0,1}] = the same of row m over the plan[1]
                             * columns of column tile tile_n; ln_tiles must be plan[4] */
  int ln_tiles;
} svg_gemm_desc;
int svg_op_gemm_ex(svg_ctx* ctx, const svg_gemm_desc* desc, int* path, void* stream);
/* What svg_op_gemm_ex would launch for desc, without launching: plan[5] = {kernel family, column tile, split-K, gn_rows (rows per GroupNorm
 * row tile, 0: the launch cannot emit gn_part), ln_tiles (LayerNorm column tiles, 0: it cannot emit ln_part)}.  The models ask the same
 * question before every launch that emits: plan, fill gn_part / ln_part / ln_tiles from the answer, launch.  gn_part / ln_part set where the
 * plan has 0 (split-K, batch > 1 for gn_part, out_f32 = 1, GEGLU, a conv with ln_part ...) or an ln_tiles other than the plan's make
 * svg_op_gemm_ex return an error without launching anything. */
int svg_op_gemm_plan(svg_ctx* ctx, const svg_gemm_desc* desc, int* plan);
/* Fused GEGLU feed-forward of a BasicTransformerBlock (C = 320): out = ff.net.2(GEGLU(ff.net.0(LayerNorm(x)))) + residual in ONE
 * kernel (the M x 4C intermediate never reaches HBM).  x, residual, out: (M,C) bf16; w1 (8C,C) = [h; gate], b1 (8C), w2 (C,4C),
 * b2 (C), LayerNorm gamma / beta (C): f32 in the state_dict layout (folded and packed inside: test hook). */
int svg_op_ff_fused(svg_ctx* ctx, const uint16_t* x, const float* ln_gamma, const float* ln_beta, const float* w1,
                    const float* b1, const float* w2, const float* b2, const uint16_t* residual, uint16_t* out, int M,
                    int C, void* stream);
/* Cross-attention of a BasicTransformerBlock (C = 320: 8 heads of 40, context of L <= 80 tokens) in ONE kernel:
 * out = x + to_out(softmax(to_q(LayerNorm(x)) K^T / sqrt(40)) V) + bo.  x, out (M,320) 16-bit; k (N,L,320) and vt (N,320,Lp) 16-bit: the
 * projected context of each of the N = M / rows_per_sample samples; wq, wo (320,320), bo, LayerNorm gamma / beta (320): f32 in the
 * state_dict layout (folded, head-padded and packed inside: test hook).  Chained form: x == NULL and a (M,320) = the self-attention's
 * output, r (M,320) its residual, wp (320,320) / bp (320) its output projection: x = r + a wp^T + bp is formed inside the kernel. */
int svg_op_xattn_fused(svg_ctx* ctx, const uint16_t* x, const uint16_t* a, const uint16_t* r, const float* wp, const float* bp,
                       const float* ln_gamma, const float* ln_beta, const float* wq, const uint16_t* k, const uint16_t* vt, int Lp,
                       const float* wo, const float* bo, uint16_t* out, int M, int rows_per_sample, int L, void* stream);
/* dropout mask of one site of the training step: out[i] = 1/(1-p) (kept) or 0, i < n (tests regenerate the masks with it) */
int svg_op_dropout_mask(svg_ctx* ctx, uint64_t seed, int site, float p, float* out, int64_t n, void* stream);
/* The training-step kernels of the latent Transformer one by one (test hooks: each is its launcher, nothing is added).  f32 device
 * buffers; a dropout site is (seed, site, p) as in svg_op_dropout_mask, which draws the same mask; p = 0: no dropout.
 * svg_op_xf_gemm_tn: dW[N][K] (+)= dY[M][N]^T X[M][K], db[N] (+)= column sums of dY (db may be NULL); ldy / ldx: row strides of dY / X.
 * svg_op_xf_gemm_nn: out[M][K] = gate(dY[M][N] W[N][K]) + add; gate (M,K) or NULL: x * (gate > 0 ? gate_scale : 0); add (M,K) or NULL,
 *   may be `out` itself; *splits (or NULL) receives the number of contraction chunks the launch used (the slabs come from the arena).
 * svg_op_xf_relu_drop: r = dropout(max(h, 0)).
 * svg_op_xf_add_ln_train: y = LayerNorm(x + dropout(r)) gamma + beta over rows of d <= 3072 (r may be NULL); keeps xhat (M,d), rstd (M).
 * svg_op_xf_ln_bwd: dz = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)); dz_drop (or NULL) = dz * the site's mask; dgamma / dbeta (d)
 *   (+)= column sums of dy xhat / dy.
 * svg_op_xf_attention_train: q (Tq,B,ldq), k / v (Tk,B,ldk), heads * hd columns each; mask (Tq,Tk) additive or NULL; P (B,heads,Tq,Tk)
 *   = softmax(q k^T / sqrt(hd) + mask), o (Tq,B,heads*hd) = dropout(P) v.  T <= 32.
 * svg_op_xf_attention_bwd: dq (Tq,B,lddq), dk / dv (Tk,B,lddk) from dout (Tq,B,heads*hd), q, k, v and the kept P.
 * svg_op_xf_embed_post_train: emb (B*T, d - d_txt) -> y (T,B,d) = dropout(v * scale + pe[pe_row[b]]), the last d_txt channels from text (B,d_txt).
 * svg_op_xf_embed_post_bwd: de (B*T, d_img) = dy (T,B,d)[:, :, :d_img] * mask * scale.
 * svg_op_xf_criterion: pred (Tt,B,D) rows t >= t0 against expected (B,Tt,D), D = 4 fh fw; dpred (Tt,B,D) device (rows < t0: zero),
 *   losses: FIVE HOST floats {total, mse, l1, gdl, contrastive}; synchronises the stream. */
int svg_op_xf_gemm_tn(svg_ctx* ctx, const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int M, int N, int K,
                      int accumulate, void* stream);
int svg_op_xf_gemm_nn(svg_ctx* ctx, const float* dY, int ldy, const float* W, float* out, int M, int N, int K, const float* gate,
                      float gate_scale, const float* add, int* splits, void* stream);
int svg_op_xf_relu_drop(svg_ctx* ctx, const float* h, float* r, int64_t n, uint64_t seed, int site, float p, void* stream);
int svg_op_xf_add_ln_train(svg_ctx* ctx, const float* x, const float* r, uint64_t seed, int site, float p, const float* gamma,
                           const float* beta, float* y, float* xhat, float* rstd, int M, int d, float eps, void* stream);
int svg_op_xf_ln_bwd(svg_ctx* ctx, const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* dz_drop,
                     uint64_t seed, int site, float p, float* dgamma, float* dbeta, int M, int d, int accumulate, void* stream);
int svg_op_xf_attention_train(svg_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldk, const float* mask, float* o,
                              float* P, int Tq, int Tk, int B, int heads, int hd, uint64_t seed, int site, float p, void* stream);
int svg_op_xf_attention_bwd(svg_ctx* ctx, const float* dout, const float* q, int ldq, const float* k, const float* v, int ldk,
                            const float* P, float* dq, int lddq, float* dk, float* dv, int lddk, int Tq, int Tk, int B, int heads, int hd,
                            uint64_t seed, int site, float p, void* stream);
int svg_op_xf_embed_post_train(svg_ctx* ctx, const float* emb, const float* pe, const int32_t* pe_row, const float* text, int d_txt,
                               float* y, int B, int T, int d, float scale, uint64_t seed, int site, float p, void* stream);
int svg_op_xf_embed_post_bwd(svg_ctx* ctx, const float* dy, float* de, int B, int T, int d, int d_img, float scale, uint64_t seed, int site,
                             float p, void* stream);
int svg_op_xf_criterion(svg_ctx* ctx, const float* pred, const float* expected, float* dpred, float* losses, int Tt, int B, int D, int t0,
                        int fh, int fw, float w_mse, float w_l1, float w_gdl, float alpha, float w_nce, float temperature, void* stream);
/* The kernels of the FVD evaluation one by one (test hooks: each is the launcher the I3D forward / svg_frechet_distance calls, nothing
 * is added).  Device buffers; activations f32 channels-last (B,T,H,W,C).
 * svg_op_conv3d: Unit3D without its BatchNorm arithmetic: x (B,T,H,W,Cin_pad), Cin_pad % 4 == 0; w / bias as svg_op_pack_conv3d leaves
 *   them (bias may be NULL); TF 'SAME' padding: the output sizes and front pads are computed inside from (size, k, stride) by the rule
 *   the model uses, out_thw receives {To, Ho, Wo}; y (B,To,Ho,Wo,ldc) of y_elems floats, of which channels [coff, coff + Cout) are
 *   written; k / stride: {t, h, w}.
 * svg_op_pack_conv3d: w (Cout,Cin,taps) in PyTorch's layout -> wout (Cout,taps,Cin_pad) (padded channels 0), bout (Cout); with gamma /
 *   beta / mean / var: BatchNorm (eval) folded in (wout = w gamma / sqrt(var + eps), bout = beta - mean gamma / sqrt(var + eps));
 *   otherwise bout = cbias, or 0 when that is NULL too.
 * svg_op_maxpool3d_same: MaxPool3dSamePadding, sizes and pads as for the conv (the zero padding takes part in the max); C % 4 == 0.
 * svg_op_avgpool_thw: x (B,T,HW,C) -> y (B,T-kt+1,C), the mean over kt frames x the whole plane.  svg_op_time_mean: x (B,To,C) -> y (B,C).
 * svg_op_ncthw_to_nthwc: x (B,C,T,H,W) -> y (B,T,H,W,Cp), channels C .. Cp-1 zero.
 * svg_op_fd_moments: x (n,d) f32 -> mean f64[d], cov f64[d][d] (unbiased); n >= 2, even d <= 2048 as svg_frechet_distance.
 * svg_op_sym_eig: symmetric A f64 (d,d), d even -> eig f64[d] (unordered), V f64 (d,d) whose column k is the eigenvector of eig[k]. */
int svg_op_conv3d(svg_ctx* ctx, const float* x, int B, int T, int H, int W, int Cin_pad, const float* w, const float* bias, float* y,
                  int64_t y_elems, int Cout, int ldc, int coff, const int* k, const int* stride, int relu, int* out_thw, void* stream);
int svg_op_pack_conv3d(svg_ctx* ctx, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                       const float* cbias, float* wout, float* bout, int Cout, int Cin, int Cin_pad, int taps, float eps, void* stream);
int svg_op_maxpool3d_same(svg_ctx* ctx, const float* x, float* y, int64_t y_elems, int B, int T, int H, int W, int C, const int* k,
                          const int* stride, int* out_thw, void* stream);
int svg_op_avgpool_thw(svg_ctx* ctx, const float* x, float* y, int B, int T, int HW, int C, int kt, void* stream);
int svg_op_time_mean(svg_ctx* ctx, const float* x, float* y, int B, int To, int C, void* stream);
int svg_op_ncthw_to_nthwc(svg_ctx* ctx, const float* x, float* y, int B, int C, int T, int H, int W, int Cp, void* stream);
int svg_op_fd_moments(svg_ctx* ctx, const float* x, int n, int d, double* mean, double* cov, void* stream);
int svg_op_sym_eig(svg_ctx* ctx, const double* A, int d, double* eig, double* V, void* stream);
/* MX block-scaled fp8 (BASELINE configs[4]): OCP e4m3 elements with one E8M0 scale per 32 consecutive K elements.
 * svg_op_quant_mx: x (rows,K) bf16 -> q (rows,K) e4m3 bytes, scales (rows,K/32) bytes; shared exponent floor(log2(amax)) - 8,
 * round to nearest even, saturating at +-448 (OCP MX v1.0).  K % 32 == 0. */
int svg_op_quant_mx(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t rows, int K, void* stream);
/* The activation quantiser of the MX fp8 conv path on caller buffers (test hook): x (P,C) 16-bit -> q (P,Cp) e4m3 bytes and scales
 * (P,Cp/32) bytes, Cp = C rounded up to 128; same conversion as svg_op_quant_mx, except that an all-zero block and the padding
 * channels C .. Cp - 1 get scale byte 127 (zero bytes).  C % 32 == 0. */
int svg_op_quant_act_mx(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t P, int C, void* stream);
/* C[M,N] = act(Q(A)[M,K] Q(W)[N,K]^T + bias + residual) on v_mfma_scale_f32_16x16x128_f8f6f4 (f32 accumulate), both operands
 * quantised on the fly by the routine above; act 0 none, 1 SiLU, 2 GELU.  K % 128 == 0, N % 4 == 0. */
int svg_op_gemm_fp8(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C,
                    int M, int N, int K, int act, int out_f32, void* stream);
/* svg_op_gemm_fp8 with the row strides of C (ldc >= N) and of the residual (ldr >= N), multiples of 4 elements, as the models' linear()
 * passes them; path (int[1], or NULL) receives the column tile of the kernel instantiation that was launched (64 / 128).  Test hook. */
int svg_op_gemm_fp8_ex(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C,
                       int M, int N, int K, int act, int out_f32, int ldc, int ldr, int* path, void* stream);
/* GroupNorm (+SiLU) on NHWC bf16. */
int svg_op_groupnorm(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta,
                     uint16_t* out, int B, int HW, int C, int groups, float eps, int silu,
                     void* stream);
/* GroupNorm on a full descriptor, optionally forced onto one kernel path (test hook).  x (B,HW,C1) and x2 (B,HW,C2, or NULL with
 * C2 = 0): the two sources of a channel concat [x | x2], 16-bit or (f32_in = 1) f32, separately allocated; gamma, beta (C1 + C2) f32
 * on the device; out (B,HW,C1+C2) 16-bit.  part1 / part2 (optional): producer column sums of each source, [B * tps][C_src][2] =
 * (sum, sum of squares) per row tile and channel, tps tiles per sample (the GemmArgs::gn_part layout).  C1 + C2 a multiple of 8 and
 * of groups, C1 a multiple of 8, groups <= 64, C1 + C2 <= 8192.
 * force = 0: the library's choice.  force = 1: exactly `kind` — 0 small<maxch, vw> (one launch; instantiated <5,8> <10,8> <5,4>
 * <20,4>; needs channels per group and C1 multiples of vw and HW * cpg / vw <= 256 * maxch), 1 stats+apply (any shape),
 * 2 finish+apply (needs part1, and part2 when C2 > 0).  A forced path the shape does not admit is an error before any launch.
 * path (int[8], or NULL) receives {kind, maxch, vw, CV, PL, nchunk, nblk, threads}: CV channel vectors x PL pixel lanes per block
 * of `threads` threads, the statistics grid (nchunk, B), the apply grid (nblk, B); zero where a path has none.
 * svg_op_groupnorm_mx: the same inputs (16-bit, force = 0) through the MX fp8 apply pass (kind 3, finish+apply_mx): q (B*HW, Cp)
 * e4m3 bytes and sc (B*HW, Cp/32) E8M0 bytes, Cp = C rounded up to 128 (padding channels: zero data, scale byte 127), stats
 * (B,groups,2) = the (mean, rstd) table it used.  *fused = 0 (nothing written, path kind -1) when the pass does not serve the call:
 * no column sums for a source, C % 32 != 0, or SVG_GN_MX=0 / SVG_GN_EPI=0.
 * Numerics contract of every GroupNorm path (and of svg_op_gn_finish / svg_op_ln_finish): the variance is the one-pass form
 * E[x^2] - mean^2 in f32.  With e = 2^-24, L the longest run of sequential f32 additions of the path (small<M,V>: M V + 8, at most 88;
 * stats+apply: pixels per thread + 2048 / groups + nchunk; finish: column-sum entries per thread + 8) and k = |mean| / sigma of a group,
 * rstd is within e (3 L + 5) (1 + k^2) / 2 relative of exact arithmetic on the same inputs, and so is the output next to its own
 * rounding.  That reaches one output ulp (2^-7 bf16, 2^-10 fp16) at k = sqrt(2^18 / (3 L + 5)) in bf16 and sqrt(2^15 / (3 L + 5)) in
 * fp16: k = 31 and 11 at L = 88; below that the result is the fp64 one to within two output roundings.  A constant group (var = 0) comes
 * out as beta within |gamma| (L + 1) e |mean| rsqrt(eps).  The bound is a worst case; DESIGN.md lists the errors measured against fp64.
 * An all-zero 32-channel block of the MX output carries scale byte 127 (svg_op_quant_mx writes 0 there); both decode to zeros. */
typedef struct svg_gn_desc {
  const void *x, *x2;
  int C1, C2, f32_in;
  const float *gamma, *beta;
  uint16_t* out;
  int B, HW, groups;
  float eps;
  int silu;
  const float* part1;
  int tps1;
  const float* part2;
  int tps2;
  int force, kind, maxch, vw;
  uint8_t *q, *sc;
  float* stats;
} svg_gn_desc;
int svg_op_groupnorm_ex(svg_ctx* ctx, const svg_gn_desc* desc, int* path, void* stream);
int svg_op_groupnorm_mx(svg_ctx* ctx, const svg_gn_desc* desc, int* fused, int* path, void* stream);
/* (mean, rstd) per (sample, group) from producer column sums (layout as part1 / part2 above) -> stats (B,groups,2) (test hook) */
int svg_op_gn_finish(svg_ctx* ctx, const float* part1, int C1, int tps1, const float* part2, int C2, int tps2, float* stats, int B,
                     int HW, int groups, float eps, void* stream);
/* GroupNorm folded into a following 1x1 projection: Wb (B,N,C) 16-bit = W[n][c] gamma[c] rstd[b][g(c)], bb (B,N) = bias[n] (0 when
 * NULL) + sum_c W[n][c] (beta[c] - mean rstd gamma[c]); W (N,C), stats (B,groups,2) f32 on the device (test hook) */
int svg_op_gn_fold_weights(svg_ctx* ctx, const float* W, const float* bias, const float* gamma, const float* beta, const float* stats,
                           uint16_t* Wb, float* bb, int B, int N, int C, int groups, void* stream);
/* LayerNorm row statistics rs[m] = rstd, rm[m] = rstd * mean of x (M,C) 16-bit (two passes over the row in registers), and the
 * same from `tiles` (sum, sum of squares) partials per row, part (M,tiles,2) (one pass: E[x^2] - mean^2).  C % 8 == 0, C <= 2048. */
int svg_op_ln_stats(svg_ctx* ctx, const uint16_t* x, float* rs, float* rm, int M, int C, float eps, void* stream);
int svg_op_ln_finish(svg_ctx* ctx, const float* part, int tiles, float* rs, float* rm, int M, int C, float eps, void* stream);
/* rows of f32 scores (row stride ld_in) -> 16-bit softmax(s * scale) (row stride ld_out); output columns cols .. ld_out - 1 are
 * written as zero, input columns >= cols are never read */
int svg_op_softmax_rows(svg_ctx* ctx, const float* s_in, uint16_t* p_out, int64_t rows, int cols, int ld_in, int ld_out, float scale,
                        void* stream);
/* LayerNorm folding at load time: bias_out[n] = bias_in[n] (0 when NULL) + sum_k w[n][k] beta[k], then w[n][k] *= gamma[k] in place;
 * and out[n] = sum_k w[n][k] of a 16-bit (N,K) matrix */
int svg_op_fold_ln(svg_ctx* ctx, float* w, const float* bias_in, const float* gamma, const float* beta, float* bias_out, int N, int K,
                   void* stream);
int svg_op_rowsum(svg_ctx* ctx, const uint16_t* w, float* out, int N, int K, void* stream);
/* The element-wise and layout kernels at the VAE / UNet boundary (csrc/eltwise.hip) and add_noise of the sampling loop, one by one
 * (test hooks: each checks its arguments and calls the launcher the models call, nothing is added).  Device buffers.
 * svg_op_img_to_act: img (N,sh,sw,3) u8 -> out (N,H,W,8) 16-bit = 2 (p / 255 - 0.5), channels 3..7 zero; (sh,sw) != (H,W): nearest source
 *   pixel floor(dst * in / out) in f32, as svg_resize_nearest_u8; out 16-byte aligned.
 * svg_op_act_to_img: x (N,h,w,ldc) f32, channels 0..2 -> img (N,oh,ow,3) u8 = round-half-even(clamp(x / 2 + 0.5, 0, 1) 255), nearest
 *   resized, and / or float_out (N,3,h,w) f32 = the same channels untouched; either may be NULL, not both.
 * svg_op_nchw_to_act: x (N,C,h,w) f32 -> out (N,h,w,Cpad) 16-bit = x * scale, channels C..Cpad-1 zero.  svg_op_nchw_to_actf32: the same
 *   to (N,h,w,C) f32.  svg_op_actf32_pad_h16: x (P,C) f32 -> out (P,Cpad) 16-bit, zero padded.
 * svg_op_actf32_to_nchw: x (N,h,w,ld) f32, ld >= C -> out (N,C,h,w) f32.
 * svg_op_pixel_linear_f32: y[p][o] = b[o] (0 when NULL) + sum_i w[o][i] x[p][i] over P pixels; row strides ldx, ldy; Cin <= 8.
 * svg_op_vae_sample: mom (N,h,w,ldm) f32 = [mean(4) | logvar(4) | ...] -> z (N,4,h,w) = 0.18215 (mean + exp(0.5 clamp(logvar, -30, 20)) eps),
 *   eps (N,4,h,w) or NULL (the mode: 0.18215 mean); mom_nchw (N,8,h,w, or NULL) receives the moments as they came (logvar not clamped).
 * svg_op_concat_channels: out (P,Ca+Cb) = [a (P,Ca) | b (P,Cb)] 16-bit; Ca, Cb multiples of 8, pointers 16-byte aligned.
 * svg_op_f32_to_h16 / svg_op_h16_to_f32: n elements, round to nearest even / exact.  svg_op_f32_to_h16_x8: the same conversion eight
 *   elements per thread; n % 8 == 0, x 32-byte and y 16-byte aligned, anything else is an error.
 * svg_op_timestep_embed: t f32[N] -> out (N,dim) 16-bit = [cos | sin](t exp(-ln(10000) i / (dim / 2))), i < dim / 2; dim even.
 * svg_op_add_noise: out = sa x0 + s1a noise over n floats; out may be x0. */
int svg_op_img_to_act(svg_ctx* ctx, const uint8_t* img, uint16_t* out, int N, int sh, int sw, int H, int W, void* stream);
int svg_op_act_to_img(svg_ctx* ctx, const float* x, int ldc, uint8_t* img, float* float_out, int N, int h, int w, int oh, int ow,
                      void* stream);
int svg_op_nchw_to_act(svg_ctx* ctx, const float* x, uint16_t* out, int N, int C, int h, int w, int Cpad, float scale, void* stream);
int svg_op_nchw_to_actf32(svg_ctx* ctx, const float* x, float* out, int N, int C, int h, int w, float scale, void* stream);
int svg_op_actf32_pad_h16(svg_ctx* ctx, const float* x, int C, uint16_t* out, int Cpad, int64_t P, void* stream);
int svg_op_actf32_to_nchw(svg_ctx* ctx, const float* x, int ld, float* out, int N, int C, int h, int w, void* stream);
int svg_op_pixel_linear_f32(svg_ctx* ctx, const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int64_t P, int Cin,
                            int Cout, void* stream);
int svg_op_vae_sample(svg_ctx* ctx, const float* mom, int ldm, const float* eps, float* z, float* mom_nchw, int N, int h, int w,
                      void* stream);
int svg_op_concat_channels(svg_ctx* ctx, const uint16_t* a, int Ca, const uint16_t* b, int Cb, uint16_t* out, int64_t P, void* stream);
int svg_op_f32_to_h16(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream);
int svg_op_f32_to_h16_x8(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream);
int svg_op_h16_to_f32(svg_ctx* ctx, const uint16_t* x, float* y, int64_t n, void* stream);
int svg_op_timestep_embed(svg_ctx* ctx, const float* t, uint16_t* out, int N, int dim, void* stream);
int svg_op_add_noise(svg_ctx* ctx, const float* x0, const float* noise, float* out, int64_t n, float sa, float s1a, void* stream);
/* The update kernels of the sampling loop (csrc/sampler.hip), one by one on caller data (test hooks: each checks its arguments on the
 * host and calls the launcher the loop calls).  f32 device buffers of n elements; eps = eps_u + guidance (eps_c - eps_u), or eps_u when
 * eps_c is NULL.  The row (8 floats, laid out per rule as in csrc/sampler_plan.h) is given in exactly one of two ways: `row`, 8 HOST
 * floats, or row idx[0] of the DEVICE table `tab` under the DEVICE counter `idx`; the other way's pointers are NULL.  Nothing on the host
 * can check idx[0] against the size of the table.  A null tensor, n < 0 or a row given both ways or neither is SVG_ERR_INVALID, and
 * nothing is launched.
 * svg_op_ddim_step: x_out = DDIM step with clip_sample; x_out may be x.
 * svg_op_dpmpp_step: x_out = DPM-Solver++(2M) step, m_out (may be NULL) = the x0 prediction; m_prev is read only by a second-order row
 *   (row[5] != 0).  x_out may be x and m_out may be m_prev.  Refused: a second-order argument row with m_prev NULL, and ANY table row
 *   with m_prev NULL (its order is on the device).
 * svg_op_lms_step: x_out = x + sum_k c_k d_{i-k}, the combined eps stored to slot i & 3 of the ring dhist (4 x n floats); x_out may be x.
 *   `order` and `step` are read for a table row only, where the caller must state what the row holds: both, like those of an argument
 *   row, are refused unless step >= 0 and 1 <= order <= min(4, step + 1).
 * svg_op_lms_input: o0 (and o1 unless NULL) = x * c, c the argument or, with tab and idx, element 1 of the table row; o0 may be x.
 * svg_op_sampler_tvec: tvec[0 .. nb-1] = element 0 (the timestep) of the table row idx[0]; nb > 0.
 * svg_op_sampler_bump: idx[0] += 1. */
int svg_op_ddim_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, float* x_out, int64_t n,
                     const float* row, const float* tab, const int* idx, void* stream);
int svg_op_dpmpp_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, const float* m_prev,
                      float* x_out, float* m_out, int64_t n, const float* row, const float* tab, const int* idx, void* stream);
int svg_op_lms_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, float* dhist, float* x_out,
                    int64_t n, const float* row, const float* tab, const int* idx, int order, int step, void* stream);
int svg_op_lms_input(svg_ctx* ctx, const float* x, float* o0, float* o1, int64_t n, float c, const float* tab, const int* idx,
                     void* stream);
int svg_op_sampler_tvec(svg_ctx* ctx, float* tvec, int nb, const float* tab, const int* idx, void* stream);
int svg_op_sampler_bump(svg_ctx* ctx, int* idx, void* stream);
/* LayerNorm over the last dim of (M,C) bf16. */
int svg_op_layernorm(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta,
                     uint16_t* out, int M, int C, float eps, void* stream);
/* softmax(Q K^T * scale) V per (batch, head).  q (B,Sq,heads*d) bf16 row stride ldq; k (B,Skv,·)
 * row stride ldk; vt (B,heads*d,SkvPad) = V transposed, row stride ldvt (kv contiguous);
 * out (B,Sq,heads*d) row stride ldo.  Skv valid keys (columns >= Skv are masked). */
int svg_op_attention(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, const uint16_t* vt,
                     uint16_t* out, int B, int heads, int Sq, int Skv, int d, int ldq, int ldk,
                     int ldvt, int ldo, int64_t q_bstride, int64_t k_bstride, int64_t vt_bstride,
                     int64_t o_bstride, float scale, void* stream);
/* svg_op_attention on a full descriptor, optionally forced onto one kernel instantiation (test hook).  Fields as svg_op_attention
 * (qb / kb / vtb / ob: batch strides in elements; kb = vtb = 0 shares one context between all samples).  d: 8, 16, 32, 40, 64, 80
 * or 160; strides multiples of 8 elements (ldo: of 4); ldvt >= Skv rounded up to 8.
 * V^T pad contract: the kernels stage V^T in whole 8-key chunks, so the pad keys Skv .. ceil8(Skv) - 1 of every V^T row are read and
 * multiplied by P = 0; they must be finite (0 * Inf or NaN is NaN).  Columns from ceil8(Skv) on are never read.  The models write
 * finite values there: the V^T projection masks the padded token rows of its B operand (n_valid), so they hold the bias.
 * force = 0: the library's own choice (SVG_ATTN_QB / NST / BC / HV / DMA and Sq >= 512, as svg_op_attention).  force = 1: exactly
 * {kernel, qblocks, nst, bc, hv}: kernel 0 = attn_kernel<d, qblocks (1, or 2 for d <= 64), nst (LDS stages: 1, or 2 without bc and
 * d != 160), bc (bias columns: d = 8 or 40, nst 1), hv (V^T read ahead: bc and qblocks 2)>, kernel 1 = attn_dma40_kernel (d = 40,
 * given as qblocks 2, nst 3, bc 1, hv 1).  A forced variant that is not instantiated for d, an unsupported d, a short ldvt or a
 * misaligned stride return an error without launching anything.  path (int[6], or NULL) receives what ran: {kernel, d, qblocks,
 * nst, bc, hv}. */
typedef struct svg_attn_desc {
  const uint16_t *q, *k, *vt;
  uint16_t* out;
  int B, heads, Sq, Skv, d;
  int ldq, ldk, ldvt, ldo;
  int64_t qb, kb, vtb, ob;
  float scale;
  int force, kernel, qblocks, nst, bc, hv;
} svg_attn_desc;
int svg_op_attention_ex(svg_ctx* ctx, const svg_attn_desc* desc, int* path, void* stream);
/* The VAE mid block's fused single-head attention (d = C = 512) whatever SVG_VAE_ATTN_FUSED says (test hook): per sample b,
 * out[b] = softmax(q[b] k[b]^T / sqrt(C)) v[b] over S keys.  q, k: rows of stride ldqk (the model passes one [q | k] buffer,
 * ldqk = 2C), sample stride qkb; vt (B, C, ldvt) = V transposed, sample stride vtb; out rows of stride ldo, sample stride ob.
 * S % 64 != 0, C != 512, strides not multiples of 8 (ldo: 4), ldqk < C, ldvt < S or ldo < C return an error. */
int svg_op_vae_attention(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, int ldqk, int64_t qkb, const uint16_t* vt, int ldvt,
                         int64_t vtb, uint16_t* out, int ldo, int64_t ob, int B, int S, int C, void* stream);
/* fp16-storage twins of the hooks above (identical contracts; 16-bit buffers hold IEEE half) */
int svg_op_gemm_f16(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C, int M,
                    int N, int K, int act, int out_f32, void* stream);
int svg_op_conv3x3_f16(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, uint16_t* out, int B, int H, int W,
                       int Cin, int Cout, int mode, void* stream);
int svg_op_conv3x3_gn_f16(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const float* gamma,
                          const float* beta, uint16_t* conv_out, uint16_t* gn_out, int B, int H, int W, int Cin, int Cout,
                          int groups, float eps, int silu, int* used_epilogue_stats, void* stream);
int svg_op_gemm_lnstats_f16(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual,
                            uint16_t* C, int M, int N, int K, int batch, float* rs, float* rm, int* used, void* stream);
int svg_op_gemm_ex_f16(svg_ctx* ctx, const svg_gemm_desc* desc, int* path, void* stream);
int svg_op_gemm_plan_f16(svg_ctx* ctx, const svg_gemm_desc* desc, int* plan);
int svg_op_gemm_cat_f16(svg_ctx* ctx, const uint16_t* A, const uint16_t* A2, const uint16_t* W, const float* bias, uint16_t* C,
                        int M, int N, int K, int k_split, void* stream);
int svg_op_ff_fused_f16(svg_ctx* ctx, const uint16_t* x, const float* ln_gamma, const float* ln_beta, const float* w1,
                        const float* b1, const float* w2, const float* b2, const uint16_t* residual, uint16_t* out, int M, int C,
                        void* stream);
int svg_op_xattn_fused_f16(svg_ctx* ctx, const uint16_t* x, const uint16_t* a, const uint16_t* r, const float* wp, const float* bp,
                           const float* ln_gamma, const float* ln_beta, const float* wq, const uint16_t* k, const uint16_t* vt, int Lp,
                           const float* wo, const float* bo, uint16_t* out, int M, int rows_per_sample, int L, void* stream);
int svg_op_conv3x3_mx_f16(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual,
                          uint16_t* out, uint8_t* q_out, uint8_t* s_out, int B, int H, int W, int Cin, int Cout, int mode, void* stream);
int svg_op_quant_mx_f16(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t rows, int K, void* stream);
int svg_op_gemm_fp8_f16(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C,
                        int M, int N, int K, int act, int out_f32, void* stream);
int svg_op_quant_act_mx_f16(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t P, int C, void* stream);
int svg_op_conv3x3_mx_ex_f16(svg_ctx* ctx, const svg_conv_mx_desc* desc, int* path, void* stream);
int svg_op_gemm_fp8_ex_f16(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C,
                           int M, int N, int K, int act, int out_f32, int ldc, int ldr, int* path, void* stream);
int svg_op_groupnorm_f16(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta, uint16_t* out, int B, int HW,
                         int C, int groups, float eps, int silu, void* stream);
int svg_op_conv3x3_f32s_f16(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual,
                            const float* residual_f32, float* out, const float* gamma, const float* beta, uint16_t* gn_out, int B, int H,
                            int W, int Cin, int Cout, int mode, int groups, float eps, int silu, int* halo_width, int* used_epilogue_stats,
                            void* stream);
int svg_op_groupnorm_f32_f16(svg_ctx* ctx, const float* x, const float* gamma, const float* beta, uint16_t* out, int B, int HW, int C,
                             int groups, float eps, int silu, void* stream);
int svg_op_layernorm_f16(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta, uint16_t* out, int M, int C,
                         float eps, void* stream);
int svg_op_attention_f16(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int heads,
                         int Sq, int Skv, int d, int ldq, int ldk, int ldvt, int ldo, int64_t q_bstride, int64_t k_bstride,
                         int64_t vt_bstride, int64_t o_bstride, float scale, void* stream);
int svg_op_attention_ex_f16(svg_ctx* ctx, const svg_attn_desc* desc, int* path, void* stream);
int svg_op_vae_attention_f16(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, int ldqk, int64_t qkb, const uint16_t* vt, int ldvt,
                             int64_t vtb, uint16_t* out, int ldo, int64_t ob, int B, int S, int C, void* stream);
int svg_op_groupnorm_ex_f16(svg_ctx* ctx, const svg_gn_desc* desc, int* path, void* stream);
int svg_op_groupnorm_mx_f16(svg_ctx* ctx, const svg_gn_desc* desc, int* fused, int* path, void* stream);
int svg_op_gn_fold_weights_f16(svg_ctx* ctx, const float* W, const float* bias, const float* gamma, const float* beta, const float* stats,
                               uint16_t* Wb, float* bb, int B, int N, int C, int groups, void* stream);
int svg_op_ln_stats_f16(svg_ctx* ctx, const uint16_t* x, float* rs, float* rm, int M, int C, float eps, void* stream);
int svg_op_softmax_rows_f16(svg_ctx* ctx, const float* s_in, uint16_t* p_out, int64_t rows, int cols, int ld_in, int ld_out, float scale,
                            void* stream);
int svg_op_rowsum_f16(svg_ctx* ctx, const uint16_t* w, float* out, int N, int K, void* stream);
int svg_op_img_to_act_f16(svg_ctx* ctx, const uint8_t* img, uint16_t* out, int N, int sh, int sw, int H, int W, void* stream);
int svg_op_nchw_to_act_f16(svg_ctx* ctx, const float* x, uint16_t* out, int N, int C, int h, int w, int Cpad, float scale, void* stream);
int svg_op_actf32_pad_h16_f16(svg_ctx* ctx, const float* x, int C, uint16_t* out, int Cpad, int64_t P, void* stream);
int svg_op_concat_channels_f16(svg_ctx* ctx, const uint16_t* a, int Ca, const uint16_t* b, int Cb, uint16_t* out, int64_t P, void* stream);
int svg_op_f32_to_h16_f16(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream);
int svg_op_f32_to_h16_x8_f16(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream);
int svg_op_h16_to_f32_f16(svg_ctx* ctx, const uint16_t* x, float* y, int64_t n, void* stream);
int svg_op_timestep_embed_f16(svg_ctx* ctx, const float* t, uint16_t* out, int N, int dim, void* stream);
/* f32 skinny GEMM of the latent Transformer: Y[M,N] = X[M,K] * W[N,K]^T + bias (relu_in: X:=max(X,0)). */
int svg_op_xf_gemm(svg_ctx* ctx, const float* X, const float* W, const float* bias, float* Y,
                   int M, int N, int K, int relu_in, void* stream);
/* The forward kernels of the latent Transformer, the CLIP text tower and the MiniLM sentence encoder one by one (test hooks: each is
 * its launcher, nothing is added; f32 device buffers).  Each hook checks what its launcher assumes of its arguments and returns
 * SVG_ERR_INVALID without launching when a check fails.
 * svg_xf_gemm_describe: host only (no context, no device): path[3] = {form, mt, ksplit} of the launch svg_op_xf_gemm(_ex) makes for
 *   (M, N, K): form 1 = 16-column form, 2 = column-block form; mt = accumulator height in 16-row tiles; ksplit = split-K factor.
 * svg_op_xf_gemm_ex: Y[M,N] = act_in(X[M,K]) W[N,K]^T + bias[N] + residual[M,N]; bias / residual may be NULL; act_in 0 none, 1 ReLU,
 *   2 quick-GELU, 3 exact GELU; 1 <= M <= 336, K % 8 == 0, N % 4 == 0; path (or NULL) receives the three ints of the launch made.
 * svg_op_xf_add_ln: y = LayerNorm(x + r) gamma + beta over M rows of d <= 3072 (r may be NULL).
 * svg_op_xf_embed_post: emb (B*T, d - d_txt) -> y (T,B,d) = v * scale + pe[pe_row[b]]; the last d_txt channels of every token come
 *   from text (B,d_txt); pe is a table of 64 rows of d: pe_row (B int32, or NULL: row b, B <= 64) holds values in 0..63.
 * svg_op_xf_attention: o (Tq,B,heads*hd) = softmax(q k^T / sqrt(hd) + mask + kpad) v per (batch row, head); q rows (t*B + b) of
 *   stride ldq, k / v rows of stride ldk; mask (Tq,Tk) and kpad (B,Tk) additive, may be NULL; Tq, Tk <= 32.
 * svg_op_xf_attention_qkv: packed rows (b*T + t) of [q | k | v] (3*heads*hd floats) -> o (B*T, heads*hd); lens NULL: causal (CLIP);
 *   lens (B int32): bidirectional over the first clamp(lens[b], 1, T) keys (BERT); T <= 128, hd <= 64.
 * svg_op_xf_embed_tokens: y[row] = tok[clamp(ids[row], 0, vocab-1)] + pos[row % T]; svg_op_xf_embed_bert: + type0; d % 4 == 0.
 * svg_op_xf_mean_pool_norm: out[b] = normalize(mean of the first clamp(lens[b], 0, T) rows of x[b]) (zeros for no rows).
 * svg_op_xf_walk: one layer-walking launch over a caller's stage table (small != 0: the small-row form, rows is ignored and 8 is
 *   taken); the table passes the launch's own validation; the hook waits for the launch and raises a barrier give-up; info[4] receives
 *   {workgroups of the launch, dynamic LDS bytes, accumulator height (0: small-row form), sizeof(svg_walk_stage)}.  SVG_ERR_RUNTIME
 *   when the walk is unavailable. */
typedef struct svg_walk_stage {
  int32_t kind, bar;            /* 0 GEMM, 1 RED, 2 LN, 3 ATTN, 4 EMBED, 5 GEMMF; bar: device-wide barrier before the stage */
  int32_t M, N, K, ld;          /* GEMM(F): X is M x K with row stride ld, W is N x K; RED / LN / EMBED: an M x N result */
  int32_t ksplit, relu;         /* slabs to add up (GEMM: K / 128; LN: 0 = none); ReLU on the result (RED, GEMMF) */
  const float *X, *W;
  float* slab;
  const float *bias, *res;
  float* Y;
  const float *g1, *b1, *g2, *b2;
  float* Y2;
  float eps;
  int32_t Tq, Tk, B, heads, hd; /* ATTN (B, T also EMBED / GEMMF with perm or pe) */
  int32_t q_ld, kv_ld, q_span, kv_span;
  const float *qs, *ks, *vs, *mask, *kpad;
  const float* pe;              /* EMBED / GEMMF: 64 rows (of N + d_txt floats / of ld_res floats) */
  const int32_t* pe_row;
  const float* text;
  int32_t d_txt, T;
  float scale;
  int32_t ldy, ld_res, reuse_x, perm;   /* GEMMF */
  float* Yln;
} svg_walk_stage;
int svg_xf_gemm_describe(int M, int N, int K, int* path);
int svg_op_xf_gemm_ex(svg_ctx* ctx, const float* X, const float* W, const float* bias, const float* residual, float* Y, int M, int N, int K,
                      int act_in, int* path, void* stream);
int svg_op_xf_add_ln(svg_ctx* ctx, const float* x, const float* r, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                     void* stream);
int svg_op_xf_embed_post(svg_ctx* ctx, const float* emb, const float* pe, const int32_t* pe_row, const float* text, int d_txt, float* y, int B,
                         int T, int d, float scale, void* stream);
int svg_op_xf_attention(svg_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldk, const float* mask, const float* kpad,
                        float* o, int Tq, int Tk, int B, int heads, int hd, void* stream);
int svg_op_xf_attention_qkv(svg_ctx* ctx, const float* qkv, const int32_t* lens, float* o, int B, int T, int heads, int hd, void* stream);
int svg_op_xf_embed_tokens(svg_ctx* ctx, const int32_t* ids, const float* tok, const float* pos, float* y, int rows, int T, int d, int vocab,
                           void* stream);
int svg_op_xf_embed_bert(svg_ctx* ctx, const int32_t* ids, const float* word, const float* pos, const float* type0, float* y, int rows, int T,
                         int d, int vocab, void* stream);
int svg_op_xf_mean_pool_norm(svg_ctx* ctx, const float* x, const int32_t* lens, float* out, int B, int T, int d, void* stream);
int svg_op_xf_walk(svg_ctx* ctx, const svg_walk_stage* stages, int n_stages, int rows, int small, int* info, void* stream);

/* ---- measurement ---------------------------------------------------------------------------- */
/* When enabled (on = 1), every launch of each kernel family is bracketed by hipEvents on its stream;
 * svg_prof_report waits for the context's own brackets (no device-wide sync) and writes "name calls total_ms flops bytes\n" lines into buf.
 * on = 2 additionally keeps one entry per call-site signature, reported as "@family|shape ..." lines. */
int svg_prof_enable(svg_ctx* ctx, int on);
int svg_prof_reset(svg_ctx* ctx);
int svg_prof_report(svg_ctx* ctx, char* buf, int buflen);
/* Has a layer-walking forward of the latent Transformer (models/transformer.py:47-68 in one launch, xf_walk.hip) on this device given up at a
 * device-wide barrier since the last Transformer call / status query?  0 = no; SVG_ERR_RUNTIME = yes: that forward's output is NaN-filled,
 * the walk is now off for the device (later forwards run the per-GEMM kernels) and the forward must be re-issued.  Call it where the
 * forward's result is consumed (after synchronising its stream).  The event is also raised by the next svg_transformer_* call; the VAE /
 * UNet / DDIM entry points log it and keep running. */
int svg_transformer_status(svg_ctx* ctx);
/* workspace bytes currently reserved by the context */
int64_t svg_workspace_bytes(svg_ctx* ctx);

/* ---- workspace ownership ("workspace arena sized at svg_create / first call; no allocation in steady state") ----
 * The reference has no counterpart: torch's caching allocator serves its intermediates (utils/sd_utils.py:247-261 allocates per
 * step).  Here every model call plans its intermediates into one arena per context.  A caller sizes it once:
 *   svg_reserve_workspace   at least `bytes` of workspace from now on;
 *   svg_plan_begin .. svg_plan_end   every model call in between runs its planning pass ONLY (nothing is launched, outputs are
 *                           not written) and records its need; svg_plan_end reserves the largest and returns it in *bytes
 *                           (the cross-attention K / V cache of svg_ddim_loop is sized too).
 * A call that still needs more grows the arena without freeing or synchronising (the outgrown block is released by the next
 * reserve / plan end / svg_destroy): safe while another thread of the process captures a stream.
 * svg_workspace_growths: (re)allocations since svg_create — constant once the workload has been planned.
 * Threads: one context per thread; svg_destroy, svg_model_configure, svg_finalize and svg_reserve_workspace synchronise the device
 * and therefore wait for any other thread's capture window inside the library (the DDIM loop's, the training step's) to close. */
int svg_reserve_workspace(svg_ctx* ctx, int64_t bytes);
int svg_plan_begin(svg_ctx* ctx);
int svg_plan_end(svg_ctx* ctx, int64_t* bytes);
int64_t svg_workspace_growths(svg_ctx* ctx);
/* capture windows open inside the library right now, over all contexts of the process (tests: drive a call into another
 * thread's window, $SVG_TEST_CAPTURE_HOLD_MS keeps svg_ddim_loop's open) */
int svg_debug_captures_active(void);
#ifdef __cplusplus
}
#endif
#endif /* SVG_HIP_H */
