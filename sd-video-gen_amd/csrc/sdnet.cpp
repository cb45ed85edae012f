// Shared pieces of the SD networks (VAE, UNet): weight packing by state_dict name and the
// conv / linear / resnet building blocks over NHWC bf16 activations.
#include "models.h"
#include <algorithm>
#include <cstdlib>

namespace SDNS {

// elements one kernel launch may address per operand (32-bit byte offsets); $SVG_CHUNK_LIMIT lowers it so that the tests can
// drive the batch / row chunking of conv3x3() and linear() at small sizes (cached; the tests toggle it in-process and call svg_env_refresh)
static int64_t chunk_limit() {
  const int64_t full = (1LL << 31) - 1;
  const int64_t v = svg_env_i64("SVG_CHUNK_LIMIT", full);
  return v > 0 && v < full ? v : full;
}

float* keep_f32(svg_ctx* ctx, WeightStore& ws, const std::string& name, int64_t numel) {
  const Weight& w = ws.get(name);
  SVG_CHECK(w.numel == numel, "weight %s has %lld elements, expected %lld", name.c_str(), (long long)w.numel, (long long)numel);
  return w.f32;   // stays in the store (small 1-D parameters)
}

ConvW load_conv3x3(svg_ctx* ctx, WeightStore& ws, const std::string& prefix, int Cin, int Cout, hipStream_t s, bool fp8) {
  const Weight& w = ws.get(prefix + ".weight", {Cout, Cin, 3, 3});
  ConvW cw;
  cw.Cout = Cout;
  cw.Opad = (int)align_up(Cout, 4);
  cw.Cin = (Cin < 64) ? 8 : Cin;       // small-Cin convs (image / latent inputs) run on 8 padded channels
  SVG_CHECK(Cin <= 8 || Cin % 64 == 0, "conv %s: Cin=%d must be <= 8 or a multiple of 64", prefix.c_str(), Cin);
  cw.w = (h16*)ctx->dalloc((int64_t)cw.Opad * 9 * cw.Cin * sizeof(h16));
  pack_conv3x3(w.f32, cw.w, Cout, Cin, cw.Opad, cw.Cin, s);
  cw.b = (float*)ctx->dalloc(cw.Opad * sizeof(float));
  HIP_OK(hipMemsetAsync(cw.b, 0, cw.Opad * sizeof(float), s));
  HIP_OK(hipMemcpyAsync(cw.b, keep_f32(ctx, ws, prefix + ".bias", Cout), Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (fp8 && Cin % 64 == 0 && cw.Opad >= 128) {   // MX fp8 copy, quantised from the f32 weights (one rounding, not two)
    cw.Cp = (int)align_up(Cin, 128);
    cw.w8 = (uint8_t*)ctx->dalloc((int64_t)cw.Opad * 9 * cw.Cp);
    cw.w8s = (uint8_t*)ctx->dalloc((int64_t)9 * (cw.Cp / 128) * cw.Opad * 4);
    pack_conv3x3_mx(w.f32, cw.w8, cw.w8s, Cout, Cin, cw.Opad, cw.Cp, s);
  }
  HIP_OK(hipStreamSynchronize(s));
  ws.release(prefix + ".weight");
  return cw;
}

PackedLinear load_linear(svg_ctx* ctx, WeightStore& ws, const std::string& prefix, int N, int K, bool bias, hipStream_t s,
                         const NormW* fold) {
  const Weight& w = ws.get(prefix + ".weight");
  SVG_CHECK(w.numel == (int64_t)N * K && w.shape[0] == N, "weight %s.weight: expected [%d,%d(,1,1)]", prefix.c_str(), N, K);
  PackedLinear pl;
  pl.N = (int)align_up(N, 4); pl.K = K; pl.n_valid = N;
  pl.w = (h16*)ctx->dalloc((int64_t)pl.N * K * sizeof(h16));
  if (bias || fold) {
    pl.b = (float*)ctx->dalloc(pl.N * sizeof(float));
    HIP_OK(hipMemsetAsync(pl.b, 0, pl.N * sizeof(float), s));
    if (bias) HIP_OK(hipMemcpyAsync(pl.b, keep_f32(ctx, ws, prefix + ".bias", N), N * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  if (fold) {   // b += W beta, W *= gamma (on the f32 copy, which is released below), before the bf16 rounding
    SVG_CHECK(fold->C == K, "fold: norm width %d != K %d", fold->C, K);
    fold_ln_weights(w.f32, pl.b, fold->g, fold->b, pl.b, N, K, s);
  }
  pack_linear(w.f32, pl.w, N, K, pl.N, s);
  if (fold) {
    pl.ln_s = (float*)ctx->dalloc(pl.N * sizeof(float));
    rowsum_h16(pl.w, pl.ln_s, pl.N, K, s);
  }
  HIP_OK(hipStreamSynchronize(s));
  ws.release(prefix + ".weight");
  return pl;
}

void add_fp8_copy(svg_ctx* ctx, PackedLinear& pl, hipStream_t s) {
  if (!pl.w || pl.ln_s || pl.K % 128 != 0 || pl.N % 4 != 0 || pl.w8) return;
  pl.w8 = (uint8_t*)ctx->dalloc((int64_t)pl.N * pl.K);
  pl.w8s = (uint8_t*)ctx->dalloc((int64_t)pl.N * (pl.K / 32));
  quant_mx_h16(ctx, pl.w, pl.K, pl.w8, pl.w8s, pl.N, pl.K, s);
  HIP_OK(hipStreamSynchronize(s));
}

NormW load_norm(svg_ctx* ctx, WeightStore& ws, const std::string& prefix, int C) {
  NormW n;
  n.C = C;
  n.g = keep_f32(ctx, ws, prefix + ".weight", C);
  n.b = keep_f32(ctx, ws, prefix + ".bias", C);
  return n;
}

GnEmit emit_for(svg_ctx* ctx, int N, int64_t hw, int Cout) {
  GnEmit e;
  if (hw >= 1024) e.buf = ctx->arena.get<float>(gn_part_floats(N, hw, Cout));
  return e;
}

// fills g.gn_part / emit->st when the launch of g leaves the output's GroupNorm column sums per `rows` output rows (gemm_plan()'s
// gn_rows, or the 16 x 16 pixel block of the fp8 halo conv) and a sample is whole row tiles
static void attach_gn_emit(GemmArgs& g, GnEmit* emit, int rows_per_sample, int rows) {
  if (!emit || !emit->buf || rows_per_sample < 1024) return;   // small images take the single-launch GroupNorm (one read)
  if (rows <= 0 || rows_per_sample % rows != 0) return;
  g.gn_part = emit->buf;
  emit->st.part = emit->buf;
  emit->st.tiles_per_sample = rows_per_sample / rows;
}

void plan_ln_emit(GemmArgs& g, const GemmPlan& plan, LnEmit* ln) {
  if (ln) ln->tiles = 0;
  if (!ln || !ln->buf) return;
  const int tiles = plan.ln_tiles;
  if (tiles > 0 && tiles <= 5) { g.ln_part = ln->buf; g.ln_tiles = tiles; ln->tiles = tiles; }   // C = 1280 (8 tiles): the finish costs what the 8 us pass did
}

ConvDims conv_out_dims(int amode, int H, int W) {
  switch (amode) {
    case A_CONV_S1: return {H, W};
    case A_CONV_S2P1: case A_CONV_S2ASYM: return {H / 2, W / 2};
    case A_CONV_UP2: return {2 * H, 2 * W};
    default: throw SvgError("conv3x3: bad mode");
  }
}

bool conv3x3_fp8_ok(const ConvW& cw, int B, int H, int W, bool up2) {
  return cw.w8 != nullptr && conv_halo_fp8_supported(B, up2 ? 2 * H : H, up2 ? 2 * W : W, cw.Cin, cw.Opad);
}

GemmArgs conv3x3_fp8_args(const ConvW& cw, h16* out, int B, int H, int W, int amode, const ConvOpts& o) {
  SVG_CHECK((amode == A_CONV_S1 || amode == A_CONV_UP2) && !o.out_f32 && !o.residual_f32, "conv3x3_fp8: stride 1 (mode %d), 16-bit output and residual only", amode);
  SVG_CHECK(conv3x3_fp8_ok(cw, B, H, W, amode == A_CONV_UP2), "conv3x3_fp8: %d x %dx%d x %d -> %d does not qualify", B, H, W, cw.Cin, cw.Opad);
  const ConvDims d = conv_out_dims(amode, H, W);
  GemmArgs g;
  g.H = H; g.W = W; g.Cin = cw.Cin; g.amode = amode; g.Ho = d.Ho; g.Wo = d.Wo;
  g.K = 9 * cw.Cin; g.M = B * d.Ho * d.Wo; g.N = cw.Opad; g.n_valid = cw.Opad;
  g.bias = cw.b;
  g.bias_bn = o.bias_bn; g.bias_bn_ld = o.bias_bn_ld; g.rows_per_batch = d.Ho * d.Wo;
  g.residual = o.residual; g.ldr = cw.Opad;
  g.C = out; g.ldc = cw.Opad;
  return g;
}

void conv3x3_fp8(svg_ctx* ctx, const uint8_t* x8, const uint8_t* xs, const ConvW& cw, h16* out, int B, int H, int W, int amode, hipStream_t s,
                 const ConvOpts& o) {
  GemmArgs g = conv3x3_fp8_args(cw, out, B, H, W, amode, o);
  attach_gn_emit(g, o.emit, g.Ho * g.Wo, 256);   // one partial per 16 x 16 pixel block, like the fp16 halo conv
  conv_halo_fp8(ctx, x8, xs, cw.w8, cw.w8s, cw.Opad, g, s);
}

GemmArgs conv3x3_args(const h16* x, const ConvW& cw, int B, int H, int W, int amode, int out_f32) {
  GemmArgs g;
  g.A = x; g.H = H; g.W = W; g.Cin = cw.Cin;
  g.amode = (cw.Cin == 8) ? A_CONV_SMALLC : amode;
  SVG_CHECK(cw.Cin != 8 || amode == A_CONV_S1, "small-Cin conv supports stride 1 only");
  const ConvDims d = conv_out_dims(amode, H, W);
  g.Ho = d.Ho; g.Wo = d.Wo;
  g.Wt = cw.w; g.ldb = 9 * cw.Cin; g.K = 9 * cw.Cin;
  g.M = B * g.Ho * g.Wo; g.N = cw.Opad; g.n_valid = cw.Opad;
  g.bias = cw.b;
  g.out_f32 = out_f32;
  return g;
}

void conv3x3(svg_ctx* ctx, const h16* x, const ConvW& cw, void* out, int B, int H, int W, int amode, hipStream_t s, const ConvOpts& o) {
  SVG_CHECK(!o.residual_f32 || (o.out_f32 == 2 && !o.residual), "conv3x3: an f32 residual needs the f32-stream output and no 16-bit residual");
  // the kernels address an operand with 32-bit byte offsets: an input or output of 2^31 elements or more (the 512 x 512
  // VAE levels beyond ~30 images) is processed in batch chunks
  {
    const int up = amode == A_CONV_UP2 ? 4 : 1;
    const int64_t per_img = std::max<int64_t>((int64_t)H * W * std::max(cw.Cin, 8), (int64_t)H * W * up * cw.Opad);
    const int64_t lim = chunk_limit();
    if ((int64_t)B * per_img > lim && B > 1) {
      const int chunk = (int)std::max<int64_t>(1, lim / per_img);
      const ConvDims d = conv_out_dims(amode, H, W);
      ConvOpts c = o;               // per chunk: its slice of every operand; no statistics
      c.emit = nullptr;
      for (int b0 = 0; b0 < B; b0 += chunk) {
        const int64_t off = (int64_t)b0 * d.Ho * d.Wo * cw.Opad;
        if (o.bias_bn) c.bias_bn = o.bias_bn + (int64_t)b0 * (o.bias_bn_ld ? o.bias_bn_ld : cw.Opad);
        if (o.residual) c.residual = o.residual + off;
        if (o.residual_f32) c.residual_f32 = o.residual_f32 + off;
        conv3x3(ctx, x + (int64_t)b0 * H * W * cw.Cin, cw, o.out_f32 ? (void*)((float*)out + off) : (void*)((h16*)out + off), std::min(chunk, B - b0),
                H, W, amode, s, c);
      }
      return;
    }
  }
  GemmArgs g = conv3x3_args(x, cw, B, H, W, amode, o.out_f32);
  g.bias_bn = o.bias_bn; g.bias_bn_ld = o.bias_bn_ld; g.rows_per_batch = g.Ho * g.Wo;
  g.residual = o.residual; g.ldr = cw.Opad;
  g.C = out; g.ldc = cw.Opad;
  g.residual_f32 = o.residual_f32;
  const GemmPlan plan = gemm_plan(g);
  attach_gn_emit(g, o.emit, g.Ho * g.Wo, plan.gn_rows);
  gemm_auto(ctx, g, plan, s, PK_CONV3);
}

int conv3x3_halo_width(const ConvW& cw, int B, int H, int W, int amode, int out_f32) {
  const GemmPlan plan = gemm_plan(conv3x3_args(nullptr, cw, B, H, W, amode, out_f32));
  return plan.family == GF_HALO ? plan.bn : 0;
}

void linear(svg_ctx* ctx, const h16* A, int lda, const PackedLinear& pl, void* C, int ldc, int M, hipStream_t s, const LinearOpts& o) {
  if (o.ln) o.ln->tiles = 0;
  SVG_CHECK(!o.residual_f32 || (o.out_f32 == 2 && !o.residual), "linear: an f32 residual needs the f32-stream output and no 16-bit residual");
  SVG_CHECK((pl.ln_s != nullptr) == (o.ln_rs != nullptr), "linear: LayerNorm-folded weights need the row statistics (and only they)");
  {   // 32-bit operand offsets in the kernels: split very tall problems (1 x 1 convs on the 512 x 512 VAE levels) by rows
    const int64_t lim = chunk_limit();
    const int64_t per_row = std::max<int64_t>(lda, std::max(ldc, o.ldr));
    if ((int64_t)M * per_row > lim && M > 1) {
      SVG_CHECK(!o.A2, "linear: a two-source A operand is not split by rows");
      const int chunk = (int)(lim / per_row) & ~255;
      SVG_CHECK(chunk >= 256, "linear: a %lld-element operand limit is below one 256-row slab of %lld-wide rows", (long long)lim, (long long)per_row);
      const int csz = o.out_f32 ? 4 : 2;
      LinearOpts c = o;             // per chunk: its rows of every operand; no statistics
      c.emit = nullptr; c.rows_per_sample = 0; c.ln = nullptr;
      for (int m0 = 0; m0 < M; m0 += chunk) {
        if (o.residual) c.residual = o.residual + (int64_t)m0 * o.ldr;
        if (o.residual_f32) c.residual_f32 = o.residual_f32 + (int64_t)m0 * o.ldr;
        if (o.ln_rs) c.ln_rs = o.ln_rs + m0;
        if (o.ln_rm) c.ln_rm = o.ln_rm + m0;
        linear(ctx, A + (int64_t)m0 * lda, lda, pl, (char*)C + (int64_t)m0 * ldc * csz, ldc, std::min(chunk, M - m0), s, c);
      }
      return;
    }
  }
  if (pl.w8 && !o.A2 && !o.ln_rs && o.act != ACT_GEGLU && o.out_f32 != 2 && M >= 1024 && lda == pl.K && gemm_fp8_supported(M, pl.N, pl.K)) {
    // MX fp8: the activations are quantised per 32-element block on the way in (one extra pass over A), f32 accumulate
    ctx->arena.push();
    uint8_t* aq = ctx->arena.get<uint8_t>((int64_t)M * pl.K);
    uint8_t* as = ctx->arena.get<uint8_t>((int64_t)M * (pl.K / 32));
    quant_mx_h16(ctx, A, lda, aq, as, M, pl.K, s);
    GemmArgs g8;
    g8.M = M; g8.N = pl.N; g8.K = pl.K; g8.bias = pl.b; g8.act = o.act; g8.residual = o.residual; g8.ldr = o.ldr; g8.C = C; g8.ldc = ldc; g8.out_f32 = o.out_f32;
    gemm_fp8(ctx, aq, as, pl.w8, pl.w8s, g8, s);
    ctx->arena.pop();
    return;
  }
  GemmArgs g;
  g.ln_rs = o.ln_rs; g.ln_rm = o.ln_rm; g.ln_s = pl.ln_s;
  g.A = A; g.lda = lda; g.Wt = pl.w; g.ldb = pl.K; g.M = M; g.N = pl.N; g.K = pl.K; g.n_valid = pl.N;
  g.bias = pl.b; g.act = o.act; g.residual = o.residual; g.ldr = o.ldr; g.C = C; g.ldc = ldc; g.out_f32 = o.out_f32;
  g.A2 = o.A2; g.lda2 = o.lda2; g.k_split = o.k_split;
  g.residual_f32 = o.residual_f32;
  const GemmPlan plan = gemm_plan(g);
  attach_gn_emit(g, o.emit, o.rows_per_sample, plan.gn_rows);
  plan_ln_emit(g, plan, o.ln);
  gemm_auto(ctx, g, plan, s, PK_GEMM);
}

void vt_proj_into(svg_ctx* ctx, const PackedLinear& wv, const h16* src, int B, int rows, int rows_pad, int K, h16* vt, hipStream_t s,
                  const float* ln_rs, const float* ln_rm) {
  const int C = wv.N;
  GemmArgs g;
  g.A = wv.w; g.lda = K; g.Wt = src; g.ldb = K; g.M = C; g.N = rows_pad; g.n_valid = rows; g.K = K;
  g.batch = B; g.sA = 0; g.sB = (int64_t)rows * K; g.sC = (int64_t)C * rows_pad;
  g.C = vt; g.ldc = rows_pad;
  SVG_CHECK((wv.ln_s != nullptr) == (ln_rs != nullptr), "vt_proj: LayerNorm-folded weights need the token statistics");
  if (wv.b) { g.bias = wv.b; g.bias_row = 1; }   // the output rows are the projection's columns
  if (ln_rs) {   // the normalised tokens are the B operand here: statistics per column, sums per row
    g.ln_rs = ln_rs; g.ln_rm = ln_rm; g.ln_s = wv.ln_s; g.ln_swapped = 1; g.ln_zstride = rows;
  }
  gemm_auto(ctx, g, s, PK_GEMM);
}

// per-device kernel attributes (dynamic LDS limits) of every kernel instantiation of this namespace
void sd_init_device() {
  gemm_init_device();
  gemm_pp_init_device();
  gemm_ws_init_device();
  vae_attn_init_device();
  conv_halo_init_device();
  ff_fused_init_device();
  xattn_fused_init_device();
  gemm_fp8_init_device();
  conv_halo_fp8_init_device();
}

}  // namespace SDNS
