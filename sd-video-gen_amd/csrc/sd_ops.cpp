// C ABI, operator level: the kernels the SD graphs are made of, on caller buffers (used by the parity tests).  Compiled once per
// storage type: the bf16 build exports svg_op_<name>, the -DSVG_F16 build svg_op_<name>_f16 (16-bit buffers are IEEE half there).
#include "models.h"
#include "../../include/svg_hip.h"
#include <cstdlib>

#if SD_F16
#define SVG_OP(name) name##_f16
#else
#define SVG_OP(name) name
#endif

using namespace SDNS;

// The temporary ConvW of a conv hook: the caller's OIHW f32 weights (+ optional bias) staged in the arena and packed there, as 16-bit
// weights or (mx) as the MX fp8 copy alone.  Arena order: [w |] f32 staging | bias [| w8 | w8s]
static ConvW stage_conv(svg_ctx* ctx, const float* w_oihw, const float* bias, int Cin, int Cout, bool mx, hipStream_t s) {
  ConvW cw;
  cw.Cin = Cin; cw.Cout = Cout; cw.Opad = (int)align_up(Cout, 4);
  const int64_t nw = (int64_t)Cout * Cin * 9;
  if (!mx) cw.w = ctx->arena.get<h16>((int64_t)cw.Opad * 9 * Cin);
  float* wdev = ctx->arena.get<float>(nw);
  cw.b = ctx->arena.get<float>(cw.Opad);
  if (mx) {
    cw.Cp = (int)align_up(Cin, 128);
    cw.w8 = ctx->arena.get<uint8_t>((int64_t)cw.Opad * 9 * cw.Cp);
    cw.w8s = ctx->arena.get<uint8_t>((int64_t)9 * (cw.Cp / 128) * cw.Opad * 4);
  }
  if (SVG_LAUNCHING(ctx)) {
    HIP_OK(hipMemcpyAsync(wdev, w_oihw, (size_t)nw * sizeof(float), hipMemcpyDefault, s));
    HIP_OK(hipMemsetAsync(cw.b, 0, cw.Opad * sizeof(float), s));
    if (bias) HIP_OK(hipMemcpyAsync(cw.b, bias, Cout * sizeof(float), hipMemcpyDefault, s));
    if (mx) pack_conv3x3_mx(wdev, cw.w8, cw.w8s, Cout, Cin, cw.Opad, cw.Cp, s);
    else pack_conv3x3(wdev, cw.w, Cout, Cin, cw.Opad, Cin, s);
  }
  return cw;
}

extern "C" {

int SVG_OP(svg_op_gemm)(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C,
                int M, int N, int K, int act, int out_f32, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    run_planned(ctx, [&]() {
      GemmArgs g;
      g.A = (const h16*)A; g.lda = K; g.Wt = (const h16*)W; g.ldb = K; g.M = M; g.N = N; g.K = K; g.n_valid = N;
      g.bias = bias; g.residual = (const h16*)residual; g.act = act; g.out_f32 = out_f32;
      g.C = C;
      if (act == ACT_GEGLU) {
        // caller passes W rows as [h(0..F-1); gate(0..F-1)], F = N/2: pack here (test hook)
        const int F = N / 2;
        h16* wp = ctx->arena.get<h16>((int64_t)N * K);
        float* bp = ctx->arena.get<float>(N);
        float* wf = ctx->arena.get<float>((int64_t)N * K);
        if (SVG_LAUNCHING(ctx)) {
          h16_to_f32((const h16*)W, wf, (int64_t)N * K, s);
          pack_geglu(wf, bias, wp, bp, F, K, s);
        }
        g.Wt = wp; g.bias = bias ? bp : nullptr; g.ldc = F; g.ldr = F;
      } else {
        g.ldc = N; g.ldr = N;
      }
      gemm_auto(ctx, g, s, PK_GEMM);
    });
  });
}

int SVG_OP(svg_op_conv3x3)(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, uint16_t* out, int B, int H, int W,
                   int Cin, int Cout, int mode, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    run_planned(ctx, [&]() {
      SVG_CHECK(mode >= 0 && mode <= 3, "conv3x3: bad mode");
      const int amodes[4] = {A_CONV_S1, A_CONV_S2P1, A_CONV_S2ASYM, A_CONV_UP2};
      const ConvW cw = stage_conv(ctx, w_oihw, bias, Cin, Cout, false, s);
      GemmArgs g = conv3x3_args((const h16*)x, cw, B, H, W, amodes[mode], 0);
      g.C = out; g.ldc = Cout;
      SVG_CHECK(Cout % 4 == 0, "conv3x3 op: Cout must be a multiple of 4");
      gemm_auto(ctx, g, s, PK_CONV3);
    });
  });
}

// conv3x3 (stride 1, pad 1) in MX fp8 (conv_halo_fp8.hip): x (B,H,W,Cin) h16 and the f32 OIHW weights are quantised on the device
// (e4m3 + E8M0 per 32 channels), the conv runs on v_mfma_scale_f32_16x16x128_f8f6f4; out h16 (B,H,W,Cout) = conv + bias (+ residual).
// q_out / s_out (optional): the quantised activations ((B*H*W, Cp) bytes, Cp = Cin rounded up to 128) and their scales, for the tests.
// mode 3: nearest-2x upsample fused in front (out is (B,2H,2W,Cout)), as svg_op_conv3x3.
int SVG_OP(svg_op_conv3x3_mx)(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual, uint16_t* out,
                      uint8_t* q_out, uint8_t* s_out, int B, int H, int W, int Cin, int Cout, int mode, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(Cout % 4 == 0 && Cin % 64 == 0, "conv3x3_mx op: Cout %% 4 and Cin %% 64 must be 0");
    SVG_CHECK(mode == 0 || mode == 3, "conv3x3_mx op: mode 0 (stride 1) or 3 (nearest-2x upsample in front)");
    const bool up2 = mode == 3;
    run_planned(ctx, [&]() {
      const ConvW cw = stage_conv(ctx, w_oihw, bias, Cin, Cout, true, s);
      const int64_t P = (int64_t)B * H * W;
      uint8_t* q = ctx->arena.get<uint8_t>(P * cw.Cp);
      uint8_t* qs = ctx->arena.get<uint8_t>(P * (cw.Cp / 32));
      quant_act_mx(ctx, (const h16*)x, Cin, q, qs, P, s);
      ConvOpts o; o.residual = (const h16*)residual;
      conv3x3_fp8(ctx, q, qs, cw, (h16*)out, B, H, W, up2 ? A_CONV_UP2 : A_CONV_S1, s, o);
      if (SVG_LAUNCHING(ctx)) {
        if (q_out) HIP_OK(hipMemcpyAsync(q_out, q, (size_t)P * cw.Cp, hipMemcpyDeviceToDevice, s));
        if (s_out) HIP_OK(hipMemcpyAsync(s_out, qs, (size_t)P * (cw.Cp / 32), hipMemcpyDeviceToDevice, s));
      }
    });
  });
}

// the same conv on a descriptor (svg_hip.h: svg_conv_mx_desc) with everything conv3x3_fp8 takes — the per-sample bias rows and the
// GroupNorm column sums included — and the packed weights read back; path = {column tile, tn_major, workgroups} as conv_halo_fp8
// launched it.  Test hook.
int SVG_OP(svg_op_conv3x3_mx_ex)(svg_ctx* ctx, const svg_conv_mx_desc* d, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(d != nullptr, "conv3x3_mx_ex: no descriptor");
    SVG_CHECK(d->x && d->w_oihw && d->out, "conv3x3_mx_ex: x, w_oihw and out are required");
    SVG_CHECK(d->Cout > 0 && d->Cin > 0 && d->Cin % 64 == 0, "conv3x3_mx_ex: Cin %% 64 must be 0");
    SVG_CHECK(d->mode == 0 || d->mode == 3, "conv3x3_mx_ex: mode 0 (stride 1) or 3 (nearest-2x upsample in front)");
    const int amode = d->mode == 3 ? A_CONV_UP2 : A_CONV_S1;
    const ConvDims od = conv_out_dims(amode, d->H, d->W);
    SVG_CHECK(conv_halo_fp8_supported(d->B, od.Ho, od.Wo, d->Cin, (int)align_up(d->Cout, 4)), "conv3x3_mx_ex: %d x %dx%d x %d -> %d is not a shape of conv_halo_fp8",
              d->B, od.Ho, od.Wo, d->Cin, d->Cout);
    Fp8ConvPath p;
    run_planned(ctx, [&]() {
      const ConvW cw = stage_conv(ctx, d->w_oihw, d->bias, d->Cin, d->Cout, true, s);
      const int64_t P = (int64_t)d->B * d->H * d->W;
      uint8_t* q = ctx->arena.get<uint8_t>(P * cw.Cp);
      uint8_t* qs = ctx->arena.get<uint8_t>(P * (cw.Cp / 32));
      quant_act_mx(ctx, (const h16*)d->x, d->Cin, q, qs, P, s);
      ConvOpts o; o.bias_bn = d->bias_bn; o.bias_bn_ld = d->bias_bn_ld; o.residual = (const h16*)d->residual;
      GemmArgs g = conv3x3_fp8_args(cw, (h16*)d->out, d->B, d->H, d->W, amode, o);
      g.gn_part = d->gn_part;
      conv_halo_fp8(ctx, q, qs, cw.w8, cw.w8s, cw.Opad, g, s, &p);
      if (SVG_LAUNCHING(ctx)) {
        if (d->q_out) HIP_OK(hipMemcpyAsync(d->q_out, q, (size_t)P * cw.Cp, hipMemcpyDeviceToDevice, s));
        if (d->s_out) HIP_OK(hipMemcpyAsync(d->s_out, qs, (size_t)P * (cw.Cp / 32), hipMemcpyDeviceToDevice, s));
        if (d->w8_out) HIP_OK(hipMemcpyAsync(d->w8_out, cw.w8, (size_t)cw.Opad * 9 * cw.Cp, hipMemcpyDeviceToDevice, s));
        if (d->w8s_out) HIP_OK(hipMemcpyAsync(d->w8s_out, cw.w8s, (size_t)9 * (cw.Cp / 128) * cw.Opad * 4, hipMemcpyDeviceToDevice, s));
      }
    });
    if (path) { path[0] = p.bn; path[1] = p.tn_major; path[2] = p.workgroups; }
  });
}

// conv3x3 (stride 1) whose epilogue leaves the GroupNorm column sums, followed by the GroupNorm that consumes them
int SVG_OP(svg_op_conv3x3_gn)(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const float* gamma, const float* beta,
                      uint16_t* conv_out, uint16_t* gn_out, int B, int H, int W, int Cin, int Cout, int groups, float eps, int silu,
                      int* used_epilogue_stats, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(Cout % 4 == 0 && Cin % 64 == 0, "conv3x3_gn op: Cout %% 4 and Cin %% 64 must be 0");
    int used = 0;
    run_planned(ctx, [&]() {
      const ConvW cw = stage_conv(ctx, w_oihw, bias, Cin, Cout, false, s);
      float* gdev = ctx->arena.get<float>(Cout);
      float* bdev = ctx->arena.get<float>(Cout);
      if (SVG_LAUNCHING(ctx)) {
        HIP_OK(hipMemcpyAsync(gdev, gamma, Cout * sizeof(float), hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(bdev, beta, Cout * sizeof(float), hipMemcpyDefault, s));
      }
      GnEmit e;
      e.buf = ctx->arena.get<float>(gn_part_floats(B, (int64_t)H * W, Cout));
      ConvOpts o; o.emit = &e;
      conv3x3(ctx, (const h16*)x, cw, conv_out, B, H, W, A_CONV_S1, s, o);
      used = e.st.valid() ? 1 : 0;
      groupnorm(ctx, (const h16*)conv_out, Cout, nullptr, 0, gdev, bdev, (h16*)gn_out, B, H * W, groups, eps, silu, s, &e.st, nullptr);
    });
    if (used_epilogue_stats) *used_epilogue_stats = used;
  });
}

// conv3x3 of the VAE's f32 residual stream: f32 output (+ 16-bit or f32 residual), optionally followed by the GroupNorm on it
int SVG_OP(svg_op_conv3x3_f32s)(svg_ctx* ctx, const uint16_t* x, const float* w_oihw, const float* bias, const uint16_t* residual,
                                const float* residual_f32, float* out, const float* gamma, const float* beta, uint16_t* gn_out, int B, int H, int W,
                                int Cin, int Cout, int mode, int groups, float eps, int silu, int* halo_width, int* used_epilogue_stats,
                                void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(Cout % 4 == 0 && (Cin % 64 == 0 || (Cin == 8 && mode == 0)), "conv3x3_f32s op: Cout %% 4 and Cin %% 64 (or Cin 8, mode 0) must be 0");
    SVG_CHECK(mode == 0 || mode == 2 || mode == 3, "conv3x3_f32s op: mode 0 (stride 1), 2 (stride 2, pad (0,1,0,1)) or 3 (nearest-2x upsample)");
    SVG_CHECK(!(residual && residual_f32), "conv3x3_f32s op: one residual");
    SVG_CHECK(!gn_out || (gamma && beta), "conv3x3_f32s op: the GroupNorm needs gamma and beta");
    const int amode = mode == 0 ? A_CONV_S1 : (mode == 2 ? A_CONV_S2ASYM : A_CONV_UP2);
    const ConvDims d = conv_out_dims(amode, H, W);
    int used = 0, hw = 0;
    run_planned(ctx, [&]() {
      const ConvW cw = stage_conv(ctx, w_oihw, bias, Cin, Cout, false, s);
      hw = conv3x3_halo_width(cw, B, H, W, amode, 2);
      GnEmit e;
      e.buf = ctx->arena.get<float>(gn_part_floats(B, (int64_t)d.Ho * d.Wo, Cout));
      ConvOpts o; o.residual = (const h16*)residual; o.residual_f32 = residual_f32; o.out_f32 = 2; o.emit = gn_out ? &e : nullptr;
      conv3x3(ctx, (const h16*)x, cw, out, B, H, W, amode, s, o);
      used = e.st.valid() ? 1 : 0;
      if (gn_out) groupnorm_f32(ctx, out, Cout, gamma, beta, (h16*)gn_out, B, d.Ho * d.Wo, groups, eps, silu, s, &e.st);
    });
    if (halo_width) *halo_width = hw;
    if (used_epilogue_stats) *used_epilogue_stats = used;
  });
}

// GroupNorm (+SiLU) on an f32 NHWC input (the VAE's f32 residual stream), 16-bit output; statistics pass or single-launch small-HW path
int SVG_OP(svg_op_groupnorm_f32)(svg_ctx* ctx, const float* x, const float* gamma, const float* beta, uint16_t* out, int B, int HW, int C,
                                 int groups, float eps, int silu, void* stream) {
  return svg_guard(ctx, [&] {
    run_planned(ctx, [&]() { groupnorm_f32(ctx, x, C, gamma, beta, (h16*)out, B, HW, groups, eps, silu, (hipStream_t)stream); });
  });
}

// svg_gemm_desc -> GemmArgs, field by field (svg_hip.h)
static GemmArgs gemm_desc_args(const svg_gemm_desc* d) {
  GemmArgs g;
  g.amode = d->amode; g.H = d->H; g.W = d->W; g.Cin = d->Cin; g.Ho = d->Ho; g.Wo = d->Wo;
  g.A = (const h16*)d->A; g.lda = d->lda; g.Wt = (const h16*)d->Wt; g.ldb = d->ldb; g.n_valid = d->n_valid;
  g.C = d->C; g.ldc = d->ldc; g.M = d->M; g.N = d->N; g.K = d->K; g.batch = d->batch; g.sA = d->sA; g.sB = d->sB; g.sC = d->sC;
  g.alpha = d->alpha; g.bias = d->bias; g.bias_row = d->bias_row; g.bias_zs = d->bias_zs;
  g.bias_bn = d->bias_bn; g.rows_per_batch = d->rows_per_batch; g.bias_bn_ld = d->bias_bn_ld;
  g.residual = (const h16*)d->residual; g.ldr = d->ldr; g.act = d->act; g.out_f32 = d->out_f32;
  g.ln_rs = d->ln_rs; g.ln_rm = d->ln_rm; g.ln_s = d->ln_s; g.ln_swapped = d->ln_swapped; g.ln_zstride = d->ln_zstride;
  g.vt_out = (h16*)d->vt_out; g.vt_n0 = d->vt_n0; g.vt_rows = d->vt_rows; g.vt_ld = d->vt_ld; g.vt_bs = d->vt_bs;
  g.A2 = (const h16*)d->A2; g.lda2 = d->lda2; g.k_split = d->k_split;
  g.gn_part = d->gn_part; g.ln_part = d->ln_part; g.ln_tiles = d->ln_tiles;
  return g;
}

// the whole GEMM epilogue contract on caller buffers (svg_hip.h: svg_gemm_desc): the descriptor goes into GemmArgs field by field and
// through gemm_auto as the models call it; path = {family, column tile, split-K} of the plan that was launched.  Test hook.
int SVG_OP(svg_op_gemm_ex)(svg_ctx* ctx, const svg_gemm_desc* d, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(d != nullptr, "gemm_ex: no descriptor");
    GemmPlan p;
    run_planned(ctx, [&]() {
      const GemmArgs g = gemm_desc_args(d);
      p = gemm_plan(g);
      gemm_auto(ctx, g, p, (hipStream_t)stream, g.amode == A_DENSE ? PK_GEMM : PK_CONV3);
    });
    if (path) { path[0] = p.family; path[1] = p.bn; path[2] = p.splitk; }
  });
}

// gemm_plan() of the descriptor: {family, column tile, split-K, gn_rows, ln_tiles}; nothing is launched.  Test hook.
int SVG_OP(svg_op_gemm_plan)(svg_ctx* ctx, const svg_gemm_desc* d, int* plan) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(d != nullptr && plan != nullptr, "gemm_plan: no descriptor / no result array");
    const GemmPlan p = gemm_plan(gemm_desc_args(d));
    plan[0] = p.family; plan[1] = p.bn; plan[2] = p.splitk; plan[3] = p.gn_rows; plan[4] = p.ln_tiles;
  });
}

// C[M,N] = [A | A2][M, K] * W[N,K]^T + bias: dense GEMM whose A operand is the channel concat of two tensors (A: k_split columns)
int SVG_OP(svg_op_gemm_cat)(svg_ctx* ctx, const uint16_t* A, const uint16_t* A2, const uint16_t* W, const float* bias, uint16_t* C, int M, int N,
                    int K, int k_split, void* stream) {
  return svg_guard(ctx, [&] {
    run_planned(ctx, [&]() {
      GemmArgs g;
      g.A = (const h16*)A; g.lda = k_split; g.A2 = (const h16*)A2; g.lda2 = K - k_split; g.k_split = k_split;
      g.Wt = (const h16*)W; g.ldb = K; g.M = M; g.N = N; g.K = K; g.n_valid = N; g.bias = bias; g.C = C; g.ldc = N;
      gemm_auto(ctx, g, (hipStream_t)stream, PK_GEMM);
    });
  });
}

// C = A W^T + bias + residual (h16) with the LayerNorm row statistics of C taken from the epilogue's row partials (GemmArgs::ln_part
// + ln_finish): rs[m] = rstd, rm[m] = rstd * mean over the N columns; *used = column tiles that emitted (0: the launch could not, rs / rm
// then come from the ln_stats pass).  Test hook.
int SVG_OP(svg_op_gemm_lnstats)(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, uint16_t* C, int M,
                        int N, int K, int batch, float* rs, float* rm, int* used, void* stream) {
  return svg_guard(ctx, [&] {
    int tiles = 0;
    run_planned(ctx, [&]() {
      GemmArgs g;
      g.A = (const h16*)A; g.lda = K; g.Wt = (const h16*)W; g.ldb = K; g.M = M; g.N = N; g.K = K; g.n_valid = N; g.bias = bias;
      g.residual = (const h16*)residual; g.ldr = N; g.C = C; g.ldc = N;
      if (batch > 1) { g.batch = batch; g.sA = (int64_t)M * K; g.sB = 0; g.sC = (int64_t)M * N; }
      float* part = ctx->arena.get<float>((int64_t)batch * M * 16);
      const GemmPlan plan = gemm_plan(g);
      tiles = plan.ln_tiles <= 8 ? plan.ln_tiles : 0;
      if (tiles > 0) { g.ln_part = part; g.ln_tiles = tiles; }
      gemm_auto(ctx, g, plan, (hipStream_t)stream, PK_GEMM);
      if (tiles > 0) ln_finish(ctx, part, tiles, rs, rm, batch * M, N, 1e-5f, (hipStream_t)stream);
      else ln_stats(ctx, (const h16*)C, rs, rm, batch * M, N, 1e-5f, (hipStream_t)stream);
    });
    if (used) *used = tiles;
  });
}

// fused GEGLU feed-forward of a transformer block at C = 320: out = ff2(GEGLU(ff1(LayerNorm(x)))) + residual.  Weights in the
// state_dict layout (W1 [2*4C][C] = [h; gate], W2 [C][4C]); folding, packing and the row statistics happen here (test hook).
int SVG_OP(svg_op_ff_fused)(svg_ctx* ctx, const uint16_t* x, const float* ln_gamma, const float* ln_beta, const float* w1, const float* b1,
                    const float* w2, const float* b2, const uint16_t* residual, uint16_t* out, int M, int C, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(ff_fused_supported(C, 1 << 30), "ff_fused op: C = %d is not supported (320)", C);
    run_planned(ctx, [&]() {
      const int F = 4 * C;
      float* w1d = ctx->arena.get<float>((int64_t)2 * F * C);
      float* b1d = ctx->arena.get<float>(2 * F);
      float* b1f = ctx->arena.get<float>(2 * F);
      float* gd = ctx->arena.get<float>(C);
      float* bd = ctx->arena.get<float>(C);
      float* w2d = ctx->arena.get<float>((int64_t)C * F);
      float* b2d = ctx->arena.get<float>(C);
      h16* w1p = ctx->arena.get<h16>((int64_t)2 * F * C);
      float* b1p = ctx->arena.get<float>(2 * F);
      float* s1 = ctx->arena.get<float>(2 * F);
      h16* w2p = ctx->arena.get<h16>((int64_t)C * F);
      if (SVG_LAUNCHING(ctx)) {
        HIP_OK(hipMemcpyAsync(w1d, w1, (size_t)2 * F * C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(b1d, b1, (size_t)2 * F * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(gd, ln_gamma, (size_t)C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(bd, ln_beta, (size_t)C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(w2d, w2, (size_t)C * F * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(b2d, b2, (size_t)C * 4, hipMemcpyDefault, s));
        fold_ln_weights(w1d, b1d, gd, bd, b1f, 2 * F, C, s);
        pack_geglu(w1d, b1f, w1p, b1p, F, C, s);
        rowsum_h16(w1p, s1, 2 * F, C, s);
        pack_ff2_perm(w2d, w2p, C, F, s);
      }
      // the kernel derives the LayerNorm statistics from the rows it holds (the UNet's path)
      ff_fused(ctx, (const h16*)x, C, w1p, b1p, s1, w2p, b2d, (const h16*)residual, C, (h16*)out, C, M, s);
    });
  });
}

// one-launch cross-attention of a C = 320 block (xattn_fused.hip).  x (M,320): the block input (pre-LayerNorm rows, also the residual) — or,
// chained form (a != null): x is not given, the kernel starts from a (M,320) = the self-attention's output, r its residual and wp (320,320) /
// bp its output projection.  k (N,L,320) and vt (N,320,Lp) are the projected context of every sample (rows_per_sample rows each); weights
// f32 in the state_dict layout; folding, padding and packing happen here (test hook).
int SVG_OP(svg_op_xattn_fused)(svg_ctx* ctx, const uint16_t* x, const uint16_t* a, const uint16_t* r, const float* wp, const float* bp,
                               const float* ln_gamma, const float* ln_beta, const float* wq, const uint16_t* k, const uint16_t* vt, int Lp,
                               const float* wo, const float* bo, uint16_t* out, int M, int rows_per_sample, int L, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    constexpr int C = 320;
    SVG_CHECK(xattn_fused_supported(C, 8, std::max(M, 128 * 192), rows_per_sample, L) && M % rows_per_sample == 0,
              "xattn_fused op: needs 8 heads of 40, L <= 80, samples of a multiple of 128 rows (M %d, rows per sample %d, L %d)", M, rows_per_sample, L);
    SVG_CHECK((x != nullptr) != (a != nullptr), "xattn_fused op: give either x (plain form) or a, r, wp, bp (chained form)");
    const int N = M / rows_per_sample;
    run_planned(ctx, [&]() {
      float* wqd = ctx->arena.get<float>((int64_t)C * C);
      float* wod = ctx->arena.get<float>((int64_t)C * C);
      float* wpd = ctx->arena.get<float>((int64_t)C * C);
      float* gd = ctx->arena.get<float>(C);
      float* bd = ctx->arena.get<float>(C);
      float* bod = ctx->arena.get<float>(C);
      float* bpd = ctx->arena.get<float>(C);
      h16* Wq = ctx->arena.get<h16>((int64_t)384 * C);
      float* sq = ctx->arena.get<float>(384);
      float* bq = ctx->arena.get<float>(384);
      h16* Wo = ctx->arena.get<h16>((int64_t)C * 384);
      h16* Wp = ctx->arena.get<h16>((int64_t)C * C);
      h16* kp = ctx->arena.get<h16>(xattn_kv_pack_elems(N));
      h16* vp = ctx->arena.get<h16>(xattn_kv_pack_elems(N));
      if (SVG_LAUNCHING(ctx)) {
        HIP_OK(hipMemcpyAsync(wqd, wq, (size_t)C * C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(wod, wo, (size_t)C * C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(gd, ln_gamma, (size_t)C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(bd, ln_beta, (size_t)C * 4, hipMemcpyDefault, s));
        HIP_OK(hipMemcpyAsync(bod, bo, (size_t)C * 4, hipMemcpyDefault, s));
        xattn_pack_q(wqd, gd, bd, Wq, sq, bq, a ? 1 : 0, s);
        xattn_pack_o(wod, Wo, s);
        xattn_pack_kv((const h16*)k, C, (int64_t)L * C, (const h16*)vt, Lp, (int64_t)C * Lp, kp, vp, N, L, s);
        if (a) {
          HIP_OK(hipMemcpyAsync(wpd, wp, (size_t)C * C * 4, hipMemcpyDefault, s));
          HIP_OK(hipMemcpyAsync(bpd, bp, (size_t)C * 4, hipMemcpyDefault, s));
          pack_linear(wpd, Wp, C, C, C, s);
        }
      }
      if (a) xattn_fused(ctx, (const h16*)a, C, (const h16*)r, C, Wp, bpd, nullptr, nullptr, Wq, sq, bq, kp, vp, Wo, bod, (h16*)out, C, M, rows_per_sample, L, s);
      else xattn_fused(ctx, (const h16*)x, C, nullptr, 0, nullptr, nullptr, nullptr, nullptr, Wq, sq, bq, kp, vp, Wo, bod, (h16*)out, C, M, rows_per_sample, L, s);
    });
  });
}

// MX fp8 quantiser: x (rows,K) bf16 -> q (rows,K) e4m3 bytes + scales (rows,K/32) E8M0 bytes
int SVG_OP(svg_op_quant_mx)(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t rows, int K, void* stream) {
  return svg_guard(ctx, [&] {
    quant_mx_h16(ctx, (const h16*)x, K, q, scales, rows, K, (hipStream_t)stream);
  });
}

// the conv path's activation quantiser on caller buffers: x (P,C) 16-bit -> q (P,Cp) e4m3 bytes + scales (P,Cp/32), Cp = C rounded up to 128.  Test hook.
int SVG_OP(svg_op_quant_act_mx)(svg_ctx* ctx, const uint16_t* x, uint8_t* q, uint8_t* scales, int64_t P, int C, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && q && scales && P > 0 && C > 0 && C % 32 == 0, "quant_act_mx op: P %lld C %d unsupported (C %% 32 must be 0)", (long long)P, C);
    quant_act_mx(ctx, (const h16*)x, C, q, scales, P, (hipStream_t)stream);
  });
}

// C = act(Q(A) Q(W)^T + bias + residual) with both operands quantised to MX fp8 on the fly (test hook / benchmark of the fp8 GEMM)
int SVG_OP(svg_op_gemm_fp8)(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C, int M, int N,
                    int K, int act, int out_f32, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    run_planned(ctx, [&]() {
      uint8_t* aq = ctx->arena.get<uint8_t>((int64_t)M * K);
      uint8_t* as = ctx->arena.get<uint8_t>((int64_t)M * (K / 32));
      uint8_t* wq = ctx->arena.get<uint8_t>((int64_t)N * K);
      uint8_t* wsc = ctx->arena.get<uint8_t>((int64_t)N * (K / 32));
      quant_mx_h16(ctx, (const h16*)A, K, aq, as, M, K, s);
      quant_mx_h16(ctx, (const h16*)W, K, wq, wsc, N, K, s);
      GemmArgs g;
      g.M = M; g.N = N; g.K = K; g.bias = bias; g.residual = (const h16*)residual; g.ldr = N; g.act = act; g.out_f32 = out_f32; g.C = C; g.ldc = N;
      gemm_fp8(ctx, aq, as, wq, wsc, g, s);
    });
  });
}

// the same with the output and residual row strides linear() passes (ldc >= N, ldr >= N); path[0] = the column tile gemm_fp8 launched.  Test hook.
int SVG_OP(svg_op_gemm_fp8_ex)(svg_ctx* ctx, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* residual, void* C, int M, int N,
                       int K, int act, int out_f32, int ldc, int ldr, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(A && W && C && M > 0 && N > 0 && K > 0 && ldc >= N && (!residual || ldr >= N) && ldc % 4 == 0 && ldr % 4 == 0,
              "gemm_fp8_ex: M %d N %d K %d ldc %d ldr %d unsupported", M, N, K, ldc, ldr);
    int bn = -1;
    run_planned(ctx, [&]() {
      uint8_t* aq = ctx->arena.get<uint8_t>((int64_t)M * K);
      uint8_t* as = ctx->arena.get<uint8_t>((int64_t)M * (K / 32));
      uint8_t* wq = ctx->arena.get<uint8_t>((int64_t)N * K);
      uint8_t* wsc = ctx->arena.get<uint8_t>((int64_t)N * (K / 32));
      quant_mx_h16(ctx, (const h16*)A, K, aq, as, M, K, s);
      quant_mx_h16(ctx, (const h16*)W, K, wq, wsc, N, K, s);
      GemmArgs g;
      g.M = M; g.N = N; g.K = K; g.bias = bias; g.residual = (const h16*)residual; g.ldr = ldr; g.act = act; g.out_f32 = out_f32; g.C = C; g.ldc = ldc;
      gemm_fp8(ctx, aq, as, wq, wsc, g, s, &bn);
    });
    if (path) path[0] = bn;
  });
}

int SVG_OP(svg_op_groupnorm)(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta, uint16_t* out, int B, int HW, int C,
                     int groups, float eps, int silu, void* stream) {
  return svg_guard(ctx, [&] {
    run_planned(ctx, [&]() {
      groupnorm(ctx, (const h16*)x, C, nullptr, 0, gamma, beta, (h16*)out, B, HW, groups, eps, silu, (hipStream_t)stream);
    });
  });
}

// GroupNorm on a full descriptor (svg_hip.h: svg_gn_desc): two sources, f32 input, caller-supplied producer column sums and a forced
// kernel path; path = {kind, maxch, vw, CV, PL, nchunk, nblk, threads} of what ran.  Test hook.
static void gn_desc_stats(const svg_gn_desc* d, GnStats& s1, GnStats& s2) {
  s1.part = d->part1; s1.tiles_per_sample = d->tps1;
  s2.part = d->part2; s2.tiles_per_sample = d->tps2;
}
static void gn_path_out(const GnPath& p, int* path) {
  if (!path) return;
  path[0] = p.kind; path[1] = p.maxch; path[2] = p.vw; path[3] = p.CV; path[4] = p.PL; path[5] = p.nchunk; path[6] = p.nblk; path[7] = p.threads;
}
int SVG_OP(svg_op_groupnorm_ex)(svg_ctx* ctx, const svg_gn_desc* d, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(d != nullptr, "groupnorm_ex: no descriptor");
    SVG_CHECK(d->x && d->gamma && d->beta && d->out && (d->C2 == 0 || d->x2), "groupnorm_ex: x, gamma, beta, out (and x2 when C2 > 0) are required");
    GnStats s1, s2;
    gn_desc_stats(d, s1, s2);
    GnPath f, p;
    f.kind = d->kind; f.maxch = d->maxch; f.vw = d->vw;
    run_planned(ctx, [&]() {
      groupnorm_ex(ctx, d->x, d->C1, d->x2, d->C2, d->f32_in != 0, d->gamma, d->beta, (h16*)d->out, d->B, d->HW, d->groups, d->eps, d->silu,
                   (hipStream_t)stream, &s1, &s2, d->force ? &f : nullptr, &p);
    });
    gn_path_out(p, path);
  });
}

// GroupNorm with MX fp8 output on the same descriptor (16-bit input, the statistics from part1 / part2): q (B*HW, Cp) e4m3 bytes, sc
// (B*HW, Cp/32) E8M0 bytes, stats (B, groups, 2) the (mean, rstd) table it used; *fused = 0 when groupnorm_mx declines (nothing is written).
int SVG_OP(svg_op_groupnorm_mx)(svg_ctx* ctx, const svg_gn_desc* d, int* fused, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(d != nullptr, "groupnorm_mx: no descriptor");
    SVG_CHECK(!d->f32_in && !d->force, "groupnorm_mx: 16-bit input, no forced path");
    SVG_CHECK(d->x && d->gamma && d->beta && d->q && d->sc && d->stats && (d->C2 == 0 || d->x2), "groupnorm_mx: x, gamma, beta, q, sc, stats (and x2 when C2 > 0) are required");
    GnStats s1, s2;
    gn_desc_stats(d, s1, s2);
    GnPath p;
    bool ok = false;
    run_planned(ctx, [&]() {
      ok = groupnorm_mx(ctx, (const h16*)d->x, d->C1, (const h16*)d->x2, d->C2, d->gamma, d->beta, d->q, d->sc, d->B, d->HW, d->groups, d->eps,
                        d->silu, (hipStream_t)stream, &s1, &s2, d->stats, &p);
    });
    if (fused) *fused = ok ? 1 : 0;
    gn_path_out(p, path);
  });
}

// gn_fold_weights on caller buffers (device): Wb (B,N,C) 16-bit, bb (B,N).  Test hook.
int SVG_OP(svg_op_gn_fold_weights)(svg_ctx* ctx, const float* W, const float* bias, const float* gamma, const float* beta, const float* stats,
                                   uint16_t* Wb, float* bb, int B, int N, int C, int groups, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(groups > 0 && C % groups == 0 && B > 0 && N > 0, "gn_fold_weights: C=%d groups=%d unsupported", C, groups);
    gn_fold_weights(W, bias, gamma, beta, stats, (h16*)Wb, bb, B, N, C, groups, (hipStream_t)stream);
  });
}

// ln_stats, softmax_rows and rowsum_h16 on caller buffers.  Test hooks.
int SVG_OP(svg_op_ln_stats)(svg_ctx* ctx, const uint16_t* x, float* rs, float* rm, int M, int C, float eps, void* stream) {
  return svg_guard(ctx, [&] {
    ln_stats(ctx, (const h16*)x, rs, rm, M, C, eps, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_softmax_rows)(svg_ctx* ctx, const float* s_in, uint16_t* p_out, int64_t rows, int cols, int ld_in, int ld_out, float scale,
                                void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(rows > 0 && cols > 0 && ld_in >= cols && ld_out >= cols, "softmax_rows: rows=%lld cols=%d ld_in=%d ld_out=%d unsupported", (long long)rows,
              cols, ld_in, ld_out);
    softmax_rows(ctx, s_in, (h16*)p_out, rows, cols, ld_in, ld_out, scale, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_rowsum)(svg_ctx* ctx, const uint16_t* w, float* out, int N, int K, void* stream) {
  return svg_guard(ctx, [&] {
    rowsum_h16((const h16*)w, out, N, K, (hipStream_t)stream);
  });
}

#if !SD_F16
// the f32-only kernels of norm.hip on caller buffers (one export: no 16-bit storage is involved).  Test hooks.
int svg_op_gn_finish(svg_ctx* ctx, const float* part1, int C1, int tps1, const float* part2, int C2, int tps2, float* stats, int B, int HW,
                     int groups, float eps, void* stream) {
  return svg_guard(ctx, [&] {
    const int C = C1 + C2;
    SVG_CHECK(groups > 0 && C % groups == 0 && part1 && tps1 > 0 && (C2 == 0 || (part2 && tps2 > 0)), "gn_finish: C=%d groups=%d or partials unsupported", C, groups);
    GnStats s1, s2;
    s1.part = part1; s1.tiles_per_sample = tps1; s2.part = part2; s2.tiles_per_sample = tps2;
    gn_finish(ctx, s1, C1, C2 ? &s2 : nullptr, C2, stats, B, HW, groups, eps, (hipStream_t)stream);
  });
}
int svg_op_ln_finish(svg_ctx* ctx, const float* part, int tiles, float* rs, float* rm, int M, int C, float eps, void* stream) {
  return svg_guard(ctx, [&] {
    ln_finish(ctx, part, tiles, rs, rm, M, C, eps, (hipStream_t)stream);
  });
}
int svg_op_fold_ln(svg_ctx* ctx, float* w, const float* bias_in, const float* gamma, const float* beta, float* bias_out, int N, int K, void* stream) {
  return svg_guard(ctx, [&] {
    fold_ln_weights(w, bias_in, gamma, beta, bias_out, N, K, (hipStream_t)stream);
  });
}
// the f32 / u8 kernels of eltwise.hip and add_noise of sampler.hip on caller buffers (one export each).  Test hooks.
int svg_op_act_to_img(svg_ctx* ctx, const float* x, int ldc, uint8_t* img, float* float_out, int N, int h, int w, int oh, int ow, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && (img || float_out) && ldc >= 3 && N > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "act_to_img op: bad arguments (ldc %d N %d %dx%d -> %dx%d)",
              ldc, N, h, w, oh, ow);
    act_to_img(x, ldc, img, float_out, N, h, w, oh, ow, (hipStream_t)stream);
  });
}
int svg_op_nchw_to_actf32(svg_ctx* ctx, const float* x, float* out, int N, int C, int h, int w, float scale, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && out && N > 0 && C > 0 && h > 0 && w > 0, "nchw_to_actf32 op: bad arguments (N %d C %d %dx%d)", N, C, h, w);
    nchw_to_actf32(x, out, N, C, h, w, scale, (hipStream_t)stream);
  });
}
int svg_op_actf32_to_nchw(svg_ctx* ctx, const float* x, int ld, float* out, int N, int C, int h, int w, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && out && N > 0 && C > 0 && ld >= C && h > 0 && w > 0, "actf32_to_nchw op: bad arguments (N %d C %d ld %d %dx%d)", N, C, ld, h, w);
    actf32_to_nchw(x, ld, out, N, C, h, w, (hipStream_t)stream);
  });
}
int svg_op_pixel_linear_f32(svg_ctx* ctx, const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int64_t P, int Cin, int Cout,
                            void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && w && y && P > 0 && Cin > 0 && Cout > 0 && ldx >= Cin && ldy >= Cout, "pixel_linear_f32 op: bad arguments (P %lld Cin %d Cout %d ldx %d ldy %d)",
              (long long)P, Cin, Cout, ldx, ldy);
    pixel_linear_f32(x, ldx, w, b, y, ldy, P, Cin, Cout, (hipStream_t)stream);
  });
}
int svg_op_vae_sample(svg_ctx* ctx, const float* mom, int ldm, const float* eps, float* z, float* mom_nchw, int N, int h, int w, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(mom && z && ldm >= 8 && N > 0 && h > 0 && w > 0, "vae_sample op: bad arguments (ldm %d N %d %dx%d)", ldm, N, h, w);
    vae_sample(mom, ldm, eps, z, mom_nchw, N, h, w, (hipStream_t)stream);
  });
}
int svg_op_add_noise(svg_ctx* ctx, const float* x0, const float* noise, float* out, int64_t n, float sa, float s1a, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x0 && noise && out && n > 0, "add_noise op: bad arguments (n %lld)", (long long)n);
    add_noise(x0, noise, out, n, sa, s1a, (hipStream_t)stream);
  });
}
// the update kernels of sampler.hip on caller buffers, each through the launcher the loop calls.  Test hooks.  The row of a launch
// is either `row` (kSamplerRow host floats) or row idx[0] of the device table `tab`: exactly one of the two.
static SamplerRowArg op_row(const char* what, const float* row, const float* tab, const int* idx) {
  SVG_CHECK((row != nullptr) != (tab != nullptr), "%s op: exactly one of an argument row and a table row", what);
  SVG_CHECK(!tab || idx, "%s op: a table row needs its device counter", what);
  SVG_CHECK(!row || !idx, "%s op: an argument row takes no device counter", what);
  return row ? sampler_row(row) : sampler_row_at(tab, idx);
}
int svg_op_ddim_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, float* x_out, int64_t n,
                     const float* row, const float* tab, const int* idx, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && eps_u && x_out && n >= 0, "ddim_step op: null tensor or negative size (n %lld)", (long long)n);
    ddim_step(x, eps_u, eps_c, guidance, x_out, n, op_row("ddim_step", row, tab, idx), (hipStream_t)stream);
  });
}
int svg_op_dpmpp_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, const float* m_prev, float* x_out,
                      float* m_out, int64_t n, const float* row, const float* tab, const int* idx, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && eps_u && x_out && n >= 0, "dpmpp_step op: null tensor or negative size (n %lld)", (long long)n);
    // k of a table row is on the device: the launcher cannot tell a second-order row there, and the kernel would read through null
    SVG_CHECK(m_prev || !tab, "dpmpp_step op: a table row needs m_prev");
    dpmpp_step(x, eps_u, eps_c, guidance, m_prev, x_out, m_out, n, op_row("dpmpp_step", row, tab, idx), (hipStream_t)stream);
  });
}
int svg_op_lms_step(svg_ctx* ctx, const float* x, const float* eps_u, const float* eps_c, float guidance, float* dhist, float* x_out, int64_t n,
                    const float* row, const float* tab, const int* idx, int order, int step, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && eps_u && dhist && x_out && n >= 0, "lms_step op: null tensor or negative size (n %lld)", (long long)n);
    const SamplerRowArg r = op_row("lms_step", row, tab, idx);
    // the launcher checks the order and step of an argument row; those of a table row are on the device, so the caller states them
    if (tab) SVG_CHECK(step >= 0 && order >= 1 && order <= 4 && order <= step + 1, "lms_step op: order %d at step %d", order, step);
    lms_step(x, eps_u, eps_c, guidance, dhist, x_out, n, r, (hipStream_t)stream);
  });
}
int svg_op_lms_input(svg_ctx* ctx, const float* x, float* o0, float* o1, int64_t n, float c, const float* tab, const int* idx, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && o0 && n >= 0, "lms_input op: null tensor or negative size (n %lld)", (long long)n);
    SVG_CHECK((tab != nullptr) == (idx != nullptr), "lms_input op: a table row needs the table and its device counter");
    lms_input(x, o0, o1, n, tab ? sampler_row_at(tab, idx) : sampler_scale(c), (hipStream_t)stream);
  });
}
int svg_op_sampler_tvec(svg_ctx* ctx, float* tvec, int nb, const float* tab, const int* idx, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(tvec && tab && idx && nb > 0, "sampler_tvec op: bad arguments (nb %d)", nb);
    sampler_tvec(tvec, nb, tab, idx, (hipStream_t)stream);
  });
}
int svg_op_sampler_bump(svg_ctx* ctx, int* idx, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(idx, "sampler_bump op: null counter");
    sampler_bump(idx, (hipStream_t)stream);
  });
}
#endif

// the kernels of eltwise.hip with a 16-bit side on caller buffers.  Test hooks.
int SVG_OP(svg_op_img_to_act)(svg_ctx* ctx, const uint8_t* img, uint16_t* out, int N, int sh, int sw, int H, int W, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(img && out && N > 0 && sh > 0 && sw > 0 && H > 0 && W > 0 && ((uintptr_t)out & 15) == 0, "img_to_act op: bad arguments (N %d %dx%d -> %dx%d)",
              N, sh, sw, H, W);
    img_to_act(img, (h16*)out, N, sh, sw, H, W, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_nchw_to_act)(svg_ctx* ctx, const float* x, uint16_t* out, int N, int C, int h, int w, int Cpad, float scale, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && out && N > 0 && C > 0 && Cpad >= C && h > 0 && w > 0, "nchw_to_act op: bad arguments (N %d C %d -> %d %dx%d)", N, C, Cpad, h, w);
    nchw_to_act(x, (h16*)out, N, C, h, w, Cpad, scale, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_actf32_pad_h16)(svg_ctx* ctx, const float* x, int C, uint16_t* out, int Cpad, int64_t P, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && out && P > 0 && C > 0 && Cpad >= C, "actf32_pad_h16 op: bad arguments (P %lld C %d -> %d)", (long long)P, C, Cpad);
    actf32_pad_h16(x, C, (h16*)out, Cpad, P, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_concat_channels)(svg_ctx* ctx, const uint16_t* a, int Ca, const uint16_t* b, int Cb, uint16_t* out, int64_t P, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(a && b && out && P > 0 && Ca > 0 && Cb > 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0,
              "concat_channels op: bad arguments (P %lld Ca %d Cb %d, 16-byte aligned pointers)", (long long)P, Ca, Cb);
    concat_channels((const h16*)a, Ca, (const h16*)b, Cb, (h16*)out, P, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_f32_to_h16)(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && y && n > 0, "f32_to_h16 op: bad arguments (n %lld)", (long long)n);
    f32_to_h16(x, (h16*)y, n, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_f32_to_h16_x8)(svg_ctx* ctx, const float* x, uint16_t* y, int64_t n, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && y && n > 0, "f32_to_h16_x8 op: bad arguments (n %lld)", (long long)n);
    f32_to_h16_x8(x, (h16*)y, n, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_h16_to_f32)(svg_ctx* ctx, const uint16_t* x, float* y, int64_t n, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(x && y && n > 0, "h16_to_f32 op: bad arguments (n %lld)", (long long)n);
    h16_to_f32((const h16*)x, y, n, (hipStream_t)stream);
  });
}
int SVG_OP(svg_op_timestep_embed)(svg_ctx* ctx, const float* t, uint16_t* out, int N, int dim, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(t && out && N > 0 && dim >= 2 && dim % 2 == 0, "timestep_embed op: bad arguments (N %d dim %d)", N, dim);
    timestep_embed(t, (h16*)out, N, dim, (hipStream_t)stream);
  });
}

int SVG_OP(svg_op_layernorm)(svg_ctx* ctx, const uint16_t* x, const float* gamma, const float* beta, uint16_t* out, int M, int C,
                     float eps, void* stream) {
  return svg_guard(ctx, [&] {
    layernorm(ctx, (const h16*)x, gamma, beta, (h16*)out, M, C, eps, (hipStream_t)stream);
  });
}

int SVG_OP(svg_op_attention)(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* out, int B, int heads,
                     int Sq, int Skv, int d, int ldq, int ldk, int ldvt, int ldo, int64_t qb, int64_t kb, int64_t vtb,
                     int64_t ob, float scale, void* stream) {
  return svg_guard(ctx, [&] {
    AttnArgs a;
    a.q = (const h16*)q; a.k = (const h16*)k; a.vt = (const h16*)vt; a.out = (h16*)out;
    a.B = B; a.heads = heads; a.Sq = Sq; a.Skv = Skv; a.d = d;
    a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo; a.qb = qb; a.kb = kb; a.vtb = vtb; a.ob = ob; a.scale = scale;
    attention(ctx, a, (hipStream_t)stream);
  });
}

// attention on a full descriptor (svg_hip.h: svg_attn_desc), optionally forced onto one instantiation; path = {kernel, d, QB, NST,
// BC, HV} of what ran.  Test hook.
int SVG_OP(svg_op_attention_ex)(svg_ctx* ctx, const svg_attn_desc* d, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(d != nullptr, "attention_ex: no descriptor");
    AttnArgs a;
    a.q = (const h16*)d->q; a.k = (const h16*)d->k; a.vt = (const h16*)d->vt; a.out = (h16*)d->out;
    a.B = d->B; a.heads = d->heads; a.Sq = d->Sq; a.Skv = d->Skv; a.d = d->d;
    a.ldq = d->ldq; a.ldk = d->ldk; a.ldvt = d->ldvt; a.ldo = d->ldo; a.qb = d->qb; a.kb = d->kb; a.vtb = d->vtb; a.ob = d->ob;
    a.scale = d->scale;
    AttnPath f, p;
    f.kernel = d->kernel; f.d = d->d; f.qb = d->qblocks; f.nst = d->nst; f.bc = d->bc; f.hv = d->hv;
    attention(ctx, a, (hipStream_t)stream, d->force ? &f : nullptr, &p);
    if (path) { path[0] = p.kernel; path[1] = p.d; path[2] = p.qb; path[3] = p.nst; path[4] = p.bc; path[5] = p.hv; }
  });
}

// the VAE mid block's fused single-head attention (attn_vae.hip), whatever SVG_VAE_ATTN_FUSED says.  Test hook.
int SVG_OP(svg_op_vae_attention)(svg_ctx* ctx, const uint16_t* q, const uint16_t* k, int ldqk, int64_t qkb, const uint16_t* vt, int ldvt,
                                 int64_t vtb, uint16_t* out, int ldo, int64_t ob, int B, int S, int C, void* stream) {
  return svg_guard(ctx, [&] {
    vae_attention(ctx, (const h16*)q, (const h16*)k, ldqk, qkb, (const h16*)vt, ldvt, vtb, (h16*)out, ldo, ob, B, S, C, (hipStream_t)stream);
  });
}

}  // extern "C"
