// C ABI, operator level: the forward kernels of the latent Transformer / CLIP text tower / MiniLM encoder one by one, one
// layer-walking launch over a caller's stage table, and the training-step kernels (xf_train.hip) one by one (test hooks: each is its
// launcher and nothing else).  Every hook checks what its launcher silently assumes of its arguments and refuses (svg_fail) instead of
// launching.
#include "models.h"
#include "xf_walk.h"
#include "../../include/svg_hip.h"
#include <vector>

namespace {
// the dropout site (seed, site, p) of an operator-level call: the seed goes through the context's device word, as the kernels read it
XfDrop op_drop(svg_ctx* ctx, const char* what, uint64_t seed, int site, float p, hipStream_t s) {
  SVG_CHECK(p >= 0.f && p < 1.f && site >= 0, "%s: bad dropout site (site %d, p %g)", what, site, p);
  if (!ctx->seed_scratch) ctx->seed_scratch = (uint64_t*)ctx->dalloc(sizeof(uint64_t));
  HIP_OK(hipMemcpyAsync(ctx->seed_scratch, &seed, sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));            // `seed` is a stack word
  return XfDrop{ctx->seed_scratch, (uint32_t)site, p};
}
}  // namespace

extern "C" {

int svg_xf_gemm_describe(int M, int N, int K, int* path) {
  return svg_guard(nullptr, [&] {
    SVG_CHECK(path && M >= 1 && N >= 1 && K >= 1, "svg_xf_gemm_describe: bad argument");
    const XfGemmPath p = xf_gemm_describe(M, N, K);
    path[0] = p.form; path[1] = p.mt; path[2] = p.ksplit;
  });
}

int svg_op_xf_gemm(svg_ctx* ctx, const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, int relu_in,
                   void* stream) {
  return svg_guard(ctx, [&] {
    run_planned(ctx, [&]() { xf_gemm(ctx, X, W, bias, Y, M, N, K, relu_in, (hipStream_t)stream); });
  });
}

int svg_op_xf_gemm_ex(svg_ctx* ctx, const float* X, const float* W, const float* bias, const float* residual, float* Y, int M, int N, int K,
                      int act_in, int* path, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && X && W && Y, "svg_op_xf_gemm_ex: null argument");
    SVG_CHECK(M >= 1 && N >= 1 && K >= 1, "svg_op_xf_gemm_ex: empty problem %d x %d x %d", M, N, K);
    SVG_CHECK(act_in >= 0 && act_in <= 3, "svg_op_xf_gemm_ex: act_in %d (0 none, 1 ReLU, 2 quick-GELU, 3 GELU)", act_in);
    XfGemmPath ran{0, 0, 0};
    run_planned(ctx, [&]() { xf_gemm(ctx, X, W, bias, Y, M, N, K, act_in, (hipStream_t)stream, residual, &ran); });
    if (path) { path[0] = ran.form; path[1] = ran.mt; path[2] = ran.ksplit; }
  });
}

int svg_op_xf_add_ln(svg_ctx* ctx, const float* x, const float* r, const float* gamma, const float* beta, float* y, int M, int d, float eps,
                     void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && x && gamma && beta && y, "svg_op_xf_add_ln: null argument");
    SVG_CHECK(M >= 1 && d >= 1, "svg_op_xf_add_ln: empty problem %d x %d", M, d);
    xf_add_ln(x, r, gamma, beta, y, M, d, eps, (hipStream_t)stream);
  });
}

int svg_op_xf_embed_post(svg_ctx* ctx, const float* emb, const float* pe, const int32_t* pe_row, const float* text, int d_txt, float* y, int B,
                         int T, int d, float scale, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && emb && pe && y, "svg_op_xf_embed_post: null argument");
    SVG_CHECK(B >= 1 && T >= 1 && d >= 1 && d_txt >= 0 && d_txt < d, "svg_op_xf_embed_post: B %d T %d d %d d_txt %d", B, T, d, d_txt);
    SVG_CHECK(d_txt == 0 || text, "svg_op_xf_embed_post: %d text channels without a text buffer", d_txt);
    SVG_CHECK(pe_row || B <= 64, "svg_op_xf_embed_post: batch row %d has no row in the 64-row positional table (pass pe_row)", B - 1);
    xf_embed_post(emb, pe, pe_row, text, d_txt, y, B, T, d, scale, (hipStream_t)stream);
  });
}

int svg_op_xf_attention(svg_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldk, const float* mask, const float* kpad,
                        float* o, int Tq, int Tk, int B, int heads, int hd, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && q && k && v && o, "svg_op_xf_attention: null argument");
    SVG_CHECK(Tq >= 1 && Tk >= 1 && B >= 1 && heads >= 1 && hd >= 1, "svg_op_xf_attention: Tq %d Tk %d B %d heads %d hd %d", Tq, Tk, B, heads, hd);
    SVG_CHECK(ldq >= heads * hd && ldk >= heads * hd, "svg_op_xf_attention: row strides %d / %d below heads * hd = %d", ldq, ldk, heads * hd);
    xf_attention(q, ldq, k, v, ldk, mask, o, Tq, Tk, B, heads, hd, (hipStream_t)stream, kpad);
  });
}

int svg_op_xf_attention_qkv(svg_ctx* ctx, const float* qkv, const int32_t* lens, float* o, int B, int T, int heads, int hd, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && qkv && o, "svg_op_xf_attention_qkv: null argument");
    SVG_CHECK(B >= 1 && heads >= 1, "svg_op_xf_attention_qkv: B %d heads %d", B, heads);
    if (lens) xf_attention_padded(qkv, lens, o, B, T, heads, hd, (hipStream_t)stream);
    else xf_attention_causal(qkv, o, B, T, heads, hd, (hipStream_t)stream);
  });
}

int svg_op_xf_embed_tokens(svg_ctx* ctx, const int32_t* ids, const float* tok, const float* pos, float* y, int rows, int T, int d, int vocab,
                           void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ids && tok && pos && y, "svg_op_xf_embed_tokens: null argument");
    SVG_CHECK(rows >= 1 && T >= 1 && vocab >= 1 && d >= 4 && d % 4 == 0, "svg_op_xf_embed_tokens: rows %d T %d vocab %d d %d (a multiple of 4: 16-byte loads)",
              rows, T, vocab, d);
    xf_embed_tokens(ids, tok, pos, y, rows, T, d, vocab, (hipStream_t)stream);
  });
}

int svg_op_xf_embed_bert(svg_ctx* ctx, const int32_t* ids, const float* word, const float* pos, const float* type0, float* y, int rows, int T,
                         int d, int vocab, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ids && word && pos && type0 && y, "svg_op_xf_embed_bert: null argument");
    SVG_CHECK(rows >= 1 && T >= 1 && vocab >= 1 && d >= 4 && d % 4 == 0, "svg_op_xf_embed_bert: rows %d T %d vocab %d d %d (a multiple of 4: 16-byte loads)",
              rows, T, vocab, d);
    xf_embed_bert(ids, word, pos, type0, y, rows, T, d, vocab, (hipStream_t)stream);
  });
}

int svg_op_xf_mean_pool_norm(svg_ctx* ctx, const float* x, const int32_t* lens, float* out, int B, int T, int d, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && x && lens && out, "svg_op_xf_mean_pool_norm: null argument");
    SVG_CHECK(B >= 1 && T >= 1 && d >= 1, "svg_op_xf_mean_pool_norm: B %d T %d d %d", B, T, d);
    xf_mean_pool_norm(x, lens, out, B, T, d, (hipStream_t)stream);
  });
}

int svg_op_xf_walk(svg_ctx* ctx, const svg_walk_stage* stages, int n_stages, int rows, int small, int* info, void* stream) {
  return svg_guard(ctx, [&] {
    hipStream_t s = (hipStream_t)stream;
    SVG_CHECK(ctx && stages, "svg_op_xf_walk: null argument");
    SVG_CHECK(n_stages >= 1 && n_stages <= kWalkMaxOps, "svg_op_xf_walk: %d stages (at most %d)", n_stages, kWalkMaxOps);
    if (small) rows = kWalkSmallRows;
    SVG_CHECK(rows >= 1 && rows <= kWalkMaxRows, "svg_op_xf_walk: %d rows (at most %d)", rows, kWalkMaxRows);
    const int grid = xf_walk_grid();
    if (!xf_walk_enabled(s) || grid < 8) throw SvgHipError("svg_op_xf_walk: the layer-walking launch is unavailable on this device / stream");
    std::vector<WalkOp> ops(n_stages);
    int Tq = 1, Tk = 1, hd = 4;                            // the largest attention job of the table sizes the LDS
    for (int i = 0; i < n_stages; ++i) {
      const svg_walk_stage& g = stages[i];
      WalkOp op{};
      op.kind = g.kind; op.bar = g.bar; op.M = g.M; op.N = g.N; op.K = g.K; op.ld = g.ld; op.ksplit = g.ksplit; op.relu = g.relu;
      op.X = g.X; op.W = g.W; op.slab = g.slab; op.bias = g.bias; op.res = g.res; op.Y = g.Y;
      op.g1 = g.g1; op.b1 = g.b1; op.g2 = g.g2; op.b2 = g.b2; op.Y2 = g.Y2; op.eps = g.eps;
      op.Tq = g.Tq; op.Tk = g.Tk; op.B = g.B; op.heads = g.heads; op.hd = g.hd;
      op.q_ld = g.q_ld; op.kv_ld = g.kv_ld; op.q_span = g.q_span; op.kv_span = g.kv_span;
      op.qs = g.qs; op.ks = g.ks; op.vs = g.vs; op.mask = g.mask; op.kpad = g.kpad;
      op.pe = g.pe; op.pe_row = g.pe_row; op.text = g.text; op.d_txt = g.d_txt; op.T = g.T; op.scale = g.scale;
      op.ldy = g.ldy; op.ld_res = g.ld_res; op.reuse_x = g.reuse_x; op.perm = g.perm; op.Yln = g.Yln;
      ops[i] = op;
      if (g.kind == WK_ATTN) {
        SVG_CHECK(g.hd >= 4 && g.hd % 4 == 0 && g.Tq >= 1 && g.Tq <= 32 && g.Tk >= 1 && g.Tk <= 32 && g.heads >= 1 && g.B >= 1,
                  "svg_op_xf_walk: stage %d: attention Tq %d Tk %d (at most 32) head dim %d (a multiple of 4)", i, g.Tq, g.Tk, g.hd);
        SVG_CHECK(g.q_ld >= g.heads * g.hd && g.kv_ld >= g.heads * g.hd, "svg_op_xf_walk: stage %d: row strides below heads * hd", i);
        Tq = std::max(Tq, g.Tq); Tk = std::max(Tk, g.Tk); hd = std::max(hd, g.hd);
      }
      if (g.kind == WK_EMBED || (g.kind == WK_GEMMF && g.pe))
        SVG_CHECK(g.pe_row || g.B <= 64, "svg_op_xf_walk: stage %d: batch row %d has no row in the 64-row positional table (pass pe_row)", i, g.B - 1);
    }
    const int64_t lds = small ? xf_walk_small_lds_bytes(std::max(Tq, Tk), hd) : xf_walk_lds_bytes(rows, Tq, Tk, hd);
    if (small) xf_walk_small_launch(ctx, ops.data(), n_stages, lds, s);
    else xf_walk_launch(ctx, ops.data(), n_stages, rows, lds, s);
    if (info) { info[0] = grid; info[1] = (int)lds; info[2] = small ? 0 : xf_walk_mt(rows); info[3] = (int)sizeof(svg_walk_stage); }
    HIP_OK(hipStreamSynchronize(s));                       // a give-up of THIS launch is raised by this call
    xf_walk_check(ctx);
  });
}

// ---- the training kernels one by one ---------------------------------------------------------------------------------------------
int svg_op_dropout_mask(svg_ctx* ctx, uint64_t seed, int site, float p, float* out, int64_t n, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && out && n >= 0, "svg_op_dropout_mask: bad argument");
    xf_drop_mask(op_drop(ctx, "svg_op_dropout_mask", seed, site, p, (hipStream_t)stream), out, n, (hipStream_t)stream);
  });
}

int svg_op_xf_gemm_tn(svg_ctx* ctx, const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int M, int N, int K, int accumulate,
                      void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && dY && X && dW, "svg_op_xf_gemm_tn: null argument");
    xf_gemm_tn(dY, ldy, X, ldx, dW, db, M, N, K, accumulate, (hipStream_t)stream);
  });
}

int svg_op_xf_gemm_nn(svg_ctx* ctx, const float* dY, int ldy, const float* W, float* out, int M, int N, int K, const float* gate, float gate_scale,
                      const float* add, int* splits, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && dY && W && out, "svg_op_xf_gemm_nn: null argument");
    SVG_CHECK(M > 0 && N > 0 && K > 0, "svg_op_xf_gemm_nn: empty problem %d x %d x %d", M, N, K);
    run_planned(ctx, [&]() {
      float* slabs = ctx->arena.get<float>(xf_gemm_nn_slab_floats(M, N, K));
      if (SVG_LAUNCHING(ctx)) xf_gemm_nn(dY, ldy, W, slabs, out, M, N, K, gate, gate_scale, add, (hipStream_t)stream);
    });
    if (splits) *splits = xf_gemm_nn_splits(N, K);
  });
}

int svg_op_xf_relu_drop(svg_ctx* ctx, const float* h, float* r, int64_t n, uint64_t seed, int site, float p, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && h && r && n >= 0, "svg_op_xf_relu_drop: bad argument");
    xf_relu_drop(h, r, n, op_drop(ctx, "svg_op_xf_relu_drop", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
  });
}

int svg_op_xf_add_ln_train(svg_ctx* ctx, const float* x, const float* r, uint64_t seed, int site, float p, const float* gamma, const float* beta,
                           float* y, float* xhat, float* rstd, int M, int d, float eps, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && x && gamma && beta && y && xhat && rstd, "svg_op_xf_add_ln_train: null argument");
    xf_add_ln_train(x, r, op_drop(ctx, "svg_op_xf_add_ln_train", seed, site, p, (hipStream_t)stream), gamma, beta, y, xhat, rstd, M, d, eps,
                    (hipStream_t)stream);
  });
}

int svg_op_xf_ln_bwd(svg_ctx* ctx, const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* dz_drop,
                     uint64_t seed, int site, float p, float* dgamma, float* dbeta, int M, int d, int accumulate, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && dy && xhat && rstd && gamma && dz && dgamma && dbeta, "svg_op_xf_ln_bwd: null argument");
    xf_ln_bwd(dy, xhat, rstd, gamma, dz, dz_drop, op_drop(ctx, "svg_op_xf_ln_bwd", seed, site, p, (hipStream_t)stream), dgamma, dbeta, M, d,
              accumulate, (hipStream_t)stream);
  });
}

int svg_op_xf_attention_train(svg_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldk, const float* mask, float* o,
                              float* P, int Tq, int Tk, int B, int heads, int hd, uint64_t seed, int site, float p, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && q && k && v && o && P, "svg_op_xf_attention_train: null argument");
    xf_attention_train(q, ldq, k, v, ldk, mask, o, P, Tq, Tk, B, heads, hd,
                       op_drop(ctx, "svg_op_xf_attention_train", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
  });
}

int svg_op_xf_attention_bwd(svg_ctx* ctx, const float* dout, const float* q, int ldq, const float* k, const float* v, int ldk, const float* P,
                            float* dq, int lddq, float* dk, float* dv, int lddk, int Tq, int Tk, int B, int heads, int hd, uint64_t seed,
                            int site, float p, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && dout && q && k && v && P && dq && dk && dv, "svg_op_xf_attention_bwd: null argument");
    xf_attention_bwd(dout, q, ldq, k, v, ldk, P, dq, lddq, dk, dv, lddk, Tq, Tk, B, heads, hd,
                     op_drop(ctx, "svg_op_xf_attention_bwd", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
  });
}

int svg_op_xf_embed_post_train(svg_ctx* ctx, const float* emb, const float* pe, const int32_t* pe_row, const float* text, int d_txt, float* y,
                               int B, int T, int d, float scale, uint64_t seed, int site, float p, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && emb && pe && y, "svg_op_xf_embed_post_train: null argument");
    xf_embed_post_train(emb, pe, pe_row, text, d_txt, y, B, T, d, scale,
                        op_drop(ctx, "svg_op_xf_embed_post_train", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
  });
}

int svg_op_xf_embed_post_bwd(svg_ctx* ctx, const float* dy, float* de, int B, int T, int d, int d_img, float scale, uint64_t seed, int site,
                             float p, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && dy && de, "svg_op_xf_embed_post_bwd: null argument");
    xf_embed_post_bwd(dy, de, B, T, d, d_img, scale, op_drop(ctx, "svg_op_xf_embed_post_bwd", seed, site, p, (hipStream_t)stream),
                      (hipStream_t)stream);
  });
}

int svg_op_xf_criterion(svg_ctx* ctx, const float* pred, const float* expected, float* dpred, float* losses, int Tt, int B, int D, int t0,
                        int fh, int fw, float w_mse, float w_l1, float w_gdl, float alpha, float w_nce, float temperature, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && pred && expected && dpred && losses, "svg_op_xf_criterion: null argument");
    SVG_CHECK(Tt > 0 && B > 0, "svg_op_xf_criterion: empty problem (%d x %d rows)", Tt, B);
    float h_losses[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    run_planned(ctx, [&]() {
      float* part = ctx->arena.get<float>((int64_t)Tt * B * 3);          // the per-row partial sums and the device copy of the losses
      float* part2 = ctx->arena.get<float>((int64_t)Tt * B);
      float* d_losses = ctx->arena.get<float>(5);
      if (!SVG_LAUNCHING(ctx)) return;
      xf_criterion(pred, expected, dpred, part, part2, d_losses, Tt, B, D, t0, fh, fw, w_mse, w_l1, w_gdl, alpha, w_nce, temperature,
                   (hipStream_t)stream);
      HIP_OK(hipMemcpyAsync(h_losses, d_losses, sizeof(h_losses), hipMemcpyDeviceToHost, (hipStream_t)stream));
      HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    });
    for (int i = 0; i < 5; ++i) losses[i] = h_losses[i];                 // losses: host memory
  });
}

}  // extern "C"
