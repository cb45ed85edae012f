// Forward plan and stage tables of the latent Transformer (xf_plan.h).  Pure host code: no HIP runtime call, no kernel, no workspace
// allocation of its own, no environment lookup — every fact it decides on comes in through its arguments.
#include "xf_plan.h"
#include <cmath>

namespace {
// q (Tq*B rows of q_ld floats, q_span floats to the end of its buffer), k / v (Tk*B rows of kv_ld floats) -> o
WalkOp attn_op(const XfModel& m, int B, const float* q, int q_ld, int64_t q_span, const float* k, const float* v, int kv_ld, int64_t kv_span, int Tq,
               int Tk, const float* mask, const float* kpad, float* o) {
  WalkOp op{};
  op.kind = WK_ATTN; op.bar = 1; op.Tq = Tq; op.Tk = Tk; op.B = B; op.heads = m.heads; op.hd = m.d_model / m.heads;
  op.q_ld = q_ld; op.kv_ld = kv_ld; op.q_span = (int)q_span; op.kv_span = (int)kv_span;
  op.qs = q; op.ks = k; op.vs = v; op.mask = mask; op.kpad = kpad; op.Y = o;
  return op;
}
}  // namespace

XfWalkWs xf_walk_workspace(const XfModel& m, const XfChunk& c, int form, float* (*alloc)(void*, int64_t), void* user) {
  const int64_t d = m.d_model, d_img = d - m.text_dim, ffn = m.ffn, d_lat = m.d_lat;
  const int64_t Ms = (int64_t)c.Ts * c.B, Mt = (int64_t)c.Tt * c.B, Mx = std::max(Ms, Mt);
  auto get = [&](int64_t n) { return alloc(user, n); };
  XfWalkWs w{};
  if (form == XF_WALK) {
    auto slabs = [&](int64_t M, int64_t N, int64_t K) { return (K / 128) * M * N; };
    int64_t sa = std::max(slabs(Mx, 3 * d, d), std::max(slabs(Mx, ffn, d), slabs(Mx, d, ffn)));
    sa = std::max(sa, std::max(slabs(Mx, d_img, d_lat), slabs(Mx, d_lat, d)));
    w.slabA = get(sa);
    w.slabB = get(std::max(slabs(Ms, 2 * d, d), slabs(Mt, d_img, d_lat)));
    // row buffers with fixed roles (a stage never writes a buffer another workgroup still reads in the same stage): the embeddings; the
    // encoder's norm1 / norm2 results; the memory; the decoder's norm1 / norm2 / norm3 results
    w.xs_e = get(Ms * d);
    w.xt_e = c.same() ? w.xs_e : get(Mt * d);
    w.e1 = get(Ms * d); w.e2 = get(Ms * d); w.mem = get(Ms * d);
    w.t1 = get(Mt * d); w.t2 = get(Mt * d); w.t3 = get(Mt * d);
    w.o = get(Mx * d);
    w.h = get(Mx * ffn);
    w.qkv = get(Mx * 3 * d);     // reduced self-attention projections; the cross-attention's q
    w.kvm = get(Ms * 2 * d);     // reduced K, V of the encoder memory
  } else {
    w.xs_e = get(Ms * d);                     // embeddings
    w.xt_e = c.same() ? w.xs_e : get(Mt * d);
    w.qkv = get(Mx * 3 * d);
    w.kvm = get(Ms * 2 * d);
    w.o = get(Mx * d);
    w.h = get(Mx * ffn);
    w.pA = get(Mx * d);                       // pre-LayerNorm sums: attention block, cross-attention block,
    w.pB = get(Mx * d);
    w.pC = get(Mx * d);                       // feed-forward block (the next layer's input)
    w.pM = get(Ms * d);                       // the last encoder layer's (the memory, before its two norms)
    w.lA = get(Mx * d);                       // the normalised rows the consumers publish
    w.lB = get(Mx * d);
    w.lC = get(Mx * d);
  }
  return w;
}

// ---- the split-K form (xf_walk.hip: xf_walk_kernel) -------------------------------------------------------------------------------------
// Stages per encoder layer: GEMM in_proj | add slabs + bias | attention | GEMM out_proj | add slabs + bias + residual + LayerNorm |
// GEMM linear1 | add slabs + bias, ReLU | GEMM linear2 | add + LayerNorm.  A decoder layer has the cross-attention block in between; its
// K / V projection of the encoder memory shares the stage of the self-attention in_proj (no barrier of its own).  The final encoder /
// decoder LayerNorm rides on the last layer's add + LayerNorm stage (Y2).
void xf_walk_table(const XfModel& m, const XfChunk& c, const XfWalkWs& ws, std::vector<WalkOp>& ops) {
  const int d = m.d_model, d_img = d - m.text_dim, ffn = m.ffn, d_lat = m.d_lat, B = c.B, Ts = c.Ts, Tt = c.Tt;
  const int Ms = Ts * B, Mt = Tt * B;
  const bool same = c.same();
  float *slabA = ws.slabA, *slabB = ws.slabB, *qkv = ws.qkv, *kvm = ws.kvm, *o = ws.o, *h = ws.h, *e1 = ws.e1, *e2 = ws.e2, *mem = ws.mem,
        *t1 = ws.t1, *t2 = ws.t2, *t3 = ws.t3;
  auto gemm = [&](const float* X, int ld, const float* W, float* slab, int M, int N, int K, bool bar = true) {
    WalkOp op{};
    op.kind = WK_GEMM; op.bar = bar; op.M = M; op.N = N; op.K = K; op.ld = ld; op.ksplit = K / 128; op.X = X; op.W = W; op.slab = slab;
    ops.push_back(op);
  };
  auto red = [&](const float* slab, int M, int N, int K, const float* bias, float* Y, bool relu, bool bar = true) {
    WalkOp op{};
    op.kind = WK_RED; op.bar = bar; op.M = M; op.N = N; op.ksplit = K / 128; op.slab = (float*)slab; op.bias = bias; op.Y = Y; op.relu = relu;
    ops.push_back(op);
  };
  // y = LN(x + (slabs + bias)) g + b [; y2 = LN(y) g2 + b2]
  auto ln = [&](const float* slab, int M, int K, const float* bias, const float* res, const float* g, const float* b, float* Y,
                const float* g2 = nullptr, const float* b2 = nullptr, float* Y2 = nullptr) {
    WalkOp op{};
    op.kind = WK_LN; op.bar = 1; op.M = M; op.N = d; op.ksplit = slab ? K / 128 : 0; op.slab = (float*)slab; op.bias = bias; op.res = res;
    op.g1 = g; op.b1 = b; op.Y = Y; op.g2 = g2; op.b2 = b2; op.Y2 = Y2; op.eps = 1e-5f;
    ops.push_back(op);
  };
  auto attn = [&](const float* q, int q_ld, int64_t q_span, const float* k, const float* v, int kv_ld, int64_t kv_span, int Tq, int Tk, const float* msk,
                  const float* kpad) { ops.push_back(attn_op(m, B, q, q_ld, q_span, k, v, kv_ld, kv_span, Tq, Tk, msk, kpad, o)); };
  auto embed = [&](const float* slab, int T, float* Y, bool bar) {
    WalkOp op{};
    op.kind = WK_EMBED; op.bar = bar; op.M = B * T; op.N = d_img; op.ksplit = d_lat / 128; op.slab = (float*)slab; op.bias = m.w.emb_b; op.Y = Y;
    op.pe = m.pe; op.pe_row = c.pe_row; op.text = c.text; op.d_txt = m.text_dim; op.T = T; op.B = B; op.scale = sqrtf((float)d);
    ops.push_back(op);
  };

  // embeddings (the launch's inputs: no barrier before the first stage)
  gemm(c.src, d_lat, m.w.emb_w, slabA, B * Ts, d_img, d_lat, false);
  if (!same) gemm(c.tgt, d_lat, m.w.emb_w, slabB, B * Tt, d_img, d_lat, false);
  embed(slabA, Ts, ws.xs_e, true);
  if (!same) embed(slabB, Tt, ws.xt_e, false);
  const float* xs_cur = ws.xs_e;
  for (int i = 0; i < m.enc_layers; ++i) {
    const XfModel::LayerW& w = m.w.enc[i];
    const bool last = (i + 1 == m.enc_layers);
    gemm(xs_cur, d, w.in_w, slabA, Ms, 3 * d, d);
    red(slabA, Ms, 3 * d, d, w.in_b, qkv, false);
    attn(qkv, 3 * d, (int64_t)Ms * 3 * d, qkv + d, qkv + 2 * d, 3 * d, (int64_t)Ms * 3 * d - d, Ts, Ts, nullptr, c.src_pad);
    gemm(o, d, w.out_w, slabA, Ms, d, d);
    ln(slabA, Ms, d, w.out_b, xs_cur, w.n_w[0], w.n_b[0], e1);
    gemm(e1, d, w.l1_w, slabA, Ms, ffn, d);
    red(slabA, Ms, ffn, d, w.l1_b, h, true);
    gemm(h, ffn, w.l2_w, slabA, Ms, d, ffn);
    if (last) ln(slabA, Ms, ffn, w.l2_b, e1, w.n_w[1], w.n_b[1], nullptr, m.w.encn_w, m.w.encn_b, mem);   // + transformer.encoder.norm
    else ln(slabA, Ms, ffn, w.l2_b, e1, w.n_w[1], w.n_b[1], e2);
    xs_cur = e2;
  }
  if (m.enc_layers == 0) ln(nullptr, Ms, 0, nullptr, xs_cur, m.w.encn_w, m.w.encn_b, mem);
  const float* xt_cur = ws.xt_e;
  for (int i = 0; i < m.dec_layers; ++i) {
    const XfModel::LayerW& w = m.w.dec[i];
    const bool last = (i + 1 == m.dec_layers);
    gemm(xt_cur, d, w.in_w, slabA, Mt, 3 * d, d);
    gemm(mem, d, w.cin_w + (int64_t)d * d, slabB, Ms, 2 * d, d, false);                            // K, V of the memory: rows d .. 3d of in_proj
    red(slabA, Mt, 3 * d, d, w.in_b, qkv, false);
    red(slabB, Ms, 2 * d, d, w.cin_b + d, kvm, false, false);
    attn(qkv, 3 * d, (int64_t)Mt * 3 * d, qkv + d, qkv + 2 * d, 3 * d, (int64_t)Mt * 3 * d - d, Tt, Tt, c.mask, c.tgt_pad);
    gemm(o, d, w.out_w, slabA, Mt, d, d);
    ln(slabA, Mt, d, w.out_b, xt_cur, w.n_w[0], w.n_b[0], t1);
    gemm(t1, d, w.cin_w, slabA, Mt, d, d);                                                          // q: rows 0 .. d of in_proj
    red(slabA, Mt, d, d, w.cin_b, qkv, false);
    attn(qkv, d, (int64_t)Mt * d, kvm, kvm + d, 2 * d, (int64_t)Ms * 2 * d, Tt, Ts, nullptr, nullptr);
    gemm(o, d, w.cout_w, slabA, Mt, d, d);
    ln(slabA, Mt, d, w.cout_b, t1, w.n_w[1], w.n_b[1], t2);
    gemm(t2, d, w.l1_w, slabA, Mt, ffn, d);
    red(slabA, Mt, ffn, d, w.l1_b, h, true);
    gemm(h, ffn, w.l2_w, slabA, Mt, d, ffn);
    if (last) ln(slabA, Mt, ffn, w.l2_b, t2, w.n_w[2], w.n_b[2], nullptr, m.w.decn_w, m.w.decn_b, t3);     // + transformer.decoder.norm
    else ln(slabA, Mt, ffn, w.l2_b, t2, w.n_w[2], w.n_b[2], t3);
    xt_cur = t3;
  }
  if (m.dec_layers == 0) { ln(nullptr, Mt, 0, nullptr, xt_cur, m.w.decn_w, m.w.decn_b, t3); xt_cur = t3; }
  gemm(xt_cur, d, m.w.out_w, slabA, Mt, d_lat, d);
  red(slabA, Mt, d_lat, d, m.w.out_b, c.out, false);
}

// ---- the small-row form (xf_walk.hip: xf_walk_small_kernel): at most 8 rows per forward — single-clip sampling ------------------------
// Stages per encoder layer: in_proj (LayerNorm of its input folded in; q, k, v as column blocks of one stage) | attention | out_proj + bias +
// residual | linear1 (LayerNorm 1 folded in) + bias + ReLU | linear2 + bias + residual — 5 device-wide barriers instead of 9; a decoder layer
// has 8 instead of 16 (the K / V projection of the encoder memory rides on the self-attention in_proj's barrier, with the encoder's two final
// LayerNorms folded into its input).  What flows between layers is the PRE-LayerNorm sum; the consumer normalises its own LDS copy of the rows
// and publishes the normalised rows (Yln) for the residual of the stage after next.
void xf_walk_small_table(const XfModel& m, const XfChunk& c, const XfWalkWs& ws, int grid, std::vector<WalkOp>& ops) {
  const int d = m.d_model, ffn = m.ffn, d_lat = m.d_lat, B = c.B, Ts = c.Ts, Tt = c.Tt;
  const int Ms = Ts * B, Mt = Tt * B;
  float *qkv = ws.qkv, *kvm = ws.kvm, *o = ws.o, *h = ws.h, *pA = ws.pA, *pB = ws.pB, *pC = ws.pC, *lA = ws.lA, *lB = ws.lB, *lC = ws.lC;
  const int blk = 8 * grid;                                               // widest column block a stage serves (8 columns per workgroup)
  struct Ln { const float* g1 = nullptr; const float* b1 = nullptr; const float* g2 = nullptr; const float* b2 = nullptr; float* Yln = nullptr; };
  // Y[:, 0..N) = act(LN(X) W^T + bias) (+ res); first block of a stage: barrier (unless `nobar`), X staged and normalised; further blocks reuse it.
  // embed_T > 0: the embedding — X rows in (b, t) order, Y rows (t, b), scaled, the positional row added
  auto gemmf = [&](const float* X, int ld, int M, int K, const float* W, const float* bias, int N, float* Y, int ldy, const Ln& ln, bool relu,
                   const float* res, int ld_res, bool bar, int embed_T = 0) {
    for (int n0 = 0; n0 < N; n0 += blk) {
      WalkOp op{};
      op.kind = WK_GEMMF; op.bar = (n0 == 0 && bar) ? 1 : 0; op.reuse_x = n0 == 0 ? 0 : 1;
      op.M = M; op.N = std::min(blk, N - n0); op.K = K; op.ld = ld; op.X = X; op.W = W + (int64_t)n0 * K; op.bias = bias ? bias + n0 : nullptr;
      op.Y = Y + n0; op.ldy = ldy; op.res = res ? res + n0 : nullptr; op.ld_res = ld_res; op.relu = relu ? 1 : 0; op.eps = 1e-5f;
      if (n0 == 0) { op.g1 = ln.g1; op.b1 = ln.b1; op.g2 = ln.g2; op.b2 = ln.b2; op.Yln = ln.Yln; }
      if (embed_T) { op.perm = 1; op.B = B; op.T = embed_T; op.scale = sqrtf((float)d); op.pe = m.pe + n0; op.pe_row = c.pe_row; }
      ops.push_back(op);
    }
  };
  auto attn = [&](const float* q, int q_ld, int64_t q_span, const float* k, const float* v, int kv_ld, int64_t kv_span, int Tq, int Tk, const float* msk,
                  const float* kpad) { ops.push_back(attn_op(m, B, q, q_ld, q_span, k, v, kv_ld, kv_span, Tq, Tk, msk, kpad, o)); };
  auto embed = [&](const float* x, int T, float* Y) {                    // the launch's inputs: no barrier before the first stage
    gemmf(x, d_lat, B * T, d_lat, m.w.emb_w, m.w.emb_b, d, Y, d, Ln{}, false, nullptr, d, false, T);
  };

  embed(c.src, Ts, ws.xs_e);
  if (!c.same()) embed(c.tgt, Tt, ws.xt_e);
  // ---- encoder.  `cur` = the layer's input rows before their LayerNorm (`cln`: its parameters; none for the embedding), `curl` = where
  // the normalised rows are published (the embedding itself when there is no norm)
  const float* cur = ws.xs_e; Ln cln; const float* curl = ws.xs_e;
  for (int i = 0; i < m.enc_layers; ++i) {
    const XfModel::LayerW& w = m.w.enc[i];
    const bool last = (i + 1 == m.enc_layers);
    Ln l0 = cln; if (l0.g1) { l0.Yln = lA; curl = lA; }
    gemmf(cur, d, Ms, d, w.in_w, w.in_b, 3 * d, qkv, 3 * d, l0, false, nullptr, 0, true);
    attn(qkv, 3 * d, (int64_t)Ms * 3 * d, qkv + d, qkv + 2 * d, 3 * d, (int64_t)Ms * 3 * d - d, Ts, Ts, nullptr, c.src_pad);
    gemmf(o, d, Ms, d, w.out_w, w.out_b, d, pA, d, Ln{}, false, curl, d, true);
    gemmf(pA, d, Ms, d, w.l1_w, w.l1_b, ffn, h, ffn, Ln{w.n_w[0], w.n_b[0], nullptr, nullptr, lB}, true, nullptr, 0, true);
    float* pout = last ? ws.pM : pC;
    gemmf(h, ffn, Ms, ffn, w.l2_w, w.l2_b, d, pout, d, Ln{}, false, lB, d, true);
    cur = pout; cln = Ln{w.n_w[1], w.n_b[1], nullptr, nullptr, nullptr}; curl = nullptr;
  }
  // the memory = encoder.norm(norm2(last sum)) (or encoder.norm(embedding) for an empty encoder): folded into every consumer
  Ln lmem = m.enc_layers ? Ln{cln.g1, cln.b1, m.w.encn_w, m.w.encn_b, nullptr} : Ln{m.w.encn_w, m.w.encn_b, nullptr, nullptr, nullptr};
  const float* memp = cur;
  // ---- decoder
  cur = ws.xt_e; cln = Ln{}; curl = ws.xt_e;
  for (int i = 0; i < m.dec_layers; ++i) {
    const XfModel::LayerW& w = m.w.dec[i];
    Ln l0 = cln; if (l0.g1) { l0.Yln = lA; curl = lA; }
    gemmf(cur, d, Mt, d, w.in_w, w.in_b, 3 * d, qkv, 3 * d, l0, false, nullptr, 0, true);
    gemmf(memp, d, Ms, d, w.cin_w + (int64_t)d * d, w.cin_b + d, 2 * d, kvm, 2 * d, lmem, false, nullptr, 0, false);     // K, V of the memory
    attn(qkv, 3 * d, (int64_t)Mt * 3 * d, qkv + d, qkv + 2 * d, 3 * d, (int64_t)Mt * 3 * d - d, Tt, Tt, c.mask, c.tgt_pad);
    gemmf(o, d, Mt, d, w.out_w, w.out_b, d, pA, d, Ln{}, false, curl, d, true);
    gemmf(pA, d, Mt, d, w.cin_w, w.cin_b, d, qkv, d, Ln{w.n_w[0], w.n_b[0], nullptr, nullptr, lB}, false, nullptr, 0, true);   // q of the cross-attention
    attn(qkv, d, (int64_t)Mt * d, kvm, kvm + d, 2 * d, (int64_t)Ms * 2 * d, Tt, Ts, nullptr, nullptr);
    gemmf(o, d, Mt, d, w.cout_w, w.cout_b, d, pB, d, Ln{}, false, lB, d, true);
    gemmf(pB, d, Mt, d, w.l1_w, w.l1_b, ffn, h, ffn, Ln{w.n_w[1], w.n_b[1], nullptr, nullptr, lC}, true, nullptr, 0, true);
    gemmf(h, ffn, Mt, ffn, w.l2_w, w.l2_b, d, pC, d, Ln{}, false, lC, d, true);
    cur = pC; cln = Ln{w.n_w[2], w.n_b[2], nullptr, nullptr, nullptr}; curl = nullptr;
  }
  Ln lout = m.dec_layers ? Ln{cln.g1, cln.b1, m.w.decn_w, m.w.decn_b, nullptr} : Ln{m.w.decn_w, m.w.decn_b, nullptr, nullptr, nullptr};
  gemmf(cur, d, Mt, d, m.w.out_w, m.w.out_b, d_lat, c.out, d_lat, lout, false, nullptr, 0, true);
}

void xf_walk_account(const std::vector<WalkOp>& ops, double* flops, double* bytes) {
  *flops = 0; *bytes = 0;
  for (const WalkOp& op : ops)
    if (op.kind == WK_GEMM || op.kind == WK_GEMMF) {
      *flops += 2.0 * op.M * (double)op.N * op.K;
      *bytes += 4.0 * ((double)op.N * op.K + (op.reuse_x ? 0.0 : (double)op.M * op.K) + (double)op.M * op.N);
    }
}

namespace {
// The length of the table a form would get for a chunk of this shape: the builder itself, run over stand-in addresses (no memory behind them)
int count_stages(const XfModel& m, const XfShape& sh, int B, int form, int grid) {
  float* const fake = (float*)(uintptr_t)0x1000;
  XfChunk c{B, sh.Ts, sh.Tt, fake, sh.same ? fake : fake + 1, nullptr, nullptr, nullptr, nullptr, nullptr, fake};
  const XfWalkWs ws = xf_walk_workspace(m, c, form, [](void*, int64_t) { return (float*)(uintptr_t)0x1000; }, nullptr);
  std::vector<WalkOp> ops;
  ops.reserve(192);
  if (form == XF_WALK) xf_walk_table(m, c, ws, ops);
  else xf_walk_small_table(m, c, ws, grid, ops);
  return (int)ops.size();
}
}  // namespace

XfPlan xf_plan(const XfModel& m, const XfShape& sh, const XfDevice& dev, const XfKnobs& knobs) {
  const int d = m.d_model, d_img = d - m.text_dim, hd = d / m.heads, Tmax = std::max(sh.Ts, sh.Tt);
  // The layer-walking launch (xf_walk.hip) can serve up to kWalkMaxRows rows, and alone on the device it is ahead of the per-GEMM kernels at
  // every size (28 % at 6-48 rows, 8 % at 168).  But it owns every compute unit while it runs: the sampling loop's two stream groups, whose
  // 168-row forwards overlap on the per-GEMM path, serialise (4250 vs 4709 frames/s without denoising, profiles/README.md).  So by default
  // it takes the latency-bound sizes only (SVG_XF_WALK_ROWS, default 96 rows = 16 clips x 6 tokens); larger batches go through the per-GEMM
  // kernels, which stream W once for up to 336 rows (SVG_XF_WALK_SPLIT=1: through the walk in chunks).
  const int Bw = std::max(1, (int)std::min<int64_t>(kWalkMaxRows, knobs.walk_rows) / Tmax);
  XfPlan p;
  p.Bc = std::max(1, 336 / Tmax);
  // off for this device (SVG_XF_WALK=0, ranks sharing it, an earlier give-up, a grid the device cannot hold) or a stream under capture
  if (!dev.walk_enabled) return p;
  const int Bchunk = std::min(sh.B, Bw), rows = Bchunk * Tmax;
  const int64_t lds = xf_walk_lds_bytes(rows, Tmax, Tmax, hd);
  p.refusal = XF_SHAPE;
  if (!(xf_walk_gemm_ok(d, d) && xf_walk_gemm_ok(m.ffn, d) && xf_walk_gemm_ok(d, m.ffn) && xf_walk_gemm_ok(d_img, m.d_lat) && xf_walk_gemm_ok(m.d_lat, d)))
    return p;
  if (d > 3072 || hd % 4 || m.text_dim % 4 || !xf_walk_available(rows, lds, dev.lds_limit)) return p;
  const int n = count_stages(m, sh, Bchunk, XF_WALK, dev.grid);
  p.refusal = XF_STAGES;
  if (n > kWalkMaxOps) return p;
  p.refusal = XF_OFF;
  if (sh.B > Bw && knobs.walk_split == 0) return p;
  p.refusal = XF_TAKEN; p.form = XF_WALK; p.Bc = Bw; p.rows = rows; p.lds_bytes = lds; p.n_stages = n;

  // at most 8 rows (one clip): the small-row form — whole-K GEMM stages with LayerNorm / bias / residual folded in, 5 + 8 instead of 9 + 16
  // stages per encoder / decoder layer.
  // $SVG_XF_WALK_SMALL: 1 always (where the shapes fit), 0 never, unset: where it is ahead of the split-K walk — d_model <= 1024 (measured, one
  // clip of 6 tokens, profiles/r05_walk_small_vs_splitk.txt: d = 256 0.789 -> 0.618 ms, 512 0.811 -> 0.637, 1024 0.897 -> 0.785; d = 2048
  // 1.053 vs 1.059: there a stage is bound by the 64 KB of weights a compute unit has to pull per column block, not by the stage count)
  if (knobs.walk_small == 0 || (knobs.walk_small < 0 && d > 1024)) return p;
  if (sh.has_text || m.text_dim != 0 || sh.B * Tmax > kWalkSmallRows || hd % 4) return p;
  for (int K : {d, m.ffn, m.d_lat})
    if (K % 256 != 0 || K < 256 || K > kWalkSmallMaxK) return p;
  const int64_t lds_small = xf_walk_small_lds_bytes(Tmax, hd);
  if (dev.grid < 8 || !xf_walk_available(kWalkSmallRows, lds_small, dev.lds_limit)) return p;
  // a GEMM stage is cut into column blocks of 8 x (workgroups of the grid) columns: the table's length depends on the grid
  const int ns = count_stages(m, sh, Bchunk, XF_WALK_SMALL, dev.grid);
  if (ns > kWalkMaxOps) return p;
  p.form = XF_WALK_SMALL; p.rows = kWalkSmallRows; p.lds_bytes = lds_small; p.n_stages = ns;
  return p;
}

// ---- what xf_gemm launches (xformer.hip takes its decision from here) ------------------------------------------------------------------
// Two forms (same-box kbench, profiles/README.md): up to 47 rows the 16-column form (every wave streams its own K slice, X straight from
// L2: 1.6-3.1 TB/s at 6 rows) is ahead; from 48 rows on X re-reads bound it and the column-block form (X shared through LDS) wins: 71 vs
// 53 TFLOP/s at 168 x 6144 x 2048.  The column-block form needs one whole 32-wide K step (its masked W loads read row offset 0).
XfGemmPath xf_gemm_describe(int M, int N, int K) {
  XfGemmPath p;
  const int mt = cdiv(M, 16);
  p.mt = mt <= 4 ? mt : (mt <= 6 ? 6 : (mt <= 8 ? 8 : (mt <= 11 ? 11 : (mt <= 16 ? 16 : 21))));
  const int steps = cdiv(K, 32);
  p.ksplit = 1;
  if (M >= 48 && K >= 32) {
    p.form = 2;
    const int nb = cdiv(N, 64);
    // enough workgroups for two per CU while each keeps >= 8 steps (two rounds of its 4-deep pipeline)
    while (nb * p.ksplit < 512 && steps / (p.ksplit * 2) >= 8 && p.ksplit < 16) p.ksplit *= 2;
  } else {
    p.form = 1;
    const int nb = cdiv(N, 16);
    // K split: enough workgroups to put >= 2 on every CU while every wave (of 8) keeps >= 2 steps of 32 (its load pipeline)
    while (nb * p.ksplit < 512 && steps / (8 * p.ksplit * 2) >= 2 && p.ksplit < 8) p.ksplit *= 2;
  }
  return p;
}
