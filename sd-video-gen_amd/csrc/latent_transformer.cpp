// Latent-sequence Transformer graph (reference: models/transformer.py:47-68 over torch.nn.Transformer
// defaults — post-norm, ReLU, final encoder/decoder LayerNorm, sequence-first).  f32 throughout.
#include "xf_plan.h"
#include "../../include/svg_hip.h"

void XfModel::configure(const char* kv) {
  auto m = parse_kv(kv);
  auto geti = [&](const char* k, int& dst) { if (m.count(k)) dst = (int)m[k][0]; };
  // a configure call describes the whole model: keys it leaves out go back to their defaults (a context that held a
  // text-conditioned model must not keep its text_dim for the next, plain one)
  d_lat = 0; d_model = 0; heads = 8; enc_layers = 0; dec_layers = 0; ffn = 2048; text_dim = 0;
  geti("d_lat", d_lat); geti("d_model", d_model); geti("heads", heads);
  geti("enc_layers", enc_layers); geti("dec_layers", dec_layers); geti("ffn", ffn); geti("text_dim", text_dim);
  ready = false;
}

void XfModel::finalize(svg_ctx* ctx, int64_t* n_params) {
  SVG_CHECK(d_lat > 0 && d_model > 0 && heads > 0, "transformer: configure d_lat/d_model/heads first");
  SVG_CHECK(d_model % heads == 0 && d_model % 16 == 0 && d_lat % 16 == 0 && ffn % 16 == 0,
            "transformer: d_model %d / d_lat %d / ffn %d must be multiples of 16 (and d_model of heads)", d_model, d_lat, ffn);
  const int64_t d = d_model;
  SVG_CHECK(text_dim >= 0 && text_dim < d_model, "transformer: text_dim %d out of range", text_dim);
  each_param(w, [&](const std::string& name, std::initializer_list<int64_t> shape, const float*& slot) { slot = ws.get(name, shape).f32; });
  // positional table (models/positional_encoding.py:16-30): use the state_dict buffer when it was handed
  // over, else build it — sin/cos in double, rounded to f32.
  if (!pe || pe_d != d) { pe = (float*)ctx->dalloc(64 * d * sizeof(float)); pe_d = (int)d; }
  if (ws.has("positional_encoder.pos_encoding")) {
    const Weight& t = ws.get("positional_encoder.pos_encoding");
    SVG_CHECK(t.numel == 64 * d, "positional_encoder.pos_encoding has %lld elements", (long long)t.numel);
    HIP_OK(hipMemcpy(pe, t.f32, 64 * d * sizeof(float), hipMemcpyDeviceToDevice));
  } else {
    std::vector<float> h(64 * d);
    for (int pos = 0; pos < 64; ++pos)
      for (int i = 0; i < d; i += 2) {
        float div = expf((float)i * (-logf(10000.0f)) / (float)d);
        h[pos * d + i] = sinf((float)pos * div);
        if (i + 1 < d) h[pos * d + i + 1] = cosf((float)pos * div);
      }
    HIP_OK(hipMemcpy(pe, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (!iota) {
    iota = (int32_t*)ctx->dalloc(64 * sizeof(int32_t));
    int32_t h[64];
    for (int i = 0; i < 64; ++i) h[i] = i;
    HIP_OK(hipMemcpy(iota, h, sizeof(h), hipMemcpyHostToDevice));
  }
  int64_t n = 0;
  for (auto& kv : ws.map)
    if (kv.first != "positional_encoder.pos_encoding") n += kv.second.numel;
  if (n_params) *n_params = n;
  ready = true;
}

namespace {
// the per-GEMM kernels (xformer.hip) as the operations of xf_graph()
struct XfRun {
  static constexpr bool kSharesEmbedding = true;   // src == tgt: one embedding serves both stacks
  svg_ctx* ctx; const XfModel* m; hipStream_t s; const XfChunk& c;
  const XfModel::LayerW& layer(bool dec, int i) const { return dec ? m->w.dec[i] : m->w.enc[i]; }
  float* gemm(const float* X, const float* w, const float* b, int M, int N, int K, int relu_in = 0) {
    float* Y = ctx->arena.get<float>((int64_t)M * N);
    xf_gemm(ctx, X, w, b, Y, M, N, K, relu_in, s);
    return Y;
  }
  float* ln(const float* x, const float* r, const float* g, const float* b, int M) {
    float* y = ctx->arena.get<float>((int64_t)M * m->d_model);
    if (SVG_LAUNCHING(ctx)) {
      ProfScope ps(ctx, PK_XF_MISC, s, 0, 12.0 * M * m->d_model);
      xf_add_ln(x, r, g, b, y, M, m->d_model, 1e-5f, s);
    }
    return y;
  }
  float* add_ln(const XfModel::LayerW& L, int k, const float* x, const float* r, int M) { return ln(x, r, L.n_w[k], L.n_b[k], M); }
  float* final_ln(bool dec, const float* x, int M) { return dec ? ln(x, nullptr, m->w.decn_w, m->w.decn_b, M) : ln(x, nullptr, m->w.encn_w, m->w.encn_b, M); }
  float* mha(const XfModel::LayerW& L, bool cross, const float* xq, int Tq, const float* xkv, int Tk, const float* mask, const float* kpad) {
    const int d = m->d_model, hd = d / m->heads, B = c.B;
    float* o = ctx->arena.get<float>((int64_t)Tq * B * d);
    if (!cross) {
      float* qkv = gemm(xq, L.in_w, L.in_b, Tq * B, 3 * d, d);
      if (SVG_LAUNCHING(ctx)) {
        ProfScope ps(ctx, PK_XF_MISC, s, 0, 0);
        xf_attention(qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, mask, o, Tq, Tk, B, m->heads, hd, s, kpad);
      }
      return gemm(o, L.out_w, L.out_b, Tq * B, d, d);
    }
    float* q = gemm(xq, L.cin_w, L.cin_b, Tq * B, d, d);
    float* kv = gemm(xkv, L.cin_w + (int64_t)d * d, L.cin_b + d, Tk * B, 2 * d, d);
    if (SVG_LAUNCHING(ctx)) {
      ProfScope ps(ctx, PK_XF_MISC, s, 0, 0);
      xf_attention(q, d, kv, kv + d, 2 * d, mask, o, Tq, Tk, B, m->heads, hd, s);
    }
    return gemm(o, L.cout_w, L.cout_b, Tq * B, d, d);
  }
  float* ffn(const XfModel::LayerW& L, const float* x, int M) {
    float* h = gemm(x, L.l1_w, L.l1_b, M, m->ffn, m->d_model);
    return gemm(h, L.l2_w, L.l2_b, M, m->d_model, m->ffn, /*relu_in=*/1);
  }
  float* embed(int, const float* x, int T) {
    const int d = m->d_model, d_img = d - m->text_dim, B = c.B;
    float* e = gemm(x, m->w.emb_w, m->w.emb_b, B * T, d_img, m->d_lat);
    float* y = ctx->arena.get<float>((int64_t)B * T * d);
    if (SVG_LAUNCHING(ctx)) {
      ProfScope ps(ctx, PK_XF_MISC, s, 0, 8.0 * B * T * d);
      xf_embed_post(e, m->pe, c.pe_row, c.text, m->text_dim, y, B, T, d, sqrtf((float)d), s);
    }
    return y;
  }
  float* out(const float* x, int M) {
    xf_gemm(ctx, x, m->w.out_w, m->w.out_b, c.out, M, m->d_lat, m->d_model, 0, s);
    return c.out;
  }
};
}  // namespace

void XfModel::forward(svg_ctx* ctx, const float* src, const float* tgt, int B, int Ts, int Tt, const float* mask,
                      const int32_t* pe_row, float* out, hipStream_t s, const float* text, const float* src_pad, const float* tgt_pad) {
  SVG_CHECK(ready, "transformer: svg_finalize has not been called");
  SVG_CHECK((text_dim > 0) == (text != nullptr), "transformer: the text-conditioned variant needs (and only it takes) a text embedding");
  SVG_CHECK(B >= 1 && Ts >= 1 && Tt >= 1 && Ts <= 32 && Tt <= 32, "transformer: B=%d Ts=%d Tt=%d unsupported (sequences up to 32 tokens)", B, Ts, Tt);
  SVG_CHECK(pe_row || B <= 64, "transformer: batch %d > max_len 64 of the positional table", B);
  // which form runs, and in chunks of how many batch rows: decided once, in xf_plan.cpp, from the facts of this device and the knobs
  // (both established at svg_create / svg_env_refresh, not looked up per forward)
  const XfDevice dev{xf_walk_enabled(s), xf_walk_grid(), kWalkMaxLds};
  const XfPlan p = xf_plan(*this, XfShape{B, Ts, Tt, text != nullptr, tgt == src}, dev,
                           XfKnobs{svg_env_i64("SVG_XF_WALK_ROWS", 96), svg_env_i64("SVG_XF_WALK_SPLIT", 0), svg_env_i64("SVG_XF_WALK_SMALL", -1)});
  // One chunk of batch rows.  Per-GEMM: B*max(Ts,Tt) <= 336, the rows one pass of the weight stream serves.  The walks: allocate the
  // workspace (also on the dry pass), build the stage table, account it as the per-GEMM kernels would, launch once.
  auto chunk = [&](const XfChunk& c) {
    if (p.form == XF_PER_GEMM) {
      XfRun r{ctx, this, s, c};
      xf_graph(r, *this, c);
      return;
    }
    const XfWalkWs wk = xf_walk_workspace(*this, c, p.form, [](void* u, int64_t n) { return ((svg_ctx*)u)->arena.get<float>(n); }, ctx);
    if (!SVG_LAUNCHING(ctx)) return;
    const bool small = p.form == XF_WALK_SMALL;
    std::vector<WalkOp> ops;
    ops.reserve(160);
    if (small) xf_walk_small_table(*this, c, wk, dev.grid, ops);
    else xf_walk_table(*this, c, wk, ops);
    double flops, bytes;
    xf_walk_account(ops, &flops, &bytes);
    ProfScope ps(ctx, PK_XF_GEMM, s, flops, bytes, small ? "walk_small" : "walk");
    const int T = std::max(Ts, Tt), hd = d_model / heads;
    if (small) xf_walk_small_launch(ctx, ops.data(), (int)ops.size(), xf_walk_small_lds_bytes(T, hd), s);
    else xf_walk_launch(ctx, ops.data(), (int)ops.size(), c.B * T, xf_walk_lds_bytes(c.B * T, T, T, hd), s);
  };
  run_planned(ctx, [&]() {
    // PE rows: the reference indexes the table by batch row (positional_encoding.py:33-35)
    const int32_t* rows = iota;
    if (pe_row) {
      int32_t* r = ctx->arena.get<int32_t>(B);
      if (SVG_LAUNCHING(ctx)) HIP_OK(hipMemcpyAsync(r, pe_row, B * sizeof(int32_t), hipMemcpyDefault, s));
      rows = r;
    }
    if (B <= p.Bc) {
      chunk(XfChunk{B, Ts, Tt, src, tgt, mask, text, src_pad, tgt_pad, rows, out});
    } else {
      for (int b0 = 0; b0 < B; b0 += p.Bc) {
        const int bc = std::min(p.Bc, B - b0);
        ctx->arena.push();
        float* tmp = ctx->arena.get<float>((int64_t)Tt * bc * d_lat);
        const float* srcc = src + (int64_t)b0 * Ts * d_lat;
        const float* tgtc = (tgt == src) ? srcc : tgt + (int64_t)b0 * Tt * d_lat;
        chunk(XfChunk{bc, Ts, Tt, srcc, tgtc, mask, text ? text + (int64_t)b0 * text_dim : nullptr, src_pad ? src_pad + (int64_t)b0 * Ts : nullptr,
                      tgt_pad ? tgt_pad + (int64_t)b0 * Tt : nullptr, rows + b0, tmp});
        if (SVG_LAUNCHING(ctx))
          HIP_OK(hipMemcpy2DAsync(out + (int64_t)b0 * d_lat, (size_t)B * d_lat * sizeof(float), tmp,
                                  (size_t)bc * d_lat * sizeof(float), (size_t)bc * d_lat * sizeof(float), Tt,
                                  hipMemcpyDeviceToDevice, s));
        ctx->arena.pop();
      }
    }
  });
}

extern "C" int svg_transformer_forward_text(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                            const float* mask, const int32_t* pe_row, float* out, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "transformer: model not configured");
    xf_walk_check(ctx);
    ctx->xf()->forward(ctx, src, tgt, B, Ts, Tt, mask, pe_row, out, (hipStream_t)stream, text);
  });
}

extern "C" int svg_transformer_forward_padded(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                              const float* mask, const float* src_pad, const float* tgt_pad, const int32_t* pe_row, float* out,
                                              void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "transformer: model not configured");
    xf_walk_check(ctx);
    ctx->xf()->forward(ctx, src, tgt, B, Ts, Tt, mask, pe_row, out, (hipStream_t)stream, text, src_pad, tgt_pad);
  });
}

extern "C" int svg_transformer_forward(svg_ctx* ctx, const float* src, const float* tgt, int B, int Ts, int Tt, const float* mask,
                                       const int32_t* pe_row, float* out, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "transformer: model not configured");
    xf_walk_check(ctx);
    ctx->xf()->forward(ctx, src, tgt, B, Ts, Tt, mask, pe_row, out, (hipStream_t)stream);
  });
}
