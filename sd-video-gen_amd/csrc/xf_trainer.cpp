// Training step of the latent Transformer: forward in train mode keeping what backward needs, the criterion, backward through
// every layer, Adam.  Reference: trainers/trainer.py:111-190 (train_loop body: pred = model(new_batch, y_input, tgt_mask);
// loss_fn(pred[-F:], y_expected[-F:]); opt.zero_grad(); loss.backward(); opt.step()), :65-109 (criterion), :192-260
// (validation_loop: the same loss in eval mode) over torch.nn.Transformer (post-norm, ReLU, dropout after the positional
// encoding, on the attention probabilities, after each sublayer and inside the feed-forward) and torch.optim.Adam(lr).
// The Stable Diffusion side stays frozen (encode_batch is the VAE encoder the sampling path already has).
#include "xf_plan.h"
#include "../../include/svg_hip.h"
#include <cmath>
#include <cstring>
#include <cstdlib>

struct XfTrain {
  struct Slot { float* g = nullptr; float* m = nullptr; float* v = nullptr; float* e = nullptr; int64_t n = 0; };
  std::unordered_map<std::string, Slot> slots;   // by state_dict name: svg_transformer_tensor / svg_transformer_set_tensor only
  std::vector<std::string> names;                 // the tensors of d_tens, in its order
  XfTable<float*> g;                              // Slot::g by role: what backward writes through
  XfAdamTensor* d_tens = nullptr;
  XfAdamChunk* d_chunks = nullptr;
  int n_chunks = 0;
  int step = 0;
  float** d_ema = nullptr;       // [tensors] Slot::e in the order of d_tens: the averaged weights (nullptr until first asked for)
  float ema_decay = 0.f;         // > 0: every optimizer step also updates them
  bool has_grads = false;        // a backward pass has been enqueued since the state was created
  double* d_norm_part = nullptr; // [n_chunks] per-chunk sums of squares of the gradient-norm pass
  double* d_norm = nullptr;      // the global gradient 2-norm, where the clipped update reads it
  double* h_norm = nullptr;      // pinned mirror
  float* d_losses = nullptr;     // [5]
  float* h_losses = nullptr;     // pinned mirror: a device-to-pageable copy goes through the runtime's staging path and its host thread
  // One plan per call signature (shapes + every criterion / dropout parameter except the seed): the workspace high-water mark and,
  // for the loss (+ backward) calls, the captured hipGraph of the whole step.  ~540 launches per step cost more host time than
  // the GPU needs to run them (15.3 ms wall against 9.3 ms of kernels); the graph replays them from fixed staging buffers.
  struct Plan {
    svg_train_cfg cfg{}; int B = 0, Ts = 0, Tt = 0, backward = 0, mode = 0; bool has_mask = false, has_text = false;
    int64_t high = 0;
    hipGraphExec_t exec = nullptr;
    char* arena_base = nullptr;
    float *src = nullptr, *tgt = nullptr, *exp = nullptr, *text = nullptr, *mask = nullptr;
  };
  std::vector<Plan> plans;
  uint64_t* d_seed = nullptr;     // device seed word read by every dropout site
  uint64_t* h_seed = nullptr;     // pinned ring of 16 seeds (a call that does not synchronise must not race the next one's seed)
  hipEvent_t seed_ev[16] = {};    // recorded behind each slot's upload: the 17th unsynchronised call waits for the 1st one's copy
  int seed_slot = 0;
  // The training step's own workspace.  The captured graph bakes workspace addresses: if it lived in the context-wide arena, a
  // VAE / UNet / CLIP call of the same context on ANOTHER stream (or a forward that regrows the arena) could reuse or move the
  // memory while the graph is still running.  loss_pass swaps these in for the duration of its planning and launches.
  Arena ws;
  DevBuf ws_buf;
  std::vector<void*> bufs;       // device allocations of the training state (freed with it)
  void* dalloc(int64_t bytes) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, (size_t)std::max<int64_t>(bytes, 256)));
    bufs.push_back(p);
    return p;
  }
  ~XfTrain() {
    for (auto& pl : plans) if (pl.exec) hipGraphExecDestroy(pl.exec);
    for (void* p : bufs) hipFree(p);
    if (h_losses) hipHostFree(h_losses);
    if (h_seed) hipHostFree(h_seed);
    if (h_norm) hipHostFree(h_norm);
    for (auto e : seed_ev) if (e) hipEventDestroy(e);
    if (ws_buf.p) hipFree(ws_buf.p);
  }
};

namespace {

constexpr int kAdamChunk = 1 << 16;

// what a forward operation leaves for its backward: activations, and the parameters (w) with where their gradients go (gw, gb)
struct LinTape { const float* x = nullptr; int M = 0, N = 0, K = 0; const float* w = nullptr; float* gw = nullptr; float* gb = nullptr; };
struct LnTape { float* xhat = nullptr; float* rstd = nullptr; const float* w = nullptr; float* gw = nullptr; float* gb = nullptr; XfDrop dr{nullptr, 0, 0.f}; int M = 0; };
struct MhaTape {
  LinTape in_q, in_kv, outp;   // self: in_q is the whole packed projection
  float *qkv = nullptr, *q = nullptr, *kv = nullptr, *P = nullptr;
  const float* mask = nullptr;
  int Tq = 0, Tk = 0;
  bool self = true;
  XfDrop dr{nullptr, 0, 0.f};
};
struct FfnTape { LinTape l1, l2; float* r = nullptr; float gate_scale = 1.f; };
struct LayerTape { MhaTape sa, ca; FfnTape ff; LnTape n[3]; };     // an encoder layer leaves ca and n[2] unused

// the training kernels (xf_train.hip) as the operations of xf_graph(), and their backward counterparts
struct Run {
  static constexpr bool kSharesEmbedding = false;   // each embedding draws its own dropout mask
  svg_ctx* ctx; XfModel* m; XfTrain* tr; hipStream_t s; int B; const uint64_t* seed; float p; bool grads;
  bool acc;      // SVG_BACKWARD_ACCUMULATE: every gradient store adds to its slot
  const float* text = nullptr;
  uint32_t site = 0;
  std::vector<LayerTape> enc, dec;
  LinTape e_lin[2], l_out;
  XfDrop e_drop[2];
  LnTape n_enc, n_dec;
  struct Layer { const XfModel::LayerW& w; const XfTable<float*>::Layer& g; LayerTape& t; };
  Layer layer(bool d, int i) { return d ? Layer{m->w.dec[i], tr->g.dec[i], dec[i]} : Layer{m->w.enc[i], tr->g.enc[i], enc[i]}; }
  bool go() const { return SVG_LAUNCHING(ctx); }
  XfDrop drop() { return XfDrop{seed, site++, p}; }
  template <typename T> T* get(int64_t n) { return ctx->arena.get<T>(n); }

  // ---- linear ------------------------------------------------------------------------------------------------------------
  float* lin(LinTape& t, const float* x, const float* w, const float* b, float* gw, float* gb, int M, int N, int K) {
    t = LinTape{x, M, N, K, w, gw, gb};
    float* y = get<float>((int64_t)M * N);
    for (int m0 = 0; m0 < M; m0 += 336)       // xf_gemm streams W once per 336 rows (it plans its own split-K slabs in the dry pass)
      xf_gemm(ctx, x + (int64_t)m0 * K, w, b, y + (int64_t)m0 * N, std::min(336, M - m0), N, K, 0, s);
    return y;
  }
  // dW, db of the layer; dx = gate(dy W) + add (dx == nullptr: not wanted)
  void lin_bwd(const LinTape& t, const float* dy, float* dx, const float* add = nullptr, const float* gate = nullptr, float gate_scale = 1.f,
               bool accumulate = false) {
    float* slabs = dx ? get<float>(xf_gemm_nn_slab_floats(t.M, t.N, t.K)) : nullptr;
    if (!go()) return;
    // (dW on a side stream beside the dX chain — a fork / join per linear layer inside the captured step — was bit-equal and 6-9 %
    // slower per step; removed, DESIGN.md "Training")
    xf_gemm_tn(dy, t.N, t.x, t.K, t.gw, t.gb, t.M, t.N, t.K, accumulate || acc, s);
    if (dx) xf_gemm_nn(dy, t.N, t.w, slabs, dx, t.M, t.N, t.K, gate, gate_scale, add, s);
  }

  // ---- add + LayerNorm --------------------------------------------------------------------------------------------------
  float* ln(LnTape& t, const float* x, const float* r, const float* w, const float* b, float* gw, float* gb, int M, bool drop_r) {
    const int d = m->d_model;
    t.w = w; t.gw = gw; t.gb = gb; t.M = M;
    t.dr = drop_r ? drop() : XfDrop{seed, 0, 0.f};
    t.xhat = get<float>((int64_t)M * d);
    t.rstd = get<float>(M);
    float* y = get<float>((int64_t)M * d);
    if (go()) xf_add_ln_train(x, r, t.dr, w, b, y, t.xhat, t.rstd, M, d, 1e-5f, s);
    return y;
  }
  float* add_ln(const Layer& L, int k, const float* x, const float* r, int M) { return ln(L.t.n[k], x, r, L.w.n_w[k], L.w.n_b[k], L.g.n_w[k], L.g.n_b[k], M, true); }
  float* final_ln(bool d, const float* x, int M) {
    return d ? ln(n_dec, x, nullptr, m->w.decn_w, m->w.decn_b, tr->g.decn_w, tr->g.decn_b, M, false)
             : ln(n_enc, x, nullptr, m->w.encn_w, m->w.encn_b, tr->g.encn_w, tr->g.encn_b, M, false);
  }
  // returns dz (gradient of both the residual input and, masked in *dz_drop, of the sublayer output)
  float* add_ln_bwd(const LnTape& t, const float* dy, float** dz_drop) {
    const int d = m->d_model;
    float* dz = get<float>((int64_t)t.M * d);
    float* dzd = nullptr;
    if (dz_drop) { dzd = t.dr.p > 0.f ? get<float>((int64_t)t.M * d) : dz; *dz_drop = dzd; }
    if (go()) xf_ln_bwd(dy, t.xhat, t.rstd, t.w, dz, dzd == dz ? nullptr : dzd, t.dr, t.gw, t.gb, t.M, d, acc, s);
    return dz;
  }

  // ---- multi-head attention (training takes no key-padding bias) ------------------------------------------------------------
  float* mha(const Layer& L, bool cross, const float* xq, int Tq, const float* xkv, int Tk, const float* mask, const float*) {
    const int d = m->d_model, hd = d / m->heads;
    MhaTape& t = cross ? L.t.ca : L.t.sa;
    t.Tq = Tq; t.Tk = Tk; t.self = !cross; t.mask = mask;
    float* o = get<float>((int64_t)Tq * B * d);
    t.P = get<float>((int64_t)B * m->heads * Tq * Tk);
    if (!cross) {
      t.qkv = lin(t.in_q, xq, L.w.in_w, L.w.in_b, L.g.in_w, L.g.in_b, Tq * B, 3 * d, d);
      t.dr = drop();
      if (go()) xf_attention_train(t.qkv, 3 * d, t.qkv + d, t.qkv + 2 * d, 3 * d, mask, o, t.P, Tq, Tk, B, m->heads, hd, t.dr, s);
      return lin(t.outp, o, L.w.out_w, L.w.out_b, L.g.out_w, L.g.out_b, Tq * B, d, d);
    }
    const int64_t dd = (int64_t)d * d;
    t.q = lin(t.in_q, xq, L.w.cin_w, L.w.cin_b, L.g.cin_w, L.g.cin_b, Tq * B, d, d);
    t.kv = lin(t.in_kv, xkv, L.w.cin_w + dd, L.w.cin_b + d, L.g.cin_w + dd, L.g.cin_b + d, Tk * B, 2 * d, d);
    t.dr = drop();
    if (go()) xf_attention_train(t.q, d, t.kv, t.kv + d, 2 * d, mask, o, t.P, Tq, Tk, B, m->heads, hd, t.dr, s);
    return lin(t.outp, o, L.w.cout_w, L.w.cout_b, L.g.cout_w, L.g.cout_b, Tq * B, d, d);
  }
  // da: gradient of the block output.  dxq = ... + add_q; self: the k/v gradients flow into the same dxq; cross: dmem (+)= ...
  void mha_bwd(const MhaTape& t, const float* da, float* dxq, const float* add_q, float* dmem, bool dmem_accumulate) {
    const int d = m->d_model, hd = d / m->heads;
    float* d_o = get<float>((int64_t)t.Tq * B * d);
    lin_bwd(t.outp, da, d_o);
    if (t.self) {
      float* dqkv = get<float>((int64_t)t.Tq * B * 3 * d);
      if (go())
        xf_attention_bwd(d_o, t.qkv, 3 * d, t.qkv + d, t.qkv + 2 * d, 3 * d, t.P, dqkv, 3 * d, dqkv + d, dqkv + 2 * d, 3 * d, t.Tq, t.Tk, B,
                         m->heads, hd, t.dr, s);
      lin_bwd(t.in_q, dqkv, dxq, add_q);
    } else {
      float* dq = get<float>((int64_t)t.Tq * B * d);
      float* dkv = get<float>((int64_t)t.Tk * B * 2 * d);
      if (go())
        xf_attention_bwd(d_o, t.q, d, t.kv, t.kv + d, 2 * d, t.P, dq, d, dkv, dkv + d, 2 * d, t.Tq, t.Tk, B, m->heads, hd, t.dr, s);
      lin_bwd(t.in_q, dq, dxq, add_q);
      lin_bwd(t.in_kv, dkv, dmem, dmem_accumulate ? dmem : nullptr);
    }
  }

  // ---- feed-forward: linear2(dropout(relu(linear1(x)))) ---------------------------------------------------------------------
  float* ffn(const Layer& L, const float* x, int M) {
    FfnTape& t = L.t.ff;
    float* h = lin(t.l1, x, L.w.l1_w, L.w.l1_b, L.g.l1_w, L.g.l1_b, M, m->ffn, m->d_model);
    t.r = get<float>((int64_t)M * m->ffn);
    const XfDrop dr = drop();
    t.gate_scale = dr.p > 0.f ? 1.f / (1.f - dr.p) : 1.f;
    if (go()) xf_relu_drop(h, t.r, (int64_t)M * m->ffn, dr, s);
    return lin(t.l2, t.r, L.w.l2_w, L.w.l2_b, L.g.l2_w, L.g.l2_b, M, m->d_model, m->ffn);
  }
  void ffn_bwd(const FfnTape& t, const float* df, float* dx, const float* add) {
    float* dh = get<float>((int64_t)t.l1.M * m->ffn);
    lin_bwd(t.l2, df, dh, nullptr, t.r, t.gate_scale);        // r > 0 exactly where ReLU and the dropout let the gradient through
    lin_bwd(t.l1, dh, dx, add);
  }

  // ---- embedding + positional encoding (which: 0 source, 1 target) ----------------------------------------------------------
  float* embed(int which, const float* x, int T) {
    const int d = m->d_model, d_img = d - m->text_dim;
    float* e = lin(e_lin[which], x, m->w.emb_w, m->w.emb_b, tr->g.emb_w, tr->g.emb_b, B * T, d_img, m->d_lat);
    float* y = get<float>((int64_t)B * T * d);
    e_drop[which] = drop();
    if (go()) xf_embed_post_train(e, m->pe, m->iota, text, m->text_dim, y, B, T, d, sqrtf((float)d), e_drop[which], s);
    return y;
  }
  void embed_bwd(int which, const float* dy, int T, bool accumulate) {
    const int d = m->d_model, d_img = d - m->text_dim;
    float* de = get<float>((int64_t)B * T * d_img);
    if (go()) xf_embed_post_bwd(dy, de, B, T, d, d_img, sqrtf((float)d), e_drop[which], s);
    lin_bwd(e_lin[which], de, nullptr, nullptr, nullptr, 1.f, accumulate);
  }
  float* out(const float* x, int M) { return lin(l_out, x, m->w.out_w, m->w.out_b, tr->g.out_w, tr->g.out_b, M, m->d_lat, m->d_model); }
};

void ensure_train(svg_ctx* ctx, XfModel* m) {
  if (m->train) return;
  SVG_CHECK(m->ready, "transformer: svg_finalize has not been called");
  std::unique_ptr<XfTrain> tr(new XfTrain());
  std::vector<XfAdamTensor> tens;
  std::vector<XfAdamChunk> chunks;
  std::vector<std::string> names;
  for (auto& kv : m->ws.map)
    if (kv.first != "positional_encoder.pos_encoding") names.push_back(kv.first);
  std::sort(names.begin(), names.end());
  for (auto& n : names) {
    const Weight& w = m->ws.get(n);
    XfTrain::Slot sl;
    sl.n = w.numel;
    sl.g = (float*)tr->dalloc(3 * w.numel * sizeof(float));
    sl.m = sl.g + w.numel; sl.v = sl.m + w.numel;
    HIP_OK(hipMemset(sl.g, 0, 3 * w.numel * sizeof(float)));
    tr->slots[n] = sl;
    const int ti = (int)tens.size();
    tens.push_back(XfAdamTensor{w.f32, sl.g, sl.m, sl.v});
    for (int64_t off = 0; off < w.numel; off += kAdamChunk)
      chunks.push_back(XfAdamChunk{ti, (int32_t)std::min<int64_t>(kAdamChunk, w.numel - off), off});
  }
  tr->d_tens = (XfAdamTensor*)tr->dalloc(tens.size() * sizeof(XfAdamTensor));
  tr->d_chunks = (XfAdamChunk*)tr->dalloc(chunks.size() * sizeof(XfAdamChunk));
  tr->d_losses = (float*)tr->dalloc(5 * sizeof(float));
  tr->d_norm_part = (double*)tr->dalloc(chunks.size() * sizeof(double));
  tr->d_norm = (double*)tr->dalloc(sizeof(double));
  HIP_OK(hipHostMalloc((void**)&tr->h_norm, sizeof(double), hipHostMallocDefault));
  HIP_OK(hipHostMalloc((void**)&tr->h_losses, 5 * sizeof(float), hipHostMallocDefault));
  tr->d_seed = (uint64_t*)tr->dalloc(sizeof(uint64_t));
  HIP_OK(hipHostMalloc((void**)&tr->h_seed, 16 * sizeof(uint64_t), hipHostMallocDefault));
  HIP_OK(hipMemcpy(tr->d_tens, tens.data(), tens.size() * sizeof(XfAdamTensor), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(tr->d_chunks, chunks.data(), chunks.size() * sizeof(XfAdamChunk), hipMemcpyHostToDevice));
  tr->n_chunks = (int)chunks.size();
  tr->names = names;
  m->each_param(tr->g, [&](const std::string& name, std::initializer_list<int64_t>, float*& slot) { slot = tr->slots.at(name).g; });
  m->train = tr.release();
}

// expected == nullptr: forward only (train-mode dropout when backward != 0), the prediction (Tt,B,D_lat) goes to pred_out
void loss_pass(svg_ctx* ctx, XfModel* m, const svg_train_cfg& cfg, const float* src, const float* tgt, const float* expected, const float* text,
               int B, int Ts, int Tt, const float* mask, int backward, float* losses_host, hipStream_t s, float* pred_out = nullptr) {
  SVG_CHECK(m->ready, "transformer: svg_finalize has not been called");
  SVG_CHECK((m->text_dim > 0) == (text != nullptr), "transformer: the text-conditioned variant needs (and only it takes) a text embedding");
  SVG_CHECK(B >= 1 && B <= 64 && Ts >= 1 && Tt >= 1 && Ts <= 32 && Tt <= 32, "transformer training: B=%d Ts=%d Tt=%d unsupported (B <= 64, T <= 32)", B, Ts, Tt);
  SVG_CHECK(cfg.dropout_p >= 0.f && cfg.dropout_p < 1.f, "dropout_p %g out of range", cfg.dropout_p);
  if (expected) {
    SVG_CHECK(cfg.frames_to_predict >= 1 && cfg.frames_to_predict <= Tt, "frames_to_predict %d out of range 1..%d", cfg.frames_to_predict, Tt);
    SVG_CHECK(cfg.feat_h > 0 && cfg.feat_w > 0 && 4 * cfg.feat_h * cfg.feat_w == m->d_lat, "criterion: D_lat %d is not 4 x %d x %d", m->d_lat,
              cfg.feat_h, cfg.feat_w);
    SVG_CHECK(cfg.w_contrastive == 0.f || (cfg.temperature > 0.f && cfg.feat_h * cfg.feat_w <= 4096), "contrastive loss: bad temperature / patch count");
  }
  ensure_train(ctx, m);
  XfTrain* tr = m->train;
  if (expected && backward) tr->has_grads = true;
  const int d = m->d_model, Ms = Ts * B, Mt = Tt * B;
  auto body = [&](const float* src, const float* tgt, const float* expected, const float* text, const float* mask) {
    Run r{ctx, m, tr, s, B, tr->d_seed, backward ? cfg.dropout_p : 0.f, backward != 0, backward == SVG_BACKWARD_ACCUMULATE};
    r.text = text;
    r.enc.resize(m->enc_layers); r.dec.resize(m->dec_layers);
    float* pred = xf_graph(r, *m, XfChunk{B, Ts, Tt, src, tgt, mask, text, nullptr, nullptr, m->iota, nullptr});
    if (!expected) {                                           // forward only
      if (r.go()) HIP_OK(hipMemcpyAsync(pred_out, pred, (size_t)Mt * m->d_lat * sizeof(float), hipMemcpyDeviceToDevice, s));
      return;
    }

    // criterion on the last frames_to_predict positions (trainer.py:145)
    float* dpred = r.get<float>((int64_t)Mt * m->d_lat);
    float* part = r.get<float>((int64_t)Mt * 3);
    float* part2 = r.get<float>(Mt);
    if (r.go())
      xf_criterion(pred, expected, dpred, part, part2, tr->d_losses, Tt, B, m->d_lat, Tt - cfg.frames_to_predict, cfg.feat_h, cfg.feat_w, cfg.w_mse,
                   cfg.w_l1, cfg.w_gdl, cfg.gdl_alpha, cfg.w_contrastive, cfg.temperature, s);
    if (!backward) return;

    // ---- backward ----------------------------------------------------------------------------------------------------------
    float* dx = r.get<float>((int64_t)Mt * d);
    r.lin_bwd(r.l_out, dpred, dx);
    float* dxt = r.add_ln_bwd(r.n_dec, dx, nullptr);
    float* dmem = r.get<float>((int64_t)Ms * d);
    bool dmem_set = false;
    for (int i = m->dec_layers - 1; i >= 0; --i) {
      LayerTape& t = r.dec[i];
      float *dzd = nullptr, *dz;
      dz = r.add_ln_bwd(t.n[2], dxt, &dzd);                     // x2 + dropout(ff(x2))
      float* dx2 = r.get<float>((int64_t)Mt * d);
      r.ffn_bwd(t.ff, dzd, dx2, dz);
      dz = r.add_ln_bwd(t.n[1], dx2, &dzd);                     // x1 + dropout(cross(x1, mem))
      float* dx1 = r.get<float>((int64_t)Mt * d);
      r.mha_bwd(t.ca, dzd, dx1, dz, dmem, dmem_set);
      dmem_set = true;
      dz = r.add_ln_bwd(t.n[0], dx1, &dzd);                     // x + dropout(self(x))
      float* dx0 = r.get<float>((int64_t)Mt * d);
      r.mha_bwd(t.sa, dzd, dx0, dz, nullptr, false);
      dxt = dx0;
    }
    if (!dmem_set && r.go()) SDNS::fill_f32(dmem, (int64_t)Ms * d, 0.f, s);
    float* dxs = r.add_ln_bwd(r.n_enc, dmem, nullptr);
    for (int i = m->enc_layers - 1; i >= 0; --i) {
      LayerTape& t = r.enc[i];
      float *dzd = nullptr, *dz;
      dz = r.add_ln_bwd(t.n[1], dxs, &dzd);
      float* dx1 = r.get<float>((int64_t)Ms * d);
      r.ffn_bwd(t.ff, dzd, dx1, dz);
      dz = r.add_ln_bwd(t.n[0], dx1, &dzd);
      float* dx0 = r.get<float>((int64_t)Ms * d);
      r.mha_bwd(t.sa, dzd, dx0, dz, nullptr, false);
      dxs = dx0;
    }
    r.embed_bwd(0, dxs, Ts, false);
    r.embed_bwd(1, dxt, Tt, true);                // the embedding layer is shared: second contribution accumulates
  };
  // ---- the plan of this call signature ----------------------------------------------------------------------------------------
  struct ArenaSwap {       // the training workspace stands in for the context arena until this call returns (or throws)
    svg_ctx* c; XfTrain* t;
    ArenaSwap(svg_ctx* c_, XfTrain* t_) : c(c_), t(t_) { std::swap(c->arena, t->ws); std::swap(c->arena_buf, t->ws_buf); }
    ~ArenaSwap() { std::swap(c->arena, t->ws); std::swap(c->arena_buf, t->ws_buf); }
  } arena_swap(ctx, tr);
  const int mode = expected ? 0 : 2;
  XfTrain::Plan* pl = nullptr;
  for (auto& c : tr->plans)
    if (c.B == B && c.Ts == Ts && c.Tt == Tt && c.backward == backward && c.mode == mode && c.has_mask == (mask != nullptr) &&
        c.has_text == (text != nullptr) && c.cfg.frames_to_predict == cfg.frames_to_predict && c.cfg.feat_h == cfg.feat_h &&
        c.cfg.feat_w == cfg.feat_w && c.cfg.w_mse == cfg.w_mse && c.cfg.w_l1 == cfg.w_l1 && c.cfg.w_gdl == cfg.w_gdl &&
        c.cfg.gdl_alpha == cfg.gdl_alpha && c.cfg.w_contrastive == cfg.w_contrastive && c.cfg.temperature == cfg.temperature &&
        c.cfg.dropout_p == cfg.dropout_p) { pl = &c; break; }
  if (!pl) {
    tr->plans.emplace_back();
    pl = &tr->plans.back();
    pl->cfg = cfg; pl->B = B; pl->Ts = Ts; pl->Tt = Tt; pl->backward = backward; pl->mode = mode;
    pl->has_mask = mask != nullptr; pl->has_text = text != nullptr;
    ctx->arena.reset(); ctx->arena.dry = true; ctx->arena.high = 0;          // dry pass: the workspace this signature needs
    try { body(src, tgt, expected, text, mask); } catch (...) { ctx->arena.dry = false; tr->plans.pop_back(); throw; }
    ctx->arena.dry = false;
    pl->high = ctx->arena.high;
  }
  ctx->ensure_arena(pl->high);
  tr->seed_slot = (tr->seed_slot + 1) & 15;
  if (!tr->seed_ev[tr->seed_slot]) HIP_OK(hipEventCreateWithFlags(&tr->seed_ev[tr->seed_slot], hipEventDisableTiming));
  else HIP_OK(hipEventSynchronize(tr->seed_ev[tr->seed_slot]));       // the slot's previous upload (16 calls ago) has been read
  tr->h_seed[tr->seed_slot] = cfg.seed;
  HIP_OK(hipMemcpyAsync(tr->d_seed, tr->h_seed + tr->seed_slot, sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(tr->seed_ev[tr->seed_slot], s));
  const bool graph_env = svg_env_i64("SVG_TRAIN_GRAPH", 1) != 0;
  // hipGraph replay of the whole step: needs a capturable (non-null) stream; the inputs go through fixed staging buffers
  if (graph_env && expected && s != nullptr && !ctx->prof) {
    if (!pl->src) {
      pl->src = (float*)tr->dalloc((int64_t)B * Ts * m->d_lat * sizeof(float));
      pl->tgt = (float*)tr->dalloc((int64_t)B * Tt * m->d_lat * sizeof(float));
      pl->exp = (float*)tr->dalloc((int64_t)B * Tt * m->d_lat * sizeof(float));
      if (text) pl->text = (float*)tr->dalloc((int64_t)B * m->text_dim * sizeof(float));
      if (mask) pl->mask = (float*)tr->dalloc((int64_t)Tt * Tt * sizeof(float));
    }
    HIP_OK(hipMemcpyAsync(pl->src, src, (size_t)B * Ts * m->d_lat * sizeof(float), hipMemcpyDefault, s));
    HIP_OK(hipMemcpyAsync(pl->tgt, tgt, (size_t)B * Tt * m->d_lat * sizeof(float), hipMemcpyDefault, s));
    HIP_OK(hipMemcpyAsync(pl->exp, expected, (size_t)B * Tt * m->d_lat * sizeof(float), hipMemcpyDefault, s));
    if (text) HIP_OK(hipMemcpyAsync(pl->text, text, (size_t)B * m->text_dim * sizeof(float), hipMemcpyDefault, s));
    if (mask) HIP_OK(hipMemcpyAsync(pl->mask, mask, (size_t)Tt * Tt * sizeof(float), hipMemcpyDefault, s));
    if (!pl->exec || pl->arena_base != ctx->arena.base) {       // first use, or the workspace moved since the capture
      if (pl->exec) { HIP_OK(hipGraphExecDestroy(pl->exec)); pl->exec = nullptr; }
      hipGraph_t g = nullptr;
      {
        CaptureScope cap;             // shared with other captures, exclusive against device-wide syncs (common.h)
        HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
          ctx->arena.reset();
          body(pl->src, pl->tgt, pl->exp, pl->text, pl->mask);
        } catch (...) {
          hipStreamEndCapture(s, &g);
          if (g) hipGraphDestroy(g);
          throw;
        }
        HIP_OK(hipStreamEndCapture(s, &g));
      }
      const hipError_t e = hipGraphInstantiate(&pl->exec, g, nullptr, nullptr, 0);
      hipGraphDestroy(g);
      HIP_OK(e);
      pl->arena_base = ctx->arena.base;
    }
    HIP_OK(hipGraphLaunch(pl->exec, s));
  } else {
    ctx->arena.reset();
    body(src, tgt, expected, text, mask);
  }
  if (losses_host) {
    HIP_OK(hipMemcpyAsync(tr->h_losses, tr->d_losses, 5 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    memcpy(losses_host, tr->h_losses, 5 * sizeof(float));
  }
}

// The training state, and with `ema` the averaged weights (a copy of the parameters as they stand), for the entry points that put
// state back or configure it.  Whatever is missing is allocated under the device-wide lock after a device-wide synchronisation: an
// optimizer step still running on another stream has then written the parameters the copy reads.
XfTrain* state_for_restore(svg_ctx* ctx, XfModel* m, bool ema) {
  SVG_CHECK(m->ready, "transformer: svg_finalize has not been called");
  if (m->train && (!ema || m->train->d_ema)) return m->train;
  DeviceWideScope lk;
  HIP_OK(hipDeviceSynchronize());
  ensure_train(ctx, m);
  XfTrain* tr = m->train;
  if (!ema) return tr;
  std::vector<float*> tab;
  for (auto& n : tr->names) {
    XfTrain::Slot& sl = tr->slots.at(n);
    if (!sl.e) sl.e = (float*)tr->dalloc(sl.n * sizeof(float));
    HIP_OK(hipMemcpy(sl.e, m->ws.get(n).f32, sl.n * sizeof(float), hipMemcpyDeviceToDevice));
    tab.push_back(sl.e);
  }
  float** d = (float**)tr->dalloc(tab.size() * sizeof(float*));
  HIP_OK(hipMemcpy(d, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice));
  HIP_OK(hipDeviceSynchronize());
  tr->d_ema = d;
  return tr;
}

}  // namespace

// caller holds DeviceWideScope when m->train exists (svg_destroy, svg_model_configure, svg_load_weight)
void xf_train_free(XfModel* m) {
  if (!m->train) return;
  hipDeviceSynchronize();
  delete m->train;
  m->train = nullptr;
}

extern "C" int svg_transformer_loss(svg_ctx* ctx, const svg_train_cfg* cfg, const float* src, const float* tgt, const float* expected,
                                    const float* text, int B, int Ts, int Tt, const float* mask, int backward, float* losses, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf, "transformer: model not configured");
    SVG_CHECK(cfg && src && tgt && expected, "svg_transformer_loss: null argument");
    // 0, 1 or SVG_BACKWARD_ACCUMULATE: the plan (and its captured graph) is keyed on the normalised mode
    const int mode = backward == 0 ? 0 : (backward == SVG_BACKWARD_ACCUMULATE ? SVG_BACKWARD_ACCUMULATE : 1);
    loss_pass(ctx, ctx->xf, *cfg, src, tgt, expected, text, B, Ts, Tt, mask, mode, losses, (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_forward_train(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                             const float* mask, float dropout_p, uint64_t seed, float* out, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf, "transformer: model not configured");
    SVG_CHECK(src && tgt && out, "svg_transformer_forward_train: null argument");
    svg_train_cfg cfg{};
    cfg.dropout_p = dropout_p;
    cfg.seed = seed;
    loss_pass(ctx, ctx->xf, cfg, src, tgt, nullptr, text, B, Ts, Tt, mask, /*train mode*/ 1, nullptr, (hipStream_t)stream, out);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_adam_step(svg_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf && ctx->xf->train, "adam step: no gradients yet (call svg_transformer_loss with backward=1 first)");
    SVG_CHECK(lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam step: bad hyper-parameters");
    XfTrain* tr = ctx->xf->train;
    tr->step += 1;
    xf_adam(tr->d_tens, tr->d_chunks, tr->n_chunks, lr, beta1, beta2, eps, tr->step, tr->ema_decay > 0.f ? tr->d_ema : nullptr, tr->ema_decay,
            (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

namespace {
// enqueues the norm pass; host != nullptr: reads the norm back (synchronises)
void grad_norm_pass(XfTrain* tr, double* host, hipStream_t s) {
  xf_grad_norm(tr->d_tens, tr->d_chunks, tr->n_chunks, tr->d_norm_part, tr->d_norm, s);
  if (!host) return;
  HIP_OK(hipMemcpyAsync(tr->h_norm, tr->d_norm, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  *host = *tr->h_norm;
}
}  // namespace

extern "C" int svg_transformer_grad_norm(svg_ctx* ctx, double* out, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf && out, "svg_transformer_grad_norm: null argument");
    SVG_CHECK(ctx->xf->train && ctx->xf->train->has_grads, "gradient norm: no gradients yet (call svg_transformer_loss with backward=1 first)");
    grad_norm_pass(ctx->xf->train, out, (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_optim_step(svg_ctx* ctx, const svg_optim_cfg* cfg, double* grad_norm_out, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf && cfg, "svg_transformer_optim_step: null argument");
    SVG_CHECK(ctx->xf->train && ctx->xf->train->has_grads, "optimizer step: no gradients yet (call svg_transformer_loss with backward=1 first)");
    SVG_CHECK(cfg->lr >= 0.f && cfg->beta1 >= 0.f && cfg->beta1 < 1.f && cfg->beta2 >= 0.f && cfg->beta2 < 1.f && cfg->eps >= 0.f,
              "optimizer step: bad hyper-parameters");
    SVG_CHECK(cfg->weight_decay >= 0.f, "optimizer step: weight_decay %g is negative", cfg->weight_decay);
    SVG_CHECK(cfg->max_grad_norm >= 0.f, "optimizer step: max_grad_norm %g is negative", cfg->max_grad_norm);
    SVG_CHECK(cfg->grad_scale > 0.f, "optimizer step: grad_scale %g is not positive", cfg->grad_scale);
    XfTrain* tr = ctx->xf->train;
    hipStream_t s = (hipStream_t)stream;
    const bool clip = cfg->max_grad_norm > 0.f;
    double norm = 0.0;
    if (clip || grad_norm_out) grad_norm_pass(tr, grad_norm_out ? &norm : nullptr, s);
    tr->step += 1;
    xf_adamw(tr->d_tens, tr->d_chunks, tr->n_chunks, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, tr->step, cfg->weight_decay, cfg->decoupled != 0,
             cfg->grad_scale, cfg->max_grad_norm, clip ? tr->d_norm : nullptr, tr->ema_decay > 0.f ? tr->d_ema : nullptr, tr->ema_decay, s);
    if (grad_norm_out) *grad_norm_out = (double)cfg->grad_scale * norm;
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_tensor(svg_ctx* ctx, int kind, const char* name, float* out, int64_t numel, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf && name && out, "svg_transformer_tensor: null argument");
    XfModel* m = ctx->xf;
    SVG_CHECK(m->ws.has(name), "svg_transformer_tensor: no tensor named %s", name);
    const Weight& w = m->ws.get(name);
    SVG_CHECK(numel == w.numel, "svg_transformer_tensor: %s has %lld elements, caller asked for %lld", name, (long long)w.numel, (long long)numel);
    const float* srcp = w.f32;
    if (kind != SVG_TENSOR_PARAM) {
      SVG_CHECK(kind == SVG_TENSOR_GRAD || kind == SVG_TENSOR_EXP_AVG || kind == SVG_TENSOR_EXP_AVG_SQ || kind == SVG_TENSOR_EMA,
                "svg_transformer_tensor: kind %d", kind);
      SVG_CHECK(m->train && m->train->slots.count(name), "svg_transformer_tensor: %s has no training state", name);
      const XfTrain::Slot& sl = m->train->slots.at(name);
      SVG_CHECK(kind != SVG_TENSOR_EMA || m->train->d_ema,
                "svg_transformer_tensor: no averaged weights yet (svg_transformer_ema_configure or svg_transformer_set_tensor(SVG_TENSOR_EMA) first)");
      srcp = kind == SVG_TENSOR_GRAD ? sl.g : (kind == SVG_TENSOR_EXP_AVG ? sl.m : (kind == SVG_TENSOR_EXP_AVG_SQ ? sl.v : sl.e));
    }
    HIP_OK(hipMemcpyAsync(out, srcp, numel * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_set_tensor(svg_ctx* ctx, int kind, const char* name, const float* data, int64_t numel, void* stream) {
  try {
    SVG_CHECK(ctx && ctx->xf && name && data, "svg_transformer_set_tensor: null argument");
    XfModel* m = ctx->xf;
    SVG_CHECK(kind == SVG_TENSOR_EXP_AVG || kind == SVG_TENSOR_EXP_AVG_SQ || kind == SVG_TENSOR_EMA,
              "svg_transformer_set_tensor: kind %d cannot be set (parameters go through svg_load_weight, gradients come from svg_transformer_loss)", kind);
    SVG_CHECK(m->ws.has(name) && strcmp(name, "positional_encoder.pos_encoding") != 0, "svg_transformer_set_tensor: no trained tensor named %s", name);
    const Weight& w = m->ws.get(name);
    SVG_CHECK(numel == w.numel, "svg_transformer_set_tensor: %s has %lld elements, caller gave %lld", name, (long long)w.numel, (long long)numel);
    XfTrain* tr = state_for_restore(ctx, m, kind == SVG_TENSOR_EMA);
    const XfTrain::Slot& sl = tr->slots.at(name);
    float* dst = kind == SVG_TENSOR_EXP_AVG ? sl.m : (kind == SVG_TENSOR_EXP_AVG_SQ ? sl.v : sl.e);
    HIP_OK(hipMemcpyAsync(dst, data, numel * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_optim_step_count(svg_ctx* ctx, int64_t* out) {
  try {
    SVG_CHECK(ctx && ctx->xf && out, "svg_transformer_optim_step_count: null argument");
    *out = ctx->xf->train ? ctx->xf->train->step : 0;
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_set_optim_step_count(svg_ctx* ctx, int64_t step) {
  try {
    SVG_CHECK(ctx && ctx->xf, "svg_transformer_set_optim_step_count: model not configured");
    SVG_CHECK(step >= 0 && step <= 0x7fffffff, "svg_transformer_set_optim_step_count: step %lld out of range", (long long)step);
    state_for_restore(ctx, ctx->xf, false)->step = (int)step;
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_transformer_ema_configure(svg_ctx* ctx, float decay) {
  try {
    SVG_CHECK(ctx && ctx->xf, "svg_transformer_ema_configure: model not configured");
    SVG_CHECK(decay >= 0.f && decay < 1.f, "svg_transformer_ema_configure: decay %g is outside [0, 1)", decay);
    if (decay == 0.f) {                                   // updates off; the buffers (if any) keep their values
      if (ctx->xf->train) ctx->xf->train->ema_decay = 0.f;
      return 0;
    }
    state_for_restore(ctx, ctx->xf, true)->ema_decay = decay;
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

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

extern "C" int svg_op_dropout_mask(svg_ctx* ctx, uint64_t seed, int site, float p, float* out, int64_t n, void* stream) {
  try {
    SVG_CHECK(ctx && out && n >= 0, "svg_op_dropout_mask: bad argument");
    xf_drop_mask(op_drop(ctx, "svg_op_dropout_mask", seed, site, p, (hipStream_t)stream), out, n, (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

// ---- the training kernels one by one (test hooks: each is its launcher and nothing else) ------------------------------------------
extern "C" int svg_op_xf_gemm_tn(svg_ctx* ctx, const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int M, int N, int K,
                                 int accumulate, void* stream) {
  try {
    SVG_CHECK(ctx && dY && X && dW, "svg_op_xf_gemm_tn: null argument");
    xf_gemm_tn(dY, ldy, X, ldx, dW, db, M, N, K, accumulate, (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_gemm_nn(svg_ctx* ctx, const float* dY, int ldy, const float* W, float* out, int M, int N, int K, const float* gate,
                                 float gate_scale, const float* add, int* splits, void* stream) {
  try {
    SVG_CHECK(ctx && dY && W && out, "svg_op_xf_gemm_nn: null argument");
    SVG_CHECK(M > 0 && N > 0 && K > 0, "svg_op_xf_gemm_nn: empty problem %d x %d x %d", M, N, K);
    run_planned(ctx, [&]() {
      float* slabs = ctx->arena.get<float>(xf_gemm_nn_slab_floats(M, N, K));
      if (SVG_LAUNCHING(ctx)) xf_gemm_nn(dY, ldy, W, slabs, out, M, N, K, gate, gate_scale, add, (hipStream_t)stream);
    });
    if (splits) *splits = xf_gemm_nn_splits(N, K);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_relu_drop(svg_ctx* ctx, const float* h, float* r, int64_t n, uint64_t seed, int site, float p, void* stream) {
  try {
    SVG_CHECK(ctx && h && r && n >= 0, "svg_op_xf_relu_drop: bad argument");
    xf_relu_drop(h, r, n, op_drop(ctx, "svg_op_xf_relu_drop", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_add_ln_train(svg_ctx* ctx, const float* x, const float* r, uint64_t seed, int site, float p, const float* gamma,
                                      const float* beta, float* y, float* xhat, float* rstd, int M, int d, float eps, void* stream) {
  try {
    SVG_CHECK(ctx && x && gamma && beta && y && xhat && rstd, "svg_op_xf_add_ln_train: null argument");
    xf_add_ln_train(x, r, op_drop(ctx, "svg_op_xf_add_ln_train", seed, site, p, (hipStream_t)stream), gamma, beta, y, xhat, rstd, M, d, eps,
                    (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_ln_bwd(svg_ctx* ctx, const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* dz_drop,
                                uint64_t seed, int site, float p, float* dgamma, float* dbeta, int M, int d, int accumulate, void* stream) {
  try {
    SVG_CHECK(ctx && dy && xhat && rstd && gamma && dz && dgamma && dbeta, "svg_op_xf_ln_bwd: null argument");
    xf_ln_bwd(dy, xhat, rstd, gamma, dz, dz_drop, op_drop(ctx, "svg_op_xf_ln_bwd", seed, site, p, (hipStream_t)stream), dgamma, dbeta, M, d,
              accumulate, (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_attention_train(svg_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldk, const float* mask,
                                         float* o, float* P, int Tq, int Tk, int B, int heads, int hd, uint64_t seed, int site, float p,
                                         void* stream) {
  try {
    SVG_CHECK(ctx && q && k && v && o && P, "svg_op_xf_attention_train: null argument");
    xf_attention_train(q, ldq, k, v, ldk, mask, o, P, Tq, Tk, B, heads, hd,
                       op_drop(ctx, "svg_op_xf_attention_train", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_attention_bwd(svg_ctx* ctx, const float* dout, const float* q, int ldq, const float* k, const float* v, int ldk,
                                       const float* P, float* dq, int lddq, float* dk, float* dv, int lddk, int Tq, int Tk, int B, int heads,
                                       int hd, uint64_t seed, int site, float p, void* stream) {
  try {
    SVG_CHECK(ctx && dout && q && k && v && P && dq && dk && dv, "svg_op_xf_attention_bwd: null argument");
    xf_attention_bwd(dout, q, ldq, k, v, ldk, P, dq, lddq, dk, dv, lddk, Tq, Tk, B, heads, hd,
                     op_drop(ctx, "svg_op_xf_attention_bwd", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_embed_post_train(svg_ctx* ctx, const float* emb, const float* pe, const int32_t* pe_row, const float* text, int d_txt,
                                          float* y, int B, int T, int d, float scale, uint64_t seed, int site, float p, void* stream) {
  try {
    SVG_CHECK(ctx && emb && pe && y, "svg_op_xf_embed_post_train: null argument");
    xf_embed_post_train(emb, pe, pe_row, text, d_txt, y, B, T, d, scale,
                        op_drop(ctx, "svg_op_xf_embed_post_train", seed, site, p, (hipStream_t)stream), (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_embed_post_bwd(svg_ctx* ctx, const float* dy, float* de, int B, int T, int d, int d_img, float scale, uint64_t seed,
                                        int site, float p, void* stream) {
  try {
    SVG_CHECK(ctx && dy && de, "svg_op_xf_embed_post_bwd: null argument");
    xf_embed_post_bwd(dy, de, B, T, d, d_img, scale, op_drop(ctx, "svg_op_xf_embed_post_bwd", seed, site, p, (hipStream_t)stream),
                      (hipStream_t)stream);
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}

extern "C" int svg_op_xf_criterion(svg_ctx* ctx, const float* pred, const float* expected, float* dpred, float* losses, int Tt, int B, int D,
                                   int t0, int fh, int fw, float w_mse, float w_l1, float w_gdl, float alpha, float w_nce, float temperature,
                                   void* stream) {
  try {
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
    return 0;
  } catch (const std::exception& e) { return svg_fail(ctx, e); }
}
