// Training step of the latent Transformer: forward in train mode keeping what backward needs, the criterion, backward through
// every layer, Adam.  Reference: trainers/trainer.py:111-190 (train_loop body: pred = model(new_batch, y_input, tgt_mask);
// loss_fn(pred[-F:], y_expected[-F:]); opt.zero_grad(); loss.backward(); opt.step()), :65-109 (criterion), :192-260
// (validation_loop: the same loss in eval mode) over torch.nn.Transformer (post-norm, ReLU, dropout after the positional
// encoding, on the attention probabilities, after each sublayer and inside the feed-forward) and torch.optim.Adam(lr).
// The Stable Diffusion side stays frozen (encode_batch is the VAE encoder the sampling path already has).
// This file: the training state (XfTrain), the step as operations of xf_graph() and their backward (Run), loss_pass, and the public
// training entry points.  The per-kernel test hooks are in xf_ops.cpp.
#include "xf_plan.h"
#include "../../include/svg_hip.h"
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <tuple>

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
  // The signature of a call: the shapes, the mode and every criterion / dropout parameter except the seed.
  struct Sig {
    int B, Ts, Tt, backward;       // backward: 0, 1 or SVG_BACKWARD_ACCUMULATE
    bool loss, has_mask, has_text; // loss == false: forward only
    int frames_to_predict, feat_h, feat_w;
    float w_mse, w_l1, w_gdl, gdl_alpha, w_contrastive, temperature, dropout_p;
    auto key() const {
      return std::make_tuple(B, Ts, Tt, backward, loss, has_mask, has_text, frames_to_predict, feat_h, feat_w, w_mse, w_l1, w_gdl, gdl_alpha,
                             w_contrastive, temperature, dropout_p);
    }
    bool operator==(const Sig& o) const { return key() == o.key(); }
  };
  // One plan per signature: the workspace high-water mark and, for the loss (+ backward) calls, the captured hipGraph of the whole
  // step.  ~540 launches per step cost more host time than the GPU needs to run them (15.3 ms wall against 9.3 ms of kernels); the
  // graph replays them from fixed staging buffers.
  struct Plan {
    Sig sig{};
    int64_t high = 0;
    GraphExec exec;
    char* arena_base = nullptr;
    float *src = nullptr, *tgt = nullptr, *exp = nullptr, *text = nullptr, *mask = nullptr;
  };
  std::vector<Plan> plans;
  // The seed word every dropout site reads, fed through a pinned ring of 16 (a call that does not synchronise must not race the
  // next one's seed); an event behind each slot's upload makes the 17th unsynchronised call wait for the 1st one's copy.
  struct SeedRing {
    uint64_t *d_seed = nullptr, *h_seed = nullptr;
    hipEvent_t ev[16] = {};
    int slot = 0;
    void upload(uint64_t seed, hipStream_t s) {
      slot = (slot + 1) & 15;
      if (!ev[slot]) HIP_OK(hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming));
      else HIP_OK(hipEventSynchronize(ev[slot]));       // the slot's previous upload (16 calls ago) has been read
      h_seed[slot] = seed;
      HIP_OK(hipMemcpyAsync(d_seed, h_seed + slot, sizeof(uint64_t), hipMemcpyHostToDevice, s));
      HIP_OK(hipEventRecord(ev[slot], s));
    }
    ~SeedRing() { if (h_seed) hipHostFree(h_seed); for (auto e : ev) if (e) hipEventDestroy(e); }
  } seed;
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
    for (void* p : bufs) hipFree(p);
    if (h_losses) hipHostFree(h_losses);
    if (h_norm) hipHostFree(h_norm);
    if (ws_buf.p) hipFree(ws_buf.p);
  }
};

namespace {

constexpr int kAdamChunk = 1 << 16;
using Sig = XfTrain::Sig;
struct Inputs { const float *src, *tgt, *expected, *text, *mask; };   // expected == nullptr: forward only

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

// One pass over the step: the training kernels (xf_train.hip) as the operations of xf_graph(), their backward counterparts, and
// step() = forward, criterion, backward.  The order of launches and of arena.get calls IS the captured graph and the workspace layout.
struct Run {
  static constexpr bool kSharesEmbedding = false;   // each embedding draws its own dropout mask
  svg_ctx* ctx; XfModel* m; XfTrain* tr; const Sig& sig; hipStream_t s; const int B; const uint64_t* seed; const float p;
  const bool acc;    // SVG_BACKWARD_ACCUMULATE: every gradient store adds to its slot
  const float* text = nullptr;
  uint32_t site = 0;
  std::vector<LayerTape> enc, dec;
  LinTape e_lin[2], l_out;
  XfDrop e_drop[2];
  LnTape n_enc, n_dec;
  Run(svg_ctx* ctx_, XfModel* m_, XfTrain* tr_, const Sig& g, hipStream_t s_)
      : ctx(ctx_), m(m_), tr(tr_), sig(g), s(s_), B(g.B), seed(tr_->seed.d_seed), p(g.backward ? g.dropout_p : 0.f),
        acc(g.backward == SVG_BACKWARD_ACCUMULATE), enc(m_->enc_layers), dec(m_->dec_layers) {}
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

  // ---- the step ---------------------------------------------------------------------------------------------------------------
  // forward only: the prediction (Tt,B,D_lat) goes to pred_out
  void step(const Inputs& in, float* pred_out) {
    text = in.text;
    float* pred = xf_graph(*this, *m, XfChunk{B, sig.Ts, sig.Tt, in.src, in.tgt, in.mask, in.text, nullptr, nullptr, m->iota, nullptr});
    if (!sig.loss) {
      if (go()) HIP_OK(hipMemcpyAsync(pred_out, pred, (size_t)sig.Tt * B * m->d_lat * sizeof(float), hipMemcpyDeviceToDevice, s));
      return;
    }
    float* dpred = criterion(pred, in.expected);
    if (sig.backward) backward(dpred);
  }
  // on the last frames_to_predict positions (trainer.py:145); returns the gradient of the prediction
  float* criterion(const float* pred, const float* expected) {
    const int Mt = sig.Tt * B;
    float* dpred = get<float>((int64_t)Mt * m->d_lat);
    float* part = get<float>((int64_t)Mt * 3);
    float* part2 = get<float>(Mt);
    if (go())
      xf_criterion(pred, expected, dpred, part, part2, tr->d_losses, sig.Tt, B, m->d_lat, sig.Tt - sig.frames_to_predict, sig.feat_h, sig.feat_w,
                   sig.w_mse, sig.w_l1, sig.w_gdl, sig.gdl_alpha, sig.w_contrastive, sig.temperature, s);
    return dpred;
  }
  // backward of one post-norm sublayer y = LN(x + dropout(f(x))), f the feed-forward or an attention: returns dx
  float* ffn_sub_bwd(const LnTape& n, const FfnTape& f, const float* dy) {
    float* dzd = nullptr;
    float* dz = add_ln_bwd(n, dy, &dzd);
    float* dx = get<float>((int64_t)n.M * m->d_model);
    ffn_bwd(f, dzd, dx, dz);
    return dx;
  }
  float* mha_sub_bwd(const LnTape& n, const MhaTape& a, const float* dy, float* dmem = nullptr, bool dmem_accumulate = false) {
    float* dzd = nullptr;
    float* dz = add_ln_bwd(n, dy, &dzd);
    float* dx = get<float>((int64_t)n.M * m->d_model);
    mha_bwd(a, dzd, dx, dz, dmem, dmem_accumulate);
    return dx;
  }
  void backward(const float* dpred) {
    const int d = m->d_model, Ms = sig.Ts * B, Mt = sig.Tt * B;
    float* dx = get<float>((int64_t)Mt * d);
    lin_bwd(l_out, dpred, dx);
    float* dxt = add_ln_bwd(n_dec, dx, nullptr);
    float* dmem = get<float>((int64_t)Ms * d);
    bool dmem_set = false;
    for (int i = m->dec_layers - 1; i >= 0; --i) {
      const LayerTape& t = dec[i];
      dxt = ffn_sub_bwd(t.n[2], t.ff, dxt);                     // x2 + dropout(ff(x2))
      dxt = mha_sub_bwd(t.n[1], t.ca, dxt, dmem, dmem_set);     // x1 + dropout(cross(x1, mem))
      dmem_set = true;
      dxt = mha_sub_bwd(t.n[0], t.sa, dxt);                     // x + dropout(self(x))
    }
    if (!dmem_set && go()) SDNS::fill_f32(dmem, (int64_t)Ms * d, 0.f, s);
    float* dxs = add_ln_bwd(n_enc, dmem, nullptr);
    for (int i = m->enc_layers - 1; i >= 0; --i) {
      const LayerTape& t = enc[i];
      dxs = ffn_sub_bwd(t.n[1], t.ff, dxs);
      dxs = mha_sub_bwd(t.n[0], t.sa, dxs);
    }
    embed_bwd(0, dxs, sig.Ts, false);
    embed_bwd(1, dxt, sig.Tt, true);                // the embedding layer is shared: second contribution accumulates
  }
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
  tr->seed.d_seed = (uint64_t*)tr->dalloc(sizeof(uint64_t));
  HIP_OK(hipHostMalloc((void**)&tr->seed.h_seed, 16 * sizeof(uint64_t), hipHostMallocDefault));
  HIP_OK(hipMemcpy(tr->d_tens, tens.data(), tens.size() * sizeof(XfAdamTensor), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(tr->d_chunks, chunks.data(), chunks.size() * sizeof(XfAdamChunk), hipMemcpyHostToDevice));
  tr->n_chunks = (int)chunks.size();
  tr->names = names;
  m->each_param(tr->g, [&](const std::string& name, std::initializer_list<int64_t>, float*& slot) { slot = tr->slots.at(name).g; });
  m->train = tr.release();
}

void check_call(const XfModel* m, const Sig& g) {
  SVG_CHECK(m->ready, "transformer: svg_finalize has not been called");
  SVG_CHECK((m->text_dim > 0) == g.has_text, "transformer: the text-conditioned variant needs (and only it takes) a text embedding");
  SVG_CHECK(g.B >= 1 && g.B <= 64 && g.Ts >= 1 && g.Tt >= 1 && g.Ts <= 32 && g.Tt <= 32,
            "transformer training: B=%d Ts=%d Tt=%d unsupported (B <= 64, T <= 32)", g.B, g.Ts, g.Tt);
  SVG_CHECK(g.dropout_p >= 0.f && g.dropout_p < 1.f, "dropout_p %g out of range", g.dropout_p);
  if (!g.loss) return;
  SVG_CHECK(g.frames_to_predict >= 1 && g.frames_to_predict <= g.Tt, "frames_to_predict %d out of range 1..%d", g.frames_to_predict, g.Tt);
  SVG_CHECK(g.feat_h > 0 && g.feat_w > 0 && 4 * g.feat_h * g.feat_w == m->d_lat, "criterion: D_lat %d is not 4 x %d x %d", m->d_lat, g.feat_h,
            g.feat_w);
  SVG_CHECK(g.w_contrastive == 0.f || (g.temperature > 0.f && g.feat_h * g.feat_w <= 4096), "contrastive loss: bad temperature / patch count");
}

// the training workspace stands in for the context arena until the call returns (or throws)
struct ArenaSwap {
  svg_ctx* c; XfTrain* t;
  ArenaSwap(svg_ctx* c_, XfTrain* t_) : c(c_), t(t_) { std::swap(c->arena, t->ws); std::swap(c->arena_buf, t->ws_buf); }
  ~ArenaSwap() { std::swap(c->arena, t->ws); std::swap(c->arena_buf, t->ws_buf); }
};

// the plan of a signature; a new one takes its workspace need from a dry pass of the step, and is dropped again if that throws
template <class Body>
XfTrain::Plan& find_or_plan(svg_ctx* ctx, XfTrain* tr, const Sig& sig, Body&& dry_pass) {
  for (auto& pl : tr->plans)
    if (pl.sig == sig) return pl;
  tr->plans.emplace_back();
  tr->plans.back().sig = sig;
  ctx->arena.dry = true; ctx->arena.high = 0;
  try { dry_pass(); } catch (...) { ctx->arena.dry = false; tr->plans.pop_back(); throw; }
  ctx->arena.dry = false;
  tr->plans.back().high = ctx->arena.high;
  return tr->plans.back();
}

// a replayed step reads its inputs from the plan's fixed staging buffers (allocated at the signature's first replay)
Inputs stage(XfModel* m, XfTrain::Plan& pl, const Inputs& in, hipStream_t s) {
  const Sig& g = pl.sig;
  const int64_t rows_s = (int64_t)g.B * g.Ts * m->d_lat, rows_t = (int64_t)g.B * g.Tt * m->d_lat;
  const struct { float** slot; const float* from; int64_t floats; } table[] = {
      {&pl.src, in.src, rows_s}, {&pl.tgt, in.tgt, rows_t}, {&pl.exp, in.expected, rows_t},
      {&pl.text, in.text, (int64_t)g.B * m->text_dim}, {&pl.mask, in.mask, (int64_t)g.Tt * g.Tt}};
  for (auto& e : table) {
    if (!e.from) continue;                         // no text / no mask: the slot stays null
    if (!*e.slot) *e.slot = (float*)m->train->dalloc(e.floats * sizeof(float));
    HIP_OK(hipMemcpyAsync(*e.slot, e.from, (size_t)e.floats * sizeof(float), hipMemcpyDefault, s));
  }
  return Inputs{pl.src, pl.tgt, pl.exp, pl.text, pl.mask};
}

// in.expected == nullptr: forward only (train-mode dropout when backward != 0), the prediction (Tt,B,D_lat) goes to pred_out
void loss_pass(svg_ctx* ctx, XfModel* m, const svg_train_cfg& cfg, const Inputs& in, int B, int Ts, int Tt, int backward, float* losses_host,
               hipStream_t s, float* pred_out = nullptr) {
  const Sig sig{B, Ts, Tt, backward, in.expected != nullptr, in.mask != nullptr, in.text != nullptr, cfg.frames_to_predict, cfg.feat_h,
                cfg.feat_w, cfg.w_mse, cfg.w_l1, cfg.w_gdl, cfg.gdl_alpha, cfg.w_contrastive, cfg.temperature, cfg.dropout_p};
  check_call(m, sig);
  ensure_train(ctx, m);
  XfTrain* tr = m->train;
  if (sig.loss && backward) tr->has_grads = true;
  ArenaSwap arena_swap(ctx, tr);
  auto body = [&](const Inputs& x) { ctx->arena.reset(); Run(ctx, m, tr, sig, s).step(x, pred_out); };
  XfTrain::Plan& pl = find_or_plan(ctx, tr, sig, [&]() { body(in); });
  ctx->ensure_arena(pl.high);
  tr->seed.upload(cfg.seed, s);
  // hipGraph replay of the whole step: needs a capturable (non-null) stream; the inputs go through fixed staging buffers
  if (svg_env_i64("SVG_TRAIN_GRAPH", 1) != 0 && sig.loss && s != nullptr && !ctx->prof) {
    const Inputs staged = stage(m, pl, in, s);
    if (!pl.exec || pl.arena_base != ctx->arena.base) {       // first use, or the workspace moved since the capture
      pl.exec = {};
      pl.exec = capture_graph(s, [&]() { body(staged); });
      pl.exec.drop_template();                                  // a plan lives long: the executable graph is all its replays need
      pl.arena_base = ctx->arena.base;
    }
    HIP_OK(hipGraphLaunch(pl.exec.h, s));
  } else {
    body(in);
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

// where a slot keeps a tensor of the training state (nullptr: `kind` names none)
float* slot_ptr(const XfTrain::Slot& sl, int kind) {
  return kind == SVG_TENSOR_GRAD ? sl.g : kind == SVG_TENSOR_EXP_AVG ? sl.m : kind == SVG_TENSOR_EXP_AVG_SQ ? sl.v : kind == SVG_TENSOR_EMA ? sl.e : nullptr;
}

void check_adam_hyper(const char* who, float lr, float beta1, float beta2, float eps) {
  SVG_CHECK(lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "%s: bad hyper-parameters", who);
}

// enqueues the norm pass; host != nullptr: reads the norm back (synchronises)
void grad_norm_pass(XfTrain* tr, double* host, hipStream_t s) {
  xf_grad_norm(tr->d_tens, tr->d_chunks, tr->n_chunks, tr->d_norm_part, tr->d_norm, s);
  if (!host) return;
  HIP_OK(hipMemcpyAsync(tr->h_norm, tr->d_norm, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  *host = *tr->h_norm;
}

}  // namespace

// caller holds DeviceWideScope when m->train exists (svg_destroy, svg_model_configure, svg_load_weight)
void xf_train_free(XfModel* m) {
  if (!m->train) return;
  hipDeviceSynchronize();
  delete m->train;
  m->train = nullptr;
}
void XfModel::weights_changed(bool locked) {
  if (locked) xf_train_free(this);
  else if (train) { DeviceWideScope lk; xf_train_free(this); }
  ready = false;
}

extern "C" int svg_transformer_loss(svg_ctx* ctx, const svg_train_cfg* cfg, const float* src, const float* tgt, const float* expected,
                                    const float* text, int B, int Ts, int Tt, const float* mask, int backward, float* losses, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "transformer: model not configured");
    SVG_CHECK(cfg && src && tgt && expected, "svg_transformer_loss: null argument");
    // 0, 1 or SVG_BACKWARD_ACCUMULATE: the plan (and its captured graph) is keyed on the normalised mode
    const int mode = backward == 0 ? 0 : (backward == SVG_BACKWARD_ACCUMULATE ? SVG_BACKWARD_ACCUMULATE : 1);
    loss_pass(ctx, ctx->xf(), *cfg, Inputs{src, tgt, expected, text, mask}, B, Ts, Tt, mode, losses, (hipStream_t)stream);
  });
}

extern "C" int svg_transformer_forward_train(svg_ctx* ctx, const float* src, const float* tgt, const float* text, int B, int Ts, int Tt,
                                             const float* mask, float dropout_p, uint64_t seed, float* out, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "transformer: model not configured");
    SVG_CHECK(src && tgt && out, "svg_transformer_forward_train: null argument");
    svg_train_cfg cfg{};
    cfg.dropout_p = dropout_p;
    cfg.seed = seed;
    loss_pass(ctx, ctx->xf(), cfg, Inputs{src, tgt, nullptr, text, mask}, B, Ts, Tt, /*train mode*/ 1, nullptr, (hipStream_t)stream, out);
  });
}

extern "C" int svg_transformer_adam_step(svg_ctx* ctx, float lr, float beta1, float beta2, float eps, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && ctx->xf()->train, "adam step: no gradients yet (call svg_transformer_loss with backward=1 first)");
    check_adam_hyper("adam step", lr, beta1, beta2, eps);
    XfTrain* tr = ctx->xf()->train;
    tr->step += 1;
    xf_adam(tr->d_tens, tr->d_chunks, tr->n_chunks, lr, beta1, beta2, eps, tr->step, tr->ema_decay > 0.f ? tr->d_ema : nullptr, tr->ema_decay,
            (hipStream_t)stream);
  });
}

extern "C" int svg_transformer_grad_norm(svg_ctx* ctx, double* out, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && out, "svg_transformer_grad_norm: null argument");
    SVG_CHECK(ctx->xf()->train && ctx->xf()->train->has_grads, "gradient norm: no gradients yet (call svg_transformer_loss with backward=1 first)");
    grad_norm_pass(ctx->xf()->train, out, (hipStream_t)stream);
  });
}

extern "C" int svg_transformer_optim_step(svg_ctx* ctx, const svg_optim_cfg* cfg, double* grad_norm_out, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && cfg, "svg_transformer_optim_step: null argument");
    SVG_CHECK(ctx->xf()->train && ctx->xf()->train->has_grads, "optimizer step: no gradients yet (call svg_transformer_loss with backward=1 first)");
    check_adam_hyper("optimizer step", cfg->lr, cfg->beta1, cfg->beta2, cfg->eps);
    SVG_CHECK(cfg->weight_decay >= 0.f, "optimizer step: weight_decay %g is negative", cfg->weight_decay);
    SVG_CHECK(cfg->max_grad_norm >= 0.f, "optimizer step: max_grad_norm %g is negative", cfg->max_grad_norm);
    SVG_CHECK(cfg->grad_scale > 0.f, "optimizer step: grad_scale %g is not positive", cfg->grad_scale);
    XfTrain* tr = ctx->xf()->train;
    hipStream_t s = (hipStream_t)stream;
    const bool clip = cfg->max_grad_norm > 0.f;
    double norm = 0.0;
    if (clip || grad_norm_out) grad_norm_pass(tr, grad_norm_out ? &norm : nullptr, s);
    tr->step += 1;
    xf_adamw(tr->d_tens, tr->d_chunks, tr->n_chunks, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, tr->step, cfg->weight_decay, cfg->decoupled != 0,
             cfg->grad_scale, cfg->max_grad_norm, clip ? tr->d_norm : nullptr, tr->ema_decay > 0.f ? tr->d_ema : nullptr, tr->ema_decay, s);
    if (grad_norm_out) *grad_norm_out = (double)cfg->grad_scale * norm;
  });
}

extern "C" int svg_transformer_tensor(svg_ctx* ctx, int kind, const char* name, float* out, int64_t numel, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && name && out, "svg_transformer_tensor: null argument");
    XfModel* m = ctx->xf();
    SVG_CHECK(m->ws.has(name), "svg_transformer_tensor: no tensor named %s", name);
    const Weight& w = m->ws.get(name);
    SVG_CHECK(numel == w.numel, "svg_transformer_tensor: %s has %lld elements, caller asked for %lld", name, (long long)w.numel, (long long)numel);
    const float* srcp = w.f32;
    if (kind != SVG_TENSOR_PARAM) {
      SVG_CHECK(kind == SVG_TENSOR_GRAD || kind == SVG_TENSOR_EXP_AVG || kind == SVG_TENSOR_EXP_AVG_SQ || kind == SVG_TENSOR_EMA,
                "svg_transformer_tensor: kind %d", kind);
      SVG_CHECK(m->train && m->train->slots.count(name), "svg_transformer_tensor: %s has no training state", name);
      SVG_CHECK(kind != SVG_TENSOR_EMA || m->train->d_ema,
                "svg_transformer_tensor: no averaged weights yet (svg_transformer_ema_configure or svg_transformer_set_tensor(SVG_TENSOR_EMA) first)");
      srcp = slot_ptr(m->train->slots.at(name), kind);
    }
    HIP_OK(hipMemcpyAsync(out, srcp, numel * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

extern "C" int svg_transformer_set_tensor(svg_ctx* ctx, int kind, const char* name, const float* data, int64_t numel, void* stream) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && name && data, "svg_transformer_set_tensor: null argument");
    XfModel* m = ctx->xf();
    SVG_CHECK(kind == SVG_TENSOR_EXP_AVG || kind == SVG_TENSOR_EXP_AVG_SQ || kind == SVG_TENSOR_EMA,
              "svg_transformer_set_tensor: kind %d cannot be set (parameters go through svg_load_weight, gradients come from svg_transformer_loss)", kind);
    SVG_CHECK(m->ws.has(name) && strcmp(name, "positional_encoder.pos_encoding") != 0, "svg_transformer_set_tensor: no trained tensor named %s", name);
    const Weight& w = m->ws.get(name);
    SVG_CHECK(numel == w.numel, "svg_transformer_set_tensor: %s has %lld elements, caller gave %lld", name, (long long)w.numel, (long long)numel);
    XfTrain* tr = state_for_restore(ctx, m, kind == SVG_TENSOR_EMA);
    HIP_OK(hipMemcpyAsync(slot_ptr(tr->slots.at(name), kind), data, numel * sizeof(float), hipMemcpyDefault, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

extern "C" int svg_transformer_optim_step_count(svg_ctx* ctx, int64_t* out) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf() && out, "svg_transformer_optim_step_count: null argument");
    *out = ctx->xf()->train ? ctx->xf()->train->step : 0;
  });
}

extern "C" int svg_transformer_set_optim_step_count(svg_ctx* ctx, int64_t step) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "svg_transformer_set_optim_step_count: model not configured");
    SVG_CHECK(step >= 0 && step <= 0x7fffffff, "svg_transformer_set_optim_step_count: step %lld out of range", (long long)step);
    state_for_restore(ctx, ctx->xf(), false)->step = (int)step;
  });
}

extern "C" int svg_transformer_ema_configure(svg_ctx* ctx, float decay) {
  return svg_guard(ctx, [&] {
    SVG_CHECK(ctx && ctx->xf(), "svg_transformer_ema_configure: model not configured");
    SVG_CHECK(decay >= 0.f && decay < 1.f, "svg_transformer_ema_configure: decay %g is outside [0, 1)", decay);
    if (decay == 0.f) {                                   // updates off; the buffers (if any) keep their values
      if (ctx->xf()->train) ctx->xf()->train->ema_decay = 0.f;
      return;
    }
    state_for_restore(ctx, ctx->xf(), true)->ema_decay = decay;
  });
}
