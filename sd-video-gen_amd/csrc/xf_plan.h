// The forward plan of the latent Transformer and the stage tables of its two single-launch forms (xf_plan.cpp: no HIP runtime call, no
// kernel).  XfModel::forward asks xf_plan() once and dispatches on the answer; the tables are plain functions of the model, the chunk's
// shape and its workspace, so the decision and the tables can be dumped and pinned on a machine without a GPU
// (tools/host_sanitize/xf_plan_dump.cpp, tests/test_xf_plan_cpu.py).
#pragma once
#include "models.h"
#include "xf_walk.h"

enum XfForm : int {
  XF_PER_GEMM = 0,     // one launch per GEMM / LayerNorm / attention (xformer.hip)
  XF_WALK = 1,         // one launch walks the layers, split-K GEMM stages (xf_walk_kernel)
  XF_WALK_SMALL = 2,   // the same for at most kWalkSmallRows rows, whole-K stages with the LayerNorms folded in (xf_walk_small_kernel)
};
// why a forward does not take the split-K walk
enum XfRefusal : int { XF_TAKEN = 0, XF_OFF = 1 /* walk off, or more rows than $SVG_XF_WALK_ROWS and no split */, XF_SHAPE = 2, XF_STAGES = 3 };

struct XfShape { int B, Ts, Tt; bool has_text, same; };                     // same: src and tgt are one buffer
struct XfDevice { bool walk_enabled; int grid; int64_t lds_limit; };        // grid: workgroups of a walk launch
struct XfKnobs { int64_t walk_rows = 96, walk_split = 0, walk_small = -1; };  // $SVG_XF_WALK_ROWS / _SPLIT / _SMALL (-1: unset)
struct XfPlan {
  int form = XF_PER_GEMM;
  int Bc = 1;                  // batch rows of one chunk (a forward of more is cut into chunks)
  int rows = 0;                // of a walk launch of a full chunk, with its dynamic LDS and the length of its stage table
  int64_t lds_bytes = 0;
  int n_stages = 0;
  int refusal = XF_OFF;
};
XfPlan xf_plan(const XfModel& m, const XfShape& sh, const XfDevice& dev, const XfKnobs& knobs);

// one chunk of a forward: its inputs and output, and the workspace of its stage table
struct XfChunk {
  int B, Ts, Tt;
  const float *src, *tgt, *mask, *text, *src_pad, *tgt_pad;
  const int32_t* pe_row;
  float* out;                  // (Tt, B, d_lat)
  bool same() const { return tgt == src && Ts == Tt; }
};
struct XfWalkWs {
  float *xs_e, *xt_e, *qkv, *kvm, *o, *h;
  float *slabA, *slabB, *e1, *e2, *mem, *t1, *t2, *t3;       // split-K form: slabs, the rows each LayerNorm leaves
  float *pA, *pB, *pC, *pM, *lA, *lB, *lC;                   // small-row form: pre-LayerNorm sums, the normalised rows consumers publish
};
// the workspace of a form in allocation order: alloc(n) hands out n floats (the arena; a counting stand-in where only sizes matter)
XfWalkWs xf_walk_workspace(const XfModel& m, const XfChunk& c, int form, float* (*alloc)(void*, int64_t), void* user);
void xf_walk_table(const XfModel& m, const XfChunk& c, const XfWalkWs& ws, std::vector<WalkOp>& ops);
void xf_walk_small_table(const XfModel& m, const XfChunk& c, const XfWalkWs& ws, int grid, std::vector<WalkOp>& ops);
// what the per-GEMM kernels would account for the same work: W once, X (unless still staged) and the product once
void xf_walk_account(const std::vector<WalkOp>& ops, double* flops, double* bytes);

// The network, written once for the per-kernel paths (models/transformer.py:47-68 over torch.nn.Transformer defaults: post-norm, final
// encoder / decoder LayerNorm, sequence-first).  A runner R supplies the operations: the inference runner launches the per-GEMM kernels
// (latent_transformer.cpp), the training runner also records what backward needs and draws the dropout sites in this order
// (xf_trainer.cpp).  r.layer(dec, i) is the runner's handle of a layer: its weights, and whatever else the runner keeps per layer.
template <class R>
float* xf_graph(R& r, const XfModel& m, const XfChunk& c) {
  const int Ts = c.Ts, Tt = c.Tt, Ms = Ts * c.B, Mt = Tt * c.B;
  float* xs = r.embed(0, c.src, Ts);
  float* xt = (R::kSharesEmbedding && c.same()) ? xs : r.embed(1, c.tgt, Tt);
  // nn.Transformer: src_key_padding_mask -> encoder self-attention keys, tgt_key_padding_mask -> decoder self-attention keys;
  // the cross-attention takes none (memory_key_padding_mask is not passed at models/transformer.py:64)
  for (int i = 0; i < m.enc_layers; ++i) {
    auto&& L = r.layer(false, i);
    xs = r.add_ln(L, 0, xs, r.mha(L, false, xs, Ts, xs, Ts, nullptr, c.src_pad), Ms);
    xs = r.add_ln(L, 1, xs, r.ffn(L, xs, Ms), Ms);
  }
  float* mem = r.final_ln(false, xs, Ms);
  for (int i = 0; i < m.dec_layers; ++i) {
    auto&& L = r.layer(true, i);
    xt = r.add_ln(L, 0, xt, r.mha(L, false, xt, Tt, xt, Tt, c.mask, c.tgt_pad), Mt);
    xt = r.add_ln(L, 1, xt, r.mha(L, true, xt, Tt, mem, Ts, nullptr, nullptr), Mt);
    xt = r.add_ln(L, 2, xt, r.ffn(L, xt, Mt), Mt);
  }
  return r.out(r.final_ln(true, xt, Mt), Mt);
}
