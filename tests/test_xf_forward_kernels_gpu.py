"""The forward kernels of the latent Transformer (csrc/xformer.hip) and the stages of its layer-walking launch (csrc/xf_walk.hip) one by
one against fp64, element by element.  The same kernels serve the CLIP text tower and the MiniLM sentence encoder.

Each kernel is driven alone through its operator-level hook (svg_op_xf_gemm_ex, _add_ln, _embed_post, _attention, _attention_qkv,
_embed_tokens, _embed_bert, _mean_pool_norm) and each walk stage through svg_op_xf_walk with a table of one to three stages.  The
conventions are those of tests/test_train_kernels_gpu.py, whose helpers are imported: every output buffer is filled with NaN and carries a
pad of 64 NaN rows behind it that must still be NaN afterwards (so must the columns of a wider buffer that belong to no output); every
valid element must be finite; the reference is fp64 on the same f32 inputs; every element is judged, none left out.  The worst
err / bound per kernel and data class goes through conftest.margin(..., tol=1.0, unit="err/bound").

TWO DATA CLASSES
  exact   small integers: if every term of a sum is a multiple of q and the magnitudes add up to at most 2^24 q, the f32 result is the fp64
          one in ANY order (sums_exact(), asserted per case); the bound is 0: bit equality.  Kernels with one: xf_gemm (act_in 0 / 1), the
          walk's GEMM + reduce stages, the small-row GEMM without a LayerNorm, the two embedding lookups (one or two f32 additions in a
          fixed order: bit equal to the torch f32 sum), xf_embed_post (per element one of the two f32 results the language allows: the
          multiply-add fused or not).  LayerNorm statistics, softmax and the pooling divisions round whatever the data is.
  random  unit normal data (for act_in 2 / 3 with inputs out to |x| = 8), judged by the bounds below.  e = 2^-24; a sum of n f32 terms costs
          (n + 2) e sum |a| |b| in any order (split-K slabs, wave partial sums and MFMA chains are orders of the same n terms); each further
          rounding costs e |y|; every bound is multiplied by 1.01 for the products of two of its terms.  No constant was fitted to what the
          GPU returns.  Hardware / libm functions by the project's precedents: rsqrtf at 2 ulp = 4 e (tests/test_ff_fused_gpu.py; sqrtf is
          taken the same), expf / erff at 4 ulp = 8 e (tests/test_train_kernels_gpu.py), __expf(t) as v_exp_f32 of a rounded product with
          relative error (|t| / 2 + 2) 2^-23 = (|t| + 4) e (tests/test_gemm_epilogue_gpu.py::_check_silu).

BOUNDS
  xf_gemm      y = act(x) W^T + bias + residual is ONE sum of n = K + [bias] + [residual] terms: (n + 2) e (|act(x)| |W|^T + |bias| + |res|),
               plus the activation's own error da as a perturbation of the operand: sum_k |W| da.
               act 1 (ReLU): da = 0.   act 2 (quick-GELU x / (1 + __expf(t)), t = fl(-1.702f x), the reference takes the f32 constant):
               u = e^t carries |t| e (the product's rounding) + (|t| + 4) e; 1 + u rounds once, the division once:
               da = |a| ((u / (1 + u)) (2 |t| + 4) e + 2 e).   act 3 (0.5 x (1 + erff(z)), z = fl(x * 0.70710678f)): z carries 2 e |z| (the
               constant, the product), erf'(z) = 2 / sqrt(pi) e^(-z^2); erff 8 e |erf|; the sum 1 + erf rounds once; 0.5 x is exact, the last
               product rounds once:  da = 0.5 |x| (8 e |erf| + 4 e |z| e^(-z^2) / sqrt(pi) + e |1 + erf|) + e |a|.
  xf_add_ln    z = x + r: dz = e |z| (r given).  The rest is add_ln_train's derivation in tests/test_train_kernels_gpu.py with block-sum depth
               D = ceil(d / 256) + 9:  dmean = D e mean|z| + mean(dz);  rel(rstd) = ((D + 4) / 2 + 4) e + (dmean^2 + 2 sqrt(var mean(dz^2)) +
               mean(dz^2)) / (2 (var + eps));  dxhat = rstd (dz + dmean + e |z - mean|) + |xhat| (rel(rstd) + e);
               dy = |g| dxhat + e |xhat g| + e |y|.  Mean-50 rows and constant rows (var = 0: y = b within the bound) by the same formulas.
  xf_embed_post / embed_tokens / embed_bert   exact class only (above).
  xf_attention s = q.k scale + mask + kpad: ds = (hd + 2) e |q|.|k| scale + 6 e |s0| (rsqrtf, the product, the sum) + e (|s0| + |mask| + |kpad|)
               per bias added;  delta_i = max_j (ds_ij + e |s_ij - max_i|);  P: rel = 2 delta_i + 8 e (expf) + (Tk + 2) e + 2 e (1 / sum, the
               product);  o = sum_j P v: sum_j dP |v| + (Tk + 3) e sum_j P |v|   -- `attention` of the training file without dropout.  A key
               masked with -inf has P = 0 exactly: the V rows of keys that no query of their batch row may see hold 1e30.
  xf_attention_qkv   the CLIP / BERT kernel scales q before the product, one more rounding per term: ds = (hd + 7) e |q|.|k| scale (hd + 2 for
               the sum, 1 for q scale, 4 for rsqrtf).  __expf(t_j), t_j = s_j - max: rel_j = 2 delta + (|t_j| + 4) e + sum_k P_k (|t_k| + 4) e
               (the denominator) + (T + 2) e + 2 e, plus 2^-126 absolute (a flushed subnormal);  o as above.  Causal: V of the keys past a
               cut holds 1e30, so a query before the cut that gives a future key any weight is off by ~1e26.  Padded: keys >= clamp(len, 1, T)
               hold 1e30; every query row i0 < T is written and judged.
  xf_mean_pool_norm   a = sum_{t < len} x / len: da = (len + 2) e sum|x| / len + e |a|;  sq = sum a^2 (depth D = ceil(d / 256) + 9):
               dsq = 2 sum |a| da + (D + 1) e sq;  nrm = sqrtf(sq): rel = dsq / (2 sq) + 4 e;  out = a / nrm: da / nrm + |out| (rel + e).
               len 0: exact zeros.
  WK_GEMM + WK_RED   xf_gemm's bound with n = K + [bias] + [res]; ReLU is exact.
  WK_LN        z = sum of slabs + bias + res: dz = (K + [bias] + [res] + 2) e magnitudes (no GEMM: ([bias] + [res]) e |z|); then xf_add_ln's
               formulas with D = ceil(N / 1024) + 11 (a thread folds each of its <= 3 vectors in two levels and adds them in sequence, six
               shuffle levels, three wave sums, the division).  The second norm is judged as a chain: its input error is the first's dy.
  WK_EMBED     v = x W^T + bias (dv as WK_GEMM); y = v scale + pe: scale dv + e |v scale| + e |y| (two roundings, or one fused); text channels
               the same with dv = 0.
  WK_ATTN      the stage of both walking kernels: xf_attention's bound (its score sum is another order of the same hd terms).
  WK_GEMMF     x = LN2(LN1(X)) by WK_LN's formulas with D = K / 128 + 7 (32 threads per row: K / 128 vectors in sequence, two levels inside a
               vector, five shuffle levels, the division), error dx;  p = x W^T + bias: (K + [bias] + 2) e magnitudes + sum |W| dx;
               embedding epilogue p scale + pe as WK_EMBED; ReLU exact; + res: e |y|.  Yln is judged by dx.

SHAPES AND THE PATH EACH TAKES (asserted from what the hook reports)
  xf_gemm form 1 (16-column form): (1,16,32) (15,36,40) (16,64,256) mt 1; (17,4,8) mt 2; (33,96,1024) mt 3 ksplit 2; (47,256,2048) mt 3
  ksplit 4; (5,64,4096) mt 1 ksplit 8;  K < 32 (the only way into form 1 with mt >= 4): M 48 / 64 / 90 / 128 / 176 / 250 / 336 at (20,24) ->
  mt 3 / 4 / 6 / 8 / 11 / 16 / 21, and (336,64,8) mt 21.   Form 2 (column-block form), M 48 / 49 / 64 / 90 / 128 / 170 / 250 / 336 -> mt 3 / 4 /
  4 / 6 / 8 / 11 / 16 / 21, each at (36,40) ksplit 1 with N and K tails, (64,512) ksplit 2, (100,552) ksplit 2 with a K tail (552 = 17 x 32 + 8),
  and (48,64,4096) ksplit 16.  Every case runs act_in 0..3 (random) and 0 / 1 (exact) with bias / residual null or set in rotation;
  test_gemm_cases_cover_cpu asserts that every act_in, a null and a set bias and residual appear on both forms with and without split-K.
  INSTANTIATIONS NO LEGAL (M, N, K) REACHES (test_describe_equals_the_old_rule_cpu confirms it over its grid): xf_gemm2_kernel<1> and <2>
  (form 2 needs M >= 48, i.e. mt >= 3); xf_gemm_kernel<4 .. 21> are reached only with K < 32 (K = 8, 16, 24).  Everything else is reached.
  xf_add_ln d 4 .. 3072: one to twelve values per thread.  xf_attention_qkv T > 64 reaches the second score register (key lane + 64).
  Walk: GEMM M 5 / 32 / 48 / 64 / 90 / 128 / 176 -> xf_walk_kernel<1 / 2 / 3 / 4 / 6 / 8 / 11>; LN N > 2048 reaches the third vector per
  thread; ATTN with B heads = 1408 jobs takes a second pass of the job loop on any grid up to 1407; GEMMF N = 4 / grid + 4 / 8 grid - 4 ->
  1 / 2 / 8 columns per workgroup.

The CPU half (not marked gpu) pushes a torch-f32 emulation of each kernel, in the kernel's order where order matters (block sums, split-K
slabs, the two-register key scan), through the same data and the same judges; test_judge_rejects_cpu requires every judge to reject the
defects listed in MUTATIONS."""
import ctypes
import math

import pytest
import torch

from conftest import margin
from sd_video_gen_amd import _lib
import test_train_kernels_gpu as TK
from test_train_kernels_gpu import E, F32, F64, LN_EPS, NAN, SLACK, _gen, cdiv, f32c, qmin, randint, sums_exact

gpu = pytest.mark.gpu
BIG = 1e30
HEIGHTS = (1, 2, 3, 4, 6, 8, 11, 16, 21)


class Tally(TK.Tally):
    def check(self, report):
        for cls, (r, label) in sorted(self.worst.items()):
            print("[xf_forward] %-24s %-7s worst err/bound %.3f at %s" % (self.kernel, cls, r, label))
            if report:
                margin("xf forward kernel %s, %s class" % (self.kernel, cls), r, 1.0, unit="err/bound")
            else:
                assert r < 1.0, "%s %s: err/bound %.3g at %s" % (self.kernel, cls, r, label)
            if cls == "exact":
                assert r == 0.0, "%s: the exact class is not bit-equal at %s" % (self.kernel, label)


def old_rule(M, N, K):
    """(form, mt, ksplit) as xf_gemm / xf_gemm_v2 chose them before xf_gemm_describe existed, transcribed from that code"""
    mt = next(h for h in HEIGHTS if cdiv(M, 16) <= h)
    steps, ks = cdiv(K, 32), 1
    if M >= 48 and K >= 32:
        nb = cdiv(N, 64)
        while nb * ks < 512 and steps // (ks * 2) >= 8 and ks < 16:
            ks *= 2
        return 2, mt, ks
    nb = cdiv(N, 16)
    while nb * ks < 512 and steps // (8 * ks * 2) >= 2 and ks < 8:
        ks *= 2
    return 1, mt, ks


def butterfly(s, lanes):
    """the xor-shuffle fold of the last axis (lanes wide); every lane ends with the sum"""
    idx = torch.arange(lanes)
    o = lanes // 2
    while o:
        s = s + s[..., idx ^ o]
        o //= 2
    return s


def walk_block_sum(v, drop_third=False):
    """row sums of v (M, N <= 3072) in the order of the walk's LayerNorm stage: thread t folds its vectors t, t + 256, t + 512 in two levels
    each and adds them in sequence, 64 lanes fold by xor, the four wave sums are added in order"""
    M, N = v.shape
    w = torch.zeros(M, 3072, dtype=F32)
    w[:, :N] = v
    w = w.view(M, 768, 4)
    pv = ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])).view(M, 3, 256)
    s = torch.zeros(M, 256, dtype=F32)
    for i in range(3):
        if i * 1024 < N and not (drop_third and i == 2):
            s = s + pv[:, i]
    s = butterfly(s.view(M, 4, 64), 64)[:, :, 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def small_row_sum(v):
    """row sums of v (M, K) in the order of the small-row kernel's LayerNorm: 32 threads per row, thread j folds the vectors at 4 j + 128 i"""
    M, K = v.shape
    w = v.reshape(M, K // 128, 32, 4)
    pv = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    s = torch.zeros(M, 32, dtype=F32)
    for i in range(K // 128):
        s = s + pv[:, i]
    return butterfly(s, 32)[:, 0]


def ln_f32(z, g, b, row_sum, one_pass=False):
    n = f32c(float(z.shape[1]))
    mean = row_sum(z) / n
    if one_pass:
        var = (row_sum(z * z) / n - mean * mean).clamp_min(0.0)
    else:
        t = z - mean[:, None]
        var = row_sum(t * t) / n
    rstd = torch.rsqrt(var + f32c(LN_EPS))
    return (z - mean[:, None]) * rstd[:, None] * g[None, :] + b[None, :]


def ln_ref(z, dz, g, b, D):
    """fp64 y = LN(z) g + b and its bound for an input known to dz (module docstring)"""
    mean = z.mean(1, keepdim=True)
    t = z - mean
    var = (t * t).mean(1, keepdim=True)
    v = var + float(f32c(LN_EPS))
    rstd = v ** -0.5
    dmean = D * E * z.abs().mean(1, keepdim=True) + dz.mean(1, keepdim=True)
    dz2 = (dz * dz).mean(1, keepdim=True)
    rel = ((D + 4) / 2 + 4) * E + (dmean ** 2 + 2 * (var * dz2).sqrt() + dz2) / (2 * v)
    xhat = t * rstd
    dxh = rstd * (dz + dmean + E * t.abs()) + xhat.abs() * (rel + E)
    g64, b64 = g.to(F64)[None, :], b.to(F64)[None, :]
    y = xhat * g64 + b64
    return y, g64.abs() * dxh + E * (xhat * g64).abs() + E * y.abs()


def gemm_ref(a, da, W, bias, res):
    """fp64 y = a W^T + bias + res with a known to da (a, da fp64), its bound (without the 1.01) and the magnitudes"""
    W64 = W.to(F64)
    y, mag = a @ W64.t(), a.abs() @ W64.abs().t()
    n = a.shape[1]
    for t in (bias, res):
        if t is not None:
            y, mag, n = y + t.to(F64), mag + t.to(F64).abs(), n + 1
    return y, (n + 2) * E * mag + da @ W64.abs().t(), mag


# =====================================================================================================================================
# activations on the GEMM's input
# =====================================================================================================================================
C_QG = float(f32c(1.702))
C_RS2 = f32c(0.70710678118654752)


def act_f32(x, act, mut=None):
    if act == 1:
        return x.clamp_min(0.0)
    if act == 2:
        c = f32c(1.7) if mut == "qgelu_1p7" else f32c(1.702)
        return x / (f32c(1.0) + torch.exp(-c * x))
    if act == 3:
        if mut == "gelu_tanh":
            return torch.nn.functional.gelu(x, approximate="tanh")
        return f32c(0.5) * x * (f32c(1.0) + torch.erf(x * C_RS2))
    return x


def act_ref(x, act):
    """fp64 activation of the f32 input and the bound da of what the kernel's f32 evaluation may differ by"""
    x = x.to(F64)
    if act == 1:
        return x.clamp_min(0.0), torch.zeros_like(x)
    if act == 2:
        t = -C_QG * x
        u = torch.exp(t)
        a = x / (1 + u)
        return a, a.abs() * ((u / (1 + u)) * (2 * t.abs() + 4) * E + 2 * E)
    if act == 3:
        z = x / math.sqrt(2.0)
        er = torch.erf(z)
        a = 0.5 * x * (1 + er)
        return a, 0.5 * x.abs() * (8 * E * er.abs() + 4 * E * z.abs() * torch.exp(-z * z) / math.sqrt(math.pi) + E * (1 + er).abs()) + E * a.abs()
    return x, torch.zeros_like(x)


# =====================================================================================================================================
# attention references
# =====================================================================================================================================
def heads_tbd(t, H):
    """(T, B, d) -> (B, H, T, hd)"""
    T, B, d = t.shape
    return t.reshape(T, B, H, d // H).permute(1, 2, 0, 3)


def attn_ref(kind, q, k, v, bias, bmag, nb):
    """q (B,H,Tq,hd), k, v (B,H,Tk,hd) fp64; bias: additive fp64 (B,H|1,Tq|1,Tk) with -inf entries or None, bmag the sum of the finite
    magnitudes that went into it, nb how many f32 additions built it.  -> o, bound (without the 1.01), P"""
    hd, Tk = q.shape[3], k.shape[2]
    scale = hd ** -0.5
    s0 = q @ k.transpose(2, 3) * scale
    A = q.abs() @ k.abs().transpose(2, 3) * scale
    ds = (hd + 2) * E * A + 6 * E * s0.abs() if kind == "mha" else (hd + 7) * E * A
    s = s0
    if bias is not None:
        ds = ds + nb * E * (s0.abs() + bmag)
        s = s0 + bias
    live = torch.isfinite(s)
    zero = torch.zeros_like(s)
    t = torch.where(live, s - s.amax(3, keepdim=True), zero)
    delta = torch.where(live, ds + E * t.abs(), zero).amax(3, keepdim=True)
    P = torch.softmax(s, 3)
    if kind == "mha":
        dP = P * (2 * delta + 8 * E + (Tk + 2) * E + 2 * E)
    else:
        ex = (t.abs() + 4) * E
        dP = P * (2 * delta + ex + (P * ex).sum(3, keepdim=True) + (Tk + 2) * E + 2 * E) + torch.where(live, torch.full_like(s, 2.0 ** -126), zero)
    return P @ v, dP @ v.abs() + (Tk + 3) * E * (P @ v.abs()), P


def back_tbd(o):
    B, H, T, hd = o.shape
    return o.permute(2, 0, 1, 3).reshape(T, B, H * hd)


def mha_operands(g, Tq, Tk, B, H, hd):
    """q (Tq,B,d) and k, v (Tk,B,d) as column blocks of wider NaN-filled buffers with different row strides (d + 4 and 2 d + 8)"""
    d = H * hd
    bq, bkv = torch.full((Tq, B, d + 4), NAN), torch.full((Tk, B, 2 * d + 8), NAN)
    q, k, v = bq[:, :, 4:], bkv[:, :, 4:4 + d], bkv[:, :, 4 + d:4 + 2 * d]
    for t in (q, k, v):
        t.copy_(torch.randn(t.shape, generator=g))
    return q, k, v


def mha_bias(g, Tq, Tk, B, mask_kind, pad_kind):
    """mask (Tq,Tk) or None: 'causal' (-inf above the diagonal) or 'float' (a finite bias); kpad (B,Tk) or None: -inf on some keys, key 0 always
    visible.  -> mask, kpad, dead (B,Tk): keys no query of the batch row may see"""
    mask = kpad = None
    if mask_kind == "causal":
        mask = torch.full((Tq, Tk), float("-inf")).triu(1)
    elif mask_kind == "float":
        mask = torch.randn(Tq, Tk, generator=g)
    if pad_kind:
        kpad = torch.zeros(B, Tk)
        kpad[torch.rand(B, Tk, generator=g) < 0.4] = float("-inf")
        kpad[:, 0] = 0.0
    dead = torch.zeros(B, Tk, dtype=torch.bool)
    if mask_kind == "causal":
        dead[:, Tq:] = True
    if kpad is not None:
        dead |= torch.isinf(kpad)
    return mask, kpad, dead


def mha_reference(q, k, v, mask, kpad, H):
    bias = bmag = None
    nb = (mask is not None) + (kpad is not None)
    if nb:
        B, Tq, Tk = q.shape[1], q.shape[0], k.shape[0]
        bias, bmag = torch.zeros(B, 1, Tq, Tk, dtype=F64), torch.zeros(B, 1, Tq, Tk, dtype=F64)
        for t in ([] if mask is None else [mask.to(F64)[None, None]]) + ([] if kpad is None else [kpad.to(F64)[:, None, None, :]]):
            bias = bias + t
            bmag = bmag + torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))
    o, do, _ = attn_ref("mha", heads_tbd(q.to(F64), H), heads_tbd(k.to(F64), H), heads_tbd(v.to(F64), H), bias, bmag, nb)
    return back_tbd(o), SLACK * back_tbd(do)


def mha_f32(q, k, v, mask, kpad, H):
    hd = q.shape[2] // H
    qh, kh, vh = heads_tbd(q, H), heads_tbd(k, H), heads_tbd(v, H)
    s = (qh @ kh.transpose(2, 3)) * torch.rsqrt(f32c(float(hd)))
    if mask is not None:
        s = s + mask[None, None]
    if kpad is not None:
        s = s + kpad[:, None, None, :]
    e = torch.exp(s - s.amax(3, keepdim=True))
    P = e * (f32c(1.0) / e.sum(3, keepdim=True))
    return back_tbd(P @ vh)


def qkv_split(qkv, H):
    """(B, T, 3 d) -> q, k, v (B, H, T, hd)"""
    B, T, d3 = qkv.shape
    t = qkv.reshape(B, T, 3, H, d3 // (3 * H)).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def qkv_visible(T, lens, B):
    """(B, 1, T, T) bool: causal (lens None): key j <= query i; padded: key j < clamp(len, 1, T) for every query"""
    j = torch.arange(T)
    if lens is None:
        return (j[None, :] <= j[:, None])[None, None].expand(B, 1, T, T)
    eff = lens.long().clamp(1, T)
    return (j[None, :] < eff[:, None])[:, None, None, :].expand(B, 1, T, T)


def qkv_f32(qkv, lens, H, mut=None):
    """the CLIP / BERT kernel in f32: q scaled first, keys 0..63 and 64..127 in two registers per lane, __expf, the lane sums folded by xor"""
    B, T, _ = qkv.shape
    q, k, v = qkv_split(qkv, H)
    hd = q.shape[3]
    j = torch.arange(T)
    if lens is None:
        vis = (j[None, :] <= (j[:, None] + (1 if mut == "causal_off_by_one" else 0)))[None, None].expand(B, 1, T, T)
    elif mut == "lens_unclamped":
        vis = (j[None, :] < lens.long()[:, None])[:, None, None, :].expand(B, 1, T, T)
    else:
        vis = qkv_visible(T, lens, B)
    if mut == "key64_ignored" and T > 64:
        vis = vis.clone()
        vis[..., 64] = False
    s = (q * torch.rsqrt(f32c(float(hd)))) @ k.transpose(2, 3)
    s = torch.where(vis, s, torch.full_like(s, float("-inf")))
    e = torch.where(vis, torch.exp(s - s.amax(3, keepdim=True)), torch.zeros_like(s))
    e2 = torch.zeros(B, H, T, 128)
    e2[..., :T] = e
    tot = butterfly(e2[..., :64] + e2[..., 64:], 64)[..., :1]
    P = e * (f32c(1.0) / tot)
    return (P @ v).permute(0, 2, 1, 3).reshape(B, T, -1)


def qkv_reference(qkv, lens, H):
    B, T, _ = qkv.shape
    q, k, v = (t.to(F64) for t in qkv_split(qkv, H))
    vis = qkv_visible(T, lens, B)
    bias = torch.where(vis, torch.zeros(B, 1, T, T, dtype=F64), torch.full((B, 1, T, T), float("-inf"), dtype=F64))
    o, do, _ = attn_ref("qkv", q, k, v, bias, torch.zeros_like(bias), 0)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, -1)
    return back(o), SLACK * back(do)


# =====================================================================================================================================
# The two implementations behind one interface
# =====================================================================================================================================
class Gpu(TK.Gpu):
    grid = None

    def ip(self, t):
        return None if t is None else self.up(t.to(torch.int32))

    # ---- per-kernel hooks ----
    def gemm(self, X, W, bias, res, act):
        (M, K), N = X.shape, W.shape[0]
        Y = self.out(M, N)
        path = (ctypes.c_int * 3)(-1, -1, -1)
        self.call("svg_op_xf_gemm_ex", self.up(X), self.up(W), self.up(bias), self.up(res), Y.data_ptr(), M, N, K, act, path)
        return self.take(Y, M), tuple(path)

    def add_ln(self, x, r, g, b):
        M, d = x.shape
        y = self.out(M, d)
        self.call("svg_op_xf_add_ln", self.up(x), self.up(r), self.up(g), self.up(b), y.data_ptr(), M, d, LN_EPS)
        return self.take(y, M)

    def embed_post(self, emb, pe, pe_row, text, B, T, d, scale):
        y = self.out(T * B, d)
        self.call("svg_op_xf_embed_post", self.up(emb), self.up(pe), self.ip(pe_row), self.up(text), 0 if text is None else text.shape[1], y.data_ptr(), B, T, d,
                  float(scale))
        return self.take(y, T * B, (T, B, d))

    def attn(self, q, k, v, mask, kpad, H, walk=None):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        o = self.out(Tq * B, d)
        if walk is None:
            self.call("svg_op_xf_attention", self.up(q), q.stride(1), self.up(k), self.up(v), k.stride(1), self.up(mask), self.up(kpad), o.data_ptr(), Tq, Tk, B,
                      H, d // H)
        else:
            self.walk([self.attn_stage(q, k, v, mask, kpad, H, o, bar=0)], min(176, Tq * B), walk == "small")
        return self.take(o, Tq * B, (Tq, B, d))

    def attn_qkv(self, qkv, lens, H):
        B, T, d3 = qkv.shape
        o = self.out(B * T, d3 // 3)
        self.call("svg_op_xf_attention_qkv", self.up(qkv), self.ip(lens), o.data_ptr(), B, T, H, d3 // (3 * H))
        return self.take(o, B * T, (B, T, d3 // 3))

    def embed_tokens(self, ids, tok, pos, type0, T):
        rows, (vocab, d) = ids.numel(), tok.shape
        y = self.out(rows, d)
        if type0 is None:
            self.call("svg_op_xf_embed_tokens", self.ip(ids), self.up(tok), self.up(pos), y.data_ptr(), rows, T, d, vocab)
        else:
            self.call("svg_op_xf_embed_bert", self.ip(ids), self.up(tok), self.up(pos), self.up(type0), y.data_ptr(), rows, T, d, vocab)
        return self.take(y, rows)

    def mean_pool(self, x, lens):
        B, T, d = x.shape
        o = self.out(B, d)
        self.call("svg_op_xf_mean_pool_norm", self.up(x), self.ip(lens), o.data_ptr(), B, T, d)
        return self.take(o, B)

    # ---- the walk ----
    def walk(self, stages, rows, small):
        arr = (_lib.WalkStage * len(stages))(*stages)
        info = (ctypes.c_int * 4)(0, 0, 0, 0)
        self.call("svg_op_xf_walk", arr, len(stages), rows, int(small), info)
        assert info[3] == ctypes.sizeof(_lib.WalkStage), "svg_walk_stage and its ctypes mirror differ in size"
        assert info[0] >= 8 and info[0] % 8 == 0, "grid %d" % info[0]
        Gpu.grid = info[0]
        return info

    def walk_grid(self):
        """workgroups of a walk launch on this device (from info_out of a one-stage launch)"""
        if Gpu.grid is None:
            self.small_gemmf(dict(X=torch.zeros(1, 256), W=torch.zeros(4, 256)))
        return Gpu.grid

    def up_views(self, *views):
        """device pointers of column blocks of ONE wider CPU buffer (uploaded once), and the pointer behind the buffer"""
        base = views[0]._base
        assert all(v._base is base for v in views)
        dev = base.contiguous().cuda()
        self.keep.append(dev)
        return [dev.data_ptr() + 4 * (v.storage_offset() - base.storage_offset()) for v in views] + [dev.data_ptr() + 4 * dev.numel()]

    def attn_stage(self, q, k, v, mask, kpad, H, o, bar):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        (pq, endq), (pk, pv, endk) = self.up_views(q), self.up_views(k, v)
        return _lib.WalkStage(kind=_lib.WK_ATTN, bar=bar, Tq=Tq, Tk=Tk, B=B, heads=H, hd=d // H, q_ld=q.stride(1), kv_ld=k.stride(1), q_span=(endq - pq) // 4,
                              kv_span=(endk - pk) // 4, qs=pq, ks=pk, vs=pv, mask=self.up(mask), kpad=self.up(kpad), Y=o.data_ptr())

    def walk_gemm_red(self, X, W, bias, res, relu):
        (M, K), N = X.shape, W.shape[0]
        ks = K // 128
        slab, Y = self.out(ks * M, N), self.out(M, N)
        st = [_lib.WalkStage(kind=_lib.WK_GEMM, bar=0, M=M, N=N, K=K, ld=X.stride(0), ksplit=ks, X=self.up(X), W=self.up(W), slab=slab.data_ptr()),
              _lib.WalkStage(kind=_lib.WK_RED, bar=1, M=M, N=N, ksplit=ks, relu=int(relu), slab=slab.data_ptr(), bias=self.up(bias), res=self.up(res), Y=Y.data_ptr())]
        info = self.walk(st, M, False)
        assert info[2] == next(h for h in HEIGHTS if cdiv(M, 16) <= h), "M %d ran height %d" % (M, info[2])
        self.take(slab, ks * M)
        return self.take(Y, M)

    def walk_ln(self, X, W, bias, res, g1, b1, g2, b2, want_y):
        """LN over (X W^T, 3 slabs, when X is given) + bias + res -> (Y or None, Y2 or None)"""
        M, N = (res if res is not None else X).shape[0], g1.shape[0]
        Y, Y2 = self.out(M, N), self.out(M, N)
        st, ks, slab = [], 0, None
        if X is not None:
            K = X.shape[1]
            ks = K // 128
            slab = self.out(ks * M, N)
            st.append(_lib.WalkStage(kind=_lib.WK_GEMM, bar=0, M=M, N=N, K=K, ld=X.stride(0), ksplit=ks, X=self.up(X), W=self.up(W), slab=slab.data_ptr()))
        st.append(_lib.WalkStage(kind=_lib.WK_LN, bar=len(st), M=M, N=N, ksplit=ks, slab=None if slab is None else slab.data_ptr(), bias=self.up(bias), res=self.up(res),
                                 g1=self.up(g1), b1=self.up(b1), g2=self.up(g2), b2=self.up(b2), Y=Y.data_ptr() if want_y else None,
                                 Y2=Y2.data_ptr() if g2 is not None else None, eps=LN_EPS))
        self.walk(st, M, False)
        y, y2 = self.take(Y, M), self.take(Y2, M)
        if not want_y:
            assert bool(torch.isnan(y).all()), "a null Y was written"
        if g2 is None:
            assert bool(torch.isnan(y2).all()), "a null Y2 was written"
        return (y if want_y else None), (y2 if g2 is not None else None)

    def walk_embed(self, X, W, bias, text, pe, pe_row, B, T, scale):
        (M, K), N = X.shape, W.shape[0]
        d_txt = 0 if text is None else text.shape[1]
        ks = K // 128
        slab, Y = self.out(ks * M, N), self.out(T * B, N + d_txt)
        st = [_lib.WalkStage(kind=_lib.WK_GEMM, bar=0, M=M, N=N, K=K, ld=X.stride(0), ksplit=ks, X=self.up(X), W=self.up(W), slab=slab.data_ptr()),
              _lib.WalkStage(kind=_lib.WK_EMBED, bar=1, M=M, N=N, ksplit=ks, slab=slab.data_ptr(), bias=self.up(bias), Y=Y.data_ptr(), pe=self.up(pe),
                             pe_row=self.ip(pe_row), text=self.up(text), d_txt=d_txt, T=T, B=B, scale=float(scale))]
        self.walk(st, M, False)
        return self.take(Y, T * B, (T, B, N + d_txt))

    def gemmf_stage(self, c, X_ptr, bar, reuse=False, W=None, outs=None):
        """one WK_GEMMF stage from the case dict c (small_cases); Y (and Yln) buffers are appended to outs"""
        X, W = c["X"], (c["W"] if W is None else W)
        (M, K), N = X.shape, W.shape[0]
        ldy = N + c.get("ldy_extra", 0)
        Y = self.out(M, ldy)
        Yln = self.out(M, K) if c.get("yln") and not reuse else None
        res, pe = c.get("res"), c.get("pe")
        outs.append((Y, Yln, M, N))
        return _lib.WalkStage(kind=_lib.WK_GEMMF, bar=bar, M=M, N=N, K=K, ld=X.stride(0), X=X_ptr, W=self.up(W), bias=self.up(c.get("bias")), res=self.up(res),
                              Y=Y.data_ptr(), g1=self.up(c.get("g1")), b1=self.up(c.get("b1")), g2=self.up(c.get("g2")), b2=self.up(c.get("b2")), eps=LN_EPS,
                              relu=int(c.get("relu", 0)), pe=self.up(pe), pe_row=self.ip(c.get("pe_row")), scale=float(c.get("scale", 0.0)), B=c.get("B", 0),
                              T=c.get("T", 0), perm=int(c.get("perm", 0)), ldy=ldy, ld_res=(res.stride(0) if res is not None else (pe.stride(0) if pe is not None else 0)),
                              reuse_x=int(reuse), Yln=None if Yln is None else Yln.data_ptr())

    def small_gemmf(self, c):
        """-> {"Y": .., "Yln": .. (if asked), "Y1": .. (the reuse_x stage, if W1 is given), "o": .. (an attention stage in front, if attn is given)}"""
        outs, st, o = [], [], None
        if "attn" in c:
            q, k, v, mask, kpad, H = c["attn"]
            o = self.out(q.shape[0] * q.shape[1], q.shape[2])
            st.append(self.attn_stage(q, k, v, mask, kpad, H, o, bar=0))
        xp = self.up(c["X"])
        st.append(self.gemmf_stage(c, xp, bar=len(st), outs=outs))
        if "W1" in c:
            st.append(self.gemmf_stage(c, xp, bar=0, reuse=True, W=c["W1"], outs=outs))
        self.walk(st, 8, True)
        got = {}
        for name, (Y, Yln, M, N) in zip(("Y", "Y1"), outs):
            y = self.take(Y, M)
            assert bool(torch.isnan(y[:, N:]).all()), "columns past N of a wider Y were written"
            got[name] = y[:, :N]
            if Yln is not None:
                got["Yln"] = self.take(Yln, M)
        if o is not None:
            q = c["attn"][0]
            got["o"] = self.take(o, q.shape[0] * q.shape[1], tuple(q.shape))
        return got


class Emu:
    """torch f32 on the CPU, in the kernels' order where order matters; mut: one defect (MUTATIONS)"""
    grid = 256

    def __init__(self, mut=None):
        self.mut = mut

    def walk_grid(self):
        return self.grid

    def gemm(self, X, W, bias, res, act):
        (M, K), N = X.shape, W.shape[0]
        form, mt, ks = old_rule(M, N, K)
        A = act_f32(X, act, self.mut)
        steps = cdiv(K, 32)
        live = steps - 1 if self.mut == "gemm_drop_last_step" and steps > 1 else steps
        cols = lambda sts: [k for st in sts if st < live for k in range(st * 32, min(K, st * 32 + 32))]
        dot = lambda idx: A[:, idx] @ W[:, idx].t() if idx else torch.zeros(M, N)
        slabs = []
        for kz in range(ks):
            if form == 1:          # eight waves interleave over the steps of the slab and meet in LDS in order
                part = [dot(cols(range(kz * 8 + w, steps, 8 * ks))) for w in range(8)]
                s = part[0]
                for p in part[1:]:
                    s = s + p
            else:                   # a contiguous range of steps per slab, one chain
                per = cdiv(steps, ks)
                s = dot(cols(range(kz * per, min(steps, kz * per + per))))
            slabs.append(s)
        if self.mut == "gemm_slab_twice" and ks > 1 and K % 32:
            slabs.append(slabs[-1])
        y = slabs[0]
        for s in slabs[1:]:
            y = y + s
        if bias is not None:
            y = y + (bias * float(ks) if self.mut == "gemm_bias_per_slab" else bias)[None, :]
        if res is not None and not (self.mut == "gemm_res_skipped_split" and ks > 1):
            y = y + res
        return y, (form, mt, ks)

    def add_ln(self, x, r, g, b):
        return ln_f32(x if r is None else x + r, g, b, TK.block_sum, self.mut == "ln_one_pass_var")

    def embed_post(self, emb, pe, pe_row, text, B, T, d, scale):
        if text is not None and self.mut == "text_off_by_one_clip":
            text = text.roll(1, 0)
        return TK.embed_formula(emb, pe, pe_row, text, B, T, d, scale, 0, 0, 0.0, fused=False)

    def attn(self, q, k, v, mask, kpad, H, walk=None):
        return mha_f32(q, k, v, mask, kpad, H)

    def attn_qkv(self, qkv, lens, H):
        return qkv_f32(qkv, lens, H, self.mut)

    def embed_tokens(self, ids, tok, pos, type0, T):
        rows = ids.numel()
        y = tok[ids.long().clamp(0, tok.shape[0] - 1)] + pos[torch.arange(rows) % T]
        return y if type0 is None else y + type0[None, :]

    def mean_pool(self, x, lens):
        B, T, d = x.shape
        out = torch.zeros(B, d)
        for b in range(B):
            n = int(lens[b].clamp(0, T))
            a = torch.zeros(d)
            for t in range(n):
                a = a + x[b, t]
            a = a / torch.maximum(f32c(float(n)), f32c(1e-9))
            nrm = torch.maximum(torch.sqrt(TK.block_sum((a * a)[None, :])[0]), f32c(1e-12))
            out[b] = a / nrm
        return out

    # ---- the walk ----
    @staticmethod
    def slab_sum(X, W):
        """the split-K GEMM stage + the consumer's slab sum: 128-wide K slices, added ascending"""
        acc = torch.zeros(X.shape[0], W.shape[0])
        for kz in range(X.shape[1] // 128):
            acc = acc + X[:, kz * 128:(kz + 1) * 128] @ W[:, kz * 128:(kz + 1) * 128].t()
        return acc

    def walk_gemm_red(self, X, W, bias, res, relu):
        y = self.slab_sum(X, W)
        if bias is not None:
            y = y + bias[None, :]
        if res is not None:
            y = y + res
        return y.clamp_min(0.0) if relu else y

    def walk_ln(self, X, W, bias, res, g1, b1, g2, b2, want_y):
        z = self.slab_sum(X, W) if X is not None else torch.zeros(res.shape if res is not None else (1, g1.shape[0]))
        if bias is not None:
            z = z + bias[None, :]
        if res is not None:
            z = z + res
        rs = lambda v: walk_block_sum(v, self.mut == "ln_third_vector_dropped")
        y = ln_f32(z, g1, b1, rs, self.mut == "ln_one_pass_var")
        y2 = None if g2 is None else ln_f32(y, g1 if self.mut == "ln2_gamma_from_first" else g2, b2, rs)
        return (y if want_y else None), y2

    def walk_embed(self, X, W, bias, text, pe, pe_row, B, T, scale):
        v = self.slab_sum(X, W) + bias[None, :]
        if text is not None and self.mut == "text_off_by_one_clip":
            text = text.roll(1, 0)
        return TK.embed_formula(v, pe, pe_row, text, B, T, v.shape[1] + (0 if text is None else text.shape[1]), scale, 0, 0, 0.0, fused=False)

    def small_gemmf(self, c):
        X = c["X"]
        M, K = X.shape
        got = {}
        x = X
        if c.get("perm") and self.mut != "perm_not_applied":      # rows in flight are (t, b), the launch's inputs (b, t)
            r = torch.arange(M)
            x = X[(r % c["B"]) * c["T"] + r // c["B"]]
        if c.get("g1") is not None:
            x = ln_f32(x, c["g1"], c["b1"], small_row_sum)
            if c.get("g2") is not None:
                x = ln_f32(x, c["g1"] if self.mut == "ln2_gamma_from_first" else c["g2"], c["b2"], small_row_sum)
            if c.get("yln"):
                got["Yln"] = x
        for name, W in (("Y", c["W"]),) + ((("Y1", c["W1"]),) if "W1" in c else ()):
            v = torch.zeros(M, W.shape[0])
            for w in range(4):       # a wave takes a quarter of K in two halves; the eight partial sums meet in LDS in order
                h = [x[:, w * (K // 4) + hh * (K // 8):w * (K // 4) + (hh + 1) * (K // 8)] @ W[:, w * (K // 4) + hh * (K // 8):w * (K // 4) + (hh + 1) * (K // 8)].t()
                     for hh in range(2)]
                v = v + (h[0] + h[1])
            if c.get("bias") is not None:
                v = v + c["bias"][None, :]
            if c.get("pe") is not None:
                rows = (torch.arange(M) % c["B"]) if c.get("pe_row") is None else c["pe_row"].long()[torch.arange(M) % c["B"]]
                v = v * f32c(c["scale"]) + c["pe"][rows]
            if c.get("relu"):
                v = v.clamp_min(0.0)
            if c.get("res") is not None:
                v = v + c["res"]
            got[name] = v
        if "attn" in c:
            got["o"] = mha_f32(*c["attn"])
        return got


# =====================================================================================================================================
# xf_gemm
# =====================================================================================================================================
# (M, N, K, form, mt, ksplit): what each shape is expected to launch
GEMM_CASES = ([(1, 16, 32, 1, 1, 1), (15, 36, 40, 1, 1, 1), (16, 64, 256, 1, 1, 1), (17, 4, 8, 1, 2, 1), (33, 96, 1024, 1, 3, 2), (47, 256, 2048, 1, 3, 4),
               (5, 64, 4096, 1, 1, 8)]
              + [(M, 20, 24, 1, mt, 1) for M, mt in ((48, 3), (64, 4), (90, 6), (128, 8), (176, 11), (250, 16), (336, 21))] + [(336, 64, 8, 1, 21, 1)]
              + [(M, N, K, 2, mt, ks) for M, mt in ((48, 3), (49, 4), (64, 4), (90, 6), (128, 8), (170, 11), (250, 16), (336, 21))
                 for (N, K, ks) in ((36, 40, 1), (64, 512, 2), (100, 552, 2))]
              + [(48, 64, 4096, 2, 3, 16)])
COMBOS = [(False, False), (True, False), (False, True), (True, True)]       # (bias, residual)


def gemm_runs():
    """(case, class, act_in, bias, residual): every case runs act_in 0..3 on random data and 0 / 1 on integers, bias / residual in rotation"""
    for i, c in enumerate(GEMM_CASES):
        for act in range(4):
            yield (c, "random", act) + COMBOS[(i + act) % 4]
        for act in range(2):
            yield (c, "exact", act) + COMBOS[(i + act + 2) % 4]


def gemm_data(cls, M, N, K, act, has_b, has_r):
    g = _gen(21, M, N, K, act, cls == "exact")
    if cls == "exact":
        X, W = randint(g, -4, 4, (M, K)), randint(g, -4, 4, (N, K))
        bias, res = randint(g, -64, 64, (N,)), randint(g, -64, 64, (M, N))
    else:
        X, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        if act >= 2:                                                         # the quick-GELU tail and the erff saturation
            X.view(-1)[::5] = torch.linspace(-8.0, 8.0, X.view(-1)[::5].numel())
    return X, W, (bias if has_b else None), (res if has_r else None)


def sweep_gemm(impl, tally):
    for (M, N, K, form, mt, ks), cls, act, has_b, has_r in gemm_runs():
        X, W, bias, res = gemm_data(cls, M, N, K, act, has_b, has_r)
        label = "M %d N %d K %d form %d mt %d ksplit %d act %d%s%s" % (M, N, K, form, mt, ks, act, " bias" if has_b else "", " res" if has_r else "")
        y, path = impl.gemm(X, W, bias, res, act)
        assert path == (form, mt, ks), "%s: the launch reports %s" % (label, path)
        a, da = act_ref(X, act)
        want, bound, mag = gemm_ref(a, da, W, bias, res)
        if cls == "exact":
            assert sums_exact(mag, min(qmin(X) * qmin(W), qmin(bias, res))), "the exact class's premise"
            tally.add("exact", label, {"y": y}, {"y": (want, 0.0)})
        else:
            tally.add("random", label, {"y": y}, {"y": (want, SLACK * bound)})


# =====================================================================================================================================
# xf_add_ln
# =====================================================================================================================================
ADD_LN_D = [4, 252, 256, 260, 384, 2048, 2432, 3072]


def sweep_add_ln(impl, tally):
    for d in ADD_LN_D:
        for has_r in (False, True):
            g = _gen(22, d, has_r)
            x = TK.ln_rows(g, 3, d)
            r = torch.randn(3, d, generator=g) if has_r else None
            if has_r:
                r[2] = 0.0                                                   # the constant row stays constant
            gam, bet = 1 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
            y = impl.add_ln(x, r, gam, bet)
            z = x.to(F64) if r is None else x.to(F64) + r.to(F64)
            want, dy = ln_ref(z, E * z.abs() if has_r else torch.zeros_like(z), gam, bet, cdiv(d, 256) + 9)
            tally.add("random", "d %d%s" % (d, " r" if has_r else ""), {"y": y}, {"y": (want, SLACK * dy)})
            assert float((want[2] - bet.to(F64)).abs().max()) <= float(dy[2].max()), "a constant row: the reference is beta within the bound"


# =====================================================================================================================================
# xf_embed_post
# =====================================================================================================================================
def sweep_embed_post(impl, tally):
    B, T, d = 3, 5, 40
    for d_txt in (0, 8):
        for pe_row in (None, torch.tensor([63, 5, 5], dtype=torch.int32)):
            g = _gen(23, d_txt, pe_row is None)
            emb, pe = torch.randn(B * T, d - d_txt, generator=g), torch.randn(64, d, generator=g)
            text = torch.randn(B, d_txt, generator=g) if d_txt else None
            scale = math.sqrt(d)
            y = impl.embed_post(emb, pe, pe_row, text, B, T, d, scale)
            a, b = (TK.embed_formula(emb, pe, pe_row, text, B, T, d, scale, 0, 0, 0.0, fused) for fused in (False, True))
            want = torch.where(y == b, b, a)                                 # per element one of the two roundings the language allows
            tally.add("exact", "d_txt %d%s" % (d_txt, "" if pe_row is None else " pe_row"), {"y": y}, {"y": (want.to(F64), 0.0)})


# =====================================================================================================================================
# xf_attention and the walk's attention stage
# =====================================================================================================================================
MHA_T = [(1, 1), (6, 6), (16, 17), (32, 32), (5, 32)]
MHA_HD = [4, 16, 80, 256]


def mha_case(Tq, Tk, hd, mask_kind, pad_kind, B=3, H=2):
    g = _gen(24, Tq, Tk, hd, len(mask_kind or ""), pad_kind, B, H)
    q, k, v = mha_operands(g, Tq, Tk, B, H, hd)
    mask, kpad, dead = mha_bias(g, Tq, Tk, B, mask_kind, pad_kind)
    v[dead.t()[:, :, None].expand(Tk, B, H * hd)] = BIG
    label = "Tq %d Tk %d hd %d B %d H %d mask %s%s" % (Tq, Tk, hd, B, H, mask_kind, " kpad" if pad_kind else "")
    return label, (q, k, v, mask, kpad, H)


def sweep_mha(impl, tally, walk=None):
    for (Tq, Tk) in MHA_T:
        for hd in MHA_HD:
            for mask_kind in (None, "causal", "float"):
                for pad_kind in (False, True):
                    label, ops = mha_case(Tq, Tk, hd, mask_kind, pad_kind)
                    o = impl.attn(*ops, walk=walk)
                    tally.add("random", label, {"o": o}, {"o": mha_reference(*ops)})


def sweep_walk_attn_jobs(impl, tally):
    """B heads = 1408 jobs of Tq = Tk = 1: more jobs than workgroups, so a workgroup takes a second job (and the barrier in front of it)"""
    grid = impl.walk_grid()
    assert grid <= 1407, "the walk launches %d workgroups: 1408 attention jobs no longer reach the second pass of the job loop; enlarge this case" % grid
    label, ops = mha_case(1, 1, 4, None, False, B=176, H=8)
    tally.add("random", label + " (grid %d)" % grid, {"o": impl.attn(*ops, walk="walk")}, {"o": mha_reference(*ops)})


# =====================================================================================================================================
# xf_attention_causal / xf_attention_padded
# =====================================================================================================================================
QKV_T = [1, 2, 63, 64, 65, 77, 128]
QKV_HD = [1, 20, 64]


def sweep_qkv(impl, tally):
    B, H = 2, 2
    for T in QKV_T:
        for hd in QKV_HD:
            g = _gen(25, T, hd)
            base = torch.randn(B, T, 3 * H * hd, generator=g)
            vcols = slice(2 * H * hd, 3 * H * hd)
            cut = 63 if T > 64 else (T - 1) // 2                             # causal: V of the keys past the cut is 1e30
            runs = [("causal", None, None)] + ([("causal cut %d" % cut, None, cut + 1)] if T > 1 else [])
            runs += [("lens %s" % (ls,), torch.tensor(ls, dtype=torch.int32), "lens") for ls in ([1, 5], [64, 65], [T, 0], [T + 3, 1])]
            for name, lens, dead_from in runs:
                qkv = base.clone()
                if dead_from == "lens":
                    for b in range(B):
                        qkv[b, int(lens[b].clamp(1, T)):, vcols] = BIG
                elif dead_from is not None:
                    qkv[:, dead_from:, vcols] = BIG
                o = impl.attn_qkv(qkv, lens, H)
                tally.add("random", "T %d hd %d %s" % (T, hd, name), {"o": o}, {"o": qkv_reference(qkv, lens, H)})


# =====================================================================================================================================
# xf_embed_tokens / xf_embed_bert / xf_mean_pool_norm
# =====================================================================================================================================
def sweep_lookup(impl, tally):
    T, vocab = 7, 11
    for d in (4, 384, 772):
        for bert in (False, True):
            g = _gen(26, d, bert)
            ids = torch.randint(0, vocab, (2 * T,), generator=g).to(torch.int32)
            ids[3], ids[9], ids[0], ids[13] = -1, vocab + 5, 0, vocab - 1
            tok, pos, type0 = torch.randn(vocab, d, generator=g), torch.randn(T, d, generator=g), (torch.randn(d, generator=g) if bert else None)
            y = impl.embed_tokens(ids, tok, pos, type0, T)
            want = tok[ids.long().clamp(0, vocab - 1)] + pos[torch.arange(2 * T) % T]
            want = want if type0 is None else want + type0[None, :]
            tally.add("exact", "%s d %d" % ("bert" if bert else "tokens", d), {"y": y}, {"y": (want.to(F64), 0.0)})


def sweep_pool(impl, tally):
    B, T = 4, 9
    lens = torch.tensor([0, 1, 9, 12], dtype=torch.int32)
    for d in (4, 384, 1000):
        g = _gen(27, d)
        x = torch.randn(B, T, d, generator=g)
        out = impl.mean_pool(x, lens)
        D = cdiv(d, 256) + 9
        want, bound = torch.zeros(B, d, dtype=F64), torch.zeros(B, d, dtype=F64)
        for b in range(B):
            n = int(lens[b].clamp(0, T))
            if n == 0:
                continue
            xs = x[b, :n].to(F64)
            a = xs.sum(0) / n
            da = (n + 2) * E * xs.abs().sum(0) / n + E * a.abs()
            sq = (a * a).sum()
            dsq = 2 * (a.abs() * da).sum() + (D + 1) * E * sq
            nrm = sq.sqrt()
            want[b] = a / nrm
            bound[b] = da / nrm + want[b].abs() * (dsq / (2 * sq) + 4 * E + E)
        tally.add("random", "d %d" % d, {"out": out}, {"out": (want, SLACK * bound)})
        assert bool((out[0] == 0).all()), "len 0 must give exact zeros"


# =====================================================================================================================================
# walk stages: GEMM + reduce, LayerNorm, embedding
# =====================================================================================================================================
def wide(t, extra=12):
    """t as the leading columns of a wider NaN-filled buffer (row stride > columns)"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), NAN)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def sweep_walk_gemm(impl, tally):
    n = 0
    for M in (5, 32, 48, 64, 90, 128, 176):
        for (N, K) in ((128, 128), (256, 384)):
            for cls in ("exact", "random"):
                has_b, has_r, relu = [(0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1), (1, 1, 0), (0, 0, 1)][n % 6]
                n += 1
                g = _gen(28, M, N, K, cls == "exact")
                if cls == "exact":
                    X, W, bias, res = randint(g, -4, 4, (M, K)), randint(g, -4, 4, (N, K)), randint(g, -64, 64, (N,)), randint(g, -64, 64, (M, N))
                else:
                    X, W, bias, res = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
                X, bias, res = wide(X), (bias if has_b else None), (res if has_r else None)
                label = "M %d N %d K %d%s%s%s" % (M, N, K, " bias" if has_b else "", " res" if has_r else "", " relu" if relu else "")
                y = impl.walk_gemm_red(X, W, bias, res, relu)
                want, bound, mag = gemm_ref(X.to(F64), torch.zeros(M, K, dtype=F64), W, bias, res)
                want = want.clamp_min(0.0) if relu else want
                if cls == "exact":
                    assert sums_exact(mag, 1.0), "the exact class's premise"
                tally.add(cls, label, {"y": y}, {"y": (want, 0.0 if cls == "exact" else SLACK * bound)})


WALK_LN_N = [128, 1024, 2048, 2176, 3072]


def sweep_walk_ln(impl, tally):
    n = 0
    for N in WALK_LN_N:
        for fed in (True, False):                                              # by a GEMM stage of three slabs, or no slabs at all
            for (second, want_y) in ((False, True), (True, True), (True, False)):
                has_b = n % 2 == 1
                n += 1
                g = _gen(29, N, fed, second, want_y)
                M, K = 3, 384
                res = TK.ln_rows(g, M, N)
                X = W = None
                if fed:
                    X, W = wide(0.25 * torch.randn(M, K, generator=g)), torch.randn(N, K, generator=g)
                    X[2] = 0.0                                                 # the constant row stays constant (without a bias)
                bias = 0.5 * torch.randn(N, generator=g) if has_b else None
                g1, b1, g2, b2 = (1 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g), 1 + 0.2 * torch.randn(N, generator=g),
                                  0.1 * torch.randn(N, generator=g))
                if not second:
                    g2 = b2 = None
                y, y2 = impl.walk_ln(X, W, bias, res, g1, b1, g2, b2, want_y)
                if fed:
                    z, dz, _ = gemm_ref(X.to(F64), torch.zeros(M, K, dtype=F64), W, bias, res)
                else:
                    z = res.to(F64) + (0 if bias is None else bias.to(F64)[None, :])
                    dz = (E * z.abs()) if has_b else torch.zeros_like(z)
                D = cdiv(N, 1024) + 11
                w1, d1 = ln_ref(z, dz, g1, b1, D)
                got, ref = {}, {}
                if want_y:
                    got["y"], ref["y"] = y, (w1, SLACK * d1)
                if second:
                    w2, d2 = ln_ref(w1, d1, g2, b2, D)
                    got["y2"], ref["y2"] = y2, (w2, SLACK * d2)
                tally.add("random", "N %d %s%s%s%s" % (N, "3 slabs" if fed else "no slabs", " bias" if has_b else "", " + second norm" if second else "",
                                                        "" if want_y else " (Y null)"), got, ref)


def sweep_walk_embed(impl, tally):
    B, T, d_img, K = 3, 6, 128, 256
    for d_txt in (0, 128):
        for pe_row in (None, torch.tensor([63, 5, 5], dtype=torch.int32)):
            g = _gen(30, d_txt, pe_row is None)
            d = d_img + d_txt
            X, W, bias = wide(torch.randn(B * T, K, generator=g)), torch.randn(d_img, K, generator=g) / 16, torch.randn(d_img, generator=g)
            text = torch.randn(B, d_txt, generator=g) if d_txt else None
            pe, scale = torch.randn(64, d, generator=g), math.sqrt(d)
            y = impl.walk_embed(X, W, bias, text, pe, pe_row, B, T, scale)
            v, dv, _ = gemm_ref(X.to(F64), torch.zeros(B * T, K, dtype=F64), W, bias, None)
            if d_txt:
                v = torch.cat([v, text.to(F64)[:, None, :].expand(B, T, d_txt).reshape(B * T, d_txt)], 1)
                dv = torch.cat([dv, torch.zeros(B * T, d_txt, dtype=F64)], 1)
            rows = torch.arange(B) if pe_row is None else pe_row.long()
            s64 = float(f32c(scale))
            vs = v.reshape(B, T, d).permute(1, 0, 2) * s64
            want = vs + pe.to(F64)[rows][None]
            bound = dv.reshape(B, T, d).permute(1, 0, 2) * s64 + E * vs.abs() + E * want.abs()
            tally.add("random", "d_txt %d%s" % (d_txt, "" if pe_row is None else " pe_row"), {"y": y}, {"y": (want, SLACK * bound)})


# =====================================================================================================================================
# the small-row launch: WK_GEMMF
# =====================================================================================================================================
def small_cases(grid):
    """[(label, class, case dict)]: the plain product at every (M, K) and columns-per-workgroup count, then each epilogue / prologue feature"""
    out = []
    mk = lambda *key: _gen(31, *key)
    for M in (1, 6, 8):
        for K in (256, 768, 2048):
            for cls in ("exact", "random"):
                g = mk(M, K, cls == "exact")
                X, W = (randint(g, -4, 4, (M, K)), randint(g, -4, 4, (4, K))) if cls == "exact" else (torch.randn(M, K, generator=g), torch.randn(4, K, generator=g))
                out.append(("M %d K %d N 4" % (M, K), cls, dict(X=wide(X, 4) if M == 6 else X, W=W)))
    for N in (grid + 4, 8 * grid - 4):
        for cls in ("exact", "random"):
            g = mk(N, cls == "exact")
            X, W, b = ((randint(g, -4, 4, (8, 256)), randint(g, -4, 4, (N, 256)), randint(g, -64, 64, (N,))) if cls == "exact" else
                       (torch.randn(8, 256, generator=g), torch.randn(N, 256, generator=g), torch.randn(N, generator=g)))
            out.append(("M 8 K 256 N %d bias" % N, cls, dict(X=X, W=W, bias=b, ldy_extra=4)))
    M, K, N = 6, 768, grid + 4
    g = mk(7)
    X, W, W1 = TK.ln_rows(g, M, K), torch.randn(N, K, generator=g), torch.randn(12, K, generator=g)
    ln = lambda: dict(zip(("g1", "b1", "g2", "b2"), (1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), 1 + 0.2 * torch.randn(K, generator=g),
                                                    0.1 * torch.randn(K, generator=g))))
    l1 = {k: v for k, v in ln().items() if k in ("g1", "b1")}
    bias, res = torch.randn(N, generator=g), wide(torch.randn(M, N, generator=g), 8)
    pe = wide(torch.randn(64, N, generator=g), 4)
    out.append(("LN1 + bias", "random", dict(X=X, W=W, bias=bias, **l1)))
    out.append(("LN1 + LN2 + Yln + relu", "random", dict(X=wide(X, 4), W=W, relu=1, yln=1, **ln())))
    out.append(("bias + relu + res (ld_res > N)", "random", dict(X=X, W=W, bias=bias, relu=1, res=res)))
    out.append(("embedding epilogue: pe_row, perm", "random", dict(X=X, W=W, bias=bias, pe=pe, pe_row=torch.tensor([63, 5], dtype=torch.int32), scale=math.sqrt(N), B=2, T=3,
                                                                 perm=1)))
    out.append(("embedding epilogue: rows b", "random", dict(X=X, W=W, bias=bias, pe=pe, scale=math.sqrt(N), B=2, T=3)))
    out.append(("LN1 + Yln, then a reuse_x stage", "random", dict(X=X, W=W, W1=W1, yln=1, **l1)))
    out.append(("an attention stage in front", "random", dict(X=X, W=W, bias=bias, attn=mha_case(6, 6, 16, "causal", True)[1], **l1)))
    return out


def small_reference(cls, c):
    X = c["X"]
    M, K = X.shape
    x = X.to(F64)
    if c.get("perm"):
        r = torch.arange(M)
        x = x[(r % c["B"]) * c["T"] + r // c["B"]]
    dx = torch.zeros_like(x)
    ref = {}
    if c.get("g1") is not None:
        D = K // 128 + 7
        x, dx = ln_ref(x, dx, c["g1"], c["b1"], D)
        if c.get("g2") is not None:
            x, dx = ln_ref(x, dx, c["g2"], c["b2"], D)
        if c.get("yln"):
            ref["Yln"] = (x, SLACK * dx)
    for name, W in (("Y", c["W"]),) + ((("Y1", c["W1"]),) if "W1" in c else ()):
        y, dy, mag = gemm_ref(x, dx, W, c.get("bias"), None)
        if c.get("pe") is not None:
            rows = (torch.arange(M) % c["B"]) if c.get("pe_row") is None else c["pe_row"].long()[torch.arange(M) % c["B"]]
            ys = y * float(f32c(c["scale"]))
            y, dy = ys + c["pe"].to(F64)[rows], dy * float(f32c(c["scale"])) + E * ys.abs() + E * (ys + c["pe"].to(F64)[rows]).abs()
        if c.get("relu"):
            y = y.clamp_min(0.0)
        if c.get("res") is not None:
            y = y + c["res"].to(F64)
            dy = dy + E * y.abs()
        if cls == "exact":
            assert sums_exact(mag, 1.0) and c.get("g1") is None, "the exact class's premise"
        ref[name] = (y, 0.0 if cls == "exact" else SLACK * dy)
    if "attn" in c:
        ref["o"] = mha_reference(*c["attn"])
    return ref


def sweep_small(impl, tally):
    for label, cls, c in small_cases(impl.walk_grid()):
        tally.add(cls, label, impl.small_gemmf(c), small_reference(cls, c))


# =====================================================================================================================================
SWEEPS = {"xf_gemm": sweep_gemm, "xf_add_ln": sweep_add_ln, "xf_embed_post": sweep_embed_post, "xf_attention": sweep_mha, "xf_attention_qkv": sweep_qkv,
          "xf_embed_tokens / bert": sweep_lookup, "xf_mean_pool_norm": sweep_pool}
WALK_SWEEPS = {"walk GEMM + RED": sweep_walk_gemm, "walk LN": sweep_walk_ln, "walk EMBED": sweep_walk_embed,
               "walk ATTN": lambda impl, tally: sweep_mha(impl, tally, walk="walk"), "walk ATTN second job": sweep_walk_attn_jobs, "walk small GEMMF": sweep_small}
ALL = dict(SWEEPS, **WALK_SWEEPS)


def run(impl, name):
    t = Tally(name)
    ALL[name](impl, t)
    return t


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------
def test_describe_equals_the_old_rule_cpu():
    """xf_gemm_describe (what xf_gemm now launches from) against the rule it replaced, over a grid of legal shapes; and which
    instantiations the grid reaches.  The grid of a launch is (ceil(N / 16 | 64), ksplit) and the slabs ksplit M N floats: functions of the
    path alone, so equal paths are equal launches."""
    reached = {}
    Ns = [4, 16, 20, 36, 64, 96, 100, 128, 256, 512, 1024, 2048, 4096, 8192, 32768]
    Ks = [8, 16, 24, 32, 40, 64, 256, 512, 552, 1024, 2048, 4096, 8192, 16384]
    for M in range(1, 337):
        for N in Ns:
            for K in Ks:
                p = _lib.xf_gemm_describe(M, N, K)
                assert p == old_rule(M, N, K), "(%d, %d, %d): describe %s, the old rule %s" % (M, N, K, p, old_rule(M, N, K))
                reached.setdefault(p[:2], set()).add(K)
    for c in GEMM_CASES:
        assert _lib.xf_gemm_describe(*c[:3]) == c[3:] == old_rule(*c[:3]), c
    assert {(2, 1), (2, 2)}.isdisjoint(reached), "form 2 needs M >= 48"
    assert all(max(reached[(1, mt)]) < 32 for mt in HEIGHTS if mt >= 4), "form 1 with mt >= 4 only with K < 32"
    assert set(reached) == {(1, mt) for mt in HEIGHTS} | {(2, mt) for mt in HEIGHTS if mt >= 3}
    assert {c[3:5] for c in GEMM_CASES} == set(reached), "the GPU cases reach every reachable instantiation"
    assert {1, 2, 4, 8} <= {c[5] for c in GEMM_CASES if c[3] == 1} and {1, 2, 16} <= {c[5] for c in GEMM_CASES if c[3] == 2}


def test_gemm_cases_cover_cpu():
    """every act_in, a null and a set bias, a null and a set residual: on both forms, with and without split-K; the exact class on both too"""
    seen = {}
    for (M, N, K, form, mt, ks), cls, act, has_b, has_r in gemm_runs():
        seen.setdefault((form, ks > 1, cls), set()).update({("act", act), ("bias", has_b), ("res", has_r)})
    full = {("act", a) for a in range(4)} | {("bias", False), ("bias", True), ("res", False), ("res", True)}
    for form in (1, 2):
        for split in (False, True):
            assert seen[(form, split, "random")] == full, (form, split)
            assert seen[(form, split, "exact")] == full - {("act", 2), ("act", 3)}, (form, split)


@pytest.mark.parametrize("kernel", list(ALL))
def test_emulation_cpu(kernel):
    """the f32 emulation of each kernel passes its judge on every case and class: the bounds are not tighter than an honest f32 implementation"""
    run(Emu(), kernel).check(report=False)


# defect -> the sweep whose judge must reject it
MUTATIONS = {"gemm_drop_last_step": "xf_gemm", "gemm_slab_twice": "xf_gemm", "gemm_bias_per_slab": "xf_gemm", "gemm_res_skipped_split": "xf_gemm",
             "gelu_tanh": "xf_gemm", "qgelu_1p7": "xf_gemm", "key64_ignored": "xf_attention_qkv", "causal_off_by_one": "xf_attention_qkv",
             "lens_unclamped": "xf_attention_qkv", "ln_one_pass_var": "xf_add_ln", "ln2_gamma_from_first": "walk LN", "ln_third_vector_dropped": "walk LN",
             "perm_not_applied": "walk small GEMMF", "text_off_by_one_clip": "xf_embed_post"}
# defects that change no integer sum (an activation's constant): only the random class can see them
RANDOM_ONLY = {"gelu_tanh", "qgelu_1p7"}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judge_rejects_cpu(mut):
    """each defect of the emulation is outside its judge (the sound emulation is inside: test_emulation_cpu); a defect that every class of the
    kernel can see is rejected in every class that has a case with the feature"""
    t = run(Emu(mut), MUTATIONS[mut])
    rej = t.rejected()
    print("[xf_forward] mutation %-26s %s" % (mut, {c: "%.3g" % t.worst[c][0] for c in rej}))
    assert rej.get("random", rej.get("exact")), "the judge of %s accepts the defect %s" % (MUTATIONS[mut], mut)
    if mut.startswith("gemm_"):
        assert rej["exact"], "the exact class of xf_gemm accepts the defect %s" % mut
    if mut == "ln_one_pass_var":
        assert run(Emu(mut), "walk LN").rejected()["random"], "the judge of the walk's LayerNorm accepts a one-pass variance"
    if mut == "text_off_by_one_clip":
        assert run(Emu(mut), "walk EMBED").rejected()["random"], "the judge of the walk's embedding accepts text channels of the wrong clip"


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", list(SWEEPS))
def test_kernel_against_fp64(ctx, kernel):
    run(Gpu(ctx), kernel).check(report=True)


@gpu
@pytest.mark.parametrize("stage", list(WALK_SWEEPS))
def test_walk_stage_against_fp64(ctx, stage):
    """a walk that is unavailable on the test machine is a failure (svg_op_xf_walk returns an error), not a skip"""
    run(Gpu(ctx), stage).check(report=True)


@gpu
def test_refusals(ctx):
    """every check of a hook: the call returns non-zero, the outputs stay NaN, and a valid call on the same context afterwards is right.
    Every buffer is sized for the shape requested: nothing depends on the guard for memory safety."""
    impl = Gpu(ctx)
    nan = lambda *s: torch.full(s, NAN, device="cuda", dtype=F32)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=F32)
    i32 = lambda *v: torch.tensor(v, device="cuda", dtype=torch.int32)
    P = lambda t: t.data_ptr()
    untouched = lambda *ts: all(bool(torch.isnan(t).all()) for t in ts)
    path = (ctypes.c_int * 3)()
    # xf_gemm: act_in 4, K % 8, N % 4, M = 337, null operands
    for (M, N, K, act) in ((5, 16, 32, 4), (5, 16, 36, 0), (5, 18, 32, 0), (337, 16, 32, 0), (5, 16, 32, -1)):
        X, W, Y = rnd(M, K), rnd(N, K), nan(M, N)
        assert impl.refused("svg_op_xf_gemm_ex", P(X), P(W), None, None, P(Y), M, N, K, act, path) and untouched(Y), (M, N, K, act)
    X, W, Y = rnd(5, 32), rnd(16, 32), nan(5, 16)
    assert impl.refused("svg_op_xf_gemm_ex", None, P(W), None, None, P(Y), 5, 16, 32, 0, path) and untouched(Y)
    assert impl.refused("svg_op_xf_gemm_ex", P(X), P(W), None, None, None, 5, 16, 32, 0, path)
    # xf_add_ln: d = 3073, null gamma
    x, g, b, y = rnd(3, 3073), rnd(3073), rnd(3073), nan(3, 3073)
    assert impl.refused("svg_op_xf_add_ln", P(x), None, P(g), P(b), P(y), 3, 3073, LN_EPS) and untouched(y)
    assert impl.refused("svg_op_xf_add_ln", P(x), None, None, P(b), P(y), 3, 3072, LN_EPS) and untouched(y)
    # xf_embed_post: text channels without text, batch row 64 without pe_row (a 64-row table), null pe
    emb, pe, y = rnd(65 * 2, 8), rnd(64, 8), nan(65 * 2, 8)
    assert impl.refused("svg_op_xf_embed_post", P(emb), P(pe), None, None, 4, P(y), 2, 2, 8, 1.0) and untouched(y)
    assert impl.refused("svg_op_xf_embed_post", P(emb), P(pe), None, None, 0, P(y), 65, 2, 8, 1.0) and untouched(y)
    assert impl.refused("svg_op_xf_embed_post", P(emb), None, None, None, 0, P(y), 2, 2, 8, 1.0) and untouched(y)
    # xf_attention: T = 33, a row stride below heads * hd, null v
    q, k, v, o = rnd(33, 1, 8), rnd(33, 1, 8), rnd(33, 1, 8), nan(33, 1, 8)
    assert impl.refused("svg_op_xf_attention", P(q), 8, P(k), P(v), 8, None, None, P(o), 33, 4, 1, 1, 8) and untouched(o)
    assert impl.refused("svg_op_xf_attention", P(q), 8, P(k), P(v), 8, None, None, P(o), 4, 33, 1, 1, 8) and untouched(o)
    assert impl.refused("svg_op_xf_attention", P(q), 4, P(k), P(v), 8, None, None, P(o), 4, 4, 1, 1, 8) and untouched(o)
    assert impl.refused("svg_op_xf_attention", P(q), 8, P(k), None, 8, None, None, P(o), 4, 4, 1, 1, 8) and untouched(o)
    # xf_attention_qkv: T = 129, hd = 65, T = 0 — causal and padded
    qkv, o, lens = rnd(129, 3 * 65), nan(129, 65), i32(1)
    for ln in (None, P(lens)):
        assert impl.refused("svg_op_xf_attention_qkv", P(qkv), ln, P(o), 1, 129, 1, 8) and untouched(o)
        assert impl.refused("svg_op_xf_attention_qkv", P(qkv), ln, P(o), 1, 4, 1, 65) and untouched(o)
        assert impl.refused("svg_op_xf_attention_qkv", P(qkv), ln, P(o), 1, 0, 1, 8) and untouched(o)
    # the embedding lookups: d % 4, null table;  pooling: null lens
    ids, tok, pos, y = i32(0, 1), rnd(4, 8), rnd(2, 8), nan(2, 8)
    assert impl.refused("svg_op_xf_embed_tokens", P(ids), P(tok), P(pos), P(y), 2, 2, 6, 4) and untouched(y)
    assert impl.refused("svg_op_xf_embed_bert", P(ids), P(tok), P(pos), P(pos), P(y), 2, 2, 6, 4) and untouched(y)
    assert impl.refused("svg_op_xf_embed_bert", P(ids), P(tok), P(pos), None, P(y), 2, 2, 8, 4) and untouched(y)
    assert impl.refused("svg_op_xf_mean_pool_norm", P(tok), None, P(y), 2, 2, 8) and untouched(y)
    # the walk: no stages, 177 rows, head dim 6, a small-row stage in the split-K launch, a GEMM the tiles do not fit, batch row 64 of the table
    info = (ctypes.c_int * 4)()
    q, o = rnd(4, 1, 24), nan(4, 1, 24)
    att = lambda hd: _lib.WalkStage(kind=_lib.WK_ATTN, Tq=4, Tk=4, B=1, heads=1, hd=hd, q_ld=24, kv_ld=24, q_span=96, kv_span=96, qs=P(q), ks=P(q), vs=P(q), Y=P(o))
    one = lambda s: (_lib.WalkStage * 1)(s)
    assert impl.refused("svg_op_xf_walk", one(att(8)), 0, 4, 0, info) and impl.refused("svg_op_xf_walk", one(att(8)), 1, 177, 0, info)
    assert impl.refused("svg_op_xf_walk", one(att(6)), 1, 4, 0, info) and impl.refused("svg_op_xf_walk", None, 1, 4, 0, info) and untouched(o)
    X, W, Y, slab = rnd(4, 256), rnd(128, 256), nan(4, 128), nan(2 * 4, 128)
    gf = _lib.WalkStage(kind=_lib.WK_GEMMF, M=4, N=128, K=256, ld=256, ldy=128, X=P(X), W=P(W), Y=P(Y))
    assert impl.refused("svg_op_xf_walk", one(gf), 1, 4, 0, info) and untouched(Y)
    gm = _lib.WalkStage(kind=_lib.WK_GEMM, M=4, N=128, K=192, ld=256, ksplit=1, X=P(X), W=P(W), slab=P(slab))
    assert impl.refused("svg_op_xf_walk", one(gm), 1, 4, 0, info) and untouched(slab)
    pe, yy = rnd(64, 128), nan(65, 128)
    em = (_lib.WalkStage * 2)(_lib.WalkStage(kind=_lib.WK_GEMM, M=65, N=128, K=128, ld=128, ksplit=1, X=P(rnd(65, 128)), W=P(W), slab=P(nan(65, 128))),
                              _lib.WalkStage(kind=_lib.WK_EMBED, bar=1, M=65, N=128, ksplit=1, slab=P(slab), bias=P(pe), Y=P(yy), pe=P(pe), B=65, T=1, scale=1.0))
    assert impl.refused("svg_op_xf_walk", em, 2, 65, 0, info) and untouched(yy)
    # a valid call of each family afterwards, judged as in the sweeps
    t = Tally("after a refusal")
    X, W, bias, res = gemm_data("random", 15, 36, 40, 3, True, True)
    a, da = act_ref(X, 3)
    want, bound, _ = gemm_ref(a, da, W, bias, res)
    t.add("random", "xf_gemm", {"y": impl.gemm(X, W, bias, res, 3)[0]}, {"y": (want, SLACK * bound)})
    label, ops = mha_case(6, 6, 16, "causal", True)
    t.add("random", "xf_attention", {"o": impl.attn(*ops)}, {"o": mha_reference(*ops)})
    t.add("random", "walk ATTN", {"o": impl.attn(*ops, walk="walk")}, {"o": mha_reference(*ops)})
    t.check(report=False)
