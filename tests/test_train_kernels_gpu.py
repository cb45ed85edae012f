"""The training-step kernels of the latent Transformer (csrc/xf_train.hip) one by one against fp64, element by element.

Each kernel is driven alone through its operator-level hook (svg_op_xf_*): the backward GEMMs, ReLU + dropout, the training LayerNorm
and its backward, the training attention and its backward, the embedding pair and the criterion.  Every output buffer is filled with NaN
and carries a pad of 64 NaN rows behind it that must still be NaN afterwards; the reference is fp64 on the same f32 inputs; every element
is judged, none left out.  The worst err / bound per kernel and data class goes through conftest.margin(..., tol=1.0, unit="err/bound").

TWO DATA CLASSES
  exact   small integers (or multiples of a power of two): if every term of a sum is a multiple of q and the magnitudes add up to at most
          2^24 q, every partial sum is representable and the f32 result is the fp64 one in ANY order (sums_exact(), checked per case).
          The bound is 0: bit equality.  Kernels with one: xf_gemm_tn, xf_gemm_nn + xf_nn_finish (gate scale 2 = 1 / (1 - 0.5)),
          ln_bwd_params (dgamma / dbeta), relu_drop, embed_post_bwd.  LayerNorm statistics, softmax and the criterion's divisions round
          whatever the data is: they have the random class only.
  random  unit-scale normal data, judged by the bounds below: e = 2^-24, "abs" = the same contraction on magnitudes (the fp64 reference
          run on absolute values).  A sum of n f32 terms costs (n + 2) e sum |a| |b| in any order; each further rounding costs e |y|.
          Every bound is multiplied by 1.01 for the products of two of its terms.  No constant here was fitted to what the GPU returns.

BOUNDS (random class)
  xf_gemm_tn   dW: (M + 2) e |dY|^T |X|, accumulate: + e |dW|.   db: (M + 2) e sum_m |dY|, accumulate: + e |db|.
  xf_gemm_nn   v = dY W: (N + 2) e |dY| |W| whatever the split count (the slabs are partial sums of the same N terms);
               gate: (.) gate_scale + e |v gate_scale| where the gate is open, exactly 0 where it is shut;  add: + e |out|.
  relu_drop    bit equal to max(h, 0) * mask: one f32 product.
  add_ln_train z = x + r mask: dz = e |r mask| + e |z| (two roundings, or one if the compiler contracts them; the bound takes two).
               A block sum of d values: a thread adds its ceil(d / 256) values in sequence, six shuffle levels, three adds of the wave
               sums, the division: depth D = ceil(d / 256) + 9.   A = mean |z|.
               dmean = D e A + mean(dz)
               var^ is taken about mean^: sum (z - mean^)^2 = sum (z - mean)^2 + d (mean^ - mean)^2 exactly, and the input error moves
               the variance by at most 2 sqrt(var mean(dz^2)) + mean(dz^2); each term of the sum carries 3 e (difference, two for the
               square), the sum D e, the sum with eps e;  rsqrtf 2 ulp = 4 e (as tests/test_ff_fused_gpu.py takes it):
               rel(rstd) = ((D + 4) / 2 + 4) e + (dmean^2 + 2 sqrt(var mean(dz^2)) + mean(dz^2)) / (2 (var + eps))
               dxhat = rstd (dz + dmean + e |z - mean|) + |xhat| (rel(rstd) + e)        dy = |g| dxhat + e |xhat g| + e |y|
               Rows with mean 50 and spread 1 and constant rows (var = 0: xhat is dmean rstd at most) are judged by the same formulas.
  ln_bwd       gd = dy g (e |gd|);  m1 = mean gd: dm1 = (D + 1) e mean |gd|;  m2 = mean gd xhat: dm2 = (D + 2) e mean |gd xhat|
               dz = rstd (gd - m1 - xhat m2):  rstd [e |gd| + dm1 + |xhat| dm2 + e |xhat m2| + 2 e (|gd| + |m1| + |xhat m2|)] + e |dz|
               dz_drop = dz mask: the above times mask + e |dz mask|
               dgamma = sum_m dy xhat: (M + 2) e sum |dy xhat|;  dbeta = sum_m dy: (M + 2) e sum |dy|;  accumulate: + e |y|.
               Chained on the forward kernel's own xhat / rstd the reference stays the fp64 one and the bounds carry the forward's
               dxhat and rel(rstd): dm2 += mean(|gd| dxhat), dz += rstd |m2| dxhat + |dz| rel(rstd), dgamma += sum |dy| dxhat.
  attention    s = q.k scale + mask: ds = (hd + 2) e |q|.|k| scale + 6 e |s|  (rsqrtf(hd) at 2 ulp = 4 e, the product, the sum);
               delta_i = max_j (ds_ij + e |s_ij - max_i|);   P: rel = 2 delta_i + 8 e (expf) + (Tk + 2) e (the row sum) + 2 e (1 / sum, product)
               o = sum_j P mask v:  sum_j dP mask |v| + (Tk + 3) e sum_j P mask |v|
               backward:  dPd = dO.v mask: (hd + 2) e |dO|.|v| mask + e |dPd|;   pd = P mask: e |pd|
               dot_i = sum_j dPd P: sum_j d(dPd) P + (Tk + 2) e sum_j |dPd| P
               dS = P (dPd - dot) scale: P scale [d(dPd) + d(dot) + e |dPd - dot|] + 7 e |dS|   -- the cancellation, on magnitudes
               dq = sum_j dS k: sum_j d(dS) |k| + (Tk + 2) e sum_j |dS| |k|;  dk likewise over i with q;
               dv = sum_i pd dO: (Tq + 3) e sum_i |pd| |dO|.
               Chained on the forward kernel's P (error dP above): d(pd) += dP mask, d(dot) += sum_j |dPd| dP, d(dS) += dP |dPd - dot| scale.
               expf / logf / powf: the HIP math documentation is not on the build machine, so 4 ulp = 8 e each, as the issue sets.
  embed_post   y = (v scale + pe) mask: three f32 operations, of which the compiler may contract the first two into one fma; per element
               the result must be one of the two (the unfused replay in torch f32, the fused one through fp64).  Backward:
               de = dy mask scale, two products, bit equal to the torch f32 replay.
  criterion    reference: oracle/train_oracle.criterion in fp64 with autograd.  dpred per element, with inv_n = 1 / ((Tt - t0) B D):
               12 e (|g_mse| + |g_l1| + sum |gdl terms| + |g_nce|)   (at most six roundings inside a component, five sums joining them, one more for
               the contrastive kernel's +=)  +  w_gdl inv_n sum d(mag) with d(au) = e (|gx| + |gy| + |u|) for u = |gx| - |gy|, mag = 1 |
               2 au | alpha au^(alpha - 1) (powf: 8 e + |alpha - 1| d(au) / au)  +  2 mag w_gdl inv_n for a term whose |u| <= d(au) (its sign is
               rounding)  +  the contrastive part:  logits l = <g, p> / tau: dl = 7 e |g|.|p| / tau + e |l - max|, delta = max_j dl;
               rho1 = 2 delta + (hw + 12) e + 8 e |log se| + e |lse| + e |l_ii - lse| + 8 e   (the diagonal softmax of direction 1)
               rho2 = 2 delta2 + (hw + 12) e                                                 (the weights of direction 2)
               d(d_c) = |g_c| (sm_ii rho1 + 2 e) + (rho2 + (hw + 5) e) sum_j sm2_j |gt_jc| + 3 e (|.| + |.| + |g_c|), times w / (2 tau R).
               Losses: a row sum has depth ceil(D / 256) + 9, the rows are added in sequence: (ceil(D / 256) + rows + 16) e on magnitudes
               (+ 3 e per term); the contrastive loss additionally 2 (delta + (hw + 12) e + 8 e |log se| + e |lse|) per position.
               A GDL or contrastive term of weight 0 is not evaluated by the kernels: its reported loss is 0 (the oracle does the same
               for the contrastive term), and the reference follows.

The CPU half (not marked gpu) pushes a torch-f32 emulation of each kernel, in the kernel's order where order matters (the LayerNorm block
sums, the split-K slabs, the row batches), through the same data and the same judges, and test_judge_rejects_cpu requires every judge to
reject the defects listed in MUTATIONS."""
import ctypes
import math

import pytest
import torch

from conftest import margin
from oracle import train_oracle as TR
from sd_video_gen_amd import _lib

gpu = pytest.mark.gpu
E = 2.0 ** -24
PAD = 64
F64, F32 = torch.float64, torch.float32
NAN = float("nan")
SEED = 0x1234ABCD5678EF01
SLACK = 1.01
LN_EPS = 1e-5


def cdiv(a, b):
    return (a + b - 1) // b


def f32c(v):
    return torch.tensor(v, dtype=F32)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def draw(cls, g, shape, lo=-4, hi=4):
    return randint(g, lo, hi, shape) if cls == "exact" else torch.randn(shape, generator=g)


def quantum(t):
    """per element of an fp64 tensor the largest power of two that divides it (inf for 0)"""
    m, ex = torch.frexp(t)
    iv = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (iv & -iv).to(F64)
    return torch.where(t == 0, torch.full_like(t, float("inf")), torch.ldexp(low, ex - 53))


def qmin(*ts):
    return min([float("inf")] + [float(quantum(t.to(F64)).min()) for t in ts if t is not None and t.numel()])


def sums_exact(absdot, q):
    """a sum of terms that are all multiples of q is exact in f32, in any order, if the sum of their magnitudes stays within 2^24 q"""
    return bool((absdot <= 2.0 ** 24 * q).all())


def ratio(got, want, bound):
    """worst err / bound of one output; a bound of 0 asks for equality; inf for a non-finite or missing element"""
    o = got.detach().cpu().to(F64)
    assert o.shape == want.shape, (o.shape, want.shape)
    if o.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(o).all()):
        return float("inf")
    err = (o - want).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    return float(torch.where(err == 0, torch.zeros_like(err), err / b).max())


class Tally:
    """the worst err / bound per data class of one kernel, with the case it came from"""

    def __init__(self, kernel):
        self.kernel, self.worst = kernel, {}

    def add(self, cls, label, got, ref):
        """got: {name: tensor}; ref: {name: (want, bound)}"""
        assert set(got) == set(ref), (sorted(got), sorted(ref))
        for k in ref:
            r = ratio(got[k], *ref[k])
            if r >= self.worst.get(cls, (-1.0, ""))[0]:
                self.worst[cls] = (r, "%s %s" % (label, k))

    def check(self, report):
        for cls, (r, label) in sorted(self.worst.items()):
            print("[train_kernels] %-22s %-7s worst err/bound %.3f at %s" % (self.kernel, cls, r, label))
            if report:
                margin("train kernel %s, %s class" % (self.kernel, cls), r, 1.0, unit="err/bound")
            else:
                assert r < 1.0, "%s %s: err/bound %.3g at %s" % (self.kernel, cls, r, label)
            if cls == "exact":
                assert r == 0.0, "%s: the exact class is not bit-equal at %s" % (self.kernel, label)

    def rejected(self):
        return {cls: r >= 1.0 for cls, (r, _) in self.worst.items()}


# ---- dropout masks: the counter-based generator of xf_train.hip restated on 64-bit integers -----------------------------------------
M64 = (1 << 64) - 1


def _s64(c):
    c &= M64
    return c - (1 << 64) if c >= (1 << 63) else c


def drop_mask_cpu(seed, site, p, n):
    if p == 0.0:
        return torch.ones(n)
    shr32 = lambda t: (t >> 32) & 0xFFFFFFFF
    x = torch.arange(n, dtype=torch.int64) * _s64(0xD1B54A32D192ED03) + _s64(seed ^ (0x9E3779B97F4A7C15 * (site + 1)))
    for _ in range(2):
        x = (x ^ shr32(x)) * _s64(0xD6E8FEB86659FD93)
    x = x ^ shr32(x)
    u = ((x >> 40) & 0xFFFFFF).to(F32) * f32c(1.0 / 16777216.0)
    return torch.where(u >= f32c(p), f32c(1.0) / (f32c(1.0) - f32c(p)), f32c(0.0))


def nn_splits(N, K):
    """xf_gemm_nn_splits (the GPU tests assert it against what the hook reports)"""
    z = max(1, 512 // cdiv(K, 64))
    while z > 1 and cdiv(N, z) < 64:
        z >>= 1
    return z


def nn_chunk(N, Z):
    return cdiv(cdiv(N, Z), 64) * 64


def block_sum(v):
    """row sums of v (M, d <= 3072) in the order of the 256-thread blocks: a thread adds the columns t, t + 256, ..., the 64 lanes fold by
    xor 32 .. 1, the four wave sums are added in order"""
    M, d = v.shape
    w = torch.zeros(M, 3072, dtype=F32)
    w[:, :d] = v
    w = w.view(M, 12, 256)
    s = torch.zeros(M, 256, dtype=F32)
    for i in range(cdiv(d, 256)):
        s = s + w[:, i]
    s = s.view(M, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    s = s[:, :, 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


# =====================================================================================================================================
# The two implementations behind one interface: the HIP kernels through their hooks, and the torch-f32 emulation (with its defects)
# =====================================================================================================================================
def stream():
    return torch.cuda.current_stream().cuda_stream


class Gpu:
    mut = None

    def __init__(self, ctx):
        self.ctx, self.lib, self.keep = ctx, ctx.lib, []
        self.splits_seen = {}

    # -- buffers --
    def up(self, t):
        """device pointer of a CPU tensor that may be a column slice of a wider buffer (the whole buffer is uploaded)"""
        if t is None:
            return None
        base = t._base if t._base is not None else t
        dev = base.contiguous().cuda()
        self.keep.append(dev)
        return dev.data_ptr() + (t.storage_offset() - base.storage_offset()) * t.element_size()

    def out(self, rows, cols, init=None):
        """(rows + PAD, cols) of NaN (rows < `rows`: init, when given)"""
        o = torch.full((rows + PAD, cols), NAN, device="cuda", dtype=F32)
        if init is not None:
            o[:rows] = init.reshape(rows, cols).cuda()
        return o

    def take(self, o, rows, shape=None):
        torch.cuda.synchronize()
        assert bool(torch.isnan(o[rows:]).all()), "the NaN pad behind an output was written"
        r = o[:rows].cpu()
        return r if shape is None else r.reshape(shape)

    def call(self, name, *args):
        self.ctx.check(getattr(self.lib, name)(self.ctx.h, *args, stream()), name)

    def refused(self, name, *args):
        rc = getattr(self.lib, name)(self.ctx.h, *args, stream())
        torch.cuda.synchronize()
        return rc != 0

    # -- kernels --
    def drop_mask(self, seed, site, p, n):
        return self.ctx.dropout_mask(seed, site, p, n).cpu()

    def gemm_tn(self, dY, X, old_dW, old_db, accumulate, want_db):
        (M, N), K = dY.shape, X.shape[1]
        dW = self.out(N, K, old_dW if accumulate else None)
        db = self.out(1, N, old_db if accumulate and want_db else None)
        self.call("svg_op_xf_gemm_tn", self.up(dY), dY.stride(0), self.up(X), X.stride(0), dW.data_ptr(), db.data_ptr() if want_db else None,
                  M, N, K, int(accumulate))
        dbo = self.take(db, 1)[0]
        if not want_db:
            assert bool(torch.isnan(dbo).all()), "a null db: the bias buffer was written"
        return self.take(dW, N), (dbo if want_db else None)

    def gemm_nn(self, dY, W, gate, gate_scale, add, alias):
        (M, N), K = dY.shape, W.shape[1]
        out = self.out(M, K, add if alias else None)
        z = ctypes.c_int(-1)
        add_p = out.data_ptr() if alias else self.up(add)
        self.call("svg_op_xf_gemm_nn", self.up(dY), dY.stride(0), self.up(W), out.data_ptr(), M, N, K, self.up(gate), float(gate_scale), add_p,
                  ctypes.byref(z))
        self.splits_seen[(N, K)] = z.value
        return self.take(out, M)

    def relu_drop(self, h, seed, site, p):
        rr = torch.full((h.numel() + PAD,), NAN, device="cuda", dtype=F32)
        self.call("svg_op_xf_relu_drop", self.up(h), rr.data_ptr(), h.numel(), seed, site, float(p))
        torch.cuda.synchronize()
        assert bool(torch.isnan(rr[h.numel():]).all())
        return rr[:h.numel()].cpu().reshape(h.shape)

    def add_ln(self, x, r, seed, site, p, g, b):
        M, d = x.shape
        y, xh, rs = self.out(M, d), self.out(M, d), self.out(M, 1)
        self.call("svg_op_xf_add_ln_train", self.up(x), self.up(r), seed, site, float(p), self.up(g), self.up(b), y.data_ptr(), xh.data_ptr(),
                  rs.data_ptr(), M, d, LN_EPS)
        return self.take(y, M), self.take(xh, M), self.take(rs, M)[:, 0]

    def ln_bwd(self, dy, xhat, rstd, g, seed, site, p, old_dg, old_db, accumulate, want_drop):
        M, d = dy.shape
        dz, dzd = self.out(M, d), self.out(M, d)
        dg, db = self.out(1, d, old_dg if accumulate else None), self.out(1, d, old_db if accumulate else None)
        self.call("svg_op_xf_ln_bwd", self.up(dy), self.up(xhat), self.up(rstd), self.up(g), dz.data_ptr(), dzd.data_ptr() if want_drop else None,
                  seed, site, float(p), dg.data_ptr(), db.data_ptr(), M, d, int(accumulate))
        dzd_o = self.take(dzd, M)
        if not want_drop:
            assert bool(torch.isnan(dzd_o).all()), "a null dz_drop: the buffer was written"
        return self.take(dz, M), (dzd_o if want_drop else None), self.take(dg, 1)[0], self.take(db, 1)[0]

    def attn_fwd(self, q, k, v, mask, heads, seed, site, p):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        o, P = self.out(Tq * B, d), self.out(B * heads * Tq, Tk)
        self.call("svg_op_xf_attention_train", self.up(q), q.stride(1), self.up(k), self.up(v), k.stride(1), self.up(mask), o.data_ptr(),
                  P.data_ptr(), Tq, Tk, B, heads, d // heads, seed, site, float(p))
        return self.take(o, Tq * B, (Tq, B, d)), self.take(P, B * heads * Tq, (B, heads, Tq, Tk))

    def attn_bwd(self, dout, q, k, v, P, heads, seed, site, p, packed):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        if packed:       # dq | . | . of a (Tq, B, 3d) buffer, . | dk | dv of a (Tk, B, 3d) buffer: the other columns stay NaN
            bq, bkv = self.out(Tq * B, 3 * d), self.out(Tk * B, 3 * d)
            pq, pk, pv, lq, lk = bq.data_ptr(), bkv.data_ptr() + 4 * d, bkv.data_ptr() + 8 * d, 3 * d, 3 * d
        else:
            bq, bkv = self.out(Tq * B, d), self.out(Tk * B, 2 * d)
            pq, pk, pv, lq, lk = bq.data_ptr(), bkv.data_ptr(), bkv.data_ptr() + 4 * d, d, 2 * d
        self.call("svg_op_xf_attention_bwd", self.up(dout), self.up(q), q.stride(1), self.up(k), self.up(v), k.stride(1), self.up(P), pq, lq, pk, pv,
                  lk, Tq, Tk, B, heads, d // heads, seed, site, float(p))
        oq, okv = self.take(bq, Tq * B), self.take(bkv, Tk * B)
        if packed:
            assert bool(torch.isnan(oq[:, d:]).all()) and bool(torch.isnan(okv[:, :d]).all()), "columns outside dq / dk / dv were written"
            oq, okv = oq[:, :d], okv[:, d:]
        return oq.reshape(Tq, B, d), okv[:, :d].reshape(Tk, B, d), okv[:, d:].reshape(Tk, B, d)

    def embed_fwd(self, emb, pe, pe_row, text, B, T, d, scale, seed, site, p):
        d_txt = 0 if text is None else text.shape[1]
        y = self.out(T * B, d)
        self.call("svg_op_xf_embed_post_train", self.up(emb), self.up(pe), self.up(pe_row), self.up(text), d_txt, y.data_ptr(), B, T, d,
                  float(scale), seed, site, float(p))
        return self.take(y, T * B, (T, B, d))

    def embed_bwd(self, dy, B, T, d, d_img, scale, seed, site, p):
        de = self.out(B * T, d_img)
        self.call("svg_op_xf_embed_post_bwd", self.up(dy), de.data_ptr(), B, T, d, d_img, float(scale), seed, site, float(p))
        return self.take(de, B * T)

    def criterion(self, pred, expected, t0, fh, fw, w):
        Tt, B, D = pred.shape
        dp = self.out(Tt * B, D)
        losses = (ctypes.c_float * 5)(*([NAN] * 5))
        self.call("svg_op_xf_criterion", self.up(pred), self.up(expected), dp.data_ptr(), losses, Tt, B, D, t0, fh, fw, w.get("w_mse", 0.0),
                  w.get("w_l1", 0.0), w.get("w_gdl", 0.0), float(w.get("alpha", 1)), w.get("w_contrastive", 0.0), w.get("temperature", 0.07))
        return torch.tensor(list(losses), dtype=F32), self.take(dp, Tt * B, (Tt, B, D))


class Emu:
    """torch f32 on the CPU; mut: one defect (MUTATIONS)"""

    def __init__(self, mut=None):
        self.mut = mut

    def drop_mask(self, seed, site, p, n):
        return drop_mask_cpu(seed, site, p, n)

    def gemm_tn(self, dY, X, old_dW, old_db, accumulate, want_db):
        (M, N), K = dY.shape, X.shape[1]
        acc = torch.zeros(N, K)
        last = ((M - 1) // 32) * 32
        for m0 in range(0, M, 32):                                     # the row batches of the kernel
            if self.mut == "tn_drop_last_batch" and m0 == last:
                continue
            acc = acc + dY[m0:m0 + 32].t() @ X[m0:m0 + 32]
        db = None
        if want_db:                                                     # lane group l holds the rows m = l mod 4, groups added in order
            grp = [dY[l::4].sum(0) if l < M else torch.zeros(N) for l in range(4)]
            if self.mut == "tn_db_lane_group":
                grp[3] = torch.zeros(N)
            db = ((grp[0] + grp[1]) + grp[2]) + grp[3]
        if accumulate and self.mut != "tn_acc_ignores_old":
            acc = acc + old_dW
            db = None if db is None else db + old_db
        if self.mut == "tn_edge_col" and K > 1:
            acc[:, K - 1] = acc[:, K - 2]
        return acc, db

    def gemm_nn(self, dY, W, gate, gate_scale, add, alias):
        (M, N), K = dY.shape, W.shape[1]
        Z = nn_splits(N, K)
        chunk = nn_chunk(N, Z)
        v = None
        for z in range(Z):                                              # slabs added z ascending
            lo, hi = z * chunk, min(N, (z + 1) * chunk)
            if lo < N:
                slab = dY[:, lo:hi] @ W[lo:hi]
            else:
                slab = torch.full((M, K), 3.0) if self.mut == "nn_stale_slab" else torch.zeros(M, K)
            v = slab if v is None else v + slab
        if self.mut == "nn_edge_col" and K > 1:
            v[:, K - 1] = v[:, K - 2]
        if gate is not None:
            open_ = gate >= 0 if self.mut == "nn_gate_ge" else gate > 0
            v = torch.where(open_, v * f32c(gate_scale), torch.zeros(()))
        return v if add is None else v + add

    def relu_drop(self, h, seed, site, p):
        return torch.clamp_min(h, 0.0) * drop_mask_cpu(seed, site, p, h.numel()).reshape(h.shape)

    def add_ln(self, x, r, seed, site, p, g, b):
        M, d = x.shape
        z = x if r is None else x + r * drop_mask_cpu(seed, site, p, M * d).reshape(M, d)
        mean = block_sum(z) / f32c(float(d))
        if self.mut == "ln_one_pass_var":
            var = (block_sum(z * z) / f32c(float(d)) - mean * mean).clamp_min(0.0)
        else:
            t = z - mean[:, None]
            var = block_sum(t * t) / f32c(float(d))
        rstd = torch.rsqrt(var + f32c(LN_EPS))
        xhat = (z - mean[:, None]) * rstd[:, None]
        return xhat * g[None, :] + b[None, :], xhat, rstd

    def ln_bwd(self, dy, xhat, rstd, g, seed, site, p, old_dg, old_db, accumulate, want_drop):
        M, d = dy.shape
        gd = dy * g[None, :]
        m1 = block_sum(gd) / f32c(float(d))
        m2 = block_sum(gd * xhat) / f32c(float(d))
        if self.mut == "ln_bwd_no_m2":
            m2 = torch.zeros_like(m2)
        dz = rstd[:, None] * (gd - m1[:, None] - xhat * m2[:, None])
        dzd = dz * drop_mask_cpu(seed, site, p, M * d).reshape(M, d) if want_drop else None
        sg = [((dy * xhat)[w::4].sum(0) if w < M else torch.zeros(d)) for w in range(4)]          # wave w takes the rows m = w mod 4
        sb = [(dy[w::4].sum(0) if w < M else torch.zeros(d)) for w in range(4)]
        dg, db = ((sg[0] + sg[1]) + sg[2]) + sg[3], ((sb[0] + sb[1]) + sb[2]) + sb[3]
        if accumulate:
            dg, db = old_dg + dg, old_db + db
        return dz, dzd, dg, db

    @staticmethod
    def _heads(t, heads):
        T, B, d = t.shape
        return t.reshape(T, B, heads, d // heads).permute(1, 2, 0, 3)          # (B, H, T, hd)

    def attn_fwd(self, q, k, v, mask, heads, seed, site, p):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        hd = d // heads
        qh, kh, vh = self._heads(q, heads), self._heads(k, heads), self._heads(v, heads)
        s = (qh @ kh.transpose(2, 3)) * torch.rsqrt(f32c(float(hd)))
        if mask is not None:
            s = s + mask[None, None]
        e = torch.exp(s - s.amax(3, keepdim=True))
        P = e * (f32c(1.0) / e.sum(3, keepdim=True))
        pd = P * drop_mask_cpu(seed, site, p, P.numel()).reshape(P.shape)
        return (pd @ vh).permute(2, 0, 1, 3).reshape(Tq, B, d), P

    def attn_bwd(self, dout, q, k, v, P, heads, seed, site, p, packed):
        (Tq, B, d), Tk = q.shape, k.shape[0]
        hd = d // heads
        scale = torch.rsqrt(f32c(float(hd)))
        if self.mut == "attn_scale_twice":
            scale = scale * scale
        qh, kh, vh, doh = (self._heads(t, heads) for t in (q, k, v, dout))
        m = drop_mask_cpu(seed, site, p, P.numel()).reshape(P.shape)
        dPd = (doh @ vh.transpose(2, 3)) * m
        pd = P if self.mut == "attn_dv_undropped" else P * m
        dot = (dPd * P).sum(3, keepdim=True)
        dS = P * (dPd - dot) * scale
        back = lambda t, T: t.permute(2, 0, 1, 3).reshape(T, B, d)
        return back(dS @ kh, Tq), back(dS.transpose(2, 3) @ qh, Tk), back(pd.transpose(2, 3) @ doh, Tk)

    def embed_fwd(self, emb, pe, pe_row, text, B, T, d, scale, seed, site, p):
        return embed_formula(emb, pe, pe_row, text, B, T, d, scale, seed, site, p, fused=False)

    def embed_bwd(self, dy, B, T, d, d_img, scale, seed, site, p):
        return embed_bwd_formula(dy, B, T, d, d_img, scale, seed, site, p)

    def criterion(self, pred, expected, t0, fh, fw, w):
        return criterion_emu(pred, expected, t0, fh, fw, w, self.mut)


# =====================================================================================================================================
# xf_gemm_tn
# =====================================================================================================================================
TN_M = [1, 3, 31, 32, 33, 64, 65, 97, 400]
TN_NK = [(4, 4), (60, 68), (128, 128), (260, 64), (96, 32)]


def strided_pair(cls, g, M, N, K):
    """dY = the columns [N, 2N) of an (M, 3N) buffer, X = the columns [4, 4 + K) of an (M, K + 8) buffer; everything else NaN"""
    by, bx = torch.full((M, 3 * N), NAN), torch.full((M, K + 8), NAN)
    by[:, N:2 * N] = draw(cls, g, (M, N))
    bx[:, 4:4 + K] = draw(cls, g, (M, K))
    return by[:, N:2 * N], bx[:, 4:4 + K]


def ref_tn(cls, dY, X, old_dW, old_db, accumulate):
    M = dY.shape[0]
    a, b = dY.to(F64), X.to(F64)
    dW, A = a.t() @ b, a.abs().t() @ b.abs()
    db, Ab = a.sum(0), a.abs().sum(0)
    bW, bb = (M + 2) * E * A, (M + 2) * E * Ab
    if accumulate:
        dW, db = dW + old_dW.to(F64), db + old_db.to(F64)
        A, Ab = A + old_dW.to(F64).abs(), Ab + old_db.to(F64).abs()
        bW, bb = bW + E * dW.abs(), bb + E * db.abs()
    if cls == "exact":
        olds = (old_dW, old_db) if accumulate else ()
        assert sums_exact(A, min([qmin(dY) * qmin(X)] + [qmin(t) for t in olds])) and sums_exact(Ab, qmin(dY, *olds)), "the exact class's premise"
        return {"dW": (dW, 0.0), "db": (db, 0.0)}
    return {"dW": (dW, SLACK * bW), "db": (db, SLACK * bb)}


def sweep_gemm_tn(impl, tally):
    cases = [(M, 132, 124, False) for M in TN_M] + [(M, N, K, False) for (N, K) in TN_NK for M in (33, 97)] + [(33, 68, 124, True), (97, 68, 60, True)]
    for cls in ("exact", "random"):
        for i, (M, N, K, strided) in enumerate(cases):
            g = _gen(11, M, N, K, cls == "exact")
            dY, X = strided_pair(cls, g, M, N, K) if strided else (draw(cls, g, (M, N)), draw(cls, g, (M, K)))
            want_db, accumulate = i % 2 == 0, (i // 2) % 2 == 1           # db null / present x accumulate 0 / 1, in turn
            old_dW, old_db = draw(cls, g, (N, K), -64, 64), draw(cls, g, (N,), -64, 64)
            dW, db = impl.gemm_tn(dY, X, old_dW, old_db, accumulate, want_db)
            ref = ref_tn(cls, dY, X, old_dW, old_db, accumulate)
            got = {"dW": dW}
            if want_db:
                got["db"] = db
            else:
                ref.pop("db")
            tally.add(cls, "M %d N %d K %d%s%s%s" % (M, N, K, " strided" if strided else "", " acc" if accumulate else "", " db" if want_db else ""), got, ref)


# =====================================================================================================================================
# xf_gemm_nn + xf_nn_finish, relu_drop
# =====================================================================================================================================
NN_M = [1, 15, 16, 17, 95, 96, 97, 100, 200]
NN_NK = [(4, 4), (12, 4), (16, 64), (20, 60), (64, 132), (260, 64), (1024, 132), (2048, 64), (96, 2048)]
NN_CASES = [(M, 260, 68, False) for M in NN_M] + [(M, N, K, False) for (N, K) in NN_NK for M in (17, 100)] + [(17, 68, 132, True), (100, 68, 260, True)]


def test_nn_cases_cover_the_split_counts():
    """Z = 1, a Z > 1 whose tail split is empty (Z chunk >= N + chunk) and a Z that is no power of two are among the cases"""
    zs = {(N, K): nn_splits(N, K) for (_, N, K, _) in NN_CASES}
    assert 1 in zs.values()
    assert any(z > 1 and z * nn_chunk(N, z) >= N + nn_chunk(N, z) for (N, K), z in zs.items())
    assert any(z & (z - 1) for z in zs.values())


def ref_nn(cls, dY, W, r, gate_scale, add):
    N = dY.shape[1]
    a, w = dY.to(F64), W.to(F64)
    v, A = a @ w, a.abs() @ w.abs()
    bound = (N + 2) * E * A
    if r is not None:
        gs = float(f32c(gate_scale))
        open_ = r.to(F64) > 0
        v, A = torch.where(open_, v * gs, torch.zeros_like(v)), torch.where(open_, A * gs, torch.zeros_like(v))
        bound = torch.where(open_, bound * gs + E * v.abs(), torch.zeros_like(v))
    if add is not None:
        v, A = v + add.to(F64), A + add.to(F64).abs()
        bound = bound + E * v.abs()
    if cls == "exact":
        assert sums_exact(A, min(qmin(dY) * qmin(W), qmin(add))), "the exact class's premise"
        return {"out": (v, 0.0)}
    return {"out": (v, SLACK * bound)}


def sweep_gemm_nn(impl, tally):
    for cls in ("exact", "random"):
        p = 0.5 if cls == "exact" else 0.25                                   # gate scale 2 is a power of two
        for i, (M, N, K, strided) in enumerate(NN_CASES):
            g = _gen(12, M, N, K, cls == "exact")
            dY, _ = strided_pair(cls, g, M, N, 4) if strided else (draw(cls, g, (M, N)), None)
            W = draw(cls, g, (N, K))
            use_gate, use_add, alias = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 1, 1)][i % 5]
            r = None
            if use_gate:                                                      # zeros, negatives and positives, through the kernel under test
                h = randint(g, -2, 2, (M, K)) if cls == "exact" else torch.randn(M, K, generator=g) * (torch.rand(M, K, generator=g) > 0.2)
                r = impl.relu_drop(h, SEED, 5, p)
                want_r = torch.clamp_min(h, 0.0) * drop_mask_cpu(SEED, 5, p, M * K).reshape(M, K)
                tally.add("exact", "gate of M %d K %d" % (M, K), {"r": r}, {"r": (want_r.to(F64), 0.0)})
                r = want_r
            add = draw(cls, g, (M, K), -64, 64) if use_add else None
            out = impl.gemm_nn(dY, W, r, 1.0 / (1.0 - p), add, bool(alias))
            label = "M %d N %d K %d Z %d%s%s%s" % (M, N, K, nn_splits(N, K), " strided" if strided else "", " gate" if use_gate else "",
                                                   (" add==out" if alias else " add") if use_add else "")
            tally.add(cls, label, {"out": out}, ref_nn(cls, dY, W, r, 1.0 / (1.0 - p), add))


def sweep_relu_drop(impl, tally):
    for n in (1, 255, 1000, 4096 * 256 + 77):                                # the last: past one pass of the grid-stride loop
        for p in (0.0, 0.25):
            g = _gen(13, n)
            h = torch.randn(n, generator=g) * (torch.rand(n, generator=g) > 0.1)
            want = torch.clamp_min(h, 0.0) * drop_mask_cpu(SEED, 9, p, n)
            tally.add("exact", "n %d p %g" % (n, p), {"r": impl.relu_drop(h, SEED, 9, p)}, {"r": (want.to(F64), 0.0)})


# =====================================================================================================================================
# add_ln_train / ln_bwd / ln_bwd_params
# =====================================================================================================================================
LN_D = [1, 4, 255, 256, 257, 400, 2048, 2432, 3072]
LN_M = [1, 2, 3, 5, 400]
# (M, d, r present, p, accumulate, dz_drop wanted)
LN_CASES = ([(5, d, True, 0.25, i % 2 == 1, True) for i, d in enumerate(LN_D)] + [(M, 400, True, 0.25, i % 2 == 0, True) for i, M in enumerate(LN_M)]
            + [(3, 400, False, 0.0, False, False), (5, 257, True, 0.0, True, False), (3, 256, False, 0.0, True, True)])


def ln_rows(g, M, d):
    """unit-scale rows, every third row (from the second) with mean 50 and spread 1, every third (from the third) constant"""
    x = torch.randn(M, d, generator=g)
    x[1::3] += 50.0
    consts = torch.tensor([7.25, -0.0123, 64.0, 0.3])
    for n, m in enumerate(range(2, M, 3)):
        x[m] = consts[n % 4]
    return x


def ref_ln_fwd(x, r, mask, g, b):
    """fp64 y, xhat, rstd and their bounds (module docstring); also returns (dxhat, rel_rstd) for the chained backward"""
    M, d = x.shape
    D = cdiv(d, 256) + 9
    x64 = x.to(F64)
    if r is None:
        z, dz = x64, torch.zeros_like(x64)
    else:
        rm = r.to(F64) * mask.to(F64)
        z = x64 + rm
        dz = E * rm.abs() + E * z.abs()
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
    dy = g64.abs() * dxh + E * (xhat * g64).abs() + E * y.abs()
    ref = {"y": (y, SLACK * dy), "xhat": (xhat, SLACK * dxh), "rstd": (rstd[:, 0], SLACK * (rstd * rel)[:, 0])}
    return ref, SLACK * dxh, SLACK * rel


def ref_ln_bwd(cls, dy, xhat, rstd, g, mask, old_dg, old_db, accumulate, want_drop, dxh=None, rel=None):
    """xhat / rstd: what the reference takes as exact (fp64); dxh / rel: how far the kernel's own inputs may be from them (chained)"""
    M, d = dy.shape
    D = cdiv(d, 256) + 9
    dy64, xh, rs, g64 = dy.to(F64), xhat.to(F64), rstd.to(F64).reshape(M, 1), g.to(F64)[None, :]
    dxh = torch.zeros_like(xh) if dxh is None else dxh
    rel = torch.zeros_like(rs) if rel is None else rel
    gd = dy64 * g64
    m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    dm1 = (D + 1) * E * gd.abs().mean(1, keepdim=True)
    dm2 = (D + 2) * E * (gd * xh).abs().mean(1, keepdim=True) + (gd.abs() * dxh).mean(1, keepdim=True)
    dz = rs * (gd - m1 - xh * m2)
    bdz = (rs * (E * gd.abs() + dm1 + xh.abs() * dm2 + m2.abs() * dxh + E * (xh * m2).abs() + 2 * E * (gd.abs() + m1.abs() + (xh * m2).abs()))
           + dz.abs() * (rel + E))
    ref = {"dz": (dz, SLACK * bdz)}
    if want_drop:
        m = mask.to(F64)
        ref["dz_drop"] = (dz * m, SLACK * (bdz * m + E * (dz * m).abs()))
    dg, db = (dy64 * xh).sum(0), dy64.sum(0)
    Ag, Ab = (dy64 * xh).abs().sum(0), dy64.abs().sum(0)
    bg, bb = (M + 2) * E * Ag + (dy64.abs() * dxh).sum(0), (M + 2) * E * Ab
    if accumulate:
        dg, db = dg + old_dg.to(F64), db + old_db.to(F64)
        Ag, Ab = Ag + old_dg.to(F64).abs(), Ab + old_db.to(F64).abs()
        bg, bb = bg + E * dg.abs(), bb + E * db.abs()
    if cls == "exact":
        olds = (old_dg, old_db) if accumulate else ()
        assert sums_exact(Ag, min([qmin(dy) * qmin(xhat)] + [qmin(t) for t in olds])) and sums_exact(Ab, qmin(dy, *olds)), "the exact class's premise"
        ref.update(dgamma=(dg, 0.0), dbeta=(db, 0.0))
    else:
        ref.update(dgamma=(dg, SLACK * bg), dbeta=(db, SLACK * bb))
    return ref


def sweep_ln(impl, tally_f, tally_b, tally_p):
    for i, (M, d, has_r, p, accumulate, want_drop) in enumerate(LN_CASES):
        g = _gen(14, M, d, i)
        label = "M %d d %d%s p %g%s" % (M, d, " r" if has_r else "", p, " acc" if accumulate else "")
        x = ln_rows(g, M, d)
        r = torch.randn(M, d, generator=g) if has_r else None
        if has_r:
            r[2::3] = 0.0                                                     # the constant rows stay constant
        gam, bet = 1 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
        mask = impl.drop_mask(SEED, 3, p, M * d).reshape(M, d)
        assert torch.equal(mask, drop_mask_cpu(SEED, 3, p, M * d).reshape(M, d)), "svg_op_dropout_mask against its restatement"
        y, xhat, rstd = impl.add_ln(x, r, SEED, 3, p, gam, bet)
        ref, dxh, rel = ref_ln_fwd(x, r, mask, gam, bet)
        tally_f.add("random", label, {"y": y, "xhat": xhat, "rstd": rstd}, ref)
        dy = torch.randn(M, d, generator=g)
        old_dg, old_db = torch.randn(d, generator=g), torch.randn(d, generator=g)
        # (a) on xhat / rstd from fp64, rounded to f32: independent of the forward kernel
        xh32, rs32 = ref["xhat"][0].to(F32), ref["rstd"][0].to(F32)
        names = ("dz", "dz_drop", "dgamma", "dbeta")
        out = impl.ln_bwd(dy, xh32, rs32, gam, SEED, 3, p, old_dg, old_db, accumulate, want_drop)
        refb = ref_ln_bwd("random", dy, xh32, rs32, gam, mask, old_dg, old_db, accumulate, want_drop)
        split(tally_b, tally_p, "random", label + " fp64 xhat", dict(zip(names, out)), refb)
        # (b) chained on the forward kernel's own outputs, against the fp64 chain
        out = impl.ln_bwd(dy, xhat, rstd, gam, SEED, 3, p, old_dg, old_db, accumulate, want_drop)
        refb = ref_ln_bwd("random", dy, ref["xhat"][0], ref["rstd"][0], gam, mask, old_dg, old_db, accumulate, want_drop, dxh, rel.reshape(M, 1))
        split(tally_b, tally_p, "random", label + " chained", dict(zip(names, out)), refb)
        # (c) the exact class of the parameter sums: integer dy, xhat in eighths, integer old values
        dyi, xhi = randint(g, -4, 4, (M, d)), randint(g, -16, 16, (M, d)) / 8
        ogi, obi = randint(g, -64, 64, (d,)), randint(g, -64, 64, (d,))
        out = impl.ln_bwd(dyi, xhi, torch.ones(M), gam, SEED, 3, p, ogi, obi, accumulate, False)
        refb = ref_ln_bwd("exact", dyi, xhi, torch.ones(M), gam, mask, ogi, obi, accumulate, False)
        tally_p.add("exact", label, {"dgamma": out[2], "dbeta": out[3]}, {k: refb[k] for k in ("dgamma", "dbeta")})


def split(tally_b, tally_p, cls, label, got, ref):
    got = {k: v for k, v in got.items() if v is not None}
    tally_b.add(cls, label, {k: got[k] for k in got if k.startswith("dz")}, {k: ref[k] for k in ref if k.startswith("dz")})
    tally_p.add(cls, label, {k: got[k] for k in ("dgamma", "dbeta")}, {k: ref[k] for k in ("dgamma", "dbeta")})


# =====================================================================================================================================
# attn_train_fwd / attn_train_bwd
# =====================================================================================================================================
ATTN_CASES = [(1, 1, 1, 1, 8), (3, 4, 11, 11, 8), (2, 2, 5, 11, 64), (2, 2, 11, 5, 65), (2, 4, 6, 6, 100), (1, 2, 11, 11, 304), (1, 1, 32, 32, 256)]


def attn_operands(g, B, H, Tq, Tk, hd, packed):
    """q (Tq, B, d), k and v (Tk, B, d) as column slices: packed = the thirds of (T, B, 3d) buffers, else q alone and k | v of (Tk, B, 2d);
    the columns that belong to no operand are NaN"""
    d = H * hd
    if packed:
        bq, bkv = torch.full((Tq, B, 3 * d), NAN), torch.full((Tk, B, 3 * d), NAN)
        q, k, v = bq[:, :, :d], bkv[:, :, d:2 * d], bkv[:, :, 2 * d:]
    else:
        bq, bkv = torch.empty(Tq, B, d), torch.empty(Tk, B, 2 * d)
        q, k, v = bq[:, :, :], bkv[:, :, :d], bkv[:, :, d:]
    for t in (q, k, v):
        t.copy_(torch.randn(t.shape, generator=g))
    return q, k, v


def heads64(t, H):
    T, B, d = t.shape
    return t.to(F64).reshape(T, B, H, d // H).permute(1, 2, 0, 3)


def ref_attn_fwd(q, k, v, mask, H, m):
    (Tq, B, d), Tk = q.shape, k.shape[0]
    hd = d // H
    qh, kh, vh, m = heads64(q, H), heads64(k, H), heads64(v, H), m.to(F64)
    scale = hd ** -0.5
    s0 = qh @ kh.transpose(2, 3) * scale
    s = s0 if mask is None else s0 + mask.to(F64)[None, None]
    live = torch.isfinite(s)
    ds = (hd + 2) * E * (qh.abs() @ kh.abs().transpose(2, 3)) * scale + 6 * E * s0.abs()
    mx = s.amax(3, keepdim=True)
    sm = torch.where(live, s - mx, torch.zeros_like(s))
    delta = torch.where(live, ds + E * sm.abs(), torch.zeros_like(s)).amax(3, keepdim=True)
    P = torch.softmax(s, 3)
    dP = P * (2 * delta + 8 * E + (Tk + 2) * E + 2 * E)
    o = (P * m) @ vh
    do = (dP * m) @ vh.abs() + (Tk + 3) * E * ((P * m) @ vh.abs())
    back = lambda t: t.permute(2, 0, 1, 3).reshape(Tq, B, d)
    return {"o": (back(o), SLACK * back(do)), "P": (P, SLACK * dP)}


def ref_attn_bwd(dout, q, k, v, P, H, m, dPin=None):
    """P: what the reference takes as exact (fp64); dPin: how far the kernel's own P may be from it (chained)"""
    (Tq, B, d), Tk = q.shape, k.shape[0]
    hd = d // H
    qh, kh, vh, doh, m, P = heads64(q, H), heads64(k, H), heads64(v, H), heads64(dout, H), m.to(F64), P.to(F64)
    dPin = torch.zeros_like(P) if dPin is None else dPin
    scale = hd ** -0.5
    dPd = doh @ vh.transpose(2, 3) * m
    b_dPd = (hd + 2) * E * (doh.abs() @ vh.abs().transpose(2, 3)) * m + E * dPd.abs()
    pd = P * m
    b_pd = E * pd.abs() + dPin * m
    dot = (dPd * P).sum(3, keepdim=True)
    b_dot = (b_dPd * P).sum(3, keepdim=True) + (Tk + 2) * E * (dPd.abs() * P).sum(3, keepdim=True) + (dPd.abs() * dPin).sum(3, keepdim=True)
    dS = P * (dPd - dot) * scale
    b_dS = P * scale * (b_dPd + b_dot + E * (dPd - dot).abs()) + 7 * E * dS.abs() + dPin * (dPd - dot).abs() * scale
    dq = dS @ kh
    b_dq = b_dS @ kh.abs() + (Tk + 2) * E * (dS.abs() @ kh.abs())
    dk = dS.transpose(2, 3) @ qh
    b_dk = b_dS.transpose(2, 3) @ qh.abs() + (Tq + 2) * E * (dS.abs().transpose(2, 3) @ qh.abs())
    dv = pd.transpose(2, 3) @ doh
    b_dv = b_pd.transpose(2, 3) @ doh.abs() + (Tq + 2) * E * (pd.abs().transpose(2, 3) @ doh.abs())
    back = lambda t, T: t.permute(2, 0, 1, 3).reshape(T, B, d)
    return {"dq": (back(dq, Tq), SLACK * back(b_dq, Tq)), "dk": (back(dk, Tk), SLACK * back(b_dk, Tk)), "dv": (back(dv, Tk), SLACK * back(b_dv, Tk))}


def sweep_attn(impl, tally_f, tally_b):
    n = 0
    for (B, H, Tq, Tk, hd) in ATTN_CASES:
        for packed in (True, False):
            causal, p = [(False, 0.0), (True, 0.25), (False, 0.25), (True, 0.0)][n % 4]       # mask x p in turn; both layouts see both of each
            n += 1 if packed else 2
            g = _gen(15, B, H, Tq, Tk, hd, packed)
            label = "B %d H %d Tq %d Tk %d hd %d %s%s p %g" % (B, H, Tq, Tk, hd, "packed" if packed else "q | kv", " causal" if causal else "", p)
            q, k, v = attn_operands(g, B, H, Tq, Tk, hd, packed)
            mask = torch.full((Tq, Tk), float("-inf")).triu(1) if causal else None
            m = impl.drop_mask(SEED, 7, p, B * H * Tq * Tk).reshape(B, H, Tq, Tk)
            o, P = impl.attn_fwd(q, k, v, mask, H, SEED, 7, p)
            ref = ref_attn_fwd(q, k, v, mask, H, m)
            tally_f.add("random", label, {"o": o, "P": P}, ref)
            dout = torch.randn(Tq, B, H * hd, generator=g)
            P32 = ref["P"][0].to(F32)                                          # (a) P from fp64, rounded: independent of the forward kernel
            out = impl.attn_bwd(dout, q, k, v, P32, H, SEED, 7, p, packed)
            tally_b.add("random", label + " fp64 P", dict(zip(("dq", "dk", "dv"), out)), ref_attn_bwd(dout, q, k, v, P32, H, m))
            out = impl.attn_bwd(dout, q, k, v, P, H, SEED, 7, p, packed)         # (b) chained on the forward kernel's P
            tally_b.add("random", label + " chained", dict(zip(("dq", "dk", "dv"), out)), ref_attn_bwd(dout, q, k, v, ref["P"][0], H, m, ref["P"][1]))


# =====================================================================================================================================
# embed_post_train / embed_post_bwd
# =====================================================================================================================================
def embed_formula(emb, pe, pe_row, text, B, T, d, scale, seed, site, p, fused):
    d_txt = 0 if text is None else text.shape[1]
    v = emb.reshape(B, T, d - d_txt)
    if d_txt:
        v = torch.cat([v, text[:, None, :].expand(B, T, d_txt)], 2)
    v = v.permute(1, 0, 2)                                                   # (T, B, d)
    rows = torch.arange(B) if pe_row is None else pe_row.long()
    pos = pe[rows][None, :, :].expand(T, B, d)
    s = f32c(scale)
    t = (v.to(F64) * s.to(F64) + pos.to(F64)).to(F32) if fused else v * s + pos      # the product of two f32 is exact in fp64
    return t * drop_mask_cpu(seed, site, p, T * B * d).reshape(T, B, d)


def embed_bwd_formula(dy, B, T, d, d_img, scale, seed, site, p):
    m = drop_mask_cpu(seed, site, p, T * B * d).reshape(T, B, d)
    return (dy * m * f32c(scale))[:, :, :d_img].permute(1, 0, 2).reshape(B * T, d_img)


def sweep_embed(impl, tally):
    n = 0
    for B in (1, 3):
        for T in (1, 6):
            for (d, d_txt) in ((32, 0), (400, 384)):
                perm, p = [(False, 0.0), (True, 0.25), (False, 0.25), (True, 0.0)][n % 4]
                n += 1
                g = _gen(16, B, T, d)
                label = "B %d T %d d %d text %d%s p %g" % (B, T, d, d_txt, " pe_row" if perm else "", p)
                emb, pe = torch.randn(B * T, d - d_txt, generator=g), torch.randn(64, d, generator=g)
                text = torch.randn(B, d_txt, generator=g) if d_txt else None
                pe_row = torch.randperm(B, generator=g).to(torch.int32) if perm else None
                scale = math.sqrt(d)
                y = impl.embed_fwd(emb, pe, pe_row, text, B, T, d, scale, SEED, 2, p)
                a, b = (embed_formula(emb, pe, pe_row, text, B, T, d, scale, SEED, 2, p, fused) for fused in (False, True))
                want = torch.where(y == b, b, a)                             # per element one of the two roundings the language allows
                tally.add("exact", label + " fwd", {"y": y}, {"y": (want.to(F64), 0.0)})
                dy = torch.randn(T, B, d, generator=g)
                de = impl.embed_bwd(dy, B, T, d, d - d_txt, scale, SEED, 2, p)
                tally.add("exact", label + " bwd", {"de": de}, {"de": (embed_bwd_formula(dy, B, T, d, d - d_txt, scale, SEED, 2, p).to(F64), 0.0)})


# =====================================================================================================================================
# criterion
# =====================================================================================================================================
CRIT_FEAT = [(1, 1), (2, 2), (4, 8), (8, 8), (16, 16), (16, 32)]      # the last: 512 positions, two passes of the 256 threads of nce_kernel
CRIT_ROWS = [(3, 2, 0), (6, 3, 2), (4, 1, 3)]
CRIT_W = [dict(w_mse=1.0), dict(w_l1=1.0), dict(w_gdl=1.0, alpha=1), dict(w_gdl=1.0, alpha=2), dict(w_gdl=0.3, alpha=1.5, w_l1=1.0),
          dict(w_contrastive=1.0, temperature=0.07), dict(w_mse=1.0, w_gdl=1.0, alpha=2, w_contrastive=0.1, temperature=0.2)]


def crit_data(g, Tt, B, fh, fw):
    D = 4 * fh * fw
    pred, exp_tb = 0.7 * torch.randn(Tt, B, D, generator=g), 0.7 * torch.randn(Tt, B, D, generator=g)
    same = torch.rand(Tt, B, D, generator=g) < 0.1                           # a tenth with pred == expected: sign(0) of the L1 term
    pred[same] = exp_tb[same]
    if fw > 1:                                                               # a tenth with equal horizontal neighbours: gx == 0
        eq = (torch.rand(Tt, B, D, generator=g) < 0.1) & ((torch.arange(D) % fw) > 0)[None, None, :]
        idx = eq.nonzero()
        for t, b, c in idx.tolist():
            pred[t, b, c] = pred[t, b, c - 1]
    return pred, exp_tb.permute(1, 0, 2).contiguous()                        # expected (B, Tt, D)


def shifted(x, fh, fw):
    """x (..., 4, fh, fw) -> the vertical and horizontal differences"""
    return x[..., 1:, :] - x[..., :-1, :], x[..., :, 1:] - x[..., :, :-1]


def ref_criterion(pred, expected, t0, fh, fw, w):
    """the five losses and dpred in fp64 from oracle/train_oracle.criterion with autograd, and their bounds (module docstring)"""
    Tt, B, D = pred.shape
    hw, F_ = fh * fw, Tt - t0
    x = pred.to(F64)[t0:].clone().requires_grad_(True)
    y = expected.to(F64).permute(1, 0, 2)[t0:]
    total, terms = TR.criterion(x, y, F_, (fh, fw), **w)
    total.backward()
    dpred = torch.cat([torch.zeros(t0, B, D, dtype=F64), x.grad])
    losses = torch.stack([total.detach()] + [terms[k].detach().to(F64) for k in ("mse", "l1", "gdl", "contrastive")])
    if not w.get("w_gdl", 0.0):
        losses[3] = 0.0                                                       # the kernel does not evaluate a GDL term of weight 0 (nor the contrastive one)
    # ---- bounds ----
    xd = x.detach()
    w_mse, w_l1, w_gdl, alpha = w.get("w_mse", 0.0), w.get("w_l1", 0.0), w.get("w_gdl", 0.0), float(w.get("alpha", 1))
    w_nce, tau = w.get("w_contrastive", 0.0), w.get("temperature", 0.07)
    inv_n = 1.0 / (F_ * B * D)
    df = xd - y
    comp = (w_mse * 2 * df * inv_n).abs() + (w_l1 * torch.sign(df) * inv_n).abs()
    extra = torch.zeros_like(df)
    rows = Tt * B
    depth = (cdiv(D, 256) + rows + 16) * E
    if w_gdl:
        X5, Y5 = xd.reshape(F_, B, 4, fh, fw), y.reshape(F_, B, 4, fh, fw)
        comp5, extra5 = torch.zeros_like(X5), torch.zeros_like(X5)
        for (gx, gy), ax in zip(zip(shifted(X5, fh, fw), shifted(Y5, fh, fw)), (3, 4)):
            u = gx.abs() - gy.abs()
            au = u.abs()
            dau = E * (gx.abs() + gy.abs() + au)
            if alpha == 1.0:
                mag, dmag = torch.ones_like(au), torch.zeros_like(au)
            elif alpha == 2.0:
                mag, dmag = 2 * au, 2 * dau + E * 2 * au
            else:
                mag = alpha * au ** (alpha - 1)
                dmag = torch.where(au > 0, mag * (9 * E + abs(alpha - 1) * dau / au.clamp_min(1e-300)), alpha * dau ** (alpha - 1))
            live = (gx != 0).to(F64)                                          # sign(gx) = 0 kills the term on both sides
            c = w_gdl * inv_n * mag * live
            e = w_gdl * inv_n * live * (dmag + torch.where(au <= dau, 2 * mag + 2 * dmag, torch.zeros_like(au)))
            lo = [slice(None)] * 5
            hi = [slice(None)] * 5
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            for sl in (lo, hi):
                comp5[tuple(sl)] += c
                extra5[tuple(sl)] += e
        comp, extra = comp + comp5.reshape(F_, B, D), extra + extra5.reshape(F_, B, D)
    b_nce_loss = 0.0
    if w_nce:
        G = y.reshape(F_ * B, 4, hw).transpose(1, 2)                          # (R, hw, 4)
        Pm = xd.reshape(F_ * B, 4, hw).transpose(1, 2)
        R = F_ * B * hw
        sc = w_nce * 0.5 / tau / R

        def direction(A_, B_):
            """rows of softmax(A B^T / tau) with their logit error delta"""
            L = A_ @ B_.transpose(1, 2) / tau
            mx = L.amax(2, keepdim=True)
            dl = 7 * E * (A_.abs() @ B_.abs().transpose(1, 2)) / tau + E * (L - mx).abs()
            lse = torch.logsumexp(L, 2, keepdim=True)
            return L, torch.softmax(L, 2), dl.amax(2, keepdim=True), lse, mx

        L1, S1, d1, lse1, mx1 = direction(G, Pm)
        L2, S2, d2, lse2, mx2 = direction(Pm, G)
        lii = torch.diagonal(L1, dim1=1, dim2=2)[..., None]
        sii = torch.diagonal(S1, dim1=1, dim2=2)[..., None]
        logse1, logse2 = (lse1 - mx1).abs(), (lse2 - mx2).abs()
        rho1 = 2 * d1 + (hw + 12) * E + 8 * E * logse1 + E * lse1.abs() + E * (lii - lse1).abs() + 8 * E
        rho2 = 2 * d2 + (hw + 12) * E
        t1, t2 = (sii - 1) * G, S2 @ G
        b_d = G.abs() * (sii * rho1 + 2 * E) + (rho2 + (hw + 5) * E) * (S2 @ G.abs()) + 3 * E * (t1.abs() + t2.abs() + G.abs())
        d_c = t1 + t2 - G
        nce_c = (sc * d_c.abs()).transpose(1, 2).reshape(F_, B, D)
        comp = comp + nce_c
        extra = extra + (sc * b_d).transpose(1, 2).reshape(F_, B, D) * SLACK
        per_pos = (d1 + (hw + 12) * E + 8 * E * logse1 + E * lse1.abs()) + (d2 + (hw + 12) * E + 8 * E * logse2 + E * lse2.abs()) + 2 * (d1 + E * lii.abs())
        terms_abs = (lse1.abs() + lii.abs()) + (lse2.abs() + lii.abs())
        b_nce_loss = 0.5 / R * float((per_pos + (cdiv(hw, 256) + rows + 16) * E * terms_abs).sum()) + 3 * E * float(losses[4].abs())
    b_dp = torch.cat([torch.zeros(t0, B, D, dtype=F64), SLACK * (12 * E * comp + extra)])
    b_loss = torch.zeros(5, dtype=F64)
    b_loss[1] = (depth + 5 * E) * losses[1].abs()
    b_loss[2] = (depth + 4 * E) * losses[2].abs()
    if w_gdl:
        b_loss[3] = (depth + 4 * E) * losses[3].abs() + inv_n * gdl_terms_abs_error(xd, y, fh, fw, alpha)
    b_loss[4] = b_nce_loss
    b_loss[0] = abs(w_mse) * b_loss[1] + abs(w_l1) * b_loss[2] + abs(w_gdl) * b_loss[3] + abs(w_nce) * b_loss[4] + 8 * E * (
        abs(w_mse) * losses[1].abs() + abs(w_l1) * losses[2].abs() + abs(w_gdl) * losses[3].abs() + abs(w_nce) * losses[4].abs())
    return {"losses": (losses, SLACK * b_loss), "dpred": (dpred, b_dp)}


def gdl_terms_abs_error(xd, y, fh, fw, alpha):
    """sum over the GDL terms of the error of |u|^alpha: alpha |u|^(alpha - 1) d(au) + (powf: 9 e, square: 2 e) |u|^alpha"""
    F_, B, D = xd.shape
    X5, Y5 = xd.reshape(F_, B, 4, fh, fw), y.reshape(F_, B, 4, fh, fw)
    tot = 0.0
    for gx, gy in zip(shifted(X5, fh, fw), shifted(Y5, fh, fw)):
        au = (gx.abs() - gy.abs()).abs()
        dau = E * (gx.abs() + gy.abs() + au)
        if alpha == 1.0:
            tot += float(dau.sum())
        else:
            tot += float((alpha * au ** (alpha - 1) * dau + 9 * E * au ** alpha).sum())
    return tot


def criterion_emu(pred, expected, t0, fh, fw, w, mut=None):
    """loss_rows_kernel / nce_kernel / loss_finish_kernel in torch f32"""
    Tt, B, D = pred.shape
    hw, F_ = fh * fw, Tt - t0
    w_mse, w_l1, w_gdl = (f32c(w.get(k, 0.0)) for k in ("w_mse", "w_l1", "w_gdl"))
    alpha = f32c(float(w.get("alpha", 1)))
    w_nce, tau = f32c(w.get("w_contrastive", 0.0)), f32c(w.get("temperature", 0.07))
    n_rows = Tt if mut == "crit_inv_n_all_rows" else F_
    inv_n = f32c(1.0) / (f32c(float(n_rows)) * f32c(float(B)) * f32c(float(D)))
    x, y = pred[t0:], expected.permute(1, 0, 2)[t0:]
    df = x - y
    sgn = torch.sign(df)
    if mut == "crit_sign0_is_1":
        sgn = torch.where(df == 0, torch.ones_like(df), sgn)
    gacc = w_mse * 2.0 * df * inv_n + w_l1 * sgn * inv_n
    s_gdl = torch.zeros(F_, B)
    if float(w_gdl) != 0.0:
        X5, Y5 = x.reshape(F_, B, 4, fh, fw), y.reshape(F_, B, 4, fh, fw)
        acc = torch.zeros_like(X5)
        for (gx, gy), ax in zip(zip(shifted(X5, fh, fw), shifted(Y5, fh, fw)), (3, 4)):
            u = gx.abs() - gy.abs()
            au = u.abs()
            if float(alpha) == 1.0:
                val, mag = au, torch.ones_like(au)
            elif float(alpha) == 2.0:
                val, mag = u * u, 2.0 * au
            else:
                val, mag = torch.pow(au, alpha), alpha * torch.pow(au, alpha - 1.0)
            t = mag * torch.sign(u) * torch.sign(gx)
            lo, hi = [slice(None)] * 5, [slice(None)] * 5
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            acc[tuple(hi)] += t                                                # this element is the + end
            acc[tuple(lo)] -= t                                                # the - end, where the term is counted
            s_gdl = s_gdl + val.sum((2, 3, 4)) * (2.0 if mut == "crit_gdl_both_ends" else 1.0)
        gacc = gacc + w_gdl * acc.reshape(F_, B, D) * inv_n
    s_nce = torch.zeros(F_, B)
    if float(w_nce) != 0.0:
        inv_tau = f32c(1.0) / tau
        G, Pm = y.reshape(F_ * B, 4, hw).transpose(1, 2), x.reshape(F_ * B, 4, hw).transpose(1, 2)
        R = f32c(float(F_)) * f32c(float(B)) * f32c(float(hw))
        L1, L2 = (G @ Pm.transpose(1, 2)) * inv_tau, (Pm @ G.transpose(1, 2)) * inv_tau
        mx1, mx2 = L1.amax(2, keepdim=True), L2.amax(2, keepdim=True)
        se1 = torch.exp(L1 - mx1).sum(2, keepdim=True)
        e2 = torch.exp(L2 - mx2)
        se2 = e2.sum(2, keepdim=True)
        lii = torch.diagonal(L1, dim1=1, dim2=2)[..., None]
        lse1, lse2 = mx1 + torch.log(se1), mx2 + torch.log(se2)
        sm_ii = torch.exp(lii - lse1)
        dvec = (sm_ii - 1.0) * G + (e2 @ G) * (f32c(1.0) / se2)
        if mut != "crit_nce_no_minus_g":
            dvec = dvec - G
        sc = w_nce * 0.5 * inv_tau / R
        gacc = gacc + (sc * dvec).transpose(1, 2).reshape(F_, B, D)
        s_nce = ((lse1 - lii) + (lse2 - lii)).sum((1, 2)).reshape(F_, B)
    n_el = f32c(float(F_)) * B * D
    mse, l1, gdl = (df * df).sum() / n_el, df.abs().sum() / n_el, s_gdl.sum() / n_el
    nce = 0.5 * s_nce.sum() / (f32c(float(F_)) * B * hw) if float(w_nce) != 0.0 else f32c(0.0)
    total = w_mse * mse + w_l1 * l1 + w_gdl * gdl + w_nce * nce
    return torch.stack([total, mse, l1, gdl, nce]), torch.cat([torch.zeros(t0, B, D), gacc])


def sweep_criterion(impl, tally):
    n = 0
    for (fh, fw) in CRIT_FEAT:
        for w in CRIT_W:
            Tt, B, t0 = CRIT_ROWS[n % 3]
            n += 1
            g = _gen(17, fh, fw, n)
            pred, expected = crit_data(g, Tt, B, fh, fw)
            losses, dpred = impl.criterion(pred, expected, t0, fh, fw, w)
            assert bool((dpred[:t0] == 0).all()), "rows t < t0 of dpred must come back zero"
            tally.add("random", "feat %dx%d Tt %d B %d t0 %d %s" % (fh, fw, Tt, B, t0, sorted(w.items())), {"losses": losses, "dpred": dpred},
                      ref_criterion(pred, expected, t0, fh, fw, w))


# =====================================================================================================================================
# the sweeps, by kernel: name -> (function, tallies)
# =====================================================================================================================================
def run_all(impl, which, report):
    """runs the sweeps named in `which` and returns {tally name: Tally}"""
    T = {}
    mk = lambda name: T.setdefault(name, Tally(name))
    if "gemm_tn" in which:
        sweep_gemm_tn(impl, mk("xf_gemm_tn"))
    if "gemm_nn" in which:
        sweep_gemm_nn(impl, mk("xf_gemm_nn + xf_nn_finish"))
    if "relu_drop" in which:
        sweep_relu_drop(impl, mk("relu_drop"))
    if "ln" in which:
        sweep_ln(impl, mk("add_ln_train"), mk("ln_bwd"), mk("ln_bwd_params"))
    if "attn" in which:
        sweep_attn(impl, mk("attn_train_fwd"), mk("attn_train_bwd"))
    if "embed" in which:
        sweep_embed(impl, mk("embed_post_train / bwd"))
    if "criterion" in which:
        sweep_criterion(impl, mk("criterion"))
    return T


KERNELS = ["gemm_tn", "gemm_nn", "relu_drop", "ln", "attn", "embed", "criterion"]


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------
def test_dropout_restatement_cpu():
    """the restated generator: p = 0 keeps everything, p = 0.25 keeps about three quarters at 4/3, and sites / seeds differ"""
    m = drop_mask_cpu(SEED, 3, 0.25, 1 << 16)
    assert set(m.unique().tolist()) == {0.0, float(f32c(1.0) / (f32c(1.0) - f32c(0.25)))}
    assert abs(float((m > 0).float().mean()) - 0.75) < 0.01
    assert not torch.equal(m, drop_mask_cpu(SEED, 4, 0.25, 1 << 16)) and not torch.equal(m, drop_mask_cpu(SEED + 1, 3, 0.25, 1 << 16))
    assert bool((drop_mask_cpu(SEED, 3, 0.0, 100) == 1).all())


@pytest.mark.parametrize("kernel", KERNELS)
def test_emulation_cpu(kernel):
    """the f32 emulation of each kernel passes its judge on every case and both data classes (and the exact-class premises hold)"""
    for t in run_all(Emu(), [kernel], False).values():
        t.check(report=False)


MUTATIONS = {"tn_drop_last_batch": "gemm_tn", "tn_edge_col": "gemm_tn", "tn_db_lane_group": "gemm_tn", "tn_acc_ignores_old": "gemm_tn",
             "nn_edge_col": "gemm_nn", "nn_stale_slab": "gemm_nn", "nn_gate_ge": "gemm_nn",
             "ln_one_pass_var": "ln", "ln_bwd_no_m2": "ln", "attn_dv_undropped": "attn", "attn_scale_twice": "attn",
             "crit_gdl_both_ends": "criterion", "crit_sign0_is_1": "criterion", "crit_nce_no_minus_g": "criterion", "crit_inv_n_all_rows": "criterion"}
# the tally (and the classes) that must reject each defect
MUT_TALLY = {"tn": "xf_gemm_tn", "nn": "xf_gemm_nn + xf_nn_finish", "ln_one_pass_var": "add_ln_train", "ln_bwd_no_m2": "ln_bwd", "attn": "attn_train_bwd",
             "crit": "criterion"}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judge_rejects_cpu(mut):
    """each defect of the emulation is outside the judge, in every data class the kernel has (the sound emulation is inside: test_emulation_cpu)"""
    T = run_all(Emu(mut), [MUTATIONS[mut]], False)
    name = MUT_TALLY.get(mut) or MUT_TALLY[mut.split("_")[0]]
    rej = T[name].rejected()
    print("[train_kernels] mutation %-22s %s" % (mut, {c: "%.3g" % T[name].worst[c][0] for c in rej}))
    assert rej and all(rej.values()), "the judge of %s accepts the defect %s in the class(es) %s" % (name, mut, [c for c, r in rej.items() if not r])


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_against_fp64(ctx, kernel):
    impl = Gpu(ctx)
    if kernel == "relu_drop":
        assert torch.equal(impl.drop_mask(SEED, 9, 0.25, 100003), drop_mask_cpu(SEED, 9, 0.25, 100003)), "svg_op_dropout_mask against its restatement"
    T = run_all(impl, [kernel], True)
    if kernel == "gemm_nn":
        for (N, K), z in impl.splits_seen.items():
            assert z == nn_splits(N, K), "N %d K %d: the hook reports %d splits, the restatement %d" % (N, K, z, nn_splits(N, K))
        zs = impl.splits_seen
        assert 1 in zs.values() and any(z & (z - 1) for z in zs.values())
        assert any(z > 1 and z * nn_chunk(N, z) >= N + nn_chunk(N, z) for (N, K), z in zs.items())
    for t in T.values():
        t.check(report=True)


def _valid_after(impl, which):
    """the next valid call on the same context is correct"""
    for t in run_all(impl, [which], False).values():
        t.check(report=False)


@gpu
def test_refusals(ctx):
    """every SVG_CHECK of a launcher: the call returns non-zero, the outputs stay NaN, and the next valid call on the context is right.
    Every buffer is sized for the shape requested: nothing depends on the guard for memory safety."""
    impl = Gpu(ctx)
    nan = lambda *s: torch.full(s, NAN, device="cuda", dtype=F32)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=F32)
    P = lambda t: t.data_ptr()
    untouched = lambda *ts: all(bool(torch.isnan(t).all()) for t in ts)
    # LayerNorm, d = 3073
    M, d = 3, 3073
    x, g, b, y, xh, rs = rnd(M, d), rnd(d), rnd(d), nan(M, d), nan(M, d), nan(M)
    assert impl.refused("svg_op_xf_add_ln_train", P(x), None, SEED, 0, 0.0, P(g), P(b), P(y), P(xh), P(rs), M, d, LN_EPS) and untouched(y, xh, rs)
    dz, dg, db = nan(M, d), nan(d), nan(d)
    assert impl.refused("svg_op_xf_ln_bwd", P(x), P(x), P(rnd(M)), P(g), P(dz), None, SEED, 0, 0.0, P(dg), P(db), M, d, 0) and untouched(dz, dg, db)
    # attention, T = 33; hd = 301 at T = 32 (the backward's four staged operands: 154 112 bytes of LDS against 153 600)
    for (T, hd, fwd_refuses) in ((33, 8, True), (32, 301, False)):
        q, k, v, do = rnd(T, 1, hd), rnd(T, 1, hd), rnd(T, 1, hd), rnd(T, 1, hd)
        o, Pm, dq, dk, dv = nan(T, 1, hd), nan(1, 1, T, T), nan(T, 1, hd), nan(T, 1, hd), nan(T, 1, hd)
        if fwd_refuses:
            assert impl.refused("svg_op_xf_attention_train", P(q), hd, P(k), P(v), hd, None, P(o), P(Pm), T, T, 1, 1, hd, SEED, 0, 0.0) and untouched(o, Pm)
        Pin = torch.softmax(rnd(1, 1, T, T), 3)
        assert impl.refused("svg_op_xf_attention_bwd", P(do), P(q), hd, P(k), P(v), hd, P(Pin), P(dq), hd, P(dk), P(dv), hd, T, T, 1, 1, hd, SEED, 0, 0.0)
        assert untouched(dq, dk, dv)
    # the backward GEMMs, N = 6
    M, N, K = 5, 6, 8
    dY, X, W, dW, dbias, out = rnd(M, N), rnd(M, K), rnd(N, K), nan(N, K), nan(N), nan(M, K)
    assert impl.refused("svg_op_xf_gemm_tn", P(dY), N, P(X), K, P(dW), P(dbias), M, N, K, 0) and untouched(dW, dbias)
    z = ctypes.c_int(-1)
    assert impl.refused("svg_op_xf_gemm_nn", P(dY), N, P(W), P(out), M, N, K, None, 1.0, None, ctypes.byref(z)) and untouched(out)
    # criterion: D != 4 fh fw; 4097 positions with the contrastive term
    for (D, fh, fw, w_nce) in ((36, 2, 4, 0.0), (4 * 4097, 17, 241, 1.0)):
        pred, expc, dp = rnd(2, 1, D), rnd(1, 2, D), nan(2, 1, D)
        losses = (ctypes.c_float * 5)(*([NAN] * 5))
        assert impl.refused("svg_op_xf_criterion", P(pred), P(expc), P(dp), losses, 2, 1, D, 0, fh, fw, 1.0, 0.0, 0.0, 1.0, w_nce, 0.07) and untouched(dp)
        assert all(math.isnan(v) for v in losses)
    for which in ("gemm_tn", "gemm_nn", "embed"):
        _valid_after(impl, which)
    # a valid LayerNorm, attention and criterion call each, judged as in the sweeps
    g0 = _gen(18)
    x, gam, bet = ln_rows(g0, 3, 257), torch.ones(257), torch.zeros(257)
    y, xhat, rstd = impl.add_ln(x, None, SEED, 0, 0.0, gam, bet)
    t = Tally("add_ln_train after a refusal")
    t.add("random", "M 3 d 257", {"y": y, "xhat": xhat, "rstd": rstd}, ref_ln_fwd(x, None, None, gam, bet)[0])
    q, k, v = attn_operands(g0, 1, 1, 32, 32, 300, False)                     # hd = 300 at T = 32: exactly the LDS budget of the backward
    o, Pm = impl.attn_fwd(q, k, v, None, 1, SEED, 0, 0.0)
    ref = ref_attn_fwd(q, k, v, None, 1, torch.ones(1, 1, 32, 32))
    t.add("random", "attention T 32 hd 300", {"o": o, "P": Pm}, ref)
    dout = torch.randn(32, 1, 300, generator=g0)
    out = impl.attn_bwd(dout, q, k, v, ref["P"][0].to(F32), 1, SEED, 0, 0.0, False)
    t.add("random", "attention backward T 32 hd 300", dict(zip(("dq", "dk", "dv"), out)),
          ref_attn_bwd(dout, q, k, v, ref["P"][0].to(F32), 1, torch.ones(1, 1, 32, 32)))
    pred, expected = crit_data(g0, 3, 2, 4, 4)
    w = dict(w_mse=1.0, w_contrastive=0.5, temperature=0.2)
    losses, dpred = impl.criterion(pred, expected, 1, 4, 4, w)
    t.add("random", "criterion 4x4", {"losses": losses, "dpred": dpred}, ref_criterion(pred, expected, 1, 4, 4, w))
    t.check(report=False)
