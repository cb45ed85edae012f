"""Fused attention (csrc/attn.hip, attn_vae.hip, xattn_fused.hip) on every kernel instantiation, against an fp64 reference.

svg_op_attention_ex runs one AttnArgs descriptor on a forced instantiation and reports what ran ({kernel, d, QB, NST, BC, HV});
every case asserts that path first.  PATHS lists every instantiation attention_describe can name: attn_kernel<d, QB, NST, BC, HV>
for d = 8, 16, 32, 40, 64, 80, 160 (QB 2 for d <= 64; NST 2 except d = 160, whose two stages do not fit; BC for d = 8, 40; HV with
BC and QB 2) and attn_dma40_kernel.  The kernels are correct for any Sq, so a forced QB = 2 or dma40 path runs at small shapes too.

Reference: fp64 on the device, from the kernel's own inputs (already rounded to the storage type): p = softmax(q k^T scale),
ref = p v.  Judging:
  * exact selection: key j of each (sample, head) carries a distinct +-1 code in m >= log2(Skv) dimensions (spread over the head
    dimension), times 32; query i carries the scaled code of one chosen key.  The chosen score then beats every other one by
    >= 2 * 32^2 * scale * log2(e) >= 160 in exp2 units (asserted), so every other P underflows to exactly 0 in f32 — also every
    earlier tile's running sum, which is rescaled by exp2(<= -160) = 0.  The output must EQUAL v[chosen] bit for bit: the PV product
    is P_r v with P_r the rounded P of the chosen key (exact in f32) and the normaliser is P_r itself (ones-row paths) or P within
    a few f32 ulps of 1 (l_run paths, d % 32 = 0), which rounds back to v.  No tolerance: this checks K rows, dma40's permuted K
    slots, V^T columns, head and sample offsets, tail masking and the online rescale.
  * random data, per element, a bound from the arithmetic (the same for every path):
        |out - ref| <= u |ref| + 1.01 (u + ln2 u_Q A_i + g_i) (sum_j p_ij |v_j| + |ref_i|) + t sum_j |v_j|
    A perturbation e_j of the weight of key j moves out_i by sum_j p_ij e_j (v_j - out_i) to first order when the normaliser is
    built from the same weights (ones-row paths), or by sum_j p_ij e_j v_j when it is not (l_run paths, for the rounding of P only);
    both are bounded by max|e_j| (sum_j p_ij |v_j| + |ref_i|).  The weight errors:
      u      rounding P to the storage type before PV (u = 2^-8 bf16, 2^-11 fp16), and the output rounding (the u |ref| term);
      u_Q    BC and dma40 store q * scale * log2(e) in 16 bits: the exp2 argument of key j moves by <= u_Q A_i,
             A_i = max_j sum_k |q_ik c k_jk| (c = scale log2 e); u_Q = u there, 0 elsewhere;
      g_i    = 2^-24 (ln2 (2 (d + 3) + 4 (R + 1)) A_i + 2 (R + 1) + 2 Skv + 4): the f32 QK^T accumulation (d products, plus the
             three shift pieces on BC paths: <= (d + 3) 2^-24 (A_i + |shift|) <= 2 (d + 3) 2^-24 A_i), the rounding of c, of the
             exp2 argument and of the shift at each of the R = ceil(Skv / 64) possible rescales (4 A_i each), v_exp_f32 (1 ulp, on
             P and on each rescale factor), the f32 PV and row-sum accumulations over Skv keys, 1 / l and the final product;
      t      underflow of a small P in the storage type: 2^-25 absolute in fp16 (subnormal spacing 2^-24), 2^-126 in bf16, against a
             normaliser >= 1 (the key that set the running max or shift has P = 1).
    The per-path aggregate rel-L2 < 2 tol of test_ops_gpu::test_attention is asserted as well.
  * out starts as NaN: every element outside the [B][Sq][heads * d] rows (the ldo gaps, the batch gaps, a row past Sq) must still
    be NaN; every valid one must be finite.  Inputs are laid out in NaN-filled buffers, so a stray read of a gap poisons the result.
    The V^T pad keys Skv .. ceil8(Skv) - 1 hold a large finite value (svg_hip.h: they must be finite): the result must be bit
    identical to a zero pad.
Every test runs on the bf16 build (svg_op_*) and on the fp16 build (svg_op_*_f16)."""
import ctypes as C
import math
import zlib

import pytest
import torch

from conftest import rel_l2
from sd_video_gen_amd import _lib

pytestmark = pytest.mark.gpu

REG, DMA40 = 0, 1                    # path[0]: AttnKernel (csrc/kernels.h)
LOG2E = 1.4426950408889634
PAD_BIG = 30000.0                    # a large V^T pad value both storage types hold exactly enough (fp16 max 65504)


class _Half:
    """storage type the current test runs in"""
    dtype = torch.bfloat16
    suffix = ""
    u = 2.0 ** -8
    tiny = 2.0 ** -126
    tol = 4e-3


HALF = _Half()


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def _storage(request):
    if request.param == "bf16":
        HALF.dtype, HALF.suffix, HALF.u, HALF.tiny, HALF.tol = torch.bfloat16, "", 2.0 ** -8, 2.0 ** -126, 4e-3
    else:
        HALF.dtype, HALF.suffix, HALF.u, HALF.tiny, HALF.tol = torch.float16, "_f16", 2.0 ** -11, 2.0 ** -25, 5e-4
    yield request.param
    HALF.dtype, HALF.suffix, HALF.u, HALF.tiny, HALF.tol = torch.bfloat16, "", 2.0 ** -8, 2.0 ** -126, 4e-3


def stream():
    return torch.cuda.current_stream().cuda_stream


def _variants():
    out = []
    for d in (8, 16, 32, 40, 64, 80, 160):
        if d == 40:
            out.append((DMA40, 40, 2, 3, 1, 1))
        for qb in ((1, 2) if d <= 64 else (1,)):
            if d % 16 == 8:
                out.append((REG, d, qb, 1, 1, 0))
                if qb == 2:
                    out.append((REG, d, qb, 1, 1, 1))
            out.append((REG, d, qb, 1, 0, 0))
            if d != 160:
                out.append((REG, d, qb, 2, 0, 0))
    return out


PATHS = _variants()


def path_id(p):
    return "dma40" if p[0] == DMA40 else "d%d-qb%d-nst%d%s%s" % (p[1], p[2], p[3], "-bc" if p[4] else "", "-hv" if p[5] else "")


def attn_ex(ctx, force=None, **f):
    """svg_op_attention_ex(_f16) on a descriptor of the given fields (tensors by pointer, ints as pointers); returns (status, path)"""
    d = _lib.AttnDesc()
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    if force is not None:
        d.force = 1
        d.kernel, _, d.qblocks, d.nst, d.bc, d.hv = force
    path = (C.c_int * 6)(*([-1] * 6))
    rc = getattr(ctx.lib, "svg_op_attention_ex" + HALF.suffix)(ctx.h, C.byref(d), path, stream())
    return rc, tuple(path)


def ceil8(n):
    return (n + 7) // 8 * 8


# ---- problems: logical q (B, Sq, heads, d), k / v (B, Skv, heads, d) in the storage type, laid out in NaN-filled buffers ----------
class Problem:
    def __init__(self, q, k, v, scale, layout="dense", pad=0.0):
        B, Sq, H, d = q.shape
        Skv = k.shape[1]
        Cc = H * d
        dt = q.dtype
        self.q, self.k, self.v, self.scale = q, k, v, scale
        self.B, self.Sq, self.Skv, self.H, self.d, self.C = B, Sq, Skv, H, d, Cc
        nan = float("nan")
        dev = q.device
        shared = layout == "shared"          # kb = vtb = 0: one context for every sample
        if shared:
            assert bool((k == k[:1]).all()) and bool((v == v[:1]).all())
        gaps = layout in ("gaps", "shared")
        Kp = ceil8(Skv)
        if layout == "unet":                 # the UNet self-attention: one [q | k] buffer, ldq = ldk = 2C
            assert Sq == Skv
            ldq = ldk = 2 * Cc
            qb = kb = Sq * 2 * Cc
            qk = torch.full((B * qb,), nan, device=dev, dtype=dt)
            qk.as_strided((B, Sq, Cc), (qb, ldq, 1), 0).copy_(q.reshape(B, Sq, Cc))
            qk.as_strided((B, Skv, Cc), (kb, ldk, 1), Cc).copy_(k.reshape(B, Skv, Cc))
            self.qbuf, self.kbuf = qk, qk
            qptr, kptr = qk.data_ptr(), qk.data_ptr() + Cc * qk.element_size()
            ldvt, ldo = Kp, Cc
            vtb, ob = Cc * ldvt, Sq * Cc
        else:
            ldq, ldk = (Cc + 8, Cc + 16) if gaps else (Cc, Cc)
            ldvt, ldo = (Kp + 24, Cc + 12) if gaps else (Kp, Cc)
            qb = Sq * ldq + (40 if gaps else 0)
            kb = 0 if shared else Skv * ldk + (24 if gaps else 0)
            vtb = 0 if shared else Cc * ldvt + (16 if gaps else 0)
            ob = Sq * ldo + (36 if gaps else 0)
            nk = 1 if shared else B
            self.qbuf = torch.full((B * qb,), nan, device=dev, dtype=dt)
            self.qbuf.as_strided((B, Sq, Cc), (qb, ldq, 1)).copy_(q.reshape(B, Sq, Cc))
            self.kbuf = torch.full((nk * max(kb, Skv * ldk),), nan, device=dev, dtype=dt)
            self.kbuf.as_strided((nk, Skv, Cc), (max(kb, 1), ldk, 1)).copy_(k[:nk].reshape(nk, Skv, Cc))
            qptr, kptr = self.qbuf.data_ptr(), self.kbuf.data_ptr()
        nv = 1 if shared else B
        self.vtbuf = torch.full((nv * max(vtb, Cc * ldvt),), nan, device=dev, dtype=dt)
        vt = self.vtbuf.as_strided((nv, Cc, ldvt), (max(vtb, 1), ldvt, 1))
        vt[:, :, :Skv] = v[:nv].reshape(nv, Skv, Cc).transpose(1, 2)
        vt[:, :, Skv:Kp] = pad
        self.out = torch.full(((B - 1) * ob + (Sq + 1) * ldo,), nan, device=dev, dtype=dt)   # one row past Sq
        self.fields = dict(q=qptr, k=kptr, vt=self.vtbuf, out=self.out, B=B, heads=H, Sq=Sq, Skv=Skv, d=d, ldq=ldq, ldk=ldk,
                           ldvt=ldvt, ldo=ldo, qb=qb, kb=kb, vtb=vtb, ob=ob, scale=scale)
        self.oview = (ob, ldo)

    def set_pad(self, val):
        Kp = ceil8(self.Skv)
        f = self.fields
        nv = self.vtbuf.numel() // max(f["vtb"], self.C * f["ldvt"])
        self.vtbuf.as_strided((nv, self.C, f["ldvt"]), (max(f["vtb"], 1), f["ldvt"], 1))[:, :, self.Skv:Kp] = val

    def run(self, ctx, path):
        self.out.fill_(float("nan"))
        rc, got = attn_ex(ctx, force=path, **self.fields)
        ctx.check(rc, "attention_ex")
        torch.cuda.synchronize()
        assert got == tuple(path), "kernel path %s, expected %s" % (got, tuple(path))
        ob, ldo = self.oview
        o = self.out.as_strided((self.B, self.Sq, self.C), (ob, ldo, 1))
        written = torch.zeros(self.out.numel(), dtype=torch.bool, device=self.out.device)
        written.as_strided((self.B, self.Sq, self.C), (ob, ldo, 1)).fill_(True)
        assert bool(self.out[~written].isnan().all()), "%d elements written outside the [B][Sq][heads * d] rows" % (
            int((~self.out[~written].isnan()).sum()))
        assert bool(torch.isfinite(o).all()), "%d valid elements not written or not finite" % int((~torch.isfinite(o)).sum())
        return o.reshape(self.B, self.Sq, self.H, self.d).clone()

    def reference(self):
        f64 = torch.float64
        qh = self.q.to(f64).permute(0, 2, 1, 3)
        kh = self.k.to(f64).permute(0, 2, 1, 3)
        vh = self.v.to(f64).permute(0, 2, 1, 3)
        sc = float(torch.tensor(self.scale, dtype=torch.float32))
        p = torch.softmax((qh @ kh.transpose(-1, -2)) * sc, dim=-1)
        ref = p @ vh
        A = (sc * LOG2E) * (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True)
        spv = p @ vh.abs()
        sv = vh.abs().sum(-2, keepdim=True)
        return ref.permute(0, 2, 1, 3), A.permute(0, 2, 1, 3), spv.permute(0, 2, 1, 3), sv.permute(0, 2, 1, 3)


def check_bound(prob, path, out):
    """the per-element bound of the module docstring, then the aggregate rel-L2 of test_attention"""
    ref, A, spv, sv = prob.reference()
    u = HALF.u
    uq = u if (path[0] == DMA40 or path[4]) else 0.0
    R = (prob.Skv + 63) // 64
    g = 2.0 ** -24 * (math.log(2) * (2 * (prob.d + 3) + 4 * (R + 1)) * A + 2 * (R + 1) + 2 * prob.Skv + 4)
    bound = u * ref.abs() + 1.01 * (u + math.log(2) * uq * A + g) * (spv + ref.abs()) + HALF.tiny * sv
    err = (out.double() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), "%d elements outside the bound; first at (b, q, head, c) = %s: |err| %.3g, bound %.3g" % (
        int((~ok).sum()), tuple(int(i) for i in (~ok).nonzero()[0]), float(err[~ok][0]), float(bound[~ok][0]))
    assert rel_l2(out.float(), ref) < 2 * HALF.tol


# ---- exact selection ---------------------------------------------------------------------------------------------------------
EXACT_SCALE = 0.07        # 2 * 32^2 * 0.07 * log2(e) = 206.8 >= 160 in exp2 units


def selection_problem(B, H, Sq, Skv, d, seed, code=32.0, scale=EXACT_SCALE, shared=False):
    """q, k, v of an exact-selection case and the chosen key of every (b, head, query); shared: one context for every sample"""
    g = torch.Generator().manual_seed(seed)
    m = max(1, math.ceil(math.log2(Skv)))
    assert m <= d and 2 ** m >= Skv, "d = %d holds no %d distinct codes" % (d, Skv)
    q = torch.zeros(B, Sq, H, d, dtype=torch.float64)
    k = torch.randint(-2, 3, (B, Skv, H, d), generator=g).double()         # q is 0 outside the code dimensions
    sgn = torch.randint(0, 2, (B, Skv, H, d), generator=g).double() * 2 - 1
    v = sgn * (0.25 + 3.75 * torch.rand(B, Skv, H, d, generator=g, dtype=torch.float64))      # normal numbers in both types
    dims = {}
    bits = {}
    for b in range(1 if shared else B):
        for h in range(H):
            dims[b, h] = torch.randperm(d, generator=g)[:m]
            codes = torch.randperm(2 ** m, generator=g)[:Skv]
            bits[b, h] = ((codes[:, None] >> torch.arange(m)[None, :]) & 1).double() * 2 - 1      # (Skv, m) of +-1
            k[b, :, h, dims[b, h]] = code * bits[b, h]
    if shared:
        k[1:], v[1:] = k[:1].clone(), v[:1].clone()
    # key 0, the ragged last tile, both sides of every 64-key seam, the rest random; a different order per (b, head)
    special = sorted({0, Skv - 1, Skv - 2, (Skv - 1) // 64 * 64} | {s for t in range(64, Skv, 64) for s in (t - 1, t)})
    special = [s for s in special if 0 <= s < Skv]
    chosen = torch.zeros(B, H, Sq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            ch = torch.randint(0, Skv, (Sq,), generator=g)
            rot = (b * H + h) % len(special)
            sp = special[rot:] + special[:rot]
            pos = torch.randperm(Sq, generator=g)[:len(sp)]
            ch[pos] = torch.tensor(sp[:len(pos)])
            chosen[b, h] = ch
            key = (0 if shared else b, h)
            q[b, :, h, dims[key]] = code * bits[key][ch]
    dt = HALF.dtype
    return q.to(dt).cuda(), k.to(dt).cuda(), v.to(dt).cuda(), chosen.cuda()


def check_selection(prob, chosen, out, scale):
    # the construction: the chosen score leads every other by >= 160 in exp2 units
    qh = prob.q.double().permute(0, 2, 1, 3)
    kh = prob.k.double().permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    top = s.gather(-1, chosen[..., None])
    if prob.Skv > 1:
        others = s.scatter(-1, chosen[..., None], float("-inf")).amax(-1, keepdim=True)
        assert float((top - others).min()) >= 160.0
    want = torch.gather(prob.v.permute(0, 2, 1, 3), 2, chosen[..., None].expand(-1, -1, -1, prob.d)).permute(0, 2, 1, 3)
    bad = out != want
    assert not bool(bad.any()), "%d elements differ from v[chosen]; first at (b, q, head, c) = %s: %g vs %g" % (
        int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(out[bad][0]), float(want[bad][0]))


# (B, heads, Sq, Skv): Sq around the 32-row blocks and the 128 / 256-query workgroups, Skv around the 8-key chunks and the 64-key
# tiles; B * heads never a multiple of 8 (a ragged XCD remap)
SHAPES = [(3, 3, 33, 129), (1, 5, 257, 65), (2, 3, 1, 1100), (1, 1, 513, 9), (3, 1, 31, 77), (2, 5, 129, 8), (1, 3, 255, 1),
          (5, 1, 32, 64), (1, 3, 511, 80), (3, 3, 127, 63), (2, 1, 256, 7), (1, 7, 512, 1024)]


def _pick(pi, k):
    return [SHAPES[(pi * 5 + k * 7 + i * 3) % len(SHAPES)] for i in range(2)]


def _exact_cases():
    out = []
    for pi, p in enumerate(PATHS):
        for j, (B, H, Sq, Skv) in enumerate(_pick(pi, 0)):
            if p[1] == 8:
                Skv = min(Skv, 256)                       # 8 dimensions hold 256 codes
            layout = "dense" if j == 0 else "shared"
            out.append(pytest.param(p, (B, H, Sq, Skv), layout, id="%s-%dx%dx%dx%d-%s" % (path_id(p), B, H, Sq, Skv, layout)))
    # every path once at >= 1024 keys (d = 8: 256)
    for p in PATHS:
        out.append(pytest.param(p, (2, 3, 65, 256 if p[1] == 8 else 1100), "gaps", id="%s-long-gaps" % path_id(p)))
    return out


@pytest.mark.parametrize("path,shape,layout", _exact_cases())
def test_exact_selection(ctx, path, shape, layout):
    B, H, Sq, Skv = shape
    d = path[1]
    q, k, v, chosen = selection_problem(B, H, Sq, Skv, d, zlib.crc32(repr((path, shape, layout)).encode()), shared=layout == "shared")
    prob = Problem(q, k, v, EXACT_SCALE, layout=layout, pad=PAD_BIG)
    check_selection(prob, chosen, prob.run(ctx, path), EXACT_SCALE)


# ---- random data, edge cases of the running max / shift -----------------------------------------------------------------------
def random_problem(B, H, Sq, Skv, d, seed, shared=False):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, H, d, generator=g)
    k = torch.randn(B, Skv, H, d, generator=g)
    v = torch.randn(B, Skv, H, d, generator=g)
    if shared:
        k[1:], v[1:] = k[:1].clone(), v[:1].clone()
    dt = HALF.dtype
    return q.to(dt).cuda(), k.to(dt).cuda(), v.to(dt).cuda()


def _random_cases():
    out = []
    for pi, p in enumerate(PATHS):
        for j, (B, H, Sq, Skv) in enumerate(_pick(pi, 1)):
            layout = ("unet" if Sq == Skv else "dense") if j == 0 else "gaps"
            if j == 0 and Sq != Skv:
                Sq = Skv = max(Sq, Skv) if max(Sq, Skv) <= 600 else 257        # the UNet layout is a self-attention
                layout = "unet"
            out.append(pytest.param(p, (B, H, Sq, Skv), layout, id="%s-%dx%dx%dx%d-%s" % (path_id(p), B, H, Sq, Skv, layout)))
    return out


@pytest.mark.parametrize("path,shape,layout", _random_cases())
def test_random_bound(ctx, path, shape, layout):
    B, H, Sq, Skv = shape
    q, k, v = random_problem(B, H, Sq, Skv, path[1], zlib.crc32(repr((path, shape, layout)).encode()))
    prob = Problem(q, k, v, 1.0 / math.sqrt(path[1]), layout=layout)
    out = prob.run(ctx, path)
    check_bound(prob, path, out)
    if Skv % 8:
        prob.set_pad(PAD_BIG)                 # large finite pad keys: bit-identical
        assert torch.equal(prob.run(ctx, path), out), "a finite V^T pad changed the result"


@pytest.mark.parametrize("path", [pytest.param(p, id=path_id(p)) for p in PATHS])
def test_running_max_edges(ctx, path):
    """four heads, four shift regimes (B = 3, 65 queries, 333 keys = 5 tiles + a ragged one of 13):
    head 0, scores that grow by ~8 exp2 units every tile (a rescale / shift move on every tile);
    head 1, a spike of ~+40 exp2 units in the ragged last tile for a third of the queries;
    head 2, a first tile whose scores are ~-60 exp2 units below the rest;
    head 3, |scores * scale * log2(e)| up to ~100."""
    d = path[1]
    B, H, Sq, Skv = 3, 4, 65, 333
    scale = 1.0 / math.sqrt(d)
    c = scale * LOG2E
    g = torch.Generator().manual_seed(zlib.crc32(repr(path).encode()))
    q = torch.randn(B, Sq, H, d, generator=g, dtype=torch.float64)
    k = torch.randn(B, Skv, H, d, generator=g, dtype=torch.float64)
    v = torch.randn(B, Skv, H, d, generator=g, dtype=torch.float64)
    tile = torch.arange(Skv) // 64
    q[:, :, 0, 0] = 1.0
    k[:, :, 0, 0] = round(8.0 / c) * tile.double()                             # +8 per tile
    lead = Sq // 3
    for b in range(B):
        w = q[b, :lead, 1, :].mean(0)
        k[b, Skv - 3, 1, :] = w * (40.0 / c) / float(w.pow(2).sum())
    q[:, :, 2, 0] = 1.0
    k[:, :, 2, 0] = torch.where(tile == 0, -float(round(60.0 / c)), 0.0).double()
    s3 = (q[:, :, 3] @ k[:, :, 3].transpose(-1, -2)).abs().amax() * c
    a = math.sqrt(100.0 / float(s3))
    q[:, :, 3] *= a
    k[:, :, 3] *= a
    dt = HALF.dtype
    prob = Problem(q.to(dt).cuda(), k.to(dt).cuda(), v.to(dt).cuda(), scale, layout="gaps", pad=PAD_BIG)
    sc = prob.q.double().permute(0, 2, 1, 3) @ prob.k.double().permute(0, 2, 3, 1) * c
    assert float(sc[:, 3].abs().amax()) > 80 and float(sc[:, 1, :lead, Skv - 3].mean()) > 20
    check_bound(prob, path, prob.run(ctx, path))


@pytest.mark.parametrize("path", [pytest.param(p, id=path_id(p)) for p in PATHS])
def test_batch_invariance(ctx, path):
    """bit-exact: permuting the samples of a batch permutes the outputs; a B = 1 call on one sample equals its slice of B = 3"""
    d = path[1]
    B, H, Sq, Skv = 3, 3, 97, 150
    q, k, v = random_problem(B, H, Sq, Skv, d, 77 + d)
    scale = 1.0 / math.sqrt(d)
    full = Problem(q, k, v, scale, layout="gaps", pad=PAD_BIG).run(ctx, path)
    perm = torch.tensor([2, 0, 1], device="cuda")
    permuted = Problem(q[perm], k[perm], v[perm], scale, layout="dense").run(ctx, path)
    assert torch.equal(permuted, full[perm])
    one = Problem(q[1:2], k[1:2], v[1:2], scale, layout="dense").run(ctx, path)
    assert torch.equal(one, full[1:2])


def test_default_dispatch(ctx):
    """without a forced variant the library picks what the UNet always took (default SVG_ATTN_* knobs): dma40 for d = 40 at >= 512
    queries, the bias-column form below that, QB = 2 (and BC + HV at d = 8) from 512 queries for d <= 64, one block above"""
    want = {(40, 4096): (DMA40, 40, 2, 3, 1, 1), (40, 512): (DMA40, 40, 2, 3, 1, 1), (40, 511): (REG, 40, 1, 1, 1, 0),
            (40, 256): (REG, 40, 1, 1, 1, 0), (80, 1024): (REG, 80, 1, 1, 0, 0), (160, 256): (REG, 160, 1, 1, 0, 0),
            (160, 64): (REG, 160, 1, 1, 0, 0), (64, 512): (REG, 64, 2, 1, 0, 0), (64, 100): (REG, 64, 1, 1, 0, 0),
            (8, 600): (REG, 8, 2, 1, 1, 1), (8, 200): (REG, 8, 1, 1, 1, 0), (16, 700): (REG, 16, 2, 1, 0, 0),
            (32, 33): (REG, 32, 1, 1, 0, 0)}
    for (d, Sq), p in want.items():
        q, k, v = random_problem(1, 2, Sq, 77, d, Sq + d)
        prob = Problem(q, k, v, 1.0 / math.sqrt(d))
        rc, got = attn_ex(ctx, **prob.fields)
        ctx.check(rc, "attention_ex")
        torch.cuda.synchronize()
        assert got == p, "d %d, Sq %d: default path %s, expected %s" % (d, Sq, got, p)


def test_refusals(ctx):
    """variants that are not instantiated for d, an unsupported d, a short ldvt, misaligned strides: an error, nothing written"""
    def refused(what, prob, force=None, **over):
        prob.out.fill_(float("nan"))
        f = dict(prob.fields, **over)
        rc, _ = attn_ex(ctx, force=force, **f)
        torch.cuda.synchronize()
        assert rc == _lib.SVG_ERR_INVALID, "%s: status %d, expected a refusal" % (what, rc)
        assert len(ctx.lib.svg_last_error(ctx.h)) > 0
        assert bool(prob.out.isnan().all()), what + ": out was written"

    probs = {d: Problem(*random_problem(2, 2, 64, 40, d, d), 0.1) for d in (16, 40, 80, 160)}
    refused("BC at d = 16", probs[16], (REG, 16, 1, 1, 1, 0))
    refused("BC at d = 80", probs[80], (REG, 80, 1, 1, 1, 0))
    refused("QB = 2 at d = 80", probs[80], (REG, 80, 2, 1, 0, 0))
    refused("dma40 at d = 16", probs[16], (DMA40, 16, 2, 3, 1, 1))
    refused("dma40 at d = 80", probs[80], (DMA40, 80, 2, 3, 1, 1))
    refused("dma40 with other fields", probs[40], (DMA40, 40, 1, 1, 1, 0))
    refused("HV without BC", probs[16], (REG, 16, 2, 1, 0, 1))
    refused("HV at QB = 1", probs[40], (REG, 40, 1, 1, 1, 1))
    refused("BC with two stages", probs[40], (REG, 40, 1, 2, 1, 0))
    refused("two stages at d = 160", probs[160], (REG, 160, 1, 2, 0, 0))
    refused("three stages", probs[16], (REG, 16, 1, 3, 0, 0))
    refused("unknown kernel", probs[16], (5, 16, 1, 1, 0, 0))
    refused("d = 24", probs[16], None, d=24, ldq=48, ldk=48, ldo=48)
    refused("d = 24, forced", probs[16], (REG, 24, 1, 1, 0, 0), d=24, ldq=48, ldk=48, ldo=48)
    refused("ldvt below ceil8(Skv)", probs[40], None, ldvt=32, Skv=40 + 1)
    refused("ldvt below ceil8(Skv), forced dma40", probs[40], (DMA40, 40, 2, 3, 1, 1), Skv=41)
    refused("ldq not a multiple of 8", probs[40], None, ldq=84)
    refused("ldk not a multiple of 8", probs[40], (DMA40, 40, 2, 3, 1, 1), ldk=84)
    refused("ldvt not a multiple of 8", probs[40], None, ldvt=44)
    refused("ldo not a multiple of 4", probs[40], None, ldo=82)
    refused("no keys", probs[40], None, Skv=0)


# ---- VAE fused attention (attn_vae.hip) -------------------------------------------------------------------------------------
VAE_C = 512


def vae_run(ctx, q, k, v, pad_cols=8, ldo_pad=8):
    """q, k, v (B, S, 512): q | k interleaved in one buffer (ldqk = 2C, vae.cpp), V^T rows of S + pad_cols (NaN past S), out rows of
    C + ldo_pad in a NaN-filled buffer with gaps between samples; returns out (B, S, C)"""
    B, S, Cc = q.shape
    dt = q.dtype
    nan = float("nan")
    qkb = S * 2 * Cc
    qk = torch.full((B * qkb,), nan, device="cuda", dtype=dt)
    qk.as_strided((B, S, Cc), (qkb, 2 * Cc, 1), 0).copy_(q)
    qk.as_strided((B, S, Cc), (qkb, 2 * Cc, 1), Cc).copy_(k)
    ldvt = S + pad_cols
    vtb = Cc * ldvt + 16
    vt = torch.full((B * vtb,), nan, device="cuda", dtype=dt)
    vt.as_strided((B, Cc, S), (vtb, ldvt, 1)).copy_(v.transpose(1, 2))
    ldo = Cc + ldo_pad
    ob = S * ldo + 24
    out = torch.full((B * ob,), nan, device="cuda", dtype=dt)
    es = qk.element_size()
    rc = getattr(ctx.lib, "svg_op_vae_attention" + HALF.suffix)(ctx.h, qk.data_ptr(), qk.data_ptr() + Cc * es, 2 * Cc, qkb, vt.data_ptr(),
                                                                 ldvt, vtb, out.data_ptr(), ldo, ob, B, S, Cc, stream())
    ctx.check(rc, "vae_attention")
    torch.cuda.synchronize()
    o = out.as_strided((B, S, Cc), (ob, ldo, 1))
    written = torch.zeros(out.numel(), dtype=torch.bool, device="cuda")
    written.as_strided((B, S, Cc), (ob, ldo, 1)).fill_(True)
    assert bool(out[~written].isnan().all()), "vae_attention wrote outside its rows"
    assert bool(torch.isfinite(o).all()), "vae_attention left valid elements unwritten or not finite"
    return o.clone()


VAE_SHAPES = [(1, 64), (3, 128), (3, 640), (1, 4096)]


@pytest.mark.parametrize("B,S", VAE_SHAPES)
def test_vae_attention_exact_selection(ctx, B, S):
    """codes of 64 (the kernel's scale is 1 / sqrt(512): 2 * 64^2 / sqrt(512) * log2(e) = 522 exp2 units of margin); v[chosen] bit
    for bit: the chosen P is exp2(0) = 1 exactly and the row sum is that P"""
    scale = 1.0 / math.sqrt(VAE_C)
    q, k, v, chosen = selection_problem(B, 1, S, S, VAE_C, 9000 + S + B, code=64.0, scale=scale)
    prob = Problem(q, k, v, scale)      # (for check_selection's construction check only)
    out = vae_run(ctx, q[:, :, 0], k[:, :, 0], v[:, :, 0])
    check_selection(prob, chosen, out[:, :, None, :], scale)


@pytest.mark.parametrize("B,S", VAE_SHAPES)
def test_vae_attention_bound(ctx, B, S):
    """the module's per-element bound re-derived for this kernel: P is rounded to the storage type and the row sum is built from the
    rounded P (u); Q is not pre-scaled (u_Q = 0); the scores are four f32 partial sums of 128 products each, added in f32, then scaled
    (d = 512 in g_i); the shift and rescale factor move once per 32-key tile (R = S / 32); PV and the row sums accumulate S keys."""
    g = torch.Generator().manual_seed(S + B)
    dt = HALF.dtype
    q = (torch.randn(B, S, VAE_C, generator=g) * 0.5).to(dt).cuda()
    k = (torch.randn(B, S, VAE_C, generator=g) * 0.5).to(dt).cuda()
    v = torch.randn(B, S, VAE_C, generator=g).to(dt).cuda()
    k[:, S // 3] = (q[:, S // 5] * 2).to(dt)                       # one dominant key for some queries, outside the first tile
    out = vae_run(ctx, q, k, v)
    scale = 1.0 / math.sqrt(VAE_C)
    prob = Problem(q[:, :, None], k[:, :, None], v[:, :, None], scale)
    ref, A, spv, sv = prob.reference()
    ref, A, spv, sv = ref[:, :, 0], A[:, :, 0], spv[:, :, 0], sv[:, :, 0]
    u = HALF.u
    R = S // 32
    gm = 2.0 ** -24 * (math.log(2) * (2 * (VAE_C + 3) + 4 * (R + 1)) * A + 2 * (R + 1) + 2 * S + 4)
    bound = u * ref.abs() + 1.01 * (u + gm) * (spv + ref.abs()) + HALF.tiny * sv
    err = (out.double() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), "%d elements outside the bound; worst |err| %.3g" % (int((~ok).sum()), float(err.max()))
    assert rel_l2(out.float(), ref) < 2 * HALF.tol


def test_vae_attention_refusals(ctx):
    dt = HALF.dtype
    S = 128
    buf = torch.zeros(2 * S * 2 * VAE_C + 4096, device="cuda", dtype=dt)
    vt = torch.zeros(2 * VAE_C * (S + 64), device="cuda", dtype=dt)
    out = torch.full((2 * S * VAE_C + 4096,), float("nan"), device="cuda", dtype=dt)
    fn = getattr(ctx.lib, "svg_op_vae_attention" + HALF.suffix)

    def refused(what, S=S, Cc=VAE_C, ldqk=2 * VAE_C, ldvt=S, ldo=VAE_C):
        rc = fn(ctx.h, buf.data_ptr(), buf.data_ptr(), ldqk, S * ldqk, vt.data_ptr(), ldvt, Cc * ldvt, out.data_ptr(), ldo, S * ldo, 2, S,
                Cc, stream())
        torch.cuda.synchronize()
        assert rc == _lib.SVG_ERR_INVALID, "%s: status %d, expected a refusal" % (what, rc)
        assert bool(out.isnan().all()), what + ": out was written"

    refused("S % 64 != 0", S=96, ldvt=96)
    refused("C != 512", Cc=256, ldqk=512, ldo=256)
    refused("ldqk not a multiple of 8", ldqk=2 * VAE_C + 4)
    refused("ldvt not a multiple of 8", ldvt=S + 4)
    refused("ldo not a multiple of 4", ldo=VAE_C + 2)
    refused("ldvt < S", ldvt=S - 8)


# ---- the C = 320 cross-attention in one launch (xattn_fused.hip) -------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8, 64, 65, 80])
@pytest.mark.parametrize("rows", [128, 384])
def test_xattn_fused_contexts(ctx, L, rows):
    """xattn_fused at every context length class (the kernel masks keys 16 t + 4 lq + e >= L for L <= 80) and samples of 128 and
    384 rows, three samples with distinct contexts: out starts as NaN and is written everywhere; swapping two samples' contexts
    swaps their outputs bit for bit; the attention branch against fp64 (see _xattn_bound)."""
    Cc, H, D = 320, 8, 40
    Lp = ceil8(L)
    N = 3
    M = N * rows
    dt = HALF.dtype
    g = torch.Generator().manual_seed(31 * L + rows)
    rnd = lambda *sh: torch.randn(*sh, generator=g).cuda()
    wq, wo = rnd(Cc, Cc) / math.sqrt(Cc), rnd(Cc, Cc) / math.sqrt(Cc)
    bo = 0.1 * rnd(Cc)
    gamma, beta = 1.0 + 0.1 * rnd(Cc), 0.1 * rnd(Cc)
    x = rnd(M, Cc).to(dt)
    x[rows:2 * rows] = x[:rows]                       # samples 0 and 1: the same rows, different contexts
    k = rnd(N, L, Cc).to(dt)
    v = rnd(N, L, Cc).to(dt)

    def run(kk, vv):
        vt = torch.full((N, Cc, Lp), PAD_BIG, device="cuda", dtype=dt)
        vt[:, :, :L] = vv.transpose(1, 2)
        out = torch.full((M, Cc), float("nan"), device="cuda", dtype=dt)
        rc = getattr(ctx.lib, "svg_op_xattn_fused" + HALF.suffix)(ctx.h, x.data_ptr(), None, None, None, None, gamma.data_ptr(),
                                                                   beta.data_ptr(), wq.data_ptr(), kk.contiguous().data_ptr(),
                                                                   vt.data_ptr(), Lp, wo.data_ptr(), bo.data_ptr(), out.data_ptr(), M,
                                                                   rows, L, stream())
        ctx.check(rc, "xattn_fused")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), "%d elements not written or not finite" % int((~torch.isfinite(out)).sum())
        return out

    out = run(k, v)
    o3 = out.view(N, rows, Cc)
    assert not torch.equal(o3[0], o3[1]), "samples 0 and 1 share their rows but not their contexts"
    sw = torch.tensor([1, 0, 2], device="cuda")
    o_sw = run(k[sw].contiguous(), v[sw].contiguous()).view(N, rows, Cc)
    assert torch.equal(o_sw, o3[sw]), "swapping the contexts of two samples with equal rows did not swap their outputs"
    _xattn_bound(x.float(), gamma, beta, wq, wo, bo, k, v, out, N, rows, L)


def _xattn_bound(x32, gamma, beta, wq, wo, bo, k, v, out, N, rows, L):
    """The attention branch y = out - x against fp64, per element.  The kernel forms q with the LayerNorm folded into 16-bit weights
    W_q' = W_q diag(gamma) and f32 statistics, rounds q, P and the attention output O to the storage type, and applies to_out with
    16-bit W_out in f32.  With q, a = softmax(q k^T / sqrt(40)) v and y_ref = a W_out^T + b_out formed in fp64:
      dq   = u |q| + (u + 40 * 2^-20) |x_n| |W_q'|^T + u |W_q beta|   (rounding of q and of the weights, f32 to_q of 320 products
             and the statistics, for rows of near-zero mean as here);
      dA_i = c max_j sum_k dq_ik |k_jk|                               (how far q's error moves an exp2 argument, c = log2(e) / sqrt(40));
      e_a  = (u + ln2 dA_i + g_i) (sum_j p_ij |v_j| + |a_i|)          (the attention bound of the module docstring, one key tile);
      |out - x - y_ref| <= u |x + y_ref| + 1.01 [ (e_a + u |a|) |W_out|^T + u |a| |W_out|^T + 322 * 2^-24 (|a| |W_out|^T + |b_out| + |x|) ]
    (O's rounding, W_out's rounding, the f32 accumulation of to_out, bias and residual; the output rounding)."""
    f64 = torch.float64
    C_, H, D = 320, 8, 40
    u = HALF.u
    M = N * rows
    xd = x32.double()
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    xn = (xd - mu) / torch.sqrt(var + 1e-5)
    wqg = wq.double() * gamma.double()[None, :]
    qd = xn @ wqg.t() + (wq.double() @ beta.double())[None, :]
    dq = u * qd.abs() + (u + 40 * 2.0 ** -20) * (xn.abs() @ wqg.abs().t()) + u * (wq.double() @ beta.double()).abs()[None, :]
    q4 = qd.view(N, rows, H, D).transpose(1, 2)
    dq4 = dq.view(N, rows, H, D).transpose(1, 2)
    kk = k.to(f64).view(N, L, H, D).transpose(1, 2)
    vv = v.to(f64).view(N, L, H, D).transpose(1, 2)
    c = LOG2E / math.sqrt(D)
    p = torch.softmax(q4 @ kk.transpose(-1, -2) / math.sqrt(D), dim=-1)
    a = p @ vv
    A = c * (q4.abs() @ kk.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    dA = c * (dq4 @ kk.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    gi = 2.0 ** -24 * (math.log(2) * (2 * (D + 8) + 8) * (A + dA) + 6 + 2 * L + 4)
    ea = (u + math.log(2) * dA + gi) * (p @ vv.abs() + a.abs())
    ea = ea.transpose(1, 2).reshape(M, C_)
    a2 = a.transpose(1, 2).reshape(M, C_)
    wod = wo.double()
    yref = a2 @ wod.t() + bo.double()[None, :]
    e = ((ea + u * a2.abs()) @ wod.abs().t() + u * (a2.abs() @ wod.abs().t())
         + 2.0 ** -24 * (C_ + 2) * (a2.abs() @ wod.abs().t() + bo.double().abs()[None, :] + xd.abs()))
    bound = u * (xd + yref).abs() + 1.01 * e
    err = (out.double() - (xd + yref)).abs()
    ok = err <= bound
    assert bool(ok.all()), "%d elements outside the bound; worst |err| %.3g (bound there %.3g)" % (
        int((~ok).sum()), float(err.max()), float(bound.flatten()[int(err.argmax())]))
    assert rel_l2(out.double() - xd, yref) < 4 * HALF.tol
