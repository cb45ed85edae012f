"""The fused GEGLU feed-forward (csrc/ff_fused.hip: ff_pair_kernel) against fp64, element by element.

    out = ff.net.2( GEGLU( LayerNorm(x) W1^T + b1 ) ) + b2 + residual,  C = 320, 1280 hidden units, one launch.

The kernel has its own statistics, LayerNorm fold, GELU call site, P rounding, LDS swap between the waves of a pair, k-permuted and
column-dealt W2 and epilogue; none of it goes through gemm_plan() or the shared tile epilogue, and the UNet reaches it from 24 576 rows
up only.  Here it is driven through svg_op_ff_fused(_f16) at M in {1, 16, 17, 32, 33, 127, 128, 129, 333}: an MFMA row tile is 16 rows, a
wave pair owns 32, a workgroup 128.

THE JUDGE (judge()).  A worst-case bound through both GEMMs is useless (the 16-bit roundings of W1' and P summed in magnitude over
K = 320 and K = 1280 give 1-6 |y|), so the fp64 reference multiplies the operands the kernel multiplies and rounds where it rounds:
    W1~ = round16(f32(W1 gamma))   (fold_ln: one f32 product; pack_geglu: one conversion)      b1' = b1 + W1 beta
    s1  = row sums of W1~           W2~ = round16(W2)
    mean, var: fp64 from the 16-bit x;  rs = (var + 1e-5f)^-1/2
    t = acc rs - s1 rs mean + b1'   (acc = x W1~^T);  h | g = the two halves of t;  p = h gelu(g), exact erf form
    P~ = round16(p);   y = P~ W2~^T + b2 + residual
test_fold_premise checks W1~ (bit for bit), b1' and s1 against svg_op_fold_ln / svg_op_rowsum.

Error carried into p, e = 2^-24 (f32 unit roundoff), C = 320, A = mean |x| of the row, v = var + eps:
    dmean = (C/4 + 4) e A          a lane adds its 80 values in sequence (79 additions), two shuffle additions, the product with the
                                   rounded constant 1/320 (2 e); 2 e |mean| on a row whose sum is exact in f32 (below)
    rel(rs) = (C/8 + 8) e + dmean^2 / (2 v)
                                   two-pass variance in f32: 3 e per term (the difference, squared, and the square), 81 additions, the
                                   product with 1/320 (2 e), the sum with eps (e): (C/4 + 7) e on v, half of it on v^-1/2, and rsqrtf at
                                   2 ulp (4 e): 47.5 e, taken as (C/8 + 8) e = 48 e.  (A looser term here lets an output column
                                   off by one fp16 ulp through on the grid class: test_judge_rejects_cpu[col_ulp] guards it.)
                                   The second term is the variance taken about mean^ instead of mean: sum (x - mean^)^2 = sum (x - mean)^2
                                   + C (mean^ - mean)^2 exactly, so v^ <= v + dmean^2 and rs^ >= rs (1 - dmean^2 / (2 v)); it matters on
                                   constant rows far from zero only (v = eps there)
    d(rm) = rs dmean + |rs mean| (rel(rs) + e)                               rm = fl(rs^ mean^)
    d(acc) = (C + 2) e |x| |W1~|^T                                            GEMM1's f32 accumulation
    d(s1) = (ceil(C / 256) + 8) e sum |W1~|      d(b1') = (ceil(C / 256) + 9) e |W1| |beta| + e |b1'|, 0 if beta = 0
                                   the bounds test_norm_paths_gpu.py asserts for rowsum_h16 / fold_ln (per-thread run, six shuffle levels,
                                   two LDS levels, the sum with bias_in): the judge takes s1 and b1' in fp64 and does not replay their order
    dt = rs d(acc) + |acc rs| (rel(rs) + e) + |s1| d(rm) + d(s1) |rs mean| + e |s1 rs mean| + e |acc rs - s1 rs mean| + e |t| + d(b1')
                                   (the three f32 operations of the fold: two products, the difference, the sum with b1')
    dp = |gelu(g)| dh + (|h| + dh) (1.13 dg + GELU_ABS_ERR + 2 e |gelu(g)|) + 2 e |p|
                                   1.13: gelu's largest slope; GELU_ABS_ERR = 2.7e-7: gelu_erf's documented error (csrc/igemm_epi.h)
Exact sums: if every term of a sum is a multiple of a power of two q and the magnitudes of the terms add up to at most 2^24 q, every
partial sum is representable and the f32 sum is exact in any order (sums_exact()).  Per row, with q the product of the largest powers
of two dividing the row's x and the whole W1~: where that holds for GEMM1, d(acc) = 0; for the row's own sum, dmean = 2 e |mean|; for
a row of W1~, d(s1) = 0.  The grid class meets all three in every row (test_emulation_cpu checks it against f32 arithmetic), and so do
the shifted rows of the offset class behind the one-hot-W2 data's W1 (their x are coarse multiples of a power of two): there the bound is the
statistics' and the fold's alone, which is what lets the judge see a one-pass variance.
Rounding of P:  lo = round16(p - dp), hi = round16(p + dp): a hidden unit whose interval straddles a rounding boundary may land on
either side.  Per element, none left out:
    |out - y| <= u |y| + tiny + 1.01 [ (hi - lo) |W2~|^T + (1280 + 4) e (|P~| |W2~|^T + |b2| + |res|) ]
u = 2^-8 (bf16) / 2^-11 (fp16): the one output rounding; tiny = 2^-134 / 2^-25: half the spacing of the storage type's subnormals,
where u |y| is no longer the rounding error (fp16 outputs below 2^-14); 1280 + 4: GEMM2's f32 accumulation and the epilogue's sums;
1.01: products of two of the terms above.

Exact cases (the exact GEMM2 data; the gates of the one-hot-W2 data): a gate pre-activation of 8 gives gelu_erf(8) = 8.0f by the kernel's own formula
(8 - 8 * 2^p(6), 2^p(6) ~ 1e-9, less than half an ulp of 8), and with W1 = 0 the fold returns b1 whatever the statistics are.

test_emulation_cpu / test_judge_rejects_cpu run an f32 torch emulation of the kernel's arithmetic through the same judge and the same
data without a GPU, and require the judge to reject ten mutations of it.  Every test runs in bf16 and fp16 storage."""
import math
import threading

import pytest
import torch

from conftest import margin
from sd_video_gen_amd import _lib
from test_gemm_epilogue_gpu import GELU_ABS_ERR, HALF, _gelu_exact, _storage, stream  # noqa: F401  (_storage: the autouse fixture)

gpu = pytest.mark.gpu
E32 = 2.0 ** -24
C, FH = 320, 1280
ROWS = [1, 16, 17, 32, 33, 127, 128, 129, 333]
EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the kernel's 1e-5f
PAD = 64                                                  # NaN rows behind the output
F64 = torch.float64


def tiny():
    return 2.0 ** -134 if HALF.dtype == torch.bfloat16 else 2.0 ** -25


def r16(t):
    """round to the storage type, back in fp64"""
    return t.to(HALF.dtype).to(F64)


def cdiv(a, b):
    return (a + b - 1) // b


class Data:
    """one problem: x (M, C) and res (M, C) | None in the storage type, the f32 parameters in the state_dict layout (w1 = [h; gate])"""

    def __init__(self, x, gamma, beta, w1, b1, w2, b2, res, kinds=None):
        self.x, self.gamma, self.beta, self.w1, self.b1, self.w2, self.b2, self.res = x, gamma, beta, w1, b1, w2, b2, res
        self.kinds = kinds            # offset class: (names, kind of every row)

    def to(self, dev):
        mv = lambda t: None if t is None else t.to(dev)
        return Data(mv(self.x), mv(self.gamma), mv(self.beta), mv(self.w1), mv(self.b1), mv(self.w2), mv(self.b2), mv(self.res),
                    None if self.kinds is None else (self.kinds[0], self.kinds[1].to(dev)))

    def rows(self, idx):
        return Data(self.x[idx].contiguous(), self.gamma, self.beta, self.w1, self.b1, self.w2, self.b2,
                    None if self.res is None else self.res[idx].contiguous(), None)


# ---- the data classes (generated on the CPU: the GPU tests and the CPU emulation see the same numbers) --------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def params_random(g):
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    w1 = torch.randn(2 * FH, C, generator=g) / math.sqrt(C)
    b1 = 0.1 * torch.randn(2 * FH, generator=g)
    w2 = torch.randn(C, FH, generator=g) / math.sqrt(FH)
    b2 = 0.1 * torch.randn(C, generator=g)
    return gamma, beta, w1, b1, w2, b2


def data_random(M, seed=1):
    """the distribution of test_ops_gpu.py::test_ff_fused"""
    g = _gen(1, M, seed)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(HALF.dtype)
    p = params_random(g)
    res = torch.randn(M, C, generator=g).to(HALF.dtype)
    return Data(x, *p, res)


def data_grid(M):
    """x in eighths within [-2, 2], W1 in 32nds within +-1/8, gamma 1, beta 0: every product of GEMM1 is a multiple of 1/256 and every
    partial sum stays below 80, so acc and s1 are exact in f32"""
    g = _gen(2, M)
    x = (_randint(g, -16, 16, (M, C)) / 8).to(HALF.dtype)
    w1 = _randint(g, -4, 4, (2 * FH, C)) / 32
    b1 = _randint(g, -16, 16, (2 * FH,)) / 16
    w2 = _randint(g, -8, 8, (C, FH)) / 64
    b2 = _randint(g, -8, 8, (C,)) / 4
    res = (_randint(g, -16, 16, (M, C)) / 8).to(HALF.dtype)
    return Data(x, torch.ones(C), torch.zeros(C), w1, b1, w2, b2, res)


def offset_kinds():
    shifts = [8, 64, 512] if HALF.dtype == torch.bfloat16 else [8, 64]       # fp16: up to 64
    return ["plain"] + ["shift %d sigma" % s for s in shifts] + ["constant", "zero", "scaled 2^-10", "scaled 2^6"], shifts


def data_offset(M):
    """random rows next to rows shifted by a multiple of their standard deviation, constant rows (variance 0), all-zero rows and rows
    scaled by 2^-10 / 2^6: the fold's cancellation acc rs - s1 rs mean and the in-kernel two-pass variance"""
    g = _gen(3, M)
    names, shifts = offset_kinds()
    kind = (torch.arange(M) + M) % len(names)
    x = torch.randn(M, C, generator=g) * 1.5
    for i, s in enumerate(shifts):
        x[kind == 1 + i] += s * 1.5
    nk = 1 + len(shifts)
    consts = torch.tensor([0.3, -1.0, 7.25, 64.0, -0.0123])
    rows_c = (kind == nk).nonzero().flatten()
    x[rows_c] = consts[torch.arange(rows_c.numel()) % consts.numel()][:, None].expand(-1, C)
    x[kind == nk + 1] = 0
    x[kind == nk + 2] *= 2.0 ** -10
    x[kind == nk + 3] *= 2.0 ** 6
    p = params_random(g)
    res = torch.randn(M, C, generator=g).to(HALF.dtype)
    return Data(x.to(HALF.dtype), *p, res, kinds=(names, kind))


def data_exact(M):
    """exact GEMM2 data: W1 = 0 (t = b1 whatever LayerNorm does), every gate bias 8 (gelu_erf(8) = 8.0f), h biases integers / 8 in [-1, 1]: P is an
    integer in [-8, 8]; W2 dense integers in [-2, 2], b2 in quarters, residual integers in [-64, 64]: every product and partial sum of
    GEMM2 and the epilogue is exact in f32 (|sum| <= 1280 * 16 + 16 + 64)"""
    g = _gen(4, M)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.2
    x[M // 2] = 1.75                                                   # a constant row
    hb = _randint(g, -8, 8, (FH,)) / 8
    b1 = torch.cat([hb, torch.full((FH,), 8.0)])
    w2 = _randint(g, -2, 2, (C, FH))
    b2 = _randint(g, -16, 16, (C,)) / 4
    res = _randint(g, -64, 64, (M, C)).to(HALF.dtype)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return Data(x.to(HALF.dtype), gamma, beta, torch.zeros(2 * FH, C), b1, w2, b2, res)


def exact_want(d):
    P = 8.0 * d.b1[:FH].to(F64)
    y = (d.w2.to(F64) @ P)[None, :] + d.b2.to(F64)[None, :] + d.res.to(F64)
    return y.to(HALF.dtype)


def onehot_w2(r):
    """output column n reads hidden unit 4 n + r with weight 1"""
    w2 = torch.zeros(C, FH)
    w2[torch.arange(C), 4 * torch.arange(C) + r] = 1.0
    return w2


def data_gemm1(M, r, offset=False):
    """one-hot W2, GEMM1: gate rows of W1 zero and gate biases 8 (gate = 8.0f exactly), h rows dense integers / 32, gamma 1, beta 0, h biases 0;
    one-hot W2, b2 = 0, no residual: out = round16(round16(8 h)), h = (x . w - mean s1) rs.  offset: the rows of the offset class — behind
    the one-hot W2 the bound is that of ONE hidden unit, not a sum of 1280 magnitudes, so a statistic off in its fourth digit shows"""
    g = _gen(5, M)                                                     # the same x and W1 in all four rounds
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(HALF.dtype)
    kinds = None
    if offset:
        do = data_offset(M)
        x, kinds = do.x, do.kinds
    w1 = torch.cat([_randint(g, -4, 4, (FH, C)) / 32, torch.zeros(FH, C)])
    b1 = torch.cat([torch.zeros(FH), torch.full((FH,), 8.0)])
    return Data(x, torch.ones(C), torch.zeros(C), w1, b1, onehot_w2(r), torch.zeros(C), None, kinds=kinds)


def gelu_ramp():
    """1280 gate values over [-8, 8]: a coarse sweep, dense near 0 and on both sides of +-6 (where the polynomial clamps), dealt to the
    hidden units by a fixed permutation"""
    f = torch.float64
    v = torch.cat([torch.linspace(-8, 8, 512, dtype=f), torch.linspace(-0.25, 0.25, 256, dtype=f),
                   torch.linspace(-6.5, -5.5, 192, dtype=f), torch.linspace(5.5, 6.5, 192, dtype=f), torch.linspace(-5, -1, 128, dtype=f)])
    assert v.numel() == FH
    return v[torch.randperm(FH, generator=_gen(6))].float()


def data_gelu(M, r):
    """one-hot W2, GELU: W1 = 0, h biases 1, gate biases the ramp: p = gelu_erf(ramp) unmixed, out = round16(p)"""
    g = _gen(7, M)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(HALF.dtype)
    b1 = torch.cat([torch.ones(FH), gelu_ramp()])
    return Data(x, torch.ones(C), torch.zeros(C), torch.zeros(2 * FH, C), b1, onehot_w2(r), torch.zeros(C), None)


# ---- the judge -------------------------------------------------------------------------------------------------------------------------
def quantum(t):
    """per element of an fp64 tensor the largest power of two that divides it (inf for 0)"""
    m, ex = torch.frexp(t)
    iv = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (iv & -iv).to(F64)
    return torch.where(t == 0, torch.full_like(t, float("inf")), torch.ldexp(low, ex - 53))


def sums_exact(absdot, q):
    """a sum of terms that are all multiples of q is exact in f32, in any order, if the sum of their magnitudes stays below 2^24 q"""
    return absdot <= 2.0 ** 24 * q


def operands(d):
    """W1~, b1', s1, W2~ in fp64 and the error bounds of b1' and s1 (module docstring)"""
    W1t = (d.w1 * d.gamma[None, :]).to(HALF.dtype).to(F64)
    terms = (d.w1.to(F64).abs() @ d.beta.to(F64).abs())
    b1p = d.b1.to(F64) + d.w1.to(F64) @ d.beta.to(F64)
    db1 = ((cdiv(C, 256) + 9) * E32 * terms + E32 * b1p.abs()) * (terms > 0)
    s1 = W1t.sum(1)
    s1abs = W1t.abs().sum(1)
    ds1 = (cdiv(C, 256) + 8) * E32 * s1abs * ~sums_exact(s1abs, quantum(W1t).amin(1))
    return W1t, b1p, db1, s1, ds1, d.w2.to(HALF.dtype).to(F64)


def reference(d):
    """(y, bound) of the module docstring, both (M, C) fp64, on d's device"""
    W1t, b1p, db1, s1, ds1, W2t = operands(d)
    x = d.x.to(F64)
    qx = quantum(x).amin(1, keepdim=True)
    mean = x.mean(1, keepdim=True)
    v = ((x - mean) ** 2).mean(1, keepdim=True) + EPS
    rs = v ** -0.5
    sum_exact = sums_exact(x.abs().sum(1, keepdim=True), qx)
    dmean = torch.where(sum_exact, 2 * E32 * mean.abs(), (C / 4 + 4) * E32 * x.abs().mean(1, keepdim=True))
    rrs = (C / 8 + 8) * E32 + dmean ** 2 / (2 * v)
    rm = rs * mean
    drm = rs * dmean + rm.abs() * (rrs + E32)
    acc = x @ W1t.t()
    absacc = x.abs() @ W1t.abs().t()
    qw = quantum(W1t).amin()
    dacc = (C + 2) * E32 * absacc * ~sums_exact(absacc.amax(1, keepdim=True), qx * qw)
    t1, t2 = acc * rs, s1[None, :] * rm
    t = t1 - t2 + b1p[None, :]
    dt = (rs * dacc + t1.abs() * (rrs + E32) + s1.abs()[None, :] * drm + ds1[None, :] * rm.abs() + E32 * t2.abs()
          + E32 * (t1 - t2).abs() + E32 * t.abs() + db1[None, :])
    h, g, dh, dg = t[:, :FH], t[:, FH:], dt[:, :FH], dt[:, FH:]
    gl = _gelu_exact(g)
    p = h * gl
    dp = gl.abs() * dh + (h.abs() + dh) * (1.13 * dg + GELU_ABS_ERR + 2 * E32 * gl.abs()) + 2 * E32 * p.abs()
    lo, hi, Pt = r16(p - dp), r16(p + dp), r16(p)
    res = torch.zeros_like(x) if d.res is None else d.res.to(F64)
    y = Pt @ W2t.t() + d.b2.to(F64)[None, :] + res
    acc_terms = Pt.abs() @ W2t.abs().t() + d.b2.to(F64).abs()[None, :] + res.abs()
    bound = HALF.u * y.abs() + tiny() + 1.01 * ((hi - lo) @ W2t.abs().t() + (FH + 4) * E32 * acc_terms)
    return y, bound


def judge(d, out, what, report=True, ref=None):
    """out (M, C): every element finite and inside the bound; returns the worst err / bound (reported through margin())"""
    y, bound = reference(d) if ref is None else ref
    o = out.to(F64)
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite elements in the rows below M" % (what, int((~torch.isfinite(o)).sum()))
    ratio = (o - y).abs() / bound
    worst = float(ratio.max())
    if d.kinds is not None:
        names, kind = d.kinds
        per = ["%s %.3f" % (n, float(ratio[kind == i].max())) for i, n in enumerate(names) if bool((kind == i).any())]
        print("[ff_fused] %s: worst err/bound per row kind: %s" % (what, ", ".join(per)))
    print("[ff_fused] %-58s worst err/bound %.3f, mean bound / mean |y| %.2e" % (what, worst, float(bound.mean() / y.abs().mean().clamp_min(1e-30))))
    if report:
        return margin("ff_fused " + what, worst, 1.0, unit="err/bound")
    return worst


def rejected(d, out, ref=None):
    """the judge's verdict without an assertion: the worst err / bound (inf for a non-finite element)"""
    y, bound = reference(d) if ref is None else ref
    o = out.to(F64)
    if not bool(torch.isfinite(o).all()):
        return float("inf")
    return float(((o - y).abs() / bound).max())


def gelu_window(d):
    """the GELU window: [round16(gelu(g) - delta), round16(gelu(g) + delta)] per hidden unit, delta = GELU_ABS_ERR + e |gelu(g)|"""
    gl = _gelu_exact(d.b1[FH:].to(F64))
    delta = GELU_ABS_ERR + E32 * gl.abs()
    return r16(gl - delta), r16(gl + delta)


def gelu_least_error(d, out, units):
    """the stored value shows the f32 one only up to its rounding: the least |gelu_erf(g) - gelu(g)| that explains out (M, C), column n
    holding hidden unit units[n], is its distance from gelu(g) less half an ulp of out; returned in units of delta, the worst element.
    (Information next to the window check: 0 where out is the rounded exact value.)"""
    gl = _gelu_exact(d.b1[FH:].to(F64))[units][None, :]
    delta = GELU_ABS_ERR + E32 * gl.abs()
    _, ex = torch.frexp(out)
    half_ulp = torch.ldexp(torch.full_like(out, HALF.u), ex - 1).clamp_min(tiny())
    return float((((out - gl).abs() - half_ulp).clamp_min(0.0) / delta).max())


# ---- the launch ------------------------------------------------------------------------------------------------------------------------
def launch(ctx, d, M=None, res="own", out=None, Cc=C, strm=None):
    """svg_op_ff_fused(_f16) on d (already on the device).  res: 'own' (d.res) | 'x' (the x buffer itself) | None.  Returns the
    (M + PAD, C) output, prefilled with NaN, and the status"""
    M = d.x.shape[0] if M is None else M
    if out is None:
        out = torch.full((M + PAD, d.x.shape[1]), float("nan"), device="cuda", dtype=HALF.dtype)
    rp = {"own": None if d.res is None else d.res.data_ptr(), "x": d.x.data_ptr(), None: None}[res]
    assert d.x.dtype == HALF.dtype and d.x.is_contiguous() and (d.res is None or (d.res.dtype == HALF.dtype and d.res.is_contiguous()))
    rc = getattr(ctx.lib, "svg_op_ff_fused" + HALF.suffix)(ctx.h, d.x.data_ptr(), d.gamma.data_ptr(), d.beta.data_ptr(), d.w1.data_ptr(),
                                                           d.b1.data_ptr(), d.w2.data_ptr(), d.b2.data_ptr(), rp, out.data_ptr(), M, Cc,
                                                           stream() if strm is None else strm)
    return out, rc


def run(ctx, d, **kw):
    """launch, check the status, the NaN rows behind M; returns the M written rows"""
    M = d.x.shape[0]
    out, rc = launch(ctx, d, **kw)
    ctx.check(rc, "ff_fused")
    torch.cuda.synchronize()
    assert bool(out[M:].isnan().all()), "%d elements written in the rows past M = %d" % (int((~out[M:].isnan()).sum()), M)
    return out[:M]


def tag(M):
    return "M%d %s" % (M, "bf16" if HALF.dtype == torch.bfloat16 else "fp16")


# ---- 1: the premise of the judge -------------------------------------------------------------------------------------------------------
@gpu
def test_fold_premise(ctx):
    """W1~ = round16(f32(W1 gamma)) bit for bit, b1' and s1 inside the bounds the judge charges for them, from the library's own fold_ln
    and rowsum on the random class's parameters"""
    d = data_random(1).to("cuda")
    W1t, b1p, db1, s1, ds1, _ = operands(d)
    w = d.w1.clone()
    bout = torch.full((2 * FH,), float("nan"), device="cuda")
    assert ctx.lib.svg_op_fold_ln(ctx.h, w.data_ptr(), d.b1.data_ptr(), d.gamma.data_ptr(), d.beta.data_ptr(), bout.data_ptr(), 2 * FH, C, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(w, d.w1 * d.gamma[None, :]), "fold_ln: W1 gamma is one f32 product"
    assert torch.equal(w.to(HALF.dtype).to(F64), W1t)
    rb = float(((bout.to(F64) - b1p).abs() / db1.clamp_min(1e-300)).max())
    wh = w.to(HALF.dtype)
    so = torch.full((2 * FH,), float("nan"), device="cuda")
    assert getattr(ctx.lib, "svg_op_rowsum" + HALF.suffix)(ctx.h, wh.data_ptr(), so.data_ptr(), 2 * FH, C, stream()) == 0
    torch.cuda.synchronize()
    rsum = float(((so.to(F64) - s1).abs() / ds1.clamp_min(1e-300)).max())      # (a row whose sum is exact: 0 / 0)
    margin("ff_fused premise: fold_ln bias vs fp64 %s" % tag(2 * FH), rb, 1.0, unit="err/bound")
    margin("ff_fused premise: rowsum vs fp64 %s" % tag(2 * FH), rsum, 1.0, unit="err/bound")
    # the grid class: s1 exact
    dg = data_grid(1).to("cuda")
    wg = (dg.w1 * dg.gamma[None, :]).to(HALF.dtype)
    assert getattr(ctx.lib, "svg_op_rowsum" + HALF.suffix)(ctx.h, wg.data_ptr(), so.data_ptr(), 2 * FH, C, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(so.to(F64), wg.to(F64).sum(1)), "grid class: the row sums are exact in f32"


# ---- 2: data classes through the judge -------------------------------------------------------------------------------------------------
CLASSES = {"grid": data_grid, "random": data_random, "offset": data_offset}


@gpu
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_data_class(ctx, cls, M):
    d = CLASSES[cls](M).to("cuda")
    judge(d, run(ctx, d), "%s %s" % (cls, tag(M)))


@gpu
@pytest.mark.parametrize("M", ROWS)
def test_residual_alias_and_null(ctx, M):
    """residual == x (the UNet's own call) equals the distinct-buffer result bit for bit; residual = NULL is judged with res = 0"""
    d = data_random(M, seed=2).to("cuda")
    da = Data(d.x, d.gamma, d.beta, d.w1, d.b1, d.w2, d.b2, d.x.clone())
    distinct = run(ctx, da)
    alias = run(ctx, da, res="x")
    assert torch.equal(alias, distinct), "residual == x: %d elements differ from the distinct-buffer call" % int((alias != distinct).sum())
    judge(da, alias, "residual = x %s" % tag(M))
    dn = Data(d.x, d.gamma, d.beta, d.w1, d.b1, d.w2, d.b2, None)
    judge(dn, run(ctx, dn, res=None), "residual = NULL %s" % tag(M))


# ---- 3: GEMM2, bias pairing, swap and permutations: exact ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [1, 33, 129, 333])
def test_gemm2_exact(ctx, M):
    """every (hidden unit, output column) pair: pack_geglu's h / gate interleave of the bias, the pair's P swap through LDS, pack_ff2_perm,
    the slab row dealing and cperm, the late waves' carried fragments, the epilogue's column map — out EQUALS the fp64 result rounded once"""
    d = data_exact(M).to("cuda")
    want = exact_want(d)
    out = run(ctx, d)
    bad = out != want
    assert not bool(bad.any()), "%d elements differ from the exact result; first at (m, n) = %s: %g vs %g" % (
        int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(out[bad][0]), float(want[bad][0]))
    again = run(ctx, d)
    assert torch.equal(again, out), "a second launch differs in %d elements" % int((again != out).sum())


# ---- 4: GEMM1 pairing, the GELU tails --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("M", [33, 129])
def test_gemm1_pairing(ctx, M, offset):
    """every hidden unit's h through a one-hot W2 (four rounds): a unit reading the wrong W1 row, row sum or statistic is off by O(1).
    offset: on the rows of the offset class, where GEMM1 is exact on the shifted rows (their x are coarse multiples of a power of two) and
    the bound is the statistics' and the fold's alone"""
    worst = 0.0
    for r in range(4):
        d = data_gemm1(M, r, offset).to("cuda")
        worst = max(worst, judge(d, run(ctx, d, res=None), "GEMM1 one-hot round %d %s" % (r, tag(M)), report=False))
    margin("ff_fused GEMM1 one-hot%s %s" % (" offset rows" if offset else "", tag(M)), worst, 1.0, unit="err/bound")


@gpu
def test_gelu_tails(ctx):
    """the fused kernel's GELU unmixed: out in [round16(gelu(g) - delta), round16(gelu(g) + delta)] on a ramp over [-8, 8]"""
    M = 33
    n = torch.arange(C, device="cuda")
    worst = 0.0
    for r in range(4):
        d = data_gelu(M, r).to("cuda")
        out = run(ctx, d, res=None).to(F64)
        worst = max(worst, gelu_least_error(d, out, 4 * n + r))
        lo, hi = gelu_window(d)
        lo, hi = lo[4 * n + r][None, :], hi[4 * n + r][None, :]
        bad = ~((out >= lo) & (out <= hi))
        gv = d.b1[FH:][4 * n + r][None, :].expand(M, -1)
        assert not bool(bad.any()), "round %d: %d elements outside the GELU window; first at g = %.6g: %.8g, window [%.8g, %.8g]" % (
            r, int(bad.sum()), float(gv[bad][0]), float(out[bad][0]), float(lo.expand(M, -1)[bad][0]), float(hi.expand(M, -1)[bad][0]))


    margin("ff_fused GELU ramp, least error consistent with the output / delta %s" % tag(M), worst, 1.0, unit="err/delta")


# ---- 5: invariance, concurrency, refusal -----------------------------------------------------------------------------------------------
@gpu
def test_row_permutation(ctx):
    """the rows of x and the residual permuted: the output rows permute bit for bit (every row changes lane, row tile, pair, early / late
    wave and workgroup)"""
    M = 333
    d = data_random(M, seed=3).to("cuda")
    perm = torch.randperm(M, generator=_gen(8)).to("cuda")
    base = run(ctx, d)
    moved = run(ctx, d.rows(perm))
    assert torch.equal(moved, base[perm]), "%d rows differ after the permutation" % int((moved != base[perm]).any(1).sum())


@gpu
def test_two_contexts_at_once(ctx):
    """two threads, two contexts, two streams, 8 launches each at M = 128 * 600 + 77 (enough workgroups for the two grids to share CUs):
    every output is bit-identical to the single-context result.  A fixed count with one comparison per output."""
    M, N = 128 * 600 + 77, 8
    ds = [data_random(M, seed=10 + t).to("cuda") for t in range(2)]
    want = [run(ctx, d).clone() for d in ds]
    ctxs = [_lib.Context(0) for _ in range(2)]
    outs = [[torch.full((M + PAD, C), float("nan"), device="cuda", dtype=HALF.dtype) for _ in range(N)] for _ in range(2)]
    torch.cuda.synchronize()
    errs = [None, None]

    def work(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for i in range(N):
                    _, rc = launch(ctxs[t], ds[t], out=outs[t][i], strm=s.cuda_stream)
                    ctxs[t].check(rc, "ff_fused")
                s.synchronize()
        except Exception as ex:  # noqa: BLE001  (reported by the main thread)
            errs[t] = ex

    ths = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    try:
        [t.start() for t in ths]
        [t.join(120) for t in ths]
        if any(t.is_alive() for t in ths):
            # a launch that has not come back in two minutes is hung: nothing more may go to that GPU, so the session ends here instead of
            # failing one test and launching the rest of the suite behind a hung stream (the contexts are left as they are)
            pytest.exit("test_two_contexts_at_once: a worker thread's ff_fused launches did not finish within 120 s", returncode=3)
        assert errs == [None, None], "worker errors: %s" % errs
        torch.cuda.synchronize()
        bad = [[i for i in range(N) if not torch.equal(outs[t][i][:M], want[t])] for t in range(2)]
        assert bad == [[], []], "launches that differ from the single-context result, per context: %s" % bad
        assert all(bool(o[M:].isnan().all()) for t in range(2) for o in outs[t])
    finally:
        if not any(t.is_alive() for t in ths):
            [c.close() for c in ctxs]


@gpu
def test_refused_width(ctx):
    """C != 320: an error, and the NaN-filled output stays untouched"""
    M, Cc = 128, 640
    g = _gen(9)
    x = torch.randn(M, Cc, generator=g).to(HALF.dtype).cuda()
    d = Data(x, torch.ones(Cc).cuda(), torch.zeros(Cc).cuda(), torch.zeros(8 * Cc, Cc).cuda(), torch.zeros(8 * Cc).cuda(),
             torch.zeros(Cc, 4 * Cc).cuda(), torch.zeros(Cc).cuda(), x.clone())
    out, rc = launch(ctx, d, Cc=Cc)
    torch.cuda.synchronize()
    assert rc == _lib.SVG_ERR_INVALID, "status %d, expected a refusal" % rc
    assert len(ctx.lib.svg_last_error(ctx.h)) > 0
    assert bool(out.isnan().all()), "the output was written"


# ---- 6: the judge on the CPU -----------------------------------------------------------------------------------------------------------
def gelu_poly32(x):
    """gelu_erf of csrc/igemm_epi.h in f32 (its FMAs as a product and a sum)"""
    a = x.abs().clamp(max=6.0)
    p = torch.full_like(x, 3.4645448e-05)
    for c in (-0.000782622703, 0.00812418268, -0.0534785727, -0.458721816, -1.15121768, -0.999991402):
        p = p * a + c
    return -x.abs() * torch.exp2(p) + x.clamp(min=0.0)


def emulate(d, mut=None):
    """the stages of ff_pair_kernel in f32 torch: two-pass statistics, the fold, gelu_erf's polynomial, the rounding of P, f32 GEMM2, one
    output rounding.  mut: one deliberate defect (test_judge_rejects_cpu)"""
    f32 = torch.float32
    x = d.x.to(f32)
    W1t = (d.w1 * d.gamma[None, :]).to(HALF.dtype).to(f32)
    b1p = (d.b1.to(F64) + d.w1.to(F64) @ d.beta.to(F64)).to(f32)
    if mut == "swap_b1":
        b1p = torch.cat([b1p[FH:], b1p[:FH]])
    s1 = W1t.sum(1)
    W2t = d.w2.to(HALF.dtype).to(f32)
    if mut == "swap_w2_k":
        W2t = W2t.clone()
        W2t[:, [517, 518]] = W2t[:, [518, 517]]
    mean = x.sum(1, keepdim=True) * f32_const(1.0 / C)
    if mut == "one_pass_var":
        var = ((x * x).sum(1, keepdim=True) * f32_const(1.0 / C) - mean * mean).clamp(min=0.0)
    else:
        var = ((x - mean) ** 2).sum(1, keepdim=True) * f32_const(1.0 / C)
    rs = torch.rsqrt(var + f32_const(1e-5))
    rm = rs * mean
    if mut == "neighbour_rs":
        rs = rs.roll(1, 0)
    acc = x @ W1t.t()
    t = acc * rs - s1[None, :] * rm + b1p[None, :]
    h, g = t[:, :FH], t[:, FH:]
    gl = torch.nn.functional.gelu(g, approximate="tanh") if mut == "tanh_gelu" else gelu_poly32(g)
    P = (h * gl).to(HALF.dtype).to(f32)
    if mut == "drop_unit":
        P[:, 777] = 0
    elif mut == "drop_chunk":
        P[:, 64 * 7:64 * 8] = 0
    elif mut == "roll_rows":
        P = P.roll(1, 0)
    y = P @ W2t.t()
    if mut == "swap_halves":
        y = torch.cat([y[:, C // 2:], y[:, :C // 2]], dim=1)
    y = y + d.b2[None, :]
    if d.res is not None:
        y = y + d.res.to(f32)
    out = y.to(HALF.dtype)
    if mut == "col_ulp":
        bits = out[:, 123].contiguous().view(torch.int16) + 1                  # one storage ulp away from zero
        out[:, 123] = bits.view(HALF.dtype)
    return out


def f32_const(v):
    return torch.tensor(v, dtype=torch.float32)


CPU_M = 161
MUT_M = 640


@pytest.mark.parametrize("cls", list(CLASSES))
def test_emulation_cpu(cls):
    """the data classes on the CPU: the emulation passes the judge on every data class (and the grid class's premise holds: GEMM1 and s1 exact)"""
    d = CLASSES[cls](CPU_M)
    if cls == "grid":
        W1t = (d.w1 * d.gamma[None, :]).to(HALF.dtype)
        assert torch.equal((d.x.float() @ W1t.float().t()).double(), d.x.double() @ W1t.double().t())
        assert torch.equal(W1t.float().sum(1).double(), W1t.double().sum(1))
        assert torch.equal(d.x.float().sum(1).double(), d.x.double().sum(1))
        assert float(operands(d)[4].max()) == 0.0, "the judge charges nothing for the grid class's s1"
    assert judge(d, emulate(d), "emulation %s %s" % (cls, tag(CPU_M)), report=False) < 1.0
    dn = Data(d.x, d.gamma, d.beta, d.w1, d.b1, d.w2, d.b2, None)
    assert judge(dn, emulate(dn), "emulation %s, no residual %s" % (cls, tag(CPU_M)), report=False) < 1.0


def test_emulation_exact_and_onehot_cpu():
    """the exact GEMM2 data and the one-hot-W2 data on the CPU"""
    d = data_exact(129)
    assert torch.equal(emulate(d), exact_want(d))
    n = torch.arange(C)
    for r in (0, 3):
        for offset in (False, True):
            d = data_gemm1(CPU_M, r, offset)
            assert judge(d, emulate(d), "emulation GEMM1 one-hot round %d" % r, report=False) < 1.0
        d = data_gelu(33, r)
        lo, hi = gelu_window(d)
        out = emulate(d).to(F64)
        assert bool(((out >= lo[4 * n + r][None, :]) & (out <= hi[4 * n + r][None, :])).all())
        least = gelu_least_error(d, out, 4 * n + r)
        print("[ff_fused] emulation GELU ramp round %d: least error consistent with the output %.3f delta" % (r, least))
        assert least < 1.0 < gelu_least_error(d, emulate(d, "tanh_gelu").to(F64), 4 * n + r)


MUTATIONS = {"drop_unit": "random", "drop_chunk": "random", "roll_rows": "random", "swap_halves": "random", "swap_b1": "random",
             "neighbour_rs": "offset", "one_pass_var": "gemm1-offset", "col_ulp": "grid", "swap_w2_k": "exact", "tanh_gelu": "gelu"}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judge_rejects_cpu(mut):
    """each defect of the emulation is outside the judge (the unmutated emulation is inside: test_emulation_cpu)"""
    cls = MUTATIONS[mut]
    if cls == "exact":
        d = data_exact(129)
        assert torch.equal(emulate(d), exact_want(d)) and not torch.equal(emulate(d, mut), exact_want(d))
        return
    if cls == "gelu":
        n = torch.arange(C)
        d = data_gelu(33, 1)
        lo, hi = gelu_window(d)
        out = emulate(d, mut).to(F64)
        inside = (out >= lo[4 * n + 1][None, :]) & (out <= hi[4 * n + 1][None, :])
        assert not bool(inside.all())
        assert bool((~inside)[:, (d.b1[FH:][4 * n + 1] < -1)].any()), "the negative tail shows the tanh form"
        return
    # one_pass_var: the shifted rows behind the one-hot W2 (512 sigma in bf16, 64 sigma in fp16): behind a dense W2 the bound adds 1280
    # magnitudes while the defect's errors add like a random walk
    # col_ulp and one_pass_var are judged over MUT_M rows, so that the rejection rests on several elements (fp16: five of the column's
    # 640 for col_ulp, whose error is between 0.5 and 1.5 ulp by construction) and not on one
    big = mut in ("col_ulp", "one_pass_var")
    d = data_gemm1(MUT_M, 1, offset=True) if cls == "gemm1-offset" else CLASSES[cls](MUT_M if big else CPU_M)
    y, bound = ref = reference(d)
    assert rejected(d, emulate(d), ref) < 1.0
    ratio = (emulate(d, mut).to(F64) - y).abs() / bound
    factor, n_out = rejected(d, emulate(d, mut), ref), int((~(ratio <= 1)).sum())
    print("[ff_fused] mutation %-14s on %-12s data: %.3g x the bound, %d elements outside" % (mut, cls, factor, n_out))
    assert factor > 1.0, "the judge accepts the mutation %s (%.3f of the bound)" % (mut, factor)
    assert not big or n_out >= 4, "the rejection of %s rests on %d elements" % (mut, n_out)
