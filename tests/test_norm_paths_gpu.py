"""GroupNorm, LayerNorm, row softmax and their helper kernels (csrc/norm.hip) on every kernel path, against fp64 references.

svg_op_groupnorm_ex runs one GroupNorm descriptor (two sources, f32 input, caller-supplied producer column sums) on a forced path and
reports what ran, {kind, maxch, vw, CV, PL, nchunk, nblk, threads}; every case asserts that report against describe_py(), a plain
Python statement of the dispatch rule and launch geometry.  Paths: small<5,8> small<10,8> small<5,4> small<20,4> (one launch per
(sample, group)), stats+apply, finish+apply (statistics from column sums) and finish+apply_mx (MX fp8 output, 16-bit input only).

Reference: fp64 from the kernel's own inputs.  Every comparison is per element against gn_ref_bound(), derived from the arithmetic
of the path and holding no fitted constant.  With e = 2^-24 (f32 unit roundoff), u the 16-bit unit roundoff (2^-8 bf16, 2^-11 fp16),
n = HW * cpg values per group, A = mean|x|, m2 = mean x^2 and L the longest run of sequential f32 additions a term passes through:
    |mean^ - mean| <= (L + 1) e A =: dm                          (L additions, the division)
    |var^ - var|   <= e ((L + 2) m2 + 2 (L + 1) |mean| A + mean^2 + var) + dm^2 =: dv
                      (squares + L additions + division; the square of mean^; the subtraction) — with m2 = var + mean^2 this is
                      the cancellation factor (1 + mean^2 / var) of the one-pass form E[x^2] - mean^2
    rstd^ in [rsqrt(v + dv') (1 - 4e), rsqrt(max(v - dv', eps (1 - 2e))) (1 + 4e)],  v = var + eps, dv' = dv + e v
                      (the sum var + eps; rsqrtf at 2 ulp; the clamp var^ >= 0 keeps rstd^ <= rsqrt(eps)); dr = the larger distance to rstd
    out before rounding: a = fl(rstd^ gamma), sh = fl(beta - mean^ a), f = fma(x, a, sh):
        E = 1.01 (|x - mean| |gamma| (dr + e (rstd + dr)) + dm (rstd + dr) |gamma| + 2 e |mean| (rstd + dr) |gamma| + e |beta| + e |y|)
    SiLU f * rcp(1 + __expf(-f)): |silu'| <= 1.1; __expf is v_exp_f32 (1 ulp) of a rounded product, (2 + 2|f|) ulp allowed; the sum, rcpf
        (1 ulp) and the product add 4e:   E_s = 1.1 E + 1.01 e (8 + 4 |y|) |silu(y)|
    stored value: bound = E (1 + u) + u |y| + tiny   (tiny: 2^-25 for fp16 subnormals, 2^-134 for bf16)
L per path: small<M,V>: M V + 8 (per-thread run, six shuffle levels, two LDS levels); stats+apply: pixels per thread + PL cpg (group
reduction) + nchunk; finish paths: ceil(tps1 n1 / 256) + ceil(tps2 n2 / 256) + 8, + 1 for the f32 rounding of the supplied sums.
For integer-exact data (small integers: every partial sum exact in any order) L = 0 is used: s / n, q / n - mean^2, rsqrtf and the fma
are then the only roundings.  test_gn_bounds_hold_for_emulated_paths_cpu replays the summation order of each path in numpy f32 on every
random / offset input of this file (RANDOM_CASES, OFFSET_CASES, the single-ratio cases and the random inputs of the MX test) and checks the replay against the
same bound, without a GPU; it also checks that the bound is not
vacuous: for groups with |mean| <= sigma it stays below 2 u (|gamma| max(|x - mean| rstd, 1) + |beta|) + tiny, i.e. within two output roundings
of the pre-activation magnitude of an element at least one sigma from the mean (largest over all cases: 1.05 u bf16, 1.34 u fp16 — stats+apply on one group of 8 channels, L = 2052).

One-hot probes: x = 0 except one 2^k per (sample, group), every (sample, group) at another position; a missed element gives
x rsqrt(eps), a doubled one about 1 / sqrt(2) of the right value — both far outside the bound, which is a few f32 ulps here since a
one-term sum is exact.  Positions: first / last pixel, every residue modulo PL and 4 PL, both sides of each chunk and block seam, first
/ last channel of a group (a group boundary inside an 8-channel vector when cpg % 8 != 0), both sides of the C1 seam, every register
slot of the small kernels (at UNet shapes that fill their registers exactly); at small shapes B = n samples probe every position of
every group in one launch.
Inputs sit in separately allocated NaN-guarded buffers (a stray read poisons a group), outputs are prefilled with NaN inside NaN
guards (an element not written, or written outside, shows).  Every GPU test runs in bf16 and fp16 storage."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from sd_video_gen_amd import _lib

gpu = pytest.mark.gpu
E32 = 2.0 ** -24
SMALL, STATS, FINISH, MX = 0, 1, 2, 3
SMALL_PATHS = [(SMALL, 5, 8), (SMALL, 10, 8), (SMALL, 5, 4), (SMALL, 20, 4)]
TWO_STAGE = [(STATS, 0, 0), (FINISH, 0, 0)]
PATHS = SMALL_PATHS + TWO_STAGE
G = 64                               # guard elements on each side of every buffer


def path_id(p):
    return {SMALL: "small<%d,%d>" % (p[1], p[2]), STATS: "stats+apply", FINISH: "finish+apply", MX: "finish+apply_mx"}[p[0]]


class _Half:
    dtype, suffix, u, tiny, name = torch.bfloat16, "", 2.0 ** -8, 2.0 ** -134, "bf16"


HALF = _Half()
STORAGE = {"bf16": (torch.bfloat16, "", 2.0 ** -8, 2.0 ** -134), "fp16": (torch.float16, "_f16", 2.0 ** -11, 2.0 ** -25)}


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def _storage(request):
    HALF.dtype, HALF.suffix, HALF.u, HALF.tiny = STORAGE[request.param]
    HALF.name = request.param
    yield request.param
    HALF.dtype, HALF.suffix, HALF.u, HALF.tiny = STORAGE["bf16"]
    HALF.name = "bf16"


def stream():
    return torch.cuda.current_stream().cuda_stream


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the dispatch rule and launch geometry, stated plainly (groupnorm_describe must agree) ------------------------------------------
def small_fits(C1, C2, HW, groups, maxch, vw):
    cpg = (C1 + C2) // groups
    return cpg % vw == 0 and C1 % vw == 0 and HW * (cpg // vw) <= 256 * maxch


def describe_py(C1, C2, B, HW, groups, have_stats=False, force=None, mx=False):
    Cc = C1 + C2
    cpg = Cc // groups
    if mx:
        CV = cdiv(Cc, 128) * 128 // 8
        kind = MX
    elif force is not None:
        kind = force[0]
        if kind == SMALL:
            assert small_fits(C1, C2, HW, groups, force[1], force[2])
            return (SMALL, force[1], force[2], 0, 0, 0, 0, 256)
        CV = Cc // 8
    elif HW <= 256 and small_fits(C1, C2, HW, groups, 20, 4):
        if cpg % 8 == 0:
            return (SMALL, 5 if small_fits(C1, C2, HW, groups, 5, 8) else 10, 8, 0, 0, 0, 0, 256)
        return (SMALL, 5 if small_fits(C1, C2, HW, groups, 5, 4) else 20, 4, 0, 0, 0, 0, 256)
    else:
        kind, CV = (FINISH if have_stats else STATS), Cc // 8
    PL = max(1, 256 // CV)
    threads = max(cdiv(CV * PL, 64) * 64, 64)
    nblk = max(1, min(HW // PL, max(HW // (PL * 16), cdiv(2048, B))))
    nchunk = 0
    if kind == STATS:
        nchunk = max(1, min(64, HW // (PL * 8)))
        while nchunk * 2 <= 64 and nchunk * B < 512 and HW // (nchunk * 2) >= PL * 2:
            nchunk *= 2
    return (kind, 0, 0, CV, PL, nchunk, nblk, threads)


def chain_len(desc, C1, C2, HW, groups, tps=(0, 0)):
    """L: the longest run of sequential f32 additions of the path (module docstring)"""
    kind, maxch, vw, CV, PL, nchunk = desc[:6]
    cpg = (C1 + C2) // groups
    if kind == SMALL:
        return maxch * vw + 8
    if kind == STATS:
        return cdiv(cdiv(HW, nchunk), PL) + PL * cpg + nchunk
    return cdiv(tps[0] * min(cpg, C1), 256) + cdiv(tps[1] * min(cpg, C2), 256) + 8 + 1


# ---- fp64 reference and the derived bound ---------------------------------------------------------------------------------------
def stats_ref_bound(x, groups, eps, L):
    """x (B,HW,C) f64 -> mean, rstd, dm, dr, each (B,1,groups,1)"""
    B, HW, Cc = x.shape
    xg = x.reshape(B, HW, groups, Cc // groups)
    mean = xg.mean((1, 3), keepdim=True)
    A = xg.abs().mean((1, 3), keepdim=True)
    m2 = (xg * xg).mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    dm = (L + 1) * E32 * A
    dv = E32 * ((L + 2) * m2 + 2 * (L + 1) * mean.abs() * A + mean * mean + var) + dm * dm
    v = var + eps
    dv = dv + E32 * v
    r = v.rsqrt()
    rlo = (v + dv).rsqrt() * (1 - 4 * E32)
    rhi = torch.clamp(v - dv, min=eps * (1 - 2 * E32)).rsqrt() * (1 + 4 * E32)
    return mean, r, dm, torch.maximum(r - rlo, rhi - r)


def gn_ref_bound(x, gamma, beta, groups, eps, silu, L):
    """x (B,HW,C), gamma, beta (C) f64 -> (reference, bound on |stored - reference|, pre-activation magnitude |gamma| max(|x - mean| rstd, 1)
    + |beta|), each (B,HW,C) f64"""
    B, HW, Cc = x.shape
    cpg = Cc // groups
    xg = x.reshape(B, HW, groups, cpg)
    mean, r, dm, dr = stats_ref_bound(x, groups, eps, L)
    g, bt = gamma.reshape(1, 1, groups, cpg), beta.reshape(1, 1, groups, cpg)
    y = (xg - mean) * r * g + bt
    E = 1.01 * ((xg - mean).abs() * g.abs() * (dr + E32 * (r + dr)) + dm * (r + dr) * g.abs() + 2 * E32 * mean.abs() * (r + dr) * g.abs()
                + E32 * bt.abs() + E32 * y.abs())
    mag = g.abs() * torch.clamp((xg - mean).abs() * r, min=1.0) + bt.abs()      # a one-sigma element of the channel at least
    if silu:
        ys = y * torch.sigmoid(y)
        E = 1.1 * E + 1.01 * E32 * (8 + 4 * y.abs()) * ys.abs()
        y = ys
    bound = E * (1 + HALF.u) + HALF.u * y.abs() + HALF.tiny
    return y.reshape(B, HW, Cc), bound.reshape(B, HW, Cc), mag.reshape(B, HW, Cc)


def check(out, ref, bound, what, mag=None):
    """mag: the pre-activation magnitude of gn_ref_bound; the largest error is then also printed in units of u * mag"""
    err = (out.double() - ref).abs()
    ratio = float((err / bound).max())
    in_u = "" if mag is None else "  = %.2f u of the magnitude" % float((err / (HALF.u * mag)).max())
    print("[norm] %-70s max err/bound %.3f  max err %.3e%s" % (what, ratio, float(err.max()), in_u))
    bad = ~(err <= bound)
    assert not bool(bad.any()), "%s: %d elements outside the bound, worst err/bound %.3g at %s" % (
        what, int(bad.sum()), ratio, tuple(int(i) for i in torch.nonzero(bad)[0]))
    return ratio


# ---- buffers ----------------------------------------------------------------------------------------------------------------------
def guarded(t, device="cuda"):
    """a copy of t inside its own NaN-filled allocation (0xA5 for bytes): (whole buffer, view of the payload)"""
    n = t.numel()
    fill = 0xA5 if t.dtype == torch.uint8 else float("nan")
    buf = torch.full((n + 2 * G,), fill, dtype=t.dtype, device=device)
    buf[G:G + n] = t.reshape(-1).to(device)
    return buf, buf[G:G + n].view(t.shape)


def guards_intact(buf, what):
    for part in (buf[:G], buf[-G:]):
        ok = (part == 0xA5).all() if buf.dtype == torch.uint8 else torch.isnan(part).all()
        assert bool(ok), what + ": a guard region was written"


def nan_out(shape, dtype):
    return guarded(torch.full(shape, float("nan"), dtype=dtype))


def make_parts(x, tps):
    """producer column sums of x (B,HW,Cs) f64 over tps uneven row tiles: (B * tps, Cs, 2) f32 (the GnStats layout)"""
    B, HW, Cs = x.shape
    cuts = [round(i * HW / tps) for i in range(tps + 1)]
    p = torch.zeros(B, tps, Cs, 2, dtype=torch.float64, device=x.device)
    for t in range(tps):
        seg = x[:, cuts[t]:cuts[t + 1]]
        p[:, t, :, 0] = seg.sum(1)
        p[:, t, :, 1] = (seg * seg).sum(1)
    return p.float().reshape(B * tps, Cs, 2)


class Case:
    """one GroupNorm problem: sources x1 (B,HW,C1), x2 (B,HW,C2) or None in their input type, f32 gamma / beta"""

    def __init__(self, x1, x2, gamma, beta, groups, eps=1e-5, tps=(3, 5)):
        self.x1, self.x2, self.gamma, self.beta, self.groups, self.eps, self.tps = x1, x2, gamma, beta, groups, eps, tps
        self.B, self.HW, self.C1 = x1.shape
        self.C2 = 0 if x2 is None else x2.shape[2]
        self.f32 = x1.dtype == torch.float32
        self.x64 = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], 2)

    def parts(self):
        p1 = make_parts(self.x1.double(), self.tps[0])
        p2 = make_parts(self.x2.double(), self.tps[1]) if self.x2 is not None else None
        return p1, p2

    def ref(self, silu, desc, exact=False):
        L = 0 if exact else chain_len(desc, self.C1, self.C2, self.HW, self.groups, self.tps)
        return gn_ref_bound(self.x64, self.gamma.double(), self.beta.double(), self.groups, self.eps, silu, L)

    def valid(self, path):
        if path[0] == SMALL:
            return small_fits(self.C1, self.C2, self.HW, self.groups, path[1], path[2])
        return True


def run_gn(ctx, case, silu, force=None, with_parts=False, mx=False):
    """svg_op_groupnorm_ex / svg_op_groupnorm_mx on guarded buffers -> (status, out or (q, sc, stats, fused), reported path)"""
    d = _lib.GnDesc()
    keep = [guarded(case.x1)]
    d.x, d.C1, d.f32_in = keep[0][1].data_ptr(), case.C1, int(case.f32)
    if case.x2 is not None:
        keep.append(guarded(case.x2))
        d.x2, d.C2 = keep[-1][1].data_ptr(), case.C2
    gb, bb = guarded(case.gamma), guarded(case.beta)
    d.gamma, d.beta = gb[1].data_ptr(), bb[1].data_ptr()
    d.B, d.HW, d.groups, d.eps, d.silu = case.B, case.HW, case.groups, case.eps, silu
    if with_parts:
        p1, p2 = case.parts()
        keep.append(guarded(p1))
        d.part1, d.tps1 = keep[-1][1].data_ptr(), case.tps[0]
        if p2 is not None:
            keep.append(guarded(p2))
            d.part2, d.tps2 = keep[-1][1].data_ptr(), case.tps[1]
    if force is not None:
        d.force, d.kind, d.maxch, d.vw = 1, force[0], force[1], force[2]
    path = (C.c_int * 8)(*([-9] * 8))
    Cc = case.C1 + case.C2
    if mx:
        Cp = cdiv(Cc, 128) * 128
        qb, q = guarded(torch.full((case.B * case.HW, Cp), 0xA5, dtype=torch.uint8))
        sb, sc = guarded(torch.full((case.B * case.HW, Cp // 32), 0xA5, dtype=torch.uint8))
        tb, st = nan_out((case.B, case.groups, 2), torch.float32)
        d.q, d.sc, d.stats = q.data_ptr(), sc.data_ptr(), st.data_ptr()
        fused = C.c_int(-1)
        rc = getattr(ctx.lib, "svg_op_groupnorm_mx" + HALF.suffix)(ctx.h, C.byref(d), C.byref(fused), path, stream())
        torch.cuda.synchronize()
        for b in (qb, sb, tb):
            guards_intact(b, "groupnorm_mx")
        return rc, (q, sc, st, fused.value), tuple(path)
    ob, out = nan_out((case.B, case.HW, Cc), HALF.dtype)
    d.out = out.data_ptr()
    rc = getattr(ctx.lib, "svg_op_groupnorm_ex" + HALF.suffix)(ctx.h, C.byref(d), path, stream())
    torch.cuda.synchronize()
    guards_intact(ob, "groupnorm_ex")
    if rc == 0:
        assert bool(torch.isfinite(out).all()), "groupnorm_ex: %d output elements not written or not finite" % int((~torch.isfinite(out)).sum())
    return rc, out, tuple(path)


def run_checked(ctx, case, silu, path, what, exact=False):
    """run `path` (a finish path gets the column sums), assert the reported path and geometry, compare with fp64 at the bound"""
    want = describe_py(case.C1, case.C2, case.B, case.HW, case.groups, have_stats=path[0] == FINISH, force=path)
    rc, out, ran = run_gn(ctx, case, silu, force=path, with_parts=path[0] == FINISH)
    assert rc == 0, ctx.lib.svg_last_error(ctx.h).decode()
    assert ran == want, "%s: ran %s, expected %s" % (what, ran, want)
    ref, bound, mag = case.ref(silu, want, exact)
    check(out, ref, bound, "%s %s silu%d %s" % (what, path_id(path), silu, HALF.name), mag if silu == 0 else None)
    return out


def in_dtype(f32):
    return torch.float32 if f32 else HALF.dtype


def affine(Cc, seed, dev="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    gamma = (1.0 + 0.5 * torch.randn(Cc, generator=g)).float()
    beta = (0.5 * torch.randn(Cc, generator=g)).float()
    return gamma.to(dev), beta.to(dev)


def split(x, C1, dt):
    """(B,HW,C) f32 values -> the two sources in the input type"""
    x = x.to(dt)
    if C1 == x.shape[2]:
        return x.contiguous(), None
    return x[:, :, :C1].contiguous(), x[:, :, C1:].contiguous()


# shapes where every forced path of a family is valid: (C1, C2, HW, groups)
EXHAUSTIVE = {8: [(64, 0, 40, 4), (24, 40, 40, 4)],        # cpg 16: 8-channel pieces; group 1 = channels 16..31 straddles C1 = 24
              4: [(48, 0, 40, 4), (16, 32, 40, 4)],        # cpg 12: 4-channel pieces; group 1 = channels 12..23 straddles C1 = 16
              0: [(96, 0, 20, 8), (40, 56, 20, 8)]}        # cpg 12: group boundaries inside 8-channel vectors; group 3 straddles C1 = 40


def shapes_for(path, which):
    return [EXHAUSTIVE[path[2] if path[0] == SMALL else 0][which]]


# ---- a. one-hot probes ------------------------------------------------------------------------------------------------------------
def onehot_input(B, HW, Cc, groups, positions):
    """zero except x[b, p, g * cpg + cc] = 2^k for positions[(b, g)] = (p, cc)"""
    cpg = Cc // groups
    x = torch.zeros(B, HW, Cc)
    for (b, g), (p, cc) in positions.items():
        x[b, p, g * cpg + cc] = 2.0 ** ((b + 2 * g) % 5 - 2)
    return x


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["in16", "in32"])
@pytest.mark.parametrize("two", [False, True], ids=["one-source", "two-source"])
@pytest.mark.parametrize("path", PATHS, ids=path_id)
def test_gn_onehot_every_position(ctx, path, two, f32):
    """B = HW * cpg samples: sample b puts the hot element of group g at position (b + 7 g) mod n, so every position of every group is
    probed once in one launch — every pixel lane, every channel of a vector, the group boundaries inside a vector, both sides of the C1
    seam, every thread's piece and the last id of the small kernels.  These shapes hold 80 or 120 pieces per group, so of the small
    kernels' register slots only i = 0 is live here: the other slots are probed by test_gn_onehot_small_full_registers."""
    C1, C2, HW, groups = shapes_for(path, int(two))[0]
    Cc = C1 + C2
    cpg = Cc // groups
    n = HW * cpg
    pos = {(b, g): divmod((b + 7 * g) % n, cpg) for b in range(n) for g in range(groups)}
    x1, x2 = split(onehot_input(n, HW, Cc, groups, pos), C1, in_dtype(f32))
    gamma, beta = affine(Cc, 1)
    case = Case(x1.cuda(), None if x2 is None else x2.cuda(), gamma, beta, groups, tps=(3, 5))
    for silu in (0, 1):
        run_checked(ctx, case, silu, path, "one-hot all positions", exact=True)


# per small kernel a UNet shape whose groups fill its registers exactly, HW * cpg / vw = 256 * maxch pieces: (C1, C2, HW, groups)
FULL_SMALL = {(SMALL, 5, 8): (1280, 0, 256, 32),          # cpg 40: 256 x 5 pieces of 8
              (SMALL, 10, 8): (1280, 1280, 256, 32),      # cpg 80: the 1280+1280 concat at 16 x 16, 256 x 10 pieces of 8
              (SMALL, 5, 4): (1280, 1280, 64, 32),        # the same concat at 8 x 8 in 4-channel pieces: 64 x 20
              (SMALL, 20, 4): (1280, 1280, 256, 32)}      # 256 x 20 pieces of 4: the register budget of the dispatch rule


@gpu
@pytest.mark.parametrize("data", ["onehot", "integer"])
@pytest.mark.parametrize("path", SMALL_PATHS, ids=path_id)
def test_gn_onehot_small_full_registers(ctx, path, data):
    """every register slot i < MAXCH of each small kernel and its last valid id = 256 MAXCH - 1: in slot i the pieces of threads 0, 255
    and (37 i + 11) mod 256, the hot channel moving through the piece; asserted below that the probes name every slot.  The same
    shapes with integer-exact data."""
    C1, C2, HW, groups = FULL_SMALL[path]
    Cc, maxch, vw = C1 + C2, path[1], path[2]
    cpg = Cc // groups
    nch = cpg // vw
    tot = HW * nch
    assert tot == 256 * maxch
    ids = sorted(set([tot - 1] + [256 * i + t for i in range(maxch) for t in (0, 255, (37 * i + 11) % 256)]))
    assert {i // 256 for i in ids} == set(range(maxch)) and ids[-1] == tot - 1
    pairs = [(i // nch, (i % nch) * vw + k % vw) for k, i in enumerate(ids)]
    B = max(2, cdiv(len(pairs), groups))
    if data == "onehot":
        pos = {(b, g): pairs[(b * groups + g) % len(pairs)] for b in range(B) for g in range(groups)}
        assert set(pos.values()) == set(pairs)
        xv = onehot_input(B, HW, Cc, groups, pos)
    else:
        xv = integer_input(B, HW, Cc, 31)
    for f32 in (False, True):
        x1, x2 = split(xv, C1, in_dtype(f32))
        gamma, beta = affine(Cc, 7)
        case = Case(x1.cuda(), None if x2 is None else x2.cuda(), gamma, beta, groups)
        for silu in (0, 1):
            run_checked(ctx, case, silu, path, "full registers %s %s" % (data, "f32" if f32 else "16"), exact=True)


def probe_pixels(desc, HW):
    kind, _, _, CV, PL, nchunk, nblk, _ = desc
    px = {0, HW - 1}
    px.update(range(min(HW, 5 * PL + 1)))
    px.update(range(max(0, HW - 5 * PL - 1), HW))
    for parts in (nchunk, nblk):
        if parts > 1:
            per = cdiv(HW, parts)
            ks = sorted(set(list(range(1, min(parts, 4))) + [parts // 2, parts - 1]))
            for k in ks:
                for p in (k * per - 1, k * per):
                    if 0 <= p < HW:
                        px.add(p)
    return sorted(px)


# the UNet's skip concats whose groups straddle the seam or split 8-channel vectors, and a VAE width: (C1, C2, HW, groups, f32)
PROBE_SHAPES = [(640, 320, 1024, 32, False), (1280, 640, 256, 32, False), (1280, 640, 64, 32, False), (320, 320, 4096, 32, False),
                (1280, 1280, 256, 32, False), (1280, 0, 64, 32, False), (128, 0, 2304, 32, True), (320, 0, 300, 32, False)]


@gpu
@pytest.mark.parametrize("shape", PROBE_SHAPES, ids=lambda s: "%d+%d-hw%d-g%d%s" % (s[0], s[1], s[2], s[3], "-f32" if s[4] else ""))
def test_gn_onehot_real_geometry(ctx, shape):
    """one-hot probes at the UNet's / VAE's channel counts on every path valid there: pixels 0 .. 5 PL and the last 5 PL + 1 (every
    residue modulo PL and 4 PL, the unrolled loop's tail), both sides of the first, middle and last chunk and block seams, the first and
    last channel of every group (cpg = 30: inside 8-channel vectors) and channels C1 - 1, C1 (cpg = 60: inside group 21).  The small
    kernels valid at a shape get probes in the register slots that shape fills (all of them only in
    test_gn_onehot_small_full_registers)."""
    C1, C2, HW, groups, f32 = shape
    Cc = C1 + C2
    cpg = Cc // groups
    for path in PATHS:
        if path[0] == SMALL and not small_fits(C1, C2, HW, groups, path[1], path[2]):
            continue
        geo = describe_py(C1, C2, 8, HW, groups, have_stats=path[0] == FINISH, force=path)
        if path[0] == SMALL:
            nch, tot = cpg // path[2], HW * (cpg // path[2])
            ids = sorted(set([0, min(255, tot - 1), tot - 1] + [256 * i + (37 * i + 11) % 256 for i in range(path[1]) if 256 * i + 255 < tot]))
            pairs = [(i // nch, (i % nch) * path[2] + k % path[2]) for k, i in enumerate(ids)]
            pairs = [(p, cc) for p, cc in pairs if p < HW]
        else:
            pairs = [(p, (0, cpg - 1)[k % 2]) for k, p in enumerate(probe_pixels(geo, HW))]
            pairs += [(HW // 2, cc) for cc in range(cpg)]
        B = min(8, max(2, cdiv(len(pairs), groups)))
        geo = describe_py(C1, C2, B, HW, groups, have_stats=path[0] == FINISH, force=path)
        pos = {(b, g): pairs[(b * groups + g) % len(pairs)] for b in range(B) for g in range(groups)}
        if C2:
            pos[(0, (C1 - 1) // cpg)] = (HW - 1, (C1 - 1) % cpg)      # both sides of the C1 seam
            pos[(1, C1 // cpg)] = (0, C1 % cpg)
        x1, x2 = split(onehot_input(B, HW, Cc, groups, pos), C1, in_dtype(f32))
        gamma, beta = affine(Cc, 2)
        case = Case(x1.cuda(), None if x2 is None else x2.cuda(), gamma, beta, groups, tps=(2, 7))
        for silu in (0, 1):
            run_checked(ctx, case, silu, path, "one-hot %s" % (shape,), exact=True)


# ---- b. integer-exact statistics ----------------------------------------------------------------------------------------------------
def integer_input(B, HW, Cc, seed):
    """integers in [-4, 4] plus a per-channel offset in [-3, 3]: |x| <= 7, x^2 <= 49, so sums stay exact in f32 (< 2^24) in any order
    while n = HW * cpg <= 342 000; exact in bf16 (8 bits) and fp16 too"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, HW, Cc), generator=g).float()
    return x + (torch.arange(Cc) % 7 - 3).float()


INT_SHAPES = [(24, 40, 40, 4, False), (16, 32, 40, 4, False), (640, 320, 1024, 32, False), (1280, 640, 64, 32, False), (1280, 1280, 256, 32, False),
              (256, 0, 1000, 32, True), (320, 0, 77, 32, False), (16, 32, 40, 4, True)]


@gpu
@pytest.mark.parametrize("shape", INT_SHAPES, ids=str)
def test_gn_integer_exact(ctx, shape):
    """exact sums on every valid path: the error left is s / n, q / n - mean^2, rsqrtf, the fma and the output rounding (L = 0)"""
    C1, C2, HW, groups, f32 = shape
    x1, x2 = split(integer_input(3, HW, C1 + C2, HW), C1, in_dtype(f32))
    gamma, beta = affine(C1 + C2, 3)
    case = Case(x1.cuda(), None if x2 is None else x2.cuda(), gamma, beta, groups, tps=(4, 3))
    ran = 0
    for path in PATHS:
        if case.valid(path):
            for silu in (0, 1):
                run_checked(ctx, case, silu, path, "integer %s" % (shape,), exact=True)
            ran += 1
    assert ran >= 2


# ---- c. / d. random, offset and degenerate data -------------------------------------------------------------------------------------
def random_input(B, HW, Cc, groups, seed, ratios=None):
    """N(0,1) * per-channel scale + per-channel offset; ratios: |mean| / sigma per group, cycled (None: offsets ~ N(0, 0.5));
    ratio "const": the group is constant"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, Cc, generator=g) * (0.5 + torch.rand(Cc, generator=g))
    if ratios is None:
        return x + 0.5 * torch.randn(Cc, generator=g)
    cpg = Cc // groups
    xg = x.reshape(B, HW, groups, cpg)
    for gi in range(groups):
        r = ratios[gi % len(ratios)]
        if r == "const":
            xg[:, :, gi, :] = 1.5 + gi
        else:
            sg = xg[:, :, gi, :].std()
            xg[:, :, gi, :] += float(r) * float(sg) * (-1.0 if gi % 2 else 1.0)
    return xg.reshape(B, HW, Cc)


# (C1, C2, B, HW, groups, f32): the UNet's and VAE's channel combinations, then the edges
RANDOM_CASES = [
    (640, 320, 2, 1024, 32, False), (1280, 640, 2, 256, 32, False), (1280, 640, 2, 64, 32, False), (1280, 1280, 2, 64, 32, False),
    (320, 320, 1, 4096, 32, False), (320, 0, 2, 4096, 32, False), (1280, 0, 2, 256, 32, False),
    (128, 0, 1, 2304, 32, True), (256, 0, 1, 1024, 32, True), (512, 0, 2, 576, 32, True),
    (64, 0, 2, 5, 8, False),            # HW < PL (PL = 32)
    (320, 0, 1, 301, 32, False),        # HW not divisible by PL, nchunk, nblk
    (96, 0, 3, 1, 8, False),            # HW = 1
    (64, 0, 67, 33, 4, False),          # large B
    (32, 32, 2, 50, 64, False),         # cpg 1, groups 64
    (64, 0, 2, 130, 32, False),         # cpg 2
    (128, 0, 2, 200, 32, False),        # cpg 4
    (1920, 640, 1, 20, 32, False),      # cpg 80 (two sources)
    (2560, 0, 1, 64, 32, False),        # cpg 80, 256 x 80 / 8 = the small kernels' upper edge at HW = 256 is (1280, 1280, 256)
    (8, 0, 2, 700, 1, False),           # the smallest C: one group of 8
    (8192, 0, 1, 9, 64, False),         # the largest C (CV = 1024), 64 KB of LDS in the statistics pass
    (64, 64, 1, 3000, 4, True),         # groups = 4: the longest group reduction (PL * cpg = 512), f32 two-source
]
# |mean| / sigma of 0, 1, 8, 64 (and 256: far past the contract's one-ulp point), a constant group among varying ones, and a whole
# constant sample
OFFSET_CASES = [(320, 320, 2, 1024, 32, False, (256,)), (128, 0, 1, 2304, 32, True, (256, 0)),
                (320, 320, 2, 1024, 32, False, (0, 1, 8, 64, "const")), (1280, 640, 2, 64, 32, False, (0, 1, 8, 64, "const")),
                (128, 0, 1, 2304, 32, True, (64, 8, "const", 1)), (64, 0, 2, 40, 4, False, ("const",)), (640, 320, 1, 256, 32, False, (64,))]


def build_case(c, dev="cuda"):
    C1, C2, B, HW, groups, f32 = c[:6]
    ratios = c[6] if len(c) > 6 else None
    dt = in_dtype(f32)
    x1, x2 = split(random_input(B, HW, C1 + C2, groups, HW + C1, ratios), C1, dt)
    gamma, beta = affine(C1 + C2, C1, dev)
    return Case(x1.to(dev), None if x2 is None else x2.to(dev), gamma, beta, groups, tps=(3, 5))


def case_id(c):
    off = "" if len(c) <= 6 or c[6] is None else "-offset" + ("_".join(str(r) for r in c[6]) if len(c[6]) < 3 else "")
    return "%d+%d-b%d-hw%d-g%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "-f32" if c[5] else "", off)


@gpu
@pytest.mark.parametrize("c", RANDOM_CASES + OFFSET_CASES, ids=case_id)
def test_gn_random_and_offset(ctx, c):
    """every path valid for the shape against fp64 at the derived bound; the library's own choice (no force) must be the path
    describe_py names; where several paths are valid they agree within the sum of their bounds"""
    case = build_case(c)
    rc, out0, ran = run_gn(ctx, case, 1)
    assert rc == 0, ctx.lib.svg_last_error(ctx.h).decode()
    assert ran == describe_py(case.C1, case.C2, case.B, case.HW, case.groups), "default dispatch"
    rc, _, ran = run_gn(ctx, case, 1, with_parts=True)
    assert rc == 0 and ran == describe_py(case.C1, case.C2, case.B, case.HW, case.groups, have_stats=True), "default dispatch with column sums"
    outs = []
    for path in PATHS:
        if not case.valid(path):
            continue
        for silu in (0, 1):
            out = run_checked(ctx, case, silu, path, case_id(c))
            if silu:
                outs.append((out, case.ref(1, describe_py(case.C1, case.C2, case.B, case.HW, case.groups, path[0] == FINISH, path))[1]))
    for o, b in outs[1:]:
        assert bool(((o.double() - outs[0][0].double()).abs() <= b + outs[0][1]).all()), "paths disagree beyond the sum of their bounds"


RATIOS = [0, 1, 8, 64, 256, "const"]
RATIO_SHAPES = [(320, 320, 2, 1024, 32, False), (1280, 640, 2, 64, 32, False), (128, 0, 1, 2304, 32, True)]


@gpu
@pytest.mark.parametrize("ratio", RATIOS, ids=str)
def test_gn_error_against_fp64_by_offset(ctx, ratio):
    """every group at one |mean| / sigma (or constant), every path valid at a UNet concat, the 8 x 8 level and an f32 VAE width, without
    SiLU: inside the bound, and the printed "u of the magnitude" figures are the ones DESIGN.md's numerics entry quotes"""
    for shape in RATIO_SHAPES:
        case = build_case(shape + ((ratio,),))
        for path in PATHS:
            if case.valid(path):
                run_checked(ctx, case, 0, path, "|mean|/sigma %s %s" % (ratio, case_id(shape)))


@gpu
@pytest.mark.parametrize("path", PATHS, ids=path_id)
def test_gn_batch_permutation_is_bit_exact(ctx, path):
    C1, C2, HW, groups = shapes_for(path, 1)[0]
    case = build_case((C1, C2, 9, HW, groups, False))
    out = run_checked(ctx, case, 1, path, "permutation")
    perm = torch.randperm(9, generator=torch.Generator().manual_seed(5)).cuda()
    pc = Case(case.x1[perm].contiguous(), case.x2[perm].contiguous(), case.gamma, case.beta, groups, tps=case.tps)
    out_p = run_checked(ctx, pc, 1, path, "permuted")
    assert torch.equal(out_p.view(torch.int16), out[perm].view(torch.int16))


@gpu
def test_gn_invalid_forced_paths_are_refused(ctx):
    """a forced path the shape does not admit is an error before anything launches: the output stays NaN"""
    big = build_case((320, 0, 1, 4096, 32, False))           # 4096 x 10 values per group: no small kernel holds them
    odd = build_case((40, 0, 1, 16, 4, False))               # cpg 10: neither 4- nor 8-channel pieces
    seam = build_case((8, 24, 1, 16, 2, False))              # fits every small kernel: only the path names below are wrong
    for case, path in ((big, (SMALL, 20, 4)), (big, (SMALL, 10, 8)), (odd, (SMALL, 5, 4)), (odd, (SMALL, 5, 8)), (seam, (SMALL, 7, 8)),
                       (seam, (SMALL, 10, 4)), (seam, (FINISH, 0, 0)), (seam, (7, 0, 0)), (seam, (MX, 0, 0))):
        rc, out, _ = run_gn(ctx, case, 0, force=path)
        assert rc == _lib.SVG_ERR_INVALID, path
        assert bool(torch.isnan(out).all())
    # 256 x 80 channels per group: exactly the register budget of <10,8> and <20,4>, one piece too many for the <5,*> kernels
    edge = build_case((1280, 1280, 1, 256, 32, False))
    assert edge.valid((SMALL, 10, 8)) and edge.valid((SMALL, 20, 4)) and not edge.valid((SMALL, 5, 8))
    rc, _, _ = run_gn(ctx, edge, 0, force=(SMALL, 5, 8))
    assert rc == _lib.SVG_ERR_INVALID


# ---- g. MX output ---------------------------------------------------------------------------------------------------------------------
MX_CASES = [(640, 320, 2, 1024, 32), (1280, 640, 2, 64, 32), (320, 0, 2, 300, 32), (96, 0, 3, 20, 8), (40, 56, 2, 20, 8), (320, 320, 1, 4096, 32)]


def mx_random_input(c):
    return random_input(c[2], c[3], c[0] + c[1], c[4], 12)


@gpu
@pytest.mark.parametrize("c", MX_CASES, ids=str)
@pytest.mark.parametrize("data", ["integer", "random", "onehot"])
def test_gn_mx(ctx, c, data):
    """finish+apply_mx: the (mean, rstd) table against fp64; silu = 0: e4m3 elements and E8M0 scales bit for bit (up to the sign of zero)
    against the host's fma(x, rstd gamma, beta - mean rstd gamma) from that table (f64 products rounded once to f32, as the kernel's fmas)
    quantised by mx_quant_ref; silu = 1: dequantised against fp64 at the bound of c plus the e4m3 block error: the shared exponent is
    floor(log2 amax) - 8, so elements are below 2^9 scale units; those above 448 units saturate (OCP MX: at most 64 / 512 = 2^-3 relative),
    normal ones round at 3 mantissa bits (2^-4 relative), subnormal ones (below 2^-6 units) at a spacing of 2^-9 units.  Padding channels
    are zero with scale byte 127."""
    from test_fp8_gpu import mx_quant_ref
    C1, C2, B, HW, groups = c
    Cc, cpg = C1 + C2, (C1 + C2) // groups
    if data == "integer":
        xv = integer_input(B, HW, Cc, 11)
    elif data == "random":
        xv = mx_random_input(c)
    else:
        n = HW * cpg
        xv = onehot_input(B, HW, Cc, groups, {(b, g): divmod((97 * b + 31 * g + (n - 1) * (g % 2)) % n, cpg) for b in range(B) for g in range(groups)})
    x1, x2 = split(xv, C1, HALF.dtype)
    gamma, beta = affine(Cc, 4)
    case = Case(x1.cuda(), None if x2 is None else x2.cuda(), gamma, beta, groups, tps=(2, 5))
    want = describe_py(C1, C2, B, HW, groups, mx=True)
    Cp = want[3] * 8
    exact = data != "random"
    L = 0 if exact else chain_len(want, C1, C2, HW, groups, case.tps)
    mean, r, dm, dr = stats_ref_bound(case.x64, groups, case.eps, L)
    for silu in (0, 1):
        rc, (q, sc, st, fused), ran = run_gn(ctx, case, silu, with_parts=True, mx=True)
        assert rc == 0 and fused == 1 and ran == want, (rc, fused, ran, want)
        m_k, r_k = st[:, :, 0].double(), st[:, :, 1].double()
        if exact:
            assert torch.equal(st[:, :, 0], mean.reshape(B, groups).float()), "mean of exact sums is the correctly rounded quotient"
        assert bool(((m_k - mean.reshape(B, groups)).abs() <= dm.reshape(B, groups) + E32 * mean.reshape(B, groups).abs()).all())
        assert bool(((r_k - r.reshape(B, groups)).abs() <= dr.reshape(B, groups)).all())
        qv = q.reshape(B * HW, Cp)
        assert bool((qv[:, Cc:] & 0x7f == 0).all()) and bool((sc.reshape(B * HW, Cp // 32)[:, cdiv(Cc, 32):] == 127).all()), "padding channels"
        if silu == 0:
            a = (st[:, :, 1].repeat_interleave(cpg, 1) * gamma).float()                                  # fl(rstd gamma)
            # sh = fma(-mean, a, beta), one rounding: the compiler contracts `beta - mean * a` (the build's default, fp-contract=fast;
            # v_pk_fma_f32 in the code object).  A build without contraction would round the product first and fail here in the last bit.
            sh = (beta.double() - st[:, :, 0].repeat_interleave(cpg, 1).double() * a.double()).float()
            t = (case.x64 * a.double()[:, None, :] + sh.double()[:, None, :]).float().to(HALF.dtype).float()
            q_ref, sc_ref, _ = mx_quant_ref(t.reshape(B * HW, Cc))
            assert bool((sc_ref > 0).all()), "no all-zero block in this data (the fused pass gives such a block scale byte 127, quant_mx 0)"
            assert torch.equal(sc.reshape(B * HW, Cp // 32)[:, :Cc // 32], sc_ref), "E8M0 scales"
            same = (qv[:, :Cc] == q_ref) | (((qv[:, :Cc] & 0x7f) == 0) & ((q_ref & 0x7f) == 0))
            assert bool(same.all()), "%d e4m3 elements differ" % int((~same).sum())
        else:
            ref, bound, _ = gn_ref_bound(case.x64, gamma.double(), beta.double(), groups, case.eps, 1, L)
            scale = torch.exp2(sc.reshape(B * HW, Cp // 32).double() - 127).repeat_interleave(32, 1)
            deq = (qv.view(torch.float8_e4m3fn).double() * scale)[:, :Cc].reshape(B, HW, Cc)
            h = ref.abs() + bound                                                # the 16-bit value the quantiser saw is within this
            qb = torch.maximum(h * 2.0 ** -3, scale[:, :Cc].reshape(B, HW, Cc) * 2.0 ** -9)
            check(deq, ref, bound + qb, "mx silu1 %s %s" % (c, data))


@gpu
def test_gn_mx_declines(ctx):
    """groupnorm_mx must return false (nothing written, no error) without column sums for a source, when C is not a multiple of 32, C1
    not a multiple of 8, with more than 64 groups, or more than 1024 padded channel vectors"""
    for c, parts in (((96, 0, 2, 20, 8, False), False), ((40, 8, 2, 20, 6, False), True), ((36, 60, 2, 20, 8, False), True),
                     ((128, 128, 1, 4, 128, False), True), ((8224, 0, 1, 2, 32, False), True)):
        case = build_case(c)
        rc, (q, sc, st, fused), ran = run_gn(ctx, case, 1, with_parts=parts, mx=True)
        assert rc == 0 and fused == 0 and ran[0] == -1
        assert bool((q == 0xA5).all()) and bool((sc == 0xA5).all()) and bool(torch.isnan(st).all())
    # column sums for x only, two sources
    case = build_case((40, 56, 2, 20, 8, False))
    d = _lib.GnDesc()
    keep = [guarded(t) for t in (case.x1, case.x2, case.gamma, case.beta, case.parts()[0])]
    q = torch.full((40, 128), 0xA5, dtype=torch.uint8, device="cuda")
    sc = torch.full((40, 4), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((2, 8, 2), float("nan"), device="cuda")
    d.x, d.x2, d.gamma, d.beta, d.part1 = [k[1].data_ptr() for k in keep]
    d.C1, d.C2, d.B, d.HW, d.groups, d.eps, d.silu, d.tps1 = 40, 56, 2, 20, 8, 1e-5, 1, 3
    d.q, d.sc, d.stats = q.data_ptr(), sc.data_ptr(), st.data_ptr()
    fused = C.c_int(-1)
    assert getattr(ctx.lib, "svg_op_groupnorm_mx" + HALF.suffix)(ctx.h, C.byref(d), C.byref(fused), None, stream()) == 0
    torch.cuda.synchronize()
    assert fused.value == 0 and bool((q == 0xA5).all())


# ---- gn_finish, gn_fold_weights -----------------------------------------------------------------------------------------------------
def gn_finish(ctx, p1, C1, tps1, p2, C2, tps2, B, HW, groups, eps):
    keep = [guarded(p1)] + ([guarded(p2)] if p2 is not None else [])
    sb, st = nan_out((B, groups, 2), torch.float32)
    rc = ctx.lib.svg_op_gn_finish(ctx.h, keep[0][1].data_ptr(), C1, tps1, keep[1][1].data_ptr() if p2 is not None else None, C2, tps2,
                                  st.data_ptr(), B, HW, groups, eps, stream())
    torch.cuda.synchronize()
    assert rc == 0, ctx.lib.svg_last_error(ctx.h).decode()
    guards_intact(sb, "gn_finish")
    return st


@gpu
@pytest.mark.parametrize("shape", [(1280, 640, 64, 32, 1, 4), (640, 320, 1024, 32, 8, 2), (320, 0, 4096, 32, 16, 0), (40, 56, 20, 8, 3, 5),
                                   (24, 40, 300, 4, 7, 2)], ids=str)
def test_gn_finish(ctx, shape):
    """caller partials with tps1 != tps2 and groups that straddle C1.  Integer data: mean is the correctly rounded s / n bit for bit, rstd
    within the rsqrtf bound (L = 0).  One-hot partials: the sum 1 in a single (tile, channel) entry of a single sample, moved over
    every entry in turn by the batch index: mean must be exactly fl(1 / n) for that group and 0 for every other."""
    C1, C2, HW, groups, tps1, tps2 = shape
    Cc, cpg, B = C1 + C2, (C1 + C2) // groups, 3
    x = integer_input(B, HW, Cc, 21).double().cuda()
    p1 = make_parts(x[:, :, :C1], tps1)
    p2 = make_parts(x[:, :, C1:], tps2) if C2 else None
    st = gn_finish(ctx, p1, C1, tps1, p2, C2, tps2, B, HW, groups, 1e-5)
    mean, r, dm, dr = stats_ref_bound(x, groups, 1e-5, 0)
    assert torch.equal(st[:, :, 0], mean.reshape(B, groups).float())
    assert bool(((st[:, :, 1].double() - r.reshape(B, groups)).abs() <= dr.reshape(B, groups)).all())
    # one-hot partials: entry k of the concatenated (tile, channel) tables of both sources is hot in sample k
    n1, n2 = tps1 * C1, tps2 * C2
    Bh = min(n1 + n2, 4096)
    idx = torch.unique(torch.cat([torch.arange(0, n1 + n2, max(1, (n1 + n2) // Bh))[:Bh - 4], torch.tensor([n1 - 1, n1, n1 + n2 - 1, 0])]).clamp(0, n1 + n2 - 1))
    Bh = idx.numel()
    h1 = torch.zeros(Bh, tps1 * C1, 2)
    h2 = torch.zeros(Bh, max(n2, 1), 2)
    want = torch.zeros(Bh, groups)
    inv_n = float(torch.tensor(1.0) / torch.tensor(float(cpg) * float(HW)))
    for b, k in enumerate(idx.tolist()):
        if k < n1:
            h1[b, k, 0] = 1.0
            ch = k % C1
        else:
            h2[b, k - n1, 0] = 1.0
            ch = C1 + (k - n1) % C2
        want[b, ch // cpg] = inv_n
    st = gn_finish(ctx, h1.reshape(Bh * tps1, C1, 2).cuda(), C1, tps1, h2.reshape(Bh * tps2, C2, 2).cuda() if C2 else None, C2, tps2, Bh, HW, groups, 1e-5)
    assert torch.equal(st[:, :, 0].cpu(), want)


@gpu
@pytest.mark.parametrize("shape", [(3, 320, 320, 32, True), (2, 7, 328, 41, False), (4, 64, 1280, 32, True), (1, 5, 8, 1, False)], ids=str)
def test_gn_fold_weights(ctx, shape):
    """Wb within one 16-bit rounding (plus the two f32 products) of W gamma rstd; bb within the f32 bound of a C-term dot product:
    each of the ceil(C / 256) + 8 additions and 3 roundings per term at most, times sum |W (beta - mean rstd gamma)| (+ |bias|)"""
    B, N, Cc, groups, has_bias = shape
    g = torch.Generator().manual_seed(N)
    W = torch.randn(N, Cc, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda() if has_bias else None
    gamma, beta = affine(Cc, 6)
    stats = torch.stack([torch.randn(B, groups, generator=g) * 2, 0.2 + 3 * torch.rand(B, groups, generator=g)], 2).cuda()   # differ per sample
    keep = [guarded(t) for t in (W, gamma, beta, stats)] + ([guarded(bias)] if has_bias else [])     # inputs inside NaN guards
    W, gamma, beta, stats = (k[1] for k in keep[:4])
    bias = keep[4][1] if has_bias else None
    wb_b, Wb = nan_out((B, N, Cc), HALF.dtype)
    bb_b, bb = nan_out((B, N), torch.float32)
    rc = getattr(ctx.lib, "svg_op_gn_fold_weights" + HALF.suffix)(ctx.h, W.data_ptr(), bias.data_ptr() if has_bias else None, gamma.data_ptr(),
                                                                  beta.data_ptr(), stats.data_ptr(), Wb.data_ptr(), bb.data_ptr(), B, N, Cc, groups, stream())
    torch.cuda.synchronize()
    assert rc == 0
    guards_intact(wb_b, "Wb")
    guards_intact(bb_b, "bb")
    cpg = Cc // groups
    mean = stats[:, :, 0].double().repeat_interleave(cpg, 1)[:, None, :]
    rstd = stats[:, :, 1].double().repeat_interleave(cpg, 1)[:, None, :]
    wref = W.double()[None] * gamma.double() * rstd
    check(Wb, wref, wref.abs() * (HALF.u + 2.02 * E32) + HALF.tiny, "fold Wb %s" % (shape,))
    terms = W.double()[None] * (beta.double() - mean * rstd * gamma.double())
    absum = (W.double()[None].abs() * (beta.double().abs() + (mean * rstd * gamma.double()).abs())).sum(2)
    bref = terms.sum(2) + (bias.double() if has_bias else 0.0)
    bbound = E32 * (cdiv(Cc, 256) + 8 + 4) * (absum + (bias.double().abs() if has_bias else 0.0)) * 1.01 + 1e-40
    check(bb, bref, bbound, "fold bb %s" % (shape,))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def ln_bound(x, gamma, beta, eps, onepass_L=None):
    """x (M,C) f64.  Two-pass kernels (layernorm, ln_stats): mean over 4 x 8 sequential + 6 shuffle additions (L = 38), then
    sum (x - mean^)^2: the deviation carries dm, so var is off by e (L + 3) var + 2 dm sqrt(var) + dm^2: no cancellation term, flat in
    |mean| / sigma apart from dm = (L + 1) e mean|x|.  One-pass ln_finish (onepass_L = tiles): the GroupNorm form."""
    M, Cc = x.shape
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    A = x.abs().mean(1, keepdim=True)
    if onepass_L is None:
        L = 38
        dm = (L + 1) * E32 * A
        dv = E32 * (L + 3) * (var + dm * dm) + 2 * dm * var.sqrt() + dm * dm
    else:
        L = onepass_L
        m2 = (x * x).mean(1, keepdim=True)
        dm = (L + 1) * E32 * A
        dv = E32 * ((L + 2) * m2 + 2 * (L + 1) * mean.abs() * A + mean * mean + var) + dm * dm
    v = var + eps
    dv = dv + E32 * v
    r = v.rsqrt()
    lo_floor = eps * (1 - 2 * E32)
    dr = torch.maximum(r - (v + dv).rsqrt() * (1 - 4 * E32), torch.clamp(v - dv, min=lo_floor).rsqrt() * (1 + 4 * E32) - r)
    return mean, r, dm, dr


def ln_inputs(M, Cc, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "integer":
        return (torch.randint(-4, 5, (M, Cc), generator=g).float() + (torch.arange(Cc) % 7 - 3).float())
    if kind == "onehot":
        x = torch.zeros(M, Cc)
        x[torch.arange(M), (torch.arange(M) * 37 + 5) % Cc] = 4.0
        x[0, 0], x[M - 1, :] = 2.0, 0.0
        x[M - 1, Cc - 1] = 2.0
        return x
    x = torch.randn(M, Cc, generator=g)
    if kind == "offset":
        x = x + torch.tensor([0.0, 1.0, 8.0, 64.0, -64.0])[torch.arange(M) % 5][:, None]
    return x


@gpu
@pytest.mark.parametrize("kind", ["random", "integer", "onehot", "offset"])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 4099])
@pytest.mark.parametrize("Cc", [8, 64, 320, 520, 1280, 2048])
def test_layernorm_and_ln_stats(ctx, Cc, M, kind):
    """layernorm_kernel and ln_stats_kernel (four rows share a block: M = 1, 3, 4, 5, 4099) against fp64, per element; ln_stats agrees
    with ln_finish fed with exact (integer) partials over uneven column tiles"""
    x = ln_inputs(M, Cc, kind, M + Cc).to(HALF.dtype).cuda()
    gamma, beta = affine(Cc, 8)
    xb, xg = guarded(x)
    ob, out = nan_out((M, Cc), HALF.dtype)
    assert getattr(ctx.lib, "svg_op_layernorm" + HALF.suffix)(ctx.h, xg.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), M, Cc, 1e-5, stream()) == 0
    rb, rs = nan_out((M,), torch.float32)
    mb, rm = nan_out((M,), torch.float32)
    assert getattr(ctx.lib, "svg_op_ln_stats" + HALF.suffix)(ctx.h, xg.data_ptr(), rs.data_ptr(), rm.data_ptr(), M, Cc, 1e-5, stream()) == 0
    torch.cuda.synchronize()
    for b in (ob, rb, mb):
        guards_intact(b, "layernorm")
    x64 = x.double()
    mean, r, dm, dr = ln_bound(x64, gamma, beta, 1e-5)
    g64, b64 = gamma.double(), beta.double()
    y = (x64 - mean) * r * g64 + b64
    # ((x - mean^) rstd^ gamma + beta): the subtraction, two products, the sum (each e of its result), dm and dr carried through
    t = (x64 - mean).abs()
    E = 1.01 * ((t * dr + dm * (r + dr) + 3 * E32 * (t + dm) * (r + dr)) * g64.abs() + E32 * y.abs())
    check(out, y, E * (1 + HALF.u) + HALF.u * y.abs() + HALF.tiny, "layernorm C%d M%d %s" % (Cc, M, kind))
    check(rs, r[:, 0], dr[:, 0], "ln_stats rs C%d M%d %s" % (Cc, M, kind))
    check(rm, (r * mean)[:, 0], (dr * mean.abs() + dm * (r + dr) + E32 * (r * mean).abs())[:, 0] * 1.01 + 1e-40, "ln_stats rm")
    if kind in ("integer", "onehot"):
        tiles = 3 if Cc >= 24 else 1
        cuts = [round(i * Cc / tiles) for i in range(tiles + 1)]
        part = torch.stack([torch.stack([x64[:, cuts[i]:cuts[i + 1]].sum(1), (x64[:, cuts[i]:cuts[i + 1]] ** 2).sum(1)], 1) for i in range(tiles)], 1).float()
        pb, pg = guarded(part)
        fb, rs2 = nan_out((M,), torch.float32)
        gb2, rm2 = nan_out((M,), torch.float32)
        assert ctx.lib.svg_op_ln_finish(ctx.h, pg.data_ptr(), tiles, rs2.data_ptr(), rm2.data_ptr(), M, Cc, 1e-5, stream()) == 0
        torch.cuda.synchronize()
        guards_intact(fb, "ln_finish")
        m1, r1, dm1, dr1 = ln_bound(x64, gamma, beta, 1e-5, onepass_L=0)
        check(rs2, r1[:, 0], dr1[:, 0], "ln_finish rs (exact partials)")
        assert bool(((rs2.double() - rs.double()).abs() <= (dr + dr1)[:, 0]).all()), "ln_stats and ln_finish disagree"


@gpu
@pytest.mark.parametrize("Cc,tiles", [(320, 3), (1280, 8), (640, 5)])
def test_ln_finish_offset_rows(ctx, Cc, tiles):
    """ln_finish (one pass, E[x^2] - mean^2) on rows with |mean| / sigma of 0, 1, 8, 64: follows its cancellation bound; f32 partials
    of f64 sums (one rounding each, counted in L)"""
    M = 403
    x = ln_inputs(M, Cc, "offset", 3).to(HALF.dtype).double().cuda()
    cuts = [round(i * Cc / tiles) for i in range(tiles + 1)]
    part = torch.stack([torch.stack([x[:, cuts[i]:cuts[i + 1]].sum(1), (x[:, cuts[i]:cuts[i + 1]] ** 2).sum(1)], 1) for i in range(tiles)], 1).float()
    pb, pg = guarded(part)
    rb, rs = nan_out((M,), torch.float32)
    mb, rm = nan_out((M,), torch.float32)
    assert ctx.lib.svg_op_ln_finish(ctx.h, pg.data_ptr(), tiles, rs.data_ptr(), rm.data_ptr(), M, Cc, 1e-5, stream()) == 0
    torch.cuda.synchronize()
    guards_intact(rb, "ln_finish")
    guards_intact(mb, "ln_finish")
    mean, r, dm, dr = ln_bound(x, None, None, 1e-5, onepass_L=tiles + 1)
    check(rs, r[:, 0], dr[:, 0], "ln_finish rs offset rows")
    check(rm, (r * mean)[:, 0], (dr * mean.abs() + dm * (r + dr) + E32 * (r * mean).abs())[:, 0] * 1.01, "ln_finish rm offset rows")


# ---- softmax_rows ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1000, 4096])
def test_softmax_rows(ctx, cols):
    """rows of f32 scores with NaN in the input pad columns (never read) -> probabilities; output pad columns exactly zero.  Rows: random
    under a scale sweep, equal logits, one maximum far above the rest (every other probability exactly 0, the maximum exactly 1) and a
    largest scaled logit near 1e4.  Bound per element: the argument s scale - mx carries 2 e |s scale| (product and subtraction) on
    both logits, __expf (2 + 2 |arg|) ulp, the sum over cols terms ceil(cols / 256) + 8 additions, the division 2 ulp:
    |p^ - p| <= p (4 e (|s| + |mx|) + e (8 + 4 |arg|) + e (ceil(cols / 256) + 16)) 1.01 + u p + max(tiny, 2^-126): v_exp_f32 flushes a result
    below the smallest normal f32 to zero, and the normaliser is >= 1 (the maximum's own term)."""
    rows, ld_in, ld_out = 9, cols + 5, cols + 11
    g = torch.Generator().manual_seed(cols)
    s = torch.randn(rows, cols, generator=g) * 3
    s[1] = 0.75
    s[2] = torch.randn(cols, generator=g)
    s[2, cols // 2] = 400.0
    s[3] = torch.rand(cols, generator=g) * 50 + 9950.0
    s[3, cols - 1] = 1.0e4
    for scale in (1.0, 0.044194173824159216, 7.5):
        sin = torch.full((rows, ld_in), float("nan"))
        sin[:, :cols] = s
        if scale != 1.0:
            sin[3, :cols] = s[3] / scale
        ib, sg = guarded(sin)
        ob, out = nan_out((rows, ld_out), HALF.dtype)
        rc = getattr(ctx.lib, "svg_op_softmax_rows" + HALF.suffix)(ctx.h, sg.data_ptr(), out.data_ptr(), rows, cols, ld_in, ld_out, scale, stream())
        torch.cuda.synchronize()
        assert rc == 0
        guards_intact(ob, "softmax_rows")
        assert bool((out[:, cols:] == 0).all()), "pad columns must be written as zero"
        sc64 = sg[:, :cols].float().double() * float(torch.tensor(scale, dtype=torch.float32))
        mx = sc64.max(1, keepdim=True).values
        p = torch.softmax(sc64, 1)
        arg = (sc64 - mx).abs()
        bound = p * 1.01 * E32 * (4 * (sc64.abs() + mx.abs()) + 8 + 4 * arg + cdiv(cols, 256) + 16) + HALF.u * p + max(HALF.tiny, 2.0 ** -126)
        check(out[:, :cols], p, bound, "softmax cols %d scale %g" % (cols, scale))
        if scale >= 1.0 and cols > 1:
            row = out[2, :cols].float()
            assert float(row[cols // 2]) == 1.0 and float(row.sum()) == 1.0, "a dominant logit takes probability 1 exactly"
        assert bool(((out[1, :cols].double() - 1.0 / cols).abs() <= (HALF.u + 64 * E32) / cols + HALF.tiny).all()), "equal logits"


# ---- fold_ln, rowsum_h16 --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K,has_bias", [(5, 320, True), (3, 1000, False), (2, 8, True), (4, 2563, True)])
def test_fold_ln_and_rowsum(ctx, N, K, has_bias):
    g = torch.Generator().manual_seed(K)
    w = torch.randn(N, K, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda() if has_bias else None
    gamma, beta = affine(K, 9)
    wb, wg = guarded(w)
    ob, bout = nan_out((N,), torch.float32)
    assert ctx.lib.svg_op_fold_ln(ctx.h, wg.data_ptr(), bias.data_ptr() if has_bias else None, gamma.data_ptr(), beta.data_ptr(), bout.data_ptr(), N, K, stream()) == 0
    torch.cuda.synchronize()
    guards_intact(wb, "fold_ln w")
    guards_intact(ob, "fold_ln bias")
    assert torch.equal(wg, w * gamma), "w gamma is one f32 product"
    terms = w.double() * beta.double()
    ref = terms.sum(1) + (bias.double() if has_bias else 0.0)
    bnd = 1.01 * E32 * (cdiv(K, 256) + 8 + 2) * (terms.abs().sum(1) + (bias.double().abs() if has_bias else 0.0)) + 1e-40
    check(bout, ref, bnd, "fold_ln bias N%d K%d" % (N, K))
    wh = torch.randn(N, K, generator=g).to(HALF.dtype).cuda()
    hb, hg = guarded(wh)
    sb, so = nan_out((N,), torch.float32)
    assert getattr(ctx.lib, "svg_op_rowsum" + HALF.suffix)(ctx.h, hg.data_ptr(), so.data_ptr(), N, K, stream()) == 0
    torch.cuda.synchronize()
    guards_intact(sb, "rowsum")
    check(so, wh.double().sum(1), 1.01 * E32 * (cdiv(K, 256) + 8) * wh.double().abs().sum(1) + 1e-40, "rowsum N%d K%d" % (N, K))
    ints = torch.randint(-8, 9, (N, K), generator=g).to(HALF.dtype).cuda()
    hb, hg = guarded(ints)
    assert getattr(ctx.lib, "svg_op_rowsum" + HALF.suffix)(ctx.h, hg.data_ptr(), so.data_ptr(), N, K, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(so, ints.float().sum(1)), "integer rows sum exactly"


# ---- the bound against a replay of each path's summation order (no GPU) ---------------------------------------------------------------
def _butterfly(v):
    """wave_sum over the last axis (64 lanes): the xor butterfly, in f32"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(np.float32)
    return v[..., 0]


def _block_sum(v):
    """256 per-thread values -> the block total as the kernels form it: wave butterflies, then (w0 + w1) + (w2 + w3)"""
    w = _butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]).astype(np.float32) + (w[..., 2] + w[..., 3]).astype(np.float32)).astype(np.float32)


def emu_small(x, groups, maxch, vw):
    B, HW, Cc = x.shape
    cpg = Cc // groups
    flat = x.reshape(B, HW, groups, cpg).transpose(0, 2, 1, 3).reshape(B, groups, HW * cpg)
    pad = np.zeros((B, groups, 256 * maxch * vw), np.float32)
    pad[:, :, :HW * cpg] = flat
    a = pad.reshape(B, groups, maxch, 256, vw)
    s = np.zeros((B, groups, 256), np.float32)
    q = np.zeros((B, groups, 256), np.float32)
    for i in range(maxch):
        for j in range(vw):
            f = a[:, :, i, :, j]
            s = (s + f).astype(np.float32)
            q = (q + (f * f).astype(np.float32)).astype(np.float32)
    return _block_sum(s), _block_sum(q)


def emu_stats(x, groups, CV, PL, nchunk):
    B, HW, Cc = x.shape
    cpg = Cc // groups
    ppc = cdiv(HW, nchunk)
    tot_s = np.zeros((B, groups), np.float32)
    tot_q = np.zeros((B, groups), np.float32)
    for ch in range(nchunk):
        p0, p1 = ch * ppc, min(HW, ch * ppc + ppc)
        gs = np.zeros((B, groups), np.float32)
        gq = np.zeros((B, groups), np.float32)
        for pl in range(PL):
            s = np.zeros((B, Cc), np.float32)
            q = np.zeros((B, Cc), np.float32)
            p = p0 + pl
            while p + 3 * PL < p1:
                f0, f1, f2, f3 = (x[:, p + k * PL] for k in range(4))
                s = (s + ((f0 + f1).astype(np.float32) + (f2 + f3).astype(np.float32)).astype(np.float32)).astype(np.float32)
                sq = [(f * f).astype(np.float32) for f in (f0, f1, f2, f3)]
                q = (q + ((sq[0] + sq[1]).astype(np.float32) + (sq[2] + sq[3]).astype(np.float32)).astype(np.float32)).astype(np.float32)
                p += 4 * PL
            while p < p1:
                f = x[:, p]
                s = (s + f).astype(np.float32)
                q = (q + (f * f).astype(np.float32)).astype(np.float32)
                p += PL
            sg, qg = s.reshape(B, groups, cpg), q.reshape(B, groups, cpg)
            for cc in range(cpg):                     # the group reduction walks pixel lanes, then the channels of the group
                gs = (gs + sg[:, :, cc]).astype(np.float32)
                gq = (gq + qg[:, :, cc]).astype(np.float32)
        tot_s = (tot_s + gs).astype(np.float32)
        tot_q = (tot_q + gq).astype(np.float32)
    return tot_s, tot_q


def emu_finish(p1, C1, tps1, p2, C2, tps2, groups):
    B = p1.shape[0] // tps1
    cpg = (C1 + C2) // groups
    S = np.zeros((B, groups), np.float32)
    Q = np.zeros((B, groups), np.float32)
    for g in range(groups):
        lo, hi = g * cpg, g * cpg + cpg
        acc = np.zeros((B, 256, 2), np.float32)
        for part, Cs, tps, a, b in ((p1, C1, tps1, min(lo, C1), min(hi, C1)), (p2, C2, tps2, max(lo, C1) - C1, max(hi, C1) - C1)):
            if part is None or b <= a:
                continue
            e = part.reshape(B, tps, Cs, 2)[:, :, a:b].reshape(B, tps * (b - a), 2)
            k = cdiv(e.shape[1], 256)
            pad = np.zeros((B, k * 256, 2), np.float32)
            pad[:, :e.shape[1]] = e
            for i in range(k):
                acc = (acc + pad[:, i * 256:(i + 1) * 256]).astype(np.float32)
        S[:, g], Q[:, g] = _block_sum(acc[:, :, 0]), _block_sum(acc[:, :, 1])
    return S, Q


def emu_apply(x, s, q, gamma, beta, groups, eps, silu):
    """finish the statistics and normalise as the kernels do, in f32 (fma: an f64 product and sum rounded once)"""
    B, HW, Cc = x.shape
    cpg = Cc // groups
    n = np.float32(cpg) * np.float32(HW)
    mean = (s / n).astype(np.float32)
    var = np.maximum((q / n).astype(np.float32) - (mean * mean).astype(np.float32), np.float32(0)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    a = (np.repeat(rstd, cpg, 1) * gamma[None]).astype(np.float32)
    sh = (beta[None] - (np.repeat(mean, cpg, 1) * a).astype(np.float32)).astype(np.float32)
    f = (x.astype(np.float64) * a[:, None, :] + sh[:, None, :]).astype(np.float32)
    if silu:
        with np.errstate(over="ignore"):
            f = (f * (np.float32(1) / (np.float32(1) + np.exp(-f).astype(np.float32)))).astype(np.float32)
    return torch.from_numpy(f).to(HALF.dtype)


# every input the GPU tests bound with L > 0: the random / offset / single-ratio cases as they are, and the MX test's random inputs ("mx": 16-bit
# input, column sums over (2, 5) tiles, the finish path, whose statistics and fma gn_apply_mx shares)
CPU_CASES = (RANDOM_CASES + OFFSET_CASES + [sh + ((r,),) for r in RATIOS for sh in RATIO_SHAPES]
             + [c + (False, None, "mx") for c in MX_CASES])


def cpu_case_id(c):
    return case_id(c) + ("-mx" if len(c) > 7 else "")


@pytest.mark.parametrize("c", CPU_CASES, ids=cpu_case_id)
def test_gn_bounds_hold_for_emulated_paths_cpu(c):
    """no GPU: each path's summation order replayed in numpy f32 stays inside the bound the GPU tests use, on the same inputs, and the
    bound is not vacuous: for groups with |mean| <= sigma it is below 2 u (|gamma| max(|x - mean| rstd, 1) + |beta|) + tiny"""
    is_mx = len(c) > 7
    if is_mx:
        x1, x2 = split(mx_random_input(c), c[0], HALF.dtype)
        gamma, beta = affine(c[0] + c[1], 4, "cpu")
        case = Case(x1, x2, gamma, beta, c[4], tps=(2, 5))
    else:
        case = build_case(c, dev="cpu")
    x = case.x64.float().numpy()
    gam, bet = case.gamma.numpy(), case.beta.numpy()
    worst = 0.0
    for path in ([(FINISH, 0, 0)] if is_mx else PATHS):
        if not case.valid(path):
            continue
        desc = describe_py(case.C1, case.C2, case.B, case.HW, case.groups, have_stats=path[0] == FINISH, force=path)
        if path[0] == SMALL:
            s, q = emu_small(x, case.groups, path[1], path[2])
        elif path[0] == STATS:
            s, q = emu_stats(x, case.groups, desc[3], desc[4], desc[5])
        else:
            p1, p2 = case.parts()
            s, q = emu_finish(p1.numpy(), case.C1, case.tps[0], None if p2 is None else p2.numpy(), case.C2, case.tps[1], case.groups)
        for silu in (0, 1):
            out = emu_apply(x, s, q, gam, bet, case.groups, case.eps, silu)
            ref, bound, mag = case.ref(silu, desc)
            check(out, ref, bound, "replay %s %s silu%d %s" % (cpu_case_id(c), path_id(path), silu, HALF.name))
            xg = case.x64.reshape(case.B, case.HW, case.groups, -1)
            well = (xg.mean((1, 3), keepdim=True).abs() <= xg.std((1, 3), unbiased=False, keepdim=True)).expand_as(xg).reshape(ref.shape)
            if bool(well.any()):
                k = float(((bound[well] - HALF.tiny) / (HALF.u * mag[well] + 1e-300)).max())
                worst = max(worst, k)
                assert k <= 2.0, "the bound is %.2f u of the pre-activation magnitude for a well-conditioned group" % k
    print("[norm] %s %s: bound <= %.3f u (|gamma| max(|x - mean| rstd, 1) + |beta|) on well-conditioned groups" % (case_id(c), HALF.name, worst))


def test_describe_py_matches_the_documented_cases_cpu():
    """the dispatch rule at the UNet's shapes: the 8 x 8 and 16 x 16 levels take one launch, cpg = 60 only in 4-channel pieces"""
    assert describe_py(1280, 640, 2, 64, 32)[:3] == (SMALL, 5, 4)
    assert describe_py(1280, 640, 2, 256, 32)[:3] == (SMALL, 20, 4)
    assert describe_py(1280, 1280, 2, 256, 32)[:3] == (SMALL, 10, 8)
    assert describe_py(1280, 0, 2, 64, 32)[:3] == (SMALL, 5, 8)
    assert describe_py(640, 320, 2, 1024, 32)[0] == STATS and describe_py(640, 320, 2, 1024, 32, have_stats=True)[0] == FINISH
    assert describe_py(640, 320, 2, 1024, 32, mx=True)[3] == 128
