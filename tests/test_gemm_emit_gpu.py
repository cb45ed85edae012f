"""What a GEMM / conv tile epilogue leaves behind for the next normalisation (GemmArgs::gn_part / ln_part, csrc/kernels.h), the two-source
A operand and the stride-2 / Cin = 8 conv gathers, on every kernel path, against fp64.  A sibling of tests/test_gemm_epilogue_gpu.py: the
problems are built, launched and value-checked by its run_case; this file adds the emission check behind it.

Contract under test:
  gn_part[(tile_m * N + n) * 2 + {0, 1}] = sum, sum of squares of the STORED values of column n over the rows of row tile tile_m.  A row
      tile is gn_rows consecutive rows (plan[3]); on conv_halo it is one 16 x 16 pixel block, tile_m = (b * Ho/16 + y/16) * Wo/16 + x/16.
  ln_part[((z * M + m) * ln_tiles + tile_n) * 2 + {0, 1}] = the same of row m over the bn columns of column tile tile_n (bn = path[1]).
The callers' protocol is the tests': svg_op_gemm_plan -> fill gn_part / ln_part / ln_tiles from the plan -> svg_op_gemm_ex.  Every case
asserts the plan {family, bn, splitk, gn_rows, ln_tiles} and the reported path first.

Reference: fp64 sums of the kernel's own stored C, read back (the arithmetic of C is judged by run_case as in the sibling file).
Judging, no fitted constant:
  * integer-exact and one-hot data: every stored value is a multiple of 1/4 with sum |v| < 2^22 and sum v^2 < 2^20 per partial (asserted),
    so every f32 partial sum is exact in any order: the partials must EQUAL the fp64 sums;
  * random data: |s^ - s| <= (n - 1) 2^-24 sum |v| and |q^ - q| <= (n - 1) 2^-24 sum v^2 with n the terms of the partial (gn_rows, or bn):
    the any-order f32 summation bound; the square of an 8- or 11-bit-significand value is exact in f32, so squaring adds no term;
  * gn_part / ln_part are NaN-filled between NaN guards: afterwards exactly the row_tiles x N x 2 (resp. batch x M x ln_tiles x 2) slots are
    finite and the guards untouched (a slot for a column >= N, with ldc > N, would land in a neighbour or a guard); rows past M add zero
    (the reference pads with zeros); columns n_valid .. N - 1 count with the value the epilogue stored there;
  * the launch is issued a second time into re-filled buffers: bit-identical partials and guards.
One-hot probes (run_case: onehot): operands that leave exactly one power of two per (row tile, column), at the first and last row of the
tile and both sides of every 16-row boundary, another position for every column — a lane map, butterfly or LDS meeting that drops or
doubles one element is wrong by that element's whole value; the same per (row, column tile) across the column seams for ln_part.

Paths (plan as reported by svg_op_gemm_plan; conv_halo under SVG_HALO_MIN=1, as in the sibling file):
  igemm BN 32 / 64          gn         M 300 (two 128-row tiles + 44 rows), K 64
  igemm BN 128 / 160        gn + ln    300 x 320 x 64 (BN 128: also n_valid 316, ldc 328, batch 2 for ln), 6572 x 640 x 64 and 8236 x 400 x 64 (BN 160)
  gemm_pp BN 128 / 160      gn + ln    16165 x 320 x 1024, 24357 x 320 x 1024 (192 tiles of 256 rows, the last one 37 rows)
  gemm_ws                   gn + ln    16421 x {320, 640} x 320, with and without residual
  conv_halo BN 128 / 160    gn         (1,16,16,64,128), (2,32,32,128,160), (2,32,32,64,320), (13,32,32,64,640); stride 1 and nearest-2x
  implicit-GEMM conv        gn         (31,20,20,64,320): sides no multiple of 16, 194 tiles, no split-K
Two-source A ([A | A2], igemm only) and the stride-2 / Cin = 8 gathers are value tests of run_case (per-element bound of the sibling file).
test_judge_rejects_wrong_partials needs no GPU: it shows the random-data judge rejecting a dropped or doubled element, a shifted tile
boundary or column seam and two swapped columns."""
import math

import pytest
import torch

from test_gemm_epilogue_gpu import (ACT_GEGLU, ACT_GELU, ACT_SILU, HALF, HALO, IGEMM, PP, WS, _knobs, _refused, _storage,  # noqa: F401
                                    conv_out_hw, gemm_plan, run_case)

gpu = pytest.mark.gpu
GUARD = 64          # NaN floats in front of and behind a partial buffer
_NOSK = {"SVG_IGEMM_SK": "1"}                 # gemm_plan's knob: no split-K for launches below 192 tiles


# ---- reference and judge (pure torch: also used without a GPU) ---------------------------------------------------------------
def gn_reference(stored, rows, blocks=None):
    """stored (M, N) f64 -> (s, q, sum |v|) of shape (row tiles, N).  blocks = (B, Ho, Wo): the halo conv's 16 x 16 pixel blocks"""
    M, N = stored.shape
    if blocks is not None:
        B, Ho, Wo = blocks
        assert rows == 256 and M == B * Ho * Wo and Ho % 16 == 0 and Wo % 16 == 0
        v = stored.reshape(B, Ho // 16, 16, Wo // 16, 16, N).permute(0, 1, 3, 2, 4, 5).reshape(-1, 256, N)
    else:
        tiles = (M + rows - 1) // rows
        v = torch.zeros(tiles * rows, N, dtype=stored.dtype, device=stored.device)      # rows past M contribute zero
        v[:M] = stored
        v = v.reshape(tiles, rows, N)
    return v.sum(1), (v * v).sum(1), v.abs().sum(1)


def ln_reference(stored, bn):
    """stored (R, N) f64 -> (s, q, sum |v|) of shape (R, column tiles)"""
    R, N = stored.shape
    tiles = (N + bn - 1) // bn
    v = torch.zeros(R, tiles * bn, dtype=stored.dtype, device=stored.device)
    v[:, :N] = stored
    v = v.reshape(R, tiles, bn)
    return v.sum(2), (v * v).sum(2), v.abs().sum(2)


def bounds(ref, n_terms):
    return (n_terms - 1) * 2.0 ** -24 * ref[2], (n_terms - 1) * 2.0 ** -24 * ref[1]


def judge(got_s, got_q, ref, n_terms, integer):
    """mask of the partials that pass"""
    if integer:
        return (got_s == ref[0]) & (got_q == ref[1])
    bs, bq = bounds(ref, n_terms)
    return ((got_s - ref[0]).abs() <= bs) & ((got_q - ref[1]).abs() <= bq)


def assert_exactly_summable(ref):
    assert float(ref[2].max()) < 2.0 ** 22 and float(ref[1].max()) < 2.0 ** 20, "the integer data leaves sums an f32 cannot hold exactly"


class Emit:
    """the emission half of one run_case: see the module docstring"""

    def __init__(self, plan, gn=True, ln=True, blocks=None):
        self.plan, self.blocks = tuple(plan), blocks
        self.want_gn, self.want_ln = gn and plan[3] > 0, ln and plan[4] > 0
        assert self.want_gn or self.want_ln

    def _buffer(self, n):
        return torch.full((GUARD + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)

    def prepare(self, ctx, desc, env):
        with env:
            rc, plan = gemm_plan(ctx, **desc)
        ctx.check(rc, "gemm_plan")
        assert plan == self.plan, "plan %s, expected %s" % (plan, self.plan)
        self.M, self.N, self.batch = desc["M"], desc["N"], desc["batch"]
        self.bufs = []
        if self.want_gn:
            self.tiles_m = self.M // 256 if self.plan[0] == HALO else (self.M + self.plan[3] - 1) // self.plan[3]
            self.gn = self._buffer(self.tiles_m * self.N * 2)
            desc["gn_part"] = self.gn[GUARD:]
            self.bufs.append(self.gn)
        if self.want_ln:
            self.ln = self._buffer(self.batch * self.M * self.plan[4] * 2)
            desc.update(ln_part=self.ln[GUARD:], ln_tiles=self.plan[4])
            self.bufs.append(self.ln)
        with env:                                  # ask-then-launch: the answer does not change once the statistics are asked for
            rc, plan = gemm_plan(ctx, **desc)
        assert rc == 0 and plan == self.plan, "plan %s once gn_part / ln_part are set, %s before" % (plan, self.plan)

    def _one(self, name, buf, shape, ref, n_terms, integer):
        body = buf[GUARD:-GUARD]
        assert bool(buf[:GUARD].isnan().all()) and bool(buf[-GUARD:].isnan().all()), name + ": written outside the partial buffer"
        assert bool(body.isfinite().all()), "%s: %d slots were never written" % (name, int((~body.isfinite()).sum()))
        got = body.double().reshape(*shape, 2)
        if integer:
            assert_exactly_summable(ref)
        ok = judge(got[..., 0], got[..., 1], ref, n_terms, integer)
        if not bool(ok.all()):
            i = tuple(int(v) for v in (~ok).nonzero()[0])
            bs, bq = bounds(ref, n_terms)
            raise AssertionError("%s: %d of %d partials wrong; first at %s: sum %.9g vs %.9g (bound %.3g), squares %.9g vs %.9g (bound %.3g)" % (
                name, int((~ok).sum()), ok.numel(), i, float(got[i][0]), float(ref[0][i]), 0.0 if integer else float(bs[i]),
                float(got[i][1]), float(ref[1][i]), 0.0 if integer else float(bq[i])))

    def check(self, ctx, out, integer, launch):
        """out: the stored C, (batch, M, N) f64"""
        assert out.shape == (self.batch, self.M, self.N)
        torch.cuda.synchronize()
        if self.want_gn:
            assert self.batch == 1
            self._one("gn_part", self.gn, (self.tiles_m, self.N), gn_reference(out[0], self.plan[3], self.blocks), self.plan[3], integer)
        if self.want_ln:
            self._one("ln_part", self.ln, (self.batch * self.M, self.plan[4]), ln_reference(out.reshape(-1, self.N), self.plan[1]),
                      self.plan[1], integer)
        first = [b.clone() for b in self.bufs]
        for b in self.bufs:
            b.fill_(float("nan"))
        rc, path = launch()
        ctx.check(rc, "gemm_ex (second launch)")
        torch.cuda.synchronize()
        assert path == self.plan[:3]
        for a, b in zip(first, self.bufs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the second launch left other bits in %d slots" % int(
                (a.view(torch.int32) != b.view(torch.int32)).sum())


# ---- the path x data matrix --------------------------------------------------------------------------------------------------
def _emit_bundle(tag, plan, base, feats, onehot=True, blocks=None, ln=True, a_keep=8):
    """one shape on one path: integer-exact and random data with the features of `feats`, and the one-hot probes the path can emit.
    a_keep thins the integer A so that the sums stay exactly representable: the integer weights are c[n] + k mod 3, so a row of C is
    c[n] S + T with S, T sums over the row of A, and a row partial over bn columns is about bn (2 S^2 + T^2) — S^2 reaches 25 K E[a^2]
    over thousands of rows, which has to stay below 2^20 / (3.7 bn)"""
    out = [
        (tag + "-int", plan, dict(base, a_keep=a_keep, **feats.get("int", {})), dict(blocks=blocks, ln=ln)),
        (tag + "-rand", plan, dict(base, data="rand", **feats.get("rand", {})), dict(blocks=blocks, ln=ln)),
    ]
    if onehot and plan[3] > 0:
        out.append((tag + "-onehot-gn", plan, dict(base, onehot=("gn", plan[3])), dict(blocks=blocks, ln=False)))
    if onehot and ln and plan[4] > 0:
        out.append((tag + "-onehot-ln", plan, dict(base, onehot=("ln", plan[1])), dict(gn=False)))
    return out


def _conv(B, H, W, Cin, N, mode="S1", **kw):
    Ho, Wo = (2 * H, 2 * W) if mode == "UP2" else (H, W)
    return dict(M=B * Ho * Wo, N=N, K=9 * Cin, conv=(B, H, W, Cin, mode), **kw)


_F_BIAS_RES = {"int": dict(bias="col", res_pad=8), "rand": dict(bias="col", res_pad=0, act=ACT_SILU)}
_F_PLAIN = {"int": dict(bias="col"), "rand": dict(bias="col", res_pad=8)}

EMIT_CASES = (
    _emit_bundle("igemm32", (IGEMM, 32, 1, 128, 0), dict(M=300, N=32, K=64), _F_BIAS_RES)
    + _emit_bundle("igemm64", (IGEMM, 64, 1, 128, 0), dict(M=300, N=64, K=64, lda_pad=8), _F_BIAS_RES)
    + _emit_bundle("igemm128", (IGEMM, 128, 1, 128, 3), dict(M=300, N=320, K=64), _F_BIAS_RES)
    + _emit_bundle("igemm128-nvalid", (IGEMM, 128, 1, 128, 3), dict(M=300, N=320, K=64, n_valid=316), _F_PLAIN, onehot=False)
    + _emit_bundle("igemm128-ldc", (IGEMM, 128, 1, 128, 3), dict(M=300, N=320, K=64, ldc_pad=8), _F_BIAS_RES, onehot=False)
    + _emit_bundle("igemm128-n640", (IGEMM, 128, 1, 128, 5), dict(M=300, N=640, K=64), {"rand": dict(bias="col", act=ACT_GELU)}, onehot=False)
    + _emit_bundle("igemm160", (IGEMM, 160, 1, 128, 4), dict(M=6572, N=640, K=64), _F_BIAS_RES)
    + _emit_bundle("igemm160-n400", (IGEMM, 160, 1, 128, 3), dict(M=8236, N=400, K=64, ldc_pad=8), _F_PLAIN)
    # batch 2: the LayerNorm partials are indexed by (z * M + m); GroupNorm sums are not emitted (gn_rows 0)
    + _emit_bundle("igemm128-batch2-ln", (IGEMM, 128, 1, 0, 3), dict(M=300, N=320, K=64, batch=2, sB="shared", sC_pad=16),
                   {"int": dict(bias="col"), "rand": dict(bias="col", bias_zs=True)}, onehot=False)
    + _emit_bundle("pp128", (PP, 128, 1, 256, 3), dict(M=16165, N=320, K=1024), _F_BIAS_RES, a_keep=64)
    + _emit_bundle("pp160", (PP, 160, 1, 256, 2), dict(M=24357, N=320, K=1024, ldc_pad=8), _F_PLAIN, a_keep=64)
    + _emit_bundle("ws320", (WS, 160, 1, 128, 2), dict(M=16421, N=320, K=320), {"int": dict(bias="col"), "rand": dict(bias="col", act=ACT_SILU)},
                   a_keep=32)
    + _emit_bundle("ws640-res", (WS, 160, 1, 128, 4), dict(M=16421, N=640, K=320, ldc_pad=8),
                   {"int": dict(bias="col", res_pad=8), "rand": dict(bias="col", res_pad=0)}, a_keep=32)
    + _emit_bundle("conv-igemm160", (IGEMM, 160, 1, 128, 0), _conv(31, 20, 20, 64, 320), {"int": dict(bias="col", res_pad=8), "rand": dict(bias="col")},
                   a_keep=8)
)
for _mode in ("S1", "UP2"):
    _h = 1 if _mode == "S1" else 2          # the source image of an upsampling conv has half the sides
    for _tag, _bn, (_B, _S, _Cin, _N), _feats in (
            ("halo128-1blk", 128, (1, 16, 64, 128), {"int": dict(bias="col"), "rand": dict(bias="col", res_pad=0)}),
            ("halo128-n160", 128, (2, 32, 128, 160), {"int": dict(bias="col", res_pad=8), "rand": dict(bias="col", bias_bn=(1024, None))}),
            ("halo128-n320", 128, (2, 32, 64, 320), {"int": dict(n_valid=316, ldc_pad=8), "rand": dict(bias="col", act=ACT_SILU)}),
            ("halo160-n640", 160, (13, 32, 64, 640), {"int": dict(bias="col"), "rand": dict(bias="col", res_pad=8)})):
        EMIT_CASES += _emit_bundle("%s-%s" % (_tag, _mode), (HALO, _bn, 1, 256, 0), _conv(_B, _S // _h, _S // _h, _Cin, _N, _mode, halo_min=True), _feats,
                                   onehot=_mode == "S1", blocks=(_B, _S, _S), a_keep=64)        # (UP2: four output pixels share a source pixel)


@gpu
@pytest.mark.parametrize("plan,kw,ekw", [pytest.param(p, kw, ekw, id=i) for i, p, kw, ekw in EMIT_CASES])
def test_emitted_partials(ctx, plan, kw, ekw):
    run_case(ctx, plan[:3], emit=Emit(plan, **ekw), **kw)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@gpu
def test_emission_refused_where_the_plan_cannot_emit(ctx):
    """gn_part / ln_part on a launch whose plan has gn_rows / ln_tiles 0 (split-K, batch > 1, f32 output, GEGLU, a conv with ln_part), or an
    ln_tiles that is not the plan's: an error status, nothing launched (C and the partial buffers still all NaN)"""
    dt = HALF.dtype
    part = torch.full((1 << 20,), float("nan"), device="cuda")

    def dense(M, N, K, batch=1, **f):
        A = torch.ones(batch, M, K, device="cuda", dtype=dt)
        W = torch.ones(batch, N, K, device="cuda", dtype=dt)
        ldc = f.pop("ldc", N)
        Cb = torch.full((batch, M, ldc), float("nan"), device="cuda", dtype=torch.float32 if f.get("out_f32") else dt)
        d = dict(A=A, lda=K, Wt=W, ldb=K, C=Cb, ldc=ldc, M=M, N=N, K=K, batch=batch, **f)
        if batch > 1:
            d.update(sA=M * K, sB=N * K, sC=M * ldc)
        return d

    def refuse(what, want_plan, d, **emit):
        rc, plan = gemm_plan(ctx, **d)
        assert rc == 0 and plan == want_plan, "%s: plan %s, expected %s" % (what, plan, want_plan)
        _refused(ctx, what, **dict(d, **emit))
        assert bool(part.isnan().all()), what + ": the partial buffer was written"

    refuse("gn_part with split-K", (IGEMM, 128, 5, 0, 0), dense(256, 640, 1280), gn_part=part)
    refuse("ln_part with split-K", (IGEMM, 128, 5, 0, 0), dense(256, 640, 1280), ln_part=part, ln_tiles=5)
    refuse("gn_part with batch 2", (IGEMM, 128, 1, 0, 2), dense(256, 256, 128, batch=2), gn_part=part)
    refuse("gn_part with f32 output", (IGEMM, 128, 1, 0, 0), dense(300, 320, 64, out_f32=1), gn_part=part)
    refuse("ln_part with f32 output", (IGEMM, 128, 1, 0, 0), dense(300, 320, 64, out_f32=1), ln_part=part, ln_tiles=3)
    refuse("gn_part with GEGLU", (IGEMM, 128, 1, 0, 0), dense(256, 256, 128, act=ACT_GEGLU, ldc=128), gn_part=part)
    refuse("ln_part with GEGLU", (IGEMM, 128, 1, 0, 0), dense(256, 256, 128, act=ACT_GEGLU, ldc=128), ln_part=part, ln_tiles=2)
    refuse("ln_tiles 2 where the plan has 3", (IGEMM, 128, 1, 128, 3), dense(300, 320, 64), ln_part=part, ln_tiles=2)
    refuse("ln_tiles 0 where the plan has 3", (IGEMM, 128, 1, 128, 3), dense(300, 320, 64), ln_part=part)
    x = torch.ones(2, 24, 24, 64, device="cuda", dtype=dt)
    Wc = torch.ones(128, 576, device="cuda", dtype=dt)
    Cc = torch.full((2 * 24 * 24, 128), float("nan"), device="cuda", dtype=dt)
    conv = dict(A=x, amode=1, H=24, W=24, Cin=64, Ho=24, Wo=24, Wt=Wc, ldb=576, C=Cc, ldc=128, M=2 * 24 * 24, N=128, K=576)
    with _knobs(_NOSK):          # (no split-K, so that only the conv stands between the launch and its ln_part)
        refuse("a conv with ln_part", (IGEMM, 128, 1, 128, 0), conv, ln_part=part, ln_tiles=1)


# ---- two-source A ------------------------------------------------------------------------------------------------------------
_P128 = (IGEMM, 128, 1, 128, 3)
A2_CASES = []
for _ks in (64, 192, 128):                    # k_split in {64, K - 64, K / 2} of K = 256
    A2_CASES += [
        ("a2-k%d-int-bias-res" % _ks, _P128, dict(M=300, N=320, K=256, a2=(_ks, 8), lda_pad=16, a_keep=16, bias="col", res_pad=8, ldc_pad=8), True),
        ("a2-k%d-rand-silu" % _ks, _P128, dict(M=300, N=320, K=256, a2=(_ks, 0), lda_pad=8, data="rand", bias="col", res_pad=0, act=ACT_SILU), True),
        ("a2-k%d-rand-gelu-biasbn" % _ks, _P128, dict(M=300, N=320, K=256, a2=(_ks, 16), data="rand", bias="col", bias_bn=(100, None), act=ACT_GELU,
                                                      n_valid=316), False),
    ]
A2_CASES += [("a2-k64-int-bn64", (IGEMM, 64, 1, 128, 0), dict(M=300, N=64, K=128, a2=(64, 8), bias="col"), True),
             ("a2-k128-int-ln", _P128, dict(M=300, N=320, K=256, a2=(128, 8), lda_pad=8, bias="col", ln="normal", alpha=0.5), False)]


@gpu
@pytest.mark.parametrize("plan,kw,emits", [pytest.param(p, kw, e, id=i) for i, p, kw, e in A2_CASES])
def test_two_source_a(ctx, plan, kw, emits):
    """C = [A | A2] W^T against cat([A, A2]) in fp64; ragged M, padded lda / lda2; with an emitting epilogue where `emits`"""
    run_case(ctx, plan[:3], emit=Emit(plan) if emits else None, **kw)


@gpu
def test_two_source_a_stays_on_the_tiled_kernel(ctx):
    """the shapes gemm_ws and gemm_pp take go to the tiled kernel once A2 is set (those kernels read one A)"""
    p = torch.zeros(64, device="cuda", dtype=HALF.dtype)
    for M, N, K, family in ((16421, 320, 320, WS), (24357, 320, 1024, PP)):
        d = dict(A=p, lda=K, Wt=p, ldb=K, C=p, ldc=N, M=M, N=N, K=K)
        rc, plan = gemm_plan(ctx, **d)
        assert rc == 0 and plan[0] == family, plan
        rc, plan = gemm_plan(ctx, **dict(d, lda=K // 2, A2=p, lda2=K // 2, k_split=K // 2 // 64 * 64))
        assert rc == 0 and plan[0] == IGEMM and plan[2] == 1, plan


# ---- stride-2 and Cin = 8 gathers --------------------------------------------------------------------------------------------
def _sconv(B, H, W, Cin, N, mode, **kw):
    Ho, Wo = conv_out_hw(H, W, mode)
    return dict(M=B * Ho * Wo, N=N, K=72 if mode == "SMALLC" else 9 * Cin, conv=(B, H, W, Cin, mode), **kw)


GATHER_CASES = []
for _m in ("S2P1", "S2A"):
    GATHER_CASES += [
        (_m + "-16x16-sk2-int", (IGEMM, 64, 2), _sconv(2, 16, 16, 64, 64, _m, bias="col", res_pad=8, alpha=2.0, ldc_pad=8, n_valid=60), None),
        (_m + "-16x16-sk2-rand", (IGEMM, 64, 2), _sconv(2, 16, 16, 64, 64, _m, data="rand", bias="col", act=ACT_SILU), None),
        (_m + "-16x16-int", (IGEMM, 64, 1), _sconv(2, 16, 16, 64, 64, _m, bias="col", res_pad=0, knobs=_NOSK), None),
        (_m + "-16x16-rand", (IGEMM, 64, 1), _sconv(2, 16, 16, 64, 64, _m, data="rand", bias="col", bias_bn=(64, None), knobs=_NOSK), None),
        (_m + "-12x12-sk4-int", (IGEMM, 64, 4), _sconv(1, 12, 12, 128, 64, _m, bias="col", ldc_pad=8), None),
        (_m + "-12x12-rand", (IGEMM, 64, 1), _sconv(1, 12, 12, 128, 64, _m, data="rand", bias="col", res_pad=8, knobs=_NOSK), None),
        (_m + "-13x11-sk2-int", (IGEMM, 64, 2), _sconv(1, 13, 11, 64, 64, _m, bias="col"), None),
        (_m + "-13x11-rand", (IGEMM, 64, 1), _sconv(1, 13, 11, 64, 64, _m, data="rand", bias="col", knobs=_NOSK), None),
        # without split-K the downsampler's epilogue emits GroupNorm sums like any other
        (_m + "-16x16-int-emit", (IGEMM, 64, 1), _sconv(2, 16, 16, 64, 64, _m, a_keep=8, bias="col", knobs=_NOSK), (IGEMM, 64, 1, 128, 0)),
    ]
GATHER_CASES += [
    ("smallc-n320-int", (IGEMM, 160, 1), _sconv(2, 12, 10, 8, 320, "SMALLC", bias="col", ldc_pad=8), (IGEMM, 160, 1, 128, 0)),
    ("smallc-n320-rand", (IGEMM, 160, 1), _sconv(2, 12, 10, 8, 320, "SMALLC", data="rand", bias="col", act=ACT_SILU), None),
    ("smallc-n128-int", (IGEMM, 128, 1), _sconv(2, 12, 10, 8, 128, "SMALLC", bias="col", res_pad=8), None),
    ("smallc-n128-rand", (IGEMM, 128, 1), _sconv(2, 12, 10, 8, 128, "SMALLC", data="rand", bias="col"), (IGEMM, 128, 1, 128, 0)),
]


@gpu
@pytest.mark.parametrize("path,kw,plan", [pytest.param(p, kw, e, id=i) for i, p, kw, e in GATHER_CASES])
def test_conv_gathers(ctx, path, kw, plan):
    """3x3 conv, stride 2 with padding 1 (S2P1) and with right / bottom padding only (S2A), odd sides included, and the Cin = 8 stride-1
    form (K = 72: the padded first conv), through the tiled kernel with and without split-K: path, per-element bound, NaN outside"""
    run_case(ctx, path, emit=Emit(plan) if plan else None, **kw)


# ---- the judge has teeth (no GPU) --------------------------------------------------------------------------------------------
def test_judge_rejects_wrong_partials():
    """On a stored tensor like the random cases' (unit-variance values rounded to the storage type; 300 x 320: ragged row and column tiles),
    with f32 sums standing in for the kernel: the judge accepts them, and rejects every partial that lost or doubled one element, whose
    tile boundary or column seam moved by one, or that was swapped with its neighbour column's — except where the change itself is within
    twice the bound (f32 sums may use one bound themselves), which is checked to be under 1 % of the probes."""
    g = torch.Generator().manual_seed(20)
    v = torch.randn(300, 320, generator=g, dtype=torch.float64).to(HALF.dtype).double()

    def probe(what, ref, got, n_terms, d_s, d_q, real=None):
        """d_s, d_q: what the mutation adds to (s, q), broadcastable against the partials' shape with extra leading dims; real: mask of
        the probes that stand for a stored element (default: all)"""
        bs, bq = bounds(ref, n_terms)
        skip = (d_s.abs() <= 2 * bs) & (d_q.abs() <= 2 * bq)
        share = float(skip.double().mean() if real is None else skip[real].double().mean())
        assert share < 0.01, "%s: %.2f %% of the probes are below the bound" % (what, 100 * share)
        ok = judge(got[0] + d_s, got[1] + d_q, ref, n_terms, False)
        assert not bool((ok & ~skip).any()), "%s: %d wrong partials accepted" % (what, int((ok & ~skip).sum()))

    for rows in (128, 256):
        ref = gn_reference(v, rows)
        tiles = ref[0].shape[0]
        pad = torch.zeros(tiles * rows, 320, dtype=torch.float64)
        pad[:300] = v
        t = pad.reshape(tiles, rows, 320)
        got = (t.float().sum(1).double(), (t.float() ** 2).sum(1).double())
        assert bool(judge(got[0], got[1], ref, rows, False).all())
        valid = (torch.arange(tiles * rows) < 300).reshape(tiles, rows, 1).expand_as(t)
        e = t.permute(1, 0, 2)                                # (rows, tiles, N): one probe per stored element
        keep = valid.permute(1, 0, 2)
        big = torch.full_like(e, 1e9)                         # (rows past M are no probes: made unmissable)
        probe("dropped element", ref, got, rows, torch.where(keep, -e, big), torch.where(keep, -e * e, big), keep)
        probe("doubled element", ref, got, rows, torch.where(keep, e, big), torch.where(keep, e * e, big), keep)
        shifted = gn_reference(torch.roll(v, -1, 0), rows)    # tile t holds rows t * rows + 1 .. (t + 1) * rows
        probe("row-tile boundary + 1", ref, got, rows, shifted[0] - ref[0], shifted[1] - ref[1])
        swapped = [r.reshape(tiles, 160, 2).flip(2).reshape(tiles, 320) for r in ref[:2]]
        probe("two columns swapped", ref, got, rows, swapped[0] - ref[0], swapped[1] - ref[1])
    for bn in (128, 160):
        ref = ln_reference(v, bn)
        tiles = ref[0].shape[1]
        pad = torch.zeros(300, tiles * bn, dtype=torch.float64)
        pad[:, :320] = v
        t = pad.reshape(300, tiles, bn)
        got = (t.float().sum(2).double(), (t.float() ** 2).sum(2).double())
        assert bool(judge(got[0], got[1], ref, bn, False).all())
        valid = (torch.arange(tiles * bn) < 320).reshape(1, tiles, bn).expand_as(t)
        e = t.permute(2, 0, 1)
        keep = valid.permute(2, 0, 1)
        big = torch.full_like(e, 1e9)
        probe("dropped element (row partial)", ref, got, bn, torch.where(keep, -e, big), torch.where(keep, -e * e, big), keep)
        probe("doubled element (row partial)", ref, got, bn, torch.where(keep, e, big), torch.where(keep, e * e, big), keep)
        shifted = ln_reference(torch.roll(v, -1, 1), bn)
        probe("column seam + 1", ref, got, bn, shifted[0] - ref[0], shifted[1] - ref[1])
    assert math.isfinite(float(v.abs().max()))
