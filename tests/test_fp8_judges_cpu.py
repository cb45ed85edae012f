"""No GPU: the judges of tests/test_fp8_paths_gpu.py have teeth, and its reference does not rest on torch's float8 cast alone.

An f32 emulation stands in for the kernels: the operands are dequantised from their e4m3 / E8M0 BYTES, multiplied and summed in f32 one
32-element block at a time, last block first (another order than any kernel's), the epilogue is added in f32 and the result is rounded
once to the output type.  The judges must accept that, and must reject the same emulation after each of these changes to what it reads:
  * one operand element moved by one e4m3 step;
  * one scale byte moved by one;
  * two 16-byte chunks of one operand row swapped;
  * a bias_bn row taken from the neighbouring sample;
and the partial judge must reject sums that lost or doubled one pixel.  On integer-exact data the judge is an equality, so every output the
change reaches must be flagged (a quarter-integer change can vanish in the rounding of a large bf16 value: those are counted out).  On
random data, judged on the GEMM's f32 output, a change below twice the bound cannot be told from rounding and is counted out as well;
the share of such probes is asserted to be small, as in test_judge_rejects_wrong_partials.
mx_quant_int, the integer-arithmetic restatement of the OCP MX conversion, is compared with mx_quant_ref over every finite bf16 and fp16
pattern (each seen under 48 different block maxima) and over the edge blocks."""
import pytest
import torch

from test_fp8_gpu import mx_quant_ref
from test_fp8_paths_gpu import (ACT_NONE, F64, ConvProblem, bits_to_half, e4m3_value, edge_blocks, gemm_operands, im2col, mx_dequant,
                                mx_quant_int, partials_ok, pattern_blocks, product_ok, product_reference, quant_reference, same_bytes)
from test_gemm_emit_gpu import bounds

pytestmark = []          # (the module imported above is a GPU module; nothing here needs one)
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]


# ---- the reference's own foundation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_integer_restatement_matches_mx_quant_ref_on_every_pattern(fmt):
    n_seen = 0
    for blocks in [edge_blocks(fmt)] + [pattern_blocks(fmt, s) for s in range(0, 16, 5)] + [pattern_blocks(fmt, s).flip(1) for s in (2, 9)]:
        x = bits_to_half(blocks, fmt)
        q_ref, sc_ref, deq = mx_quant_ref(x.float())
        q, sc = mx_quant_int(blocks, fmt, 0)
        assert torch.equal(sc, sc_ref), "%d scale bytes differ" % int((sc != sc_ref).sum())
        bad = ~same_bytes(q, q_ref)
        assert not bool(bad.any()), "%d bytes differ; first: input bits 0x%04x -> 0x%02x, mx_quant_ref 0x%02x" % (
            int(bad.sum()), int(blocks[bad][0]), int(q[bad][0]), int(q_ref[bad][0]))
        assert torch.equal(mx_dequant(q_ref, sc_ref), deq.double()), "the dequantised values differ"
        n_seen += blocks.numel()
    assert n_seen > 6 * 63000
    # every finite pattern is there, and the planted maxima reach the saturating significands at the largest exponent
    pats = pattern_blocks(fmt, 0)
    assert len(set(pats[:, 1:].flatten().tolist())) == (65280 if fmt == "bf16" else 63488)
    assert int(pats[:, 0].max() & 0x7fff) == (0x7f7f if fmt == "bf16" else 0x7bff)


def test_e4m3_value_matches_the_float8_type():
    b = torch.tensor([v for v in range(256) if v & 0x7f != 0x7f], dtype=torch.uint8)
    assert torch.equal(e4m3_value(b), b.view(torch.float8_e4m3fn).double())


def test_edge_bytes_written_out():
    """the conversions the issue lists, as values: 17 -> 16 and 19 -> 20 at spacing 2, 2^-10 units -> 0, 1.5 2^-10 -> 2^-9, (448, 512) -> 448"""
    for fmt in ("bf16", "fp16"):
        q, sc = mx_quant_int(edge_blocks(fmt), fmt, 0)
        d = mx_dequant(q, sc)
        assert d[0, :5].tolist() == [16.0, 20.0, 28.0, -16.0, -20.0]
        assert d[1, :5].tolist() == [1.0, 0.0, 2.0 ** -17, 2.0 ** -16, 2.0 ** -17]
        assert q[2, :4].tolist() == [0x7e, 0x7e, 0x7e, 0xfe] and d[2, 0] == 1.75
        assert sc[-1, 0] == 0 and sc[-2, 0] == 0 and bool((d[-2:] == 0).all())


# ---- an f32 emulation of the kernels, from the bytes ---------------------------------------------------------------------------------
def emulate(Ad, Wd, terms, out_dtype):
    """f32 product of dequantised operands (f64 in, exactly representable in f32), 32 columns at a time from the last block to the first,
    then the epilogue terms in f32, then one rounding to out_dtype -> f64"""
    A, W = Ad.float(), Wd.float()
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
    for k0 in reversed(range(0, A.shape[1], 32)):
        acc = acc + A[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
    for t in terms:
        acc = acc + t.float()
    return acc.to(out_dtype).to(F64)


def mutations(q, sc, row):
    """(name, q', sc') for one operand given as bytes (rows, K) / (rows, K / 32): each change hits `row` only"""
    K = q.shape[1]
    out = []
    # the largest element of the row that can still take a step up (a step of a small element is below what rounding may do to the sum)
    v = mx_dequant(q[row:row + 1], sc[row:row + 1])[0].abs()
    k = int(torch.where((q[row] & 0x7f) < 0x7e, v, torch.zeros_like(v)).argmax())
    q1 = q.clone()
    q1[row, k] += 1
    out.append(("one e4m3 step at k = %d" % k, q1, sc))
    kb = k // 32
    s1 = sc.clone()
    s1[row, kb] += 1
    out.append(("scale byte + 1 in block %d" % kb, q, s1))
    c0 = k // 16
    c1 = (c0 + 3) % (K // 16)
    q2 = q.clone()
    q2[row, 16 * c0:16 * c0 + 16], q2[row, 16 * c1:16 * c1 + 16] = q[row, 16 * c1:16 * c1 + 16], q[row, 16 * c0:16 * c0 + 16]
    out.append(("16-byte chunks %d and %d swapped" % (c0, c1), q2, sc))
    return out


def must_reject(what, ok, reached, visible, min_share):
    """ok: the judge's mask under a change; reached: the outputs the change moves; visible: those it moves by more than rounding can"""
    assert bool(ok[~reached].all()), what + ": an output the change does not reach was rejected"
    share = float(visible[reached].double().mean())
    assert share >= min_share, "%s: only %.1f %% of the outputs it reaches can show it" % (what, 100 * share)
    assert not bool((ok & visible).any()), "%s: %d wrong outputs accepted" % (what, int((ok & visible).sum()))


@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_judge_accepts_another_order_and_rejects_wrong_operands(dt):
    """random data, f32 output (the judge's sharpest form: u = 2^-23), bias and residual; changes to A and to W"""
    M, N, K = 129, 68, 256
    g = torch.Generator().manual_seed(8)
    A, W = gemm_operands(M, N, K, "rand", dt, 5)
    bias = torch.randn(N, generator=g).double()
    R = torch.randn(M, N, generator=g).to(dt).double()
    aq, asc = quant_reference(A, 0)
    wq, wsc = quant_reference(W, 0)
    terms = [bias[None, :], R]
    ref, E = product_reference(mx_dequant(aq, asc), mx_dequant(wq, wsc), K, terms, ACT_NONE)
    good = emulate(mx_dequant(aq, asc), mx_dequant(wq, wsc), terms, torch.float32)
    assert bool(product_ok(good, ref, E, torch.float32, False).all()), "the judge rejects an f32 sum in another order"
    bound = 2.0 ** -23 * ref.abs() + (1 + 2.0 ** -23) * E
    for side in ("A", "W"):
        for row in (0, 67):
            for name, q1, s1 in mutations(aq if side == "A" else wq, asc if side == "A" else wsc, row):
                if side == "A":
                    wrong = emulate(mx_dequant(q1, s1), mx_dequant(wq, wsc), terms, torch.float32)
                else:
                    wrong = emulate(mx_dequant(aq, asc), mx_dequant(q1, s1), terms, torch.float32)
                reached = torch.zeros(M, N, dtype=torch.bool)
                if side == "A":
                    reached[row] = True
                else:
                    reached[:, row] = True
                visible = reached & ((wrong - good).abs() > 2 * bound)
                must_reject("%s row %d, %s" % (side, row, name), product_ok(wrong, ref, E, torch.float32, False), reached, visible, 0.8)


def conv_from_bytes(pr, xq, xs, wd, bias_bn=None):
    """the emulated conv of a ConvProblem from activation bytes (P, Cp) / (P, Cp / 32) and dequantised weights (Np, 9 Cin)"""
    B, H, W, Cin, Cout = pr.shape
    xd = mx_dequant(xq, xs)[:, :Cin].reshape(B, H, W, Cin)
    bn = pr.bias_bn if bias_bn is None else bias_bn
    b = torch.zeros(pr.Np, dtype=F64)
    b[:Cout] = pr.bias.double()
    terms = [b[None, :], bn.double()[torch.arange(pr.M) // (pr.Ho * pr.Wo), :pr.Np]]
    return emulate(im2col(xd, "UP2" if pr.up2 else "S1"), wd, terms, pr.dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("data", ["int", "rand"])
def test_conv_judges_accept_another_order_and_reject_wrong_operands(dt, data):
    """(2, 16, 16, 64, 128) with bias and per-sample bias rows: the product judge (an equality on integer data) and the partial judge"""
    pr = ConvProblem((2, 16, 16, 64, 128), False, data, {"bias", "bias_bn"}, dt)
    xq, xs, _, _ = pr.expected_bytes("cpu")
    ref, E = pr.reference("cpu")
    good = conv_from_bytes(pr, xq, xs, pr.wd)
    assert bool(product_ok(good, ref, E, dt, pr.integer).all()), "the product judge rejects an f32 sum in another order"
    u = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    bound = torch.zeros_like(ref) if pr.integer else u * ref.abs() + (1 + u) * E
    g = torch.Generator().manual_seed(3)
    # ---- operand changes: integer data only (a 16-bit output hides one e4m3 step of random data inside its own rounding)
    if pr.integer:
        live = ((xq[:, :64] & 0x7f) > 0).any(dim=1).nonzero().flatten()
        for pix in (int(live[0]), int(live[len(live) // 2])):
            for name, q1, s1 in mutations(xq[:, :64], xs[:, :2], pix):
                q2, s2 = xq.clone(), xs.clone()
                q2[:, :64], s2[:, :2] = q1, s1
                wrong = conv_from_bytes(pr, q2, s2, pr.wd)
                exact_wrong = product_reference(im2col(mx_dequant(q2, s2)[:, :64].reshape(2, 16, 16, 64), "S1"), pr.wd, 576, [ref - (im2col(pr.xd, "S1") @ pr.wd.t())])[0]
                reached = exact_wrong != ref
                assert bool(reached.any()), name + ": the change reaches no output (sparse weights): pick another pixel"
                visible = reached & (wrong != good)
                must_reject("pixel %d, %s" % (pix, name), product_ok(wrong, ref, E, dt, True), reached, visible, 0.5)
    # ---- a bias_bn row from the neighbouring sample
    wrong = conv_from_bytes(pr, xq, xs, pr.wd, bias_bn=pr.bias_bn.flip(0))
    reached = (pr.bias_bn.flip(0) != pr.bias_bn)[torch.arange(pr.M) // 256, :pr.Np]
    visible = reached & ((wrong - good).abs() > 2 * bound) & (wrong != good)
    must_reject("bias_bn of the other sample", product_ok(wrong, ref, E, dt, pr.integer), reached, visible, 0.5 if pr.integer else 0.9)
    # ---- partial sums of the stored values: accepted in f32, rejected with one pixel lost or doubled
    blk = good.reshape(2, 256, pr.Np)
    s, q = blk.float().sum(1).double(), (blk.float() ** 2).sum(1).double()
    ok, sref = partials_ok(s, q, good, (2, 16, 16), pr.integer)
    assert bool(ok.all()), "the partial judge rejects f32 sums"
    bs, bq = (torch.zeros_like(s), torch.zeros_like(q)) if pr.integer else bounds(sref, 256)
    for j in (0, 63, 64, 255):
        v = blk[:, j, :]
        for sign, name in ((-1, "lost"), (1, "doubled")):
            ok, _ = partials_ok(s + sign * v, q + sign * v * v, good, (2, 16, 16), pr.integer)
            skip = (v.abs() <= 2 * bs) & (v * v <= 2 * bq) if not pr.integer else v == 0
            if not pr.integer:
                assert float(skip.double().mean()) < 0.02, "pixel %d %s: too many probes below the bound" % (j, name)
            assert not bool((ok & ~skip).any()), "pixel %d %s: %d wrong partials accepted" % (j, name, int((ok & ~skip).sum()))
