"""The MX-fp8 conv, GEMM and quantisers (csrc/conv_halo_fp8.hip, csrc/gemm_fp8.hip) on every kernel path, against fp64, element by
element.  A sibling of tests/test_gemm_epilogue_gpu.py / test_gemm_emit_gpu.py for the path behind `--dtype fp8`.

Hooks: svg_op_conv3x3_mx_ex (everything conv3x3_fp8 takes: bias, the per-sample bias_bn rows, residual, gn_part; reads back the
quantised activations and the packed weights; reports {column tile, tn_major, workgroups} as launched), svg_op_gemm_fp8_ex (ldc, ldr,
reports the column tile), svg_op_quant_mx, svg_op_quant_act_mx.  Every case asserts the reported path first; every test runs on the
bf16 build and on the fp16 build (_f16 twins).

Judges, from the arithmetic alone (one measured constant, F below):
  * quantisers, bit for bit (up to the sign of zero): e4m3 bytes and E8M0 scale bytes against mx_quant_ref (tests/test_fp8_gpu.py) AND
    against mx_quant_int below, an integer-only restatement of the OCP MX v1.0 conversion that does not touch torch.float8_e4m3fn.
    The packed conv weights are read through their documented layouts, e4m3 [Npad][tap][Cp] and E8M0 [tap][Cp/128][Npad][4].
    Pinned: an all-zero block gets scale byte 0 from quant_mx and 127 from quant_act_mx / pack_conv3x3_mx; padding channels and padding
    rows are zero bytes with scale byte 127.
  * product, per element: reference in fp64 from the operands dequantised out of those (just proven) bytes, epilogue as documented
    (+ bias + bias_bn[sample] + residual, activation on the GEMM), rounded once to the output type.
      integer-exact data (small integers, power-of-two factors per block, sparse weights, quarter-integer biases that differ per
      sample): every product and partial sum is an exact f32, the fp64 magnitude is asserted below 2^22 (quarter-integers in an f32;
      below 2^15 for fp16 outputs), the output must EQUAL the reference;
      random data: |out - ref| <= u |ref| + (1 + u) E, u the output's unit roundoff, E = F K 2^-23 (|Ad| |Wd|^T) + 2^-21 (sum of the
      magnitudes of the epilogue terms), E times 1.13 plus the activation's own error behind SiLU / GELU — the form of the 16-bit
      judge; (1 + u) because the output rounding applies to the computed value.  e4m3 x e4m3 products are exact in f32.
      F = 2 (MFMA_F) is the one measured constant, and it is a property of the instruction, not of these kernels: with F = 1 (a
      sequential f32 sum's worst case) gemm_fp8 missed the bound on f32 outputs at K = 128 — one MFMA per output — by up to 1.17, in
      bf16 and fp16 storage alike, while every integer-exact and one-hot case passed.  tools/probe/probe_mx_acc.hip issues one
      v_mfma_scale_f32_16x16x128_f8f6f4 per wave on its own and compares with the exact sum in double: over 3 x 524 288 dot products of
      MX-quantised N(0,1) operands (with and without an accumulator, with row scales 2^-6 .. 2^6) the error reaches 1.479 times
      128 2^-23 (|c| + sum |a b|) (profiles/r21_probe_mx_acc.txt; mean 0.09; zero on integer data); rounded up to the next power of
      two.  A chain of K / 128 such steps stays within F K 2^-23 (|Ad| |Wd|^T), since |c| never exceeds the sum of the magnitudes before it.
      (Uniformly random e4m3 BYTES, whose products span 2^-18 .. 2^17 inside one block, reach 12.4 there: no test here feeds such data.)
  * emitted GroupNorm sums: the judge of tests/test_gemm_emit_gpu.py on the stored out, read back: equal to the fp64 sums on exact and
    one-hot data, the (n - 1) 2^-24 any-order bounds with n = 256 on random data; the buffer sits between NaN guards and exactly
    blocks x Npad x 2 slots end up finite.
  * one-hot probes: one power of two per (16 x 16 pixel block, column), at the first and last pixel of the block and both sides of every
    16-pixel boundary (every image row of the block: the 4-row wave seams are among them), the hot input channel and the hot value moving
    with the probe; on the GEMM one hot K element per row that walks through every 16-byte chunk and scale block of K.
  * out starts as NaN inside NaN guards: the ldc > N gaps and the rows past M of the GEMM must still be NaN, the guards intact.
  * every launch is repeated into re-filled buffers: bit-identical output and partials.
The distance from the UNQUANTISED product (FP8_TOL) stays in tests/test_fp8_gpu.py."""
import ctypes as C
import math
import zlib

import pytest
import torch

from sd_video_gen_amd import _lib
from test_fp8_gpu import mx_quant_ref
from test_gemm_emit_gpu import assert_exactly_summable, bounds, gn_reference, judge
from test_gemm_epilogue_gpu import (ACT_GELU, ACT_NONE, ACT_SILU, GELU_ABS_ERR, HALF, _gelu_exact, _knobs, _storage,  # noqa: F401
                                    im2col, onehot_len, onehot_rows, onehot_val)
from test_norm_paths_gpu import guarded, guards_intact

pytestmark = pytest.mark.gpu
F64 = torch.float64
MFMA_F = 2.0                              # see the module docstring: measured on the instruction alone (1.479), next power of two
HALO_MIN = {"SVG_HALO_MIN": "1"}          # conv_halo_fp8 takes a conv from 192 workgroups on; the kernel does not depend on that count


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- OCP MX conversion in integer arithmetic (pure torch integers: no float8 type, no floating-point rounding) -------------------------
FORMATS = {"bf16": (8, 7, torch.bfloat16), "fp16": (5, 10, torch.float16)}       # exponent bits, mantissa bits, torch type


def bits_to_half(bits, fmt):
    """int64 16-bit patterns -> tensor of the storage type with those bits"""
    b = bits.to(torch.int64)
    return (b - 65536 * (b >= 32768)).to(torch.int16).view(FORMATS[fmt][2])


def half_to_bits(t):
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xffff


def _decompose(bits, fmt):
    """finite 16-bit patterns -> (sign, m, e) with |x| = m 2^e exactly, m < 2^(mantissa bits + 1)"""
    eb, mb, _ = FORMATS[fmt]
    b = bits.to(torch.int64)
    sign = b >> 15
    ef = (b >> mb) & ((1 << eb) - 1)
    mf = b & ((1 << mb) - 1)
    assert bool((ef != (1 << eb) - 1).all()), "finite inputs only"
    bias = (1 << (eb - 1)) - 1
    m = torch.where(ef == 0, mf, mf | (1 << mb))
    e = torch.where(ef == 0, torch.full_like(ef, 1 - bias - mb), ef - bias - mb)
    return sign, m, e


def _msb(m):
    """floor(log2 m) of 0 < m < 2^12 (0 for m = 0)"""
    r = torch.zeros_like(m)
    for i in range(1, 12):
        r = r + (m >= (1 << i)).to(m.dtype)
    return r


def mx_quant_int(bits, fmt, zero_scale=0):
    """bits (rows, K) int64 finite 16-bit patterns of `fmt` -> (e4m3 bytes (rows, K) uint8, E8M0 bytes (rows, K / 32) uint8): shared exponent
    floor(log2 amax) - 8 clamped to [-127, 126], elements x 2^-shared rounded to nearest even onto the e4m3 grid (3 mantissa bits, minimum
    normal 2^-6, subnormal spacing 2^-9), saturated at 448 = 0x7e.  zero_scale: the scale byte of an all-zero block."""
    rows, K = bits.shape
    sign, m, e = _decompose(bits, fmt)
    NEG = -100000
    fl = torch.where(m > 0, e + _msb(m), torch.full_like(e, NEG))
    flmax = fl.reshape(rows, K // 32, 32).amax(dim=-1)
    E = (flmax - 8).clamp(-127, 126)
    scale = torch.where(flmax == NEG, torch.full_like(E, zero_scale), E + 127)
    s = e - E.repeat_interleave(32, dim=1)                     # x 2^-shared = m 2^s
    flv = s + _msb(m)
    qe = torch.clamp(flv, min=-6) - 3                          # the e4m3 grid spacing at this magnitude is 2^qe
    r = qe - s                                                 # m 2^s = (m 2^-r) 2^qe
    left = torch.bitwise_left_shift(m, (-r).clamp(0, 8))
    rr = r.clamp(1, 40)
    n0 = torch.bitwise_right_shift(m, rr)
    rem = m - torch.bitwise_left_shift(n0, rr)
    half = torch.bitwise_left_shift(torch.ones_like(m), rr - 1)
    up = (rem > half) | ((rem == half) & ((n0 & 1) == 1))
    n = torch.where(r <= 0, left, n0 + up.to(m.dtype))
    n = torch.where(m > 0, n, torch.zeros_like(n))
    carry = n == 16
    n = torch.where(carry, torch.full_like(n, 8), n)
    qe = qe + carry.to(qe.dtype)
    mag = torch.where(n < 8, n, ((qe + 10) << 3) | (n - 8))
    mag = mag.clamp(max=0x7e)
    return (mag | (sign << 7)).to(torch.uint8), scale.to(torch.uint8)


def e4m3_value(q):
    """e4m3 bytes -> their values in f64, from the bit fields (0x7f / 0xff, NaN, do not occur)"""
    b = q.to(torch.int64)
    ef, mf = (b >> 3) & 15, b & 7
    mag = torch.where(ef == 0, mf.to(F64) * 2.0 ** -9, (8 + mf).to(F64) * torch.exp2((ef - 10).to(F64)))
    return torch.where((b >> 7) == 1, -mag, mag)


def mx_dequant(q, sc):
    """(rows, K) e4m3 bytes, (rows, K / 32) E8M0 bytes -> f64"""
    return e4m3_value(q) * torch.exp2(sc.to(F64) - 127).repeat_interleave(32, dim=1)


def same_bytes(a, b):
    """e4m3 bytes equal up to the sign of zero"""
    return (a == b) | (((a & 0x7f) == 0) & ((b & 0x7f) == 0))


def quant_reference(x, zero_scale):
    """x (rows, K) of a 16-bit storage type -> (q, sc) of mx_quant_ref with the scale byte of all-zero blocks set to zero_scale; asserted equal
    to the integer restatement"""
    fmt = "bf16" if x.dtype == torch.bfloat16 else "fp16"
    q, sc, _ = mx_quant_ref(x.float())
    zero = (x.float().reshape(x.shape[0], -1, 32) == 0).all(dim=-1)
    assert bool((sc[zero] == 0).all())
    sc = torch.where(zero, torch.full_like(sc, zero_scale), sc)
    qi, si = mx_quant_int(half_to_bits(x), fmt, zero_scale)
    assert torch.equal(sc, si) and bool(same_bytes(q, qi).all()), "mx_quant_ref and the integer restatement disagree"
    return q, sc


# ---- product judge (pure torch, any device: tests/test_fp8_judges_cpu.py runs it without a GPU) --------------------------------------
def product_reference(Ad, Wd, K, terms, act=ACT_NONE):
    """Ad (M, K') f64, Wd (N, K') f64 dequantised operands, K accumulated products per output, terms: f64 epilogue terms broadcastable to
    (M, N) -> (ref, E) of the module docstring"""
    acc = Ad @ Wd.t()
    E = MFMA_F * K * 2.0 ** -23 * (Ad.abs() @ Wd.abs().t())
    pre, mag = acc, acc.abs()
    for t in terms:
        pre = pre + t
        mag = mag + t.abs()
    E = E + 2.0 ** -21 * mag
    if act == ACT_SILU:
        ref = pre * torch.sigmoid(pre)
        return ref, 1.13 * E + (pre.abs() + 4) * 2.0 ** -23 * ref.abs()
    if act == ACT_GELU:
        ref = _gelu_exact(pre)
        return ref, 1.13 * E + GELU_ABS_ERR + 2.0 ** -24 * ref.abs()
    return pre, E


def product_ok(out, ref, E, out_dtype, integer):
    """mask of the elements of out (f64, read back) that pass"""
    if integer:
        return out == ref.float().to(out_dtype).to(F64)
    u = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}[out_dtype]
    return (out - ref).abs() <= u * ref.abs() + (1 + u) * E


def assert_product(what, out, ref, E, out_dtype, integer):
    if integer:
        lim = 2.0 ** 15 if out_dtype == torch.float16 else 2.0 ** 22
        assert float(ref.abs().max()) < lim, "%s: the integer data leaves |ref| = %g, not exactly representable" % (what, float(ref.abs().max()))
    else:
        u = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}[out_dtype]
        ratio = ((out - ref).abs() / (u * ref.abs() + (1 + u) * E).clamp(min=1e-300)).max()
        print("[fp8 judge] %s: worst |err| / bound = %.3f" % (what, float(ratio)))
    ok = product_ok(out, ref, E, out_dtype, integer)
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        raise AssertionError("%s: %d of %d elements %s; first at %s: %.9g vs %.9g (E %.3g)" % (
            what, int((~ok).sum()), ok.numel(), "differ from the exact result" if integer else "outside the bound", i, float(out[i]), float(ref[i]),
            float(E[i])))


def partials_ok(got_s, got_q, stored, blocks, integer):
    """the judge of tests/test_gemm_emit_gpu.py on the stored output (M, N) f64 of a conv over `blocks` = (B, Ho, Wo)"""
    ref = gn_reference(stored, 256, blocks)
    if integer:
        assert_exactly_summable(ref)
    return judge(got_s, got_q, ref, 256, integer), ref


# ---- conv problems ---------------------------------------------------------------------------------------------------------------------
def hot_channel(k, Cin):
    """input channel of one-hot probe k: walks through the 16-byte chunks and 32-channel scale blocks (37 is coprime with every Cin here)"""
    return (37 * k) % Cin


class ConvProblem:
    """one conv: operands on the CPU (seeded there, so that they do not depend on the device), the expected bytes and the fp64 reference on `dev`.
    shape (B, H, W, Cin, Cout) of the INPUT image, up2: nearest-2x upsample in front; data 'int' | 'rand' | 'onehot';
    feats: subset of {'bias', 'bias_bn', 'res'}"""

    def __init__(self, shape, up2, data, feats, dt):
        self.shape, self.up2, self.data, self.feats, self.dt = shape, up2, data, feats, dt
        B, H, W, Cin, Cout = shape
        self.Ho, self.Wo = (2 * H, 2 * W) if up2 else (H, W)
        self.Np, self.Cp = (Cout + 3) // 4 * 4, (Cin + 127) // 128 * 128
        self.M, self.P = B * self.Ho * self.Wo, B * H * W
        self.integer = data != "rand"
        g = torch.Generator().manual_seed(zlib.crc32(repr((shape, up2, data, sorted(feats))).encode()))
        Np, Ho, Wo = self.Np, self.Ho, self.Wo

        def ints(shp, lo, hi):
            return torch.randint(lo, hi + 1, shp, generator=g).to(F64)

        def keep(shp, p):
            return (torch.rand(shp, generator=g) < p).to(F64)

        if data == "int":
            # sparse on both sides: about eight non-zero products per output, so that the stored values stay small enough for the GroupNorm
            # sums of 256 of them (and of their squares) to be exact in f32 (assert_exactly_summable)
            x = ints((B, H, W, Cin), -4, 4) * keep((B, H, W, Cin), min(1.0, 8.0 / (9 * Cin * 0.06)))
            w = ints((Cout, Cin, 3, 3), -4, 4) * keep((Cout, Cin, 3, 3), 0.06)
            x[..., :32] *= 0.5                                  # different shared exponents along the channels, per pixel row and per tap
            x[:, ::3, :, 32:64] *= 2
            w[::5, 64:96] *= 0.25
            w[:, :, 1, 1] *= 2
        elif data == "rand":
            x = torch.randn((B, H, W, Cin), generator=g, dtype=F64)
            w = torch.randn((Cout, Cin, 3, 3), generator=g, dtype=F64) / math.sqrt(9 * Cin)
        else:
            # centre tap only: out[pixel][n] = x[source pixel][c] w[n][c].  Row tile of an output pixel: its 16 x 16 block; with the upsample
            # in front the probes sit on the 8 x 8 source block (each lights the 2 x 2 output pixels it is copied to)
            side = 8 if up2 else 16
            T = side * side
            L = onehot_len(T)
            p = torch.arange(self.P)
            py, px = (p % (H * W)) // W, p % W
            tile_of = ((p // (H * W)) * (H // side) + py // side) * (W // side) + px // side
            pos_of = (py % side) * side + px % side
            Hm = onehot_rows(tile_of, pos_of, torch.full((self.P,), T), T, L)
            x = torch.zeros(self.P, Cin, dtype=F64)
            w = torch.zeros(Cout, Cin, 3, 3, dtype=F64)
            n = torch.arange(Cout)
            for k in range(L):
                x[:, hot_channel(k, Cin)] = Hm[:, k] * 2.0 ** (k % 3 - 1)
            w[n, torch.tensor([hot_channel(int(v) % L, Cin) for v in n]), 1, 1] = onehot_val(n)
            x = x.reshape(B, H, W, Cin)
        self.x = x.to(dt)
        self.w = w.float()
        self.bias = self.bias_bn = self.res = None
        self.ld = Np + 12
        if "bias" in feats:
            self.bias = (ints((Cout,), -8, 8) * 0.25 if self.integer else torch.randn((Cout,), generator=g, dtype=F64)).float()
        if "bias_bn" in feats:
            assert B >= 2
            bn = ints((B, self.ld), -8, 8) * 0.25 if self.integer else torch.randn((B, self.ld), generator=g, dtype=F64)
            bn[:, 0] = torch.arange(B, dtype=F64) * 0.25        # (rows that differ per sample, whatever was drawn)
            self.bias_bn = bn.float()
        if "res" in feats:
            self.res = (ints((B, Ho, Wo, Np), -4, 4) if self.integer else torch.randn((B, Ho, Wo, Np), generator=g, dtype=F64)).to(dt)

    def expected_bytes(self, dev):
        """what the quantisers must leave: activations (P, Cp) / (P, Cp / 32), weights [Np][9][Cp] / [9][Cp / 128][Np][4]; zero blocks and
        padding carry scale byte 127.  Also keeps the dequantised operands for the product."""
        B, H, W, Cin, Cout = self.shape
        Np, Cp = self.Np, self.Cp
        q, sc = quant_reference(self.x.reshape(self.P, Cin).to(dev), 127)
        self.xd = mx_dequant(q, sc).reshape(B, H, W, Cin)
        xq = torch.zeros(self.P, Cp, dtype=torch.uint8, device=dev)
        xs = torch.full((self.P, Cp // 32), 127, dtype=torch.uint8, device=dev)
        xq[:, :Cin], xs[:, :Cin // 32] = q, sc
        wt = self.w.to(dev).permute(0, 2, 3, 1).reshape(Cout * 9, Cin)        # blocks of 32 input channels per (output channel, tap)
        wq, wsc, _ = mx_quant_ref(wt)
        wsc = torch.where((wt.reshape(Cout * 9, -1, 32) == 0).all(dim=-1), torch.full_like(wsc, 127), wsc)
        self.wd = torch.zeros(Np, 9 * Cin, dtype=F64, device=dev)
        self.wd[:Cout] = mx_dequant(wq, wsc).reshape(Cout, 9 * Cin)
        w8 = torch.zeros(Np, 9, Cp, dtype=torch.uint8, device=dev)
        w8[:Cout, :, :Cin] = wq.reshape(Cout, 9, Cin)
        s_ntb = torch.full((Np, 9, Cp // 32), 127, dtype=torch.uint8, device=dev)       # [n][tap][block of 32 channels]
        s_ntb[:Cout, :, :Cin // 32] = wsc.reshape(Cout, 9, Cin // 32)
        w8s = s_ntb.reshape(Np, 9, Cp // 128, 4).permute(1, 2, 0, 3).contiguous()       # [tap][chunk][n][4]
        return xq, xs, w8, w8s

    def reference(self, dev):
        """(ref, E) (M, Np) f64 from the dequantised operands of expected_bytes()"""
        Ad = im2col(self.xd, "UP2" if self.up2 else "S1")
        terms = []
        if self.bias is not None:
            b = torch.zeros(self.Np, dtype=F64, device=dev)
            b[:self.shape[4]] = self.bias.to(dev).to(F64)
            terms.append(b[None, :])
        if self.bias_bn is not None:
            terms.append(self.bias_bn.to(dev).to(F64)[torch.arange(self.M, device=dev) // (self.Ho * self.Wo), :self.Np])
        if self.res is not None:
            terms.append(self.res.to(dev).to(F64).reshape(self.M, self.Np))
        return product_reference(Ad, self.wd, 9 * self.shape[3], terms)


def conv_ex(ctx, **f):
    """svg_op_conv3x3_mx_ex(_f16) on a descriptor of the given fields (tensors by pointer) -> (status, path)"""
    d = _lib.ConvMxDesc()
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    path = (C.c_int * 3)(-1, -1, -1)
    rc = getattr(ctx.lib, "svg_op_conv3x3_mx_ex" + HALF.suffix)(ctx.h, C.byref(d), path, stream())
    return rc, tuple(path)


def run_conv(ctx, path, shape, up2, data, feats):
    pr = ConvProblem(shape, up2, data, feats, HALF.dtype)
    B, H, W, Cin, Cout = shape
    what = "conv %s%s %s %s %s" % (shape, " up2" if up2 else "", data, "+".join(sorted(feats)), HALF.suffix or "bf16")
    blocks = pr.M // 256
    ins = {k: guarded(t) for k, t in (("x", pr.x), ("w_oihw", pr.w), ("bias", pr.bias), ("bias_bn", pr.bias_bn), ("residual", pr.res)) if t is not None}
    outs = {"out": guarded(torch.full((pr.M, pr.Np), float("nan"), dtype=HALF.dtype)),
            "gn_part": guarded(torch.full((blocks, pr.Np, 2), float("nan"), dtype=torch.float32))}
    for k, shp in (("q_out", (pr.P, pr.Cp)), ("s_out", (pr.P, pr.Cp // 32)), ("w8_out", (pr.Np, 9, pr.Cp)), ("w8s_out", (9, pr.Cp // 128, pr.Np, 4))):
        outs[k] = guarded(torch.full(shp, 0xA5, dtype=torch.uint8))
    desc = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=3 if up2 else 0, bias_bn_ld=pr.ld if pr.bias_bn is not None else 0)
    desc.update({k: v[1] for k, v in ins.items()})
    desc.update({k: v[1] for k, v in outs.items()})

    def launch():
        with _knobs(HALO_MIN):
            rc, got = conv_ex(ctx, **desc)
        ctx.check(rc, "conv3x3_mx_ex")
        torch.cuda.synchronize()
        return got

    got = launch()
    assert got == tuple(path), "%s: launched %s, expected %s" % (what, got, tuple(path))
    for k, (buf, _) in list(ins.items()) + list(outs.items()):
        guards_intact(buf, what + ": " + k)
    # ---- the quantisers' bytes
    xq, xs, w8, w8s = pr.expected_bytes("cuda")
    assert torch.equal(outs["s_out"][1], xs), what + ": activation scales"
    assert bool(same_bytes(outs["q_out"][1], xq).all()), what + ": %d activation bytes differ" % int((~same_bytes(outs["q_out"][1], xq)).sum())
    assert torch.equal(outs["w8s_out"][1], w8s), what + ": %d weight scale bytes differ" % int((outs["w8s_out"][1] != w8s).sum())
    assert bool(same_bytes(outs["w8_out"][1], w8).all()), what + ": %d weight bytes differ" % int((~same_bytes(outs["w8_out"][1], w8)).sum())
    assert bool(((outs["q_out"][1][:, Cin:] == 0).all())) and bool((outs["w8_out"][1][Cout:] == 0).all()), what + ": padding bytes"
    # ---- the product
    out = outs["out"][1].to(F64)
    assert bool(out.isfinite().all()), what + ": %d output elements were never written" % int((~out.isfinite()).sum())
    ref, E = pr.reference("cuda")
    assert_product(what, out, ref, E, HALF.dtype, pr.integer)
    # ---- the emitted sums of the stored values
    part = outs["gn_part"][1].double()
    assert bool(part.isfinite().all()), what + ": %d gn_part slots were never written" % int((~part.isfinite()).sum())
    ok, sref = partials_ok(part[..., 0], part[..., 1], out, (B, pr.Ho, pr.Wo), pr.integer)
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        bs, bq = bounds(sref, 256)
        raise AssertionError("%s: %d of %d partials wrong; first at (block, n) = %s: sum %.9g vs %.9g (bound %.3g), squares %.9g vs %.9g (bound %.3g)" % (
            what, int((~ok).sum()), ok.numel(), i, float(part[i][0]), float(sref[0][i]), 0.0 if pr.integer else float(bs[i]), float(part[i][1]),
            float(sref[1][i]), 0.0 if pr.integer else float(bq[i])))
    if data == "onehot":
        hot = out if pr.bias is None and pr.res is None and pr.bias_bn is None else None
        if hot is not None:
            per = (hot != 0).reshape(B, pr.Ho // 16, 16, pr.Wo // 16, 16, pr.Np).sum(dim=(2, 4))
            assert bool((per[..., :Cout] == (4 if up2 else 1)).all()), what + ": not one probe per (block, column)"
    # ---- again, into re-filled buffers
    first = {k: outs[k][0].clone() for k in ("out", "gn_part")}
    outs["out"][1].fill_(float("nan"))
    outs["gn_part"][1].fill_(float("nan"))
    assert launch() == tuple(path)
    for k, a in first.items():
        b = outs[k][0]
        assert torch.equal(a.view(torch.int16 if k == "out" else torch.int32), b.view(torch.int16 if k == "out" else torch.int32)), "%s: the second launch left other bits in %s" % (what, k)


# (B, H, W, Cin, Cout) of the input image -> {column tile, tn_major, workgroups} read off conv_halo_fp8_bn and the tn_major rule (9 N > M)
S1_SHAPES = [
    ("128-1wg", (1, 16, 16, 64, 128), (128, 1, 1), {"bias", "res"}),              # one workgroup, half-padded chunk
    ("128-2tiles", (2, 32, 32, 128, 256), (128, 1, 16), {"bias", "bias_bn"}),     # two column tiles
    ("128-tm0", (3, 32, 32, 192, 256), (128, 0, 24), {"bias"}),                   # two chunks, the second with a 64-channel tail
    ("128-6wg", (3, 16, 16, 320, 132), (128, 1, 6), {"bias", "bias_bn"}),         # grid no multiple of 8, a 4-column last tile, three chunks
    ("128-6wg-res", (3, 16, 16, 320, 132), (128, 1, 6), {"bias", "res"}),
    ("128-npad", (2, 16, 16, 64, 130), (128, 1, 4), {"bias", "bias_bn"}),         # Cout no multiple of 4: two padding rows of weights
    ("160-1tile", (9, 64, 64, 64, 160), (160, 0, 144), {"bias", "bias_bn"}),
    ("160-2tiles", (6, 64, 64, 128, 320), (160, 0, 192), {"bias", "res"}),
    ("160-ragged", (11, 32, 32, 64, 644), (160, 0, 220), {"bias"}),               # 4 columns in the last tile
    ("160-tm1", (28, 16, 16, 64, 1280), (160, 1, 224), {"bias", "bias_bn"}),      # the UNet's 16 x 16 level: weight-heavy on <160>
]
UP_SHAPES = [
    ("up-128-1wg", (1, 8, 8, 64, 128), (128, 1, 1), {"bias"}),
    ("up-128", (2, 16, 16, 192, 256), (128, 1, 16), {"bias", "bias_bn"}),
    ("up-160", (9, 32, 32, 64, 160), (160, 0, 144), {"bias", "res"}),
]
CONV_CASES = [pytest.param(path, shape, up2, data, feats, id="%s-%s" % (tag, data))
              for up2, table in ((False, S1_SHAPES), (True, UP_SHAPES)) for tag, shape, path, feats in table for data in ("int", "rand", "onehot")]
# the bare probes: nothing but the conv, so that exactly one element per (block, column) is non-zero
CONV_CASES += [pytest.param((128, 1, 6), (3, 16, 16, 320, 132), False, "onehot", set(), id="128-6wg-bare-onehot"),
               pytest.param((160, 0, 220), (11, 32, 32, 64, 644), False, "onehot", set(), id="160-ragged-bare-onehot"),
               pytest.param((128, 1, 16), (2, 16, 16, 192, 256), True, "onehot", set(), id="up-128-bare-onehot")]


@pytest.mark.parametrize("path,shape,up2,data,feats", CONV_CASES)
def test_conv_mx_paths(ctx, path, shape, up2, data, feats):
    run_conv(ctx, path, shape, up2, data, feats)


def test_conv_mx_refused_shapes(ctx):
    """what conv_halo_fp8_supported refuses (too few workgroups without the knob, sides no multiple of 16, Cin no multiple of 64, fewer than
    128 columns) and a bad mode: an error status, nothing launched (out and the read-backs untouched, path not reported)"""
    dt = HALF.dtype
    for B, H, W, Cin, Cout, mode, knob in ((1, 16, 16, 64, 128, 0, False), (2, 24, 24, 64, 128, 0, True), (2, 16, 16, 96, 128, 0, True),
                                           (2, 16, 16, 64, 64, 0, True), (2, 16, 16, 64, 128, 1, True)):
        x = torch.ones(B, H, W, Cin, device="cuda", dtype=dt)
        w = torch.ones(Cout, Cin, 3, 3, device="cuda")
        up = 2 if mode == 3 else 1
        ob, out = guarded(torch.full((B * up * H * up * W, Cout), float("nan"), dtype=dt))
        qb, q = guarded(torch.full((B * H * W, (Cin + 127) // 128 * 128), 0xA5, dtype=torch.uint8))
        with _knobs(HALO_MIN if knob else {}):
            rc, path = conv_ex(ctx, x=x, w_oihw=w, out=out, q_out=q, B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=mode)
        torch.cuda.synchronize()
        assert rc == _lib.SVG_ERR_INVALID and path == (-1, -1, -1), (B, H, W, Cin, Cout, mode, rc, path)
        assert len(ctx.lib.svg_last_error(ctx.h)) > 0
        assert bool(ob.isnan().all()) and bool((qb == 0xA5).all()), "a refused conv wrote its outputs"


# ---- gemm_fp8 --------------------------------------------------------------------------------------------------------------------------
def gemm_fp8_ex(ctx, A, W, bias, res, Cbuf, M, N, K, act, out_f32, ldc, ldr):
    path = (C.c_int * 1)(-1)
    rc = getattr(ctx.lib, "svg_op_gemm_fp8_ex" + HALF.suffix)(
        ctx.h, A.data_ptr(), W.data_ptr(), bias.data_ptr() if bias is not None else None, res.data_ptr() if res is not None else None,
        Cbuf.data_ptr(), M, N, K, act, out_f32, ldc, ldr, path, stream())
    return rc, path[0]


def gemm_operands(M, N, K, data, dt, seed):
    """A (M, K), W (N, K) in the storage type, seeded on the CPU"""
    g = torch.Generator().manual_seed(seed)
    if data == "int":
        # the recipe of tests/test_fp8_gpu.py: integers in [-8, 8], blocks with other shared exponents along K and across rows
        A = torch.randint(-8, 9, (M, K), generator=g).to(F64)
        W = torch.randint(-8, 9, (N, K), generator=g).to(F64)
        A[:, :32] *= 0.5
        W[::3, 32:64] *= 4
    elif data == "rand":
        A = torch.randn((M, K), generator=g, dtype=F64)
        W = torch.randn((N, K), generator=g, dtype=F64) / math.sqrt(K)
    else:
        # one hot K element per row of A, walking through K (7 is coprime with K): out[m][n] = A[m][k(m)] W[n][k(m)].  W is dense in
        # powers of two that change with every 16-byte chunk and row, so neighbouring chunks and scale blocks carry other values:
        # a swapped chunk or scale lane is wrong by at least a factor of two
        m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
        km = (7 * m + 3) % K
        A = torch.zeros(M, K, dtype=F64)
        A[m, km] = 2.0 ** ((m + 2 * (km // 16)) % 5 - 2).to(F64)
        W = 2.0 ** ((3 * n[:, None] + 5 * (k[None, :] // 16)) % 11 - 5).to(F64)
    return A.to(dt), W.to(dt)


def run_gemm(ctx, bn, M, N, K, data, act, out_f32, ldc_pad, res_pad, bias):
    dt = HALF.dtype
    what = "gemm_fp8 %dx%dx%d %s act%d f32=%d ldc+%d res%s %s" % (M, N, K, data, act, out_f32, ldc_pad, res_pad, HALF.suffix or "bf16")
    integer = data != "rand"
    assert not (integer and act != ACT_NONE)
    seed = zlib.crc32(repr((M, N, K, data, act, out_f32, ldc_pad, res_pad, bias)).encode())
    A, W = gemm_operands(M, N, K, data, dt, seed)
    g = torch.Generator().manual_seed(seed + 1)
    ldc = N + ldc_pad
    ldr = 0 if res_pad is None else N + res_pad
    b = R = None
    if bias:
        b = (torch.randint(-8, 9, (N,), generator=g) * 0.25 if integer else torch.randn((N,), generator=g)).float()
    if res_pad is not None:
        R = (torch.randint(-4, 5, (M, ldr), generator=g).to(F64) if integer else torch.randn((M, ldr), generator=g, dtype=F64)).to(dt)
    out_dt = torch.float32 if out_f32 else dt
    ins = {k: guarded(t) for k, t in (("A", A), ("W", W), ("bias", b), ("res", R)) if t is not None}
    cb, Cv = guarded(torch.full(((M + 3) * ldc,), float("nan"), dtype=out_dt))           # 3 rows past M

    def launch():
        rc, got = gemm_fp8_ex(ctx, ins["A"][1], ins["W"][1], ins["bias"][1] if bias else None, ins["res"][1] if R is not None else None, Cv, M, N, K,
                              act, out_f32, ldc, ldr)
        ctx.check(rc, "gemm_fp8_ex")
        torch.cuda.synchronize()
        return got

    got = launch()
    assert got == bn, "%s: column tile %d, expected %d" % (what, got, bn)
    for k, (buf, _) in list(ins.items()) + [("C", (cb, Cv))]:
        guards_intact(buf, what + ": " + k)
    Ad = mx_dequant(*quant_reference(A.cuda(), 0))
    Wd = mx_dequant(*quant_reference(W.cuda(), 0))
    terms = []
    if bias:
        terms.append(b.cuda().to(F64)[None, :])
    if R is not None:
        terms.append(R.cuda().to(F64)[:, :N])
    ref, E = product_reference(Ad, Wd, K, terms, act)
    C2 = Cv.reshape(M + 3, ldc)
    assert_product(what, C2[:M, :N].to(F64), ref, E, out_dt, integer)
    assert bool(C2[:M, N:].isnan().all()) and bool(C2[M:].isnan().all()), what + ": written outside C's [M][ldc < %d] area" % N
    first = cb.clone()
    Cv.fill_(float("nan"))
    assert launch() == bn
    it = torch.int32 if out_f32 else torch.int16
    assert torch.equal(first.view(it), cb.view(it)), what + ": the second launch left other bits"


def _gemm_cases():
    """every (M, N, K) of the matrix twice: integer-exact without activation, random behind a rotating activation; ldc = N / N + 8, no
    residual / ldr = N / ldr = N + 16 and 16-bit / f32 output rotate with the shape so that each occurs on both instantiations and at
    every K.  Grids: cdiv(M, 128) x cdiv(N, bn) = 1 ... 9 workgroups, none of them 8."""
    out = []
    i = 0
    for M in (1, 129, 300):
        for N in (60, 64, 68, 132, 320):
            for K in (128, 256, 384):
                bn = 64 if N <= 64 else 128
                ldc_pad = 8 * (i % 2)
                res_pad = (None, 0, 16)[(i // 2) % 3]
                f32 = (i // 3) % 2
                out.append(pytest.param(bn, M, N, K, "int", ACT_NONE, f32, ldc_pad, res_pad, True, id="%dx%dx%d-int" % (M, N, K)))
                out.append(pytest.param(bn, M, N, K, "rand", i % 3, 1 - f32, 8 - ldc_pad, (16, None, 0)[(i // 2) % 3], i % 5 != 0,
                                        id="%dx%dx%d-rand-act%d" % (M, N, K, i % 3)))
                i += 1
    for M, N, K in ((300, 320, 384), (129, 64, 256), (300, 60, 128), (129, 132, 384)):
        out.append(pytest.param(64 if N <= 64 else 128, M, N, K, "onehot", ACT_NONE, 0, 8, None, False, id="%dx%dx%d-onehot" % (M, N, K)))
    return out


@pytest.mark.parametrize("bn,M,N,K,data,act,out_f32,ldc_pad,res_pad,bias", _gemm_cases())
def test_gemm_fp8_paths(ctx, bn, M, N, K, data, act, out_f32, ldc_pad, res_pad, bias):
    run_gemm(ctx, bn, M, N, K, data, act, out_f32, ldc_pad, res_pad, bias)


# ---- quantisers ------------------------------------------------------------------------------------------------------------------------
def pattern_blocks(fmt, shift):
    """(blocks, 32) int64: every finite 16-bit pattern of `fmt` (both signs) as an element of a block whose maximum is planted in slot 0.
    The patterns are sorted by magnitude, 31 to a block; the planted maximum lies `shift + block index` (mod 16) binades above the block's
    largest pattern, with a significand from a short list that includes 1.75 (448: the largest e4m3 value), the next pattern above it and
    the largest one (both saturate), capped at the largest finite value.  So every pattern is seen as a normal, a subnormal and a vanishing
    e4m3 element, and the maxima run through every exponent up to the type's largest."""
    eb, mb, _ = FORMATS[fmt]
    b = torch.arange(65536, dtype=torch.int64)
    b = b[((b >> mb) & ((1 << eb) - 1)) != (1 << eb) - 1]
    b = b[torch.argsort((b & 0x7fff) * 2 + (b >> 15))]
    b = torch.cat([b, torch.zeros(-b.numel() % 31, dtype=torch.int64)]).reshape(-1, 31)
    rows = b.shape[0]
    top = (b & 0x7fff).amax(dim=1)
    r = torch.arange(rows)
    one = 1 << mb
    mant = torch.tensor([0, 3 * one // 4, 3 * one // 4 + 1, one - 1, one // 2, 13 * one // 16])[r % 6]
    mx = ((((top >> mb) + (r + shift) % 16) << mb) | mant).clamp(max=((1 << eb) - 1 << mb) - 1)
    mx = torch.maximum(mx, top) | ((r % 2) << 15)
    return torch.cat([mx[:, None], b], dim=1)


def edge_blocks(fmt):
    """(blocks, 32) int64 of the storage type's patterns: RNE ties, e4m3 subnormal results, saturating maxima, 16-bit subnormal inputs, the
    exponent clamp at -127 (bf16), the largest finite values, all-zero blocks of either sign"""
    dt = FORMATS[fmt][2]
    z = [0.0] * 32

    def blk(vals):
        return vals + z[len(vals):]

    rows = [
        blk([17.0, 19.0, 31.0, -17.0, -19.0, 21.0, 23.0, 25.0, 27.0, 29.0]),         # spacing 2 below 32: 17 -> 16, 19 -> 20, ...; 31 x 16 = 496 saturates
        blk([1.0, 2.0 ** -18, 1.5 * 2.0 ** -18, 3 * 2.0 ** -18, 2.5 * 2.0 ** -18, -2.0 ** -18, 2.0 ** -17, 2.0 ** -15, 0.75 * 2.0 ** -14]),
        blk([1.8125, 1.75, 1.7578125, -1.9921875, 0.0078125]),                       # (448, 512) 2^-8 saturate
        blk([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -20, -2.0 ** -16]) if fmt == "fp16" else blk([2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -130, -2.0 ** -127]),
        blk([65504.0, -65504.0, 32768.0, 1.0, 60000.0]) if fmt == "fp16" else blk([2.0 ** 127 * 1.9921875, -2.0 ** 127, 2.0 ** 120, 2.0 ** 112, 1.0]),
        blk([2.0 ** -14, 2.0 ** -15, 2.0 ** -24]) if fmt == "fp16" else blk([2.0 ** -120, 2.0 ** -121, 2.0 ** -126, 2.0 ** -133]),       # shared exponent at / below the clamp
        z, [-0.0] * 32,
    ]
    t = torch.tensor(rows, dtype=F64).to(dt)
    assert bool((t.double() == torch.tensor(rows, dtype=F64)).all()), "an edge value is not representable in " + fmt
    return half_to_bits(t)


def run_quant(ctx, name, x, rows, K):
    """svg_op_quant_mx / svg_op_quant_act_mx (+ _f16) on x (rows, K) -> (q (rows, Kp), sc (rows, Kp / 32)) read back, guards checked"""
    Kp = (K + 127) // 128 * 128 if name == "quant_act_mx" else K
    xb, xv = guarded(x)
    qb, q = guarded(torch.full((rows, Kp), 0xA5, dtype=torch.uint8))
    sb, sc = guarded(torch.full((rows, Kp // 32), 0xA5, dtype=torch.uint8))
    ctx.check(getattr(ctx.lib, "svg_op_" + name + HALF.suffix)(ctx.h, xv.data_ptr(), q.data_ptr(), sc.data_ptr(), rows, K, stream()), name)
    torch.cuda.synchronize()
    for b in (xb, qb, sb):
        guards_intact(b, name)
    return q.cpu(), sc.cpu()


def check_quant(ctx, name, blocks, rows, K, fmt, what):
    """the first rows * K / 32 blocks as a (rows, K) matrix through quantiser `name` against both references (computed on the CPU)"""
    n = rows * (K // 32)
    assert n <= blocks.shape[0]
    bits = blocks[:n].reshape(rows, K)
    x = bits_to_half(bits, fmt)
    act = name == "quant_act_mx"
    q_ref, sc_ref = quant_reference(x, 127 if act else 0)
    q, sc = run_quant(ctx, name, x, rows, K)
    bad_s = sc[:, :K // 32] != sc_ref
    assert not bool(bad_s.any()), "%s %s: %d scale bytes differ; first block %s: %d vs %d" % (
        what, name, int(bad_s.sum()), tuple(int(v) for v in bad_s.nonzero()[0]), int(sc[:, :K // 32][bad_s][0]), int(sc_ref[bad_s][0]))
    bad = ~same_bytes(q[:, :K], q_ref)
    assert not bool(bad.any()), "%s %s: %d e4m3 bytes differ; first at %s: input bits 0x%04x -> 0x%02x, expected 0x%02x" % (
        what, name, int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]), int(bits[bad][0]), int(q[:, :K][bad][0]), int(q_ref[bad][0]))
    if act:
        assert bool((q[:, K:] == 0).all()) and bool((sc[:, K // 32:] == 127).all()), what + ": padding channels are zero bytes with scale byte 127"
    return q, sc


@pytest.mark.parametrize("shift", [0, 5, 11])
def test_quantisers_every_pattern(ctx, _storage, shift):
    """every finite pattern of the storage type through quant_mx (K = 32: one block per row, a row count that is no multiple of 16; K = 160:
    five blocks per row, an odd row count) and quant_act_mx (C = 64 and 192 with a pixel count that is no multiple of 4)"""
    fmt = _storage
    blocks = pattern_blocks(fmt, shift)
    nb = blocks.shape[0]
    assert nb > 2000
    check_quant(ctx, "quant_mx", blocks, nb if nb % 16 else nb - 3, 32, fmt, "patterns K=32")     # (the K = 160 run starts from the other end)
    rows = nb // 5 - (1 - (nb // 5) % 2)
    assert rows % 2 == 1
    check_quant(ctx, "quant_mx", blocks.flip(0), rows, 160, fmt, "patterns K=160")
    for Cc in (64, 192):
        P = nb // (Cc // 32) - 1
        P -= 1 if P % 4 == 0 else 0
        check_quant(ctx, "quant_act_mx", blocks, P, Cc, fmt, "patterns C=%d" % Cc)


def test_quantisers_edge_blocks(ctx, _storage):
    """the named edges, with the bytes they must give written out: ties to even, e4m3 subnormals, saturation, zero blocks"""
    fmt = _storage
    eb = edge_blocks(fmt)
    nb = eb.shape[0]
    for name, zero_scale in (("quant_mx", 0), ("quant_act_mx", 127)):
        q, sc = check_quant(ctx, name, eb, nb, 32, fmt, "edges")
        assert sc[0, 0] == 123 and q[0, :5].tolist() == [0x78, 0x7a, 0x7e, 0xf8, 0xfa]               # 17 -> 16, 19 -> 20, 31 -> 448 / 16, signs kept
        assert sc[1, 0] == 119 and q[1, :9].tolist()[:8] == [0x78, 0x00, 0x01, 0x02, 0x01, q[1, 5].item(), 0x01, 0x04]
        assert q[1, 5].item() & 0x7f == 0                                                              # -2^-10 units: a tie, to (either) zero
        assert sc[2, 0] == 119 and q[2, :4].tolist() == [0x7e, 0x7e, 0x7e, 0xfe]                      # 464, 448, 450 -> 448, -510 saturates
        assert sc[nb - 2, 0] == zero_scale and sc[nb - 1, 0] == zero_scale, "scale byte of an all-zero block"
        assert bool((q[nb - 2:, :32] & 0x7f == 0).all())
        if fmt == "bf16":
            assert sc[3, 0] == 0 and sc[4, 0] == 246                                                  # clamped at -127; floor(log2) = 127 -> 119 + 127
        else:
            assert sc[4, 0] == 15 - 8 + 127 and q[4, 0] == 0x7e                                       # 65504 = 1.999 x 2^15 saturates
    # K = 160 and a ragged row count: the same blocks, five to a row
    check_quant(ctx, "quant_mx", eb.repeat(5, 1), nb, 160, fmt, "edges K=160")


def test_pack_conv_weights_every_pattern(ctx, _storage):
    """pack_conv3x3_mx_kernel on weights that run through every finite 16-bit pattern (as f32) and the edge blocks: Cout = 130 (two padding
    rows), Cin = 64 (half of the 128-channel chunk is padding).  The bytes are read through the documented layouts by run_conv."""
    fmt = _storage
    Cout, Cin = 130, 64
    blocks = torch.cat([edge_blocks(fmt), pattern_blocks(fmt, 3), pattern_blocks(fmt, 8).flip(0)])
    need = Cout * 9 * (Cin // 32)
    assert blocks.shape[0] >= need
    pr = ConvProblem((2, 16, 16, Cin, Cout), False, "onehot", set(), HALF.dtype)
    wt = bits_to_half(blocks[:need].reshape(Cout * 9, Cin), fmt).float()                 # [n][tap][c]
    pr.w = wt.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
    wb, wv = guarded(pr.w)
    xb, xv = guarded(torch.zeros(2, 16, 16, Cin, dtype=HALF.dtype))
    ob, out = guarded(torch.full((512, 132), float("nan"), dtype=HALF.dtype))
    w8b, w8 = guarded(torch.full((132, 9, 128), 0xA5, dtype=torch.uint8))
    w8sb, w8s = guarded(torch.full((9, 1, 132, 4), 0xA5, dtype=torch.uint8))
    with _knobs(HALO_MIN):
        rc, path = conv_ex(ctx, x=xv, w_oihw=wv, out=out, w8_out=w8, w8s_out=w8s, B=2, H=16, W=16, Cin=Cin, Cout=Cout, mode=0)
    ctx.check(rc, "conv3x3_mx_ex")
    torch.cuda.synchronize()
    assert path == (128, 1, 4), path
    for b in (wb, xb, ob, w8b, w8sb):
        guards_intact(b, "pack")
    _, _, want8, want8s = pr.expected_bytes("cpu")
    w8, w8s = w8.cpu(), w8s.cpu()
    qi, si = mx_quant_int(blocks[:need].reshape(Cout * 9, Cin), fmt, 127)                # the integer restatement, through the same layout
    assert bool(same_bytes(want8[:Cout, :, :Cin].reshape(Cout * 9, Cin), qi).all())
    assert torch.equal(want8s.permute(2, 0, 1, 3)[:Cout, :, 0, :Cin // 32].reshape(Cout * 9, Cin // 32), si)
    assert torch.equal(w8s, want8s), "%d weight scale bytes differ" % int((w8s != want8s).sum())
    assert bool(same_bytes(w8, want8).all()), "%d weight bytes differ" % int((~same_bytes(w8, want8)).sum())
    assert bool((w8[Cout:] == 0).all()) and bool((w8[:, :, Cin:] == 0).all()) and bool((w8s[:, :, Cout:] == 127).all()) and bool((w8s[..., 2:] == 127).all())
