"""The GEMM epilogue contract (GemmArgs, csrc/kernels.h) on every kernel path, against an fp64 reference.

svg_op_gemm_ex hands a full launch descriptor to gemm_auto() and reports which kernel ran (family, column tile, split-K); every
case asserts that path first, so a retuned threshold fails here instead of moving the coverage elsewhere.  Paths: the tiled igemm
(BN 32 / 64 / 128 / 160, with and without split-K — the split-K reduce has its own epilogue, epi_value), gemm_pp, gemm_ws (with
the fused V^T write), the 3x3 conv through igemm + split-K and through conv_halo (stride 1 and nearest-2x upsample, with and
without split-K).

Reference: fp64 on the device, from the kernel's own inputs (already rounded to the storage type), epilogue as documented:
  LN(alpha * acc) -> + bias -> + per-sample bias -> + residual -> activation -> one rounding to the output type
with LN(x) = rs x - rm s (normal: per row m / column sums s[n]; swapped: per token t = z * ln_zstride + n / row sums s[m]).

Judging, from the arithmetic alone:
  * integer-exact cases (small-integer operands, powers of two for alpha / rs / rm, quarter-integer biases): every product and
    partial sum is exact in f32, so the output must EQUAL the fp64 reference rounded once to the output type;
  * random cases, per element: |out - ref| <= u |ref| + E with u the output's unit roundoff (2^-8 bf16, 2^-11 fp16, 2^-23 f32)
    and E = K 2^-23 |alpha rs| (|A| |W|^T) + 2^-21 (sum of the magnitudes of the epilogue terms), times 1.13 behind SiLU / GELU
    (their largest slope) plus the activation's own error;
  * C, and the V^T buffer, start as NaN: everything outside the written area (the ldc > N gaps, the rows past M, the batch gaps,
    the V^T columns past vt_rows) must still be NaN; columns n_valid..N-1 hold the epilogue applied to a zero accumulator.
Every test runs on the bf16 build (svg_op_gemm_ex) and on the fp16 build (svg_op_gemm_ex_f16)."""
import ctypes as C
import math
import os
import zlib

import pytest
import torch

from sd_video_gen_amd import _lib

pytestmark = pytest.mark.gpu

IGEMM, HALO, PP, WS = 0, 1, 2, 3          # path[0]: GemmFamily (csrc/kernels.h)
ACT_NONE, ACT_SILU, ACT_GELU, ACT_GEGLU = 0, 1, 2, 3
GELU_ABS_ERR = 2.7e-7                     # gelu_erf's documented error bound (csrc/igemm_epi.h)


class _Half:
    """storage type the current test runs in"""
    dtype = torch.bfloat16
    suffix = ""
    u = 2.0 ** -8


HALF = _Half()


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def _storage(request):
    HALF.dtype, HALF.suffix, HALF.u = (torch.bfloat16, "", 2.0 ** -8) if request.param == "bf16" else (torch.float16, "_f16", 2.0 ** -11)
    yield request.param
    HALF.dtype, HALF.suffix, HALF.u = torch.bfloat16, "", 2.0 ** -8


def stream():
    return torch.cuda.current_stream().cuda_stream


def gemm_ex(ctx, **f):
    """svg_op_gemm_ex(_f16) on a descriptor of the given fields (tensors are passed by pointer); returns (status, path)"""
    d = _lib.GemmDesc()
    d.alpha = 1.0
    d.batch = 1
    d.rows_per_batch = 1
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    path = (C.c_int * 3)(-1, -1, -1)
    rc = getattr(ctx.lib, "svg_op_gemm_ex" + HALF.suffix)(ctx.h, C.byref(d), path, stream())
    return rc, tuple(path)


class _knobs:
    """sets $SVG_* planning knobs the library re-reads through env_refresh, and restores them afterwards"""

    def __init__(self, env):
        self.env = dict(env or {})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        if self.env:
            _lib.env_refresh()

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if self.env:
            _lib.env_refresh()


class _halo_min(_knobs):
    """conv_halo takes a conv only from 192 workgroups on; the kernel does not depend on that count, so the small parity shapes
    lower the threshold ($SVG_HALO_MIN, re-read through env_refresh) and restore it afterwards"""

    def __init__(self, on, more=None):
        _knobs.__init__(self, dict({"SVG_HALO_MIN": "1"} if on else {}, **(more or {})))


def gemm_plan(ctx, **f):
    """svg_op_gemm_plan(_f16) of the same descriptor: (status, (family, bn, splitk, gn_rows, ln_tiles)); launches nothing"""
    d = _lib.GemmDesc()
    d.alpha = 1.0
    d.batch = 1
    d.rows_per_batch = 1
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    plan = (C.c_int * 5)(-1, -1, -1, -1, -1)
    rc = getattr(ctx.lib, "svg_op_gemm_plan" + HALF.suffix)(ctx.h, C.byref(d), plan)
    return rc, tuple(plan)


def onehot_rows(tile_of, pos_of, size_of, T, L):
    """(R, L) 0 / 1 matrix H for the one-hot probes.  Item r sits at position pos_of[r] of tile tile_of[r], which has size_of[r] <= T items.
    P(v) = {0, v - 1} and both sides of every multiple of 16 below v, in order: the probed positions of a tile of v items.  H[r][k] = 1 iff
    pos_of[r] is the (k mod |P(v)|)-th of them.  So for every tile and every k < L exactly one item of the tile has H[.][k] = 1, the item
    moves with k through the first and last position and both sides of every 16-item boundary (every wave's range in all four kernels
    is a whole number of 16-row / 16-column MFMA tiles), and a short last tile is probed the same way."""
    def P(v):
        return sorted({0, v - 1} | {p for k in range(16, v, 16) for p in (k - 1, k)})
    assert len(P(T)) == L
    dev = pos_of.device
    Hm = torch.zeros(pos_of.numel(), L, dtype=torch.bool, device=dev)
    for v in sorted({int(x) for x in size_of.unique()}):
        pv = P(v)
        idx = torch.full((T,), -1, dtype=torch.long, device=dev)
        idx[torch.tensor(pv, device=dev)] = torch.arange(len(pv), device=dev)
        sel = size_of == v
        i = idx[pos_of[sel]]
        Hm[sel] = (i[:, None] == torch.arange(L, device=dev)[None, :] % len(pv)) & (i[:, None] >= 0)
    return Hm.to(torch.float64)


def onehot_len(T):
    return 2 + 2 * ((T - 1) // 16)


def onehot_val(n):
    """the hot value of column n: a power of two that moves with the column (exact in both storage types, and so is its square)"""
    return 2.0 ** ((n % 5) - 2).to(torch.float64)


CONV_AMODE = {"S1": 1, "S2P1": 2, "S2A": 3, "UP2": 4, "SMALLC": 5}      # AMode (csrc/kernels.h)


def conv_out_hw(H, W, mode):
    """output image of a 3x3 conv: stride 1 pad 1 (S1, SMALLC: the Cin = 8 form), stride 2 pad 1 (S2P1), stride 2 with right / bottom
    padding only (S2A: F.pad(x, (0, 1, 0, 1)) then no padding, the downsamplers), nearest-2x upsample then stride 1 pad 1 (UP2)"""
    if mode == "S2P1":
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if mode == "S2A":
        return (H - 2) // 2 + 1, (W - 2) // 2 + 1
    return (2 * H, 2 * W) if mode == "UP2" else (H, W)


def im2col(x, mode):
    """x (B, H, W, Cin) f64 NHWC -> (B * Ho * Wo, 9 * Cin): K index = tap * Cin + c, tap = 3 ky + kx (the packed weight layout)"""
    if mode == "UP2":
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, Cin = x.shape
    if mode in ("S2P1", "S2A"):
        Ho, Wo = conv_out_hw(H, W, mode)
        lead = 1 if mode == "S2P1" else 0                  # rows / columns of zeros in front; behind: whatever the last window needs
        xp = torch.nn.functional.pad(x, (0, 0, lead, 2, lead, 2))
        cols = [xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] for ky in range(3) for kx in range(3)]
        assert 2 * (Ho - 1) + 2 - lead <= H and 2 * (Wo - 1) + 2 - lead <= W      # (at most one row / column of padding is ever read)
        return torch.cat(cols, dim=3).reshape(B * Ho * Wo, 9 * Cin)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)]
    return torch.cat(cols, dim=3).reshape(B * H * W, 9 * Cin)


def _check_silu(x, y):
    """silu_f(x) = x / (1 + __expf(-x)): __expf rounds its argument times log2(e) (relative |x| 2^-24 in the result) and v_exp_f32
    is within 1 ulp (2^-23); the add and the (correctly rounded) division round once each (2^-24): relative error <= (|x| / 2 + 2) 2^-23.
    Asserted with a factor 2 on that: (|x| + 4) 2^-23 |silu(x)|."""
    ref = x * torch.sigmoid(x)
    bound = (x.abs() + 4) * 2.0 ** -23 * ref.abs()
    err = (y - ref).abs()
    assert bool((err <= bound).all()), "SiLU: worst error %.3g at x = %.9g (bound %.3g)" % (
        float(err.max()), float(x.flatten()[int(err.argmax())]), float(bound.flatten()[int(err.argmax())]))


def _gelu_exact(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _check_gelu(x, y):
    """gelu_erf: |gelu - exact| <= 2.7e-7 (csrc/igemm_epi.h), plus the f32 rounding of the result and v_exp_f32's ulp on the tail term"""
    ref = _gelu_exact(x)
    bound = GELU_ABS_ERR + 2.0 ** -24 * ref.abs() + 2.0 ** -23 * x.abs() * 0.5 * torch.erfc(x.abs() / math.sqrt(2))
    err = (y - ref).abs()
    assert bool((err <= bound).all()), "GELU: worst error %.3g at x = %.9g (bound %.3g)" % (
        float(err.max()), float(x.flatten()[int(err.argmax())]), float(bound.flatten()[int(err.argmax())]))


def run_case(ctx, path, M, N, K, batch=1, conv=None, data="int", sA="own", sB="own", lda_pad=0, ldb_pad=0, ldc_pad=0, sC_pad=0,
             n_valid=None, alpha=1.0, bias=None, bias_zs=False, bias_bn=None, res_pad=None, act=ACT_NONE, out_f32=0, ln=None,
             vt=None, halo_min=False, a2=None, a_keep=1, onehot=None, knobs=None, emit=None):
    """builds one problem, runs it, checks the path, the values and the untouched memory.
    conv: (B, H, W, Cin, 'S1' | 'UP2') — A is that NHWC image, Wt packed [N][9][Cin]; bias: None | 'col' | 'row';
    bias_bn: (rows_per_batch, extra row stride or None for bias_bn_ld = 0); res_pad: residual row stride ldr = N + res_pad (None: no
    residual); ln: None | 'normal' | 'swapped'; vt: (vt_n0, vt_rows, vt_ld_pad) for the fused V^T write.
    conv modes: 'S1' | 'UP2' | 'S2P1' | 'S2A' | 'SMALLC' (conv_out_hw).  a2: (k_split, lda2_pad) — A is given as two tensors, columns
    >= k_split come from the second (row stride K - k_split + lda2_pad).  a_keep = r: integer A keeps one element in r, the rest zero
    (bounds the sums of a long K).  onehot: ('gn', rows per row tile) | ('ln', columns per column tile) — operands that leave exactly one
    power of two per (row tile, column) resp. (row, column tile) in C, see onehot_rows; judged as integer-exact.  knobs: further $SVG_*
    planning knobs for the launch.  emit: an object with prepare(ctx, desc, launch_env) (asks the plan, adds gn_part / ln_part to the
    descriptor) and check(ctx, stored C (batch, M, N) f64, integer, relaunch): tests/test_gemm_emit_gpu.py."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(repr((path, M, N, K, batch, conv, data, bias, bias_bn, ln, vt, act)).encode()))
    integer = data == "int" or onehot is not None
    dt = HALF.dtype
    f64 = torch.float64
    nv = N if n_valid is None else n_valid

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device=dev).to(f64)

    def a_ints(shape):
        t = ints(shape, -2, 2)
        return t if a_keep == 1 else t * (torch.randint(0, a_keep, shape, generator=g, device=dev) == 0)

    def randn(shape):
        return torch.randn(shape, generator=g, device=dev, dtype=f64)

    def pow2(shape, vals):
        t = torch.tensor(vals, device=dev, dtype=f64)
        return t[torch.randint(0, len(vals), shape, generator=g, device=dev)]

    desc = dict(M=M, N=N, K=K, batch=batch, alpha=alpha, act=act, out_f32=out_f32, n_valid=nv)
    # ---- A: a dense [batch | 1][M][lda] buffer (columns past K hold values that must not be read), or a conv image
    if conv is not None:
        B, H, W, Cin, mode = conv
        Ho, Wo = conv_out_hw(H, W, mode)
        assert batch == 1 and M == B * Ho * Wo and K == 9 * Cin and a2 is None
        x = (a_ints((B, H, W, Cin)) if integer else randn((B, H, W, Cin))).to(dt)
        if onehot is not None:
            # stride 1, centre tap only (the weights below): C[pixel][n] = sum_c x[pixel][c] W[n][4][c].  Row tile of a pixel: its 16 x 16 block
            # on conv_halo (position 16 ly + lx), 128 consecutive pixels on the tiled kernel
            assert onehot[0] == "gn" and mode == "S1"
            T = onehot[1]
            L = onehot_len(T)
            m = torch.arange(M, device=dev)
            if halo_min:
                py, px = (m % (H * W)) // W, m % W
                tile_of, pos_of = ((m // (H * W)) * (H // 16) + py // 16) * (W // 16) + px // 16, (py % 16) * 16 + px % 16
                size_of = torch.full((M,), T, device=dev)
            else:
                tile_of, pos_of = m // T, m % T
                size_of = torch.clamp(M - tile_of * T, max=T)
            x = torch.zeros(M, Cin, device=dev, dtype=f64)
            x[:, :L] = onehot_rows(tile_of, pos_of, size_of, T, L)
            x = x.reshape(B, H, W, Cin).to(dt)
        A_ops = [im2col(x.to(f64), mode)]
        desc.update(A=x, amode=CONV_AMODE[mode], H=H, W=W, Cin=Cin, Ho=Ho, Wo=Wo)
        keep = [x]
    else:
        ks = K if a2 is None else a2[0]                      # columns of the first source
        lda = ks + lda_pad
        nA = batch if (sA == "own" and batch > 1) else 1
        Ab = (a_ints((nA, M, lda)) if integer else randn((nA, M, lda))).to(dt)
        A2b = None
        if a2 is not None:
            assert batch == 1
            lda2 = K - ks + a2[1]
            A2b = (a_ints((M, lda2)) if integer else randn((M, lda2))).to(dt)
            desc.update(A2=A2b, lda2=lda2, k_split=ks)
        if onehot is not None:
            assert batch == 1 and a2 is None
            T = onehot[1]
            L = onehot_len(T)
            m = torch.arange(M, device=dev)
            Ab[0, :, :K] = 0
            if onehot[0] == "gn":
                Ab[0, :, :L] = onehot_rows(m // T, m % T, torch.clamp(M - (m // T) * T, max=T), T, L).to(dt)
            else:
                Ab[0, m, m % L] = 1                        # row m reads W[n][m mod L]
        A_ops = [Ab[min(z, nA - 1), :, :K].to(f64) for z in range(batch)]
        if a2 is not None:
            A_ops = [torch.cat([Ab[0, :, :ks], A2b[:, :K - ks]], dim=1).to(f64)]
        desc.update(A=Ab, lda=lda, sA=M * lda if nA > 1 else 0)
        keep = [Ab, A2b]
    # ---- W: [batch | 1][N][ldb], asymmetric; rows past n_valid hold 77 (must read as zero)
    ldb = K + ldb_pad
    nB = batch if (sB == "own" and batch > 1) else 1
    if integer:
        zi = torch.arange(nB, device=dev)[:, None, None]
        ni = torch.arange(N, device=dev)[None, :, None]
        ki = torch.arange(ldb, device=dev)[None, None, :]
        Wf = (((ni * 7 + zi * 3) % 5 - 2) + ki % 3).to(f64)
    else:
        Wf = randn((nB, N, ldb)) / math.sqrt(K)
    if onehot is not None:
        assert nv == N and nB == 1
        T = onehot[1]
        L = onehot_len(T)
        n = torch.arange(N, device=dev)
        k0 = 4 * conv[3] if conv is not None else 0          # conv: the centre tap
        Wf[0, :, :K] = 0
        if onehot[0] == "gn":
            Wf[0, n, k0 + n % L] = onehot_val(n)           # column n is hot where the row's position is the (n mod L)-th probed one
        else:
            Wf[0, :, :L] = onehot_rows(n // T, n % T, torch.clamp(N - (n // T) * T, max=T), T, L) * onehot_val(n)[:, None]
    Wf[:, nv:, :] = 77.0
    Wb = Wf.to(dt)
    W_ops = []
    for z in range(batch):
        w = Wb[min(z, nB - 1), :, :K].to(f64).clone()
        w[nv:] = 0
        W_ops.append(w)
    desc.update(Wt=Wb, ldb=ldb, sB=N * ldb if nB > 1 else 0)
    keep.append(Wb)

    acc = [A_ops[min(z, len(A_ops) - 1)] @ W_ops[z].t() for z in range(batch)]
    absacc = [A_ops[min(z, len(A_ops) - 1)].abs() @ W_ops[z].abs().t() for z in range(batch)]

    # ---- LayerNorm fold
    scale = [torch.full((M, N), abs(alpha), device=dev, dtype=f64) for _ in range(batch)]   # |d pre / d acc|
    pre = [alpha * a for a in acc]
    mag = [p.abs() for p in pre]
    if ln == "normal":
        rs = pow2((M,), [0.25, 0.5, 1.0, 2.0]) if integer else 0.5 + 1.5 * torch.rand((M,), generator=g, device=dev, dtype=f64)
        rm = pow2((M,), [-1.0, -0.5, 0.5, 1.0]) if integer else randn((M,))
        sv = ints((N,), -8, 8) if integer else 4 * randn((N,))
        rs, rm, sv = rs.float(), rm.float(), sv.float()
        desc.update(ln_rs=rs, ln_rm=rm, ln_s=sv)
        keep += [rs, rm, sv]
        for z in range(batch):
            pre[z] = pre[z] * rs.to(f64)[:, None] - rm.to(f64)[:, None] * sv.to(f64)[None, :]
            scale[z] = scale[z] * rs.to(f64).abs()[:, None]
            mag[z] = (alpha * acc[z] * rs.to(f64)[:, None]).abs() + (rm.to(f64)[:, None] * sv.to(f64)[None, :]).abs()
    elif ln == "swapped":
        zst = nv + 12
        T = (batch - 1) * zst + nv
        rs = pow2((T,), [0.25, 0.5, 1.0, 2.0]) if integer else 0.5 + 1.5 * torch.rand((T,), generator=g, device=dev, dtype=f64)
        rm = pow2((T,), [-1.0, -0.5, 0.5, 1.0]) if integer else randn((T,))
        sv = ints((M,), -8, 8) if integer else 4 * randn((M,))
        rs, rm, sv = rs.float(), rm.float(), sv.float()
        desc.update(ln_rs=rs, ln_rm=rm, ln_s=sv, ln_swapped=1, ln_zstride=zst)
        keep += [rs, rm, sv]
        n = torch.arange(N, device=dev)
        for z in range(batch):
            t = (z * zst + n).clamp(max=T - 1)
            rsz = torch.where(n < nv, rs.to(f64)[t], torch.zeros_like(t, dtype=f64))      # tokens past n_valid: rs = rm = 0
            rmz = torch.where(n < nv, rm.to(f64)[t], torch.zeros_like(t, dtype=f64))
            pre[z] = pre[z] * rsz[None, :] - rmz[None, :] * sv.to(f64)[:, None]
            scale[z] = scale[z] * rsz.abs()[None, :]
            mag[z] = (alpha * acc[z] * rsz[None, :]).abs() + (rmz[None, :] * sv.to(f64)[:, None]).abs()

    # ---- bias (per batch at z * bias_zs; the gap between batches holds values that must not be read)
    if bias is not None:
        L = N if bias == "col" else M
        zs = L + 16 if (bias_zs and batch > 1) else 0
        bb = ((ints((zs * (batch - 1) + L,), -8, 8) * 0.25) if integer else randn((zs * (batch - 1) + L,))).float()
        desc.update(bias=bb, bias_row=1 if bias == "row" else 0, bias_zs=zs)
        keep.append(bb)
        for z in range(batch):
            v = bb.to(f64)[z * zs:z * zs + L]
            v = v[None, :] if bias == "col" else v[:, None]
            pre[z] = pre[z] + v
            mag[z] = mag[z] + v.abs()
    if bias_bn is not None:
        rpb, ldpad = bias_bn
        ld = N if ldpad is None else N + ldpad
        nb = (M + rpb - 1) // rpb
        bn = (ints((nb, ld), -4, 4) if integer else randn((nb, ld))).float()
        desc.update(bias_bn=bn, rows_per_batch=rpb, bias_bn_ld=0 if ldpad is None else ld)
        keep.append(bn)
        rows = bn.to(f64)[torch.arange(M, device=dev) // rpb, :N]
        for z in range(batch):
            pre[z] = pre[z] + rows
            mag[z] = mag[z] + rows.abs()

    # ---- output layout: C covers the columns below vt_n0 (all N without a V^T write)
    n_c = vt[0] if vt is not None else N
    ldc = n_c + ldc_pad
    sC = M * ldc + sC_pad
    desc.update(ldc=ldc, sC=sC)
    if res_pad is not None:
        ldr = N + res_pad
        Rb = (ints(((batch - 1) * sC + M * ldr,), -4, 4) if integer else randn(((batch - 1) * sC + M * ldr,))).to(dt)
        desc.update(residual=Rb, ldr=ldr)
        keep.append(Rb)
        m_i = torch.arange(M, device=dev)[:, None]
        n_i = torch.arange(N, device=dev)[None, :]
        for z in range(batch):
            r = Rb.to(f64)[z * sC + m_i * ldr + n_i]
            pre[z] = pre[z] + r
            mag[z] = mag[z] + r.abs()

    out_dt = torch.float32 if out_f32 else dt
    Cbuf = torch.full(((batch - 1) * sC + (M + 3) * ldc,), float("nan"), device=dev, dtype=out_dt)    # 3 rows past M
    desc["C"] = Cbuf
    if vt is not None:
        vt_n0, vt_rows, vt_ldpad = vt
        vt_ld = vt_rows + vt_ldpad
        vt_bs = (N - vt_n0) * vt_ld + 64
        samples = M // vt_rows
        VTbuf = torch.full((samples * vt_bs,), float("nan"), device=dev, dtype=dt)
        desc.update(vt_out=VTbuf, vt_n0=vt_n0, vt_rows=vt_rows, vt_ld=vt_ld, vt_bs=vt_bs)

    launch_env = _halo_min(halo_min, knobs)
    if emit is not None:
        emit.prepare(ctx, desc, launch_env)

    def launch():
        with launch_env:
            return gemm_ex(ctx, **desc)

    rc, got = launch()
    ctx.check(rc, "gemm_ex")
    torch.cuda.synchronize()
    assert got == tuple(path), "kernel path %s, expected %s" % (got, tuple(path))

    # ---- values
    u = 2.0 ** -23 if out_f32 else HALF.u
    m_i = torch.arange(M, device=dev)[:, None]
    written = torch.zeros(Cbuf.numel(), dtype=torch.bool, device=dev)
    outs, refs, pres, bnds = [], [], [], []
    for z in range(batch):
        ref = pre[z]
        E = K * 2.0 ** -23 * scale[z] * absacc[z] + 2.0 ** -21 * mag[z]
        if act == ACT_SILU:
            x = ref
            ref = x * torch.sigmoid(x)
            E = 1.13 * E + (x.abs() + 4) * 2.0 ** -23 * ref.abs()
        elif act == ACT_GELU:
            x = ref
            ref = _gelu_exact(x)
            E = 1.13 * E + GELU_ABS_ERR + 2.0 ** -24 * ref.abs()
        idx = z * sC + m_i * ldc + torch.arange(n_c, device=dev)[None, :]
        written[idx.flatten()] = True
        outs.append(Cbuf[idx].to(f64))
        refs.append(ref[:, :n_c])
        bnds.append(u * ref[:, :n_c].abs() + 1.01 * E[:, :n_c])
        pres.append(ref)
    out, ref, bnd = torch.stack(outs), torch.stack(refs), torch.stack(bnds)
    if integer:
        want = ref.to(out_dt).to(f64)
        bad = (out != want)
        assert not bool(bad.any()), "%d elements differ from the exact result; first at (z, m, n) = %s: %g vs %g" % (
            int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(out[bad][0]), float(want[bad][0]))
    else:
        err = (out - ref).abs()
        ok = err <= bnd
        assert bool(ok.all()), "%d elements outside the bound; first at (z, m, n) = %s: |err| %.3g, bound %.3g" % (
            int((~ok).sum()), tuple(int(i) for i in (~ok).nonzero()[0]), float(err[~ok][0]), float(bnd[~ok][0]))
    assert bool(Cbuf[~written].isnan().all()), "%d elements written outside C's [batch][M][ldc < %d] area" % (
        int((~Cbuf[~written].isnan()).sum()), n_c)
    if vt is not None:
        vt_n0, vt_rows, _ = vt
        vwritten = torch.zeros(VTbuf.numel(), dtype=torch.bool, device=dev)
        mm = torch.arange(M, device=dev)
        smp, tok = mm // vt_rows, mm % vt_rows
        cols = torch.arange(N - vt_n0, device=dev)
        vidx = smp[:, None] * vt_bs + cols[None, :] * vt_ld + tok[:, None]          # [m][column]
        vwritten[vidx.flatten()] = True
        vref = pres[0][:, vt_n0:]
        vout = VTbuf[vidx].to(f64)
        if integer:
            want = vref.to(dt).to(f64)
            assert torch.equal(vout, want), "V^T: %d elements differ from the exact result" % int((vout != want).sum())
        else:
            E = K * 2.0 ** -23 * scale[0] * absacc[0] + 2.0 ** -21 * mag[0]
            assert bool(((vout - vref).abs() <= HALF.u * vref.abs() + 1.01 * E[:, vt_n0:]).all()), "V^T outside the bound"
        assert bool(VTbuf[~vwritten].isnan().all()), "%d elements written outside V^T's [sample][column][vt_rows] area" % (
            int((~VTbuf[~vwritten].isnan()).sum()))
    if emit is not None:
        emit.check(ctx, out, integer, launch)
    del keep


# Row strides and batch strides of 16-bit buffers stay multiples of 8 elements (the wide epilogue moves 16 bytes per lane), f32
# ones multiples of 4.
# ---- the path x feature matrix -------------------------------------------------------------------------------------
# Each entry: (id, expected path, problem, features).  Features a path's support predicate excludes are left out of its entries
# (gemm_pp / gemm_ws / conv: batch 1; gemm_ws: no row bias, per-sample bias, swapped fold, n_valid < N or f32 output; gemm_pp:
# no row bias or f32 output; conv_halo: no f32 output).
def _dense_bundles(tag, path, M, N, K, batch):
    """five bundles of one dense shape: batched integer-exact (16-bit / f32 output), batch-1 integer-exact with the per-sample
    bias and the normal LayerNorm fold, and random data behind SiLU and GELU (the batched shapes take the same path)"""
    nv = N - 4
    return [
        (tag + "-int-batch-colbias-res", path, dict(M=M, N=N, K=K, batch=batch, sB="shared", lda_pad=8, ldc_pad=8, sC_pad=16, n_valid=nv,
                                                  alpha=2.0, bias="col", bias_zs=True, res_pad=16)),
        (tag + "-int-batch-rowbias-lnswap-f32", path, dict(M=M, N=N, K=K, batch=batch, sA="shared", ldb_pad=8, ldc_pad=4, n_valid=nv,
                                                        alpha=0.5, bias="row", bias_zs=True, ln="swapped", out_f32=1)),
        (tag + "-int-biasbn-ln", path, dict(M=M, N=N, K=K, ldc_pad=16, alpha=0.5, bias="col", bias_bn=(M // 3, 8), res_pad=8,
                                            ln="normal", n_valid=nv)),
        (tag + "-rand-batch-silu", path, dict(M=M, N=N, K=K, batch=batch, data="rand", bias="col", bias_zs=True, res_pad=0, ldc_pad=8,
                                            act=ACT_SILU)),
        (tag + "-rand-gelu-ln-f32", path, dict(M=M, N=N, K=K, data="rand", alpha=0.7, bias="col", bias_bn=(100, None), ln="normal",
                                               act=ACT_GELU, out_f32=1)),
    ]


CASES = (
    _dense_bundles("igemm32", (IGEMM, 32, 1), 300, 32, 128, 3)
    + _dense_bundles("igemm64", (IGEMM, 64, 1), 300, 64, 128, 3)
    + _dense_bundles("igemm128", (IGEMM, 128, 1), 4096, 320, 320, 2)
    + _dense_bundles("igemm160", (IGEMM, 160, 1), 8192, 640, 320, 2)
    + _dense_bundles("splitk", (IGEMM, 128, 5), 256, 640, 1280, 3)
    + [
        # 16-bit output through the split-K reduce, batched as the GroupNorm-folded proj_in is
        ("splitk-batched-int", (IGEMM, 128, 2), dict(M=1024, N=640, K=640, batch=4, bias="col", bias_zs=True, res_pad=8, ldc_pad=8,
                                                     n_valid=636, alpha=2.0)),
        ("splitk-batched-rowbias-int", (IGEMM, 128, 2), dict(M=1024, N=640, K=640, batch=4, sA="shared", bias="row", bias_zs=True,
                                                             ln="swapped", n_valid=600)),
        # gemm_pp: batch 1 (M = 16384 + 37: a ragged last row tile)
        ("pp-int-colbias-res-ln", (PP, 128, 1), dict(M=16421, N=640, K=1280, ldc_pad=8, n_valid=636, alpha=2.0, bias="col", res_pad=8,
                                                     ln="normal")),
        ("pp-int-biasbn-lnswap", (PP, 128, 1), dict(M=16421, N=640, K=1280, bias_bn=(1024, 16), ln="swapped", n_valid=620, alpha=0.5)),
        ("pp-rand-silu", (PP, 128, 1), dict(M=16421, N=640, K=1280, data="rand", bias="col", res_pad=8, act=ACT_SILU)),
        ("pp-rand-gelu-ln", (PP, 128, 1), dict(M=16421, N=640, K=1280, data="rand", alpha=0.7, bias="col", ln="normal", act=ACT_GELU)),
        # gemm_pp at 160 columns: 26 row tiles (the last one 37 rows) x 8 column tiles in one round, 16 slabs — the shortest K it takes
        ("pp160-int-colbias-res-ln", (PP, 160, 1), dict(M=6437, N=1280, K=1024, ldc_pad=8, n_valid=1276, alpha=2.0, bias="col", res_pad=8,
                                                        ln="normal")),
        ("pp160-rand-silu", (PP, 160, 1), dict(M=6437, N=1280, K=1024, data="rand", bias="col", res_pad=8, act=ACT_SILU)),
        # gemm_ws: K = 320, >= 16384 rows, whole 160-column groups
        ("ws-int-colbias-res-ln", (WS, 160, 1), dict(M=16421, N=320, K=320, ldc_pad=8, alpha=2.0, bias="col", res_pad=8, ln="normal")),
        ("ws-int-960", (WS, 160, 1), dict(M=16384, N=960, K=320, lda_pad=8, ldc_pad=16, alpha=0.5, bias="col", res_pad=0)),
        ("ws-rand-silu", (WS, 160, 1), dict(M=16421, N=320, K=320, data="rand", bias="col", res_pad=8, act=ACT_SILU)),
        ("ws-rand-gelu-ln", (WS, 160, 1), dict(M=16384, N=960, K=320, data="rand", alpha=0.7, bias="col", ln="normal", act=ACT_GELU)),
        ("ws-vt-int-ln", (WS, 160, 1), dict(M=16384, N=960, K=320, ldc_pad=8, alpha=2.0, bias="col", ln="normal", vt=(640, 4096, 8))),
        ("ws-vt-rand", (WS, 160, 1), dict(M=16384, N=960, K=320, data="rand", bias="col", vt=(640, 4096, 4))),
        # 3x3 conv, 32 x 32, Cin = Cout = 640, B = 2: the tiled kernel at 160 columns with split-K 7
        ("conv-igemm-int-biasbn-res", (IGEMM, 160, 7), dict(M=2048, N=640, K=5760, conv=(2, 32, 32, 640, "S1"), ldc_pad=8, n_valid=632,
                                                            alpha=2.0, bias="col", bias_bn=(1024, 8), res_pad=16)),
        ("conv-igemm-int-rowbias-ln-f32", (IGEMM, 160, 7), dict(M=2048, N=640, K=5760, conv=(2, 32, 32, 640, "S1"), bias="row",
                                                                ln="normal", out_f32=1, alpha=0.5)),
        ("conv-igemm-rand-silu", (IGEMM, 160, 7), dict(M=2048, N=640, K=5760, conv=(2, 32, 32, 640, "S1"), data="rand", bias="col",
                                                       bias_bn=(1024, None), act=ACT_SILU)),
    ]
)
# conv_halo (forced below its 192-workgroup threshold): stride 1 and nearest-2x upsample, without split-K (Cin 128) and with (Cin 256)
for _mode, _H in (("S1", 32), ("UP2", 16)):
    for _B, _Cin, _sk in ((2, 128, 1), (1, 256, 2)):
        _Ho = _H if _mode == "S1" else 2 * _H
        _M, _K = _B * _Ho * _Ho, 9 * _Cin
        _pre = "halo-%s-sk%d" % (_mode, _sk)
        _cv = (_B, _H, _H, _Cin, _mode)
        CASES += [
            (_pre + "-int-biasbn-res", (HALO, 128, _sk), dict(M=_M, N=320, K=_K, conv=_cv, halo_min=True, ldc_pad=8, n_valid=316,
                                                               alpha=2.0, bias="col", bias_bn=(_Ho * _Ho, 8), res_pad=8)),
            (_pre + "-int-rowbias-ln", (HALO, 128, _sk), dict(M=_M, N=320, K=_K, conv=_cv, halo_min=True, bias="row", ln="normal",
                                                              alpha=0.5, n_valid=312)),
            (_pre + "-rand-gelu", (HALO, 128, _sk), dict(M=_M, N=320, K=_K, conv=_cv, halo_min=True, data="rand", bias="col", res_pad=0,
                                                         act=ACT_GELU)),
        ]
# conv_halo at 160 columns: 13 x 4 pixel blocks x 4 channel tiles = 208 workgroups (no split-K), two 64-channel chunks — the second patch
# buffer, the next chunk's patch pieces among the taps and the chunk boundary of the weight slabs all run
_cv = (13, 32, 32, 128, "S1")
CASES += [
    ("halo160-int-biasbn-res", (HALO, 160, 1), dict(M=13312, N=640, K=1152, conv=_cv, halo_min=True, n_valid=632, bias="col",
                                                    bias_bn=(1024, 8), res_pad=8)),
    ("halo160-rand-gelu", (HALO, 160, 1), dict(M=13312, N=640, K=1152, conv=_cv, halo_min=True, data="rand", bias="col", res_pad=0,
                                               act=ACT_GELU)),
]


@pytest.mark.parametrize("path,kw", [pytest.param(p, kw, id=i) for i, p, kw in CASES])
def test_epilogue_matrix(ctx, path, kw):
    run_case(ctx, path, **kw)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", [ACT_SILU, ACT_GELU])
def test_activation_through_identity_a(ctx, act, split):
    """A = I (M x K, ones on the diagonal), f32 output: the epilogue sees x = W[n][m] + bias[n] (one f32 add), swept over [-10, 10]
    with dense values near 0 and |x| > 6 (where gelu_erf reuses its polynomial at 6); through the tile epilogue and the split-K reduce."""
    M, N, K = (256, 640, 1280) if split else (256, 64, 256)
    want_path = (IGEMM, 128, 5) if split else (IGEMM, 64, 1)
    g = torch.Generator(device="cuda").manual_seed(act * 2 + split)
    n = M * N
    grid = torch.cat([torch.linspace(-10, 10, n // 2, device="cuda", dtype=torch.float64),
                      torch.linspace(-0.05, 0.05, n // 4, device="cuda", dtype=torch.float64),
                      torch.linspace(-1, 1, n // 8, device="cuda", dtype=torch.float64),
                      torch.linspace(5.5, 10, n // 8, device="cuda", dtype=torch.float64) * torch.tensor([1.0, -1.0], device="cuda",
                                                                                                         dtype=torch.float64).repeat(n // 16)])
    grid = grid[torch.randperm(n, generator=g, device="cuda")].reshape(N, M)          # x[m][n] = grid[n][m] + bias[n]
    A = torch.eye(M, K, device="cuda").to(HALF.dtype)
    W = torch.zeros(N, K, device="cuda", dtype=HALF.dtype)
    W[:, :M] = grid.to(HALF.dtype)
    b = (torch.rand(N, generator=g, device="cuda", dtype=torch.float64) * 2 ** -6).float()
    out = torch.full((M, N), float("nan"), device="cuda")
    rc, path = gemm_ex(ctx, A=A, lda=K, Wt=W, ldb=K, C=out, ldc=N, M=M, N=N, K=K, bias=b, act=act, out_f32=1)
    ctx.check(rc, "gemm_ex")
    assert path == want_path, "kernel path %s, expected %s" % (path, want_path)
    x = (W[:, :M].float().t() + b[None, :]).double()                 # the f32 sum the epilogue forms
    assert float(x.abs().max()) > 9.9 and int((x.abs() < 1e-2).sum()) > 100
    (_check_silu if act == ACT_SILU else _check_gelu)(x, out.double())


def test_gn_folded_proj_in_bias_zs_regression(ctx):
    """The UNet's GroupNorm-folded proj_in (unet.cpp: per-sample weights Wb[b] = W diag(gamma rstd_b), per-sample bias bb[b] at
    bias_zs = C) at the 32 x 32 level with 4 frames: M = 1024, N = K = 640, batch 4 plans split-K 2 — the split-K reduce used to add
    frame 0's folded bias to every frame."""
    Bn, HW, Cc, groups = 4, 1024, 640, 32
    g = torch.Generator(device="cuda").manual_seed(433)
    f64 = torch.float64
    x = torch.randn(Bn, HW, Cc, generator=g, device="cuda").to(HALF.dtype)
    W = torch.randn(Cc, Cc, generator=g, device="cuda", dtype=f64) / math.sqrt(Cc)
    bias = torch.randn(Cc, generator=g, device="cuda", dtype=f64)
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g, device="cuda", dtype=f64)
    beta = 0.5 * torch.randn(Cc, generator=g, device="cuda", dtype=f64)
    mean = torch.randn(Bn, groups, generator=g, device="cuda", dtype=f64)
    rstd = 0.5 + torch.rand(Bn, groups, generator=g, device="cuda", dtype=f64)
    cg = torch.arange(Cc, device="cuda") // (Cc // groups)
    a = gamma[None, :] * rstd[:, cg]                                                   # [b][c]
    Wb = (W[None, :, :] * a[:, None, :]).to(HALF.dtype).contiguous()                   # gn_fold_weights: [b][n][c]
    bb = (bias[None, :] + (W[None, :, :] * (beta[None, :] - mean[:, cg] * a)[:, None, :]).sum(-1)).float().contiguous()
    h = torch.full((Bn, HW, Cc), float("nan"), device="cuda", dtype=HALF.dtype)
    rc, path = gemm_ex(ctx, A=x, lda=Cc, Wt=Wb, ldb=Cc, C=h, ldc=Cc, M=HW, N=Cc, K=Cc, batch=Bn, sA=HW * Cc, sB=Cc * Cc, sC=HW * Cc,
                       bias=bb, bias_zs=Cc)
    ctx.check(rc, "gemm_ex")
    assert path == (IGEMM, 128, 2), "kernel path %s: the regression shape no longer takes the split-K reduce" % (path,)
    acc = torch.einsum("bmk,bnk->bmn", x.to(f64), Wb.to(f64))
    ref = acc + bb.to(f64)[:, None, :]
    bound = HALF.u * ref.abs() + 1.01 * (Cc * 2.0 ** -23 * torch.einsum("bmk,bnk->bmn", x.to(f64).abs(), Wb.to(f64).abs())
                                          + 2.0 ** -21 * (acc.abs() + bb.to(f64).abs()[:, None, :]))
    err = (h.to(f64) - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), "frames outside the bound: %s" % [int(bad[b].sum()) for b in range(Bn)]


def _refused(ctx, what, **f):
    """the call returns an error naming the problem and leaves C untouched (nothing launched)"""
    out = f["C"]
    rc, _ = gemm_ex(ctx, **f)
    torch.cuda.synchronize()
    assert rc == _lib.SVG_ERR_INVALID, "%s: status %d, expected a refusal" % (what, rc)
    assert len(ctx.lib.svg_last_error(ctx.h)) > 0
    assert bool(out.isnan().all()), what + ": C was written"


def test_refused_combinations(ctx):
    """combinations that no kernel honours per batch, and a V^T write of a partial sample: an error, not a wrong answer"""
    dt = HALF.dtype
    M, N, K, B = 256, 256, 128, 2
    A = torch.ones(B, M, K, device="cuda", dtype=dt)
    W = torch.ones(B, N, K, device="cuda", dtype=dt)
    Cb = torch.full((B, M, N), float("nan"), device="cuda", dtype=dt)
    v = torch.ones(B * max(M, N) * 2, device="cuda")
    base = dict(A=A, lda=K, Wt=W, ldb=K, C=Cb, ldc=N, M=M, N=N, K=K, batch=B, sA=M * K, sB=N * K, sC=M * N)
    _refused(ctx, "bias_bn with batch 2", bias_bn=v, rows_per_batch=64, **base)
    _refused(ctx, "normal LayerNorm fold with batch 2", ln_rs=v, ln_rm=v, ln_s=v, **base)
    _refused(ctx, "swapped LayerNorm fold with a per-batch A", ln_rs=v, ln_rm=v, ln_s=v, ln_swapped=1, ln_zstride=N, **base)
    _refused(ctx, "GEGLU with bias_zs", bias=v, bias_zs=N, act=ACT_GEGLU, **dict(base, ldc=N // 2))
    # the fused V^T write of M = 16400 rows in samples of 4096: a partial last sample
    Mv, Nv = 16400, 960
    Av = torch.ones(Mv, 320, device="cuda", dtype=dt)
    Wv = torch.ones(Nv, 320, device="cuda", dtype=dt)
    Cv = torch.full((Mv, 640), float("nan"), device="cuda", dtype=dt)
    VT = torch.full((5, 320, 4096), float("nan"), device="cuda", dtype=dt)
    _refused(ctx, "V^T write of a partial sample", A=Av, lda=320, Wt=Wv, ldb=320, C=Cv, ldc=640, M=Mv, N=Nv, K=320, vt_out=VT, vt_n0=640,
             vt_rows=4096, vt_ld=4096, vt_bs=320 * 4096)
    assert bool(VT.isnan().all())
