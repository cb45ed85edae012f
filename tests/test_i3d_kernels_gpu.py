"""The kernels of the FVD evaluation (csrc/i3d_kernels.hip) one by one against fp64, element by element.

Each kernel is driven alone through its operator-level hook (svg_op_conv3d, svg_op_pack_conv3d, svg_op_maxpool3d_same, svg_op_avgpool_thw,
svg_op_time_mean, svg_op_ncthw_to_nthwc, svg_op_fd_moments, svg_op_sym_eig) or its existing entry point (svg_fvd_preprocess,
svg_frechet_distance, svg_i3d_forward).  The hooks call the launchers the model calls and take the 'SAME' output sizes and front pads
from the model's own host rule, so that rule is under test too.  Every output buffer is filled with NaN and carries a pad of NaN behind it
that must still be NaN afterwards; the reference is oracle/i3d_oracle.py (unit3d, maxpool_same, cov, preprocess, frechet_distance,
i3d_forward; pinned to the live reference by tests/test_oracle_i3d.py) in float64 on the same f32 inputs; every element is judged, none
left out (a non-finite result, a NaN ratio included, counts as inf).  The worst err / bound per kernel and data class goes through
conftest.margin(..., tol=1.0, unit="err/bound").

TWO DATA CLASSES
  exact   small integers, conv weights that differ per tap, input channel and output channel ((31 co + 17 ci + 7 tap) mod 23 - 11), no
          BatchNorm: every product and partial sum is an integer below 2^24 (checked per case), so the f32 result is the fp64 one in any
          order.  The bound is 0: bit equality.  The max pool, the layout kernel and the scale-1 preprocess are exact on any data.
  random  unit-scale normal data, e = 2^-24, judged by the bounds below, each multiplied by 1.01 for the products of two of its terms.
          No constant here was fitted to what the GPU returns.

BOUNDS (random class)
  conv3d       K = taps Cin terms cost (K + 2) e sum |w||x| in any order, + e |y| for the bias add.  With folded BatchNorm (the
               reference folds in fp64 from the same f32 parameters; the library packs with svg_op_pack_conv3d): + 4 e sum |w||x| (rsqrtf
               at 2 ulp as tests/test_ff_fused_gpu.py takes it, plus the two products) + 4 e (|beta| + |mean scale|) for the shift.
               sum |w||x| is the oracle's unit3d on magnitudes.  With ReLU the pre-activation bound b is judged, and exactly 0 is required
               wherever the reference is below -b.  Channels of y outside [coff, coff + Cout) must keep their NaN.
  pack_conv3d  weights: relative 4 e with BatchNorm, bit equal without; padded input channels exactly 0; bias: 4 e (|beta| + |mean scale|)
               with BatchNorm, the conv bias bit for bit, exactly 0 with neither.
  maxpool      max is exact: torch.equal to the fp64 maxpool_same cast to f32.  On strictly negative data every window that touches the
               padding is exactly 0 and every other one negative (which windows touch it: maxpool_same of a constant -1).
  avgpool_thw, time_mean   a sequential sum of n terms: (n + 2) e sum |x| / n, + e |y| for the division.
  ncthw_to_nthwc           bit equal, the pad channel exactly 0.
  fvd_preprocess   bilinear interpolation is continuous in the source coordinate and piecewise linear with slope at most 1 per axis for
               values in [0,1]: a coordinate off by delta moves the value by at most delta per axis.  The f32 coordinate
               (i + 0.5) (H / Hs) - 0.5 carries the rounding of the ratio, of the product (magnitude below max(H, W)) and of the
               difference: three roundings, 3 e max(H, W), taken as delta = 4 e max(H, W).  Two axes: 2 delta; the arithmetic on the
               values in [0,1] (the division by 255, the weights 1 - l, three lerps, the subtraction of 0.5) is given 4 e; the final x 2
               doubles everything: 2 (2 delta) + 8 e.  (Counted one by one the value arithmetic is ten roundings at most; the e max(H, W)
               >= 48 e per axis that delta holds beyond the coordinate's three roundings covers the other six.)
               At 225 x 224 the scale is exactly 1, every weight is 0 or 1 and the result is bit equal to
               (v / 255 - 0.5) 2.  On a random uint8 video a wrong pixel is an error of order 0.1 - 1; the bound is about 3e-4 at 240 x 320.
  fd_moments   f64 accumulation, u = 2^-53: mean (n + 4) u mean|x|; cov (n + 4) u sum |x_a - m_a||x_b - m_b| / (n - 1), plus the second-
               order term n dm_a dm_b / (n - 1) of the mean's own error (its first-order term vanishes: sum (x - m) = 0).  The variance of a
               constant column is exactly 0 (k c is exact in f64 for an f32 c, and (n c) / n = c).
  sym_eig      tol = (1e-15 + 40 d u) |A|_F: 1e-15 is the kernel's stop threshold (off^2 <= 1e-30 diag^2), 40 its sweep cap.
               |lambda - torch.linalg.eigvalsh| <= tol after sorting, max |A V - V L| <= tol, max |V^T V - I| <= tol / |A|_F.
  frechet      closed forms on full-rank data whose relations are exact in f32 (multiples of 2^-10): FD(x, x + c) = |c|^2,
               FD(x, a x) = (1 - a)^2 (tr S + |m|^2) for a = 0.5, 2, FD(x, x) = 0; bound d tol-factor (tr S1 + tr S2) with the factor
               1e-15 + 40 d u of sym_eig.  d = 2 with n = 2 and a set with a zero-variance column against the fp64 oracle, same bound
               (both sides keep the reference's s < 1e-10 ? s : sqrt(s)).

THE NETWORK OFF ITS ONE TESTED SHAPE   svg_i3d_forward at clip lengths 10 (5 -> 5 -> 3 -> 2 in time) and 13 (7 -> 7 -> 4 -> 2), which take
the `size % stride != 0` branch of the padding rule in convs and pools, against the oracle's i3d_forward in float64, computed in the test
(about half a second per clip on 8 CPU threads).  rel-L2 keeps the project's 2e-5; per element the library may be 4 x as far from fp64 as
the f32 CPU oracle is on the same clips (both are f32 with different summation orders); that distance is measured in each run, on the
CPU and with the thread count of the machine that runs the test (6.6e-6 .. 7.9e-6 seen), so the allowance moves with it.  Row 1 of a
batch of 3 equals the clip run alone.

The CPU half (not marked gpu) pushes a torch-f32 emulation of each kernel (the conv: taps outer, 4-channel chunks inner, f32 accumulation;
a plain cyclic Jacobi in fp64 numpy) through the same data and the same judges, and test_judges_reject_cpu requires every judge to reject
the defects listed in MUTATIONS."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import margin, rel_l2
from oracle import i3d_oracle as IO

gpu = pytest.mark.gpu
E = 2.0 ** -24
U = 2.0 ** -53
PAD = 4096
F64, F32 = torch.float64, torch.float32
NAN = float("nan")
SLACK = 1.01
BN_EPS = 1e-5
RES = 224
EIG_STOP, EIG_SWEEPS = 1e-15, 40          # the kernel's stop threshold (sqrt of 1e-30) and sweep cap


def f32c(v):
    return torch.tensor(v, dtype=F32)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def ratio(got, want, bound):
    """worst err / bound of one output; a bound of 0 asks for equality; inf for a wrong shape or a non-finite or missing element"""
    o = got.detach().cpu().to(F64)
    if o.shape != want.shape or not bool(torch.isfinite(o).all()):
        return float("inf")
    if o.numel() == 0:
        return 0.0
    err = (o - want).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    return float(torch.where(err == 0, torch.zeros_like(err), err / b).max())


class Tally:
    """the worst err / bound per data class of one kernel, with the case it came from"""

    def __init__(self, kernel):
        self.kernel, self.worst = kernel, {}

    def add_ratio(self, cls, label, r):
        r = float(r)
        if not math.isfinite(r):                                        # a NaN compares false with everything: it is the worst there is
            r = float("inf")
        if r >= self.worst.get(cls, (-1.0, ""))[0]:
            self.worst[cls] = (r, label)

    def add(self, cls, label, got, ref):
        """got: {name: tensor}; ref: {name: (want, bound)}"""
        assert set(got) == set(ref), (sorted(got), sorted(ref))
        for k in ref:
            self.add_ratio(cls, "%s %s" % (label, k), ratio(got[k], *ref[k]))

    def check(self, report):
        assert self.worst, "%s: nothing was judged" % self.kernel
        for cls, (r, label) in sorted(self.worst.items()):
            print("[i3d_kernels] %-22s %-7s worst err/bound %.3f at %s" % (self.kernel, cls, r, label))
            if report:
                margin("i3d kernel %s, %s class" % (self.kernel, cls), r, 1.0, unit="err/bound")
            else:
                assert r < 1.0, "%s %s: err/bound %.3g at %s" % (self.kernel, cls, r, label)
            if cls == "exact":
                assert r == 0.0, "%s: the exact class is not bit-equal at %s" % (self.kernel, label)

    def rejected(self):
        return {cls: r >= 1.0 for cls, (r, _) in self.worst.items()}


def to_nthwc(x, Cp):
    """(B,C,T,H,W) -> (B,T,H,W,Cp) with zero pad channels: the layout the kernels take (the test's own statement of it)"""
    B, C, T, H, W = x.shape
    y = torch.zeros(B, T, H, W, Cp, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 4, 1)
    return y


# =====================================================================================================================================
# The two implementations behind one interface: the HIP kernels through their hooks, and the torch emulation (with its defects)
# =====================================================================================================================================
def stream():
    return torch.cuda.current_stream().cuda_stream


def i3(v):
    return (ctypes.c_int * 3)(*[int(a) for a in v])


class Gpu:
    mut = None

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib

    def out(self, n, dtype=F32):
        return torch.full((n + PAD,), NAN, device="cuda", dtype=dtype)

    def take(self, o, shape):
        torch.cuda.synchronize()
        n = int(np.prod(shape))
        assert bool(torch.isnan(o[n:]).all()), "the NaN pad behind an output was written"
        return o[:n].cpu().reshape(shape)

    def call(self, name, *args):
        self.ctx.check(getattr(self.lib, name)(self.ctx.h, *args, stream()), name)

    def refused(self, name, *args):
        rc = getattr(self.lib, name)(self.ctx.h, *args, stream())
        torch.cuda.synchronize()
        return rc != 0

    def pack(self, w, bn, cbias, Cp):
        Cout, Cin = w.shape[:2]
        taps = w[0, 0].numel()
        dev = [None if t is None else t.contiguous().cuda() for t in (w,) + (bn if bn else (None,) * 4) + (cbias,)]
        wo, bo = self.out(Cout * taps * Cp), self.out(Cout)
        self.call("svg_op_pack_conv3d", *[None if t is None else t.data_ptr() for t in dev], wo.data_ptr(), bo.data_ptr(), Cout, Cin, Cp, taps,
                  BN_EPS if bn else 0.0)
        return self.take(wo, (Cout, taps, Cp)), self.take(bo, (Cout,))

    def conv3d(self, x, wp, bias, ldc, coff, k, stride, relu, thw):
        """x (B,T,H,W,Cp); wp (Cout,taps,Cp) packed; thw: the output sizes the reference has (the buffer is sized by them, the hook checks
        that its own fit) -> (B,To,Ho,Wo,ldc), NaN outside the slice"""
        B, T, H, W, Cp = x.shape
        Cout = wp.shape[0]
        n = B * thw[0] * thw[1] * thw[2] * ldc
        xd, wd, bd, y = x.contiguous().cuda(), wp.contiguous().cuda(), None if bias is None else bias.contiguous().cuda(), self.out(n)
        o3 = i3((-1, -1, -1))
        self.call("svg_op_conv3d", xd.data_ptr(), B, T, H, W, Cp, wd.data_ptr(), None if bd is None else bd.data_ptr(), y.data_ptr(), n, Cout, ldc, coff,
                  i3(k), i3(stride), int(relu), o3)
        assert tuple(o3) == tuple(thw), "svg_op_conv3d reports the output %s, the reference has %s" % (tuple(o3), tuple(thw))
        return self.take(y, (B,) + tuple(thw) + (ldc,))

    def maxpool(self, x, k, stride, thw):
        B, T, H, W, C = x.shape
        n = B * thw[0] * thw[1] * thw[2] * C
        xd, y, o3 = x.contiguous().cuda(), self.out(n), i3((-1, -1, -1))
        self.call("svg_op_maxpool3d_same", xd.data_ptr(), y.data_ptr(), n, B, T, H, W, C, i3(k), i3(stride), o3)
        assert tuple(o3) == tuple(thw), "svg_op_maxpool3d_same reports the output %s, the reference has %s" % (tuple(o3), tuple(thw))
        return self.take(y, (B,) + tuple(thw) + (C,))

    def avgpool(self, x, kt):
        B, T, HW, C = x.shape
        xd, y = x.contiguous().cuda(), self.out(B * (T - kt + 1) * C)
        self.call("svg_op_avgpool_thw", xd.data_ptr(), y.data_ptr(), B, T, HW, C, kt)
        return self.take(y, (B, T - kt + 1, C))

    def time_mean(self, x):
        B, To, C = x.shape
        xd, y = x.contiguous().cuda(), self.out(B * C)
        self.call("svg_op_time_mean", xd.data_ptr(), y.data_ptr(), B, To, C)
        return self.take(y, (B, C))

    def layout(self, x, Cp):
        B, C, T, H, W = x.shape
        xd, y = x.contiguous().cuda(), self.out(B * T * H * W * Cp)
        self.call("svg_op_ncthw_to_nthwc", xd.data_ptr(), y.data_ptr(), B, C, T, H, W, Cp)
        return self.take(y, (B, T, H, W, Cp))

    def preprocess(self, v):
        B, T, H, W, _ = v.shape
        vd, y = v.contiguous().cuda(), self.out(B * 3 * T * RES * RES)
        self.call("svg_fvd_preprocess", vd.data_ptr(), B, T, H, W, y.data_ptr())
        y = self.take(y, (B, 3, T, RES, RES))
        assert torch.equal(self.ctx.fvd_preprocess(v).cpu(), y), "Context.fvd_preprocess against the same call on a NaN-padded buffer"
        return y

    def moments(self, x):
        n, d = x.shape
        xd, m, c = x.contiguous().cuda(), self.out(d, F64), self.out(d * d, F64)
        self.call("svg_op_fd_moments", xd.data_ptr(), n, d, m.data_ptr(), c.data_ptr())
        return self.take(m, (d,)), self.take(c, (d, d))

    def sym_eig(self, A):
        d = A.shape[0]
        Ad, lam, V = A.contiguous().cuda(), self.out(d, F64), self.out(d * d, F64)
        self.call("svg_op_sym_eig", Ad.data_ptr(), d, lam.data_ptr(), V.data_ptr())
        assert torch.equal(Ad.cpu(), A), "svg_op_sym_eig changed its input"
        return self.take(lam, (d,)), self.take(V, (d, d))

    def frechet(self, x1, x2):
        return self.ctx.frechet_distance(x1.cuda(), x2.cuda())


def same_pad_rule(size, k, s, mut=None):
    """the host rule of csrc/i3d.cpp (same_pad) -> (output size, front pad); mut: a defect"""
    p = max(k - s, 0) if (size % s == 0 or mut == "pad_no_mod_branch") else max(k - size % s, 0)
    front = p - p // 2 if mut == "pad_front_is_back" else p // 2
    return (size + p - k) // s + 1, front


def pad_like_kernel(x, k, stride, mut, value=0.0):
    """x (B,T,H,W,C) -> padded so that window (to, ho, wo) starts at (to st, ho sh, wo sw), and the output sizes, as the kernels' bounds
    checks see it: `front` cells in front, whatever the last window needs behind (a negative pad crops)"""
    out, pads = [], []
    for ax in (0, 1, 2):
        o, front = same_pad_rule(x.shape[1 + ax], k[ax], stride[ax], mut)
        out.append(o)
        pads.append((front, (o - 1) * stride[ax] + k[ax] - x.shape[1 + ax] - front))
    xp = F.pad(x, (0, 0) + pads[2] + pads[1] + pads[0], value=value)
    return xp, out


def sym_sqrt_rule(lam, eps=1e-10):
    lam = np.maximum(lam, 0.0)
    return np.where(lam < eps, lam, np.sqrt(lam))


class Emu:
    """torch f32 (the Fréchet chain: fp64) on the CPU, in the kernels' order where order matters; mut: one defect (MUTATIONS)"""

    def __init__(self, mut=None):
        self.mut = mut

    def pack(self, w, bn, cbias, Cp):
        Cout, Cin = w.shape[:2]
        taps = w[0, 0].numel()
        scale = bn[0] * torch.rsqrt(bn[3] + f32c(BN_EPS)) if bn else torch.ones(Cout)
        wo = torch.zeros(Cout, taps, Cp)
        wo[:, :, :Cin] = (w.reshape(Cout, Cin, taps) * scale[:, None, None]).permute(0, 2, 1)
        bo = bn[1] - bn[2] * scale if bn else (cbias.clone() if cbias is not None else torch.zeros(Cout))
        return wo, bo

    def conv3d(self, x, wp, bias, ldc, coff, k, stride, relu, thw):
        B, Cp, Cout = x.shape[0], x.shape[4], wp.shape[0]
        xp, (To, Ho, Wo) = pad_like_kernel(x, k, stride, self.mut)
        acc = torch.zeros(B, To, Ho, Wo, Cout)
        st, sh, sw = stride
        for tap in range(k[0] * k[1] * k[2]):
            dt, dh, dw = tap // (k[1] * k[2]), (tap // k[2]) % k[1], tap % k[2]
            xs = xp[:, dt:dt + (To - 1) * st + 1:st, dh:dh + (Ho - 1) * sh + 1:sh, dw:dw + (Wo - 1) * sw + 1:sw]
            for c0 in range(0, Cp, 4):                                  # one MFMA step: four channels
                acc = acc + xs[..., c0:c0 + 4] @ wp[:, tap, c0:c0 + 4].t()
        if bias is not None:
            acc = acc + bias
        if relu:
            acc = torch.clamp_min(acc, 0.0)
        y = torch.full((B, To, Ho, Wo, ldc), NAN)
        if self.mut == "conv_coff_shift" and ldc > Cout:
            coff = coff + 1 if coff + Cout < ldc else coff - 1
        y[..., coff:coff + Cout] = acc
        if self.mut == "conv_tile_last_position":
            y.view(-1, ldc)[63::64] = NAN
        if self.mut == "conv_last_cout":
            y[..., coff + Cout - 1] = NAN
        return y

    def maxpool(self, x, k, stride, thw):
        xp, _ = pad_like_kernel(x, k, stride, self.mut, value=float("-inf") if self.mut == "pool_pad_neg_inf" else 0.0)
        return F.max_pool3d(xp.permute(0, 4, 1, 2, 3), tuple(k), tuple(stride)).permute(0, 2, 3, 4, 1).contiguous()

    def avgpool(self, x, kt):
        B, T, HW, C = x.shape
        s = torch.zeros(B, T - kt + 1, C)
        for dt in range(kt):
            for q in range(HW):
                s = s + x[:, dt:dt + T - kt + 1, q]
        return s / f32c(float(kt * HW))

    def time_mean(self, x):
        s = torch.zeros(x.shape[0], x.shape[2])
        for t in range(x.shape[1]):
            s = s + x[:, t]
        return s / f32c(float(x.shape[1]))

    def layout(self, x, Cp):
        return to_nthwc(x, Cp)

    def preprocess(self, v):
        B, T, H, W, _ = v.shape
        scale = RES / min(H, W)
        rnd = math.floor if self.mut == "pre_floor_side" else math.ceil
        Hs, Ws = (RES, rnd(W * scale)) if H < W else (rnd(H * scale), RES)
        idx = []
        for size, scaled in ((H, Hs), (W, Ws)):
            start = (scaled - RES) // 2 + (1 if self.mut == "pre_crop_off_by_one" and scaled > RES else 0)
            o = torch.arange(RES, dtype=F32) + float(start)
            if self.mut == "pre_align_corners":
                f = o * (f32c(float(size - 1)) / f32c(float(scaled - 1)))
            else:
                f = torch.clamp_min((o + 0.5) * (f32c(float(size)) / f32c(float(scaled))) - 0.5, 0.0)
            i0 = f.floor().long().clamp_max(size - 1)
            idx.append((i0, torch.clamp_max(i0 + 1, size - 1), f - i0.float()))
        (y0, y1, ly), (x0, x1, lx) = idx
        p = (v.float() / 255.0).permute(0, 4, 1, 2, 3)                  # (B,3,T,H,W)
        ly, lx = ly[:, None], lx[None, :]
        top = (1 - lx) * p[..., y0, :][..., x0] + lx * p[..., y0, :][..., x1]
        bot = (1 - lx) * p[..., y1, :][..., x0] + lx * p[..., y1, :][..., x1]
        return ((1 - ly) * top + ly * bot - 0.5) * 2.0

    def moments(self, x):
        n = x.shape[0]
        x64 = x.to(F64)
        s = torch.zeros(x.shape[1], dtype=F64)
        for i in range(n):
            s = s + x64[i]
        m = s / n
        c = x64 - m
        return m, (c.t() @ c) / (n if self.mut == "cov_div_n" else n - 1)

    def sym_eig(self, A):
        """plain cyclic Jacobi in fp64 with the kernel's rotation, stop rule and sweep cap"""
        a = A.numpy().copy()
        d = a.shape[0]
        V = np.eye(d)
        for sweep in range(1 if self.mut == "jacobi_one_sweep" else EIG_SWEEPS):
            for p in range(d - 1):
                for q in range(p + 1, d):
                    if abs(a[p, q]) <= 1e-300:
                        continue
                    tau = float(a[q, q] - a[p, p]) / (2.0 * float(a[p, q]))
                    t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                    c = 1.0 / math.sqrt(1.0 + t * t)
                    s = t * c
                    J = np.array([[c, s], [-s, c]])
                    a[[p, q], :] = J.T @ a[[p, q], :]
                    a[:, [p, q]] = a[:, [p, q]] @ J
                    V[:, [p, q]] = V[:, [p, q]] @ J
            if float(((a - np.diag(np.diag(a))) ** 2).sum()) <= 1e-30 * float((np.diag(a) ** 2).sum()):
                break
        V = V.T if self.mut == "eig_vectors_transposed" else V
        return torch.from_numpy(np.diag(a).copy()), torch.from_numpy(np.ascontiguousarray(V))

    def frechet(self, x1, x2):
        if self.mut == "frechet_nan_at_n2" and x1.shape[0] == 2:
            return NAN
        (m1, S1), (m2, S2) = self.moments(x1), self.moments(x2)
        lam, V = self.sym_eig(S1)
        R = V.numpy() @ np.diag(sym_sqrt_rule(lam.numpy())) @ V.numpy().T
        lam2, _ = self.sym_eig(torch.from_numpy(R @ S2.numpy() @ R))
        return float(torch.trace(S1 + S2)) - 2.0 * float(sym_sqrt_rule(lam2.numpy()).sum()) + float(((m1 - m2) ** 2).sum())


# =====================================================================================================================================
# conv3d (through pack_conv3d) and pack_conv3d alone
# =====================================================================================================================================
# name, x (B,Cin,T,H,W), Cin_pad, kernel, stride, Cout, ldc, coff, Unit3D (BatchNorm + ReLU; otherwise a conv bias and no ReLU)
CONV_CASES = [("stem", (1, 3, 5, 9, 10), 4, (7, 7, 7), (2, 2, 2), 64, 64, 0, True),
              ("slice", (2, 16, 3, 5, 7), 16, (3, 3, 3), (1, 1, 1), 24, 40, 8, True),
              ("tails", (3, 24, 2, 3, 5), 24, (1, 1, 1), (1, 1, 1), 70, 70, 0, True),
              ("logits form", (2, 32, 3, 1, 1), 32, (1, 1, 1), (1, 1, 1), 400, 400, 0, False),
              ("stride-2 3x3x3", (1, 8, 6, 7, 6), 8, (3, 3, 3), (2, 2, 2), 16, 16, 0, True)]


def conv_operands(cls, g, xs, k, Cout, unit):
    """x, w, bn (gamma, beta, mean, var) or None, conv bias or None"""
    Cin, taps = xs[1], k[0] * k[1] * k[2]
    if cls == "exact":
        co, ci, tp = torch.arange(Cout)[:, None, None], torch.arange(Cin)[None, :, None], torch.arange(taps)[None, None, :]
        w = (((31 * co + 17 * ci + 7 * tp) % 23) - 11).float().reshape((Cout, Cin) + tuple(k))
        return randint(g, -4, 4, xs), w, None, (randint(g, -64, 64, (Cout,)) if unit else None)         # the logits form: a null bias
    x, w = torch.randn(xs, generator=g), torch.randn((Cout, Cin) + tuple(k), generator=g) / math.sqrt(Cin * taps)
    if unit:
        bn = (1 + 0.1 * torch.randn(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g),
              0.5 + torch.rand(Cout, generator=g))
        return x, w, bn, None
    return x, w, None, 0.3 * torch.randn(Cout, generator=g)


def conv_sd(w, bn, cbias):
    sd = {"u.conv3d.weight": w.to(F64)}
    if cbias is not None:
        sd["u.conv3d.bias"] = cbias.to(F64)
    if bn:
        sd.update({"u.bn.weight": bn[0].to(F64), "u.bn.bias": bn[1].to(F64), "u.bn.running_mean": bn[2].to(F64), "u.bn.running_var": bn[3].to(F64)})
    return sd


def bn_scale64(bn, Cout):
    return bn[0].to(F64) / torch.sqrt(bn[3].to(F64) + BN_EPS) if bn else torch.ones(Cout, dtype=F64)


def ref_conv(cls, x, w, bn, cbias, k, stride, relu):
    """channels-last fp64 reference (relu applied) and the bound of every element"""
    Cout, Cin, taps = w.shape[0], w.shape[1], k[0] * k[1] * k[2]
    z = IO.unit3d(conv_sd(w, bn, cbias), "u", x.to(F64), k, stride, bn=bool(bn), relu=False)
    scale = bn_scale64(bn, Cout)
    A = IO.unit3d({"u.conv3d.weight": (w.to(F64) * scale[:, None, None, None, None]).abs()}, "u", x.to(F64).abs(), k, stride, bn=False, relu=False)
    if cls == "exact":
        mag = A + (0 if cbias is None else cbias.to(F64).abs()[None, :, None, None, None])
        assert bn is None and bool((mag <= 2.0 ** 24).all()), "the exact class's premise"
        b = torch.zeros_like(z)
    else:
        b = (Cin * taps + 2) * E * A + E * z.abs()
        if bn:
            b = b + 4 * E * A + 4 * E * (bn[1].to(F64).abs() + (bn[2].to(F64) * scale).abs())[None, :, None, None, None]
        b = SLACK * b
    want = z
    if relu:
        want = torch.clamp_min(z, 0.0)
        b = torch.where(z < -b, torch.zeros_like(b), b)              # well below zero: the ReLU leaves exactly 0
    return want.permute(0, 2, 3, 4, 1).contiguous(), b.permute(0, 2, 3, 4, 1).contiguous()


def judge_slice(y, want, bound, ldc, coff):
    """y (B,To,Ho,Wo,ldc): channels [coff, coff + Cout) against the reference, every other channel still NaN"""
    Cout = want.shape[-1]
    if y.shape != want.shape[:-1] + (ldc,):
        return float("inf")
    rest = torch.cat([y[..., :coff], y[..., coff + Cout:]], dim=-1)
    if not bool(torch.isnan(rest).all()):
        return float("inf")
    return ratio(y[..., coff:coff + Cout], want, bound)


def sweep_conv3d(impl, tally):
    for cls in ("exact", "random"):
        for i, (name, xs, Cp, k, stride, Cout, ldc, coff, unit) in enumerate(CONV_CASES):
            g = _gen(21, i, cls == "exact")
            x, w, bn, cbias = conv_operands(cls, g, xs, k, Cout, unit)
            want, bound = ref_conv(cls, x, w, bn, cbias, k, stride, unit)
            wp, bp = impl.pack(w, bn, cbias, Cp)
            bias = None if (bn is None and cbias is None) else bp
            y = impl.conv3d(to_nthwc(x, Cp), wp, bias, ldc, coff, k, stride, unit, want.shape[1:4])
            tally.add_ratio(cls, name, judge_slice(y, want, bound, ldc, coff))


def sweep_pack(impl, tally):
    for (Cout, Cin, Cp, k) in ((5, 3, 4, (7, 7, 7)), (24, 16, 16, (1, 1, 1))):
        taps = k[0] * k[1] * k[2]
        for form in ("batchnorm", "conv bias", "neither"):
            g = _gen(22, Cout, Cin, len(form))
            w = torch.randn((Cout, Cin) + k, generator=g)
            bn = (1 + 0.1 * torch.randn(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g),
                  0.5 + torch.rand(Cout, generator=g)) if form == "batchnorm" else None
            cbias = torch.randn(Cout, generator=g) if form == "conv bias" else None
            wo, bo = impl.pack(w, bn, cbias, Cp)
            scale = bn_scale64(bn, Cout)
            ww = torch.zeros(Cout, taps, Cp, dtype=F64)
            ww[:, :, :Cin] = (w.to(F64).reshape(Cout, Cin, taps) * scale[:, None, None]).permute(0, 2, 1)
            if bn:
                wb = bn[1].to(F64) - bn[2].to(F64) * scale
                ref = {"w": (ww, SLACK * 4 * E * ww.abs()), "b": (wb, SLACK * 4 * E * (bn[1].to(F64).abs() + (bn[2].to(F64) * scale).abs()))}
            else:
                ref = {"w": (ww, 0.0), "b": (cbias.to(F64) if cbias is not None else torch.zeros(Cout, dtype=F64), 0.0)}
            tally.add("random" if bn else "exact", "Cout %d Cin %d->%d taps %d %s" % (Cout, Cin, Cp, taps, form), {"w": wo, "b": bo}, ref)


# =====================================================================================================================================
# maxpool3d_same, avgpool_thw, time_mean, ncthw_to_nthwc
# =====================================================================================================================================
POOL_KS = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2))]
POOL_X = [(2, 5, 7, 6), (2, 4, 8, 9)]


def sweep_maxpool(impl, tally):
    for (k, stride) in POOL_KS:
        for xs in POOL_X:
            for C in (8, 12):
                for data in ("negative", "mixed"):
                    g = _gen(23, sum(k), sum(stride), xs[1], C, data == "mixed")
                    x = torch.randn(xs + (C,), generator=g)
                    if data == "negative":
                        x = -(x.abs() + 0.1)
                    ncthw = x.permute(0, 4, 1, 2, 3).to(F64)
                    want = IO.maxpool_same(ncthw, k, stride).permute(0, 2, 3, 4, 1).to(F32)
                    y = impl.maxpool(x, k, stride, want.shape[1:4])
                    ok = y.shape == want.shape and torch.equal(y, want)
                    if ok and data == "negative":
                        pad = IO.maxpool_same(torch.full_like(ncthw, -1.0), k, stride).permute(0, 2, 3, 4, 1) == 0      # windows that touch the padding
                        assert bool(pad.any()), "a 'SAME' pool whose windows never touch the padding"
                        ok = bool((y[pad] == 0).all()) and bool((y[~pad] < 0).all())
                    tally.add_ratio("exact", "k %s stride %s x %s C %d %s" % (k, stride, xs, C, data), 0.0 if ok else float("inf"))


def ref_mean(x64, dims, n):
    y, A = x64.sum(dims) / n, x64.abs().sum(dims) / n
    return y, SLACK * ((n + 2) * E * A + E * y.abs())


def sweep_reduce(impl, t_avg, t_mean, t_layout):
    g = _gen(24)
    B, T, HW, C, kt = 2, 3, 49, 20, 2
    x = torch.randn(B, T, HW, C, generator=g)
    win = torch.stack([x[:, t:t + kt] for t in range(T - kt + 1)], 1).to(F64)        # (B,To,kt,HW,C)
    t_avg.add("random", "(2,3,49,20) kt 2", {"y": impl.avgpool(x, kt)}, {"y": ref_mean(win, (2, 3), kt * HW)})
    # against the reference's own operator on the same data
    want = F.avg_pool3d(x.to(F64).reshape(B, T, 7, 7, C).permute(0, 4, 1, 2, 3), (2, 7, 7), (1, 1, 1))[..., 0, 0].permute(0, 2, 1)
    assert float((want - ref_mean(win, (2, 3), kt * HW)[0]).abs().max()) < 1e-14
    x = torch.randn(3, 5, 400, generator=g)
    t_mean.add("random", "(3,5,400)", {"y": impl.time_mean(x)}, {"y": ref_mean(x.to(F64), (1,), 5)})
    x = torch.randn(2, 3, 3, 5, 6, generator=g)
    y = impl.layout(x, 4)
    t_layout.add("exact", "(2,3,3,5,6) -> 4 channels", {"y": y}, {"y": (to_nthwc(x, 4).to(F64), 0.0)})
    t_layout.add_ratio("exact", "pad channel", 0.0 if y.shape[-1] == 4 and bool((y[..., 3] == 0).all()) else float("inf"))


# =====================================================================================================================================
# fvd_preprocess
# =====================================================================================================================================
PRE_SIZES = [(48, 64), (64, 48), (50, 50), (240, 320), (300, 260), (225, 224)]


def test_preprocess_cases_are_what_they_claim():
    """the geometry the frame sizes were chosen for"""
    def geo(H, W):
        scale = RES / min(H, W)
        Hs, Ws = (RES, math.ceil(W * scale)) if H < W else (math.ceil(H * scale), RES)
        return Hs, Ws, (Hs - RES) // 2, (Ws - RES) // 2
    assert geo(240, 320) == (224, 299, 0, 37) and 320 * RES / 240 != 299          # UCF-101: a downscale, ceil(298.67), odd crop offset
    assert geo(300, 260) == (259, 224, 17, 0)                                       # portrait downscale, crop offset 17
    assert geo(225, 224) == (225, 224, 0, 0)                                        # scale exactly 1
    assert geo(50, 50) == (225, 224, 0, 0)            # square: 50 (224 / 50) is 224.00000000000003 in doubles, and the reference takes its ceil
    assert geo(64, 48)[0] == 299 and geo(48, 64)[1] == 299


def sweep_preprocess(impl, tally):
    for (H, W) in PRE_SIZES:
        v = torch.randint(0, 256, (2, 2, H, W, 3), dtype=torch.uint8, generator=_gen(25, H, W))
        y = impl.preprocess(v)
        want = IO.preprocess(v, dtype=F64)
        if (H, W) == (225, 224):
            plain = ((v[:, :, :RES].float() / 255.0 - 0.5) * 2.0).permute(0, 4, 1, 2, 3)          # crop offset 0: the first 224 rows
            assert float((want - plain.to(F64)).abs().max()) < 1e-6
            tally.add("exact", "225x224 (scale 1)", {"y": y}, {"y": (plain.to(F64), 0.0)})
        delta = 4 * E * max(H, W)
        tally.add("random", "%dx%d" % (H, W), {"y": y}, {"y": (want, SLACK * (2 * (2 * delta) + 8 * E))})


# =====================================================================================================================================
# the Fréchet chain: fd_moments, sym_eig, frechet_distance
# =====================================================================================================================================
def moment_data(g, n, d):
    """unit-scale columns; every third (from the second) with mean 1000 and spread 1; column 0 constant"""
    x = torch.randn(n, d, generator=g)
    x[:, 1::3] += 1000.0
    x[:, 0] = 7.25
    return x


def sweep_moments(impl, tally):
    for (n, d) in ((2, 2), (5, 16), (64, 16)):
        x = moment_data(_gen(26, n, d), n, d)
        m, c = impl.moments(x)
        x64 = x.to(F64)
        wm, wc = x64.mean(0), IO.cov(x64)
        dm = (n + 4) * U * x64.abs().mean(0)
        dev = (x64 - wm).abs()
        bc = (n + 4) * U * (dev.t() @ dev) / (n - 1) + n * dm[:, None] * dm[None, :] / (n - 1)
        tally.add("random", "n %d d %d" % (n, d), {"mean": m, "cov": c}, {"mean": (wm, SLACK * dm), "cov": (wc, SLACK * bc)})
        const = c.shape == (d, d) and float(c[0, 0]) == 0.0 and bool((c[0] == 0).all()) and bool((c[:, 0] == 0).all()) and float(m[0]) == 7.25
        tally.add_ratio("random", "n %d d %d: the constant column's variance is exactly 0" % (n, d), 0.0 if const else float("inf"))


EIG_D = [2, 6, 16, 30]


def eig_matrices(d):
    g = _gen(27, d)
    b = torch.randn(d, d, generator=g, dtype=F64)
    sym = lambda m: (m + m.t()) / 2                                              # a BLAS product need not be symmetric to the bit
    spd = sym(b @ b.t() / d) + 0.1 * torch.eye(d, dtype=F64)
    x = torch.randn(d, 2, generator=g, dtype=F64)
    u = torch.randn(d, 1, generator=g, dtype=F64)
    blk = sym(torch.randn(d, d, generator=g, dtype=F64))
    blk[1, 1] = blk[0, 0]                                                        # app == aqq with apq != 0: tau = 0
    return [("spd", spd), ("rank-2 gram", sym(x @ x.t())), ("diagonal", torch.diag(torch.randn(d, generator=g, dtype=F64))),
            ("I + u u^T", torch.eye(d, dtype=F64) + sym(u @ u.t())), ("app == aqq", blk), ("spd x 1e6", spd * 1e6), ("spd x 1e-6", spd * 1e-6)]


def sweep_sym_eig(impl, tally):
    for d in EIG_D:
        for name, A in eig_matrices(d):
            assert torch.equal(A, A.t())
            lam, V = impl.sym_eig(A)
            nrm = float(A.norm())
            tol = SLACK * (EIG_STOP + EIG_SWEEPS * d * U) * nrm
            label = "d %d %s" % (d, name)
            if lam.shape != (d,) or V.shape != (d, d) or not bool(torch.isfinite(lam).all() and torch.isfinite(V).all()):
                tally.add_ratio("random", label, float("inf"))
                continue
            tally.add_ratio("random", label + " eigenvalues", float((lam.sort().values - torch.linalg.eigvalsh(A)).abs().max()) / tol)
            tally.add_ratio("random", label + " A V - V L", float((A @ V - V * lam[None, :]).abs().max()) / tol)
            tally.add_ratio("random", label + " V^T V - I", float((V.t() @ V - torch.eye(d, dtype=F64)).abs().max()) / (tol / nrm))


def grid(g, shape, scale=1.0):
    """normal draws rounded to multiples of 2^-10: sums and power-of-two multiples of a few of them are exact in f32"""
    return torch.round(torch.randn(shape, generator=g) * scale * 1024.0) / 1024.0


def sweep_frechet(impl, tally):
    d, n = 16, 64
    g = _gen(28)
    x = grid(g, (n, d)) + 0.25
    c = grid(g, (1, d), 0.5)
    x64 = x.to(F64)
    tr, mm = float(torch.trace(IO.cov(x64))), float((x64.mean(0) ** 2).sum())
    fac = SLACK * d * (EIG_STOP + EIG_SWEEPS * d * U)
    cases = [("FD(x, x + c) = |c|^2", x + c, float((c.to(F64) ** 2).sum()), 2 * tr), ("FD(x, x) = 0", x.clone(), 0.0, 2 * tr)]
    for a in (0.5, 2.0):
        cases.append(("FD(x, %g x)" % a, x * a, (1 - a) ** 2 * (tr + mm), (1 + a * a) * tr))
    for name, x2, want, traces in cases:
        assert torch.equal((x2.to(F64) - x64), (x2 - x).to(F64)), "the relation between the two sets is exact in f32"
        tally.add_ratio("random", name, abs(impl.frechet(x, x2) - want) / (fac * traces))
    # against the fp64 oracle: d = 2 with n = 2; a zero-variance column in both sets
    g = _gen(29)
    a2, b2 = torch.randn(2, 2, generator=g), torch.randn(2, 2, generator=g)
    az, bz = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g) * 1.5 + 0.2
    az[:, 3], bz[:, 3] = 0.5, -1.25
    for name, p, q in (("d 2 n 2", a2, b2), ("zero-variance column", az, bz)):
        dd = p.shape[1]
        want = float(IO.frechet_distance(p.to(F64), q.to(F64)))
        traces = float(torch.trace(IO.cov(p.to(F64))) + torch.trace(IO.cov(q.to(F64))))
        tally.add_ratio("random", name, abs(impl.frechet(p, q) - want) / (SLACK * dd * (EIG_STOP + EIG_SWEEPS * dd * U) * traces))


# =====================================================================================================================================
# the sweeps, by kernel
# =====================================================================================================================================
def run_all(impl, which):
    """runs the sweeps named in `which` and returns {tally name: Tally}"""
    T = {}
    mk = lambda name: T.setdefault(name, Tally(name))
    if "conv3d" in which:
        sweep_conv3d(impl, mk("conv3d"))
    if "pack_conv3d" in which:
        sweep_pack(impl, mk("pack_conv3d"))
    if "maxpool" in which:
        sweep_maxpool(impl, mk("maxpool3d_same"))
    if "reduce" in which:
        sweep_reduce(impl, mk("avgpool_thw"), mk("time_mean"), mk("ncthw_to_nthwc"))
    if "preprocess" in which:
        sweep_preprocess(impl, mk("fvd_preprocess"))
    if "moments" in which:
        sweep_moments(impl, mk("fd_moments"))
    if "sym_eig" in which:
        sweep_sym_eig(impl, mk("sym_eig"))
    if "frechet" in which:
        sweep_frechet(impl, mk("frechet_distance"))
    return T


KERNELS = ["conv3d", "pack_conv3d", "maxpool", "reduce", "preprocess", "moments", "sym_eig", "frechet"]


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------
def test_same_pad_rule_cpu():
    """the restated host rule gives the oracle's output sizes, on both of its branches"""
    for size in range(1, 20):
        for k in (1, 2, 3, 7):
            for s in (1, 2, 3):
                want = IO.maxpool_same(torch.zeros(1, 1, size, 1, 1), (k, 1, 1), (s, 1, 1)).shape[2]
                assert same_pad_rule(size, k, s)[0] == want, (size, k, s)
    assert [same_pad_rule(same_pad_rule(T, 7, 2)[0], 3, 2)[0] for T in (10, 13, 16)] == [3, 4, 4]


@pytest.mark.parametrize("kernel", KERNELS)
def test_emulation_cpu(kernel):
    """the emulation of each kernel passes its judge on every case and both data classes (and the exact-class premises hold)"""
    for t in run_all(Emu(), [kernel]).values():
        t.check(report=False)


# defect -> the sweeps whose judges must reject it (the tallies of those sweeps that see the defective code)
MUTATIONS = {"pad_front_is_back": {"conv3d": ["conv3d"], "maxpool": ["maxpool3d_same"]},                  # front pad p - p / 2 instead of p / 2
             "pad_no_mod_branch": {"conv3d": ["conv3d"], "maxpool": ["maxpool3d_same"]},                  # the size % s branch dropped
             "pool_pad_neg_inf": {"maxpool": ["maxpool3d_same"]},                                          # -inf instead of 0 padding
             "conv_coff_shift": {"conv3d": ["conv3d"]},                                                    # the slice one channel off
             "conv_tile_last_position": {"conv3d": ["conv3d"]},                                            # last position of a tile dropped
             "conv_last_cout": {"conv3d": ["conv3d"]},                                                     # last Cout element dropped
             "pre_align_corners": {"preprocess": ["fvd_preprocess"]},
             "pre_crop_off_by_one": {"preprocess": ["fvd_preprocess"]},
             "pre_floor_side": {"preprocess": ["fvd_preprocess"]},                                         # floor instead of ceil of the scaled side
             "cov_div_n": {"moments": ["fd_moments"], "frechet": ["frechet_distance"]},
             "jacobi_one_sweep": {"sym_eig": ["sym_eig"], "frechet": ["frechet_distance"]},
             "eig_vectors_transposed": {"sym_eig": ["sym_eig"], "frechet": ["frechet_distance"]},
             "frechet_nan_at_n2": {"frechet": ["frechet_distance"]}}                                       # NaN for the rank-1 case only
# classes in which a defect cannot show: the scale-1 preprocess case has nothing to round up or crop
MUT_BLIND = {("pre_floor_side", "fvd_preprocess", "exact"), ("pre_align_corners", "fvd_preprocess", "exact")}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judges_reject_cpu(mut):
    """each defect of the emulation is outside every judge that sees it, in every data class that judge has (the sound emulation is
    inside: test_emulation_cpu)"""
    for sweep, names in MUTATIONS[mut].items():
        T = run_all(Emu(mut), [sweep])
        for name in names:
            rej = {c: r for c, r in T[name].rejected().items() if (mut, name, c) not in MUT_BLIND}
            print("[i3d_kernels] mutation %-24s %-18s %s" % (mut, name, {c: "%.3g" % T[name].worst[c][0] for c in rej}))
            assert rej and all(rej.values()), "the judge of %s accepts the defect %s in the class(es) %s" % (name, mut, [c for c, r in rej.items() if not r])


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_against_fp64(ctx, kernel):
    for t in run_all(Gpu(ctx), [kernel]).values():
        t.check(report=True)


@gpu
def test_refusals(ctx):
    """the argument checks of the hooks: the call returns non-zero, the outputs stay NaN, and the next valid call on the context is right.
    Every buffer is sized for the shape requested: nothing depends on a guard for memory safety."""
    impl = Gpu(ctx)
    nan = lambda n, dt=F32: torch.full((n,), NAN, device="cuda", dtype=dt)
    untouched = lambda *ts: all(bool(torch.isnan(t).all()) for t in ts)
    P = lambda t: t.data_ptr()
    x, w, o3 = torch.randn(1, 3, 5, 6, 8, device="cuda"), torch.randn(16, 27, 8, device="cuda"), i3((-1, -1, -1))
    y = nan(3 * 5 * 6 * 16)
    k3, s1 = i3((3, 3, 3)), i3((1, 1, 1))
    # y one element short of the output; a slice that runs past ldc; input channels that are no multiple of 4
    assert impl.refused("svg_op_conv3d", P(x), 1, 3, 5, 6, 8, P(w), None, P(y), y.numel() - 1, 16, 16, 0, k3, s1, 1, o3) and untouched(y)
    assert impl.refused("svg_op_conv3d", P(x), 1, 3, 5, 6, 8, P(w), None, P(y), y.numel(), 16, 16, 1, k3, s1, 1, o3) and untouched(y)
    assert impl.refused("svg_op_conv3d", P(x), 1, 3, 5, 8, 6, P(w), None, P(y), y.numel(), 16, 16, 0, k3, s1, 1, o3) and untouched(y)
    assert tuple(o3) == (-1, -1, -1)
    yp = nan(3 * 5 * 6 * 8)
    assert impl.refused("svg_op_maxpool3d_same", P(x), P(yp), yp.numel() - 1, 1, 3, 5, 6, 8, k3, s1, o3) and untouched(yp)
    assert impl.refused("svg_op_maxpool3d_same", P(x), P(yp), yp.numel(), 1, 3, 5, 8, 6, k3, s1, o3) and untouched(yp)
    e = torch.randn(4, 6, device="cuda")
    m, c = nan(6, F64), nan(36, F64)
    assert impl.refused("svg_op_fd_moments", P(e), 1, 6, P(m), P(c)) and impl.refused("svg_op_fd_moments", P(e), 8, 3, P(m), P(c)) and untouched(m, c)
    A = torch.eye(3, device="cuda", dtype=F64)
    assert impl.refused("svg_op_sym_eig", P(A), 3, P(m), P(c)) and untouched(m, c)
    for which in ("conv3d", "maxpool", "moments", "sym_eig"):
        for t in run_all(impl, [which]).values():
            t.check(report=False)


# ---- the network off its one tested shape ---------------------------------------------------------------------------------------------
W_SEED, X_SEED = 17, 23


@pytest.fixture(scope="module")
def i3d(ctx):
    from sd_video_gen_amd import fvd
    return fvd.I3D(IO.seeded_i3d_weights(W_SEED), ctx)


@gpu
@pytest.mark.parametrize("T", [10, 13])
def test_network_odd_clip_length(ctx, i3d, T):
    """clip lengths whose time axis takes the `size % stride != 0` branch of the padding rule, in convs and pools, per element"""
    sd = IO.seeded_i3d_weights(W_SEED)
    x = IO.seeded_clips(X_SEED, T)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    try:
        with torch.no_grad():
            ref64 = IO.i3d_forward({k: v.double() for k, v in sd.items()}, x.double())
            ref32 = IO.i3d_forward(sd, x)
    finally:
        torch.set_num_threads(threads)
    got = i3d(x.cuda()).cpu()
    assert got.shape == (1, 400) and bool(torch.isfinite(got).all())
    margin("I3D logits, %d-frame clip, vs the oracle in float64" % T, rel_l2(got, ref64), 2e-5)
    d32, dlib = float((ref32.double() - ref64).abs().max()), float((got.double() - ref64).abs().max())
    # the f32 oracle's own distance: within the project's 2e-5 of the largest logit, or the measure below means nothing
    margin("I3D logits, %d-frame clip: f32 CPU oracle vs float64, per element" % T, d32, 2e-5 * float(ref64.abs().max()), unit="max-abs")
    margin("I3D logits, %d-frame clip: library vs float64, per element (4 x the f32 oracle's)" % T, dlib, 4 * d32, unit="max-abs")


@gpu
def test_network_rows_are_independent_of_the_batch(ctx, i3d):
    """B = 3 clips of 10 frames (position counts that are no multiples of 64 at several layers): row 1 is the clip run alone, bit for bit"""
    x = IO.seeded_clips(X_SEED, 10, B=3).cuda()
    both = i3d(x).cpu()
    alone = i3d(x[1:2].contiguous()).cpu()
    assert bool(torch.isfinite(both).all()) and torch.equal(both[1], alone[0])
    assert not torch.equal(both[0], both[1])
