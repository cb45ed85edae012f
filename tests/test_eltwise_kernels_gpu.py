"""The VAE / UNet boundary kernels (csrc/eltwise.hip, and add_noise of csrc/sampler.hip) one by one against fp64, element by element.

Each kernel is driven alone through its operator-level hook (svg_op_img_to_act, svg_op_act_to_img, svg_op_nchw_to_act, svg_op_nchw_to_actf32,
svg_op_actf32_pad_h16, svg_op_actf32_to_nchw, svg_op_pixel_linear_f32, svg_op_vae_sample, svg_op_concat_channels, svg_op_f32_to_h16,
svg_op_f32_to_h16_x8, svg_op_h16_to_f32, svg_op_timestep_embed, svg_op_add_noise) or its existing entry point (svg_resize_nearest_u8,
svg_resize_bilinear_f32).  The hooks check their arguments and call the launcher the models call.  Every output buffer is filled with NaN
(0xAB bytes for u8) and carries a guard of the same fill behind it that must be untouched afterwards; every element is judged, none left out
(a non-finite or missing element counts as inf).  The worst err / bound per kernel and data class goes through
conftest.margin(..., tol=1.0, unit="err/bound").  Kernels with a 16-bit side run in bf16 and in fp16 storage.  No NaN is fed: the build
uses -fno-honor-nans, so what the clamps do with one is not specified.  Each kernel has a handful of tiny shapes (N in {1, 3}; 1x1, 3x5,
16x24) and one case whose item count exceeds its launcher's grid cap (8192 x 256 items; 4096 x 256 for the bilinear resize), so that
the grid-stride loop takes a second trip.

CONSTANTS   E = 2^-24 (f32 unit roundoff).  u16 = 2^-9 (bf16) / 2^-12 (fp16).  SLACK = 1.01 on every derived bound, for the products of
two of its terms.  FN = 4 E relative: 2 ulp for a device transcendental (expf, sinf, cosf), the figure tests/test_ff_fused_gpu.py takes
for rsqrtf (no HIP math accuracy table is installed beside the compiler).  No constant here was fitted to what the GPU returns.

THE 16-BIT OUTPUT ROUNDING   h(v) = u16 2^(floor(log2 v) + 1), at least tiny (2^-134 bf16 / 2^-25 fp16: half the spacing of the subnormals):
half an ulp of the storage type at magnitude v.  A kernel whose f32 value is within d of the reference y may store anything within
d + h(|y| + d) of y.  h(v) lies between u16 v (top of a binade) and 2 u16 v (bottom).  The plain product u16 |y| is NOT used as the
bound, and that is deliberate: round-to-nearest-even itself misses it in the lower half of every binade (1 + 2^-8 stores as 1 or
1 + 2^-7 in bf16, 2^-8 away, while u16 |y| is 2^-9 (1 + 2^-8)); test_half_ulp_rule_cpu shows that torch's own conversion exceeds u16 |y|
and attains h(|y|) to the bit.  h is the exact statement of the number format, never wider than one half-ulp.  Because a correct
conversion attains it, the 16-bit random-class ratios sit just below 1 (0.999) on a few thousand elements: that is the rounding, not a
thin margin of the f32 arithmetic in front of it (the f32 twin nchw_to_actf32 shows that part alone).  The same two kernels are
also held to the sharper form inside16(): the stored value lies between the stored values of y - d and y + d, which fixes the bits of
every element whose interval holds no rounding boundary.

TWO DATA CLASSES
  exact    bound 0: bit equality (the sign of zero included) on any data.
  random   unit-scale normal data unless said otherwise, fp64 reference on the same f32 inputs, judged by the bounds below.

EXACT CLASS
  nchw_to_act, nchw_to_actf32 at scale 1 (x 1.0 is exact, then one round-to-nearest-even conversion: torch's .to(dtype)), C in {3, 4, 8} to
  Cpad 8, pad channels exactly +0; actf32_pad_h16; actf32_to_nchw with ld in {4, 8, 16} for C = 4, the unused columns holding 1e30;
  concat_channels at (Ca, Cb) in {(8,8), (8,312), (320,8), (640,320)}; h16_to_f32 on every non-NaN 16-bit pattern.
  f32_to_h16, f32_to_h16_x8   against torch's .to(dtype) on: normal draws over 24 binades, exact ties (the f32 midpoint of two neighbours of
      the 16-bit type, and the f32 neighbours of that midpoint), the largest finite value, the overflow threshold (the midpoint between
      the largest finite value and 2^emax+1: the tie goes to the even side, infinity) and its f32 neighbours, FLT_MAX, and for fp16 the
      subnormal range (2^-25 and its neighbours, 3 x 2^-25, draws down to 2^-27).  The two forms agree bit for bit.
  img_to_act      all 256 byte values in each channel; the f32 chain of oracle/sd_oracle.py::encode_img (p / 255 in f32: the kernel's
      division is IEEE, 2 (x - 0.5) exact after it, one conversion); channels 3..7 exactly +0; with (sh, sw) != (H, W) the source pixel of
      torch's F.interpolate(mode='nearest') (what oracle.sd_oracle.resize_nearest_u8 calls; test_nearest_rule_cpu ties the two) at
      37 -> 16, 16 -> 37, 240 -> 64, 26 -> 22 and a non-square pair.  26 -> 22 is a pair where the float rule floor(d (float)(in / out))
      and the integer rule d in / out differ (1218 such pairs exist up to 256; found on the CPU).
  act_to_img, u8  bit for bit against the reference's f32 chain (decode_img_latents: (x / 2 + 0.5).clamp(0, 1) * 255, round half to even):
      x / 2 is exact, so an FMA contraction of the first step changes nothing.  Random data in [-1.5, 1.5]; the clamp edges; a tie set
      found on the CPU (f32 inputs around 2 ((k + 0.5) / 255 - 0.5) whose f32 product is exactly k + 0.5, for even and for odd k: the
      only inputs that tell half-to-even from half-up).  float_out is the bit-exact NCHW transpose at (h, w) whatever (oh, ow) is.
  svg_resize_nearest_u8 with C in {1, 3, 4} at the size pairs above; svg_resize_bilinear_f32 at equal sizes (weights 1 and 0).
  vae_sample      mom_nchw is the transpose of the moments as they came (logvar NOT clamped); with eps = NULL z is the one f32 product
      mean x 0.18215f, bit for bit.  pixel_linear_f32 on small integers.  timestep_embed at t = 0: [1 .. | +0 ..].

BOUNDS (random class; y the fp64 reference)
  act_to_img, second opinion   v = clamp(x / 2 + 0.5, 0, 1) 255 in fp64.  The f32 chain has two roundings below 1 and one below 256:
      at most 2 x 255 E from v.  Further than that from a half-integer the stored byte must be round(v); inside the band either
      neighbour.  The share of random-class elements inside the band is capped at 1e-3 (expected 2 x 2 x 255 E = 6e-5).
  nchw_to_act, nchw_to_actf32 at scale (float)(1 / 0.18215f)   one f32 product: d = E |y|; 16-bit output: d + h(|y| + d).
  pixel_linear_f32   (Cin + 2) E (sum |w||x| + |b|) + E |y|, in any summation order, with or without FMA contraction.  The bias is inside
      the magnitude sum because the kernel starts its accumulator from it: each of the Cin additions then rounds at a magnitude that
      includes |b|, up to Cin E |b| in all, which E |y| does not cover where the products cancel or are small next to the bias.  (The
      plain form (Cin + 2) E sum |w||x| + E |y| holds only for a bias added last; the f32 emulation, bias first, reaches 1.43 x it.)
  vae_sample   z = 0.18215 (mean + s), s = exp(0.5 clamp(lv, -30, 20)) eps (0.5 lv is exact).  On s: expf 4 E, the product with eps E; then
      on both terms the sum E (none under FMA contraction), the constant's own rounding E, the final product E: 8 E |s| + 3 E |mean|,
      taken as k E 0.18215 (|mean| + |s|) with k = 8.  The logvars -40, -30, -29.999, 0, 19.999, 20 and 25 sit on elements with mean 0
      (every second one), where the bound is relative to |s| alone.
  timestep_embed   a = t exp(x), x = -ln(10000) i / half, |x| < 9.22.  x carries the constant's rounding and two more (product, quotient):
      3 E |x| <= 27.7 E absolute, which is the relative error it leaves on exp(x); expf 4 E; the product with t E: 32.7 E, taken as
      33 E |a|.  cos and sin are 1-Lipschitz: 33 E |a| + FN |y| = d; stored within d + h(|y| + d).
  add_noise    3 E (|sa x0| + |s1a nz|): two products and a sum.
  svg_resize_bilinear_f32   as fvd_preprocess in tests/test_i3d_kernels_gpu.py, for unnormalised data: the interpolant is continuous
      and piecewise linear; per axis its slope is at most the largest difference L of neighbours along that axis in the plane.  The f32
      source coordinate (i + 0.5) (h / oh) - 0.5 has three roundings below max(h, w): delta = 4 E max(h, w).  Bound: delta (Lx + Ly) +
      4 E max |x| per plane.  A constant plane comes out within 2 E |c|.

The CPU half (not marked gpu) pushes a torch-f32 emulation of each kernel through the same data and the same judges, and
test_judges_reject_cpu requires the judges to reject the defects listed in MUTATIONS."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import margin
from oracle import sd_oracle as SO

gpu = pytest.mark.gpu
E = 2.0 ** -24
FN = 4 * E
PAD = 4096
SLACK = 1.01
F64, F32, U8 = torch.float64, torch.float32, torch.uint8
NAN, INF = float("nan"), float("inf")
SENTINEL = 1e30                                              # what unused columns of an input hold: finite, and ruinous if read
GRID_CAP, BILINEAR_CAP = 8192 * 256, 4096 * 256              # items one trip of the grid-stride loop covers
BIG_HW = 1456                                                # 1456 x 1456 = 2 119 936 pixels > GRID_CAP
S32 = float(np.float32(0.18215))                             # 0.18215f
INV_S32 = float(np.float32(1.0) / np.float32(0.18215))       # 1.f / 0.18215f as the VAE decoder passes it
LN1E4_32 = float(np.float32(math.log(10000.0)))
NEAREST_PAIRS = [(37, 16), (16, 37), (240, 64), (26, 22)]
SPECIAL_LOGVARS = [-40.0, -30.0, -29.999, 0.0, 19.999, 20.0, 25.0]
TIMESTEPS = [0.0, 1.0, 20.5, 500.0, 998.7, 999.0]
BAND_SHARE_CAP = 1e-3


class Half:
    def __init__(self, name, dtype, suffix, u16, tiny, top):
        self.name, self.dtype, self.suffix, self.u16, self.tiny, self.top = name, dtype, suffix, u16, tiny, top


HALVES = {"bf16": Half("bf16", torch.bfloat16, "", 2.0 ** -9, 2.0 ** -134, 2.0 ** 128),
          "fp16": Half("fp16", torch.float16, "_f16", 2.0 ** -12, 2.0 ** -25, 2.0 ** 16)}


def f32c(v):
    return torch.tensor(v, dtype=F32)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def exact(got, want):
    """0 if got is want bit for bit (shape and type included), else inf"""
    ok = got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want))
    return 0.0 if ok else INF


def ratio(got, want, bound):
    """worst err / bound of one output; a bound of 0 asks for equality; inf for a wrong shape or a non-finite or missing element"""
    o = got.detach().cpu().to(F64)
    if o.shape != want.shape or not bool(torch.isfinite(o).all()):
        return INF
    if o.numel() == 0:
        return 0.0
    err = (o - want).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    return float(torch.where(err == 0, torch.zeros_like(err), err / b).max())


def half_ulp16(v, H):
    """h(v): half an ulp of the storage type at magnitude v >= 0 (fp64 tensor), at least half the spacing of its subnormals"""
    _, e = torch.frexp(v)                                                 # v = m 2^e, m in [0.5, 1): 2^e = 2^(floor(log2 v) + 1)
    h = torch.ldexp(torch.full_like(v, H.u16), e)
    return torch.where(v > 0, h, torch.zeros_like(v)).clamp_min(H.tiny)


def bound16(y, d, H):
    """the stored 16-bit value of an f32 value within d of y"""
    return d + half_ulp16(y.abs() + d, H)


def inside16(got, y, d, H):
    """the same statement without the triangle inequality: rounding is monotone, so the stored value of an f32 value within d of y lies
    between the stored values of y - d and y + d (where the two agree, the bits are fixed).  0 if every element does, else inf.  d is
    widened by E |y| for the f32 step on the way from fp64 to the storage type."""
    o = got.detach().cpu().to(F64)
    if o.shape != y.shape or not bool(torch.isfinite(o).all()):
        return INF
    dd = d + E * y.abs()
    lo, hi = (y - dd).float().to(H.dtype).to(F64), (y + dd).float().to(H.dtype).to(F64)
    return 0.0 if bool(((o >= lo) & (o <= hi)).all()) else INF


class Tally:
    """the worst err / bound per data class of one kernel, with the case it came from"""

    def __init__(self, kernel):
        self.kernel, self.worst = kernel, {}

    def add_ratio(self, cls, label, r):
        r = float(r)
        if not math.isfinite(r):                                        # a NaN compares false with everything: it is the worst there is
            r = INF
        if r >= self.worst.get(cls, (-1.0, ""))[0]:
            self.worst[cls] = (r, label)

    def check(self, report, tag=""):
        assert self.worst, "%s: nothing was judged" % self.kernel
        for cls, (r, label) in sorted(self.worst.items()):
            print("[eltwise_kernels] %-22s %-5s %-7s worst err/bound %.3f at %s" % (self.kernel, tag, cls, r, label))
            if report:
                margin("eltwise kernel %s%s, %s class" % (self.kernel, " " + tag if tag else "", cls), r, 1.0, unit="err/bound")
            else:
                assert r < 1.0, "%s %s: err/bound %.3g at %s" % (self.kernel, cls, r, label)
            if cls == "exact":
                assert r == 0.0, "%s: the exact class is not bit-equal at %s" % (self.kernel, label)

    def rejected(self):
        return {cls: r >= 1.0 for cls, (r, _) in self.worst.items()}


@functools.lru_cache(maxsize=None)
def oracle_src(n_in, n_out):
    """source index of every destination index under torch's F.interpolate(mode='nearest'): the rule of oracle.sd_oracle.resize_nearest_u8"""
    return F.interpolate(torch.arange(n_in, dtype=F32).view(1, 1, n_in, 1), (n_out, 1)).view(-1).long()


def gather_hw(x, sy, sx):
    """x (N,h,w,...) -> (N,len(sy),len(sx),...)"""
    return x[:, sy][:, :, sx]


# =====================================================================================================================================
# The two implementations behind one interface: the HIP kernels through their hooks, and the torch emulation (with its defects)
# =====================================================================================================================================
def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


class Gpu:
    mut = None

    def __init__(self, ctx, H):
        self.ctx, self.lib, self.H = ctx, ctx.lib, H

    def out(self, n, dtype):
        return torch.full((n + PAD,), 0xAB if dtype == U8 else NAN, device="cuda", dtype=dtype)

    def take(self, o, shape):
        torch.cuda.synchronize()
        n = int(np.prod(shape))
        guard = o[n:]
        assert bool((guard == 0xAB).all() if o.dtype == U8 else torch.isnan(guard).all()), "the guard behind an output was written"
        return o[:n].cpu().reshape(shape)

    def fn(self, name, h16):
        return getattr(self.lib, name + (self.H.suffix if h16 else ""))

    def call(self, name, h16, *args):
        self.ctx.check(self.fn(name, h16)(self.ctx.h, *args, stream()), name)

    def refused(self, name, h16, *args):
        rc = self.fn(name, h16)(self.ctx.h, *args, stream())
        torch.cuda.synchronize()
        return rc != 0 and len(self.lib.svg_last_error(self.ctx.h)) > 0

    def img_to_act(self, img, Ho, Wo):
        N, sh, sw, _ = img.shape
        d, o = img.contiguous().cuda(), self.out(N * Ho * Wo * 8, self.H.dtype)
        self.call("svg_op_img_to_act", True, P(d), P(o), N, sh, sw, Ho, Wo)
        return self.take(o, (N, Ho, Wo, 8))

    def act_to_img(self, x, oh, ow, want_img, want_float):
        N, h, w, ldc = x.shape
        d = x.contiguous().cuda()
        img = self.out(N * oh * ow * 3, U8) if want_img else None
        fo = self.out(N * 3 * h * w, F32) if want_float else None
        self.call("svg_op_act_to_img", False, P(d), ldc, P(img), P(fo), N, h, w, oh, ow)
        return (self.take(img, (N, oh, ow, 3)) if want_img else None), (self.take(fo, (N, 3, h, w)) if want_float else None)

    def nchw_to_act(self, x, Cpad, scale):
        N, C, h, w = x.shape
        d, o = x.contiguous().cuda(), self.out(N * h * w * Cpad, self.H.dtype)
        self.call("svg_op_nchw_to_act", True, P(d), P(o), N, C, h, w, Cpad, scale)
        return self.take(o, (N, h, w, Cpad))

    def nchw_to_actf32(self, x, scale):
        N, C, h, w = x.shape
        d, o = x.contiguous().cuda(), self.out(N * h * w * C, F32)
        self.call("svg_op_nchw_to_actf32", False, P(d), P(o), N, C, h, w, scale)
        return self.take(o, (N, h, w, C))

    def actf32_pad_h16(self, x, Cpad):
        Pn, C = x.shape
        d, o = x.contiguous().cuda(), self.out(Pn * Cpad, self.H.dtype)
        self.call("svg_op_actf32_pad_h16", True, P(d), C, P(o), Cpad, Pn)
        return self.take(o, (Pn, Cpad))

    def actf32_to_nchw(self, x, C):
        N, h, w, ld = x.shape
        d, o = x.contiguous().cuda(), self.out(N * C * h * w, F32)
        self.call("svg_op_actf32_to_nchw", False, P(d), ld, P(o), N, C, h, w)
        return self.take(o, (N, C, h, w))

    def pixel_linear(self, x, w, b, ldy):
        Pn, ldx = x.shape
        Cout, Cin = w.shape
        d, wd, bd, o = x.contiguous().cuda(), w.contiguous().cuda(), None if b is None else b.contiguous().cuda(), self.out(Pn * ldy, F32)
        self.call("svg_op_pixel_linear_f32", False, P(d), ldx, P(wd), P(bd), P(o), ldy, Pn, Cin, Cout)
        return self.take(o, (Pn, ldy))

    def vae_sample(self, mom, eps, want_mom):
        N, h, w, ldm = mom.shape
        d, ed = mom.contiguous().cuda(), None if eps is None else eps.contiguous().cuda()
        z, mo = self.out(N * 4 * h * w, F32), self.out(N * 8 * h * w, F32) if want_mom else None
        self.call("svg_op_vae_sample", False, P(d), ldm, P(ed), P(z), P(mo), N, h, w)
        return self.take(z, (N, 4, h, w)), (self.take(mo, (N, 8, h, w)) if want_mom else None)

    def concat(self, a, b):
        Pn, Ca, Cb = a.shape[0], a.shape[1], b.shape[1]
        ad, bd, o = a.contiguous().cuda(), b.contiguous().cuda(), self.out(Pn * (Ca + Cb), self.H.dtype)
        self.call("svg_op_concat_channels", True, P(ad), Ca, P(bd), Cb, P(o), Pn)
        return self.take(o, (Pn, Ca + Cb))

    def f32_to_h16(self, x, x8):
        d, o = x.contiguous().cuda(), self.out(x.numel(), self.H.dtype)
        self.call("svg_op_f32_to_h16_x8" if x8 else "svg_op_f32_to_h16", True, P(d), P(o), x.numel())
        return self.take(o, (x.numel(),))

    def h16_to_f32(self, x):
        d, o = x.contiguous().cuda(), self.out(x.numel(), F32)
        self.call("svg_op_h16_to_f32", True, P(d), P(o), x.numel())
        return self.take(o, (x.numel(),))

    def timestep_embed(self, t, dim):
        d, o = t.contiguous().cuda(), self.out(t.numel() * dim, self.H.dtype)
        self.call("svg_op_timestep_embed", True, P(d), P(o), t.numel(), dim)
        return self.take(o, (t.numel(), dim))

    def add_noise(self, x0, nz, sa, s1a, inplace):
        n = x0.numel()
        nd, o = nz.contiguous().cuda(), self.out(n, F32)
        if inplace:
            o[:n] = x0.cuda()
            xd = o
        else:
            xd = x0.contiguous().cuda()
        self.call("svg_op_add_noise", False, P(xd), P(nd), P(o), n, sa, s1a)
        return self.take(o, (n,))

    def resize_nearest(self, img, dh, dw):
        N, sh, sw, C = img.shape
        d, o = img.contiguous().cuda(), self.out(N * dh * dw * C, U8)
        self.call("svg_resize_nearest_u8", False, P(d), N, sh, sw, C, P(o), dh, dw)
        return self.take(o, (N, dh, dw, C))

    def resize_bilinear(self, x, oh, ow):
        Pn, h, w = x.shape
        d, o = x.contiguous().cuda(), self.out(Pn * oh * ow, F32)
        self.call("svg_resize_bilinear_f32", False, P(d), Pn, h, w, P(o), oh, ow)
        return self.take(o, (Pn, oh, ow))


class Emu:
    """torch f32 on the CPU, operation by operation as the kernels state them; mut: one defect (MUTATIONS)"""

    def __init__(self, H, mut=None):
        self.H, self.mut = H, mut

    def src(self, n_in, n_out, skip_equal):
        """nearest_src of eltwise.hip: floor(d * ((float)in / (float)out)) in f32, capped at in - 1"""
        d = torch.arange(n_out)
        if skip_equal and n_in == n_out:
            return d
        if self.mut == "nearest_int_rule":
            return (d * n_in) // n_out
        return torch.floor(d.float() * (f32c(float(n_in)) / f32c(float(n_out)))).long().clamp_max(n_in - 1)

    def img_to_act(self, img, Ho, Wo):
        N, sh, sw, _ = img.shape
        s = gather_hw(img, self.src(sh, Ho, True), self.src(sw, Wo, True)).float()
        v = 2.0 * (s / f32c(256.0 if self.mut == "img_div_256" else 255.0) - 0.5)
        o = torch.zeros(N, Ho, Wo, 8, dtype=self.H.dtype)
        o[..., :3] = v.to(self.H.dtype)
        if self.mut == "img_pad_nonzero":
            o[..., 7] = 2.0 ** -14
        return o

    def act_to_img(self, x, oh, ow, want_img, want_float):
        N, h, w, _ = x.shape
        img = None
        if want_img:
            v = (x[..., :3] / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0
            r = torch.floor(v + 0.5) if self.mut == "act_half_up" else torch.round(v)
            img = gather_hw(r.to(U8), self.src(h, oh, True), self.src(w, ow, True)).contiguous()
        return img, (x[..., :3].permute(0, 3, 1, 2).contiguous() if want_float else None)

    def nchw_to_act(self, x, Cpad, scale):
        N, C, h, w = x.shape
        o = torch.zeros(N, h, w, Cpad, dtype=self.H.dtype)
        o[..., :C] = (x * f32c(scale)).permute(0, 2, 3, 1).to(self.H.dtype)
        return o

    def nchw_to_actf32(self, x, scale):
        return (x * f32c(scale)).permute(0, 2, 3, 1).contiguous()

    def actf32_pad_h16(self, x, Cpad):
        o = torch.zeros(x.shape[0], Cpad, dtype=self.H.dtype)
        o[:, :x.shape[1]] = x.to(self.H.dtype)
        return o

    def actf32_to_nchw(self, x, C):
        N, h, w, ld = x.shape
        if self.mut == "nchw_ld_ignored":
            x = x.reshape(-1)[:N * h * w * C].reshape(N, h, w, C)
        return x[..., :C].permute(0, 3, 1, 2).contiguous()

    def pixel_linear(self, x, w, b, ldy):
        Cout, Cin = w.shape
        acc = torch.zeros(x.shape[0], Cout) if (b is None or self.mut == "linear_no_bias") else b[None, :].expand(x.shape[0], Cout).clone()
        for i in range(Cin):
            acc = acc + w[None, :, i] * x[:, i:i + 1]
        y = torch.full((x.shape[0], ldy), NAN)
        y[:, :Cout] = acc
        return y

    def vae_sample(self, mom, eps, want_mom):
        mean, raw = mom[..., 0:4], mom[..., 4:8]
        lv = raw if self.mut == "vae_no_clamp" else raw.clamp(-40.0 if self.mut == "vae_clamp_low_40" else -30.0, 30.0 if self.mut == "vae_clamp_30" else 20.0)
        c = f32c(S32)
        if eps is None:
            z = mean * c
        else:
            s = torch.exp(0.5 * lv) * eps.permute(0, 2, 3, 1)
            z = mean * c + s if self.mut == "vae_scale_mean_only" else (mean + s) * c
        mo = torch.cat([mean, lv if self.mut == "vae_mom_clamped" else raw], -1).permute(0, 3, 1, 2).contiguous() if want_mom else None
        return z.permute(0, 3, 1, 2).contiguous(), mo

    def concat(self, a, b):
        o = torch.cat([a, b], 1)
        if self.mut == "concat_off_by_8":
            o[:, a.shape[1] - 8:a.shape[1]] = b[:, :8]
        return o

    def f32_to_h16(self, x, x8):
        if self.mut == "h16_truncate":
            keep = -65536 if self.H.name == "bf16" else -8192                   # drop the f32 mantissa bits the type does not hold
            x = (bits(x) & keep).view(F32)
        return x.to(self.H.dtype)

    def h16_to_f32(self, x):
        return x.float()

    def timestep_embed(self, t, dim):
        half = dim // 2
        den = f32c(float(half - 1 if self.mut == "ts_half_minus_1" else half))
        freq = torch.exp(-f32c(LN1E4_32) * torch.arange(half, dtype=F32) / den)
        a = t[:, None] * freq[None, :]
        parts = [torch.sin(a), torch.cos(a)] if self.mut == "ts_swap" else [torch.cos(a), torch.sin(a)]
        return torch.cat(parts, 1).to(self.H.dtype)

    def add_noise(self, x0, nz, sa, s1a, inplace):
        if self.mut == "noise_swapped":
            sa, s1a = s1a, sa
        return f32c(sa) * x0 + f32c(s1a) * nz

    def resize_nearest(self, img, dh, dw):
        return gather_hw(img, self.src(img.shape[1], dh, False), self.src(img.shape[2], dw, False)).contiguous()

    def resize_bilinear(self, x, oh, ow):
        Pn, h, w = x.shape
        idx = []
        for size, out in ((h, oh), (w, ow)):
            o = torch.arange(out, dtype=F32)
            if self.mut == "bilinear_align_corners":
                f = o * f32c((size - 1) / max(out - 1, 1))
            else:
                f = (o + 0.5) * (f32c(float(size)) / f32c(float(out))) - 0.5
                if self.mut != "bilinear_no_max":
                    f = f.clamp_min(0.0)
            i0 = f.trunc().long().clamp_max(size - 1)
            idx.append((i0, (i0 + 1).clamp_max(size - 1), f - i0.float()))
        (y0, y1, ly), (x0, x1, lx) = idx
        ly, lx = ly[:, None], lx[None, :]
        top = x[:, y0][:, :, x0] * (1.0 - lx) + x[:, y0][:, :, x1] * lx
        bot = x[:, y1][:, :, x0] * (1.0 - lx) + x[:, y1][:, :, x1] * lx
        return top * (1.0 - ly) + bot * ly


# =====================================================================================================================================
# img_to_act, svg_resize_nearest_u8
# =====================================================================================================================================
def all_bytes_image():
    """(1,16,16,3): every byte value once per channel, in a different order in each"""
    v = torch.arange(256)
    return torch.stack([(v * (2 * c + 1) + 85 * c) % 256 for c in range(3)], -1).to(U8).reshape(1, 16, 16, 3)


def ref_img_to_act(img, Ho, Wo, H):
    s = gather_hw(img, oracle_src(img.shape[1], Ho), oracle_src(img.shape[2], Wo))
    x = 2 * ((s / 255.0).float() - 0.5)                                       # oracle/sd_oracle.py::encode_img, in f32
    want = torch.zeros(img.shape[0], Ho, Wo, 8, dtype=H.dtype)
    want[..., :3] = x.to(H.dtype)
    return want


def sweep_img_to_act(impl, T, big):
    cases = [("all bytes", all_bytes_image(), 16, 16)]
    for (N, sh, sw, Ho, Wo) in [(3, 3, 5, 3, 5), (1, 1, 1, 1, 1), (1, 16, 24, 16, 24), (1, 37, 16, 16, 37)] + [(3 if a == 16 else 1, a, a, b, b) for a, b in NEAREST_PAIRS]:
        cases.append(("%dx%dx%d -> %dx%d" % (N, sh, sw, Ho, Wo), torch.randint(0, 256, (N, sh, sw, 3), dtype=U8, generator=_gen(31, N, sh, sw, Ho)), Ho, Wo))
    if big:
        cases.append(("second trip", torch.randint(0, 256, (1, BIG_HW, BIG_HW, 3), dtype=U8, generator=_gen(31, 9)), BIG_HW, BIG_HW))
    for label, img, Ho, Wo in cases:
        y = impl.img_to_act(img, Ho, Wo)
        T.add_ratio("exact", label, exact(y, ref_img_to_act(img, Ho, Wo, impl.H)))
        pad_ok = y.shape[-1] == 8 and bool((bits(y[..., 3:]) == 0).all())
        T.add_ratio("exact", label + ", pad channels +0", 0.0 if pad_ok else INF)


def sweep_resize_nearest(impl, T, big):
    cases = [(2 if a == 16 else 1, a, a, C, b, b) for a, b in NEAREST_PAIRS for C in (1, 3, 4)] + [(1, 37, 16, 3, 16, 37), (1, 5, 7, 3, 5, 7)]
    if big:
        cases.append((1, 240, 320, 3, BIG_HW, BIG_HW))
    for (N, sh, sw, C, dh, dw) in cases:
        img = torch.randint(0, 256, (N, sh, sw, C), dtype=U8, generator=_gen(32, N, sh, sw, C, dh))
        want = gather_hw(img, oracle_src(sh, dh), oracle_src(sw, dw)).contiguous()
        T.add_ratio("exact", "%dx%dx%dx%d -> %dx%d" % (N, sh, sw, C, dh, dw), exact(impl.resize_nearest(img, dh, dw), want))


# =====================================================================================================================================
# act_to_img
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def tie_inputs():
    """f32 inputs x whose f32 chain (x / 2 + 0.5) * 255 lands exactly on k + 0.5 -> (x, k), searched 64 f32 steps either side of
    2 ((k + 0.5) / 255 - 0.5) for every k in 0..254"""
    k = np.arange(255)
    x0 = (2.0 * ((k + 0.5) / 255.0 - 0.5)).astype(np.float32)
    cand = (x0.view(np.int32)[:, None] + np.arange(-64, 65, dtype=np.int32)[None, :]).view(np.float32).copy()
    cand[x0 == 0] = 0.0                                                         # k = 127: x = 0 itself (steps of its bit pattern are not neighbours)
    x = torch.from_numpy(cand)
    v = (x / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0
    hit = v == torch.from_numpy(k + 0.5).float()[:, None]
    return x[hit].clone(), torch.from_numpy(k)[:, None].expand_as(x)[hit].clone()


def pack3(vals):
    """values -> x (1,1,n,4): three per pixel in channels 0..2 (the tail repeats the first), channel 3 the sentinel"""
    n = (vals.numel() + 2) // 3
    flat = torch.cat([vals, vals[:1].expand(3 * n - vals.numel())])
    x = torch.full((1, 1, n, 4), SENTINEL, dtype=F32)
    x[..., :3] = flat.reshape(1, 1, n, 3)
    return x


def act_inputs(g, N, h, w):
    x = torch.full((N, h, w, 4), SENTINEL, dtype=F32)
    x[..., :3] = torch.rand(N, h, w, 3, generator=g) * 3.0 - 1.5
    return x


def edge_values():
    one = np.float32(1.0)
    vals = [-1.0, 1.0, 0.0, -0.0, -1.5, 1.5, -1e30, 1e30, 1.0 / 255, -1.0 / 255]
    for s in (-one, one):
        vals += [float(np.nextafter(s, np.float32(0))), float(np.nextafter(s, np.float32(2) * s))]
    return torch.tensor(vals, dtype=F32)


def judge_act_img(img, x, sy, sx):
    """-> (exact ratio against the f32 chain, ratio of the fp64 second opinion, share of elements inside the tie band)"""
    v32 = (x[..., :3] / 2 + 0.5).clamp(0, 1) * 255                             # decode_img_latents, f32
    want = gather_hw(torch.from_numpy(v32.numpy().round().astype("uint8")), sy, sx).contiguous()
    r_exact = exact(img, want)
    if img.shape != want.shape or img.dtype != U8:
        return r_exact, INF, 0.0
    v = gather_hw((x[..., :3].to(F64) / 2 + 0.5).clamp(0, 1) * 255, sy, sx)
    lo = torch.floor(v)
    band = ((v - lo) - 0.5).abs() <= 2 * 255 * E
    o = img.to(F64)
    ok = torch.where(band, (o == lo) | (o == lo + 1), o == torch.round(v))
    return r_exact, (0.0 if bool(ok.all()) else INF), float(band.double().mean())


def sweep_act_to_img(impl, T, big):
    ident = lambda n: torch.arange(n)
    sets = [("random %dx%dx%d" % s, act_inputs(_gen(33, *s), *s), True) for s in ((1, 1, 1), (3, 3, 5), (1, 16, 24), (1, 64, 64))]
    ties, ks = tie_inputs()
    assert bool((ks % 2 == 0).any()) and bool((ks % 2 == 1).any()), "the tie set needs even and odd k"
    sets += [("clamp edges", pack3(edge_values()), False), ("ties", pack3(ties), False)]
    if big:
        sets.append(("second trip", act_inputs(_gen(33, 9), 1, BIG_HW, BIG_HW), True))
    for label, x, is_random in sets:
        N, h, w, _ = x.shape
        modes = [(True, False)] if (big and h == BIG_HW) else [(True, False), (False, True), (True, True)]
        for want_img, want_float in modes:
            img, fo = impl.act_to_img(x, h, w, want_img, want_float)
            tag = "%s img %d float %d" % (label, want_img, want_float)
            if want_img:
                r_exact, r64, share = judge_act_img(img, x, ident(h), ident(w))
                T.add_ratio("exact", tag, r_exact)
                T.add_ratio("random", tag + ", fp64 second opinion", r64)
                if is_random and h * w >= 4096:
                    T.add_ratio("random", tag + ", share inside the tie band %.2e" % share, 0.0 if share <= BAND_SHARE_CAP else INF)
            else:
                T.add_ratio("exact", tag + ", no image asked", 0.0 if img is None else INF)
            if want_float:
                T.add_ratio("exact", tag + " float_out", exact(fo, x[..., :3].permute(0, 3, 1, 2).contiguous()))
    for (N, h, w, oh, ow) in [(3 if a == 16 else 1, a, a, b, b) for a, b in NEAREST_PAIRS] + [(1, 16, 37, 37, 16)]:
        x = act_inputs(_gen(34, N, h, w, oh), N, h, w)
        for want_img, want_float in ((True, True), (False, True)):
            img, fo = impl.act_to_img(x, oh, ow, want_img, want_float)
            tag = "%dx%dx%d -> %dx%d img %d" % (N, h, w, oh, ow, want_img)
            if want_img:
                r_exact, r64, _ = judge_act_img(img, x, oracle_src(h, oh), oracle_src(w, ow))
                T.add_ratio("exact", tag, r_exact)
                T.add_ratio("random", tag + ", fp64 second opinion", r64)
            T.add_ratio("exact", tag + " float_out at (h, w)", exact(fo, x[..., :3].permute(0, 3, 1, 2).contiguous()))


# =====================================================================================================================================
# the layout kernels: nchw_to_act, nchw_to_actf32, actf32_pad_h16, actf32_to_nchw, concat_channels
# =====================================================================================================================================
NHW = [(1, 1, 1), (3, 3, 5), (1, 16, 24), (3, 16, 24)]


def sweep_nchw_to_act(impl, T, big):
    H = impl.H
    cases = [(N, C, h, w) for (N, h, w) in NHW for C in (3, 4, 8)] + ([(1, 4, BIG_HW, BIG_HW)] if big else [])
    for (N, C, h, w) in cases:
        x = torch.randn(N, C, h, w, generator=_gen(35, N, C, h, w))
        nhwc = x.permute(0, 2, 3, 1)
        for scale in (1.0, INV_S32):
            if h == BIG_HW and scale != 1.0:
                continue
            y = impl.nchw_to_act(x, 8, scale)
            label = "(%d,%d,%d,%d) scale %.4g" % (N, C, h, w, scale)
            if y.shape != (N, h, w, 8):
                T.add_ratio("exact", label, INF)
                continue
            T.add_ratio("exact", label + ", pad channels +0", 0.0 if bool((bits(y[..., C:]) == 0).all()) else INF)
            if scale == 1.0:
                T.add_ratio("exact", label, exact(y[..., :C].contiguous(), nhwc.to(H.dtype).contiguous()))
            else:
                ref = nhwc.to(F64) * scale
                T.add_ratio("random", label, ratio(y[..., :C], ref, bound16(ref, SLACK * E * ref.abs(), H)))
                T.add_ratio("random", label + ", between the roundings of y -+ d", inside16(y[..., :C], ref, SLACK * E * ref.abs(), H))


def sweep_nchw_to_actf32(impl, T, big):
    cases = [(N, C, h, w) for (N, h, w) in NHW for C in (3, 4)] + ([(1, 4, BIG_HW, BIG_HW)] if big else [])
    for (N, C, h, w) in cases:
        x = torch.randn(N, C, h, w, generator=_gen(36, N, C, h, w))
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        T.add_ratio("exact", "(%d,%d,%d,%d) scale 1" % (N, C, h, w), exact(impl.nchw_to_actf32(x, 1.0), nhwc))
        if h != BIG_HW:
            ref = nhwc.to(F64) * INV_S32
            T.add_ratio("random", "(%d,%d,%d,%d) scale 1 / 0.18215f" % (N, C, h, w), ratio(impl.nchw_to_actf32(x, INV_S32), ref, SLACK * E * ref.abs()))


def sweep_actf32_pad_h16(impl, T, big):
    for (Pn, C, Cpad) in [(1, 4, 8), (15, 3, 8), (384, 4, 8), (384, 8, 8)] + ([(GRID_CAP + 777, 4, 8)] if big else []):
        x = torch.randn(Pn, C, generator=_gen(37, Pn, C))
        want = torch.zeros(Pn, Cpad, dtype=impl.H.dtype)
        want[:, :C] = x.to(impl.H.dtype)
        T.add_ratio("exact", "P %d C %d -> %d" % (Pn, C, Cpad), exact(impl.actf32_pad_h16(x, Cpad), want))


def sweep_actf32_to_nchw(impl, T, big):
    C = 4
    for (N, h, w, ld) in [(N, h, w, ld) for (N, h, w) in NHW for ld in (4, 8, 16)] + ([(1, BIG_HW, BIG_HW, 8)] if big else []):
        x = torch.full((N, h, w, ld), SENTINEL, dtype=F32)
        x[..., :C] = torch.randn(N, h, w, C, generator=_gen(38, N, h, w, ld))
        T.add_ratio("exact", "(%d,%d,%d) ld %d" % (N, h, w, ld), exact(impl.actf32_to_nchw(x, C), x[..., :C].permute(0, 3, 1, 2).contiguous()))


def sweep_concat(impl, T, big):
    cases = [(Pn, Ca, Cb) for (Ca, Cb) in ((8, 8), (8, 312), (320, 8), (640, 320)) for Pn in (1, 15, 384)] + ([(65537, 8, 312)] if big else [])
    for (Pn, Ca, Cb) in cases:
        g = _gen(39, Pn, Ca, Cb)
        a, b = torch.randn(Pn, Ca, generator=g).to(impl.H.dtype), torch.randn(Pn, Cb, generator=g).to(impl.H.dtype)
        T.add_ratio("exact", "P %d (%d, %d)" % (Pn, Ca, Cb), exact(impl.concat(a, b), torch.cat([a, b], 1)))


# =====================================================================================================================================
# f32_to_h16, f32_to_h16_x8, h16_to_f32
# =====================================================================================================================================
def step32(x, k):
    """x moved by k f32 steps away from zero (k < 0: towards it); x finite and non-zero"""
    return (bits(x) + k).view(F32)


def conversion_inputs(H):
    """an f32 vector, its length a multiple of 8, that holds what a conversion to H gets wrong"""
    g = _gen(40, len(H.name))
    draws = torch.randn(2048, generator=g) * torch.exp2(torch.randint(-12, 12, (2048,), generator=g).float())
    lo16 = draws[:512].to(H.dtype)
    up16 = (bits(lo16) + 1).view(H.dtype)                                        # the neighbour away from zero
    mid = (lo16.float() + up16.float()) / 2                                      # one more bit than the type holds: exact in f32
    assert bool(torch.isfinite(mid).all()) and bool((mid.to(F64) * 2 == lo16.to(F64) + up16.to(F64)).all())
    top16 = torch.tensor([H.top], dtype=F64)                                     # 2^(emax + 1)
    largest = top16 * (1 - 2 * H.u16)                                            # the largest finite value: 2^(emax + 1) (1 - 2^-p)
    thresh = ((largest + top16) / 2).float()                                     # a tie whose even side is infinity
    assert float(largest.float().to(H.dtype)) == float(largest) and math.isinf(float(thresh.to(H.dtype))) and math.isfinite(float(step32(thresh, -1).to(H.dtype)))
    special = torch.cat([largest.float(), thresh, step32(thresh, -1), step32(thresh, 1), torch.tensor([3.4028234663852886e38])])
    if H.name == "fp16":
        sub = torch.tensor([2.0 ** -25, 3 * 2.0 ** -25])                         # ties of the subnormal grid: to 0 and to 2^-23
        special = torch.cat([special, sub, step32(sub, 1), step32(sub, -1), torch.tensor([2.0 ** -24, 2.0 ** -14, 2.0 ** -26, 70000.0]),
                             torch.rand(256, generator=g) * 2.0 ** -14, torch.exp2(-14 - 13 * torch.rand(256, generator=g))])
    x = torch.cat([draws, mid, step32(mid, 1), step32(mid, -1), special, -special, torch.zeros(2), -torch.zeros(2)])
    assert bool(torch.isfinite(x).all())
    return torch.cat([x, x[:(-x.numel()) % 8]])


def sweep_f32_to_h16(impl, T, big):
    H = impl.H
    x = conversion_inputs(H)
    sets = [("ties, overflow, subnormals (n %d)" % x.numel(), x, True), ("n 1003", x[:1003].clone(), False), ("n 8", x[:8].clone(), True)]
    if big:
        g = _gen(41)
        n = 8 * (GRID_CAP + 8)
        sets.append(("second trip (n %d)" % n, torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 12, (n,), generator=g).float()), True))
    for label, v, both in sets:
        want = v.to(H.dtype)
        y1 = impl.f32_to_h16(v, False)
        T.add_ratio("exact", label + " f32_to_h16", exact(y1, want))
        if both:
            y8 = impl.f32_to_h16(v, True)
            T.add_ratio("exact", label + " f32_to_h16_x8", exact(y8, want))
            T.add_ratio("exact", label + " the two forms agree", exact(y8, y1))


def sweep_h16_to_f32(impl, T, big):
    H = impl.H
    allp = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(H.dtype)
    sets = [("every non-NaN pattern", allp[~torch.isnan(allp)].contiguous())]
    if big:
        r = torch.randint(0, 65536, (GRID_CAP + 777,), generator=_gen(42), dtype=torch.int32).to(torch.int16).view(H.dtype)
        sets.append(("second trip", torch.where(torch.isnan(r), torch.ones_like(r), r)))
    for label, v in sets:
        T.add_ratio("exact", label, exact(impl.h16_to_f32(v), v.float()))


# =====================================================================================================================================
# pixel_linear_f32, vae_sample, timestep_embed, add_noise
# =====================================================================================================================================
def sweep_pixel_linear(impl, T, big):
    cases = [(Pn, cfg, hb) for cfg in ((8, 8, 8, 8), (4, 4, 4, 4), (4, 4, 8, 16)) for Pn in (1, 15, 384) for hb in (True, False)]
    if big:
        cases.append((GRID_CAP + 777, (4, 4, 4, 4), True))
    for (Pn, (Cin, Cout, ldx, ldy), has_bias) in cases:
        for cls in ("exact", "random"):
            if cls == "exact" and Pn > 384:
                continue
            g = _gen(43, Pn, Cin, ldx, ldy, has_bias, cls == "exact")
            if cls == "exact":
                xs, w, b = [torch.randint(-8, 9, s, generator=g).float() for s in ((Pn, Cin), (Cout, Cin), (Cout,))]
            else:
                xs, w, b = torch.randn(Pn, Cin, generator=g), torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin), 0.3 * torch.randn(Cout, generator=g)
            b = b if has_bias else None
            x = torch.full((Pn, ldx), SENTINEL, dtype=F32)
            x[:, :Cin] = xs
            y = impl.pixel_linear(x, w, b, ldy)
            label = "P %d Cin %d Cout %d ldx %d ldy %d bias %d" % (Pn, Cin, Cout, ldx, ldy, has_bias)
            if y.shape != (Pn, ldy) or not bool(torch.isnan(y[:, Cout:]).all()):
                T.add_ratio(cls, label + ": columns beyond Cout were written", INF)
                continue
            ref = xs.to(F64) @ w.to(F64).t() + (0 if b is None else b.to(F64))
            A = xs.to(F64).abs() @ w.to(F64).abs().t() + (0 if b is None else b.to(F64).abs())
            T.add_ratio(cls, label, ratio(y[:, :Cout], ref, 0.0 if cls == "exact" else SLACK * ((Cin + 2) * E * A + E * ref.abs())))


def vae_inputs(g, N, h, w, ldm):
    mom = torch.full((N, h, w, ldm), SENTINEL, dtype=F32)
    mom[..., :4] = torch.randn(N, h, w, 4, generator=g)
    mom[..., 4:8] = 3.0 * torch.randn(N, h, w, 4, generator=g)
    k = min(len(SPECIAL_LOGVARS), N * h * w)                                      # pixel p gets SPECIAL_LOGVARS[p] in all four channels
    flat = mom.view(-1, ldm)
    flat[:k, 4:8] = torch.tensor(SPECIAL_LOGVARS[:k])[:, None]
    flat[:k:2, :4] = 0.0                                                         # mean 0: the bound is relative to |std eps| alone
    if N * h * w < len(SPECIAL_LOGVARS):
        flat[0, 4:8] = torch.tensor([-40.0, 19.999, 20.0, 25.0])
    return mom, torch.randn(N, 4, h, w, generator=g)


def sweep_vae_sample(impl, T, big):
    cases = [(N, h, w, ldm) for (N, h, w) in NHW for ldm in (8, 16)] + ([(1, BIG_HW, BIG_HW, 8)] if big else [])
    for (N, h, w, ldm) in cases:
        mom, eps = vae_inputs(_gen(44, N, h, w, ldm), N, h, w, ldm)
        mean64, raw64 = mom[..., :4].permute(0, 3, 1, 2).to(F64), mom[..., 4:8].permute(0, 3, 1, 2).to(F64)
        raw_nchw = mom[..., :8].permute(0, 3, 1, 2).contiguous()
        for use_eps, want_mom in ((True, True), (True, False), (False, True)) if h != BIG_HW else ((True, True),):
            z, mo = impl.vae_sample(mom, eps if use_eps else None, want_mom)
            label = "(%d,%d,%d) ldm %d eps %d mom %d" % (N, h, w, ldm, use_eps, want_mom)
            if use_eps:
                s = torch.exp(0.5 * raw64.clamp(-30.0, 20.0)) * eps.to(F64)
                ref = 0.18215 * (mean64 + s)
                T.add_ratio("random", label, ratio(z, ref, SLACK * 8 * E * 0.18215 * (mean64.abs() + s.abs())))
            else:
                T.add_ratio("exact", label + ": the mode", exact(z, (mom[..., :4] * f32c(S32)).permute(0, 3, 1, 2).contiguous()))
            if want_mom:
                T.add_ratio("exact", label + " mom_nchw (raw)", exact(mo, raw_nchw))
            else:
                T.add_ratio("exact", label + ", no moments asked", 0.0 if mo is None else INF)


def sweep_timestep_embed(impl, T, big):
    H = impl.H
    cases = [(torch.tensor(TIMESTEPS, dtype=F32), dim) for dim in (8, 320)]
    if big:
        cases.append((torch.rand(13108, generator=_gen(45)) * 999.0, 320))          # 13108 x 160 = 2 097 280 items
    for t, dim in cases:
        half = dim // 2
        y = impl.timestep_embed(t, dim)
        a = t.to(F64)[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)[None, :]
        ref = torch.cat([torch.cos(a), torch.sin(a)], 1)
        d = SLACK * (33 * E * torch.cat([a, a], 1).abs() + FN * ref.abs())
        label = "N %d dim %d" % (t.numel(), dim)
        T.add_ratio("random", label, ratio(y, ref, bound16(ref, d, H)))
        T.add_ratio("random", label + ", between the roundings of y -+ d", inside16(y, ref, d, H))
        zero = torch.nonzero(t == 0).flatten()
        if zero.numel() and y.shape == ref.shape:
            want = torch.cat([torch.ones(half), torch.zeros(half)]).to(H.dtype)
            T.add_ratio("exact", label + " t = 0", max(exact(y[int(i)].contiguous(), want) for i in zero))


def sweep_add_noise(impl, T, big):
    sa, s1a = float(np.sqrt(np.float32(0.7))), float(np.sqrt(np.float32(0.3)))
    for n in [1, 1003, 4 * 4 * 8 * 8] + ([GRID_CAP + 777] if big else []):
        g = _gen(46, n)
        x0, nz = torch.randn(n, generator=g), torch.randn(n, generator=g)
        ref = sa * x0.to(F64) + s1a * nz.to(F64)
        b = SLACK * 3 * E * ((sa * x0.to(F64)).abs() + (s1a * nz.to(F64)).abs())
        for inplace in (False, True):
            T.add_ratio("random", "n %d %s" % (n, "in place" if inplace else "out of place"), ratio(impl.add_noise(x0, nz, sa, s1a, inplace), ref, b))


# =====================================================================================================================================
# svg_resize_bilinear_f32
# =====================================================================================================================================
BILINEAR_PAIRS = [((1, 1), (4, 4)), ((4, 4), (1, 1)), ((5, 7), (8, 8)), ((8, 8), (5, 7)), ((32, 32), (12, 20)), ((9, 20), (24, 11))]


def sweep_resize_bilinear(impl, T, big):
    cases = [(3, hw, ohw) for hw, ohw in BILINEAR_PAIRS] + ([(1, (64, 64), (1025, 1025))] if big else [])          # 1 050 625 > BILINEAR_CAP
    for (Pn, (h, w), (oh, ow)) in cases:
        x = torch.randn(Pn, h, w, generator=_gen(47, h, w, oh, ow))
        y = impl.resize_bilinear(x, oh, ow)
        x64 = x.to(F64)
        ref = F.interpolate(x64[None], (oh, ow), mode="bilinear", align_corners=False)[0]
        Lx = (x64[:, :, 1:] - x64[:, :, :-1]).abs().amax((1, 2)) if w > 1 else torch.zeros(Pn, dtype=F64)
        Ly = (x64[:, 1:] - x64[:, :-1]).abs().amax((1, 2)) if h > 1 else torch.zeros(Pn, dtype=F64)
        b = SLACK * (4 * E * max(h, w) * (Lx + Ly) + 4 * E * x64.abs().amax((1, 2)))
        T.add_ratio("random", "%dx%d -> %dx%d" % (h, w, oh, ow), ratio(y, ref, b[:, None, None].expand_as(ref)))
        if Pn > 1:
            c = torch.tensor([0.7311, -123.456, 3.0e-5])[:, None, None].expand(3, h, w).contiguous()
            T.add_ratio("random", "%dx%d -> %dx%d constant planes" % (h, w, oh, ow),
                        ratio(impl.resize_bilinear(c, oh, ow), c[:, :1, :1].to(F64).expand(3, oh, ow), SLACK * 2 * E * c[:, :1, :1].to(F64).abs().expand(3, oh, ow)))
    for (h, w) in ((1, 1), (5, 7), (16, 24)):
        x = torch.randn(3, h, w, generator=_gen(48, h, w))
        T.add_ratio("exact", "%dx%d -> the same size" % (h, w), exact(impl.resize_bilinear(x, h, w), x))


# =====================================================================================================================================
# the sweeps, by kernel
# =====================================================================================================================================
SWEEPS = {"img_to_act": sweep_img_to_act, "nchw_to_act": sweep_nchw_to_act, "actf32_pad_h16": sweep_actf32_pad_h16, "concat_channels": sweep_concat,
          "f32_to_h16": sweep_f32_to_h16, "h16_to_f32": sweep_h16_to_f32, "timestep_embed": sweep_timestep_embed,
          "act_to_img": sweep_act_to_img, "nchw_to_actf32": sweep_nchw_to_actf32, "actf32_to_nchw": sweep_actf32_to_nchw,
          "pixel_linear_f32": sweep_pixel_linear, "vae_sample": sweep_vae_sample, "add_noise": sweep_add_noise,
          "resize_nearest_u8": sweep_resize_nearest, "resize_bilinear_f32": sweep_resize_bilinear}
KERNELS16 = ["img_to_act", "nchw_to_act", "actf32_pad_h16", "concat_channels", "f32_to_h16", "h16_to_f32", "timestep_embed"]
KERNELS32 = [k for k in SWEEPS if k not in KERNELS16]
CASES = [(k, h) for k in KERNELS16 for h in HALVES] + [(k, "bf16") for k in KERNELS32]           # (the f32 / u8 kernels exist once)
CASE_IDS = ["%s-%s" % c if c[0] in KERNELS16 else c[0] for c in CASES]


def run(impl, kernel, big=True):
    T = Tally(kernel)
    SWEEPS[kernel](impl, T, big)
    return T


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------
def test_half_ulp_rule_cpu():
    """round-to-nearest-even itself exceeds u16 |y| in the lower half of a binade and attains h(|y|); h never exceeds 2 u16 |y|"""
    for H in HALVES.values():
        x = torch.cat([torch.randn(200000, generator=_gen(50)), torch.tensor([1.0 + 2 * H.u16, 1.0 + 6 * H.u16])]).to(F64)
        err = (x.float().to(H.dtype).to(F64) - x).abs()
        h = half_ulp16(x.abs(), H)
        assert bool((err <= h).all()) and float((err / h).max()) == 1.0
        assert float((err / (H.u16 * x.abs())).max()) > 1.9
        big = x.abs() > 1e-3
        assert bool((h[big] <= 2 * H.u16 * x.abs()[big]).all()) and bool((h[big] >= H.u16 * x.abs()[big]).all())


def test_nearest_rule_cpu():
    """oracle_src is the rule of oracle.sd_oracle.resize_nearest_u8 at the tested size pairs, and 26 -> 22 is a pair where the float rule
    and the integer rule d * in // out differ"""
    for (a, b) in NEAREST_PAIRS:
        img = torch.randint(0, 256, (2, a, a, 3), dtype=U8, generator=_gen(51, a, b))
        assert torch.equal(SO.resize_nearest_u8(img, b, b), gather_hw(img, oracle_src(a, b), oracle_src(a, b)))
        assert torch.equal(Emu(HALVES["bf16"]).src(a, b, False), oracle_src(a, b))
    assert not torch.equal(oracle_src(26, 22), (torch.arange(22) * 26) // 22)


def test_tie_set_cpu():
    """the tie set has even and odd k, every member is a tie of the f32 chain, and half-up differs from half-to-even on it"""
    x, k = tie_inputs()
    assert x.numel() >= 255 and bool((k % 2 == 0).any()) and bool((k % 2 == 1).any())
    v = (x / 2 + 0.5).clamp(0, 1) * 255
    assert torch.equal(v, k.float() + 0.5)
    assert bool((torch.round(v) != torch.floor(v + 0.5)).any())


@pytest.mark.parametrize("kernel,half", CASES, ids=CASE_IDS)
def test_emulation_cpu(kernel, half):
    """the emulation of each kernel passes its judge on every case and data class: the bounds are attainable and the band cap holds"""
    run(Emu(HALVES[half]), kernel).check(report=False, tag=half if kernel in KERNELS16 else "")


# defect -> [(sweep, the data classes whose judge must reject it)]
MUTATIONS = {"act_half_up": [("act_to_img", ["exact"])],                                     # round half up
             "h16_truncate": [("f32_to_h16", ["exact"])],                                    # truncation instead of nearest-even
             "img_div_256": [("img_to_act", ["exact"])],
             "img_pad_nonzero": [("img_to_act", ["exact"])],
             "nearest_int_rule": [("resize_nearest_u8", ["exact"]), ("img_to_act", ["exact"]), ("act_to_img", ["exact"])],      # d * in // out
             "vae_no_clamp": [("vae_sample", ["random"])],
             "vae_clamp_30": [("vae_sample", ["random"])],                                   # the upper edge at 30
             "vae_clamp_low_40": [("vae_sample", ["random"])],                               # the lower edge at -40
             "vae_scale_mean_only":[("vae_sample", ["random"])],                            # 0.18215 before the noise is added
             "vae_mom_clamped": [("vae_sample", ["exact"])],                                 # the clamped logvar written to mom_nchw
             "ts_swap": [("timestep_embed", ["random", "exact"])],                           # [sin | cos]
             "ts_half_minus_1": [("timestep_embed", ["random"])],                            # half - 1 in the frequency's denominator
             "nchw_ld_ignored": [("actf32_to_nchw", ["exact"])],
             "concat_off_by_8": [("concat_channels", ["exact"])],
             "bilinear_align_corners": [("resize_bilinear_f32", ["random"])],
             "bilinear_no_max": [("resize_bilinear_f32", ["random"])],                       # the max(., 0) on the source coordinate dropped
             "noise_swapped": [("add_noise", ["random"])],                                   # sa and s1a exchanged
             "linear_no_bias": [("pixel_linear_f32", ["random", "exact"])]}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judges_reject_cpu(mut):
    """each defect of the emulation is outside the judges that see it (the sound emulation is inside: test_emulation_cpu), in both storage
    types where the kernel has a 16-bit side"""
    for kernel, classes in MUTATIONS[mut]:
        for half in (HALVES if kernel in KERNELS16 else ["bf16"]):
            T = run(Emu(HALVES[half], mut), kernel, big=False)
            rej = T.rejected()
            print("[eltwise_kernels] mutation %-24s %-20s %-5s %s" % (mut, kernel, half, {c: "%.3g" % T.worst[c][0] for c in classes}))
            assert all(rej.get(c, False) for c in classes), "the judge of %s (%s) accepts the defect %s in %s" % (kernel, half, mut, [c for c in classes if not rej.get(c)])


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel,half", CASES, ids=CASE_IDS)
def test_kernel_against_fp64(ctx, kernel, half):
    run(Gpu(ctx, HALVES[half]), kernel).check(report=True, tag=half if kernel in KERNELS16 else "")


@gpu
@pytest.mark.parametrize("half", list(HALVES))
def test_refusals(ctx, half):
    """f32_to_h16_x8 refuses n % 8 != 0 and misaligned pointers, pixel_linear_f32 refuses Cin = 9: a non-zero return, a message in
    svg_last_error, nothing written, and the context computes the next valid call.  Every buffer is sized for the call as made."""
    impl = Gpu(ctx, HALVES[half])
    x = torch.randn(64, device="cuda")
    y = torch.full((64,), NAN, device="cuda", dtype=impl.H.dtype)
    assert impl.refused("svg_op_f32_to_h16_x8", True, P(x), P(y), 12) and bool(torch.isnan(y).all())
    assert impl.refused("svg_op_f32_to_h16_x8", True, P(x) + 4, P(y), 16) and bool(torch.isnan(y).all())
    assert impl.refused("svg_op_f32_to_h16_x8", True, P(x), P(y) + 2, 16) and bool(torch.isnan(y).all())
    xs, w, o = torch.randn(4, 9, device="cuda"), torch.randn(9, 9, device="cuda"), torch.full((4 * 9,), NAN, device="cuda")
    assert impl.refused("svg_op_pixel_linear_f32", False, P(xs), 9, P(w), None, P(o), 9, 4, 9, 9) and bool(torch.isnan(o).all())
    for kernel in ("f32_to_h16", "pixel_linear_f32"):
        run(impl, kernel, big=False).check(report=False)
