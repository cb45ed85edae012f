"""The update kernels of the sampling loop (csrc/sampler.hip) one by one against fp64, element by element.

Each kernel is driven alone through its operator-level hook (svg_op_ddim_step, svg_op_dpmpp_step, svg_op_lms_step, svg_op_lms_input,
svg_op_sampler_tvec, svg_op_sampler_bump; add_noise is judged in tests/test_eltwise_kernels_gpu.py).  The hooks check their arguments on
the host and call the launcher the loop calls.  Conventions as in tests/test_eltwise_kernels_gpu.py: every output buffer is filled with NaN
and carries a NaN guard behind it (and, where a buffer starts 4 bytes past a 16-byte boundary, a NaN gap in front) that must be untouched
afterwards; every element is judged, none left out (a non-finite or missing element counts as inf); the worst err / bound per kernel and
data class goes through conftest.margin(..., tol=1.0, unit="err/bound").  The reference is fp64 on the same f32 inputs AND the same f32
row: the test builds its own rows and does not test the plan (tests/test_sampler_plan_cpu.py pins that).  No launched case hands a kernel a
null or unallocated buffer that it would read; what the hooks refuse is tested as a host error, and nothing is launched.

CONSTANTS   E = 2^-24 (f32 unit roundoff), SLACK = 1.01 on every derived bound, for the products of two of its terms.  No constant here
was fitted to what the GPU returns.

ROWS   the DDIM / DPM++ rows of a 50-step schedule at t = 980, 500, 20 and 0 (t_next = t - 20; at t = 0 it is < 0: alpha_bar = 1), from the
scaled-linear alphas in fp64, rounded to f32.  DPM++: t = 980 first order, 500 first and second order, 20 second order, 0 the `last`
row.  LMS: steps 0 .. 8 of a 9-step schedule from _lib.lms_coefs (orders 1, 2, 3, 4, 4 ...; the ring slot i & 3 wraps twice).  Plus a few
synthetic rows with coefficients of mixed sign and size (a `last` row with k != 0 among them).  Guidance: eps_c null, 7.5, 1.0, -2.0.

SIZES   n in {1, 3, 4, 5, 255, 256, 257, 1001, 2048}, and per kernel one n that exceeds one trip of the grid-stride loop (8192 x 256 items):
8192 x 256 + 1001 elements for the scalar kernels and for the scalar LMS forms (a buffer 4 bytes past a 16-byte boundary), 4 (8192 x 256 + 37)
for the 16-byte LMS form (+ 3 for lms_input, whose tail then has three elements).

DATA CLASSES   random: x_out on unit-scale normal data (LMS latents at sigma_0 = 14.6).  edge: DDIM's x_out on the clamp-edge data.
m_out: DPM++'s x0 prediction.  ring: the LMS ring slot of this step.  exact: bound 0, bit equality (every structure check below, the
clipped DDIM elements, lms_input, sampler_tvec, sampler_bump, guards, gaps and untouched inputs).

BOUNDS (a term is taken as 0 where FMA contraction may remove that rounding: every bound covers the fused and the unfused form)
  combine   e = eu + g (ec - eu):  de = 2 E |g| |ec - eu| + E |e|;  0 when ec is null.
  DDIM      num = z - s1a e, x0 = num / sa:  dx0 = (E (|s1a e| + |num|) + |s1a| de) / |sa| + E |x0|;  the clamp is 1-Lipschitz;
            out = sap x0c + s1ap e:  dout = |sap| dx0 + E |sap x0c| + |s1ap| de + E |s1ap e| + E |out|.
            exact class: where |x0| > 1 + 2 dx0 and ec is null the output is one of the two f32 results of sap (+-1) + s1ap e, the product
            rounded before the sum or not (fma32 below is the correctly rounded fused form), bit for bit.
            edge class: z built so that x0 is +-1 exactly (eps 0, z = +-sa), +-1 and +-(1 +- 2^-20) to the rounding of z, and far outside.
            These elements are judged like all others, no band is left out.
  DPM++     m = inv_a (x - sig e):  dm = |inv_a| (E |sig e| + |sig| de + E |x - sig e|) + E |m|  (judges m_out);
            d = m + k (m - mp):  dd = dm + |k| (dm + E |m - mp|) + E |k (m - mp)| + E |d|;
            out = cx x + cd d:  dout = E |cx x| + |cd| dd + E |cd d| + E |out|.  A `last` row: x_out equals m_out bit for bit (and is
            judged by dm where m_out is null).  First order (k = 0): m_prev is a NaN-filled buffer, so a finite output shows it was not read.
  LMS       16 E (|x| + sum |c_k d_{i-k}|) + |c0| de, the per-element bound of tests/test_lms_gpu.py plus the combine.  The ring slot
            i & 3 holds the combined eps within de (eps_u bit for bit when ec is null); the other three slots are unchanged, NaN where
            never written.
  lms_input one IEEE product: bit equal to torch's f32 x * c.    sampler_tvec: every output bit equal to tab[8 idx].
  sampler_bump: the counter goes up by exactly 1 and the ints around it are untouched.

STRUCTURE (exact class, bit for bit)   a table row (row r of a device table whose other rows hold 1e30, r first, middle and last) equals
the argument row; in place equals out of place (x / x_out everywhere, m_prev / m_out for DPM++, and the loop's form with both), and out of
place the inputs are left unchanged; the 16-byte and the scalar LMS forms round alike: each pointer in turn 4 bytes off, and for
n % 4 != 0 against the first n elements of the run on the next multiple of 4 (lms_step is scalar throughout then, because of the ring
stride; lms_input takes 16-byte groups plus a tail of n mod 4).

The CPU half (not marked gpu) pushes a torch-f32 emulation of each kernel, in the kernel's order and in both the fused and the unfused form,
through the same data and the same judges; test_judges_reject_cpu requires the judges to reject the defects listed in MUTATIONS, and
test_coverage_cpu pins what the case list reaches.  One defect, the scalar tail reading eps_c at i - 4 nv, cannot show through today's
launcher: lms_step never mixes 16-byte groups with a tail (n % 4 != 0 makes every ring row misaligned, so nv is 0 or the tail is empty).
Its judge is therefore exercised on the emulation of the mixed form the kernel itself supports (Emu(mixed=True): sound it passes, with the
defect it is rejected)."""
import collections
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

from conftest import margin
from test_eltwise_kernels_gpu import E, F32, F64, GRID_CAP, INF, NAN, PAD, SENTINEL, SLACK, P, Tally, _gen, bits, exact, f32c, ratio, stream

gpu = pytest.mark.gpu
I32 = torch.int32
SIZES = [1, 3, 4, 5, 255, 256, 257, 1001, 2048]
BIG_SCALAR = GRID_CAP + 1001                                  # > one trip of a scalar loop
BIG_VEC = 4 * (GRID_CAP + 37)                                 # > one trip of a 16-byte loop
GUIDANCE = [None, 7.5, 1.0, -2.0]                             # None: eps_c null
X_SCALE = 14.6                                                # sigma_0 of the LMS schedule: the scale of its latents
LMS_STEPS = 9
NROWS = 5                                                     # rows of a device table
TABS = [(0, NROWS), (2, NROWS), (4, NROWS)]                   # (row index r, rows): first, middle, last


# =====================================================================================================================================
# rows
# =====================================================================================================================================
ABAR = np.cumprod(1.0 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2)


def abar(t):
    return 1.0 if t < 0 else float(ABAR[t])


def lam(ab):
    return 0.5 * math.log(ab) - 0.5 * math.log1p(-ab)


def ddim_row(t, t_prev):
    a, ap = abar(t), abar(t_prev)
    return [t, math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(1 - ap), 0, 0, 0]


def dpmpp_row(t, t_next, t_last):
    ab = abar(t)
    sig = math.sqrt(1 - ab)
    if t_next < 0:
        return [t, 1 / math.sqrt(ab), sig, 0, 0, 0, 1, 0]
    abn = abar(t_next)
    h = lam(abn) - lam(ab)
    k = 0.5 / ((lam(ab) - lam(abar(t_last))) / h) if t_last >= 0 else 0
    return [t, 1 / math.sqrt(ab), sig, math.sqrt(1 - abn) / sig, -math.sqrt(abn) * math.expm1(-h), k, 0, 0]


@functools.lru_cache(maxsize=None)
def rows(rule):
    """name -> f32 row (8,) of one rule"""
    if rule == "ddim":
        r = {"t%d" % t: ddim_row(t, t - 20) for t in (980, 500, 20, 0)}
        r["syn_a"] = [0, 0.5, -0.75, -1.25, 3.0, 0, 0, 0]
        r["syn_b"] = [0, -2.0, 1e-3, 0.03, -1.0, 0, 0, 0]
    elif rule == "dpmpp":
        r = {"t980_o1": dpmpp_row(980, 960, -1), "t500_o1": dpmpp_row(500, 480, -1), "t500_o2": dpmpp_row(500, 480, 520),
             "t20_o2": dpmpp_row(20, 0, 40), "t0_last": dpmpp_row(0, -20, 20),
             "syn_o2_a": [0, -1.7, 0.3, -0.6, 2.5, -0.8, 0, 0], "syn_o2_b": [0, 0.9, -1.2, 1.4, -0.05, 3.0, 0, 0],
             "syn_last_k": [0, 1.1, 0.4, 0.7, 0.3, 0.5, 1, 0]}
    else:
        from sd_video_gen_amd import _lib
        r = {}
        for i in range(LMS_STEPS):
            t, sigma, _, order, c = _lib.lms_coefs(LMS_STEPS, i)
            r["s%d" % i] = [t, 1 / math.sqrt(sigma * sigma + 1), order, i] + list(c)
        r["syn_o4"] = [0, -0.37, 4, 5, -2.3, 0.004, 17.0, -0.6]
        r["syn_o3"] = [0, 3e-5, 3, 2, 0.5, -0.5, 1e-3, 0]
        r["syn_o1"] = [0, 1.0, 1, 7, -1.0, 0, 0, 0]
    return {k: torch.tensor(v, dtype=F64).to(F32) for k, v in r.items()}


def dpmpp_kind(row):
    return "last" if float(row[6]) != 0 else ("second" if float(row[5]) != 0 else "first")


def table_of(row, tab):
    r, nrows = tab
    t = torch.full((nrows, 8), SENTINEL, dtype=F32)
    t[r] = row
    return t


def lms_groups(n, stride4, offs):
    """lms_groups of sampler.hip: the 4-float groups taken with 16-byte accesses; offs: the offset of each pointer in floats"""
    if (stride4 and n % 4) or any(o % 4 for o in offs):
        return 0
    return n // 4


def fma32(a, b, c):
    """the correctly rounded f32 a b + c: the product of two f32 is exact in fp64; the fp64 sum is made odd when it is inexact (TwoSum
    gives its error exactly), after which the rounding to f32 cannot be a double rounding"""
    p, c64 = a.to(F64) * b.to(F64), c.to(F64)
    p, c64 = torch.broadcast_tensors(p, c64)
    s = p + c64
    bb = s - p
    t = (p - (s - bb)) + (c64 - bb)
    sb = s.contiguous().view(torch.int64)
    grow = (t > 0) == (s > 0)                                                  # the exact sum is further from zero than s
    odd = torch.where((t != 0) & (sb & 1 == 0), sb + torch.where(grow, 1, -1), sb)
    return odd.view(F64).to(F32)


# =====================================================================================================================================
# The two implementations behind one interface: the HIP kernels through their hooks, and the torch emulation (with its defects).
# Every method returns a namespace: out / m / ring / o0 / o1 (CPU f32, or None) and ok (guards and gaps intact, inputs unchanged).
# =====================================================================================================================================
def R(**kw):
    kw.setdefault("ok", True)
    return types.SimpleNamespace(**kw)


class Gpu:
    mut = None

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib

    def buf(self, data, n, off=0):
        """-> (base, view): a gap of `off` NaN floats, n floats (data, or NaN), a guard of PAD NaN floats"""
        base = torch.full((off + n + PAD,), NAN, device="cuda", dtype=F32)
        assert base.data_ptr() % 16 == 0
        view = base[off:off + n]
        if data is not None:
            view.copy_(data.reshape(-1))
        return base, view

    def rowargs(self, row, tab):
        """-> (row, tab, idx) of a hook and what must stay alive until the launch has run"""
        if tab is None:
            host = (ctypes.c_float * 8)(*[float(v) for v in row])
            return (host, None, None), host
        t, idx = table_of(row, tab).cuda(), torch.tensor([tab[0]], dtype=I32).cuda()
        return (None, P(t), P(idx)), (t, idx)

    def call(self, name, *args):
        self.ctx.check(getattr(self.lib, name)(self.ctx.h, *args, stream()), name)

    def finish(self, outs, inputs):
        """outs: name -> (base, view, n, off) or None; inputs: [(device view, host tensor)] that the launch must leave unchanged"""
        torch.cuda.synchronize()
        ok, res = True, {}
        for name, o in outs.items():
            if o is None:
                res[name] = None
                continue
            base, view, n, off = o
            ok = ok and bool(torch.isnan(base[:off]).all()) and bool(torch.isnan(base[off + n:]).all())
            res[name] = view.cpu()
        for dev, host in inputs:
            if dev is not None:
                ok = ok and torch.equal(bits(dev.cpu().reshape(-1)), bits(host.reshape(-1)))
        return R(ok=ok, **res)

    def ddim(self, x, eu, ec, g, row, tab=None, inplace=False):
        n = x.numel()
        xb, xv = self.buf(x, n)
        eud, ecd = eu.cuda(), None if ec is None else ec.cuda()
        ob, ov = (xb, xv) if inplace else self.buf(None, n)
        ra, keep = self.rowargs(row, tab)
        self.call("svg_op_ddim_step", P(xv), P(eud), P(ecd), float(g or 0.0), P(ov), n, *ra)
        return self.finish({"out": (ob, ov, n, 0)}, [(None if inplace else xv, x), (eud, eu), (ecd, ec)])

    def dpmpp(self, x, eu, ec, g, mp, row, tab=None, inplace=False, m="out"):
        n = x.numel()
        xb, xv = self.buf(x, n)
        mpb, mpv = self.buf(mp, n)
        eud, ecd = eu.cuda(), None if ec is None else ec.cuda()
        ob, ov = (xb, xv) if inplace else self.buf(None, n)
        mb, mv = {"null": (None, None), "alias": (mpb, mpv)}.get(m) or self.buf(None, n)
        ra, keep = self.rowargs(row, tab)
        self.call("svg_op_dpmpp_step", P(xv), P(eud), P(ecd), float(g or 0.0), P(mpv), P(ov), P(mv), n, *ra)
        return self.finish({"out": (ob, ov, n, 0), "m": None if m == "null" else (mb, mv, n, 0)},
                           [(None if inplace else xv, x), (None if m == "alias" else mpv, mp), (eud, eu), (ecd, ec)])

    def lms(self, x, eu, ec, g, ring, row, tab=None, inplace=False, off=(0, 0, 0, 0, 0)):
        n = x.numel()
        xb, xv = self.buf(x, n, off[0])
        euv = self.buf(eu, n, off[1])[1]
        ecv = None if ec is None else self.buf(ec, n, off[2])[1]
        rb, rv = self.buf(ring, 4 * n, off[3])
        ob, ov = (xb, xv) if inplace else self.buf(None, n, off[4])
        assert [t.data_ptr() % 16 for t in (xv, euv, rv, ov)] == [4 * (o % 4) for o in (off[0], off[1], off[3], off[0] if inplace else off[4])]
        ra, keep = self.rowargs(row, tab)
        order, step = (int(row[2]), int(row[3])) if tab else (0, -1)
        self.call("svg_op_lms_step", P(xv), P(euv), P(ecv), float(g or 0.0), P(rv), P(ov), n, *ra, order, step)
        r = self.finish({"out": (ob, ov, n, off[0] if inplace else off[4]), "ring": (rb, rv, 4 * n, off[3])},
                        [(None if inplace else xv, x), (euv, eu), (ecv, ec)])
        r.ring = r.ring.reshape(4, n)
        return r

    def lms_input(self, x, c, tab=None, want_o1=True, inplace=False, off=(0, 0, 0)):
        n = x.numel()
        xb, xv = self.buf(x, n, off[0])
        b0, v0 = (xb, xv) if inplace else self.buf(None, n, off[1])
        b1, v1 = self.buf(None, n, off[2]) if want_o1 else (None, None)
        row = torch.tensor([SENTINEL, c] + [SENTINEL] * 6, dtype=F32)
        (_, tp, ip), keep = self.rowargs(row, tab) if tab else ((None, None, None), None)
        self.call("svg_op_lms_input", P(xv), P(v0), P(v1), n, 0.0 if tab else float(c), tp, ip)
        return self.finish({"o0": (b0, v0, n, off[0] if inplace else off[1]), "o1": (b1, v1, n, off[2]) if want_o1 else None},
                           [(None if inplace else xv, x)])

    def tvec(self, table, r, nb):
        t, idx = table.cuda(), torch.tensor([r], dtype=I32).cuda()
        ob, ov = self.buf(None, nb)
        self.call("svg_op_sampler_tvec", P(ov), nb, P(t), P(idx))
        return self.finish({"out": (ob, ov, nb, 0)}, [(t, table), (idx, torch.tensor([r], dtype=I32))])

    def bump(self, ints, pos):
        d = ints.cuda()
        self.call("svg_op_sampler_bump", d.data_ptr() + 4 * pos)
        torch.cuda.synchronize()
        return R(out=d.cpu())


class Emu:
    """torch f32 on the CPU, operation by operation as the kernels state them.  fused: every a * b + c that the compiler may contract is
    one correctly rounded fma (the products the kernels write as fmaf are fused in both forms).  mut: one defect (MUTATIONS).
    mixed: lms_step takes 16-byte groups and a tail when n % 4 != 0 (the form the kernel supports and its launcher never selects)."""

    def __init__(self, fused=False, mut=None, mixed=False):
        self.fused, self.mut, self.mixed = fused, mut, mixed

    def mul_add(self, a, b, c):
        return fma32(a, b, c) if self.fused else a * b + c

    def row(self, row, tab):
        if tab is None:
            return row
        stride = 7 if self.mut == "table_stride_7" else 8
        return table_of(row, tab).reshape(-1)[stride * tab[0]:stride * tab[0] + 8]

    def combine(self, eu, ec, g, fma=False):
        """fma: the kernel writes this product as fmaf (LMS)"""
        if ec is None:
            return eu.clone()
        if self.mut == "cfg_swapped":
            eu, ec = ec, eu
        if self.mut == "cfg_guidance_on_ec_only":
            return eu + (f32c(g) * ec - eu)
        return fma32(f32c(g), ec - eu, eu) if fma else self.mul_add(f32c(g), ec - eu, eu)

    def written(self, new, old, nv=0, tail_defect=False):
        """what the launch leaves in a buffer that held `old` (None: NaN): items [0, 4 nv) by 16-byte groups, the rest by the scalar loop"""
        n = new.numel()
        old = torch.full_like(new, NAN) if old is None else old
        out = new.clone()
        if self.mut == "skip_second_trip":
            per = min(-(-max(nv, n - 4 * nv, 1) // 256), 8192) * 256
            out[4 * min(nv, per):4 * nv] = old[4 * min(nv, per):4 * nv]
            out[4 * nv + min(n - 4 * nv, per):] = old[4 * nv + min(n - 4 * nv, per):]
        if self.mut == "lms_tail_start" and tail_defect and n > 4 * nv:
            out[4 * nv] = old[4 * nv]
        return out

    def ddim(self, x, eu, ec, g, row, tab=None, inplace=False):
        r = self.row(row, tab)
        sa, s1a, sap, s1ap = r[1], r[2], r[3], r[4]
        e = self.combine(eu, ec, g)
        raw = self.mul_add(-s1a, e, x) / sa
        x0 = raw if self.mut == "ddim_no_clip" else raw.clamp(-1.0, 1.0)
        if self.mut == "ddim_clip_output":
            out = (sap * raw + s1ap * e).clamp(-1.0, 1.0)
        else:
            out = fma32(s1ap, e, sap * x0) if self.fused else sap * x0 + s1ap * e
        return R(out=self.written(out, x if inplace else None))

    def dpmpp(self, x, eu, ec, g, mp, row, tab=None, inplace=False, m="out"):
        r = self.row(row, tab)
        inv_a, sig, cx, cd, k = r[1], r[2], r[3], r[4], r[5]
        e = self.combine(eu, ec, g)
        mm = self.mul_add(-sig, e, x) * inv_a
        d = mm
        if float(k) != 0:
            prev = mm if (self.mut == "dpmpp_mprev_after_write" and m == "alias") else mp
            d = self.mul_add(-k if self.mut == "dpmpp_k_sign" else k, mm - prev, mm)
        if float(r[6]) != 0 and self.mut != "dpmpp_last_ignored":
            out = mm.clone()
        else:
            out = fma32(cd, d, cx * x) if self.fused else cx * x + cd * d
        old_m = mp if m == "alias" else None
        m_new = None if m == "null" else self.written(mm, old_m)
        if self.mut == "dpmpp_no_m_out" and m != "null":
            m_new = self.written(torch.full_like(mm, NAN) if old_m is None else old_m, old_m)
        return R(out=self.written(out, x if inplace else None), m=m_new)

    def lms(self, x, eu, ec, g, ring, row, tab=None, inplace=False, off=(0, 0, 0, 0, 0)):
        r = self.row(row, tab)
        n, order, slot = x.numel(), int(r[2]), int(r[3]) & 3
        c0, c1, c2, c3 = r[4], r[5], r[6], r[7]
        offs = [o for o, p in zip(off, (x, eu, ec, ring, x)) if p is not None]
        offs[-1] = off[0] if inplace else off[4]
        nv = lms_groups(n, not self.mixed, offs)
        ring = ring.reshape(4, n)
        if self.mut == "lms_tail_ec_index" and ec is not None and n > 4 * nv:
            ec = torch.cat([ec[:4 * nv], ec[:n - 4 * nv]])
        e = self.combine(eu, ec, g, fma=True)
        if self.mut == "lms_c2_c3_swapped":
            c2, c3 = c3, c2
        acc = c0 * e
        if order > 1:
            acc = fma32(c1, ring[(slot + 1) & 3 if self.mut == "lms_order2_slot" else (slot + 3) & 3], acc)
        if order > 2:
            acc = fma32(c2, ring[(slot + 2) & 3], acc)
        if order > 3:
            acc = fma32(c3, ring[(slot + 1) & 3], acc)
        out = fma32(c0, e, x) if (self.fused and order == 1) else x + acc
        ring2 = ring.clone()
        ring2[slot] = self.written(eu if self.mut == "lms_store_before_combine" else e, ring[slot], nv, True)
        return R(out=self.written(out, x if inplace else None, nv, True), ring=ring2)

    def lms_input(self, x, c, tab=None, want_o1=True, inplace=False, off=(0, 0, 0)):
        row = torch.tensor([SENTINEL, c] + [SENTINEL] * 6, dtype=F32)
        cc = self.row(row, tab)[1]
        n = x.numel()
        nv = lms_groups(n, False, [off[0], off[0] if inplace else off[1]] + ([off[2]] if want_o1 else []))
        v = x * cc
        o1 = None
        if want_o1:
            o1 = torch.full_like(v, NAN) if self.mut == "lms_input_no_o1" else self.written(v, None, nv, True)
        return R(o0=self.written(v, x if inplace else None, nv, True), o1=o1)

    def tvec(self, table, r, nb):
        if self.mut == "tvec_next_row":
            r = min(r + 1, table.shape[0] - 1)
        return R(out=table[r, 0].expand(nb).clone())

    def bump(self, ints, pos):
        out = ints.clone()
        out[pos] += 2 if self.mut == "bump_by_2" else 1
        return R(out=out)


# =====================================================================================================================================
# the fp64 references and their bounds
# =====================================================================================================================================
def ref_combine(eu, ec, g):
    e = eu.to(F64)
    if ec is None:
        return e, torch.zeros_like(e)
    d = ec.to(F64) - e
    e = e + g * d
    return e, 2 * E * abs(g) * d.abs() + E * e.abs()


def ref_ddim(x, eu, ec, g, row):
    sa, s1a, sap, s1ap = [float(v) for v in row[1:5]]
    e, de = ref_combine(eu, ec, g)
    num = x.to(F64) - s1a * e
    x0 = num / sa
    dx0 = (E * ((s1a * e).abs() + num.abs()) + abs(s1a) * de) / abs(sa) + E * x0.abs()
    x0c = x0.clamp(-1.0, 1.0)
    out = sap * x0c + s1ap * e
    dout = abs(sap) * dx0 + E * (sap * x0c).abs() + abs(s1ap) * de + E * (s1ap * e).abs() + E * out.abs()
    return out, SLACK * dout, x0, SLACK * dx0


def ref_dpmpp(x, eu, ec, g, mp, row):
    inv_a, sig, cx, cd, k = [float(v) for v in row[1:6]]
    e, de = ref_combine(eu, ec, g)
    x64 = x.to(F64)
    u = x64 - sig * e
    m = u * inv_a
    dm = abs(inv_a) * (E * (sig * e).abs() + abs(sig) * de + E * u.abs()) + E * m.abs()
    d, dd = m, dm + E * m.abs()
    if k != 0:
        diff = m - mp.to(F64)
        d = m + k * diff
        dd = dm + abs(k) * (dm + E * diff.abs()) + E * (k * diff).abs() + E * d.abs()
    if float(row[6]) != 0:
        return m, SLACK * dm, m, SLACK * dm
    out = cx * x64 + cd * d
    dout = E * (cx * x64).abs() + abs(cd) * dd + E * (cd * d).abs() + E * out.abs()
    return out, SLACK * dout, m, SLACK * dm


def ref_lms(x, eu, ec, g, ring, row):
    order, slot = int(row[2]), int(row[3]) & 3
    c = [float(v) for v in row[4:8]]
    e, de = ref_combine(eu, ec, g)
    terms = [c[0] * e] + [c[k] * ring[(slot - k) & 3].to(F64) for k in range(1, order)]
    x64 = x.to(F64)
    out = x64 + sum(terms)
    return out, SLACK * (16 * E * (x64.abs() + sum(t.abs() for t in terms)) + abs(c[0]) * de), e, SLACK * de


# =====================================================================================================================================
# cases
# =====================================================================================================================================
# rule, n, row name, guidance (None: eps_c null), tab (None: argument row; (r, rows)), inplace, m (DPM++: "out" / "null" / "alias"),
# off (floats each pointer starts past a 16-byte boundary), data ("random" / "edge"), pad4 (compare with the run on the next multiple of 4),
# c / want_o1 (lms_input), r / nb (tvec), pos / start (bump)
Case = collections.namedtuple("Case", "rule n row g tab inplace m off data pad4 want_o1",
                              defaults=("", None, None, False, "out", None, "random", False, True))
KERNELS = ["ddim_step", "dpmpp_step", "lms_step", "lms_input", "sampler_tvec", "sampler_bump"]


@functools.lru_cache(maxsize=None)
def cases(kernel, big=True):
    C = []
    if kernel == "ddim_step":
        for row in rows("ddim"):
            for g in GUIDANCE:
                C += [Case("ddim", n, row, g) for n in (SIZES if row.startswith("t") else (5, 257))]
                C.append(Case("ddim", 257, row, g, data="edge"))
        for g in (None, 7.5):
            C += [Case("ddim", 257, "t500", g, tab=tab) for tab in TABS]
            C += [Case("ddim", n, "t20", g, inplace=True) for n in (5, 1001)]
            C.append(Case("ddim", 257, "t0", g, tab=TABS[1], inplace=True, data="edge"))
        if big:
            C.append(Case("ddim", BIG_SCALAR, "t500", 7.5, tab=TABS[2], inplace=True))
    elif kernel == "dpmpp_step":
        for row in rows("dpmpp"):
            for g in GUIDANCE:
                C += [Case("dpmpp", n, row, g, m=("null" if n in (3, 256) else "out")) for n in (SIZES if row.startswith("t") else (5, 257))]
        for row in ("t980_o1", "t500_o2", "t0_last", "syn_last_k"):
            for g in (None, 7.5):
                C += [Case("dpmpp", 257, row, g, tab=tab) for tab in TABS]
                C += [Case("dpmpp", 1001, row, g, inplace=True), Case("dpmpp", 1001, row, g, m="alias"), Case("dpmpp", 1001, row, g, inplace=True, m="alias"),
                      Case("dpmpp", 5, row, g, tab=TABS[1], inplace=True, m="alias")]
        if big:
            C.append(Case("dpmpp", BIG_SCALAR, "t500_o2", 7.5, tab=TABS[0], inplace=True, m="alias"))
    elif kernel == "lms_step":
        for row in rows("lms"):
            for g in GUIDANCE:
                C += [Case("lms", n, row, g, pad4=(n in (5, 1001) and g in (None, 7.5))) for n in (SIZES if row.startswith("s") else (5, 256))]
        for row in ("s0", "s2", "s5", "s8"):
            for g in (None, 7.5):
                C += [Case("lms", n, row, g, tab=tab) for tab in TABS for n in (256, 257)]
                C += [Case("lms", n, row, g, inplace=True) for n in (1001, 2048)]
                for p in range(5):                                            # x, eps_u, eps_c, dhist, x_out in turn 4 bytes off
                    if p != 2 or g is not None:
                        C.append(Case("lms", 2048, row, g, off=tuple(int(q == p) for q in range(5))))
                C.append(Case("lms", 256, row, g, tab=TABS[1], inplace=True, off=(1, 0, 0, 0, 1)))
        if big:
            C += [Case("lms", BIG_VEC, "s5", 7.5, inplace=True), Case("lms", BIG_SCALAR, "s8", -2.0, off=(1, 0, 0, 0, 1))]
    elif kernel == "lms_input":
        for row in ("s0", "s4", "s8", "syn_o4", "syn_o3", "syn_o1"):
            C += [Case("lms_input", n, row, want_o1=(n != 4), pad4=(n % 4 != 0)) for n in SIZES]
        for row in ("s4", "syn_o4"):
            C += [Case("lms_input", 257, row, tab=tab, want_o1=(tab[0] != 2)) for tab in TABS]
            C += [Case("lms_input", n, row, inplace=True, want_o1=(n == 2048)) for n in (5, 1001, 2048)]
            C += [Case("lms_input", 2048, row, off=tuple(int(q == p) for q in range(3))) for p in range(3)]
            C.append(Case("lms_input", 1001, row, tab=TABS[2], inplace=True, off=(1, 1, 0)))
        if big:
            C += [Case("lms_input", BIG_VEC + 3, "s4", inplace=True), Case("lms_input", BIG_SCALAR, "s4", tab=TABS[1], off=(0, 1, 0), want_o1=False)]
    elif kernel == "sampler_tvec":
        C = [Case("tvec", nb, "s%d" % (nb % 9), tab=tab) for nb in (1, 63, 64, 65, 130) for tab in TABS]
    elif kernel == "sampler_bump":
        C = [Case("bump", pos, "", g=start) for pos in (0, 4, 8) for start in (0, 7, 48)]                      # n: the counter's place among 9 ints
    return tuple(C)


def label_of(c):
    s = "%s n %d row %s" % (c.rule, c.n, c.row)
    s += "" if c.g is None else " g %g" % c.g
    s += (" table row %d of %d" % c.tab if c.tab else "") + (" in place" if c.inplace else "")
    s += (" m %s" % c.m if c.rule == "dpmpp" else "") + (" off %s" % (c.off,) if c.off else "") + (" %s" % c.data if c.data != "random" else "")
    return s


def key_of(c):
    return (len(c.rule), c.n, sorted(rows("lms" if c.rule in ("lms_input", "tvec") else c.rule)).index(c.row), GUIDANCE.index(c.g), c.data == "edge")


def eps_pair(c, n, g):
    eu = torch.randn(n, generator=g)
    return eu, (None if c.g is None else torch.randn(n, generator=g))


def same(a, b):
    """0 if the two runs returned the same bits in every output that the first one has, else inf"""
    return max([exact(v, getattr(b, k)) if getattr(b, k) is not None else INF for k, v in vars(a).items() if k != "ok" and v is not None] + [0.0])


# ---- DDIM -----------------------------------------------------------------------------------------------------------------------------
def ddim_data(c, row):
    g = _gen(*key_of(c))
    eu, ec = eps_pair(c, c.n, g)
    if c.data != "edge":
        return torch.randn(c.n, generator=g), eu, ec
    eu[:8] = 0.0
    if ec is not None:
        ec[:8] = 0.0
    t = 2.0 ** -20
    targets = torch.tensor([1.0, -1.0, 1.0, -1.0, 1 + t, 1 - t, -(1 + t), -(1 - t), 1.0, -1.0, 1 + t, 1 - t, -(1 + t), -(1 - t), 3.7, -250.0, 0.3, 1e4], dtype=F64)
    x0 = targets[torch.arange(c.n) % targets.numel()]
    e = ref_combine(eu, ec, c.g)[0]
    return (float(row[1]) * x0 + float(row[2]) * e).to(F32), eu, ec


def run_ddim(impl, T, c):
    row, label = rows("ddim")[c.row], label_of(c)
    x, eu, ec = ddim_data(c, row)
    r = impl.ddim(x, eu, ec, c.g, row, c.tab, c.inplace)
    out, dout, x0, dx0 = ref_ddim(x, eu, ec, c.g, row)
    T.add_ratio(c.data, label, ratio(r.out, out, dout))
    T.add_ratio("exact", label + ": guards, gaps, inputs", 0.0 if r.ok else INF)
    if c.data == "edge":
        assert int((x0.abs() == 1).sum()) >= 4 and bool(((x0.abs() - 1).abs() < 2e-6).sum() >= 12), "the edge data misses the clamp edge"
    far = x0.abs() > 1 + 2 * dx0
    if ec is None and bool(far.any()) and r.out.shape == x.shape:
        s = torch.sign(x0).to(F32)
        c1, c2 = row[3] * s + row[4] * eu, fma32(row[4], eu, row[3] * s)
        ok = (bits(r.out) == bits(c1)) | (bits(r.out) == bits(c2))
        T.add_ratio("exact", label + ": clipped elements", 0.0 if bool(ok[far].all()) else INF)
    if c.tab or c.inplace:
        T.add_ratio("exact", label + ": equals the argument row, out of place", same(r, impl.ddim(x, eu, ec, c.g, row)))


# ---- DPM++ ----------------------------------------------------------------------------------------------------------------------------
def run_dpmpp(impl, T, c):
    row, label = rows("dpmpp")[c.row], label_of(c)
    g = _gen(*key_of(c))
    eu, ec = eps_pair(c, c.n, g)
    x = torch.randn(c.n, generator=g)
    second = float(row[5]) != 0
    mp = torch.randn(c.n, generator=g) if second else torch.full((c.n,), NAN)
    r = impl.dpmpp(x, eu, ec, c.g, mp, row, c.tab, c.inplace, c.m)
    out, dout, m, dm = ref_dpmpp(x, eu, ec, c.g, mp, row)
    T.add_ratio("random", label, ratio(r.out, out, dout))
    T.add_ratio("exact", label + ": guards, gaps, inputs", 0.0 if r.ok else INF)
    if c.m == "null":
        T.add_ratio("exact", label + ": no m_out asked", 0.0 if r.m is None else INF)
    else:
        T.add_ratio("m_out", label, INF if r.m is None else ratio(r.m, m, dm))
        if float(row[6]) != 0:
            T.add_ratio("exact", label + ": a last row returns m", INF if r.m is None else exact(r.out, r.m))
    if c.tab or c.inplace or c.m == "alias":
        plain = impl.dpmpp(x, eu, ec, c.g, mp, row)
        T.add_ratio("exact", label + ": equals the argument row, out of place", same(r, plain))


# ---- LMS ------------------------------------------------------------------------------------------------------------------------------
def lms_data(c, n, row):
    """x, eps_u, eps_c, ring: the slots of the up to three steps before step i hold data, the others NaN (never written)"""
    g = _gen(*key_of(c))
    eu, ec = eps_pair(c, n, g)
    x = torch.randn(n, generator=g) * X_SCALE
    i = int(row[3])
    ring = torch.full((4, n), NAN)
    for k in range(1, min(i, 3) + 1):
        ring[(i - k) & 3] = torch.randn(n, generator=g)
    return x, eu, ec, ring


def run_lms(impl, T, c):
    row, label = rows("lms")[c.row], label_of(c)
    n4 = -(-c.n // 4) * 4 if c.pad4 else c.n
    X, EU, EC, RING = lms_data(c, n4, row)
    x, eu, ec, ring = X[:c.n].clone(), EU[:c.n].clone(), None if EC is None else EC[:c.n].clone(), RING[:, :c.n].clone()
    off = c.off or (0, 0, 0, 0, 0)
    r = impl.lms(x, eu, ec, c.g, ring, row, c.tab, c.inplace, off)
    out, dout, e, de = ref_lms(x, eu, ec, c.g, ring, row)
    slot = int(row[3]) & 3
    T.add_ratio("random", label, ratio(r.out, out, dout))
    T.add_ratio("exact", label + ": guards, gaps, inputs", 0.0 if r.ok else INF)
    if r.ring is None or r.ring.shape != ring.shape:
        T.add_ratio("exact", label + ": the ring", INF)
    else:
        T.add_ratio("ring", label, ratio(r.ring[slot], e, de))
        if ec is None:
            T.add_ratio("exact", label + ": the ring slot is eps_u", exact(r.ring[slot], eu))
        others = [s for s in range(4) if s != slot]
        T.add_ratio("exact", label + ": the other ring slots", exact(r.ring[others], ring[others]))
    if c.tab or c.inplace or c.off:
        T.add_ratio("exact", label + ": equals the argument row, out of place, aligned", same(r, impl.lms(x, eu, ec, c.g, ring, row)))
    if c.pad4:
        p = impl.lms(X, EU, EC, c.g, RING, row)
        p.out, p.ring = p.out[:c.n].clone(), (None if p.ring is None else p.ring[:, :c.n].clone())
        T.add_ratio("exact", label + ": equals the first n of the 16-byte run at n %d" % n4, same(r, p))


def run_lms_input(impl, T, c):
    row, label = rows("lms")[c.row], label_of(c) + " o1 %d" % c.want_o1
    n4 = -(-c.n // 4) * 4 if c.pad4 else c.n
    X = torch.randn(n4, generator=_gen(*key_of(c))) * X_SCALE
    x, cc = X[:c.n].clone(), float(row[1])
    off = c.off or (0, 0, 0)
    r = impl.lms_input(x, cc, c.tab, c.want_o1, c.inplace, off)
    want = x * row[1]
    T.add_ratio("exact", label, exact(r.o0, want))
    T.add_ratio("exact", label + " o1", (0.0 if r.o1 is None else INF) if not c.want_o1 else (INF if r.o1 is None else exact(r.o1, want)))
    T.add_ratio("exact", label + ": guards, gaps, inputs", 0.0 if r.ok else INF)
    if c.tab or c.inplace or c.off:
        T.add_ratio("exact", label + ": equals the argument, out of place, aligned", same(r, impl.lms_input(x, cc, want_o1=c.want_o1)))
    if c.pad4:
        p = impl.lms_input(X, cc, want_o1=c.want_o1)
        p.o0, p.o1 = p.o0[:c.n].clone(), (None if p.o1 is None else p.o1[:c.n].clone())
        T.add_ratio("exact", label + ": equals the first n of the run at n %d" % n4, same(r, p))


def run_tvec(impl, T, c):
    r, nrows = c.tab
    table = torch.full((nrows, 8), SENTINEL, dtype=F32)
    table[r] = rows("lms")[c.row]
    got = impl.tvec(table, r, c.n)
    T.add_ratio("exact", "nb %d row %d of %d" % (c.n, r, nrows), exact(got.out, table[r, 0].expand(c.n).contiguous()))
    T.add_ratio("exact", "nb %d: guard, table, counter" % c.n, 0.0 if got.ok else INF)


def run_bump(impl, T, c):
    ints = (torch.arange(9, dtype=I32) + 1) * 1000003
    ints[c.n] = c.g
    want = ints.clone()
    want[c.n] += 1
    T.add_ratio("exact", "counter %d at place %d of 9" % (c.g, c.n), exact(impl.bump(ints, c.n).out, want))


RUNNERS = {"ddim": run_ddim, "dpmpp": run_dpmpp, "lms": run_lms, "lms_input": run_lms_input, "tvec": run_tvec, "bump": run_bump}


class SamplerTally(Tally):
    def check(self, report, tag=""):
        assert self.worst, "%s: nothing was judged" % self.kernel
        for cls, (r, label) in sorted(self.worst.items()):
            print("[sampler_kernels] %-14s %-9s %-7s worst err/bound %.3f at %s" % (self.kernel, tag, cls, r, label))
            if report:
                margin("sampler kernel %s, %s class" % (self.kernel, cls), r, 1.0, unit="err/bound")
            else:
                assert r < 1.0, "%s %s: err/bound %.3g at %s" % (self.kernel, cls, r, label)
            if cls == "exact":
                assert r == 0.0, "%s: the exact class is not bit-equal at %s" % (self.kernel, label)


def run(impl, kernel, big=True, only=None):
    T = SamplerTally(kernel)
    for c in cases(kernel, big):
        if only is None or only(c):
            RUNNERS[c.rule](impl, T, c)
    return T


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------
def test_fma32_cpu():
    """fma32 is the correctly rounded a b + c: against exact rational arithmetic on draws, and on sums that the fp64 addition rounds onto a
    tie of f32 (c odd, a b = +-(half an ulp of c) (1 - 2^-46)), where rounding the fp64 sum again goes to the even neighbour, wrongly"""
    from fractions import Fraction
    g = _gen(60)
    a, b, c = [torch.randn(400, generator=g) * torch.exp2(torch.randint(-6, 6, (400,), generator=g).float()) for _ in range(3)]
    got = fma32(a, b, c)
    for i in range(400):
        want = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(want))
        cands = [float(near), float(np.nextafter(near, np.float32(np.inf))), float(np.nextafter(near, np.float32(-np.inf)))]
        dist = [abs(Fraction(v) - want) for v in cands]
        assert abs(Fraction(float(got[i])) - want) == min(dist) and dist.count(min(dist)) == 1, (i, float(got[i]), cands)
    c = (bits(torch.randn(512, generator=g)) | 1).view(F32)
    h = ((bits(c) + 1).view(F32).to(F64) - c.to(F64)).abs() / 2
    a = (h * (1 + 2.0 ** -23) * torch.where(torch.arange(512) % 2 == 0, 1.0, -1.0) * torch.sign(c).to(F64)).to(F32)
    b = torch.full((512,), 1 - 2.0 ** -23, dtype=F32)
    assert torch.equal(a.to(F64) * b.to(F64), a.to(F64) / (1 + 2.0 ** -23) * (1 - 2.0 ** -46))
    assert torch.equal(bits(fma32(a, b, c)), bits(c))
    assert not bool(((a.to(F64) * b.to(F64) + c.to(F64)).to(F32) == c).any())


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_emulation_cpu(kernel, fused):
    """the emulation of each kernel, fused and unfused, passes its judge on every case and data class: the bounds are attainable"""
    run(Emu(fused), kernel, big=not fused).check(report=False, tag="fused" if fused else "unfused")


# defect -> [(kernel, the data classes whose judge must reject it)]
ALL3 = ["ddim_step", "dpmpp_step", "lms_step"]
MUTATIONS = {"cfg_swapped": [(k, ["random"]) for k in ALL3],                                    # eu and ec exchanged in the combine
             "cfg_guidance_on_ec_only": [(k, ["random"]) for k in ALL3],                        # eu + (g ec - eu)
             "ddim_no_clip": [("ddim_step", ["random", "edge", "exact"])],
             "ddim_clip_output": [("ddim_step", ["random", "edge", "exact"])],                  # the clamp on the output instead of x0
             "dpmpp_k_sign": [("dpmpp_step", ["random"])],
             "dpmpp_mprev_after_write": [("dpmpp_step", ["random", "exact"])],                  # m_prev read after m_out went to the same buffer
             "dpmpp_last_ignored": [("dpmpp_step", ["random", "exact"])],
             "dpmpp_no_m_out": [("dpmpp_step", ["m_out"])],
             "lms_order2_slot": [("lms_step", ["random"])],                                     # the order-2 term from slot (slot + 1) & 3
             "lms_c2_c3_swapped": [("lms_step", ["random"])],
             "lms_store_before_combine": [("lms_step", ["ring"])],                              # eps_u stored to the ring under guidance
             "lms_tail_start": [("lms_step", ["random", "exact"]), ("lms_input", ["exact"])],   # the scalar tail starts at 4 nv + 1
             "lms_tail_ec_index": [("lms_step", ["random", "exact"])],                          # the tail reads ec at i - 4 nv (mixed form: see the top)
             "lms_input_no_o1": [("lms_input", ["exact"])],
             "table_stride_7": [(k, ["random", "exact"]) for k in ALL3] + [("lms_input", ["exact"])],
             "tvec_next_row": [("sampler_tvec", ["exact"])],                                    # row idx + 1
             "bump_by_2": [("sampler_bump", ["exact"])],
             "skip_second_trip": [(k, ["random"]) for k in ALL3] + [("lms_input", ["exact"])]}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_judges_reject_cpu(mut):
    """each defect of the emulation is outside the judges that see it (the sound emulation is inside: test_emulation_cpu)"""
    mixed = mut == "lms_tail_ec_index"
    for kernel, classes in MUTATIONS[mut]:
        big = mut == "skip_second_trip"
        only = (lambda c: c.n > GRID_CAP) if big else (lambda c: c.n % 4 != 0 and c.g is not None) if mixed else None
        if mixed:
            run(Emu(mixed=True), kernel, big=False, only=only).check(report=False, tag="mixed")
        T = run(Emu(mut=mut, mixed=mixed), kernel, big=big, only=only)
        rej = {cls: r >= 1.0 for cls, (r, _) in T.worst.items()}
        print("[sampler_kernels] mutation %-26s %-12s %s" % (mut, kernel, {c: "%.3g" % T.worst[c][0] for c in classes if c in T.worst}))
        assert all(rej.get(c, False) for c in classes), "the judge of %s accepts the defect %s in %s" % (kernel, mut, [c for c in classes if not rej.get(c)])


def test_coverage_cpu():
    """what the case list reaches: every rule with null and non-null eps_c, an argument row and a table row, in place and out of place; both
    LMS forms under guidance; every LMS order; first-order, second-order and last DPM++ rows; every size, and one beyond a trip per form"""
    for kernel, rule in (("ddim_step", "ddim"), ("dpmpp_step", "dpmpp"), ("lms_step", "lms")):
        C = cases(kernel)
        assert all(c.rule == rule for c in C)
        for g_null in (True, False):
            for tab in (True, False):
                for inplace in (True, False):
                    assert any((c.g is None) == g_null and bool(c.tab) == tab and c.inplace == inplace for c in C), (kernel, g_null, tab, inplace)
        assert {c.g for c in C} == set(GUIDANCE) and set(SIZES) <= {c.n for c in C} and any(c.n > GRID_CAP for c in C)
        assert {c.tab for c in C if c.tab} == set(TABS)
    L = cases("lms_step")
    form = lambda c: "vec" if lms_groups(c.n, True, [o for o, skip in zip(c.off or (0,) * 5, (0, 0, c.g is None, 0, c.inplace)) if not skip]) else "scalar"
    assert {(form(c), c.g is not None) for c in L} == {("vec", True), ("vec", False), ("scalar", True), ("scalar", False)}
    assert any(form(c) == "vec" and c.n > 4 * GRID_CAP for c in L) and any(form(c) == "scalar" and c.n > GRID_CAP and c.off for c in L)
    assert {int(rows("lms")[c.row][2]) for c in L} == {1, 2, 3, 4} and {int(rows("lms")[c.row][3]) for c in L} >= set(range(LMS_STEPS))
    assert any(c.pad4 and c.g is not None for c in L) and {p for c in L if c.off and sum(c.off) == 1 for p in range(5) if c.off[p]} == set(range(5))
    D = cases("dpmpp_step")
    assert {dpmpp_kind(rows("dpmpp")[c.row]) for c in D} == {"first", "second", "last"}
    assert {c.m for c in D} == {"out", "null", "alias"} and any(c.inplace and c.m == "alias" for c in D)
    assert not any(c.m == "null" and c.tab for c in D)                       # (the hook refuses nothing here: m_prev is always a buffer)
    assert any(c.data == "edge" and c.g is None for c in cases("ddim_step")) and any(c.data == "edge" and c.g is not None for c in cases("ddim_step"))
    I = cases("lms_input")
    assert any(c.tab for c in I) and any(c.inplace for c in I) and {c.want_o1 for c in I} == {True, False} and set(SIZES) <= {c.n for c in I}
    assert {p for c in I if c.off and sum(c.off) == 1 for p in range(3) if c.off[p]} == set(range(3))
    assert any(c.n > 4 * GRID_CAP and not c.off for c in I) and any(c.n > GRID_CAP and c.off for c in I) and any(c.pad4 for c in I)
    assert {c.n for c in cases("sampler_tvec")} == {1, 63, 64, 65, 130}
    for name, row in list(rows("ddim").items()) + list(rows("dpmpp").items()) + list(rows("lms").items()):
        assert row.dtype == F32 and row.shape == (8,) and bool(torch.isfinite(row).all()), name
    assert set(MUTATIONS) >= {"cfg_swapped", "skip_second_trip"} and len(MUTATIONS) == 18


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_against_fp64(ctx, kernel):
    run(Gpu(ctx), kernel).check(report=True)


@gpu
def test_refusals(ctx):
    """what the hooks refuse is a ValueError, nothing is launched (every output stays NaN), and the context computes the next valid call.
    Every buffer is sized for the call as made, and none of the refused calls would be safe to launch."""
    impl = Gpu(ctx)
    n = 64
    x, eu, mp = [torch.randn(n, device="cuda") for _ in range(3)]
    out, m_out = [torch.full((n,), NAN, device="cuda") for _ in range(2)]
    ring = torch.full((4 * n,), NAN, device="cuda")
    tab, idx = table_of(rows("lms")["s2"], (0, 1)).cuda(), torch.zeros(1, dtype=I32, device="cuda")
    host = lambda r: (ctypes.c_float * 8)(*[float(v) for v in r])
    lrow, drow, d2row = rows("lms")["s2"], rows("ddim")["t500"], rows("dpmpp")["t500_o2"]

    def refused(name, *args):
        with pytest.raises(ValueError):
            impl.call(name, *args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (out, m_out, ring)) and int(idx[0]) == 0
    lms = lambda order, step, row=None, t=None, i=None, xx=x, nn=n: refused("svg_op_lms_step", P(xx), P(eu), None, 0.0, P(ring), P(out), nn, row, P(t), P(i), order, step)
    for order, step in ((3, 1), (0, 2), (5, 6), (1, -1)):                    # order > i + 1, order and step out of range
        bad = lrow.clone()
        bad[2], bad[3] = order, step
        lms(0, -1, row=host(bad))                                           # an argument row: the launcher's own check
        lms(order, step, t=tab, i=idx)                                      # a table row: the stated order and step
    lms(0, -1, t=tab, i=idx)                                                # a table row without its order and step
    lms(3, 2, row=host(lrow), t=tab, i=idx)                                 # both ways at once
    lms(3, 2)                                                               # neither
    lms(3, 2, t=tab)                                                        # a table without its counter
    lms(3, 2, row=host(lrow), xx=None)                                      # a null tensor
    lms(3, 2, row=host(lrow), nn=-1)                                        # n < 0
    dp = lambda mprev, row=None, t=None, i=None, nn=n: refused("svg_op_dpmpp_step", P(x), P(eu), None, 0.0, P(mprev), P(out), P(m_out), nn, row, P(t), P(i))
    dp(None, row=host(d2row))                                               # second order without m_prev
    dp(None, t=tab, i=idx)                                                  # any table row without m_prev
    dp(mp, row=host(d2row), nn=-1)
    refused("svg_op_dpmpp_step", P(x), None, None, 0.0, P(mp), P(out), P(m_out), n, host(d2row), None, None)
    refused("svg_op_ddim_step", P(x), P(eu), None, 0.0, None, n, host(drow), None, None)
    refused("svg_op_ddim_step", P(x), P(eu), None, 0.0, P(out), -1, host(drow), None, None)
    refused("svg_op_ddim_step", P(x), P(eu), None, 0.0, P(out), n, None, None, None)
    refused("svg_op_lms_input", None, P(out), None, n, 1.0, None, None)
    refused("svg_op_lms_input", P(x), P(out), None, -1, 1.0, None, None)
    refused("svg_op_lms_input", P(x), P(out), None, n, 1.0, P(tab), None)
    refused("svg_op_sampler_tvec", P(out), 0, P(tab), P(idx))
    refused("svg_op_sampler_tvec", P(out), 4, None, P(idx))
    refused("svg_op_sampler_bump", None)
    for kernel in ("ddim_step", "lms_step"):
        run(impl, kernel, big=False, only=lambda c: c.n == 257).check(report=False)
