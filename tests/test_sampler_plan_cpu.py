"""CPU: the schedule plan of the sampling loop (csrc/sampler_plan.cpp: the DDIM, DPM-Solver++(2M) and LMS rows of a whole loop, the add_noise pair,
the scale of z on entry, the state buffers, the argument checks) is a pure host function, so it is pinned by equality.
tools/host_sanitize/sampler_plan_dump.cpp (built host-only under ASan + UBSan, no kernel file involved: a few seconds) prints, for every case of
tests/sampler_plan_cases.txt, the plan's scalars and every row as eight bit patterns, or `refused: <message>`.

tests/golden/sampler_plan_expected.txt.xz (9950 such lines, 757 KB as text, so kept xz-compressed; `xz -dc` shows it) was recorded from the code
this plan replaced: UnetModel::ddim_coefs and dpmpp_coefs, lms_coefs, and from UnetModel::sample_loop its argument checks, the lms_row lambda, the inline DDIM packing and the table loop.  Those needed a finalized model, so
a throw-away recorder held their bodies, cut verbatim out of the previous commit's sources by line number, around the same printing loop; it was
built twice (the library's compiler and flags, and gcc -O0) with identical output.  It is the reference: the code under test never
regenerates it.  The second judge is independent of both: the closed forms in numpy."""
import lzma
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "host_sanitize")
CASES = os.path.join(ROOT, "tests", "sampler_plan_cases.txt")
DDIM, DPMPP, LMS = 0, 1, 2
STEP_COUNTS = [1, 2, 3, 4, 5, 7, 25, 50, 1000]

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None, reason="needs hipcc + make")


def lines(name):
    """the lines of tests/<name> (.xz: decompressed) that are neither comments nor empty"""
    path = os.path.join(ROOT, "tests", name)
    with (lzma.open(path, "rt") if name.endswith(".xz") else open(path)) as f:
        return [ln.rstrip("\n") for ln in f if not ln.startswith("#") and ln.strip()]


EXPECTED = "golden/sampler_plan_expected.txt.xz"


def cases():
    out = []
    for ln in lines("sampler_plan_cases.txt"):
        kv = dict(tok.split("=") for tok in ln.split())
        out.append((int(kv["sampler"]), int(kv["steps"]), int(kv["start"])))
    return out


def valid(case):
    s, n, st = case
    return s in (DDIM, DPMPP, LMS) and 1 <= n <= 1000 and 0 <= st <= n and (s != LMS or st == 0)


@pytest.fixture(scope="module")
def got():
    r = subprocess.run(["make", "-C", TOOL, "build/sampler_plan_dump"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([os.path.join(TOOL, "build", "sampler_plan_dump"), CASES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error:" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    return r.stdout.splitlines()


def test_case_list_covers_every_path():
    """the condition of the two tests below: all three rules at every step count (LMS's single-step schedule, its order ramp 1 -> 4, 1000 / n
    with a remainder), DDIM and DPM++ from step 0, an interior step, the last step (the `last` row alone) and past it (the empty loop), and
    every refusal"""
    cs = cases()
    for s in (DDIM, DPMPP):
        for n in STEP_COUNTS:
            starts = {st for (s_, n_, st) in cs if (s_, n_) == (s, n)}
            assert {0, n - 1, n} <= starts, (s, n, starts)
            assert n < 3 or any(0 < st < n - 1 for st in starts), (s, n, starts)
    assert {n for (s, n, st) in cs if s == LMS and st == 0} >= set(STEP_COUNTS)
    bad = [c for c in cs if not valid(c)]
    assert any(s == LMS and 1 <= n <= 1000 and 0 < st <= n for s, n, st in bad)                  # LMS has no history to start from
    assert any(n < 1 for s, n, st in bad) and any(n > 1000 for s, n, st in bad)
    assert any(st < 0 for s, n, st in bad) and any(1 <= n <= 1000 and st > n for s, n, st in bad)
    assert any(s not in (DDIM, DPMPP, LMS) for s, n, st in bad)


def test_plan_equals_the_rows_of_the_replaced_code(got):
    want = lines(EXPECTED)
    cs = cases()
    assert sum(ln.startswith("plan ") for ln in want) == sum(valid(c) for c in cs)
    assert sum(ln.startswith("refused: ") for ln in want) == sum(not valid(c) for c in cs)
    assert len(want) == sum(1 + n if valid((s, n, st)) else 1 for s, n, st in cs)
    bad = ["line %d: got %s\n   recorded %s" % (i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), "%d of %d lines differ (%d got):\n%s" % (len(bad), len(want), len(got), "\n".join(bad[:6]))


# ---- the closed forms, in numpy: f64 arithmetic on the f32 sequential cumprod (tests/test_sampler_cpu.py, tests/test_lms_cpu.py) ----------
BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float32) ** 2
ABAR32 = np.cumprod(np.float32(1.0) - BETAS, axis=0)
assert ABAR32.dtype == np.float32
ABAR = ABAR32.astype(np.float64)
TRAIN_SIGMA = np.sqrt((1.0 - ABAR) / ABAR)


def f32_sqrt_pair(a):
    a = np.float32(a)
    return [np.sqrt(a), np.sqrt(np.float32(1.0) - a)]


def ddim_row(t, t_prev):
    a_p = ABAR32[t_prev] if t_prev >= 0 else np.float32(1.0)
    return [np.float32(t)] + f32_sqrt_pair(ABAR32[t]) + f32_sqrt_pair(a_p) + [0.0, 0.0, 0.0]


def lam(ab):
    return 0.5 * math.log(ab) - 0.5 * math.log1p(-ab)


def dpmpp_row(t, t_next, t_last):
    ab = float(ABAR[t])
    sig = math.sqrt(1.0 - ab)
    row = [float(t), 1.0 / math.sqrt(ab), sig, 0.0, 0.0, 0.0, 0.0, 0.0]
    if t_next < 0:
        row[6] = 1.0
        return row
    abn = float(ABAR[t_next])
    h = lam(abn) - lam(ab)
    row[3] = math.sqrt(1.0 - abn) / sig
    row[4] = -math.sqrt(abn) * math.expm1(-h)
    if t_last >= 0:
        row[5] = 0.5 / ((lam(ab) - lam(float(ABAR[t_last]))) / h)
    return row


def lms_schedule(n):
    ts = np.linspace(999, 0, n, dtype=float)
    lo, hi = np.floor(ts).astype(int), np.ceil(ts).astype(int)
    fr = ts - np.floor(ts)
    return ts, np.concatenate([(1 - fr) * TRAIN_SIGMA[lo] + fr * TRAIN_SIGMA[hi], [0.0]])


def lms_row(ts, sig, i):
    """c_k = the integral over [sigma_i, sigma_{i+1}] of the Lagrange basis on sigma_i ... sigma_{i-order+1}, as a polynomial in u = tau - sigma_i"""
    order = min(i + 1, 4)
    r = [sig[i - j] - sig[i] for j in range(order)]
    h = sig[i + 1] - sig[i]
    c = [0.0] * 4
    for k in range(order):
        others = [r[j] for j in range(order) if j != k]
        prim = np.polynomial.Polynomial.fromroots(others).integ() if others else np.polynomial.Polynomial([0.0, 1.0])
        c[k] = float(prim(h)) / float(np.prod([r[k] - x for x in others]))
    return [ts[i], 1.0 / math.sqrt(sig[i] * sig[i] + 1.0), float(order), float(i)] + c


def bits(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32).view(np.int32).astype(np.int64)


def test_plan_equals_the_closed_forms(got):
    """DDIM rows and the add_noise pair to the bit (f32 sqrt is correctly rounded on both sides); DPM++ and LMS rows, and sigma_0, within one
    f32 ulp: each is one rounding of a double, and libm's log / expm1 may differ from numpy's in the last place of the double"""
    it = iter(got)
    worst = {DDIM: 0, DPMPP: 0, LMS: 0}
    for s, n, st in cases():
        head = next(it)
        if not valid((s, n, st)):
            assert head.startswith("refused: "), ((s, n, st), head)
            continue
        kv = dict(tok.split("=") for tok in head.split()[1:])
        assert head.startswith("plan ") and (int(kv["sampler"]), int(kv["steps"]), int(kv["start"])) == (s, n, st)
        ratio = 1000 // n
        t_at = lambda i: (n - 1 - i) * ratio     # noqa: E731
        noisy = 0 < st < n
        assert int(kv["add_noise"]) == noisy and int(kv["scaled_input"]) == (s == LMS) and int(kv["state"]) == {DDIM: 0, DPMPP: 1, LMS: 4}[s]
        pair = f32_sqrt_pair(ABAR32[t_at(st)]) if noisy else [1.0, 0.0]
        assert [int(kv["noise_sa"], 16), int(kv["noise_s1a"], 16)] == list(bits(pair)), (s, n, st)
        ts, sig = lms_schedule(n) if s == LMS else (None, None)
        assert abs(int(kv["z_scale"], 16) - int(bits([sig[0] if s == LMS else 1.0])[0])) <= (1 if s == LMS else 0)
        for i in range(n):
            tok = next(it).split()
            assert int(tok[0]) == i and len(tok) == 9
            row = np.array([int(v, 16) for v in tok[1:]], dtype=np.uint32).view(np.int32).astype(np.int64)
            if s == LMS:
                want = lms_row(ts, sig, i)
            elif s == DPMPP:
                want = dpmpp_row(t_at(i), t_at(i) - ratio, t_at(i - 1) if i > st else -1)
            else:
                want = ddim_row(t_at(i), t_at(i) - ratio)
            w = bits(want)
            # an ulp apart = adjacent bit patterns of one sign; a zero of the closed form (an unused slot, c_k beyond the order) is exact
            d = np.abs(row - w)
            assert np.all((w != 0) | (row == 0)) and np.all((row >= 0) == (w >= 0)), ((s, n, st), i, tok, want)
            worst[s] = max(worst[s], int(d.max()))
            assert d.max() <= (0 if s == DDIM else 1), ((s, n, st), i, tok, want)
            assert row[0] == w[0]                                         # the timestep is exact under every rule
    assert next(it, None) is None
    print("[sampler plan] worst distance from the closed forms, in f32 ulps: DDIM %d, DPM++ %d, LMS %d" % (worst[DDIM], worst[DPMPP], worst[LMS]))
