"""CPU: the GEMM / conv dispatch decision (csrc/gemm_plan.cpp: kernel family, column tile, split-K, GroupNorm rows and LayerNorm tiles per
launch) is a pure host function, so it is pinned by equality.  tools/host_sanitize/gemm_plan_dump.cpp (built host-only under ASan + UBSan, no
kernel file involved: a few seconds) prints `family bn splitk gn_rows ln_tiles fused_qkv_ok halo_width` for every descriptor of
tests/gemm_dispatch_cases.txt: every GEMM / conv problem of the bench workload (profile tags and a dry planning pass of the UNet and the VAE)
and both sides of every threshold in the predicates.  The expected tables were recorded from the five hand-copied dispatch cascades that
gemm_plan() replaced (gemm_describe after plan_splitk, gemm_emits_gn, gemm_ln_tiles, gemm_fused_qkv_supported, conv_halo_supported ?
conv_halo_bn : 0), under the default environment and under SVG_HALO_MIN=1 (what the parity tests force): they are the reference, the code
under test never regenerates them.  When a kernel path is retuned on purpose, the table changes with it in the same commit, line by line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "host_sanitize")
CASES = os.path.join(ROOT, "tests", "gemm_dispatch_cases.txt")
# the switches the decision reads: a table belongs to one setting of them
SWITCHES = ("SVG_HALO_MIN", "SVG_NO_HALO", "SVG_HALO_UP2", "SVG_HALO_SPLIT_TGT", "SVG_GEMM_WS", "SVG_GEMM_PP", "SVG_GEMM_PP_MINKT", "SVG_GEMM_BN",
            "SVG_IGEMM_SK")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None, reason="needs hipcc + make")


@pytest.fixture(scope="module")
def dump():
    r = subprocess.run(["make", "-C", TOOL, "build/gemm_plan_dump"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(TOOL, "build", "gemm_plan_dump")

    def run(*args, **env):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        r = subprocess.run([exe, *args, CASES], capture_output=True, text=True, timeout=120, env=e)
        assert r.returncode == 0 and "runtime error:" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]
        return r.stdout.splitlines()
    return run


def cases():
    with open(CASES) as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]


@pytest.mark.parametrize("table,env", [("gemm_dispatch_expected.txt", {}), ("gemm_dispatch_expected_halo_min1.txt", {"SVG_HALO_MIN": "1"})])
def test_plan_equals_the_recorded_dispatch(dump, table, env):
    with open(os.path.join(ROOT, "tests", table)) as f:
        want = f.read().splitlines()
    got = dump(**env)
    desc = cases()
    assert len(got) == len(want) == len(desc)
    bad = ["%s: got %s, recorded %s" % (d, g, w) for d, g, w in zip(desc, got, want) if g != w]
    assert not bad, "%d of %d decisions changed:\n%s" % (len(bad), len(desc), "\n".join(bad[:20]))


def test_recorded_table_covers_every_path():
    """the cap that keeps a hole out of the table: every family, every tile width, split-K on and off, every GroupNorm tile height,
    LayerNorm emit on and off occur in the recorded decisions"""
    with open(os.path.join(ROOT, "tests", "gemm_dispatch_expected.txt")) as f:
        rows = [tuple(int(v) for v in ln.split()) for ln in f]
    assert {r[0] for r in rows} == {0, 1, 2, 3}
    assert {r[1] for r in rows} >= {32, 64, 128, 160}
    assert {r[2] > 1 for r in rows} == {False, True}
    assert {r[3] for r in rows} == {0, 128, 256}
    assert {r[4] > 0 for r in rows} == {False, True}
    assert {r[5] for r in rows} == {0, 1} and {r[6] for r in rows} == {0, 128, 160}


@pytest.mark.parametrize("env", [{}, {"SVG_HALO_MIN": "1"}])
def test_plan_does_not_change_once_the_statistics_are_asked_for(dump, env):
    """ask-then-launch: the plan of a problem before gn_part / ln_part are set equals the plan after they are set from it (gemm_auto turns a
    mismatch into an error; here: no descriptor of the list has one)"""
    assert dump("--stable", **env) == []
