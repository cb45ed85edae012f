"""CPU: the forward plan of the latent Transformer (csrc/xf_plan.cpp: per-GEMM kernels, split-K walk or small-row walk, the chunk batch, the rows,
LDS bytes and stage count of a launch) and the stage tables of the two walks are pure host functions, so they are pinned by equality.
tools/host_sanitize/xf_plan_dump.cpp (built host-only under ASan + UBSan, no kernel file involved: a few seconds) prints
`form Bc rows lds_bytes n_stages refusal` for every case of tests/xf_dispatch_cases.txt and, with --table, every stage of the marked cases with
every field that is not zero, a pointer as region + offset (a parameter by its role, the workspace in allocation order, its high-water mark at the end).
The expected tables were recorded from the code this plan replaced (XfModel::forward's walk / walk_small / Bc expressions, xf_walk_usable,
xf_walk_small_usable and the tables xf_forward_walk / xf_forward_walk_small handed to the launch): they are the reference, the code under test
never regenerates them.  The replaced code predicted the stage count with hand-kept upper bounds; the plan counts the table itself, so a model
whose table fits kWalkMaxOps while the bound did not now takes the walk: those cases carry a comment in xf_dispatch_expected.txt."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "host_sanitize")
CASES = os.path.join(ROOT, "tests", "xf_dispatch_cases.txt")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None, reason="needs hipcc + make")


@pytest.fixture(scope="module")
def dump():
    r = subprocess.run(["make", "-C", TOOL, "build/xf_plan_dump"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(TOOL, "build", "xf_plan_dump")

    def run(*args):
        r = subprocess.run([exe, *args, CASES], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error:" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]
        return r.stdout.splitlines()
    return run


def lines(name):
    with open(os.path.join(ROOT, "tests", name)) as f:
        return [ln.rstrip("\n") for ln in f]


def cases():
    return [ln.strip() for ln in lines("xf_dispatch_cases.txt") if ln.strip() and not ln.startswith("#")]


def recorded():
    return [ln for ln in lines("xf_dispatch_expected.txt") if not ln.startswith("#")]


def test_plan_equals_the_recorded_dispatch(dump):
    got, want, desc = dump(), recorded(), cases()
    assert len(got) == len(want) == len(desc)
    bad = ["%s: got %s, recorded %s" % (d, g, w) for d, g, w in zip(desc, got, want) if g != w]
    assert not bad, "%d of %d decisions changed:\n%s" % (len(bad), len(desc), "\n".join(bad[:20]))


def test_tables_equal_the_recorded_tables(dump):
    """every scalar field and every pointer (as region + offset) of every stage, and the workspace high-water mark"""
    got, want = dump("--table"), lines("xf_tables_expected.txt")
    assert sum(ln.startswith("# ") for ln in want) >= 14 and sum(ln.startswith("high ") for ln in want) >= 14
    bad = ["line %d: got %s\n   recorded %s" % (i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), "%d of %d lines differ (%d got):\n%s" % (len(bad), len(want), len(got), "\n".join(bad[:6]))


def test_recorded_decisions_cover_every_path():
    """the cap that keeps a hole out of the list: every form, each cut into chunks and not, and both reasons for refusing the walk"""
    rows = [tuple(int(v) for v in ln.split()) for ln in recorded()]
    batch = [int(dict(kv.split("=") for kv in c.split()).get("B", 1)) for c in cases()]
    assert len(rows) == len(batch)
    assert {(r[0], b > r[1]) for r, b in zip(rows, batch)} == {(f, c) for f in (0, 1, 2) for c in (False, True)}
    assert {r[5] for r in rows} == {0, 1, 2, 3}                                       # taken, off, shape, stage count
    assert all((r[0] == 0) == (r[5] != 0) and (r[0] == 0) == (r[4] == 0) for r in rows)
    assert {r[2] for r in rows if r[0] == 2} == {8} and max(r[4] for r in rows) <= 512
    # the tables: both forms, one buffer and two, an empty model
    heads = [ln for ln in lines("xf_tables_expected.txt") if ln.startswith("# ")]
    assert {("grid=8" in h, "same=1" in h) for h in heads} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any("enc=0 dec=0" in h for h in heads) and any("text_dim=128" in h for h in heads) and any("split=1" in h for h in heads)
