"""The multi-way merge passes (runsk.hip: k_mergek and its planning kernels)
on the merge battery (merge_battery.py), bit for bit against np.sort of every
group of 2^(hi + lk) keys.

The battery's families put on the device what the numpy model
(test_merge_battery.py) pins on the CPU: chunks as full as fm fences allow,
chunks of one run (K - 1 empty segments), runs of zeros and all-ones keys cut
at the edges of a fence, a load row and the run, plateaus around the fences,
windows whose interpolated guess is far off, ragged last groups, and with the
capacity split chunks cut into unequal halves -- u32 at runs of 2^14 keys, u64
(each pattern in the high word, the low word and both) at 2^13, lk = 1..4.
After every pass the context is synchronised, so a chunk the planning kernels
rejected raises instead of showing only as a mismatch.

The default knobs run in this process; the planner knobs are read once per
process, so every other knob set (merge_battery.KNOB_SETS) runs in a child
process, one per key type, with the families built for the fm the plan has
under those knobs."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import merge_battery as B  # noqa: E402
from test_gpu_runs import ctx, expect, expectk, run_level  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(np.uint32, 14), (np.uint64, 13)]
IDS = ["u32", "u64"]


def run_battery(ctx, dt, hi, lk, fm, fgl=B.FG_LOG2, families=None, kind="run_mergek", nfull=2):
    """Every key array of the battery (built for chunks of fm fences of 2^fgl
    keys) through one pass; the names that differ from numpy, and the number run."""
    bad, count = [], 0
    for name, x in B.battery(dt, hi, lk, B.battery_n(hi, lk, nfull), fm, 1 << fgl, families):
        got = run_level(ctx, x, hi, kind, lk if kind == "run_mergek" else 0)
        ctx.synchronize()  # MISORT_E_INTERNAL if the pass rejected a chunk
        want = expectk(x, hi, lk) if kind == "run_mergek" else expect(x, hi)
        if not np.array_equal(got, want):
            bad.append((name, int(np.flatnonzero(got != want)[0])))
        count += 1
    return bad, count


@pytest.mark.parametrize("lk", [1, 2, 3, 4])
@pytest.mark.parametrize("dt,hi", CASES, ids=IDS)
def test_battery_default_knobs(ctx, dt, hi, lk):
    """Fused planning with k_fence_rank, the worst-case fm: the whole battery."""
    n, fm, split, fgl = B.battery_plan(dt, hi, lk)
    assert not split and fgl == B.FG_LOG2
    bad, count = run_battery(ctx, dt, hi, lk, fm)
    assert not bad and count >= 20, bad


@pytest.mark.parametrize("hi", [13, 15])
@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=IDS)
def test_battery_two_way_level(ctx, dt, hi):
    """The K = 2 battery (built as for a 2-way multi-way pass) through the
    2-way merge level of runs.hip."""
    bad, count = run_battery(ctx, dt, hi, 1, B.shape(1, np.dtype(dt).itemsize)["FM"], kind="run_merge")
    assert not bad and count >= 20, bad


CHILD = r"""
import os, sys, numpy as np
root, kb, knob_set = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "parallel-computing-mpi_amd")]
import misort
import merge_battery as B
import test_gpu_merge_battery as T
dt, hi = (np.uint32, 14) if kb == 4 else (np.uint64, 13)
knobs = B.KNOB_SETS[knob_set]
assert all(os.environ.get(k) == v for k, v in knobs.items())
ctx = misort.Context(0)
for spec in sys.argv[4:]:
    hi_, lk, fams, nfull = spec.split(":")
    lw, lk, nfull = int(hi_) if hi_ else hi, int(lk), int(nfull)
    n, fm, split, fgl = B.battery_plan(dt, lw, lk, knobs, nfull)  # the plan the pass makes under these knobs
    bad, count = T.run_battery(ctx, dt, lw, lk, fm, fgl, fams.split(",") if fams else None, nfull=nfull)
    print("LK", lk, "COUNT", count, "BAD", bad, flush=True)
ctx.close()
"""


def run_child(kb, knob_set, specs):
    """The battery in a child process under a knob set: specs =
    "hi:lk:families:full groups" (empty hi: the key type's shortest runs; empty
    families: all).  Returns the
    per-spec counts; fails on any mismatch."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MISORT_") or k == "MISORT_LIBRARY"}
    env.update(B.KNOB_SETS[knob_set])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(kb), knob_set, *specs], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = [x.split(None, 5) for x in r.stdout.splitlines() if x.startswith("LK ")]
    assert len(lines) == len(specs) and all(x[5] == "[]" for x in lines), r.stdout[-2000:]
    return [int(x[3]) for x in lines]


@pytest.mark.parametrize("knob_set", list(B.KNOB_SETS))
@pytest.mark.parametrize("dt,hi", CASES, ids=IDS)
def test_battery_knob_sets(dt, hi, knob_set):
    """The whole battery, lk = 1..4, in a child process under each knob set:
    unfused planning (k_fence_lds / k_fence_merge, k_fence_counts, k_bounds,
    k_chunk_desc) with the capacity split at its shipped add and at 40 fences
    more, fused planning without k_fence_rank, and the 64-key fence build fused
    and split.  Where the plan splits, the model shows that the run really cuts
    chunks: the clumped family has a cut in every full group."""
    kb = np.dtype(dt).itemsize
    knobs = B.KNOB_SETS[knob_set]
    for lk in (1, 2, 3, 4):
        n, fm, split, fgl = B.battery_plan(dt, hi, lk, knobs)
        assert fgl == B.fgl_of(knobs)
        if split:
            nfull = n >> (hi + lk)
            assert nfull == 2 and any(all(B.check_groups(x, hi, lk, fm, [g], True, fgl) >= 1 for g in range(nfull))
                                      for _, x in B.battery(dt, hi, lk, n, fm, 1 << fgl, ["clumped"])), lk
    counts = run_child(kb, knob_set, [":%d::2" % lk for lk in (1, 2, 3, 4)])
    assert min(counts) >= 20


@pytest.mark.parametrize("dt,hi", [(np.uint32, 21), (np.uint64, 19)], ids=IDS)
def test_global_fence_merge_levels(dt, hi):
    """Runs of 2^14 (u32) / 2^12 (u64) fences: too many for the in-LDS fence
    order, so without k_fence_rank the group's fences are merged by lk global
    fence merge levels.  lk = 2, one full group and the tail, clumped and
    clustered keys."""
    p = B.plans([B.battery_n(hi, 2, 1)], hi, 2, np.dtype(dt).itemsize, knobs=B.KNOB_SETS["norank"])[0]
    assert (p["rank"], p["a"], p["left"]) == (0, 0, 2)
    counts = run_child(np.dtype(dt).itemsize, "norank", ["%d:2:clumped,clustered:1" % hi])
    assert counts[0] >= 4


def test_bounds_line_probe(ctx):
    """k_bounds' line probe (one aligned 128-byte line around the guess before
    the gallop) runs from 2^17 searches: the smallest u32 16-way pass of 2^14-key
    runs whose plan turns it on -- unfused, with the capacity split -- on
    clumped and clustered keys.  The keys repeat group by group (the families
    depend on a key's run and position alone), so numpy sorts one group and
    the tail."""
    dt, hi, lk = np.uint32, 14, 4
    K, W = 1 << lk, 1 << hi
    lo, hi_n = 1, 1 << 28  # the plan's line is monotone in n
    assert B.plans([hi_n], hi, lk)[0]["line"] == 1
    while lo < hi_n:
        mid = (lo + hi_n) // 2
        if B.plans([mid], hi, lk)[0]["line"]:
            hi_n = mid
        else:
            lo = mid + 1
    n = lo
    p, before = B.plans([n, n - 1], hi, lk)
    assert (p["line"], before["line"], p["fuse"], p["split"]) == (1, 0, 0, 1) and 8 * 10**7 < n < 10**8
    nfull, tail = n >> (hi + lk), n & (K * W - 1)
    assert tail > 0
    for name, x1 in B.battery(dt, hi, lk, K * W + tail, p["fm"], B.FG, ["clumped", "clustered"]):
        x = np.concatenate([np.tile(x1[:K * W], nfull), x1[K * W:]])
        assert x.size == n
        got = run_level(ctx, x, hi, "run_mergek", lk)
        ctx.synchronize()
        w1 = expectk(x1, hi, lk)
        assert np.array_equal(got[nfull * K * W:], w1[K * W:]), name
        assert np.array_equal(got[:nfull * K * W].reshape(nfull, K * W), np.broadcast_to(w1[:K * W], (nfull, K * W))), name
