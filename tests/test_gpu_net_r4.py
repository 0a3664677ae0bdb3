"""The 4-byte register stages of the SORT, row and segment tiles as fused
radix-4 steps (csrc/net_r4.h) on the GPU, bit for bit against numpy.

The stages under change see at most one tile, so every size here is a tile or
two: u32 local sorts around the 2^14 and 2^15 tiles under both tile pins (the
pin is read once per process: one child process per pin), and one row-wise and
one segmented sort at the smallest row / segment length the tiles send past
level 8 (257 keys: a block of 2^9, so level 9 runs as LDS phases with the lists
(4,5,flip) and (3,4)).  The key-value row tile sorts 8-byte records and keeps
its compare-and-select stages, so it has no case here."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
import test_gpu_tile as TT  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1 << 14) - 1, 1 << 14, 1 << 15, (1 << 15) + 1, 3 * (1 << 14) + 5]
FAMILIES = ("iid", "ascending", "descending", "all_equal", "two_valued", "iid_tenth_max")
MAXK = np.uint32(0xFFFFFFFF)


def keys(family, n):
    rng = np.random.default_rng([n, FAMILIES.index(family)])
    if family == "all_equal":
        return np.full(n, 0x9E3779B9, dtype=np.uint32)
    if family == "two_valued":
        return np.where(rng.random(n) < 0.5, np.uint32(7), np.uint32(0xC0000000)).astype(np.uint32)
    x = rng.integers(0, 0xFFFFFFFF, size=n, dtype=np.uint32, endpoint=True)
    if family == "ascending":
        return np.sort(x)
    if family == "descending":
        return np.sort(x)[::-1].copy()
    if family == "iid_tenth_max":
        x[rng.random(n) < 0.1] = MAXK
    return x


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import misort
import test_gpu_net_r4 as M
import test_gpu_tile as TT
lt = int(sys.argv[3])
ctx = misort.Context(0)
assert misort.plan(1 << lt, 4) == [("tile_sort", lt - 1, 0, False)], misort.plan(1 << lt, 4)
for n in M.SIZES:
    assert misort.plan(n, 4)[0][:2] == ("tile_sort", lt - 1), (n, misort.plan(n, 4))
    for fam in M.FAMILIES:
        x = M.keys(fam, n)
        d = TT.to_dev(x)
        out = TT.to_dev(np.zeros(n, dtype=np.uint32))
        ctx.local_sort(d, out)
        got = TT.to_host(out, np.uint32)
        want = np.sort(x)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"tile 2^{lt}, n {n}, {fam}: first difference at key {i}: got {int(got[i]):#x}, "
                                 f"want {int(want[i]):#x}; {int(np.count_nonzero(got != want))} keys differ")
ctx.close()
print("NET_R4_CHILD OK")
"""


@pytest.mark.parametrize("lt", [14, 15])
def test_local_sort_u32_pinned_tile(lt):
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "parallel-computing-mpi_amd"),
                        os.path.join(ROOT, "tests"), str(lt)], env=dict(os.environ, MISORT_SORT_TILE_U32=str(lt)),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "NET_R4_CHILD OK", r.stdout[-1000:]


COLS = 257  # the smallest row the tiles sort as a block of 2^9 keys


def test_rows_u32_past_level_8(ctx):
    p = misort.rows_plan(COLS, 4)
    assert p["path"] == "tile" and p["block_log2"] == 9, p
    assert misort.rows_plan(COLS - 1, 4)["block_log2"] == 8
    rows = 2 * (1 << (p["tile_log2"] - 9)) + 3  # two tiles and a partial one
    x = keys("iid_tenth_max", rows * COLS).reshape(rows, COLS)
    x[1] = np.sort(x[1])
    x[2] = np.sort(x[2])[::-1]
    x[3] = 5
    x[4] = np.where(np.arange(COLS) % 3 == 0, 9, 2)
    got = TT.to_host(ctx.sort_rows(TT.to_dev(x)), np.uint32).reshape(rows, COLS)
    want = np.sort(x, axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:8].tolist(), got[bad[0]][:8].tolist(), want[bad[0]][:8].tolist())


def test_segments_u32_past_level_8(ctx):
    assert misort.segment_class(COLS, 4) == 9 and misort.segment_class(COLS - 1, 4) == 8
    rng = np.random.default_rng(77)
    # class-9 segments alone: 257 .. 512 keys, most of them the smallest
    lens = np.full(70, COLS, dtype=np.int64)
    lens[5:15] = rng.integers(COLS, 513, size=10)
    lens[20] = 512
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1]) + 2
    x = keys("iid_tenth_max", n)
    x[off[1]:off[2]] = np.sort(x[off[1]:off[2]])[::-1]
    x[off[2]:off[3]] = 0x1234
    x[off[3]:off[4]] = np.where(np.arange(COLS) % 2 == 0, MAXK, 0).astype(np.uint32)
    got = TT.to_host(ctx.sort_segments(TT.to_dev(x), torch.from_numpy(off).cuda()), np.uint32)
    want = x.copy()
    for a, b in zip(off[:-1], off[1:]):
        want[a:b] = np.sort(x[a:b])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), int(np.searchsorted(off, bad[0], side="right")) - 1)
