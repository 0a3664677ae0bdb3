"""The merge battery (merge_battery.py) reaches the edges of the multi-way
pass's chunking -- pinned through the numpy model, CPU only.

For u32 keys in runs of 2^14 and u64 keys in runs of 2^13 (the shortest a pass
takes), lk = 1..4, at the battery's shape (two full groups, a tail group of
K - 1 runs and a short run): every family passes the chunking invariants
(check_groups), and over the whole battery some chunk is as full as a chunk of
fm fences can be, some chunk has K - 1 empty segments, the load rows reach the
most the fences allow, the capacity split cuts chunks in every full group into
unequal halves, and the window searches (refine = window_bound) take every
branch that well-formed fences can reach.  test_gpu_merge_battery.py runs the
same keys through the kernels.

Where the arithmetic of the chunks rules a target out, the test pins what is
reachable and proves the rest unreachable, each at its assertion:
* the ka == kb branch of the window search is dead for exact fence counts;
* halves of a cut chunk cannot differ by a factor of two at these shapes;
* the load rows cannot exceed a bound the older families already reach at
  some (dtype, lk);
* u64 groups of two runs of 2^13 keys hold fewer than 2 fm fences."""
import functools

import numpy as np
import pytest

import merge_battery as B

CASES = [(np.uint32, 14), (np.uint64, 13)]
IDS = ["u32", "u64"]


@functools.lru_cache(maxsize=None)
def summary(dt, lw, lk, knob_set, families=None):
    """The battery (or the named families of it) under a knob set, through
    check_groups and chunk_stats: per array its chunk records and the number of
    chunks cut, plus the plan's (fm, split, fgl)."""
    knobs = B.KNOB_SETS[knob_set] if knob_set else None
    n, fm, split, fgl = B.battery_plan(dt, lw, lk, knobs)
    K = 1 << lk
    out = {}
    for name, x in B.battery(dt, lw, lk, n, fm, 1 << fgl, families):
        ngroups = (x.size + (K << lw) - 1) // (K << lw)
        ncut = B.check_groups(x, lw, lk, fm, range(ngroups), split, fgl)
        assert split or ncut == 0
        out[name] = (B.chunk_stats(x, lw, lk, fm, split, fgl), ncut, x.size >> (lw + lk))
    return out, fm, split, fgl


@functools.lru_cache(maxsize=None)
def old_summary(dt, lw, lk):
    """The families the GPU suite ran before: uniform, dup, equal, interleaved."""
    n, fm, split, fgl = B.battery_plan(dt, lw, lk)
    return [c for kind in B.OLD_KINDS
            for c in B.chunk_stats(B.make_keys(kind, n, lw, lk, lk, fm, dt, 1 << fgl), lw, lk, fm, split, fgl)]


def chunks_of(summ):
    return [c for stats, _, _ in summ.values() for c in stats]


def full_chunk_pin(dt, lw, lk, fm, fgl):
    """The most keys a chunk of fm fences holds: run r of it holds c_r fences,
    sum c_r = fm; the run the chunk starts in holds c_0 FG keys at most (from
    its fence to the key before its next one) and every other run (c_r + 1) FG
    - 1 (the windows before its first and after its last fence): fm FG +
    (K - 1)(FG - 1).  A group of fewer than 2 fm fences has two chunks: the first
    starts every run at 0 (no windows before: fm FG at most), the second has
    fewer than fm fences -- u64, two runs of 2^13 keys: 128 fences, fm = 67."""
    K, FGk = 1 << lk, 1 << fgl
    if (K << lw) >> fgl < 2 * fm:
        assert (np.dtype(dt).itemsize, lk, lw) == (8, 1, 13)
        return fm * FGk
    return fm * FGk + (K - 1) * (FGk - 1)


def assert_full_chunk(summ, dt, lw, lk, fm, fgl):
    K, FGk = 1 << lk, 1 << fgl
    largest = max(c["size"] for c in chunks_of(summ))
    assert largest > (fm + K - 3) * FGk, (largest, (fm + K - 3) * FGk)
    assert largest == full_chunk_pin(dt, lw, lk, fm, fgl), (largest, full_chunk_pin(dt, lw, lk, fm, fgl))
    return largest


def rows_bound(dt, lw, lk, fm, fgl):
    """The most load rows a chunk of fm fences uses, m = RW / FG: the run it
    starts in ceil(c_0 / m), every other ceil((c_r + 1) / m) (the sizes of
    full_chunk_pin), in all at most floor((fm + m - 1 + (K - 1) m) / m); in a
    group of two chunks (see full_chunk_pin) ceil(c_r / m) each."""
    S = B.shape(lk, np.dtype(dt).itemsize, fgl)
    K, m = S["K"], S["RW"] >> fgl
    if (K << lw) >> fgl < 2 * fm:
        return (fm + K * (m - 1)) // m
    return (fm + m - 1 + (K - 1) * m) // m


def assert_gallops(summ):
    """A forward and a backward gallop of three or more probes from a guess that
    was really interpolated: the fence's key strictly between the window's two
    fence keys (from v == ka or v == kb the guess is an end of the window)."""
    s = [q for c in chunks_of(summ) for q in c["searches"] if q["inner"]]
    assert max((q["fwd"] for q in s), default=0) >= 3, "no forward gallop of 3 steps from an interpolated guess"
    assert max((q["bwd"] for q in s), default=0) >= 3, "no backward gallop of 3 steps from an interpolated guess"


@pytest.mark.parametrize("lk", [1, 2, 3, 4])
@pytest.mark.parametrize("dt,lw", CASES, ids=IDS)
def test_battery_without_split(dt, lw, lk):
    """Fused planning, the worst-case fm: no chunk can exceed CAP, and the
    battery fills chunks, empties segments and uses load rows as far as fm
    fences allow."""
    S = B.shape(lk, np.dtype(dt).itemsize)
    K = S["K"]
    summ, fm, split, fgl = summary(dt, lw, lk, None)
    assert (fm, split, fgl) == (S["FM"], False, B.FG_LOG2)
    assert {n.split("/")[0] for n in summ} == set(B.FAMILIES)
    old = old_summary(dt, lw, lk)
    largest = assert_full_chunk(summ, dt, lw, lk, fm, fgl)
    assert largest >= max(c["size"] for c in old)
    assert largest <= S["CAP"] and (fm + K) << fgl <= S["CAP"]
    assert any(c["size"] > 0 and sum(1 for s in c["seg"] if s == 0) == K - 1 for c in chunks_of(summ))
    # load rows: strictly more than the older families, unless those already
    # use the most a chunk of fm fences can (rows_bound) -- then as many
    rows, rows_old, top = max(c["rows"] for c in chunks_of(summ)), max(c["rows"] for c in old), rows_bound(dt, lw, lk, fm, fgl)
    assert rows_old <= rows <= top <= S["NROWS"]
    assert rows > rows_old or rows == rows_old == top, (rows, rows_old, top)
    print("full chunk", np.dtype(dt).name, lk, "bound", (fm + K) << fgl, "old", max(c["size"] for c in old), "battery", largest,
          "rows", rows_old, rows, top)


@pytest.mark.parametrize("knob_set", list(B.KNOB_SETS))
@pytest.mark.parametrize("lk", [1, 2, 3, 4])
@pytest.mark.parametrize("dt,lw", CASES, ids=IDS)
def test_battery_under_knob_sets(dt, lw, lk, knob_set):
    """The knob sets of the GPU battery: the invariants hold on every family
    with the plan's own fm (and the 64-key fences where the set selects them);
    where the plan splits, every full group of some key array has a chunk cut,
    and some cut is lopsided."""
    kb = np.dtype(dt).itemsize
    summ, fm, split, fgl = summary(dt, lw, lk, knob_set)  # check_groups ran on every array
    S = B.shape(lk, kb, fgl)
    K, FGk = S["K"], 1 << fgl
    assert fgl == (6 if knob_set.startswith("fg6") else 7)
    # the shipped add splits u32 8- and 16-way passes only; 40 more fences split everything
    assert split == (knob_set.endswith("add40") or (knob_set == "unfused" and kb == 4 and lk >= 3))
    if not split:
        assert fm == S["FM"]
        return
    assert fm > S["FM"] and ((fm + 1) // 2 + K) * FGk <= S["CAP"]
    # some key array has a cut chunk in each of its full groups
    def cut_groups(stats):
        return {c["group"] for c in stats if c["half"] == 0}
    assert any(nfull >= 2 and cut_groups(stats) >= set(range(nfull)) for stats, _, nfull in summ.values())
    halves = [c["halves"] for c in chunks_of(summ) if c["half"] == 0]
    assert all(max(h) <= S["CAP"] for h in halves)
    # A half of m fences holds between (m - K) FG + K and m FG + (K - 1)(FG - 1)
    # keys (a run with c fences of it: (c - 1) FG + 1 to (c + 1) FG - 1, the run
    # it starts in c FG at most), so with mid = fm // 2 one half is never twice
    # the other at these fm ...
    mid = fm // 2
    assert (fm - mid) * FGk + (K - 1) * (FGk - 1) <= 2 * ((mid - K) * FGk + K)
    # ... but the halves can differ by nearly 2 K FG.  On spread keys the
    # windows cancel (the older families differ by a fence or two); the battery
    # has a cut whose first half takes every window, (K - 1)(FG - 1) keys more
    # than its fences' worth (clumped/lopsided).  K = 2 and short groups: some
    # difference.
    diff = max(abs(a - b) for a, b in halves)
    assert diff > (K - 2) * FGk, (diff, (K - 2) * FGk)


@pytest.mark.parametrize("lk", [1, 2, 3, 4])
@pytest.mark.parametrize("dt,lw", CASES, ids=IDS)
def test_window_search_branches(dt, lw, lk):
    """Every branch of the window search that exact fence counts can reach:
    the run's last window (no kb), the answer at the window's first and last
    position, long gallops both ways.  The ka == kb branch (the midpoint guess
    inside a plateau) is dead: run r's lo fences before the fence f = (v, r0)
    are those with key <= v (r < r0) or key < v (r > r0), so ka <= v < kb or
    ka < v <= kb -- pinned as never taken, also under the split's searches."""
    for knob_set in (None, "unfused_add40"):
        summ = summary(dt, lw, lk, knob_set)[0]
        s = [q for c in chunks_of(summ) for q in c["searches"]]
        assert not any(q["eq"] for q in s)
        for branch in ("last", "at_a", "at_b"):
            assert any(q[branch] for q in s), branch
        assert_gallops(summ)


@pytest.mark.parametrize("lk", [2, 3, 4])
@pytest.mark.parametrize("dt,lw", CASES, ids=IDS)
def test_full_chunk_check_needs_clumped(dt, lw, lk):
    """The checks bite: without the clumped family no chunk is full.  (K = 2
    is left out: two_valued fills a chunk there too.)"""
    rest = tuple(f for f in B.FAMILIES if f != "clumped")
    summ, fm, _, fgl = summary(dt, lw, lk, None, rest)
    with pytest.raises(AssertionError):
        assert_full_chunk(summ, dt, lw, lk, fm, fgl)
    assert_full_chunk(summary(dt, lw, lk, None, ("clumped",))[0], dt, lw, lk, fm, fgl)


@pytest.mark.parametrize("dt,lw", CASES, ids=IDS)
def test_gallop_check_needs_clustered(dt, lw):
    """The checks bite: at K = 2 only the clustered family gallops both ways
    from an interpolated guess.  (At larger K the plateaus do as well.)"""
    rest = tuple(f for f in B.FAMILIES if f != "clustered")
    with pytest.raises(AssertionError):
        assert_gallops(summary(dt, lw, 1, None, rest)[0])
    assert_gallops(summary(dt, lw, 1, None, ("clustered",))[0])
