"""Segmented sort past one workgroup of offsets and past 2^31 keys
(misort_local_sort_segments, Context.sort_segments) against the host oracle of
segment_layouts.py.  Every comparison is on bit patterns; there is no tolerance.

test_gpu_segments.py covers lengths, key families, views and refusals with at
most 1281 segments, which one workgroup of k_seg_count / k_seg_scatter takes
(2048).  Here:

- the layouts of segment_layouts.py, 2049 .. 40000 segments: the sweeps' global
  atomics, the class cursors handing each workgroup its slice of a list, the
  last workgroup's partial trip, offsets[nseg] read by a later workgroup;
- malformed offsets in several workgroups: the count and the FIRST bad index;
- three long classes with mixed lengths on a fresh context (the scratch
  buffers start empty, their size comes from the middle class), then calls that
  need less and more;
- the profiler's per-class totals summed over ten workgroups;
- segments that start above key index 2^31 (byte offsets above 2^33), and an
  out-of-place fringe copy of more than 2^32 bytes.

Not here: the pad sweeps' grid cap (2^28 vectors) needs more than 2^30 padded
keys and a host oracle of that size."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
import segment_layouts as L  # noqa: E402
from guard_bands import assert_guards, canary_for  # noqa: E402
from test_gpu_segments import SPECIALS, banded, bits, to_dev, udt  # noqa: E402

pytestmark = pytest.mark.gpu

FAMS = ("random", "sentinels", "dups", "opposed_wide")
MERGES = ("run_merge", "run_mergek")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=4)
def case(name, dt, fam):
    """(keys, offsets, oracle) of a named layout, shared by the tests that need
    it; nobody writes them."""
    u = udt(dt)
    offs, n = L.layout(name, np.dtype(u).itemsize)
    k = L.make(fam, 1000 + len(name), offs, n, u)
    w = L.want(k, offs, dt)
    return k, offs, w


def both_ways(ctx, k, offs, w, dt, what=""):
    """One call out of place and one in place against w; input (out of place)
    and offsets unchanged."""
    d, o = to_dev(k, dt), torch.from_numpy(offs).cuda()
    out = ctx.sort_segments(d, o)
    assert out.shape == d.shape and out.dtype == d.dtype and out.data_ptr() != d.data_ptr()
    np.testing.assert_array_equal(bits(out), w, err_msg=what + " out of place")
    np.testing.assert_array_equal(bits(d), k, err_msg=what + " (input changed)")
    np.testing.assert_array_equal(o.cpu().numpy(), offs, err_msg=what + " (offsets changed)")
    assert ctx.sort_segments(d, o, out=d) is d
    np.testing.assert_array_equal(bits(d), w, err_msg=what + " in place")
    np.testing.assert_array_equal(o.cpu().numpy(), offs, err_msg=what + " (offsets changed in place)")


# ---- many segments ----------------------------------------------------------------------

def many_cases():
    for name in L.LAYOUTS:
        for dt in (np.uint32, np.uint64) + ((np.float64,) if name in ("mixed", "sparse") else ()):
            for fam in FAMS:
                yield pytest.param(name, dt, fam, id=f"{name}-{dt.__name__}-{fam}")


@pytest.mark.parametrize("name,dt,fam", list(many_cases()))
def test_many_segments(ctx, name, dt, fam):
    k, offs, w = case(name, dt, fam)
    both_ways(ctx, k, offs, w, dt, f"{name}, {fam}")


@pytest.mark.parametrize("dt", [np.uint32, np.uint64, np.float64], ids=lambda d: d.__name__)
def test_mixed_views_one_element_into_storage(ctx, dt):
    k, offs, w = case("mixed", dt, "random")
    n = k.size
    canary = canary_for(k)
    dbase_in, d = banded(k, 1, canary, dt)
    dbase_out, out = banded(np.full(n, canary, dtype=k.dtype), 1, canary, dt)
    o = torch.from_numpy(offs).cuda()
    assert ctx.sort_segments(d, o, out=out) is out
    np.testing.assert_array_equal(bits(out), w)
    assert_guards(bits(dbase_out), n, 1, canary)
    np.testing.assert_array_equal(bits(d), k)
    assert_guards(bits(dbase_in), n, 1, canary)
    np.testing.assert_array_equal(o.cpu().numpy(), offs)


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_mixed_fringes_between_guard_bands(ctx, u):
    """offsets[0] = 7 and nine keys after offsets[nseg]: the fringes are copied
    out of place and untouched in place, and nothing is written outside n keys."""
    kb = np.dtype(u).itemsize
    offs = L.offsets_of(L.mixed(kb), first=7)
    n = int(offs[-1]) + 9
    k = L.make("sentinels", 31, offs, n, u)
    w = L.want(k, offs, u)
    np.testing.assert_array_equal(w[:7], k[:7])
    np.testing.assert_array_equal(w[-9:], k[-9:])
    canary = canary_for(k)
    o = torch.from_numpy(offs).cuda()
    dbase_in, d = banded(k, 4, canary, u)
    dbase_out, out = banded(np.full(n, canary, dtype=u), 4, canary, u)
    assert ctx.sort_segments(d, o, out=out) is out
    np.testing.assert_array_equal(bits(out), w)  # the fringes are k's
    assert_guards(bits(dbase_out), n, 4, canary)
    np.testing.assert_array_equal(bits(d), k)
    assert_guards(bits(dbase_in), n, 4, canary)
    ctx.sort_segments(d, o, out=d)
    np.testing.assert_array_equal(bits(d), w)
    assert_guards(bits(dbase_in), n, 4, canary)
    np.testing.assert_array_equal(o.cpu().numpy(), offs)


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_all_empty_between_guard_bands(ctx, u):
    offs, n = L.layout("all_empty", np.dtype(u).itemsize)
    assert n == 16 and offs.size == 5001
    k = L.rand(np.random.default_rng(41), n, u)
    canary = canary_for(k)
    o = torch.from_numpy(offs).cuda()
    dbase_in, d = banded(k, 4, canary, u)
    dbase_out, out = banded(np.full(n, canary, dtype=u), 4, canary, u)
    assert ctx.sort_segments(d, o, out=out) is out
    np.testing.assert_array_equal(bits(out), k)  # the input bit for bit
    assert_guards(bits(dbase_out), n, 4, canary)
    ctx.sort_segments(d, o, out=d)
    np.testing.assert_array_equal(bits(d), k)  # nothing changed
    assert_guards(bits(dbase_in), n, 4, canary)
    np.testing.assert_array_equal(o.cpu().numpy(), offs)


def test_order_of_the_lists_does_not_matter(ctx):
    """The scatter's order inside a class list is whatever the atomics give:
    three calls, each bit-identical to the oracle."""
    k, offs, w = case("mixed", np.uint32, "random")
    d, o = to_dev(k), torch.from_numpy(offs).cuda()
    for i in range(3):
        np.testing.assert_array_equal(bits(ctx.sort_segments(d, o)), w, err_msg=f"call {i}")
    np.testing.assert_array_equal(bits(d), k)
    np.testing.assert_array_equal(o.cpu().numpy(), offs)


# ---- malformed offsets across workgroups -----------------------------------------------------

MALFORMED = {  # case: (planted bad pairs, other edits, the count and the first index meant)
    "last_partial_trip": ((8999,), None, (1, 8999)),
    "three_workgroups": ((7000, 2048, 4500), None, (3, 2048)),
    "last_past_n": ((), "last", (1, 9000)),
    "negative_first_and_5000": ((5000,), "first", (2, 0)),
}


def bad_pairs(offs, n):
    """The documented definition: segment i is malformed when b < 0 or e < b or
    e > n for (b, e) = (offsets[i], offsets[i + 1]).  (count, first index)."""
    b, e = offs[:-1], offs[1:]
    bad = (b < 0) | (e < b) | (e > n)
    return int(bad.sum()), int(np.flatnonzero(bad)[0])


@pytest.mark.parametrize("what", list(MALFORMED))
@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_malformed_offsets_across_workgroups(ctx, u, what):
    nseg = 9001
    offs = L.offsets_of(L.mixed(np.dtype(u).itemsize, nseg=nseg, long_at=(0, 2047, 2048, 4000, 8990, 9000, 6000)))
    n = int(offs[-1])
    k = L.rand(np.random.default_rng(51), n, u)
    planted, edit, meant = MALFORMED[what]
    for i in planted:
        assert offs[i] > 0
        offs[i + 1] = offs[i] - 1  # pair i decreases; pair i + 1 stays well formed
    if edit == "last":
        offs[nseg] = n + 1
    elif edit == "first":
        offs[0] = -1
    count, first = bad_pairs(offs, n)
    assert (count, first) == meant
    canary = canary_for(k)
    prefill = np.full(n, canary + 1, dtype=u)
    dbase, out = banded(prefill, 4, canary, u)
    d = to_dev(k)
    with pytest.raises(misort.MisortError) as ei:
        ctx.sort_segments(d, torch.from_numpy(offs).cuda(), out=out)
    assert ei.value.code == -1
    assert f"{count} of {nseg} segments" in str(ei.value) and f"index {first} " in str(ei.value)
    np.testing.assert_array_equal(bits(out), prefill)
    assert_guards(bits(dbase), n, 4, canary)
    np.testing.assert_array_equal(bits(d), k)


# ---- long classes on a fresh context ------------------------------------------------------------

def long_calls(kb):
    """Three calls' lengths and the segments per long class each must have."""
    t = misort.tile_log2(kb)
    T = 1 << t
    first = [0, 5, 2 * T, 700, 0, 2 * T + 1, 33, 4 * T - 1, 1, T, 4 * T, 0, 4 * T + 1, 64]
    second = [3, T + 1, 0, 2 * T - 1, 40]
    third = [4 * T + 1, 9, 8 * T - 1, 0, 8 * T, 6 * T + 5]
    return ((first, {t + 1: 1, t + 2: 3, t + 3: 1}), (second, {t + 1: 2}), (third, {t + 3: 4}))


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_long_classes_on_a_fresh_context(u):
    """Scratch sized by the middle class (3 << (t + 2) keys is the largest count
    << k), lengths mixed inside it (the shortest, 2^k - 1, exactly 2^k); then a
    call that needs less and one that needs more, on the same context."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    kb = np.dtype(u).itemsize
    t = misort.tile_log2(kb)
    fresh = misort.Context(0)
    try:
        for call, (lens, longs) in enumerate(long_calls(kb)):
            cls = [misort.segment_class(x, kb) for x in lens]
            assert {c: cls.count(c) for c in set(cls) if c > t} == longs
            if call == 0:
                assert max(longs, key=lambda c: longs[c] << c) == t + 2
            offs = L.offsets_of(lens)
            for fam in ("sentinels", "opposed_wide"):
                k = L.make(fam, 61 + call, offs, int(offs[-1]), u)
                both_ways(fresh, k, offs, L.want(k, offs, u), u, f"call {call}, {fam}")
    finally:
        fresh.close()


def test_long_classes_f64_specials_on_a_fresh_context():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = misort.tile_log2(8)
    lens = [len(SPECIALS), 2 << t, 50, (2 << t) - 1, 0, 1000]
    offs = L.offsets_of(lens)
    rng = np.random.default_rng(71)
    k = L.rand(rng, int(offs[-1]), np.uint64)
    pick = rng.random(k.size) < 0.6
    k[pick] = rng.choice(SPECIALS, int(pick.sum()))
    k[:len(SPECIALS)] = SPECIALS[::-1]
    for i in (1, 3):  # both long segments hold every special
        assert set(SPECIALS.tolist()) <= set(k[offs[i]:offs[i + 1]].tolist())
    fresh = misort.Context(0)
    try:
        both_ways(fresh, k, offs, L.want(k, offs, np.float64), np.float64, "specials")
    finally:
        fresh.close()


# ---- profiler across workgroups -------------------------------------------------------------------

def profiled(ctx, fn):
    ctx.profile(True)
    try:
        ctx.profile_reset()
        fn()
        torch.cuda.synchronize()
        return ctx.profile_read(), ctx.profile_trace()
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_profile_mixed(ctx, u):
    """test_profile_tile_classes where the header's per-class totals are sums
    over ten workgroups.  A long class's block passes start with a SORT pass,
    which is a tile_sort record too (2 count 2^k keys, as for the long rows of
    sort_rows): the trace holds the tile classes' records first, in class order,
    then one per long class, and both are pinned."""
    kb = np.dtype(u).itemsize
    t = misort.tile_log2(kb)
    k, offs, w = case("mixed", u, "random")
    lens = np.diff(offs)
    cls = L.classes_of(lens, kb)
    assert lens.size > 9 * L.WG
    tiles = sorted(set(cls[(cls >= 0) & (cls <= t)].tolist()))
    longs = sorted(set(cls[cls > t].tolist()))
    assert tiles == list(range(5, t + 1)) and len(longs) == 3
    d, o = to_dev(k), torch.from_numpy(offs).cuda()
    out = []
    rec, trace = profiled(ctx, lambda: out.append(ctx.sort_segments(d, o)))
    np.testing.assert_array_equal(bits(out[0]), w)
    tile_bytes = [2 * int(lens[cls == c].sum()) * kb for c in tiles]
    block_bytes = [2 * (int((cls == c).sum()) << c) * kb for c in longs]
    got = [b for kind, _, b in trace if kind == "tile_sort"]
    assert got[:len(tiles)] == tile_bytes  # one launch per tile class present, its keys from SEG_H_KEYS
    assert len(got) - len(longs) == len(tiles) and got[len(tiles):] == block_bytes
    assert sum(tile_bytes) == 2 * int(lens[lens <= (1 << t)].sum()) * kb
    launches, ms, nbytes = rec["tile_sort"]
    assert launches == len(tiles) + len(longs) and ms > 0.0 and nbytes == sum(tile_bytes) + sum(block_bytes)
    # count and scatter, a pad and an unpad per long class
    listed = int((lens > 0).sum())
    sweeps = 2 * 8 * (lens.size + 1) + 4 * listed
    pads = 2 * sum((int(lens[cls == c].sum()) + (int((cls == c).sum()) << c)) * kb for c in longs)
    assert rec["other"][0] == 2 + 2 * len(longs) and rec["other"][2] == sweeps + pads
    # the rest: what the passes of a plain 2^k-key sort record, nothing else
    for kind in MERGES:
        assert rec[kind][0] == sum(sum(1 for q in misort.rows_plan(1 << c, kb)["passes"] if q[0] == kind)
                                   for c in longs), kind
    plain_kinds = set()
    for c in longs:
        x = to_dev(L.rand(np.random.default_rng(81), 1 << c, u))
        plain, _ = profiled(ctx, lambda: ctx.local_sort(x, out=torch.empty_like(x)))
        plain_kinds |= {kind for kind in plain if plain[kind][0]}
    assert {kind for kind in rec if rec[kind][0]} <= {"tile_sort", "other"} | plain_kinds
    assert "other" not in plain_kinds


# ---- indices at and above 2^31 ---------------------------------------------------------------------

BIG_N = (1 << 31) + (1 << 17)
BIG_FIRST = (1 << 31) + 11
ALIAS = (1 << 17) + 4096  # [0, ALIAS): where a begin truncated to 32 bits would land


def big_case(u):
    """(offsets, keys of [offsets[0], offsets[nseg]), their oracle, canary)."""
    t = misort.tile_log2(np.dtype(u).itemsize)
    lens = [0, 5, 33, 1000, 1 << t, (1 << t) + 1, 64, 1]
    offs = L.offsets_of(lens, BIG_FIRST)
    assert int(offs[-1]) + 64 <= BIG_N and int(offs[-1]) - (1 << 31) < ALIAS - 4096
    local = offs - BIG_FIRST
    body = L.make("sentinels", 91, local, int(local[-1]), u)
    return offs, body, L.want(body, local, u), canary_for(body)


def big_alloc(u, arrays, extra=0):
    """`arrays` uninitialised tensors of BIG_N keys, or a skip that names the
    free and the needed bytes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    need = arrays * BIG_N * np.dtype(u).itemsize + extra + (4 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{free} bytes of device memory are free, {need} are needed")
    dt = torch.int32 if u == np.uint32 else torch.int64
    return [torch.empty(BIG_N, dtype=dt, device="cuda") for _ in range(arrays)]


def big_windows(offs):
    return ((BIG_FIRST - 4096, BIG_FIRST), (int(offs[-1]), BIG_N), (0, ALIAS))


def big_fill(d, offs, body, canary):
    for a, b in big_windows(offs):
        d[a:b].copy_(to_dev(np.full(b - a, canary, dtype=body.dtype)))
    d[BIG_FIRST:int(offs[-1])].copy_(to_dev(body))


def big_windows_intact(d, offs, canary):
    for a, b in big_windows(offs):
        got = bits(d[a:b])
        assert (got == canary).all(), f"keys [{a}, {b}) changed: {int((got != canary).sum())} differ"


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_segments_above_2_31_in_place(ctx, u):
    """Every segment starts above key index 2^31 (byte offset 2^33 or 2^34).
    The host writes and reads three canary windows and the segments only."""
    offs, body, w, canary = big_case(u)
    (d,) = big_alloc(u, 1)
    try:
        big_fill(d, offs, body, canary)
        o = torch.from_numpy(offs).cuda()
        assert ctx.sort_segments(d, o, out=d) is d
        np.testing.assert_array_equal(bits(d[BIG_FIRST:int(offs[-1])]), w)
        big_windows_intact(d, offs, canary)
        np.testing.assert_array_equal(o.cpu().numpy(), offs)
    finally:
        del d
        torch.cuda.empty_cache()


def test_segments_above_2_31_out_of_place_u32(ctx):
    """Out of place the leading fringe is a copy of 2^33 + 44 bytes.  The input
    holds a ramp (written on the device) and the output starts as canaries, so
    a fringe that was not copied, or copied short, shows in the comparison,
    which runs on the device."""
    u = np.uint32
    offs, body, w, canary = big_case(u)
    last = int(offs[-1])
    inp, out = big_alloc(u, 2, extra=BIG_N)  # torch.equal's mask of one byte per key
    try:
        torch.arange(BIG_N // 2, dtype=torch.int64, device="cuda", out=inp.view(torch.int64))
        big_fill(inp, offs, body, canary)
        out.fill_(int(canary.view(np.int32)))
        o = torch.from_numpy(offs).cuda()
        assert ctx.sort_segments(inp, o, out=out) is out
        np.testing.assert_array_equal(bits(out[BIG_FIRST:last]), w)
        assert torch.equal(out[:BIG_FIRST], inp[:BIG_FIRST])
        assert torch.equal(out[last:], inp[last:])
        np.testing.assert_array_equal(bits(inp[BIG_FIRST:last]), body)
        big_windows_intact(inp, offs, canary)
        assert int(inp[ALIAS]) == ALIAS // 2  # the ramp: 64-bit words 0, 1, 2, ..
        np.testing.assert_array_equal(o.cpu().numpy(), offs)
    finally:
        del inp, out
        torch.cuda.empty_cache()
