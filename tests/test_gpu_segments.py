"""Segmented sort on one GPU (misort_local_sort_segments, Context.sort_segments)
against numpy on the host: every segment [offsets[i], offsets[i + 1]) sorted on
its own, u32 and u64 directly, f64 through the order-preserving 64-bit pattern
(kmap of guard_bands.py).  Every comparison is on bit patterns; there is no
tolerance.

Two paths (misort.segment_class): segments up to the largest SORT tile go
through the row tile, one launch per class LR with R = 2^(LT - LR) segments per
LDS tile; longer ones class by class through padded blocks of 2^k keys.  The
shapes are the smallest that cross each boundary."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from guard_bands import TAIL, assert_guards, canary_for, guarded  # noqa: E402
from segment_layouts import FAMILIES, make, offsets_of, rand, want  # noqa: E402

pytestmark = pytest.mark.gpu

U64 = np.uint64
DTYPES = [np.uint32, np.uint64, np.float64]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def udt(dt):
    """The unsigned dtype of a key type's bit patterns."""
    return np.uint32 if dt == np.uint32 else np.uint64


def to_dev(a, dt=None):
    """Bit patterns on the device: u32 -> int32 storage, u64 -> int64 storage, or
    (dt float64) the same bits as float64."""
    a = np.ascontiguousarray(a)
    if dt == np.float64:
        return torch.from_numpy(a.view(np.float64)).cuda()
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def bits(t):
    torch.cuda.synchronize()
    if t.element_size() == 8:
        return t.view(torch.int64).cpu().numpy().view(np.uint64)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def check(ctx, k, offs, dt, what="", in_place=False):
    d, o = to_dev(k, dt), torch.from_numpy(offs).cuda()
    if in_place:
        out = ctx.sort_segments(d, o, out=d)
        assert out is d
    else:
        out = ctx.sort_segments(d, o)
        assert out.shape == d.shape and out.dtype == d.dtype and out.data_ptr() != d.data_ptr()
    np.testing.assert_array_equal(bits(out), want(k, offs, dt), err_msg=what)
    if not in_place:
        np.testing.assert_array_equal(bits(d), k, err_msg=what + " (input changed)")
    np.testing.assert_array_equal(o.cpu().numpy(), offs, err_msg=what + " (offsets changed)")


# ---- lengths: every class, interleaved --------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_every_length_in_one_call(ctx, dt):
    u = udt(dt)
    t = misort.tile_log2(np.dtype(u).itemsize)
    lens = list(range(71)) + [(1 << j) + d for j in range(7, t + 1) for d in (-1, 0, 1)]
    lens = np.random.default_rng(11).permutation(lens)
    offs = offsets_of(lens)
    k = make("random", 12, offs, int(offs[-1]), u)
    check(ctx, k, offs, dt, "out of place")
    check(ctx, k, offs, dt, "in place", in_place=True)


# ---- counts per class x key families ---------------------------------------------------

def class_cases():
    for u in (np.uint32, np.uint64):
        t = 15 if u == np.uint32 else 13
        lt = 14 if u == np.uint32 else 13  # the tile of the classes below tile_log2 (u32: 2^14)
        for lr in (5, 9, t):
            yield u, lr, 1 << ((t if lr == t else lt) - lr)


@pytest.mark.parametrize("u,lr,r", list(class_cases()), ids=lambda v: getattr(v, "__name__", str(v)))
def test_counts_of_one_class(ctx, u, lr, r):
    kb = np.dtype(u).itemsize
    lo = 0 if lr == 5 else 1 << (lr - 1)  # lengths of the class: (lo, 2^lr]
    rng = np.random.default_rng(100 * lr + kb)
    for count in sorted({1, r - 1, r, r + 1, 2 * r + r // 2 + 1} - {0}):
        lens = rng.integers(lo + 1, (1 << lr) + 1, size=count)
        lens[rng.integers(0, count)] = 1 << lr  # a full block
        lens[rng.integers(0, count)] = lo + 1  # the shortest of the class
        assert all(misort.segment_class(int(x), kb) == lr for x in lens)
        offs = offsets_of(lens)
        for fam in FAMILIES:
            k = make(fam, 7 * count + lr, offs, int(offs[-1]), u)
            check(ctx, k, offs, u, f"{fam}, {count} segments of class {lr}")


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_families_f64_mixed_classes(ctx, fam):
    lens = [0, 1, 33, 5, 700, 64, 0, 8192, 31, 129, 2, 4097]
    offs = offsets_of(lens)
    k = make(fam, 41, offs, int(offs[-1]), np.uint64)
    check(ctx, k, offs, np.float64, fam)


# ---- long segments -----------------------------------------------------------------------

@pytest.mark.parametrize("in_place", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_long_segments_two_classes(ctx, u, in_place):
    kb = np.dtype(u).itemsize
    a, b = (1 << misort.tile_log2(kb)) + 1, (1 << 16) + 1
    assert misort.segment_class(a, kb) != misort.segment_class(b, kb) == 17
    lens = [0, 5, b, 0, a, 100, b, 33, b, 0, 1]
    offs = offsets_of(lens)
    for fam in ("random", "sentinels", "opposed"):
        k = make(fam, 51, offs, int(offs[-1]), u)
        check(ctx, k, offs, u, fam, in_place=in_place)


# ---- f64 specials ----------------------------------------------------------------------------

SPECIALS = np.array([
    0x0000000000000000, 0x8000000000000000,  # +0.0, -0.0
    0x7FF0000000000000, 0xFFF0000000000000,  # +inf, -inf
    0x7FF8000000000001, 0xFFF8000000000001, 0x7FF0000000000123, 0xFFF00000000ABCDE,  # NaNs with payloads
    0x7FFFFFFFFFFFFFFF,  # maps TO the padding value (all-ones)
    0xFFFFFFFFFFFFFFFF,  # the padding value itself as a key: maps to 0, the smallest
    0x3FF0000000000000, 0xBFF0000000000000, 0x0000000000000001, 0x8000000000000001,
], dtype=np.uint64)


@pytest.mark.parametrize("in_place", [False, True], ids=["oop", "inplace"])
def test_f64_specials_on_both_paths(ctx, in_place):
    lens = [len(SPECIALS), 3, 50, 1000, 8192, (1 << 13) + 5, 0, 40]
    offs = offsets_of(lens)
    rng = np.random.default_rng(61)
    k = rand(rng, int(offs[-1]), np.uint64)
    pick = rng.random(k.size) < 0.6
    k[pick] = rng.choice(SPECIALS, int(pick.sum()))
    k[:len(SPECIALS)] = SPECIALS[::-1]
    check(ctx, k, offs, np.float64, "specials", in_place=in_place)
    # the doubles come back in IEEE order where it is defined
    out = want(k, offs, np.float64).view(np.float64)
    seg = out[:len(SPECIALS)]
    assert np.isnan(seg[0]) and np.signbit(seg[0]) and np.isnan(seg[-1]) and not np.signbit(seg[-1])


# ---- fringes, bounds, views ---------------------------------------------------------------------

def banded(k, lead, canary, dt):
    """(device base, device view) of k between guard bands."""
    base, _ = guarded(k.size, k.dtype, lead, canary, k)
    dbase = to_dev(base, dt)
    return dbase, dbase[lead:lead + k.size]


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_fringes_copied_out_of_place_untouched_in_place(ctx, u):
    kb = np.dtype(u).itemsize
    lens = [40, 0, 700, 1, (1 << misort.tile_log2(kb)) + 9, 64]
    offs = offsets_of(lens, first=7)
    n = int(offs[-1]) + 9
    k = make("sentinels", 71, offs, n, u)
    canary = canary_for(k)
    o = torch.from_numpy(offs).cuda()
    for lead in (4, 1):
        dbase_in, d = banded(k, lead, canary, u)
        dbase_out, out = banded(np.full(n, canary, dtype=u), lead, canary, u)
        assert ctx.sort_segments(d, o, out=out) is out
        w = want(k, offs, u)
        np.testing.assert_array_equal(bits(out), w)  # the fringes are k's
        assert_guards(bits(dbase_out), n, lead, canary)
        np.testing.assert_array_equal(bits(d), k)
        assert_guards(bits(dbase_in), n, lead, canary)
        ctx.sort_segments(d, o, out=d)
        np.testing.assert_array_equal(bits(d), w)
        assert_guards(bits(dbase_in), n, lead, canary)


@pytest.mark.parametrize("which", ["in", "out", "both"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_views_one_element_into_storage(ctx, dt, which):
    u = udt(dt)
    kb = np.dtype(u).itemsize
    lens = [33, 1000, 3, (1 << misort.tile_log2(kb)) + 3, 0, 257]
    offs = offsets_of(lens)
    n = int(offs[-1])
    k = make("random", 81, offs, n, u)
    canary = canary_for(k)
    dbase_in, d = banded(k, 1 if which in ("in", "both") else 4, canary, dt)
    lead_out = 1 if which in ("out", "both") else 4
    dbase_out, out = banded(np.full(n, canary, dtype=u), lead_out, canary, dt)
    ctx.sort_segments(d, torch.from_numpy(offs).cuda(), out=out)
    np.testing.assert_array_equal(bits(out), want(k, offs, dt))
    assert_guards(bits(dbase_out), n, lead_out, canary)
    np.testing.assert_array_equal(bits(d), k)


def test_nothing_to_sort(ctx):
    k = make("random", 91, offsets_of([0]), 100, np.uint32)
    d = to_dev(k)
    for offs in ([0], [5], [3, 3, 3, 3], [0, 0], [100, 100]):
        o = torch.tensor(offs, dtype=torch.int64, device="cuda")
        np.testing.assert_array_equal(bits(ctx.sort_segments(d, o)), k, err_msg=str(offs))
        ctx.sort_segments(d, o, out=d)
        np.testing.assert_array_equal(bits(d), k, err_msg=str(offs))
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    for offs in ([0], [0, 0, 0]):
        assert ctx.sort_segments(e, torch.tensor(offs, dtype=torch.int64, device="cuda")).numel() == 0


# ---- refusals ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["decreasing", "negative_first", "last_past_n"])
def test_malformed_offsets_are_refused_before_any_key_kernel(ctx, case):
    lens = [40, 10, 700, 1, 40000, 64, 9]
    offs = offsets_of(lens)
    n = int(offs[-1])
    k = make("random", 101, offs, n, np.uint32)
    if case == "decreasing":
        offs[3], offs[4], bad = offs[4], offs[3], 3
    elif case == "negative_first":
        offs[0], bad = -2, 0
    else:
        offs[-1], bad = n + 3, len(lens) - 1
    assert 3 < TAIL
    canary = canary_for(k)
    prefill = np.full(n, canary + 1, dtype=np.uint32)
    dbase, out = banded(prefill, 4, canary, np.uint32)
    d = to_dev(k)
    with pytest.raises(misort.MisortError) as ei:
        ctx.sort_segments(d, torch.from_numpy(offs).cuda(), out=out)
    assert ei.value.code == -1 and f"index {bad} " in str(ei.value)
    np.testing.assert_array_equal(bits(out), prefill)
    assert_guards(bits(dbase), n, 4, canary)
    np.testing.assert_array_equal(bits(d), k)


def test_refused_overlaps(ctx):
    n = 4096
    base = torch.zeros(n + 8, dtype=torch.int64, device="cuda")
    o = torch.tensor([0, 100, n], dtype=torch.int64, device="cuda")
    with pytest.raises(misort.MisortError) as ei:
        ctx.sort_segments(base[:n], o, out=base[4:n + 4])
    assert ei.value.code == -1 and "overlaps d_in" in str(ei.value)
    other = torch.zeros(n, dtype=torch.int64, device="cuda")
    with pytest.raises(misort.MisortError) as ei:
        ctx.sort_segments(other, base[n - 2:n + 1], out=base[:n])  # the offsets' first word lies in out
    assert ei.value.code == -1 and "d_offsets" in str(ei.value)
    torch.cuda.synchronize()
    assert int(base.abs().sum()) == 0


def test_entry_point_refusals(ctx):
    f = misort.lib().misort_local_sort_segments
    a = torch.zeros(64, dtype=torch.int64, device="cuda")
    b = torch.zeros(64, dtype=torch.int64, device="cuda")
    o = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    p, q, s = a.data_ptr(), b.data_ptr(), ctx.native_stream
    for dt in (misort.F32, 4, -1):
        assert f(ctx._h, dt, p, q, 4, o.data_ptr(), 1, s) == -1
    assert f(ctx._h, misort.U64, p, q, -1, o.data_ptr(), 1, s) == -1
    assert f(ctx._h, misort.U64, p, q, 4, o.data_ptr(), -1, s) == -1
    assert f(ctx._h, misort.U64, p, q, 4, o.data_ptr(), 1 << 31, s) == -1
    assert f(ctx._h, misort.U64, p, q, 4, o.data_ptr() + 4, 1, s) == -1  # offsets need 8-byte alignment
    assert f(ctx._h, misort.U64, p, q, 4, None, 1, s) == -1
    assert f(ctx._h, misort.U64, None, None, 0, None, 3, s) == 0  # n == 0: no pointer is looked at
    assert f(ctx._h, misort.U64, p, p, 4, None, 0, s) == 0  # nseg == 0 in place: nothing


# ---- agreement with the existing calls -----------------------------------------------------------------

@pytest.mark.parametrize("dt,n", [(np.uint32, 100003), (np.uint64, 5000), (np.float64, 20011)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_one_segment_equals_local_sort(ctx, dt, n):
    u = udt(dt)
    k = rand(np.random.default_rng(n), n, u)
    d = to_dev(k, dt)
    got = ctx.sort_segments(d, torch.tensor([0, n], dtype=torch.int64, device="cuda"))
    ref = ctx.local_sort(d, out=torch.empty_like(d))
    np.testing.assert_array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_uniform_offsets_equal_sort_rows(ctx, dt):
    u = udt(dt)
    t = 1 << misort.tile_log2(np.dtype(u).itemsize)
    for rows, cols in ((37, 1000), (5, t + 3)):
        k = rand(np.random.default_rng(cols), rows * cols, u)
        d = to_dev(k, dt)
        o = torch.arange(0, rows * cols + 1, cols, dtype=torch.int64, device="cuda")
        got = ctx.sort_segments(d, o)
        ref = ctx.sort_rows(d.view(rows, cols))
        np.testing.assert_array_equal(bits(got), bits(ref).reshape(-1), err_msg=str(cols))


# ---- stream, profiler, repeatability ----------------------------------------------------------------------

def test_streams_and_repeatability(ctx):
    lens = [40, 0, 700, 1, 40000, 64, 9, 8193]
    offs = offsets_of(lens)
    k = make("dups", 111, offs, int(offs[-1]), np.uint32)
    d, o = to_dev(k), torch.from_numpy(offs).cuda()
    w = want(k, offs, np.uint32)
    first = ctx.sort_segments(d, o)
    np.testing.assert_array_equal(bits(first), w)
    np.testing.assert_array_equal(bits(ctx.sort_segments(d, o)), bits(first))
    torch.cuda.synchronize()
    out = torch.empty_like(d)
    ctx.sort_segments(d, o, out=out, stream=ctx.native_stream)
    ctx.synchronize()
    np.testing.assert_array_equal(bits(out), w)
    st = torch.cuda.Stream()
    out2 = torch.empty_like(d)
    with torch.cuda.stream(st):
        ctx.sort_segments(d, o, out=out2, stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(bits(out2), w)


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
def test_profile_tile_classes(ctx, u):
    size = np.dtype(u).itemsize
    lens = [40, 0, 700, 1, 3000, 64, 9, 650, 8192, 33]  # tile classes only
    classes = {misort.segment_class(x, size) for x in lens if x}
    offs = offsets_of(lens)
    d, o = to_dev(make("random", 121, offs, int(offs[-1]), u)), torch.from_numpy(offs).cuda()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        ctx.sort_segments(d, o)
        torch.cuda.synchronize()
        rec = ctx.profile_read()
        trace = ctx.profile_trace()
    finally:
        ctx.profile(False)
    launches, ms, nbytes = rec["tile_sort"]
    assert launches == len(classes) and ms > 0.0 and nbytes == 2 * sum(lens) * size
    assert sum(b for kind, _, b in trace if kind == "tile_sort") == nbytes
    assert rec["other"][0] == 2  # count and scatter
    assert all(rec[kind][0] == 0 for kind in rec if kind not in ("tile_sort", "other"))


# ---- Python argument checks ----------------------------------------------------------------------------------

def test_python_argument_checks(ctx):
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    o = torch.tensor([0, 10, 64], dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        ctx.sort_segments(d, o.to(torch.int32))
    with pytest.raises(TypeError):
        ctx.sort_segments(d.to(torch.float32), o)
    with pytest.raises(ValueError):
        ctx.sort_segments(d, o.cpu())
    with pytest.raises(ValueError):
        ctx.sort_segments(d, o.view(1, 3))
    with pytest.raises(ValueError):
        ctx.sort_segments(d, o[:0])
    with pytest.raises(ValueError):
        ctx.sort_segments(d, torch.zeros(6, dtype=torch.int64, device="cuda")[::2])
    with pytest.raises(ValueError):
        ctx.sort_segments(torch.zeros(128, dtype=torch.int32, device="cuda")[::2], o)
    with pytest.raises(ValueError):
        ctx.sort_segments(d.view(8, 8), o)
    with pytest.raises(TypeError):
        ctx.sort_segments(d, o, out=torch.zeros(64, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ctx.sort_segments(d, o, out=torch.zeros(63, dtype=torch.int32, device="cuda"))
