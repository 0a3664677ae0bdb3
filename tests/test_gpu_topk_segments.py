"""Segmented top-k on one GPU (misort_local_topk_segments, Context.topk_segments)
against tests/topk_segments_oracle.py: per segment the first min(k, len) of the
stable argsort of T(key), T = K for the smallest keys and ~K for the largest, K
the identity (u32) or the order-preserving pattern of a float32, then the fill
(index 0xFFFFFFFF, the unmapped all-ones key).  Every comparison is on bit
patterns; there is no tolerance.  The layouts and key families are those of
tests/topk_segments_cases.py: the smallest shapes at which each mechanism of
misort.topk_segments_plan can break -- every short length and both ends of
every tile class in one call, k below, at and above a block and a length, a
class with one segment fewer and more than a tile's rows, a piece with one real
record, a piece that leaves early, and the first length with a pass from
candidates to candidates."""
import ctypes
import functools

import numpy as np
import pytest

import guard_bands as GB
import segment_layouts as L
import stream_order as SO
import topk_segments_cases as C
import topk_segments_oracle as TSO
from stream_order import In, Out

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
ONES = U32(0xFFFFFFFF)
PREFILL = U32(0x5A5A5A5A)
DIRECTIONS = pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
KEYS = pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side(ctx):
    """A stream that is neither torch's default nor the context's own."""
    SO.calibrate()
    return torch.cuda.Stream()


def dev(a, f32=False, lead=0):
    """u32 bit patterns -> int32 storage, or float32 with the same bits; ``lead``
    elements of storage before the view."""
    a = np.ascontiguousarray(a, dtype=U32)
    flat = np.concatenate([np.zeros(lead, U32), a.reshape(-1)])
    t = torch.from_numpy(flat.view(F32 if f32 else np.int32)).cuda()
    return t[lead:].view(a.shape)


def dev_offs(offs):
    return torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()


def bits(t):
    torch.cuda.synchronize()
    return t.contiguous().view(torch.int32).cpu().numpy().view(U32)


def call_and_compare(ctx, keys, offs, k, largest, f32, what, want=None):
    """One call with new outputs against the oracle; the keys and the offsets
    are unchanged.  Returns (values, indices) as host bit patterns."""
    what = f"{what} k={k} {'largest' if largest else 'smallest'} {'f32' if f32 else 'u32'}"
    nseg = len(offs) - 1
    dk, do = dev(keys, f32), dev_offs(offs)
    vals, idx = ctx.topk_segments(dk, do, k, largest=largest)
    assert vals.shape == idx.shape == (nseg, k) and vals.dtype == dk.dtype and idx.dtype == torch.int32
    wv, wi = want if want is not None else TSO.topk_segments(keys, offs, k, largest, f32)
    gv, gi = bits(vals), bits(idx)
    np.testing.assert_array_equal(gi, wi, err_msg=what + " (indices)")
    np.testing.assert_array_equal(gv, wv, err_msg=what + " (values)")
    np.testing.assert_array_equal(bits(dk), keys, err_msg=what + " (keys changed)")
    np.testing.assert_array_equal(do.cpu().numpy(), offs, err_msg=what + " (offsets changed)")
    return gv, gi


def check_case(ctx, family, layout, k, largest, f32=None):
    f32 = family in C.F32_FAMILIES if f32 is None else f32
    keys, offs = C.keys_of(family, layout, largest), C.offsets(layout)
    gv, gi = call_and_compare(ctx, keys, offs, k, largest, f32, f"{family} on {layout}",
                              C.want(family, layout, k, largest, f32))
    # the fill sits exactly at the slots past the length; the real indices gather the real values
    lens = np.diff(offs)
    short = np.arange(k)[None, :] >= lens[:, None]
    assert np.array_equal(gi == TSO.FILL_INDEX, short)
    assert np.all(gv[short] == TSO.fill_key(largest, f32))
    at = (offs[:-1, None] + gi.astype(np.int64))[~short]
    np.testing.assert_array_equal(keys[at], gv[~short])


# ---- every short length in one call ---------------------------------------------------------------------

@KEYS
@DIRECTIONS
@pytest.mark.parametrize("k", C.KS["short"])
def test_every_short_length_in_one_call(ctx, k, largest, f32):
    """Lengths 0..70 and both ends of every tile class, k below, at and above a
    lane's 32 records and the lengths; empty segments first, last and adjacent."""
    check_case(ctx, "tied", "short", k, largest, f32)


# ---- counts of one class around the tile's rows --------------------------------------------------------

@DIRECTIONS
@pytest.mark.parametrize("lr", [5, 12])
def test_tile_row_counts(ctx, lr, largest):
    r = 1 << (13 - lr)
    rng = np.random.default_rng(100 * lr)
    for count in (r - 1, r, r + 1):
        lens = rng.integers(L.class_lo(lr) + 1, (1 << lr) + 1, size=count)
        lens[rng.integers(0, count)] = 1 << lr  # a full block
        assert all(misort.segment_class(int(x), 8) == lr for x in lens)
        offs = L.offsets_of(lens)
        keys = C.fam_tied(rng, offs, largest)
        for k in (1, 33):
            call_and_compare(ctx, keys, offs, k, largest, False, f"{count} segments of class {lr}")


# ---- long classes -----------------------------------------------------------------------------------------

@KEYS
@DIRECTIONS
@pytest.mark.parametrize("k", C.KS["long"])
def test_long_classes(ctx, k, largest, f32):
    """8193 (a piece with one real record), 16384, 16385 (class 15: a piece that
    leaves early), 40001, 65536 and 65537 (k = 1024: 2^14 candidates, a pass from
    records to records), with short segments and empty ones between them."""
    assert len(misort.topk_segments_plan(65537, k)) == (3 if k == 1024 else 2)
    check_case(ctx, "tied", "long", k, largest, f32)


def test_scratch_growth_then_reuse():
    """Four long classes and short ones on a fresh context: both candidate
    buffers grow in this call; a second call on other keys reuses them."""
    c = misort.Context(0)
    try:
        check_case(c, "tied", "long", 1024, True)
        check_case(c, "winners_last", "long", 1024, False)
        check_case(c, "tied", "short", 64, True)
    finally:
        c.close()


# ---- key families ------------------------------------------------------------------------------------------

@DIRECTIONS
@pytest.mark.parametrize("layout", sorted(C.LAYOUTS))
@pytest.mark.parametrize("family", [f for f in sorted(C.FAMILIES) if f != "tied"])
def test_key_families(ctx, family, layout, largest):
    for k in C.KS[layout]:
        check_case(ctx, family, layout, k, largest)
    if family in ("equal", "half_sentinel", "half_sentinel_f32"):  # all keys of a segment equal: positions 0, 1, ...
        k = C.KS[layout][-1]
        _, wi = C.want(family, layout, k, largest, family in C.F32_FAMILIES)
        lens = np.diff(C.offsets(layout))
        real = np.arange(k)[None, :] < lens[:, None]
        np.testing.assert_array_equal(wi[real], np.broadcast_to(np.arange(k, dtype=U32), wi.shape)[real])


def test_f32_order_is_the_total_order(ctx):
    """Largest: positive NaN, +inf, +0.0, -0.0, -inf, negative NaN; smallest the reverse; bit-exact."""
    pat = np.array([0x80000000, 0x7F800000, 0xFFC00000, 0x00000000, 0x7FC00000, 0xFF800000], dtype=U32)
    offs = L.offsets_of([6, 6])
    dk, do = dev(np.concatenate([pat, pat[::-1]]), True), dev_offs(offs)
    order = [4, 1, 3, 0, 5, 2]
    v, i = ctx.topk_segments(dk, do, 6, largest=True)
    np.testing.assert_array_equal(bits(i), [order, [5 - x for x in order]])
    np.testing.assert_array_equal(bits(v), [pat[order], pat[order]])
    v, i = ctx.topk_segments(dk, do, 6, largest=False)
    np.testing.assert_array_equal(bits(i), [order[::-1], [5 - x for x in order[::-1]]])


# ---- layout edges ------------------------------------------------------------------------------------------

@DIRECTIONS
def test_keys_outside_the_segments_are_ignored(ctx, largest):
    """offsets[0] > 0 and offsets[nseg] < n; the keys outside are the direction's best key."""
    lens = [40, 0, 700, 1, 8193, 64, 16385, 33]
    offs = L.offsets_of(lens, first=7)
    n = int(offs[-1]) + 9
    rng = np.random.default_rng(61)
    keys = rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype(U32) & U32(0x7FFFFFFE) | U32(2)
    keys[:7] = keys[int(offs[-1]):] = ONES if largest else 0  # poison: it would win everywhere
    for k in (1, 64, 1024):
        gv, _ = call_and_compare(ctx, keys, offs, k, largest, False, "fringes")
        assert not np.any(gv[:, 0][np.asarray(lens) > 0] == (ONES if largest else 0))


@KEYS
@DIRECTIONS
def test_all_segments_empty_and_no_keys(ctx, largest, f32):
    keys = np.arange(100, dtype=U32)
    for offs in ([0, 0], [5, 5, 5, 5], [100, 100], [0] * 3000):
        call_and_compare(ctx, keys, np.asarray(offs, dtype=np.int64), 3, largest, f32, f"empty {offs[:4]}")
    # n == 0 with nseg > 0: a normal call, every row is filled; the key pointer is not looked at
    e = dev(np.zeros(0, U32), f32)
    do = dev_offs(np.zeros(6, np.int64))
    v, i = ctx.topk_segments(e, do, 4, largest=largest)
    assert np.all(bits(i) == ONES) and np.all(bits(v) == TSO.fill_key(largest, f32)) and i.shape == (5, 4)
    out = dev(np.full((5, 4), PREFILL))
    f = misort.lib().misort_local_topk_segments
    torch.cuda.synchronize()
    assert f(ctx._h, misort.F32 if f32 else misort.U32, None, None, out.data_ptr(), 0, do.data_ptr(), 5, 4,
             int(largest), ctx.native_stream) == 0
    ctx.synchronize()
    assert np.all(bits(out) == ONES)


def test_nothing_to_do_looks_at_no_pointer(ctx):
    f = misort.lib().misort_local_topk_segments
    assert f(ctx._h, misort.U32, None, None, None, 100, None, 0, 5, 1, None) == 0   # nseg == 0
    assert f(ctx._h, misort.F32, None, None, None, 100, None, 7, 0, 0, None) == 0   # k == 0
    keys, do = dev(np.arange(15, dtype=U32)), dev_offs([0, 5, 15])
    v, i = ctx.topk_segments(keys, do, 0)
    assert v.shape == i.shape == (2, 0)
    v, i = ctx.topk_segments(keys, do[:1], 3)
    assert v.shape == i.shape == (0, 3)


@functools.lru_cache(maxsize=2)
def many_case(name):
    offs, n = L.layout(name, 8)
    assert offs.size - 1 > 2048
    return SO.tied_u32(1000 + len(name), n), offs


@pytest.mark.parametrize("name,k", [("mixed", 33), ("boundary2049", 64), ("sparse", 1024)])
def test_many_segments(ctx, name, k):
    """More segments than one workgroup of the offset sweeps and of the fill takes."""
    keys, offs = many_case(name)
    if name == "mixed":
        assert max(L.class_spans(np.diff(offs), 8)) > 13
    call_and_compare(ctx, keys, offs, k, name != "mixed", False, name)


# ---- buffers -----------------------------------------------------------------------------------------------

@DIRECTIONS
@pytest.mark.parametrize("layout,k", [("short", 33), ("short", 1024), ("long", 64), ("long", 1024)])
@pytest.mark.parametrize("with_values", [True, False], ids=["values", "indices_only"])
def test_views_and_guard_bands(ctx, layout, k, with_values, largest):
    """Keys and outputs start one element into their storage; the outputs lie
    between canary bands: exactly nseg * k elements of each are written."""
    keys, offs = C.keys_of("tied", layout, largest), C.offsets(layout)
    wv, wi = C.want("tied", layout, k, largest, False)
    nseg = len(offs) - 1
    n = nseg * k
    canary = GB.canary_for(wv.reshape(-1), wi.reshape(-1))
    dk, do = dev(keys, lead=1), dev_offs(offs)
    assert dk.data_ptr() % 16 == 4
    bases = {}
    for name in ("vals", "idx"):
        base, _ = GB.guarded(n, U32, 1, canary)
        bases[name] = torch.from_numpy(base.view(np.int32)).cuda()
    ov, oi = (bases[x][1:1 + n].view(nseg, k) for x in ("vals", "idx"))
    if with_values:
        gv, gi = ctx.topk_segments(dk, do, k, largest=largest, out_values=ov, out_indices=oi)
        assert gv is ov and gi is oi
    else:
        assert ctx.topk_segments_indices(dk, do, k, largest=largest, out=oi) is oi
    np.testing.assert_array_equal(bits(oi), wi)
    np.testing.assert_array_equal(bits(ov), wv if with_values else np.full((nseg, k), canary))
    for name in ("vals", "idx"):
        GB.assert_guards(bits(bases[name]), n, 1, canary)
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(do.cpu().numpy(), offs)


# ---- refusals, outputs unchanged ---------------------------------------------------------------------------

def raw(ctx, dt, keys, vals, idx, n, offs, nseg, k, largest=1):
    p = [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (keys, vals, idx, offs)]
    return misort.lib().misort_local_topk_segments(ctx._h, dt, p[0], p[1], p[2], n, p[3], nseg, k, largest, None)


def test_refusals_leave_the_outputs_unchanged(ctx):
    lens = [40, 10, 700, 1, 64, 9]
    nseg, k = len(lens), 8
    offs = L.offsets_of(lens)
    n = int(offs[-1])
    keys = SO.tied_u32(71, n)
    # one int64 storage: the keys, the offsets, a gap (the misaligned offsets below end in it), free space for outputs
    words = (n + 1) // 2 + (nseg + 1) + 2 + 4 * nseg * k
    base = torch.zeros(words, dtype=torch.int64, device="cuda")
    b32 = base.view(torch.int32)
    dk = b32[:n]
    dk.copy_(dev(keys))
    o_at = (n + 1) // 2
    do = base[o_at:o_at + nseg + 1]
    do.copy_(dev_offs(offs))
    free = b32[2 * (o_at + nseg + 1) + 4:]
    free.fill_(int(PREFILL))
    ov, oi = free[:nseg * k].view(nseg, k), free[nseg * k:2 * nseg * k].view(nseg, k)
    before = bits(b32).copy()

    def refused(call, needle=None):
        with pytest.raises(misort.MisortError) as e:
            call()
        assert e.value.code == -1
        if needle:
            assert needle in str(e.value)
        np.testing.assert_array_equal(bits(b32), before)

    offs32 = do.view(torch.int32)
    # an output over the key input (its start, its last element), over the offsets, over the other output
    refused(lambda: ctx.topk_segments(dk, do, k, out_values=dk[:nseg * k], out_indices=oi), "overlaps d_keys_in")
    refused(lambda: ctx.topk_segments(dk, do, k, out_values=ov, out_indices=dk[:nseg * k]), "overlaps d_keys_in")
    refused(lambda: ctx.topk_segments_indices(dk, do, k, out=b32[n - 1:n - 1 + nseg * k]), "overlaps")
    refused(lambda: ctx.topk_segments(dk[:40], do[:2], 7, out_values=ov, out_indices=offs32[:7]), "d_offsets")
    refused(lambda: ctx.topk_segments(dk[:40], do[:2], 7, out_values=offs32[3:10], out_indices=oi), "d_offsets")
    refused(lambda: ctx.topk_segments(dk, do, k, out_values=ov, out_indices=ov), "d_keys_out overlaps d_idx_out")
    refused(lambda: ctx.topk_segments(dk, do, k, out_values=ov, out_indices=free[nseg * k - 1:2 * nseg * k - 1]),
            "overlaps")
    # k above the tile, whatever the segments; key types of the 64-bit sorts; null arrays; negative sizes
    big = dev(np.full(2 * nseg * 8193, PREFILL))
    refused(lambda: ctx.topk_segments(dk, do, 8193, out_values=big[:nseg * 8193], out_indices=big[nseg * 8193:]),
            "k = 8193")
    assert np.all(bits(big) == PREFILL)
    for dt in (misort.U64, misort.F64, 7):
        assert raw(ctx, dt, dk, ov, oi, n, do, nseg, k) == -1
    assert b"MISORT_U32 or MISORT_F32" in misort.lib().misort_last_error()
    assert raw(ctx, misort.U32, None, ov, oi, n, do, nseg, k) == -1
    assert raw(ctx, misort.U32, dk, ov, None, n, do, nseg, k) == -1
    assert raw(ctx, misort.U32, dk, ov, oi, n, None, nseg, k) == -1
    for sizes in ((-1, nseg, k), (n, -1, k), (n, nseg, -1), (n, 1 << 31, k)):
        assert raw(ctx, misort.U32, dk, ov, oi, sizes[0], do, sizes[1], sizes[2]) == -1
    f = misort.lib().misort_local_topk_segments
    assert f(ctx._h, misort.U32, dk.data_ptr(), ov.data_ptr(), oi.data_ptr(), n, do.data_ptr() + 4, nseg, k, 1,
             None) == -1
    assert b"8-byte aligned" in misort.lib().misort_last_error()
    assert f(ctx._h, misort.U32, dk.data_ptr() + 2, ov.data_ptr(), oi.data_ptr(), n - 1, do.data_ptr(), nseg, k, 1,
             None) == -1
    np.testing.assert_array_equal(bits(b32), before)
    # the mirror's own checks
    with pytest.raises(TypeError):
        ctx.topk_segments(dk.view(torch.int64), do, 2)
    with pytest.raises(TypeError):
        ctx.topk_segments(dk, do.to(torch.int32), 2)
    with pytest.raises(TypeError):
        ctx.topk_segments(dk, do, k, out_values=ov.view(torch.float32))
    with pytest.raises(TypeError):
        ctx.topk_segments(dk, do, k, out_indices=oi.to(torch.int64))
    with pytest.raises(ValueError):
        ctx.topk_segments(dk, do.cpu(), 2)
    with pytest.raises(ValueError):
        ctx.topk_segments(dk.cpu(), do, 2)
    with pytest.raises(ValueError):
        ctx.topk_segments(dk, do, k, out_values=ov.cpu())
    with pytest.raises(ValueError):
        ctx.topk_segments(dk[:n - n % 2].view(2, -1), do, 2)
    with pytest.raises(ValueError):
        ctx.topk_segments(dk, do[:0], 2)
    with pytest.raises(ValueError):
        ctx.topk_segments(dk, do, k, out_values=ov, out_indices=oi.view(-1)[:nseg * k - 1])
    with pytest.raises(ValueError):
        ctx.topk_segments(dk, do, -1)
    np.testing.assert_array_equal(bits(b32), before)


@pytest.mark.parametrize("bad", [3, 2500], ids=["first_workgroup", "later_workgroup"])
@pytest.mark.parametrize("case", ["decreasing", "negative_first", "last_past_n"])
def test_malformed_offsets_are_refused_before_anything_is_written(ctx, case, bad):
    lens = np.random.default_rng(bad).integers(0, 40, size=3000)
    lens[7] = 8193  # a long class too: nothing of it may run
    nseg, k = lens.size, 5
    offs = L.offsets_of(lens, first=2)
    n = int(offs[-1]) + 3
    keys = SO.tied_u32(101, n)
    if case == "decreasing":
        offs[bad + 1] = offs[bad] - 1  # segment `bad` ends before it begins; the next one only grows
    elif case == "negative_first":
        offs[0], bad = -2, 0
    else:
        offs[-1], bad = n + 3, nseg - 1
    dk, do = dev(keys), dev_offs(offs)
    ov, oi = dev(np.full((nseg, k), PREFILL)), dev(np.full((nseg, k), PREFILL))
    with pytest.raises(misort.MisortError) as ei:
        ctx.topk_segments(dk, do, k, out_values=ov, out_indices=oi)
    msg = str(ei.value)
    assert ei.value.code == -1 and f"index {bad} " in msg and "malformed offsets" in msg
    assert "nothing was written" in msg
    assert np.all(bits(ov) == PREFILL) and np.all(bits(oi) == PREFILL)
    np.testing.assert_array_equal(bits(dk), keys)


def test_long_segments_refuse_a_large_k(ctx):
    """k = 1025 with one segment of 8193 keys: known after the count, nothing is written."""
    lens = [40, 8193, 0, 700]
    offs = L.offsets_of(lens)
    keys = SO.tied_u32(111, int(offs[-1]))
    dk, do = dev(keys), dev_offs(offs)
    ov, oi = dev(np.full((4, 1025), PREFILL)), dev(np.full((4, 1025), PREFILL))
    with pytest.raises(misort.MisortError) as e:
        ctx.topk_segments(dk, do, 1025, out_values=ov, out_indices=oi)
    assert e.value.code == -1 and "nothing was written" in str(e.value) and "k = 1025" in str(e.value)
    assert np.all(bits(ov) == PREFILL) and np.all(bits(oi) == PREFILL)
    np.testing.assert_array_equal(bits(dk), keys)
    # the same k without the long segment is served
    offs = L.offsets_of([40, 8192, 0, 700])
    call_and_compare(ctx, keys[:int(offs[-1])], offs, 1025, True, False, "k = 1025, tile classes only")


# ---- agreement with the existing entry points and with torch -----------------------------------------------

@KEYS
@DIRECTIONS
@pytest.mark.parametrize("rows,cols,k", [(64, 1000, 8), (3, 9000, 1024)])
def test_uniform_offsets_equal_topk_rows(ctx, rows, cols, k, largest, f32):
    keys = (SO.f32_keys(cols, rows * cols).view(U32) if f32 else SO.tied_u32(cols, rows * cols))
    dk = dev(keys, f32)
    do = torch.arange(0, rows * cols + 1, cols, dtype=torch.int64, device="cuda")
    sv, si = ctx.topk_segments(dk, do, k, largest=largest)
    rv, ri = ctx.topk_rows(dk.view(rows, cols), k, largest=largest)
    np.testing.assert_array_equal(bits(si), bits(ri))
    np.testing.assert_array_equal(bits(sv), bits(rv))


@KEYS
def test_smallest_equals_argsort_segments_sliced(ctx, f32):
    lens = C.LAYOUTS["long"]
    offs, k = L.offsets_of(lens), 64
    keys = C.keys_of("f32" if f32 else "tied", "long", False)
    dk, do = dev(keys, f32), dev_offs(offs)
    order = bits(ctx.argsort_segments(dk, do))
    idx = bits(ctx.topk_segments_indices(dk, do, k, largest=False))
    for i, ln in enumerate(lens):
        m = min(k, ln)
        np.testing.assert_array_equal(idx[i, :m], order[int(offs[i]):int(offs[i]) + m], err_msg=f"segment {i}")
        assert np.all(idx[i, m:] == ONES)


@DIRECTIONS
def test_against_torch_topk_on_distinct_floats(ctx, largest):
    """Finite float32 keys without ties: per segment the values and indices are torch.topk's."""
    lens, k = [1000, 5, 0, 20000, 64, 8193], 64
    offs = L.offsets_of(lens)
    n = int(offs[-1])
    g = torch.Generator(device="cpu").manual_seed(n)
    keys = ((torch.randperm(n, generator=g) - n // 2).to(torch.float32) * 0.37).cuda()  # distinct: n < 2^24
    vals, idx = ctx.topk_segments(keys, dev_offs(offs), k, largest=largest)
    torch.cuda.synchronize()
    for i, ln in enumerate(lens):
        m = min(k, ln)
        ref = torch.topk(keys[int(offs[i]):int(offs[i + 1])], m, largest=largest, sorted=True)
        assert torch.equal(vals[i, :m], ref.values), i
        assert torch.equal(idx[i, :m].long(), ref.indices), i
        assert bool((idx[i, m:] == -1).all()), i


# ---- launches ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,k", [("short", 33), ("long", 64), ("long", 1024)])
def test_tile_sort_launches_are_the_plans_passes(ctx, layout, k):
    keys, offs = C.keys_of("tied", layout, True), C.offsets(layout)
    dk, do = dev(keys), dev_offs(offs)
    ctx.topk_segments(dk, do, k)  # scratch growth out of the way
    torch.cuda.synchronize()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        vals, idx = ctx.topk_segments(dk, do, k)
        torch.cuda.synchronize()
        got = {name: v[0] for name, v in ctx.profile_read().items() if v[0]}
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    # one representative length per non-empty class: every length of a class has the class's passes
    by_class = {misort.segment_class(x, 8): x for x in C.LAYOUTS[layout] if x}
    passes = sum(len(misort.topk_segments_plan(x, k)) for x in by_class.values())
    assert got == {"tile_sort": passes, "other": 3}  # count, scatter, fill
    np.testing.assert_array_equal(bits(idx), C.want("tied", layout, k, True, False)[1])


# ---- stream order ------------------------------------------------------------------------------------------
# The call waits on its own stream by contract (the count header), so what is asserted is what is asserted
# for sort_segments: the results, computed from inputs that a producer pending on the stream writes.  Offsets
# still poisoned (all zero) would make every segment empty and every row a fill.

STREAM_LAYOUTS = {"short": ([40, 0, 700, 1, 64, 9, 8192, 0, 33], 8), "long": ([40, 0, 700, 20000, 64, 8193, 0, 33], 64)}


@functools.lru_cache(maxsize=None)
def stream_case(layout, largest, salt=0):
    lens, k = STREAM_LAYOUTS[layout]
    offs = L.offsets_of(lens, first=3)
    n = int(offs[-1]) + 5
    keys = SO.tied_u32(900 + salt + len(lens), n) | U32(1)  # never the poison
    wv, wi = TSO.topk_segments(keys, offs, k, largest)
    nseg = len(lens)
    stage = {"keys": In(keys, lead=1), "offs": In(offs), "vals": Out((nseg, k), U32, lead=1),
             "idx": Out((nseg, k), U32, lead=1)}
    return stage, {"keys": keys, "offs": offs, "vals": wv, "idx": wi}, k


def issue(c, t, k, largest, handle, suffix=""):
    c.topk_segments(t["keys" + suffix], t["offs" + suffix], k, largest=largest, out_values=t["vals" + suffix],
                    out_indices=t["idx" + suffix], stream=handle)


def run_stream(c, stream, layout, largest, mode, salt=0, pending=True):
    stage, expect, k = stream_case(layout, largest, salt)
    handle = None if mode == "current" else stream.cuda_stream
    res = SO.behind_pending_work(stream, stage, lambda t: issue(c, t, k, largest, handle),
                                 ms=SO.PRODUCER_MS if pending else 0.01,
                                 current="stream" if mode == "current" else "elsewhere")
    SO.compare(res, expect, f"topk_segments {layout} ({mode})")
    return res


@DIRECTIONS
@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("layout", sorted(STREAM_LAYOUTS))
def test_behind_pending_work_on_a_warm_context(ctx, side, layout, mode, largest):
    run_stream(ctx, side, layout, largest, mode, salt=SO.WARM_SALT, pending=False)  # other data: grows the scratch
    run_stream(ctx, side, layout, largest, mode)


@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("layout", sorted(STREAM_LAYOUTS))
def test_behind_pending_work_on_a_fresh_context(side, layout, mode):
    c = misort.Context(0)
    try:
        run_stream(c, side, layout, True, mode)
    finally:
        c.close()


def test_two_calls_chained_on_one_stream(ctx, side):
    """The second call reads other inputs and reuses the header, the lists and
    the candidates' scratch while the first's kernels may still be running: both exact."""
    specs = [("long", True, 77), ("long", False, 78)]
    cases = [stream_case(*s) for s in specs]
    stage = {f"{name}{i}": b for i, (st, _, _) in enumerate(cases) for name, b in st.items()}
    expect = {f"{name}{i}": w for i, (_, ex, _) in enumerate(cases) for name, w in ex.items()}

    def call(t):
        for i, ((_, largest, _), (_, _, k)) in enumerate(zip(specs, cases)):
            issue(ctx, t, k, largest, side.cuda_stream, suffix=str(i))
    SO.compare(SO.behind_pending_work(side, stage, call), expect, "chained")
