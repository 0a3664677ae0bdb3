"""Row-wise sort on one GPU (misort_local_sort_rows, Context.sort_rows) against
numpy on the host: np.sort(K(keys).reshape(rows, cols), axis=1) mapped back, K
the order-preserving pattern of a key (kmap of test_gpu_pairs64.py).  Every
comparison is on bit patterns; there is no tolerance.

Two paths (misort.rows_plan): "tile", cols up to the largest SORT tile, packs
R = 2^(tile_log2 - block_log2) rows into one LDS tile and stops the network at
the row length; "blocks" pads longer rows to 2^block_log2 keys and runs the
passes of one block over all of them.  Every key family mixes the row index
into the keys, so the keys of another row cannot pass for a row's own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from sort_oracles import want_rows  # noqa: E402

pytestmark = pytest.mark.gpu

U64 = np.uint64
MAX_KEYS = 1 << 21  # a case holds no more keys than this


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(a):
    """uint64 -> int64 storage, uint32 -> int32 storage, float64 as it is."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def bits(t):
    """The bit patterns of a device tensor on the host: u64 for 8-byte elements, u32 for 4-byte ones."""
    torch.cuda.synchronize()
    if t.element_size() == 8:
        return t.view(torch.int64).cpu().numpy().view(np.uint64)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def kmap(keys):
    """Order-preserving u64 pattern: u64 as it is; f64 with the sign set inverted, else the sign bit set."""
    if keys.dtype == np.float64:
        b = keys.view(np.uint64)
        return np.where(b >> U64(63) != 0, ~b, b | U64(1 << 63)).astype(np.uint64)
    return keys


def kunmap(o):
    """The f64 bit pattern of an ordered u64 pattern."""
    return np.where(o >> U64(63) != 0, o & U64(0x7FFFFFFFFFFFFFFF), ~o).astype(np.uint64)


def rand(rng, shape, dt):
    return rng.integers(0, np.iinfo(dt).max, size=shape, dtype=dt, endpoint=True)


def row_ids(rows, dt):
    return np.arange(rows, dtype=dt)[:, None]


def opposed_rows(rng, rows, cols, dt):
    """Row r's keys all lie strictly above row r + 1's: one level too many, or any
    merge across a row boundary, moves keys between rows."""
    span = dt(1 << 20)
    return (row_ids(rows, dt)[::-1] * span + rng.integers(0, 1 << 20, (rows, cols)).astype(dt)).astype(dt)


def sentinels(rng, rows, cols, dt):
    """A third all-ones (the value the kernels pad with), a third zero, shuffled
    per row; the rest random with the row in the low bits."""
    k = (rand(rng, (rows, cols), dt) & dt(~dt(0xFFFF))) | (row_ids(rows, dt) & dt(0xFFFF))
    k[:, : cols // 3] = np.iinfo(dt).max
    k[:, cols // 3: 2 * (cols // 3)] = 0
    return np.ascontiguousarray(rng.permuted(k, axis=1))


FAMILIES = {
    "random": lambda rng, rows, cols, dt: rand(rng, (rows, cols), dt) ^ (row_ids(rows, dt) * dt(0x9E3779B1)),
    "dups": lambda rng, rows, cols, dt: (row_ids(rows, dt) * dt(4) + rng.integers(0, 4, (rows, cols)).astype(dt))
    * dt(0x01000193),
    "equal": lambda rng, rows, cols, dt: np.broadcast_to(dt(0xCAFEF00D) + row_ids(rows, dt), (rows, cols)).copy(),
    "opposed_rows": opposed_rows,
    "sentinels": sentinels,
    "ascending": lambda rng, rows, cols, dt: np.arange(cols, dtype=dt)[None, :] * dt(3) + row_ids(rows, dt) * dt(7919),
    "descending": lambda rng, rows, cols, dt: np.arange(cols, 0, -1).astype(dt)[None, :] * dt(3)
    + row_ids(rows, dt) * dt(7919),
}


def make(family, seed, rows, cols, dt):
    k = np.ascontiguousarray(FAMILIES[family](np.random.default_rng(seed), rows, cols, dt))
    assert k.dtype == dt and k.shape == (rows, cols)
    return k


def check(ctx, keys, what=""):
    """Out of place into a fresh tensor: every row sorted, the input unchanged."""
    d = to_dev(keys)
    out = ctx.sort_rows(d)
    assert out.shape == d.shape and out.dtype == d.dtype and out.data_ptr() != d.data_ptr()
    np.testing.assert_array_equal(bits(out), want_rows(keys), err_msg=what)
    kb = keys.view(np.uint64) if keys.dtype == np.float64 else keys
    np.testing.assert_array_equal(bits(d), kb, err_msg=what + " (input changed)")


# ------------------------------------------------------------------ tile path

TILE_COLS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4097, 8191, 8192, 8193,
             16383, 16384, 16385, 32767, 32768]
TILE_CASES = [(np.uint32, c) for c in TILE_COLS] + [(np.uint64, c) for c in TILE_COLS if c <= 8192]


def tile_rows(cols, key_bytes):
    """One row alone, a partial tile, exactly one tile, a second tile with one
    row, several tiles with a partial last one -- capped at MAX_KEYS keys."""
    p = misort.rows_plan(cols, key_bytes)
    assert p["path"] == "tile"
    r = 1 << (p["tile_log2"] - p["block_log2"])
    cap = MAX_KEYS // cols
    assert cap >= 3
    rows = {min(x, cap) for x in (1, r - 1, r, r + 1, 2 * r + r // 2 + 1) if x > 0}
    if r == 1:
        rows |= {1, 2, 3}
    return sorted(rows)


@pytest.mark.parametrize("dt,cols", TILE_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_tile_path_random(ctx, dt, cols):
    kb = np.dtype(dt).itemsize
    for rows in tile_rows(cols, kb):
        check(ctx, make("random", 7000 + cols, rows, cols, dt), f"rows={rows}")


@pytest.mark.parametrize("family", sorted(set(FAMILIES) - {"random"}))
@pytest.mark.parametrize("dt,cols", [(np.uint32, 33), (np.uint32, 1000), (np.uint32, 8193),
                                     (np.uint64, 33), (np.uint64, 1000), (np.uint64, 4097)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_tile_path_families(ctx, dt, cols, family):
    kb = np.dtype(dt).itemsize
    for rows in tile_rows(cols, kb):
        check(ctx, make(family, 7100 + cols, rows, cols, dt), f"rows={rows}")


# ---------------------------------------------------------------- blocks path

BLOCK_COLS = {np.uint32: [32769, 40000, 131072, 131073, 300001], np.uint64: [8193, 10000, 32768, 32769, 100003]}
BLOCK_CASES = [(dt, c) for dt in BLOCK_COLS for c in BLOCK_COLS[dt]]


@pytest.mark.parametrize("family", ["random", "opposed_rows"])
@pytest.mark.parametrize("dt,cols", BLOCK_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_blocks_path(ctx, dt, cols, family):
    assert misort.rows_plan(cols, np.dtype(dt).itemsize)["path"] == "blocks"
    for rows in (1, 3, 5):
        assert rows * cols <= MAX_KEYS
        check(ctx, make(family, 7200 + cols, rows, cols, dt), f"rows={rows}")


@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=lambda v: v.__name__)
def test_blocks_path_sentinels(ctx, dt):
    cols = BLOCK_COLS[dt][1]
    for rows in (1, 3, 5):
        check(ctx, make("sentinels", 7300 + cols, rows, cols, dt), f"rows={rows}")


# ------------------------------------------------------------------------ f64

F64_SPECIAL = np.array([
    0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,  # +-0, +-inf
    0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,  # denormals
    0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,  # NaNs, varied payloads
    0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FF800000000BEEF, 0xFFF00000DEAD0000], dtype=np.uint64)


def f64_mix(rng, rows, cols):
    """Normal values of both signs, +-0.0, +-inf, denormals and NaNs of both
    signs; every row holds 0x7FFF..F (it maps to the padding pattern) and
    0xFFFF..F (the raw padding pattern: it maps to the smallest key)."""
    k = (rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-300, 300, (rows, cols))).view(np.uint64)
    pick = rng.random((rows, cols)) < 0.25
    k[pick] = F64_SPECIAL[rng.integers(0, F64_SPECIAL.size, int(pick.sum()))]
    for r in range(rows):
        k[r, (r + 1) % cols] = U64(0x7FFFFFFFFFFFFFFF)
        k[r, (r + 3) % cols] = U64(0xFFFFFFFFFFFFFFFF)
    return np.ascontiguousarray(k).view(np.float64)


# 8194: the shortest even long row -- the pad and unpad sweeps map f64 keys through 16-byte accesses
@pytest.mark.parametrize("cols", [5, 1000, 8192, 8193, 8194, 32769])
def test_f64_rows(ctx, cols):
    rows = 3
    keys = f64_mix(np.random.default_rng(7400 + cols), rows, cols)
    kb = keys.view(np.uint64)
    assert (kb == U64(0x7FFFFFFFFFFFFFFF)).any(axis=1).all() and (kb == U64(0xFFFFFFFFFFFFFFFF)).any(axis=1).all()
    if cols >= 1000:
        for pattern in F64_SPECIAL:
            assert (kb == pattern).any()
    d = to_dev(keys)
    assert d.dtype == torch.float64
    out = ctx.sort_rows(d)
    assert out.dtype == torch.float64
    got = bits(out)
    np.testing.assert_array_equal(got, want_rows(keys))  # every key bit-exact, NaN payloads included
    np.testing.assert_array_equal(bits(d), kb)
    # the documented order, in every row: the raw all-ones pattern (a negative NaN) first, 0x7FFF..F last
    assert (got[:, 0] == U64(0xFFFFFFFFFFFFFFFF)).all() and (got[:, -1] == U64(0x7FFFFFFFFFFFFFFF)).all()
    # in place gives the same
    assert ctx.sort_rows(d, out=d) is d
    np.testing.assert_array_equal(bits(d), got)


# ------------------------------------------------------- guards and aliasing

GUARD = {8: U64(0xA5A5A5A5A5A5A5A5), 4: np.uint32(0xA5A5A5A5)}
ALIAS_CASES = [(np.uint32, 1000), (np.uint32, 16384), (np.uint32, 40000), (np.uint64, 1000), (np.uint64, 10000)]


def guarded(n, dt, lead, fill=None):
    """(base, view): n elements starting `lead` elements into a 16-byte-aligned
    base tensor that keeps guard elements on both sides."""
    g = GUARD[np.dtype(dt).itemsize]
    body = np.full(n, g, dt) if fill is None else fill.reshape(-1)
    base = to_dev(np.concatenate([np.full(lead, g, dt), body, np.full(16 - lead, g, dt)]))
    assert base.data_ptr() % 16 == 0
    return base, base[lead: lead + n]


def guards_intact(base, n, lead):
    b = bits(base)
    g = GUARD[base.element_size()]
    return (b[:lead] == g).all() and (b[lead + n:] == g).all()


@pytest.mark.parametrize("dt,cols", ALIAS_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_canaries_input_unchanged_and_in_place(ctx, dt, cols):
    rows, lead = 5, 8  # 8 elements in: the view stays 16-byte aligned (the vector kernels)
    keys = make("random", 7500 + cols, rows, cols, dt)
    want = want_rows(keys)
    ib, iv = guarded(rows * cols, dt, lead, keys)
    ob, ov = guarded(rows * cols, dt, lead)
    assert iv.data_ptr() % 16 == 0 and ov.data_ptr() % 16 == 0
    inp, out = iv.view(rows, cols), ov.view(rows, cols)
    assert ctx.sort_rows(inp, out=out) is out
    np.testing.assert_array_equal(bits(out), want)
    np.testing.assert_array_equal(bits(inp), keys)  # out of place: the input is unchanged
    assert guards_intact(ob, rows * cols, lead) and guards_intact(ib, rows * cols, lead)
    assert ctx.sort_rows(inp, out=inp) is inp  # in place
    np.testing.assert_array_equal(bits(inp), want)
    assert guards_intact(ib, rows * cols, lead)


@pytest.mark.parametrize("dt,cols", [(np.uint32, 33), (np.uint32, 1001), (np.uint32, 40001),
                                     (np.uint64, 33), (np.uint64, 1001), (np.uint64, 10001)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_element_aligned_views(ctx, dt, cols):
    rows, lead = 7, 1
    keys = make("random", 7600 + cols, rows, cols, dt)
    ib, iv = guarded(rows * cols, dt, lead, keys)
    ob, ov = guarded(rows * cols, dt, lead)
    width = np.dtype(dt).itemsize
    assert iv.data_ptr() % 16 == width and ov.data_ptr() % 16 == width
    out = ctx.sort_rows(iv.view(rows, cols), out=ov.view(rows, cols))
    np.testing.assert_array_equal(bits(out), want_rows(keys))
    np.testing.assert_array_equal(bits(iv), keys.reshape(-1))
    assert guards_intact(ob, rows * cols, lead) and guards_intact(ib, rows * cols, lead)
    ctx.sort_rows(iv.view(rows, cols), out=iv.view(rows, cols))
    np.testing.assert_array_equal(bits(iv), want_rows(keys).reshape(-1))
    assert guards_intact(ib, rows * cols, lead)


@pytest.mark.parametrize("dt,cols", [(np.uint32, 1000), (np.uint32, 40000), (np.uint64, 10000)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_partial_overlap_is_refused(ctx, dt, cols):
    rows = 3
    n = rows * cols
    keys = make("random", 7700 + cols, 1, 2 * n, dt).reshape(-1)
    base = to_dev(keys)
    for shift in (1, cols, n - 1):
        for a, b in ((0, shift), (shift, 0)):
            with pytest.raises(misort.MisortError) as e:
                ctx.sort_rows(base[a: a + n].view(rows, cols), out=base[b: b + n].view(rows, cols))
            assert e.value.code == -1
    ctx.synchronize()
    np.testing.assert_array_equal(bits(base), keys)  # nothing written


# ------------------------------------------------------------------ the rest

@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=lambda v: v.__name__)
def test_one_row_equals_local_sort(ctx, dt):
    t = 1 << misort.tile_log2(np.dtype(dt).itemsize)
    for cols in (1000, t + 1, 100003):
        keys = make("dups" if cols == 1000 else "random", 7800 + cols, 1, cols, dt)
        d = to_dev(keys)
        a = ctx.sort_rows(d)
        b = ctx.local_sort(d.reshape(-1), out=torch.empty_like(d).reshape(-1))
        np.testing.assert_array_equal(bits(a).reshape(-1), bits(b))
        np.testing.assert_array_equal(bits(a), want_rows(keys))


def test_any_rank_sorts_the_last_dimension(ctx):
    keys = make("random", 79, 2 * 3 * 4, 37, np.uint32)
    d = to_dev(keys).view(2, 3, 4, 37)
    out = ctx.sort_rows(d)
    assert out.shape == (2, 3, 4, 37)
    np.testing.assert_array_equal(bits(out).reshape(24, 37), want_rows(keys))
    one = to_dev(keys[0])  # rank 1: one row
    np.testing.assert_array_equal(bits(ctx.sort_rows(one)), np.sort(keys[0]))


@pytest.mark.parametrize("dt,cols", [(np.uint32, 1000), (np.uint32, 40000), (np.uint64, 10000)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_on_the_contexts_stream(ctx, dt, cols):
    rows = 5
    keys = make("random", 8000 + cols, rows, cols, dt)
    d = to_dev(keys)
    out = torch.empty_like(d)
    torch.cuda.synchronize()
    ctx.sort_rows(d, out=out, stream=ctx.native_stream)
    ctx.synchronize()
    np.testing.assert_array_equal(bits(out), want_rows(keys))


MERGES = ("run_merge", "run_mergek")


@pytest.mark.parametrize("dt,cols,rows", [(np.uint32, 1000, 37), (np.uint32, 16384, 3), (np.uint32, 16385, 3),
                                          (np.uint64, 33, 700), (np.uint64, 8192, 3)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_profile_tile_path_is_one_tile_sort(ctx, dt, cols, rows):
    size = np.dtype(dt).itemsize
    d = to_dev(make("random", 8100 + cols, rows, cols, dt))
    out = torch.empty_like(d)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        ctx.sort_rows(d, out=out)
        torch.cuda.synchronize()
        rec = ctx.profile_read()
    finally:
        ctx.profile(False)
    launches, ms, nbytes = rec["tile_sort"]
    assert launches == 1 and ms > 0.0 and nbytes == 2 * rows * cols * size
    for kind in MERGES + ("other",):
        assert rec[kind][0] == 0, kind
    assert len(misort.KIND_NAMES) == 12


@pytest.mark.parametrize("dt,cols", [(np.uint32, 40000), (np.uint32, 300001), (np.uint64, 8193), (np.uint64, 100003)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_profile_blocks_path(ctx, dt, cols):
    size, rows = np.dtype(dt).itemsize, 3
    p = misort.rows_plan(cols, size)
    block = 1 << p["block_log2"]
    d = to_dev(make("random", 8200 + cols, rows, cols, dt))
    ctx.profile(True)
    try:
        ctx.profile_reset()
        out = ctx.sort_rows(d)
        torch.cuda.synchronize()
        rec = ctx.profile_read()
    finally:
        ctx.profile(False)
    launches, ms, nbytes = rec["other"]  # pad and unpad
    assert launches == 2 and ms > 0.0 and nbytes == 2 * (rows * cols + rows * block) * size
    for kind in ("tile_sort",) + MERGES:
        count = sum(1 for q in p["passes"] if q[0] == kind)
        assert rec[kind][0] == count, kind
        assert rec[kind][2] == count * 2 * rows * block * size, kind
    assert rec["tile_sort"][0] == 1
    np.testing.assert_array_equal(bits(out), want_rows(bits(d)))


def test_c_entry_point_rejects_bad_arguments(ctx):
    f = misort.lib().misort_local_sort_rows
    a = torch.zeros(64, dtype=torch.int64, device="cuda")
    b = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, q, s = a.data_ptr(), b.data_ptr(), ctx.native_stream
    for dt in (misort.F32, 4, -1):
        assert f(ctx._h, dt, p, q, 4, 8, s) == -1
    assert f(ctx._h, misort.U32, p, q, -1, 8, s) == -1
    assert f(ctx._h, misort.U32, p, q, 4, -8, s) == -1
    assert f(ctx._h, misort.U64, None, q, 4, 8, s) == -1
    assert f(ctx._h, misort.F64, p, None, 4, 8, s) == -1
    assert misort.lib().misort_last_error()
    for dt in (misort.U32, misort.U64, misort.F64):  # nothing to do: no pointer is looked at
        assert f(ctx._h, dt, None, None, 0, 8, s) == 0
        assert f(ctx._h, dt, None, None, 4, 0, s) == 0
    ctx.synchronize()
    assert not bits(a).any() and not bits(b).any()


def test_python_argument_checks(ctx):
    t = torch.arange(64, dtype=torch.int32, device="cuda").view(8, 8)
    with pytest.raises(ValueError):
        ctx.sort_rows(t.t())  # non-contiguous
    with pytest.raises(ValueError):
        ctx.sort_rows(t[:, ::2])
    with pytest.raises(TypeError):
        ctx.sort_rows(t, out=torch.empty(8, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ctx.sort_rows(t, out=torch.empty(7, 8, dtype=torch.int32, device="cuda"))  # too small
    with pytest.raises(TypeError):
        ctx.sort_rows(t.to(torch.float32))
    for shape in ((0, 8), (8, 0), (0,)):  # empty shapes: an empty tensor back, nothing raised
        e = torch.empty(shape, dtype=torch.int32, device="cuda")
        out = ctx.sort_rows(e)
        assert out.shape == e.shape and out.numel() == 0
        assert ctx.sort_rows(e, out=e) is e
    ctx.synchronize()
    np.testing.assert_array_equal(bits(t).reshape(-1), np.arange(64, dtype=np.uint32))
