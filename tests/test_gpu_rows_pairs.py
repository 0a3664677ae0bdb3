"""Row-wise key-value sort and argsort on one GPU (misort_local_sort_rows_pairs,
Context.sort_rows_pairs / argsort_rows) against numpy on the host:
rec = K(keys) << 32 | values, np.sort(rec, axis=1), split and mapped back; K is
the identity (u32 keys) or the order-preserving pattern of a float32.  For the
argsort the values are arange(cols) in every row.  Every comparison is on bit
patterns; there is no tolerance.

Two paths (misort.rows_plan(cols, 8)): "tile", cols <= 2^13, packs
R = 2^(tile_log2 - block_log2) rows into one LDS tile and forms the records in
registers; "blocks" pads longer rows to 2^block_log2 records.  Every key family
mixes the row index into the keys, so another row's pairs cannot pass for a
row's own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from sort_oracles import want_rows_pairs as want  # noqa: E402

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
ONES = U32(0xFFFFFFFF)
MAX_PAIRS = 1 << 21  # a case holds no more pairs than this


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(a, f32=False):
    """u32 bit patterns -> int32 storage, or float32 with the same bits."""
    a = np.ascontiguousarray(a, dtype=U32)
    return torch.from_numpy(a.view(np.float32 if f32 else np.int32)).cuda()


def bits(t):
    torch.cuda.synchronize()
    return t.view(torch.int32).cpu().numpy().view(U32)


def kmap(b, f32):
    """Order-preserving u32 pattern of a key's bits."""
    if not f32:
        return b
    return np.where(b >> U32(31) != 0, ~b, b | U32(1 << 31)).astype(U32)


def kunmap(o, f32):
    if not f32:
        return o
    return np.where(o >> U32(31) != 0, o & U32(0x7FFFFFFF), ~o).astype(U32)


def rand(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(U32)


def row_ids(rows):
    return np.arange(rows, dtype=U32)[:, None]


def opposed_rows(rng, rows, cols):
    """Row r's keys all lie strictly above row r + 1's: one level too many, or any
    merge across a row boundary, moves pairs between rows."""
    assert rows < 1 << 12
    return (row_ids(rows)[::-1] * U32(1 << 20) + rng.integers(0, 1 << 20, (rows, cols)).astype(U32)).astype(U32)


FAMILIES = {
    "random": lambda rng, rows, cols: rand(rng, (rows, cols)) ^ (row_ids(rows) * U32(0x9E3779B1)),
    "dups": lambda rng, rows, cols: (row_ids(rows) * U32(4) + rng.integers(0, 4, (rows, cols)).astype(U32))
    * U32(0x01000193),
    "equal": lambda rng, rows, cols: np.broadcast_to(U32(0xCAFEF00D) + row_ids(rows), (rows, cols)).copy(),
    "opposed_rows": opposed_rows,
    "ascending": lambda rng, rows, cols: np.arange(cols, dtype=U32)[None, :] * U32(3) + row_ids(rows) * U32(7919),
    "descending": lambda rng, rows, cols: np.arange(cols, 0, -1).astype(U32)[None, :] * U32(3)
    + row_ids(rows) * U32(7919),
}


def make(family, seed, rows, cols):
    """(keys, values) of a family.  "sentinels": a third of each row is the pair
    (0xFFFFFFFF, 0xFFFFFFFF) -- the padding record as a real record -- a third
    has key zero, the rest is random with the row in the low bits; shuffled per row."""
    rng = np.random.default_rng(seed)
    vals = rand(rng, (rows, cols))
    if family == "sentinels":
        keys = (rand(rng, (rows, cols)) & U32(0xFFFF0000)) | (row_ids(rows) & U32(0xFFFF))
        keys[:, : cols // 3] = ONES
        vals[:, : cols // 3] = ONES
        keys[:, cols // 3: 2 * (cols // 3)] = 0
        perm = np.argsort(rng.random((rows, cols)), axis=1)
        keys, vals = np.take_along_axis(keys, perm, axis=1), np.take_along_axis(vals, perm, axis=1)
    else:
        keys = FAMILIES[family](rng, rows, cols)
    keys, vals = np.ascontiguousarray(keys, dtype=U32), np.ascontiguousarray(vals, dtype=U32)
    assert keys.shape == vals.shape == (rows, cols)
    return keys, vals


def check(ctx, keys, vals, f32=False, what=""):
    """Out of place into fresh tensors, with the values and as an argsort: every
    row sorted, the inputs unchanged."""
    dk, dv = to_dev(keys, f32), to_dev(vals)
    ok, ov = ctx.sort_rows_pairs(dk, dv)
    assert ok.shape == dk.shape and ok.dtype == dk.dtype and ov.shape == dv.shape and ov.dtype == dv.dtype
    assert len({ok.data_ptr(), ov.data_ptr(), dk.data_ptr(), dv.data_ptr()}) == 4
    wk, wv = want(keys, vals, f32)
    np.testing.assert_array_equal(bits(ok), wk, err_msg=what + " (keys)")
    np.testing.assert_array_equal(bits(ov), wv, err_msg=what + " (values)")
    idx = ctx.argsort_rows(dk)
    assert idx.shape == dk.shape and idx.dtype == torch.int32
    ak, ai = want(keys, None, f32)
    np.testing.assert_array_equal(bits(idx), ai, err_msg=what + " (argsort)")
    # the argsort is the stable one, and it gathers the keys into sorted order
    np.testing.assert_array_equal(ai, np.argsort(kmap(keys, f32), axis=1, kind="stable").astype(U32))
    np.testing.assert_array_equal(np.take_along_axis(keys, bits(idx).astype(np.int64), axis=1), ak)
    np.testing.assert_array_equal(bits(dk), keys, err_msg=what + " (keys changed)")
    np.testing.assert_array_equal(bits(dv), vals, err_msg=what + " (values changed)")
    return wk, wv


# ------------------------------------------------------------------ tile path

# a multiple of 4 takes 16-byte accesses, odd lengths element accesses; 2, 6, 1002
# and 8190 are even but no multiple of 4: the 8-byte kernel
TILE_COLS = [1, 2, 3, 4, 5, 6, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 1002, 2047, 2048, 2049, 4097, 8190, 8191,
             8192]


def tile_rows(cols):
    """One row alone, a partial tile, exactly one tile, a second tile with one
    row, several tiles with a partial last one."""
    p = misort.rows_plan(cols, 8)
    assert p["path"] == "tile" and p["tile_log2"] == 13
    r = 1 << (p["tile_log2"] - p["block_log2"])
    rows = sorted({x for x in (1, r - 1, r, r + 1, 2 * r + r // 2 + 1) if x > 0})
    assert rows[-1] * cols <= MAX_PAIRS
    return rows


@pytest.mark.parametrize("cols", TILE_COLS)
def test_tile_path_random(ctx, cols):
    for rows in tile_rows(cols):
        check(ctx, *make("random", 9000 + cols, rows, cols), what=f"rows={rows}")


@pytest.mark.parametrize("family", sorted(set(FAMILIES) - {"random"}) + ["sentinels"])
@pytest.mark.parametrize("cols", [33, 1000, 1002, 4097])
def test_tile_path_families(ctx, cols, family):
    for rows in tile_rows(cols):
        keys, vals = make(family, 9100 + cols, rows, cols)
        if family == "sentinels":
            assert ((keys == ONES) & (vals == ONES)).sum(axis=1).min() == cols // 3
        wk, wv = check(ctx, keys, vals, what=f"rows={rows}")
        if family == "dups":
            assert all(len(np.unique(k)) <= 4 for k in keys)
            # the given values come out ascending inside each run of equal keys
            same = wk[:, 1:] == wk[:, :-1]
            assert same.any() and (wv[:, 1:][same] >= wv[:, :-1][same]).all()


# ---------------------------------------------------------------- blocks path

BLOCK_COLS = [8193, 10000, 32768, 32769, 100003]


@pytest.mark.parametrize("family", ["random", "opposed_rows"])
@pytest.mark.parametrize("cols", BLOCK_COLS)
def test_blocks_path(ctx, cols, family):
    assert misort.rows_plan(cols, 8)["path"] == "blocks"
    for rows in (1, 3, 5):
        assert rows * cols <= MAX_PAIRS
        check(ctx, *make(family, 9200 + cols, rows, cols), what=f"rows={rows}")


def test_blocks_path_sentinels(ctx):
    cols = 10000
    assert misort.rows_plan(cols, 8)["path"] == "blocks"
    for rows in (1, 3, 5):
        check(ctx, *make("sentinels", 9300 + cols, rows, cols), what=f"rows={rows}")


# ------------------------------------------------------------------------ f32

F32_SPECIAL = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # denormals
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,  # NaNs, varied payloads
    0x7FFFFFFF, 0xFFFFFFFF, 0x7FC0BEEF, 0xFF80DEAD], dtype=U32)


def f32_mix(rng, rows, cols):
    """Normal values of both signs, +-0.0, +-inf, denormals and NaNs of both
    signs; every row holds 0x7FFFFFFF (it maps to the padding record's high
    word) and 0xFFFFFFFF (the raw all-ones pattern: it maps to the smallest key)."""
    k = (rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-30, 30, (rows, cols))).astype(np.float32).view(U32)
    pick = rng.random((rows, cols)) < 0.25
    k[pick] = F32_SPECIAL[rng.integers(0, F32_SPECIAL.size, int(pick.sum()))]
    for r in range(rows):
        k[r, (r + 1) % cols] = U32(0x7FFFFFFF)
        k[r, (r + 3) % cols] = ONES
    return np.ascontiguousarray(k)


@pytest.mark.parametrize("cols", [5, 1000, 8192, 8193, 32769])
def test_f32_rows(ctx, cols):
    rows = 3
    rng = np.random.default_rng(9400 + cols)
    keys = f32_mix(rng, rows, cols)
    vals = rand(rng, (rows, cols))
    vals[keys == U32(0x7FFFFFFF)] = ONES  # the padding record itself as a real record
    assert (keys == U32(0x7FFFFFFF)).any(axis=1).all() and (keys == ONES).any(axis=1).all()
    if cols >= 1000:
        for pattern in F32_SPECIAL:
            assert (keys == pattern).any()
    wk, wv = check(ctx, keys, vals, f32=True)  # every key bit-exact, NaN payloads included
    # the documented order, in every row: the raw all-ones pattern (a negative NaN) first, 0x7FFFFFFF last
    assert (wk[:, 0] == ONES).all() and (wk[:, -1] == U32(0x7FFFFFFF)).all()
    dk, dv = to_dev(keys, True), to_dev(vals)
    assert dk.dtype == torch.float32
    ok, ov = ctx.sort_rows_pairs(dk, dv, out_keys=dk, out_values=dv)  # in place gives the same
    assert ok is dk and ov is dv and ok.dtype == torch.float32
    np.testing.assert_array_equal(bits(dk), wk)
    np.testing.assert_array_equal(bits(dv), wv)
    assert (bits(dk)[:, 0] == ONES).all() and (bits(dk)[:, -1] == U32(0x7FFFFFFF)).all()


# ------------------------------------------------------- guards and aliasing

GUARD = U32(0xA5A5A5A5)


def guarded(n, lead, fill=None):
    """(base, view): n elements starting `lead` elements into a 16-byte-aligned
    base tensor that keeps guard elements on both sides."""
    body = np.full(n, GUARD, U32) if fill is None else fill.reshape(-1)
    base = to_dev(np.concatenate([np.full(lead, GUARD, U32), body, np.full(16 - lead, GUARD, U32)]))
    assert base.data_ptr() % 16 == 0
    return base, base[lead: lead + n]


def guards_intact(base, n, lead):
    b = bits(base)
    return (b[:lead] == GUARD).all() and (b[lead + n:] == GUARD).all()


def aliasing_case(ctx, rows, cols, lead, seed):
    keys, vals = make("random", seed, rows, cols)
    keys[:, ::9] = keys[:, :1]  # equal keys: the values decide
    n = rows * cols
    wk, wv = want(keys, vals)
    _, ai = want(keys)

    def fresh():
        kb, kv = guarded(n, lead, keys)
        vb, vv = guarded(n, lead, vals)
        return kb, kv.view(rows, cols), vb, vv.view(rows, cols)

    def new():
        b, v = guarded(n, lead)
        return b, v.view(rows, cols)

    # out of place: the inputs are unchanged, no guard element is touched
    kb, dk, vb, dv = fresh()
    assert dk.data_ptr() % 16 == 4 * lead % 16
    (okb, ok), (ovb, ov) = new(), new()
    a, b = ctx.sort_rows_pairs(dk, dv, out_keys=ok, out_values=ov)
    assert a is ok and b is ov
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(bits(dv), vals)
    for base in (kb, vb, okb, ovb):
        assert guards_intact(base, n, lead)
    # argsort into a guarded output
    ib, idx = new()
    assert ctx.argsort_rows(dk, out=idx) is idx
    np.testing.assert_array_equal(bits(idx), ai)
    np.testing.assert_array_equal(bits(dk), keys)
    assert guards_intact(ib, n, lead) and guards_intact(kb, n, lead)
    # in place on the keys, on the values, on both
    for keys_in_place, vals_in_place in ((True, False), (False, True), (True, True)):
        kb, dk, vb, dv = fresh()
        (okb, ok), (ovb, ov) = new(), new()
        a, b = ctx.sort_rows_pairs(dk, dv, out_keys=dk if keys_in_place else ok,
                                   out_values=dv if vals_in_place else ov)
        np.testing.assert_array_equal(bits(a), wk)
        np.testing.assert_array_equal(bits(b), wv)
        if not keys_in_place:
            np.testing.assert_array_equal(bits(dk), keys)
        if not vals_in_place:
            np.testing.assert_array_equal(bits(dv), vals)
        for base in (kb, vb, okb, ovb):
            assert guards_intact(base, n, lead)


@pytest.mark.parametrize("cols", [1000, 10000])
def test_canaries_inputs_unchanged_and_in_place(ctx, cols):
    aliasing_case(ctx, 5, cols, 8, 9500 + cols)  # 8 elements in: the views stay 16-byte aligned


@pytest.mark.parametrize("cols", [33, 1001, 10001])
def test_element_aligned_views(ctx, cols):
    aliasing_case(ctx, 7, cols, 1, 9600 + cols)  # one element into the storage, odd cols


# 4096: a row is a whole 2^12 block and a tile holds two, so three tiles take the 8-byte
# kernel's unchecked non-temporal accesses and the last, one row, its bounds checks
@pytest.mark.parametrize("cols", [1000, 1002, 4096, 10000])
def test_eight_byte_aligned_views(ctx, cols):
    aliasing_case(ctx, 7, cols, 2, 9650 + cols)  # two elements in: 8-byte accesses at the most


def test_eight_byte_kernel_knob_gives_the_same(ctx, monkeypatch):
    keys, vals = make("dups", 9660, 37, 1000)
    dk, dv = to_dev(keys), to_dev(vals)
    assert dk.data_ptr() % 16 == 0 and dv.data_ptr() % 16 == 0
    monkeypatch.setenv("MISORT_ROWS_PAIRS_W", "2")  # read per call
    ok, ov = ctx.sort_rows_pairs(dk, dv)
    idx = ctx.argsort_rows(dk)
    wk, wv = want(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(idx), want(keys)[1])


@pytest.mark.parametrize("cols", [1000, 10000])
def test_partial_overlap_is_refused(ctx, cols):
    rows = 3
    n = rows * cols
    rng = np.random.default_rng(9700 + cols)
    host = [rand(rng, 2 * n) for _ in range(3)]
    base, other, third = (to_dev(h) for h in host)

    def view(t, a):
        return t[a: a + n].view(rows, cols)

    for shift in (1, cols, n - 1):
        for a, b in ((0, shift), (shift, 0)):
            calls = (
                # keys in / keys out
                lambda: ctx.sort_rows_pairs(view(base, a), view(other, 0), out_keys=view(base, b),
                                            out_values=view(third, 0)),
                # values in / values out
                lambda: ctx.sort_rows_pairs(view(other, 0), view(base, a), out_keys=view(third, 0),
                                            out_values=view(base, b)),
                # keys out / values out
                lambda: ctx.sort_rows_pairs(view(other, 0), view(third, 0), out_keys=view(base, a),
                                            out_values=view(base, b)),
                # argsort: keys in / indices out
                lambda: ctx.argsort_rows(view(base, a), out=view(base, b)),
            )
            for call in calls:
                with pytest.raises(misort.MisortError) as e:
                    call()
                assert e.value.code == -1
    # the two outputs may not be one array either
    with pytest.raises(misort.MisortError) as e:
        ctx.sort_rows_pairs(view(other, 0), view(third, 0), out_keys=view(base, 0), out_values=view(base, 0))
    assert e.value.code == -1
    ctx.synchronize()
    for t, h in zip((base, other, third), host):
        np.testing.assert_array_equal(bits(t), h)  # nothing written


# ------------------------------------------------------------------ the rest

@pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])
def test_one_row_equals_sort_pairs_and_argsort(ctx, f32):
    for cols in (1000, (1 << 13) + 1, 100003):
        keys, vals = make("dups" if cols == 1000 else "random", 9800 + cols, 1, cols)
        dk, dv = to_dev(keys, f32), to_dev(vals)
        rk, rv = ctx.sort_rows_pairs(dk, dv)
        pk, pv = ctx.sort_pairs(dk.reshape(-1), dv.reshape(-1))
        np.testing.assert_array_equal(bits(rk).reshape(-1), bits(pk))
        np.testing.assert_array_equal(bits(rv).reshape(-1), bits(pv))
        np.testing.assert_array_equal(bits(ctx.argsort_rows(dk)).reshape(-1), bits(ctx.argsort(dk.reshape(-1))))
        wk, wv = want(keys, vals, f32)
        np.testing.assert_array_equal(bits(rk), wk)
        np.testing.assert_array_equal(bits(rv), wv)


@pytest.mark.parametrize("cols", [257, 8192, 10000])
def test_argsort_rows_gathers_keys_into_sort_rows(ctx, cols):
    keys, _ = make("dups" if cols == 257 else "random", 9900 + cols, 6, cols)
    d = to_dev(keys)
    idx = ctx.argsort_rows(d)
    assert idx.dtype == d.dtype and idx.shape == d.shape
    # gathered on the host, after a synchronisation: the sorts ran on the context's
    # own stream, which torch's kernels on its default stream do not wait for
    got = bits(idx)
    np.testing.assert_array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(cols, dtype=U32), (6, cols)))
    np.testing.assert_array_equal(np.take_along_axis(keys, got.astype(np.int64), axis=1), bits(ctx.sort_rows(d)))


def test_any_rank_sorts_the_last_dimension(ctx):
    keys, vals = make("random", 99, 2 * 3 * 4, 37)
    wk, wv = want(keys, vals)
    dk, dv = to_dev(keys).view(2, 3, 4, 37), to_dev(vals).view(2, 3, 4, 37)
    ok, ov = ctx.sort_rows_pairs(dk, dv)
    assert ok.shape == ov.shape == (2, 3, 4, 37)
    np.testing.assert_array_equal(bits(ok).reshape(24, 37), wk)
    np.testing.assert_array_equal(bits(ov).reshape(24, 37), wv)
    idx = ctx.argsort_rows(dk)
    assert idx.shape == (2, 3, 4, 37)
    np.testing.assert_array_equal(bits(idx).reshape(24, 37), want(keys)[1])
    k1, v1 = to_dev(keys[0]), to_dev(vals[0])  # rank 1: one row
    ok, ov = ctx.sort_rows_pairs(k1, v1)
    assert ok.shape == ov.shape == (37,)
    np.testing.assert_array_equal(bits(ok), wk[0])
    np.testing.assert_array_equal(bits(ov), wv[0])
    np.testing.assert_array_equal(bits(ctx.argsort_rows(k1)), want(keys[:1])[1][0])


@pytest.mark.parametrize("cols", [1000, 10000])
def test_on_the_contexts_stream(ctx, cols):
    keys, vals = make("random", 10000 + cols, 5, cols)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov, idx = torch.empty_like(dk), torch.empty_like(dv), torch.empty_like(dk)
    torch.cuda.synchronize()
    ctx.sort_rows_pairs(dk, dv, out_keys=ok, out_values=ov, stream=ctx.native_stream)
    ctx.argsort_rows(dk, out=idx, stream=ctx.native_stream)
    ctx.synchronize()
    wk, wv = want(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(idx), want(keys)[1])


def test_single_column_copies_and_argsort_writes_zeros(ctx):
    keys, vals = make("random", 101, 9, 1)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = ctx.sort_rows_pairs(dk, dv)
    np.testing.assert_array_equal(bits(ok), keys)
    np.testing.assert_array_equal(bits(ov), vals)
    idx = torch.full_like(dk, 7)
    torch.cuda.synchronize()  # torch's fill is not ordered against the context's stream
    ctx.argsort_rows(dk, out=idx)
    assert not bits(idx).any()
    a, b = ctx.sort_rows_pairs(dk, dv, out_keys=dk, out_values=dv)
    assert a is dk and b is dv
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(bits(dv), vals)


MERGES = ("run_merge", "run_mergek")


def profiled(ctx, call):
    ctx.profile(True)
    try:
        ctx.profile_reset()
        out = call()
        torch.cuda.synchronize()
        return out, ctx.profile_read()
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("cols,rows", [(33, 700), (1000, 37), (8192, 3)])
def test_profile_tile_path_is_one_tile_sort(ctx, cols, rows):
    keys, vals = make("random", 10100 + cols, rows, cols)
    dk, dv = to_dev(keys), to_dev(vals)
    # bytes: 4 per element of every array in use
    for call, arrays in ((lambda: ctx.sort_rows_pairs(dk, dv), 4), (lambda: ctx.argsort_rows(dk), 2)):
        _, rec = profiled(ctx, call)
        launches, ms, nbytes = rec["tile_sort"]
        assert launches == 1 and ms > 0.0 and nbytes == arrays * 4 * rows * cols
        for kind in MERGES + ("other",):
            assert rec[kind][0] == 0, kind
    assert len(misort.KIND_NAMES) == 12


@pytest.mark.parametrize("cols", [8193, 100003])
def test_profile_blocks_path(ctx, cols):
    rows = 3
    p = misort.rows_plan(cols, 8)
    assert p["path"] == "blocks"
    block = 1 << p["block_log2"]
    keys, vals = make("random", 10200 + cols, rows, cols)
    dk, dv = to_dev(keys), to_dev(vals)
    n = rows * cols
    # pad: the arrays it reads + the padded records; unpad: the records of the rows + the arrays it writes
    for call, moved in ((lambda: ctx.sort_rows_pairs(dk, dv), (8 * n + 8 * rows * block) + (8 * n + 8 * n)),
                        (lambda: ctx.argsort_rows(dk), (4 * n + 8 * rows * block) + (8 * n + 4 * n))):
        _, rec = profiled(ctx, call)
        launches, ms, nbytes = rec["other"]
        assert launches == 2 and ms > 0.0 and nbytes == moved
        for kind in ("tile_sort",) + MERGES:
            count = sum(1 for q in p["passes"] if q[0] == kind)
            assert rec[kind][0] == count, kind
            assert rec[kind][2] == count * 2 * rows * block * 8, kind
        assert rec["tile_sort"][0] == 1


def test_c_entry_point_rejects_bad_arguments(ctx):
    f = misort.lib().misort_local_sort_rows_pairs
    t = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(4)]
    ki, vi, ko, vo = (x.data_ptr() for x in t)
    s = ctx.native_stream
    for dt in (misort.U64, misort.F64, 4, -1):
        assert f(ctx._h, dt, ki, vi, ko, vo, 4, 8, s) == -1
    assert f(ctx._h, misort.U32, ki, vi, ko, vo, -1, 8, s) == -1
    assert f(ctx._h, misort.U32, ki, vi, ko, vo, 4, -8, s) == -1
    assert f(ctx._h, misort.U32, None, vi, ko, vo, 4, 8, s) == -1  # no keys
    assert f(ctx._h, misort.F32, ki, vi, ko, None, 4, 8, s) == -1  # no value output
    assert f(ctx._h, misort.U32, ki, None, None, vo, 1, (1 << 32) + 1, s) == -1  # 32-bit column indices
    assert misort.lib().misort_last_error()
    for dt in (misort.U32, misort.F32):  # nothing to do: no pointer is looked at
        assert f(ctx._h, dt, None, None, None, None, 0, 8, s) == 0
        assert f(ctx._h, dt, None, None, None, None, 4, 0, s) == 0
    ctx.synchronize()
    for x in t:
        assert not bits(x).any()


def test_python_argument_checks(ctx):
    k = torch.arange(64, dtype=torch.int32, device="cuda").view(8, 8)
    v = torch.arange(64, dtype=torch.int32, device="cuda").view(8, 8)
    with pytest.raises(ValueError):
        ctx.sort_rows_pairs(k.t(), v)  # non-contiguous
    with pytest.raises(ValueError):
        ctx.argsort_rows(k[:, ::2])
    with pytest.raises(ValueError):
        ctx.argsort_rows(torch.tensor(3, dtype=torch.int32, device="cuda"))  # rank 0
    for bad in (torch.int64, torch.float64):  # wrong key dtype
        with pytest.raises(TypeError):
            ctx.sort_rows_pairs(k.to(bad), v)
        with pytest.raises(TypeError):
            ctx.argsort_rows(k.to(bad))
    with pytest.raises(TypeError):
        ctx.sort_rows_pairs(k, v.to(torch.int64))  # wrong values dtype
    with pytest.raises(TypeError):
        ctx.sort_rows_pairs(k, v, out_keys=torch.empty(8, 8, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        ctx.argsort_rows(k, out=torch.empty(8, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ctx.sort_rows_pairs(k, v, out_values=torch.empty(7, 8, dtype=torch.int32, device="cuda"))  # too small
    with pytest.raises(ValueError):
        ctx.argsort_rows(k, out=torch.empty(63, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ctx.sort_rows_pairs(k, v.view(4, 16))  # shape mismatch
    with pytest.raises(ValueError):
        ctx.sort_rows_pairs(k, v[:7])
    for shape in ((0, 5), (5, 0)):  # empty shapes: empty tensors back, nothing raised
        e = torch.empty(shape, dtype=torch.int32, device="cuda")
        ok, ov = ctx.sort_rows_pairs(e, e.clone())
        assert ok.shape == ov.shape == e.shape
        idx = ctx.argsort_rows(e.to(torch.float32))
        assert idx.shape == e.shape and idx.dtype == torch.int32
    ctx.synchronize()
    np.testing.assert_array_equal(bits(k).reshape(-1), np.arange(64, dtype=U32))
    np.testing.assert_array_equal(bits(v).reshape(-1), np.arange(64, dtype=U32))
