"""Row-wise top-k on one GPU (misort_local_topk_rows, Context.topk_rows) against
tests/topk_oracle.py: per row the first k of the stable argsort of T(key), T = K
for the smallest keys and ~K for the largest, K the identity (u32) or the
order-preserving pattern of a float32.  Every comparison is on bit patterns;
there is no tolerance.  The shapes are the smallest at which each mechanism of
misort.topk_plan can break: rows below, at and above a lane's 32 records and the
tile's 2^13, a second mostly empty tile, a piece with one real record, a last
pass of exactly 2^13 candidates, and the first shape with a pass from
candidates to candidates."""
import ctypes
import functools

import numpy as np
import pytest

import guard_bands as GB
import stream_order as SO
import topk_oracle as TO
from stream_order import In, Out

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
ONES = U32(0xFFFFFFFF)
DIRECTIONS = pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])


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


def to_dev(a, f32=False, lead=0):
    """u32 bit patterns -> int32 storage, or float32 with the same bits; ``lead``
    elements of storage before the view."""
    a = np.ascontiguousarray(a, dtype=U32)
    flat = np.concatenate([np.zeros(lead, U32), a.reshape(-1)])
    t = torch.from_numpy(flat.view(F32 if f32 else np.int32)).cuda()
    return t[lead:].view(a.shape)


def bits(t):
    torch.cuda.synchronize()
    return t.contiguous().view(torch.int32).cpu().numpy().view(U32)


def row_ids(rows):
    return np.arange(rows, dtype=U32)[:, None]


# ---- key families: (rng, rows, cols, largest) -> u32 bit patterns -------------------------------------

def fam_random(rng, rows, cols, largest):
    """Random keys, a third of them from 16 values: ties meet the cut."""
    k = rng.integers(0, 1 << 32, size=(rows, cols), dtype=np.uint64).astype(U32) ^ (row_ids(rows) * U32(0x9E3779B1))
    k[rng.random((rows, cols)) < 1 / 3] &= U32(0xF)
    return k


def fam_four(rng, rows, cols, largest):
    """Four distinct values: ties span the pieces and the column order is the whole test."""
    return rng.integers(0, 4, size=(rows, cols)).astype(U32) * U32(0x55555555)


def fam_equal(rng, rows, cols, largest):
    return np.broadcast_to(U32(0xCAFEF00D) + row_ids(rows), (rows, cols)).copy()


def fam_half_sentinel(rng, rows, cols, largest):
    """All 0xFFFFFFFF for smallest, all 0 for largest: T is all-ones, the record's
    high half is the sentinel's (f32: the patterns whose mapped key is that)."""
    return np.full((rows, cols), 0 if largest else ONES, dtype=U32)


def best(largest):
    return (lambda n: ONES - np.arange(n, dtype=U32) % U32(3)) if largest else (lambda n: np.arange(n, dtype=U32) % U32(3))


def fam_winners_last(rng, rows, cols, largest):
    """The winners are the row's last 1500 columns (the last piece, and the end of the one before)."""
    k = rng.integers(1 << 8, 1 << 24, size=(rows, cols)).astype(U32)
    n = min(cols, 1500)
    k[:, cols - n:] = best(largest)(n)[None, :]
    return k


def fam_winners_one_piece(rng, rows, cols, largest):
    """All winners lie in one piece of 2^13 columns, the second where there is one."""
    k = rng.integers(1 << 8, 1 << 24, size=(rows, cols)).astype(U32)
    lo = 8192 if cols >= 8192 + 1500 else 0
    n = min(cols - lo, 1500)
    at = lo + rng.permutation(min(cols - lo, 8192))[:n]
    k[:, at] = best(largest)(n)[None, :]
    return k


def fam_f32(rng, rows, cols, largest):
    """NaNs of both signs, +-0, +-inf, denormals among random floats."""
    return SO.f32_keys(int(rng.integers(1 << 30)), (rows, cols)).view(U32)


def fam_half_sentinel_f32(rng, rows, cols, largest):
    """The float patterns whose T is all-ones: the negative NaN 0xFFFFFFFF (mapped
    key 0) for largest, the positive NaN 0x7FFFFFFF for smallest."""
    return np.full((rows, cols), ONES if largest else U32(0x7FFFFFFF), dtype=U32)


FAMILIES = {"random": fam_random, "four": fam_four, "equal": fam_equal, "half_sentinel": fam_half_sentinel,
            "winners_last": fam_winners_last, "winners_one_piece": fam_winners_one_piece, "f32": fam_f32,
            "half_sentinel_f32": fam_half_sentinel_f32}
F32_FAMILIES = ("f32", "half_sentinel_f32")


@functools.lru_cache(maxsize=8)
def data(family, rows, cols, largest):
    """(keys, stable order of T) of a case: computed once, read-only."""
    f32 = family in F32_FAMILIES
    rng = np.random.default_rng([rows, cols, int(largest), sorted(FAMILIES).index(family)])
    keys = np.ascontiguousarray(FAMILIES[family](rng, rows, cols, largest), dtype=U32)
    assert keys.shape == (rows, cols)
    order = np.argsort(TO.tmap(keys, largest, f32), axis=1, kind="stable").astype(U32)
    keys.setflags(write=False)
    order.setflags(write=False)
    return keys, order


def want(keys, order, k):
    idx = order[:, :k]
    return np.take_along_axis(keys, idx.astype(np.int64), axis=1), idx


def check(ctx, family, rows, cols, ks, largest):
    f32 = family in F32_FAMILIES
    keys, order = data(family, rows, cols, largest)
    dk = to_dev(keys, f32)
    for k in ks:
        what = f"{family} {rows}x{cols} k={k} {'largest' if largest else 'smallest'}"
        vals, idx = ctx.topk_rows(dk, k, largest=largest)
        assert vals.shape == idx.shape == (rows, k) and vals.dtype == dk.dtype and idx.dtype == torch.int32
        wk, wi = want(keys, order, k)
        np.testing.assert_array_equal(bits(idx), wi, err_msg=what + " (indices)")
        np.testing.assert_array_equal(bits(vals), wk, err_msg=what + " (values)")
    np.testing.assert_array_equal(bits(dk), keys, err_msg=f"{family} {rows}x{cols} (keys changed)")
    # the oracle of this file is topk_oracle's
    k = ks[-1]
    ok, oi = TO.topk_rows(keys, k, largest, f32)
    wk, wi = want(keys, order, k)
    assert np.array_equal(ok, wk) and np.array_equal(oi, wi)


# ---- short rows: one pass, keys to outputs --------------------------------------------------------------

def short_ks(cols):
    return sorted({1, min(2, cols), cols // 2 or 1, cols})


@DIRECTIONS
@pytest.mark.parametrize("rows", [1, 3, 257])
@pytest.mark.parametrize("cols", [1, 2, 31, 32, 33, 64, 1000, 4097, 8192])
def test_short_rows(ctx, cols, rows, largest):
    """257 rows of up to 32 keys cross into a second, mostly empty tile."""
    assert len(misort.topk_plan(cols, 1)) == 1
    check(ctx, "random", rows, cols, short_ks(cols), largest)


@DIRECTIONS
@pytest.mark.parametrize("rows,cols", [(257, 31), (5, 1000), (3, 4097)])
@pytest.mark.parametrize("family", ["four", "equal", "half_sentinel", "f32", "half_sentinel_f32"])
def test_short_rows_key_families(ctx, family, rows, cols, largest):
    check(ctx, family, rows, cols, short_ks(cols), largest)
    if family in ("equal", "half_sentinel", "half_sentinel_f32"):  # all keys equal: the lowest columns, in order
        _, order = data(family, rows, cols, largest)
        np.testing.assert_array_equal(order, np.broadcast_to(np.arange(cols, dtype=U32), (rows, cols)))


# ---- long rows: pieces of 2^13, candidates in scratch ---------------------------------------------------

LONG = [(8193, 1024),    # the second piece holds one real record and 1023 sentinels
        (16384, 999),    # two full pieces; k odd: element stores
        (40001, 7),      # odd: element loads
        (65536, 1024),   # the last pass takes exactly 2^13 candidates
        (65537, 1024),   # the smallest shape with a pass from candidates to candidates
        (65537, 1)]


@DIRECTIONS
@pytest.mark.parametrize("cols,k", LONG)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_long_rows(ctx, family, cols, k, largest):
    plan = misort.topk_plan(cols, k)
    assert len(plan) == (3 if (cols, k) == (65537, 1024) else 2)
    check(ctx, family, 3, cols, [k], largest)
    if family in ("equal", "half_sentinel", "half_sentinel_f32"):  # what check() compared with: columns 0 .. k - 1
        _, order = data(family, 3, cols, largest)
        np.testing.assert_array_equal(order[:, :k], np.broadcast_to(np.arange(k, dtype=U32), (3, k)))


# ---- the buffer contract -------------------------------------------------------------------------------

@DIRECTIONS
@pytest.mark.parametrize("rows,cols,k", [(257, 33, 5), (3, 1000, 8), (3, 4096, 4096), (3, 65537, 1024)])
@pytest.mark.parametrize("with_values", [True, False], ids=["values", "indices_only"])
def test_views_and_guard_bands(ctx, rows, cols, k, with_values, largest):
    """Input and outputs start one element into their storage; the outputs lie
    between canary bands: exactly rows * k elements of each are written."""
    keys, order = data("random", rows, cols, largest)
    wk, wi = want(keys, order, k)
    n = rows * k
    canary = GB.canary_for(wk.reshape(-1), wi.reshape(-1))
    dk = to_dev(keys, lead=1)
    assert dk.data_ptr() % 16 == 4
    bases = {}
    for name in ("vals", "idx"):
        base, _ = GB.guarded(n, U32, 1, canary)
        bases[name] = torch.from_numpy(base.view(np.int32)).cuda()
    ov, oi = (bases[x][1:1 + n].view(rows, k) for x in ("vals", "idx"))
    if with_values:
        gv, gi = ctx.topk_rows(dk, k, largest=largest, out_values=ov, out_indices=oi)
        assert gv is ov and gi is oi
    else:
        assert ctx.topk_rows_indices(dk, k, largest=largest, out=oi) is oi
    np.testing.assert_array_equal(bits(oi), wi)
    np.testing.assert_array_equal(bits(ov), wk if with_values else np.full((rows, k), canary))
    for name in ("vals", "idx"):
        GB.assert_guards(bits(bases[name]), n, 1, canary)
    np.testing.assert_array_equal(bits(dk), keys)


# ---- refusals ------------------------------------------------------------------------------------------

def raw(ctx, dt, keys, vals, idx, rows, cols, k, largest=1):
    p = [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (keys, vals, idx)]
    return misort.lib().misort_local_topk_rows(ctx._h, dt, p[0], p[1], p[2], rows, cols, k, largest, None)


def test_refusals_leave_the_outputs_unchanged(ctx):
    rows, cols, k = 3, 1000, 8
    keys, _ = data("random", rows, cols, True)
    buf = to_dev(np.concatenate([keys.reshape(-1), np.full(4 * rows * k, 0x5A5A5A5A, U32)]))
    before = bits(buf).copy()
    dk = buf[:rows * cols].view(rows, cols)
    free = buf[rows * cols:]
    ov, oi = free[:rows * k].view(rows, k), free[rows * k:2 * rows * k].view(rows, k)

    def refused(call, needle=None):
        with pytest.raises(misort.MisortError) as e:
            call()
        assert e.value.code == -1
        if needle:
            assert needle in str(e.value)
        np.testing.assert_array_equal(bits(buf), before)

    flat = dk.view(-1)
    # an output overlapping the input: at its start, at its end (the last element), and the two outputs
    refused(lambda: ctx.topk_rows(dk, k, out_values=flat[:rows * k], out_indices=oi), "overlaps")
    refused(lambda: ctx.topk_rows(dk, k, out_values=ov, out_indices=flat[:rows * k]), "overlaps")
    refused(lambda: ctx.topk_rows(dk, k, out_values=ov, out_indices=buf[rows * cols - 1:rows * cols - 1 + rows * k]),
            "overlaps")
    refused(lambda: ctx.topk_rows_indices(dk, k, out=flat[-rows * k:]), "overlaps")
    refused(lambda: ctx.topk_rows(dk, k, out_values=ov, out_indices=free[rows * k - 1:2 * rows * k - 1]), "overlaps")
    refused(lambda: ctx.topk_rows(dk, k, out_values=ov, out_indices=ov), "overlaps")
    # sizes
    big = to_dev(np.full(2 * 901, 0x5A5A5A5A, U32))
    refused(lambda: ctx.topk_rows(dk[:, :4].contiguous(), 5, out_values=ov, out_indices=oi))          # k > cols
    refused(lambda: ctx.topk_rows(flat[:900].view(1, 900), 901, out_values=big[:901], out_indices=big[901:]))
    assert np.all(bits(big) == U32(0x5A5A5A5A))
    # key types of the 64-bit sorts; null arrays; negative sizes
    for dt in (misort.U64, misort.F64, 7):
        assert raw(ctx, dt, dk, ov, oi, rows, cols, k) == -1
    assert raw(ctx, misort.U32, None, ov, oi, rows, cols, k) == -1
    assert raw(ctx, misort.U32, dk, ov, None, rows, cols, k) == -1
    for shape in ((-1, cols, k), (rows, -1, k), (rows, cols, -1)):
        assert raw(ctx, misort.U32, dk, ov, oi, *shape) == -1
    np.testing.assert_array_equal(bits(buf), before)
    with pytest.raises(TypeError):
        ctx.topk_rows(dk.view(torch.int64), 2)
    with pytest.raises(TypeError):
        ctx.topk_rows(dk, k, out_values=ov.view(torch.float32))
    with pytest.raises(ValueError):
        ctx.topk_rows(dk.t(), 2)
    with pytest.raises(ValueError):
        ctx.topk_rows(dk, k, out_values=ov, out_indices=oi.view(-1)[:rows * k - 1])
    with pytest.raises(ValueError):
        ctx.topk_rows(dk, -1)
    np.testing.assert_array_equal(bits(buf), before)


def test_long_rows_refuse_a_large_k(ctx):
    keys, _ = data("random", 3, 8193, True)
    dk = to_dev(keys)
    ov = to_dev(np.full((3, 1025), 0x5A5A5A5A, U32))
    oi = to_dev(np.full((3, 1025), 0x5A5A5A5A, U32))
    with pytest.raises(misort.MisortError) as e:
        ctx.topk_rows(dk, 1025, out_values=ov, out_indices=oi)
    assert e.value.code == -1 and "misort_local_sort_rows_pairs" in str(e.value)
    assert np.all(bits(ov) == U32(0x5A5A5A5A)) and np.all(bits(oi) == U32(0x5A5A5A5A))
    np.testing.assert_array_equal(bits(dk), keys)


def test_too_many_columns_are_refused_before_any_pointer_is_used(ctx):
    """No array of 2^31 + 1 columns exists here: the null pointers are never looked at."""
    lib = misort.lib()
    assert lib.misort_local_topk_rows(ctx._h, misort.U32, None, None, None, 1, (1 << 31) + 1, 1, 1, None) == -1
    assert b"2^31" in lib.misort_last_error()


def test_empty_shapes_are_no_ops(ctx):
    lib = misort.lib()
    # no pointer is looked at
    assert lib.misort_local_topk_rows(ctx._h, misort.U32, None, None, None, 0, 100, 5, 1, None) == 0
    assert lib.misort_local_topk_rows(ctx._h, misort.F32, None, None, None, 7, 100, 0, 0, None) == 0
    assert lib.misort_local_topk_rows(ctx._h, misort.U32, None, None, None, 7, 0, 0, 0, None) == 0
    keys = to_dev(np.arange(15, dtype=U32).reshape(3, 5))
    v, i = ctx.topk_rows(keys, 0)
    assert v.shape == i.shape == (3, 0)
    v, i = ctx.topk_rows(keys[:0], 2)
    assert v.shape == i.shape == (0, 2)
    guard = to_dev(np.full(8, 0x5A5A5A5A, U32))
    ctx.topk_rows(keys, 0, out_values=guard[:0], out_indices=guard[4:4])
    assert np.all(bits(guard) == U32(0x5A5A5A5A))


# ---- launches ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,k", [(1000, 8), (8193, 1024), (65537, 1024)])
def test_one_tile_sort_launch_per_pass(ctx, cols, k):
    keys, order = data("random", 3, cols, True)
    dk = to_dev(keys)
    ctx.topk_rows(dk, k)  # scratch growth out of the way
    torch.cuda.synchronize()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        vals, idx = ctx.topk_rows(dk, k)
        torch.cuda.synchronize()
        got = {name: v[0] for name, v in ctx.profile_read().items() if v[0]}
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert got == {"tile_sort": len(misort.topk_plan(cols, k))}
    np.testing.assert_array_equal(bits(idx), order[:, :k])


# ---- stream order --------------------------------------------------------------------------------------

STREAM_SHAPES = [(64, 1000, 8), (3, 65537, 1024)]


@functools.lru_cache(maxsize=None)
def stream_case(rows, cols, k, largest, salt=0):
    keys = SO.tied_u32(900 + salt + cols, (rows, cols)) | U32(1)  # never the poison
    wk, wi = TO.topk_rows(keys, k, largest)
    stage = {"keys": In(keys), "vals": Out((rows, k), U32), "idx": Out((rows, k), U32)}
    return stage, {"keys": keys, "vals": wk, "idx": wi}


def run_topk(c, stream, rows, cols, k, largest, mode, salt=0, pending=True):
    """The call behind a producer pending on ``stream`` (or, ``pending=False``,
    behind nothing but the copies of its inputs)."""
    stage, expect = stream_case(rows, cols, k, largest, salt)
    handle = None if mode == "current" else stream.cuda_stream

    def call(t):
        c.topk_rows(t["keys"], k, largest=largest, out_values=t["vals"], out_indices=t["idx"], stream=handle)
    res = SO.behind_pending_work(stream, stage, call, ms=SO.PRODUCER_MS if pending else 0.01,
                                 current="stream" if mode == "current" else "elsewhere")
    SO.compare(res, expect, f"topk_rows {rows}x{cols} k={k} ({mode})")
    return res


@DIRECTIONS
@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("rows,cols,k", STREAM_SHAPES)
def test_behind_pending_work_on_a_warm_context(ctx, side, rows, cols, k, mode, largest):
    run_topk(ctx, side, rows, cols, k, largest, mode, salt=SO.WARM_SALT, pending=False)  # other data: grows the scratch
    res = run_topk(ctx, side, rows, cols, k, largest, mode)
    assert res.not_ready, SO.lost_sensitivity(res)


@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("rows,cols,k", STREAM_SHAPES)
def test_behind_pending_work_on_a_fresh_context(side, rows, cols, k, mode):
    """The scratch grows behind queued work, which may wait: the results only."""
    c = misort.Context(0)
    try:
        run_topk(c, side, rows, cols, k, True, mode)
    finally:
        c.close()


def test_two_calls_chained_with_no_host_wait(ctx, side):
    """The second call reads another input and reuses the candidates' scratch
    while the first may still be running: both exact."""
    shapes = [(3, 65537, 1024, True), (5, 40001, 100, False)]
    cases = [stream_case(*s, salt=77) for s in shapes]
    stage = {f"{name}{i}": b for i, (st, _) in enumerate(cases) for name, b in st.items()}
    expect = {f"{name}{i}": w for i, (_, ex) in enumerate(cases) for name, w in ex.items()}

    def call(t):
        for i, (_, _, k, largest) in enumerate(shapes):
            ctx.topk_rows(t[f"keys{i}"], k, largest=largest, out_values=t[f"vals{i}"], out_indices=t[f"idx{i}"],
                          stream=side.cuda_stream)
    call_warm = SO.behind_pending_work(side, stage, call, ms=0.01)  # grows the scratch
    SO.compare(call_warm, expect, "chained (warm-up)")
    res = SO.behind_pending_work(side, stage, call)
    SO.compare(res, expect, "chained")
    assert res.not_ready, SO.lost_sensitivity(res)


# ---- against torch on the device ------------------------------------------------------------------------

@DIRECTIONS
@pytest.mark.parametrize("rows,cols,k", [(64, 1000, 8), (3, 65537, 64)])
def test_against_torch_topk_on_distinct_floats(ctx, rows, cols, k, largest):
    """Finite float32 keys without ties: the values are torch.topk's and the
    indices gather them."""
    g = torch.Generator(device="cpu").manual_seed(cols + k)
    perm = torch.stack([torch.randperm(cols, generator=g) for _ in range(rows)])
    keys = ((perm - cols // 2).to(torch.float32) * 0.37).cuda()  # distinct: |perm| < 2^24
    vals, idx = ctx.topk_rows(keys, k, largest=largest)
    ref = torch.topk(keys, k, dim=-1, largest=largest, sorted=True)
    torch.cuda.synchronize()
    assert torch.equal(vals, ref.values)
    assert torch.equal(keys.gather(-1, idx.long()), vals)
    assert torch.equal(idx.long(), ref.indices)
