"""Key-value sort and argsort on one GPU (misort_local_sort_pairs) against numpy
on the host: pairs by np.lexsort((values, K(keys))), the argsort by the stable
np.argsort(K(keys)), K the order-preserving u32 pattern of a key.  Every
comparison is on bit patterns; there is no tolerance."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from sort_oracles import argsort_oracle, pairs_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

U32_T = torch.uint32 if hasattr(torch, "uint32") else torch.int32

# 0..5: the four-pair vector body and its tail; 1023..1025: one block of 256
# lanes x 4; 8191..8193: the u64 SORT tile; 131073: the first multi-way pass;
# 2^20 + 12345: a short last group in a multi-way pass
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 131073, (1 << 20) + 12345]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(U32_T)
    return torch.from_numpy(a).cuda()


def bits(t):
    """The 32-bit patterns of a device tensor (u32 storage or float32), on the host."""
    torch.cuda.synchronize()
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def tied_keys(rng, n):
    """Random u32 keys, a third of them from 16 values (ties the values order)."""
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k[rng.random(n) < 1 / 3] &= np.uint32(0xF)
    return k


def rand_u32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def f32_mix(rng, n):
    """Normal values of both signs, +-0.0, +-inf, denormals and NaNs of both signs."""
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # denormals
                        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF],  # NaNs
                       dtype=np.uint32)
    k = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32).view(np.uint32)
    pick = rng.random(n) < 0.25
    k[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    return k.view(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_sort_pairs_u32(ctx, n):
    rng = np.random.default_rng(1000 + n)
    keys, vals = tied_keys(rng, n), rand_u32(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = ctx.sort_pairs(dk, dv)
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(dk), keys)  # inputs untouched
    np.testing.assert_array_equal(bits(dv), vals)


ARGSORT_KEYS = {
    "dups": lambda rng, n: rng.integers(0, 5, n).astype(np.uint32),  # stability is the whole test
    "equal": lambda rng, n: np.full(n, 0xDEADBEEF, np.uint32),
    "ascending": lambda rng, n: np.arange(n, dtype=np.uint32),
    "descending": lambda rng, n: np.arange(n, 0, -1).astype(np.uint32),
}


@pytest.mark.parametrize("kind", sorted(ARGSORT_KEYS))
@pytest.mark.parametrize("n", SIZES)
def test_argsort_is_stable(ctx, n, kind):
    keys = ARGSORT_KEYS[kind](np.random.default_rng(2000 + n), n)
    dk = to_dev(keys)
    idx = ctx.argsort(dk)
    assert idx.numel() == n
    np.testing.assert_array_equal(bits(idx), argsort_oracle(keys))
    np.testing.assert_array_equal(bits(dk), keys)


def test_sentinel_collision(ctx):
    # key 0xFFFFFFFF with value 0xFFFFFFFF is the all-ones record the sort pads with
    n = 8193
    rng = np.random.default_rng(3)
    keys, vals = rand_u32(rng, n), rand_u32(rng, n)
    keys[: n // 3] = vals[: n // 3] = 0xFFFFFFFF
    keys[n // 3: 2 * (n // 3)] = vals[n // 3: 2 * (n // 3)] = 0
    perm = rng.permutation(n)
    keys, vals = keys[perm], vals[perm]
    ok, ov = ctx.sort_pairs(to_dev(keys), to_dev(vals))
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)


@pytest.mark.parametrize("n", [1025, 131073])
def test_sort_pairs_f32(ctx, n):
    rng = np.random.default_rng(4000 + n)
    keys, vals = f32_mix(rng, n), rand_u32(rng, n)
    vals[rng.random(n) < 0.5] &= np.uint32(3)  # equal keys meet equal and unequal values
    kb = keys.view(np.uint32)
    for pattern in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000001, 0x80000001):
        assert (kb == pattern).any()
    dk = to_dev(keys)
    assert dk.dtype == torch.float32
    ok, ov = ctx.sort_pairs(dk, to_dev(vals))
    assert ok.dtype == torch.float32
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)  # every key bit-exact, NaN payloads included
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(dk), kb)
    idx = ctx.argsort(dk)
    np.testing.assert_array_equal(bits(idx), argsort_oracle(keys))
    # the documented order: negative NaNs first, -0.0 before +0.0, positive NaNs last
    assert np.isnan(wk.view(np.float32)[0]) and wk[0] >> 31 == 1
    assert np.isnan(wk.view(np.float32)[-1]) and wk[-1] >> 31 == 0
    z = np.flatnonzero((wk & 0x7FFFFFFF) == 0)
    assert (np.diff(wk[z].astype(np.int64)) <= 0).all()


GUARD = 0xA5A5A5A5


def offset_view(n, off, fill=None):
    """(base, view): a view of n elements starting `off` elements into a base
    tensor that keeps guard elements on both sides."""
    base = to_dev(np.full(n + 8, GUARD, np.uint32) if fill is None else
                  np.concatenate([np.full(off, GUARD, np.uint32), fill, np.full(8 - off, GUARD, np.uint32)]))
    assert base.data_ptr() % 16 == 0
    return base, base[off: off + n]


def guards_intact(base, n, off):
    b = bits(base)
    return (b[:off] == GUARD).all() and (b[off + n:] == GUARD).all()


@pytest.mark.parametrize("in_off,out_off", [((1, 3), (1, 2)), ((0, 0), (1, 2)), ((1, 3), (0, 0)), ((0, 2), (4, 0))])
def test_misaligned_pointers(ctx, in_off, out_off):
    # offsets in elements: 0 and 4 keep the 16-byte alignment (vector kernel),
    # 1, 2 and 3 do not (the 4-byte variant of the same kernel)
    n = 4099
    rng = np.random.default_rng(5)
    keys, vals = tied_keys(rng, n), rand_u32(rng, n)
    kb, dk = offset_view(n, in_off[0], keys)
    vb, dv = offset_view(n, in_off[1], vals)
    okb, ok = offset_view(n, out_off[0])
    ovb, ov = offset_view(n, out_off[1])
    for t, off in ((dk, in_off[0]), (dv, in_off[1]), (ok, out_off[0]), (ov, out_off[1])):
        assert t.data_ptr() % 16 == 4 * off % 16
    ctx.sort_pairs(dk, dv, out_keys=ok, out_values=ov)
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(bits(dv), vals)
    assert guards_intact(okb, n, out_off[0]) and guards_intact(ovb, n, out_off[1])
    assert guards_intact(kb, n, in_off[0]) and guards_intact(vb, n, in_off[1])
    # the argsort through a misaligned output
    ib, idx = offset_view(n, out_off[0])
    ctx.argsort(dk, out=idx)
    np.testing.assert_array_equal(bits(idx), argsort_oracle(keys))
    assert guards_intact(ib, n, out_off[0])


def test_outputs_alias_inputs(ctx):
    n = 131073
    rng = np.random.default_rng(6)
    keys, vals = tied_keys(rng, n), rand_u32(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = ctx.sort_pairs(dk, dv, out_keys=dk, out_values=dv)
    assert ok is dk and ov is dv
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(dk), wk)
    np.testing.assert_array_equal(bits(dv), wv)


def test_values_only_through_the_c_entry_point(ctx):
    n = 8193
    rng = np.random.default_rng(7)
    keys, vals = tied_keys(rng, n), rand_u32(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ov = torch.empty_like(dv)
    torch.cuda.synchronize()
    rc = misort.lib().misort_local_sort_pairs(ctx._h, misort.U32, dk.data_ptr(), dv.data_ptr(), None, ov.data_ptr(),
                                              n, ctx.native_stream)
    assert rc == 0
    ctx.synchronize()
    np.testing.assert_array_equal(bits(ov), pairs_oracle(keys, vals)[1])
    np.testing.assert_array_equal(bits(dk), keys)  # no key is written anywhere
    np.testing.assert_array_equal(bits(dv), vals)


def test_on_the_contexts_stream(ctx):
    n = 131073
    rng = np.random.default_rng(8)
    keys, vals = tied_keys(rng, n), rand_u32(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = torch.empty_like(dk), torch.empty_like(dv)
    idx = torch.empty_like(dv)
    torch.cuda.synchronize()
    ctx.sort_pairs(dk, dv, out_keys=ok, out_values=ov, stream=ctx.native_stream)
    ctx.argsort(dk, out=idx, stream=ctx.native_stream)
    ctx.synchronize()
    wk, wv = pairs_oracle(keys, vals)
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    np.testing.assert_array_equal(bits(idx), argsort_oracle(keys))


def test_profile_records_the_streaming_kernels_as_other(ctx):
    n = 8193
    rng = np.random.default_rng(9)
    dk, dv = to_dev(tied_keys(rng, n)), to_dev(rand_u32(rng, n))
    names = list(misort.KIND_NAMES)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        ctx.sort_pairs(dk, dv)
        torch.cuda.synchronize()
        launches, ms, nbytes = ctx.profile_read()["other"]
        assert launches == 2 and ms > 0.0  # zip_pairs and unzip_pairs
        assert nbytes == 2 * 16 * n  # 16 bytes moved per pair, each way
        ctx.profile_reset()
        ctx.argsort(dk)
        torch.cuda.synchronize()
        launches, ms, nbytes = ctx.profile_read()["other"]
        assert launches == 2 and nbytes == 2 * 12 * n  # no values read, no keys written
    finally:
        ctx.profile(False)
    assert misort.KIND_NAMES == names and len(names) == 12


def test_wrong_key_dtype(ctx):
    k64 = torch.zeros(16, dtype=torch.float64, device="cuda")
    v = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ctx.sort_pairs(k64, v)
    with pytest.raises(TypeError):
        ctx.argsort(k64)
    with pytest.raises(TypeError):
        ctx.argsort(torch.zeros(16, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        ctx.sort_pairs(v, k64)  # values are 32-bit integers


def test_c_entry_point_rejects_other_dtypes_and_bad_arguments(ctx):
    L = misort.lib()
    k = torch.zeros(16, dtype=torch.int64, device="cuda")
    v = torch.zeros(16, dtype=torch.int32, device="cuda")
    p, q, s = k.data_ptr(), v.data_ptr(), ctx.native_stream
    for dt in (misort.U64, misort.F64, 4, -1):
        assert L.misort_local_sort_pairs(ctx._h, dt, p, q, p, q, 16, s) == -1
        assert L.misort_parallel_sort_pairs(ctx._h, dt, p, q, p, q, 16, 0, s) == -1
    assert L.misort_local_sort_pairs(ctx._h, misort.U32, p, q, p, q, -1, s) == -1
    assert L.misort_local_sort_pairs(ctx._h, misort.U32, None, q, p, q, 16, s) == -1  # no keys
    assert L.misort_local_sort_pairs(ctx._h, misort.U32, p, q, p, None, 16, s) == -1  # no value output
    assert L.misort_local_sort_pairs(ctx._h, misort.U32, p, None, None, q, (1 << 32) + 1, s) == -1  # indices
    assert L.misort_local_sort_pairs(ctx._h, misort.U32, None, None, None, None, 0, s) == 0  # nothing to do
    # MISORT_F32 stays a key type of the pair sorts alone
    assert L.misort_local_sort(ctx._h, misort.F32, q, q, 16, s) == -1
    ctx.synchronize()
    assert not v.view(torch.int32).cpu().numpy().any()
