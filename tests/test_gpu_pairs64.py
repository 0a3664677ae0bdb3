"""Stable key-value sort and argsort of 64-bit keys on one GPU
(misort_local_sort_pairs64) against numpy on the host: order =
np.argsort(K(keys), kind="stable"), K the order-preserving u64 pattern of a
key; expected keys[order], vals[order] and order as u32.  Every comparison is
on bit patterns; there is no tolerance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from sort_oracles import order_of  # noqa: E402

pytestmark = pytest.mark.gpu

# the shapes of test_gpu_pairs.py: 0..5: the four-element vector body and its
# tail; 1023..1025: one block of 256 lanes x 4; 8191..8193: the u64 SORT tile;
# 131073: the first multi-way pass; 2^20 + 12345: a short last group in one
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 131073, (1 << 20) + 12345]
U64 = np.uint64
ONES = U64(0xFFFFFFFFFFFFFFFF)


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


def rand_u32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def rand_half(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64)


def rand_u64(rng, n):
    return rand_half(rng, n) << U64(32) | rand_half(rng, n)


def few_few(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint64) << U64(32) | rng.integers(0, 4, n, dtype=np.uint64)


def sentinels(rng, n):
    k = rand_u64(rng, n)
    k[: n // 3] = ONES  # the pattern the sort pads with
    k[n // 3: 2 * (n // 3)] = 0
    return k[rng.permutation(n)]


# each family targets one way the two-pass composition can go wrong
KEYS = {
    "lo_only": lambda rng, n: rand_half(rng, n),  # pass 2 is all ties: the order comes from j alone
    "hi_only": lambda rng, n: rand_half(rng, n) << U64(32),  # pass 1 is all ties
    "few_few": few_few,  # heavy duplicates in both halves: stability is the whole test
    "opposed": lambda rng, n: np.arange(n, dtype=U64) << U64(32) | (U64(n) - np.arange(n, dtype=U64)),
    "equal": lambda rng, n: np.full(n, 0xDEADBEEFCAFEF00D, U64),
    "ascending": lambda rng, n: np.arange(n, dtype=U64) << U64(16),
    "descending": lambda rng, n: np.arange(n, 0, -1).astype(U64) << U64(16),
    "random": rand_u64,
    "sentinels": sentinels,
}


@pytest.mark.parametrize("kind", sorted(KEYS))
@pytest.mark.parametrize("n", SIZES)
def test_argsort64_u64(ctx, n, kind):
    keys = KEYS[kind](np.random.default_rng(6400 + n), n)
    assert keys.dtype == np.uint64 and keys.size == n
    dk = to_dev(keys)
    idx = ctx.argsort64(dk)
    assert idx.numel() == n and idx.dtype == torch.int32
    np.testing.assert_array_equal(bits(idx), order_of(keys).astype(np.uint32))
    np.testing.assert_array_equal(bits(dk), keys)  # input untouched


F64_SPECIAL = np.array([
    0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,  # +-0, +-inf
    0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,  # denormals
    0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,  # NaNs, varied payloads
    0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FF800000000BEEF, 0xFFF00000DEAD0000], dtype=np.uint64)


def f64_mix(rng, n):
    """Normal values of both signs, +-0.0, +-inf, denormals and NaNs of both signs."""
    k = (rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)).view(np.uint64)
    pick = rng.random(n) < 0.25
    k[pick] = F64_SPECIAL[rng.integers(0, F64_SPECIAL.size, int(pick.sum()))]
    return k.view(np.float64)


@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("n", [1025, 131073])
def test_f64_keys(ctx, n, vb):
    rng = np.random.default_rng(6500 + n)
    keys = f64_mix(rng, n)
    vals = rand_u32(rng, n) if vb == 4 else rand_u64(rng, n)
    kb = keys.view(np.uint64)
    for pattern in F64_SPECIAL:
        assert (kb == pattern).any()
    assert np.isfinite(keys).any() and (keys > 0).any() and (keys < 0).any()
    dk, dv = to_dev(keys), to_dev(vals)
    assert dk.dtype == torch.float64
    order = order_of(keys)
    idx = ctx.argsort64(dk)
    np.testing.assert_array_equal(bits(idx), order.astype(np.uint32))
    ok, ov = ctx.sort_pairs64(dk, dv)
    assert ok.dtype == torch.float64 and ov.dtype == dv.dtype
    wk = kb[order]
    np.testing.assert_array_equal(bits(ok), wk)  # every key bit-exact, NaN payloads included
    np.testing.assert_array_equal(bits(ov), vals[order])
    np.testing.assert_array_equal(bits(dk), kb)  # inputs untouched
    np.testing.assert_array_equal(bits(dv), vals)
    # the documented order: negative NaNs first, -0.0 before +0.0, positive NaNs last
    got = bits(ok)
    assert np.isnan(got.view(np.float64)[0]) and got[0] >> U64(63) == 1
    assert np.isnan(got.view(np.float64)[-1]) and got[-1] >> U64(63) == 0
    z = np.flatnonzero((got & U64(0x7FFFFFFFFFFFFFFF)) == 0)
    assert z.size >= 2 and (np.diff(z) == 1).all()
    signs = got[z] >> U64(63)
    assert signs[0] == 1 and signs[-1] == 0 and (np.diff(signs.astype(np.int64)) <= 0).all()


@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_sort_pairs64_values_in_stable_order(ctx, n, vb):
    rng = np.random.default_rng(6600 + n)
    keys = few_few(rng, n)
    vals = rand_u32(rng, n) if vb == 4 else rand_u64(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = ctx.sort_pairs64(dk, dv)
    order = order_of(keys)
    np.testing.assert_array_equal(bits(ok), keys[order])
    np.testing.assert_array_equal(bits(ov), vals[order])  # input order within a key, not value order
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(bits(dv), vals)


@pytest.mark.parametrize("vb", [4, 8])
def test_equal_keys_with_descending_values(ctx, vb):
    n = 8193
    keys = few_few(np.random.default_rng(67), n)
    vals = np.arange(n, 0, -1).astype(np.uint32 if vb == 4 else np.uint64)
    order = order_of(keys)
    want = vals[order]
    by_value = vals[np.lexsort((vals, keys))]  # the 32-bit entry point's (key, value) order
    assert not np.array_equal(want, by_value)
    ok, ov = ctx.sort_pairs64(to_dev(keys), to_dev(vals))
    np.testing.assert_array_equal(bits(ok), keys[order])
    np.testing.assert_array_equal(bits(ov), want)


GUARD = {8: U64(0xA5A5A5A5A5A5A5A5), 4: np.uint32(0xA5A5A5A5)}


def offset_view(n, width, fill=None):
    """(base, view): n elements of `width` bytes starting ONE element into a
    16-byte-aligned base tensor that keeps guard elements on both sides."""
    dt = np.uint64 if width == 8 else np.uint32
    g = GUARD[width]
    base = to_dev(np.full(n + 8, g, dt) if fill is None else
                  np.concatenate([np.full(1, g, dt), fill.view(dt), np.full(7, g, dt)]))
    assert base.data_ptr() % 16 == 0
    view = base[1: 1 + n]
    assert view.data_ptr() % 16 == width
    return base, view


def guards_intact(base, n):
    b = bits(base)
    g = GUARD[base.element_size()]
    return (b[:1] == g).all() and (b[1 + n:] == g).all()


@pytest.mark.parametrize("vb", [4, 8])
def test_element_aligned_views(ctx, vb):
    n = 4099
    rng = np.random.default_rng(68)
    keys = few_few(rng, n) | (rand_half(rng, n) & U64(0x30000))
    vals = rand_u32(rng, n) if vb == 4 else rand_u64(rng, n)
    kb, dk = offset_view(n, 8, keys)
    vbase, dv = offset_view(n, vb, vals)
    okb, ok = offset_view(n, 8)
    ovb, ov = offset_view(n, vb)
    ctx.sort_pairs64(dk, dv, out_keys=ok, out_values=ov)
    order = order_of(keys)
    np.testing.assert_array_equal(bits(ok), keys[order])
    np.testing.assert_array_equal(bits(ov), vals[order])
    np.testing.assert_array_equal(bits(dk), keys)
    np.testing.assert_array_equal(bits(dv), vals)
    for b in (kb, vbase, okb, ovb):
        assert guards_intact(b, n)
    ib, idx = offset_view(n, 4)
    ctx.argsort64(dk, out=idx)
    np.testing.assert_array_equal(bits(idx), order.astype(np.uint32))
    assert guards_intact(ib, n) and guards_intact(kb, n)
    np.testing.assert_array_equal(bits(dk), keys)


def test_out_keys_is_keys(ctx):
    n = 131073
    rng = np.random.default_rng(69)
    keys, vals = few_few(rng, n) | (rand_half(rng, n) & U64(0x70000)), rand_u64(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = ctx.sort_pairs64(dk, dv, out_keys=dk)
    assert ok is dk
    order = order_of(keys)
    np.testing.assert_array_equal(bits(dk), keys[order])
    np.testing.assert_array_equal(bits(ov), vals[order])
    np.testing.assert_array_equal(bits(dv), vals)


def test_overlapping_arguments_are_refused(ctx):
    n = 4096
    rng = np.random.default_rng(70)
    keys, vals = rand_u64(rng, n), rand_u64(rng, n + 1)
    dk, base = to_dev(keys), to_dev(vals)
    dv, shifted = base[:n], base[1:]
    spare = torch.zeros(n, dtype=torch.int64, device="cuda")
    cases = {
        "out_values is values": dict(out_keys=spare, out_values=dv),
        "out_values overlaps values, shifted": dict(out_keys=spare, out_values=shifted),
        "out_keys overlaps values": dict(out_keys=shifted, out_values=spare),
        "out_keys overlaps out_values": dict(out_keys=spare, out_values=spare),
    }
    for what, kw in cases.items():
        with pytest.raises(misort.MisortError) as e:
            ctx.sort_pairs64(dk, dv, **kw)
        assert e.value.code == -1, what
        ctx.synchronize()
        np.testing.assert_array_equal(bits(dk), keys, err_msg=what)
        np.testing.assert_array_equal(bits(base), vals, err_msg=what)
        assert not bits(spare).any(), what
    # 4-byte values: the ranges are measured in the values' own width
    v4 = to_dev(rand_u32(rng, n + 1))
    with pytest.raises(misort.MisortError) as e:
        ctx.sort_pairs64(dk, v4[:n], out_keys=spare, out_values=v4[1:])
    assert e.value.code == -1


def test_values_only_through_the_c_entry_point(ctx):
    n = 8193
    rng = np.random.default_rng(71)
    keys, vals = few_few(rng, n), rand_u32(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ov = torch.empty_like(dv)
    torch.cuda.synchronize()
    rc = misort.lib().misort_local_sort_pairs64(ctx._h, misort.U64, dk.data_ptr(), dv.data_ptr(), 4, None,
                                                ov.data_ptr(), n, ctx.native_stream)
    assert rc == 0
    ctx.synchronize()
    np.testing.assert_array_equal(bits(ov), vals[order_of(keys)])
    np.testing.assert_array_equal(bits(dk), keys)  # no key is written anywhere
    np.testing.assert_array_equal(bits(dv), vals)


def test_on_the_contexts_stream(ctx):
    n = 131073
    rng = np.random.default_rng(72)
    keys, vals = rand_u64(rng, n) & U64(0xFF000000FF), rand_u64(rng, n)
    dk, dv = to_dev(keys), to_dev(vals)
    ok, ov = torch.empty_like(dk), torch.empty_like(dv)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sort_pairs64(dk, dv, out_keys=ok, out_values=ov, stream=ctx.native_stream)
    ctx.argsort64(dk, out=idx, stream=ctx.native_stream)
    ctx.synchronize()
    order = order_of(keys)
    np.testing.assert_array_equal(bits(ok), keys[order])
    np.testing.assert_array_equal(bits(ov), vals[order])
    np.testing.assert_array_equal(bits(idx), order.astype(np.uint32))


def test_profile_records_three_other_launches(ctx):
    n = 8193
    rng = np.random.default_rng(73)
    dk, dv = to_dev(rand_u64(rng, n)), to_dev(rand_u64(rng, n))
    names = list(misort.KIND_NAMES)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        ctx.argsort64(dk)
        torch.cuda.synchronize()
        launches, ms, nbytes = ctx.profile_read()["other"]
        assert launches == 3 and ms > 0.0  # zip_lo, gather_hi, emit
        assert nbytes == 16 * n + 24 * n + (16 * n + 4 * n)
        ctx.profile_reset()
        ctx.sort_pairs64(dk, dv)
        torch.cuda.synchronize()
        launches, ms, nbytes = ctx.profile_read()["other"]
        assert launches == 3
        assert nbytes == 16 * n + 24 * n + (16 * n + 8 * n + 16 * n)  # keys written, values read and written
    finally:
        ctx.profile(False)
    assert misort.KIND_NAMES == names and len(names) == 12


def test_c_entry_point_rejects_bad_arguments(ctx):
    f = misort.lib().misort_local_sort_pairs64
    k = torch.zeros(16, dtype=torch.int64, device="cuda")
    v = torch.zeros(16, dtype=torch.int64, device="cuda")
    ko, vo = torch.zeros_like(k), torch.zeros_like(v)
    p, q, po, qo, s = k.data_ptr(), v.data_ptr(), ko.data_ptr(), vo.data_ptr(), ctx.native_stream
    for dt in (misort.U32, misort.F32, 4, -1):
        assert f(ctx._h, dt, p, q, 8, po, qo, 16, s) == -1
    for vb in (0, 2, 16):
        assert f(ctx._h, misort.U64, p, q, vb, po, qo, 16, s) == -1
    assert f(ctx._h, misort.U64, p, None, 8, po, qo, 16, s) == -1  # indices are 4 bytes
    assert f(ctx._h, misort.U64, p, q, 8, po, qo, -1, s) == -1
    assert f(ctx._h, misort.U64, p, None, 4, None, qo, (1 << 32) + 1, s) == -1  # a 32-bit tag holds 2^32 indices
    assert f(ctx._h, misort.F64, None, q, 8, po, qo, 16, s) == -1  # no keys
    assert f(ctx._h, misort.F64, p, q, 8, po, None, 16, s) == -1  # no value output
    assert misort.lib().misort_last_error()
    assert f(ctx._h, misort.U64, None, None, 4, None, None, 0, s) == 0  # nothing to do
    assert f(ctx._h, misort.F64, None, None, 8, None, None, 0, s) == 0
    ctx.synchronize()
    for t in (k, v, ko, vo):
        assert not bits(t).any()


def test_wrong_dtypes_raise_type_error(ctx):
    v = torch.zeros(16, dtype=torch.int32, device="cuda")
    k64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    for bad in (torch.zeros(16, dtype=torch.float32, device="cuda"), v):
        with pytest.raises(TypeError):
            ctx.sort_pairs64(bad, v)
        with pytest.raises(TypeError):
            ctx.argsort64(bad)
    with pytest.raises(TypeError):
        ctx.sort_pairs64(k64, torch.zeros(16, dtype=torch.int16, device="cuda"))  # 2-byte values
