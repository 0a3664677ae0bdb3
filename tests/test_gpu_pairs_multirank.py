"""The key-value sort over P ranks (misort_parallel_sort_pairs), P ranks as
threads of one process on one GPU (misort.Group): the concatenated rank outputs
against numpy's lexsort / stable argsort of the concatenated inputs, bit for
bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

U32_T = torch.uint32 if hasattr(torch, "uint32") else torch.int32


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(U32_T)
    return torch.from_numpy(a).cuda()


def bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def kmap(keys):
    if keys.dtype == np.float32:
        b = keys.view(np.uint32)
        return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return keys


def group_pairs(keys, vals, p, setup=None):
    """Sorts the pairs over p ranks (equal blocks; vals None = global indices);
    returns the concatenated (key bits, values)."""
    loc = keys.size // p
    assert loc * p == keys.size

    def rank_fn(r, ctx):
        if setup:
            setup(ctx)
        k = np.ascontiguousarray(keys[r * loc:(r + 1) * loc])
        dk = to_dev(k)
        dv = None if vals is None else to_dev(vals[r * loc:(r + 1) * loc])
        torch.cuda.synchronize()
        ok, ov = ctx.parallel_sort_pairs(dk, dv, loc, stream=ctx.native_stream)
        ctx.synchronize()
        np.testing.assert_array_equal(bits(dk), k.view(np.uint32))  # input untouched
        return bits(ok), bits(ov)

    g = misort.Group(p)
    try:
        res = g.run(rank_fn)
    finally:
        g.close()
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def dup_keys(rng, n):
    """Duplicate-heavy u32 keys: half from five values, half from the whole range."""
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    few = rng.random(n) < 0.5
    k[few] = rng.integers(0, 5, int(few.sum())).astype(np.uint32) * np.uint32(0x33333333)
    return k


def rand_u32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def check_pairs(keys, vals, p, setup=None):
    gk, gv = group_pairs(keys, vals, p, setup)
    order = np.lexsort((vals, kmap(keys)))
    np.testing.assert_array_equal(gk, keys.view(np.uint32)[order])
    np.testing.assert_array_equal(gv, vals[order])


def check_argsort(keys, p, setup=None):
    gk, gv = group_pairs(keys, None, p, setup)
    order = np.argsort(kmap(keys), kind="stable")
    np.testing.assert_array_equal(gv, order.astype(np.uint32))  # global indices, equal keys in input order
    np.testing.assert_array_equal(gk, keys.view(np.uint32)[order])


@pytest.mark.parametrize("loc", [1000, 8193, 1 << 16])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_parallel_sort_pairs(p, loc):
    rng = np.random.default_rng(100 * p + loc)
    check_pairs(dup_keys(rng, p * loc), rand_u32(rng, p * loc), p)


@pytest.mark.parametrize("loc", [1000, 8193, 1 << 16])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_parallel_argsort(p, loc):
    check_argsort(dup_keys(np.random.default_rng(200 * p + loc), p * loc), p)


def test_parallel_sort_pairs_f32():
    p, loc = 4, 8193
    rng = np.random.default_rng(31)
    k = (rng.standard_normal(p * loc) * 10.0 ** rng.integers(-30, 30, p * loc)).astype(np.float32).view(np.uint32)
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 1, 0x80000001, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF],
                       dtype=np.uint32)
    pick = rng.random(p * loc) < 0.3
    k[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    keys = k.view(np.float32)
    check_pairs(keys, rand_u32(rng, p * loc) & np.uint32(7), p)
    check_argsort(keys, p)


@pytest.mark.parametrize("mode", ["no_compress", "full_exchange"])
def test_exchange_modes_give_the_same_pairs(mode):
    p, loc = 4, 8193
    rng = np.random.default_rng(41)
    setup = {"no_compress": lambda c: c.set_compress(False), "full_exchange": lambda c: c.set_full_exchange(True)}[mode]
    check_pairs(dup_keys(rng, p * loc), rand_u32(rng, p * loc), p, setup)


def test_unequal_blocks_fail_on_every_rank():
    loc = 1000

    def rank_fn(r, ctx):
        n = loc - 1 if r == 0 else loc
        dk = to_dev(np.arange(n, dtype=np.uint32))
        with pytest.raises(misort.MisortError) as e:
            ctx.parallel_sort_pairs(dk, None, n, stream=ctx.native_stream)
        return e.value.code

    g = misort.Group(2)
    try:
        assert g.run(rank_fn) == [-1, -1]  # found before the first exchange: nothing waits
    finally:
        g.close()


def test_one_rank_equals_sort_pairs():
    n = 8193
    rng = np.random.default_rng(51)
    keys, vals = dup_keys(rng, n), rand_u32(rng, n)
    ctx = misort.Context(0)
    try:
        dk, dv = to_dev(keys), to_dev(vals)
        pk, pv = ctx.parallel_sort_pairs(dk, dv)
        lk, lv = ctx.sort_pairs(dk, dv)
        pi = ctx.parallel_sort_pairs(dk)[1]
        li = ctx.argsort(dk)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(pk), bits(lk))
        np.testing.assert_array_equal(bits(pv), bits(lv))
        np.testing.assert_array_equal(bits(pi), bits(li))
        order = np.lexsort((vals, keys))
        np.testing.assert_array_equal(bits(lk), keys[order])
        np.testing.assert_array_equal(bits(lv), vals[order])
    finally:
        ctx.close()
