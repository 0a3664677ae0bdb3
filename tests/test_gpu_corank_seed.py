"""Whole local sorts over the seeded in-LDS co-rank searches (csrc/lds_merge.h,
corank_seed.h): keys that suit the seed (iid) and keys that defeat it (sorted,
reversed, ties, structured), so that both the seeded search and the wave's
sticky fallback to the full search run in the multi-way chunks and in the u32
tile's merge levels.  ctx.local_sort must equal np.sort bit for bit.

Sizes: u32 2^18 + 3 (an 8-way and a 4-way pass over 2^14-key tiles, a partial
last group), 2^22 + 5 (three 8-way passes) and 2^21 + 5 (two 16-way passes:
the chunk shape of the 2^30 sort); u64 and f64 2^17 + 3 (8-way, 4-way) and
2^21 (two 16-way passes)."""
import functools

import numpy as np
import pytest

import tile_battery as B

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

U32_T = torch.uint32 if hasattr(torch, "uint32") else torch.int32
U64_T = torch.uint64 if hasattr(torch, "uint64") else torch.int64
FAMILIES = ("iid", "ascending", "descending", "constant", "two_values", "sawtooth", "battery")
SIZES = [("u32", (1 << 18) + 3), ("u32", (1 << 22) + 5), ("u32", (1 << 21) + 5), ("u64", (1 << 17) + 3), ("u64", 1 << 21),
         ("f64", (1 << 17) + 3), ("f64", 1 << 21)]
NP_T = {"u32": np.uint32, "u64": np.uint64, "f64": np.float64}


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(a):
    a = np.array(a)  # a writable copy: the shared inputs are read-only
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(U32_T)
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda().view(U64_T)
    return torch.from_numpy(a).cuda()


def to_host(t, dtype):
    torch.cuda.synchronize()
    if np.dtype(dtype) == np.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if np.dtype(dtype) == np.uint64:
        return t.view(torch.int64).cpu().numpy().view(np.uint64)
    return t.cpu().numpy()


def keys(family, dt, n):
    """n keys of the family as integers (u32 / u64); f64 takes them as values
    (no NaN, no -0: np.sort's order is the only one)."""
    it = np.uint32 if dt == "u32" else np.uint64
    mx = int(np.iinfo(it).max)
    rng = np.random.default_rng([n & 0xFFFFFFFF, len(family), 8 if dt != "u32" else 4])
    i = np.arange(n, dtype=np.uint64)
    if family == "iid":
        x = rng.integers(0, mx, size=n, dtype=it, endpoint=True)
    elif family == "ascending":
        x = (i * np.uint64(mx // n)).astype(it)
    elif family == "descending":
        x = (i[::-1] * np.uint64(mx // n)).astype(it)
    elif family == "constant":
        x = np.full(n, 0x5A5A5A5A, dtype=it)
    elif family == "two_values":
        x = np.where(rng.integers(0, 2, size=n) == 1, it(mx - 1), it(7)).astype(it)
    elif family == "sawtooth":
        x = (i % np.uint64((1 << 14) + 1)).astype(it)
    else:  # the SORT-tile battery's tiles one after the other, cut at n
        T = 1 << (14 if dt == "u32" else 13)
        x = B.compose(B.cycle(T, it, 3, -(-n // T)))[:n]
    if dt == "f64":
        x = x.astype(np.float64)  # values, rounded: more ties
        assert not np.any(np.isnan(x))
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def case(family, dt, n):
    x = keys(family, dt, n)
    want = np.sort(x)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dt,n", SIZES, ids=[f"{d}-{n}" for d, n in SIZES])
def test_local_sort_matches_np_sort(ctx, dt, n, family):
    x, want = case(family, dt, n)
    d = to_dev(x)
    out = to_dev(np.zeros(n, dtype=NP_T[dt]))
    ctx.local_sort(d, out)
    got = to_host(out, NP_T[dt])
    bits = np.uint32 if dt == "u32" else np.uint64
    if not np.array_equal(got.view(bits), want.view(bits)):
        k = int(np.flatnonzero(got.view(bits) != want.view(bits))[0])
        raise AssertionError(f"{dt} {family} n={n}: first difference at key {k}: got {got[k]!r}, want {want[k]!r}; "
                             f"{int(np.count_nonzero(got.view(bits) != want.view(bits)))} keys differ")
    assert np.array_equal(to_host(d, NP_T[dt]).view(bits), x.view(bits)), "the sort changed its input"


def test_plans_cover_the_seeded_kernels():
    """The sizes above run what they are meant to: 2^14-key u32 tiles (merge
    levels 11..14) and multi-way passes of every width, 16-way chunks of both
    key sizes among them."""
    lks = {}
    for dt, n in SIZES:
        p = misort.plan(n, 4 if dt == "u32" else 8)
        assert p[0][0] == "tile_sort" and p[0][1] + 1 == (14 if dt == "u32" else 13), p
        assert all(q[0] == "run_mergek" for q in p[1:]), p
        lks.setdefault(dt, set()).update(q[2] for q in p[1:])
    assert lks["u32"] == {2, 3, 4} and lks["u64"] == {2, 3, 4} and lks["f64"] == {2, 3, 4}, lks


def test_tile_sort_battery_lt14(ctx):
    """The u32 2^14 tile alone (pass_probe tile_sort), whose levels 11..14 are
    seeded merge levels, on the SORT-tile battery: every aligned tile sorted."""
    lt, T = 14, 1 << 14
    x = B.compose([t for _, t in B.battery(T, np.dtype(np.uint32), 0)])
    assert x.size % T == 0 and x.size <= 1 << 24
    d_in, d_out = to_dev(x), to_dev(np.zeros(x.size, dtype=np.uint32))
    torch.cuda.synchronize()  # the probe runs on the context's own stream
    ctx.pass_probe(d_in, d_out, "tile_sort", lt - 1, 0, False, reps=1, n=x.size)
    ctx.synchronize()
    got = to_host(d_out, np.uint32)
    want = np.sort(x.reshape(-1, T), axis=1).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first difference at key {int(bad[0])} = tile {int(bad[0]) >> lt}; {bad.size} keys differ"
