"""The SORT-tile battery itself (tile_battery.py), on the CPU: shapes, types,
determinism, the properties the GPU tests rely on (0 and MAX in one tile, an
all-MAX tile, heavy ties, a tie-free tile, no two tiles with one multiset),
and np.sort -- the expected value of the GPU tests -- pinned to the oracle's
local sort on every battery tile."""
import numpy as np
import pytest

import oracle_lib as O
import tile_battery as B

SHAPES = [(1 << 13, np.uint64), (1 << 14, np.uint32), (1 << 15, np.uint32)]
IDS = ["u64-13", "u32-14", "u32-15"]


@pytest.fixture(scope="module")
def batteries():
    return {(T, np.dtype(dt)): B.battery(T, dt, 0) for T, dt in SHAPES}


@pytest.mark.parametrize("T,dt", SHAPES, ids=IDS)
def test_generators_shape_dtype_determinism(T, dt):
    sp = B.specs(T, dt)
    assert len({s[0] for s in sp}) == len(sp)  # names are unique
    for i, s in enumerate(sp):
        a, b = B.make(s, T, dt, 5, i), B.make(s, T, dt, 5, i)
        assert a.shape == (T,) and a.dtype == np.dtype(dt), s[0]
        assert np.array_equal(a, b), s[0]


@pytest.mark.parametrize("T,dt", SHAPES, ids=IDS)
def test_battery_covers_the_families(T, dt):
    names = [s[0] for s in B.specs(T, dt)]
    zo = [n for n in names if n.startswith("zero_one")]
    for p in B.zero_one_pairs(dt):
        for ks in B.KSPECS:  # every (LO, HI) pair meets every count
            assert any(n.startswith(f"zero_one[{p[0]},k={ks},") for n in zo), (p[0], ks)
        for order in B.ORDERS:
            assert any(n.startswith(f"zero_one[{p[0]},") and f",{order}," in n for n in zo), (p[0], order)
    for R in B.RUNS:
        for pre in (f"zero_one[", f"rotated[s=R,R={R}]", f"rotated[s=R-1,R={R}]", f"interleave[R={R}]"):
            assert any(n.startswith(pre) and f"R={R}]" in n for n in names), (pre, R)
    for m in B.FEW:
        assert f"few_values[m={m}]" in names
    for j in range(1, T.bit_length()):
        for kind in ("saw", "mirror", "stairs"):
            assert f"sawtooth[{kind},j={j}]" in names
    for n in ("ascending", "descending", "organ_pipe", "bit_reversal", "sentinels_random", "around_half"):
        assert n in names
    if np.dtype(dt).itemsize == 8:
        for n in ("u64_low_word[top=1]", "u64_low_word[top=0]", "u64_high_word", "u64_opposed"):
            assert n in names


@pytest.mark.parametrize("T,dt", SHAPES, ids=IDS)
def test_generator_contents(T, dt):
    M = B.key_max(dt)
    for pi, (_, lo, hi, _) in enumerate(B.zero_one_pairs(dt)):
        for order in B.ORDERS:
            for k in (0, 1, 33, T // 2, T - 1, T):
                x = B.zero_one(T, dt, 3, 0, pair=pi, k=k, order=order, R=1 << 10)
                assert int((x == hi).sum()) == k and int((x == lo).sum()) == T - k, (pi, order, k)
    x = B.zero_one(T, dt, 3, 2, pair=0, k=700, order="one_run", R=1 << 10)
    pos = np.flatnonzero(x != 0)
    assert pos.size == 700 and pos[0] >> 10 == pos[-1] >> 10
    for m in B.FEW:
        x = B.few_values(T, dt, 1, 9, m=m)
        assert np.unique(x).size == m and x.min() == 0 and x.max() == M
    assert np.array_equal(B.sawtooth(T, dt, 0, 0, j=3, kind="saw")[:10].astype(np.uint32) & 0xFFFFFFFF,
                          np.arange(10) % 8)
    assert np.array_equal(np.sort(B.bit_reversal(T, dt, 0, 0)), B.ascending(T, dt, 0, 0))
    x = B.interleave(T, dt, 0, 0, R=1 << 9)
    for r in range(T >> 9):  # every run ascending; merged, consecutive keys come from consecutive runs
        assert np.all(np.diff(x[r << 9:(r + 1) << 9].astype(np.float64)) > 0)
    assert np.array_equal(np.argsort(x, kind="stable")[:T >> 9] >> 9, np.arange(T >> 9))
    x = B.sentinels_random(T, dt, 0, 0)
    assert np.all(x[::11][np.arange(x[::11].size) * 11 % 13 != 5] == M) and np.all(x[5::13] == 0)
    if np.dtype(dt).itemsize == 8:
        for top in (0, 1):
            x = B.u64_low_word(T, dt, 0, 4, top=top)
            assert np.unique(x >> np.uint64(32)).size == 1 and int(x[0] >> np.uint64(63)) == top
        assert np.all(B.u64_high_word(T, dt, 0, 4) & np.uint64(0xFFFFFFFF) == np.uint64(0xFFFFFFFF))
        x = np.sort(B.u64_opposed(T, dt, 0, 4))
        assert np.all(np.diff((x & np.uint64(0xFFFFFFFF)).astype(np.int64)) < 0)


@pytest.mark.parametrize("T,dt", SHAPES, ids=IDS)
def test_battery_properties(batteries, T, dt):
    tiles = [x for _, x in batteries[(T, np.dtype(dt))]]
    M = B.key_max(dt)
    assert len(tiles) << (T.bit_length() - 1) <= 1 << 24
    assert any(x.min() == 0 and x.max() == M for x in tiles)
    assert any(np.all(x == M) for x in tiles)
    assert any(np.unique(x, return_counts=True)[1].max() >= T // 2 for x in tiles)
    assert any(np.unique(x).size == T for x in tiles)
    assert len({B.multiset_id(x) for x in tiles}) == len(tiles)  # no two tiles hold one multiset


def test_tile_index_changes_the_multiset():
    T, dt = 1 << 13, np.uint64
    M = B.key_max(dt)
    for s in B.specs(T, dt):
        a, b = B.make(s, T, dt, 0, 3), B.make(s, T, dt, 0, 300)
        if np.all((a == 0) | (a == M)) and s[1] is B.zero_one:
            continue  # only the pinned values 0 and MAX, their counts given: nothing to mix into
        assert B.multiset_id(a) != B.multiset_id(b), s[0]


def test_compose_and_cycle():
    T, dt = 1 << 13, np.uint64
    tiles = B.cycle(T, dt, 0, 5)
    x = B.compose(tiles, 77)
    assert x.size == 4 * T + 77 and x.dtype == np.dtype(dt)
    assert np.array_equal(x[:T], tiles[0]) and np.array_equal(x[4 * T:], tiles[4][:77])
    assert B.compose(tiles).size == 5 * T
    n = len(B.specs(T, dt))
    two = B.cycle(T, dt, 0, n + 2)
    assert not np.array_equal(two[1], two[n + 1])  # the second round carries new tile indices
    part = B.cycle(T, dt, 0, 7, families=("few_values", "sentinels_random"))
    assert all(np.any(p == B.key_max(dt)) and np.any(p == 0) for p in part)


@pytest.mark.parametrize("T,dt", SHAPES[:2], ids=IDS[:2])
def test_numpy_sort_equals_oracle_on_every_tile(batteries, T, dt):
    for name, x in batteries[(T, np.dtype(dt))]:
        assert np.array_equal(O.local_sort(x), np.sort(x)), name
