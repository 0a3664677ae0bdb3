"""The in-LDS co-rank search (csrc/corank_seed.h: seed, window, step schedule,
clamps, failure test, fallback) through its host model lib/corank_seed_dump,
the kernels' own arithmetic built by the host compiler.  CPU only.

On every diagonal a lane of IT outputs starts at (IT = 26 and 18: the
multi-way chunks; 32: the tile's 32-key lanes) the split must be valid: every
A key before it <= every B key after it and vice versa, so the merged values
are np.sort of the pair.  On iid keys fewer than 1 in 100 waves (64
consecutive lanes) may fall back to the full search, at every shipped level
shape; on sorted pairs every wave falls back and the splits still hold."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "parallel-computing-mpi_amd", "lib", "corank_seed_dump")
ASAN_DUMP = os.path.join(ROOT, "build", "asan", "corank_seed_dump")
ITS = (26, 18, 32)
DT = {4: np.uint32, 8: np.uint64}


def run_dump(pairs, kb, it, exe=DUMP, tmp=None, extra=()):
    """pairs: list of (A, B), all of one (la, lb).  -> the program's JSON."""
    la, lb = len(pairs[0][0]), len(pairs[0][1])
    path = os.path.join(tmp, f"pairs_{kb}_{it}_{la}_{lb}_{len(pairs)}.bin")
    with open(path, "wb") as f:
        for a, b in pairs:
            assert len(a) == la and len(b) == lb
            f.write(np.ascontiguousarray(a, dtype=DT[kb]).tobytes())
            f.write(np.ascontiguousarray(b, dtype=DT[kb]).tobytes())
    r = subprocess.run([exe, str(kb), str(it), str(la), str(lb), str(len(pairs)), path, *map(str, extra)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)


def check_splits(a, b, it, res):
    """Every lane's split is a valid merge-path split of its diagonal."""
    la, lb = len(a), len(b)
    tot = la + lb
    lanes = (tot + it - 1) // it + 1
    i = np.asarray(res["splits"], dtype=np.int64)
    assert len(i) == lanes
    d = np.minimum(np.arange(lanes, dtype=np.int64) * it, tot)
    j = d - i
    assert np.all(i >= 0) and np.all(i <= la) and np.all(j >= 0) and np.all(j <= lb)
    # the conditions whose keys exist (a side's end needs none)
    m = (i > 0) & (j < lb)  # A[i - 1] <= B[j]
    assert np.all(a[i[m] - 1] <= b[j[m]])
    m = (j > 0) & (i < la)  # B[j - 1] <= A[i]
    assert np.all(b[j[m] - 1] <= a[i[m]])
    # and, spelled out on a few diagonals: the first d merged values
    s = np.sort(np.concatenate([a, b]))
    for l in range(0, lanes, 7):
        got = np.sort(np.concatenate([a[: i[l]], b[: j[l]]]))
        assert np.array_equal(got, s[: d[l]])


def sorted_keys(rng, n, kb):
    hi = np.iinfo(DT[kb]).max
    return np.sort(rng.integers(0, hi, size=n, dtype=DT[kb], endpoint=True))


def families(kb, la, lb, seed):
    """name -> (A, B), both sorted."""
    rng = np.random.default_rng(seed)
    T = DT[kb]
    mx = np.iinfo(T).max
    out = {}
    out["iid"] = (sorted_keys(rng, la, kb), sorted_keys(rng, lb, kb))
    s = sorted_keys(rng, la + lb, kb)
    out["a_below_b"] = (s[:la].copy(), s[la:].copy())
    out["b_below_a"] = (s[lb:].copy(), s[:lb].copy())
    out["all_equal"] = (np.full(la, 12345, T), np.full(lb, 12345, T))
    out["two_values"] = (np.sort(rng.integers(0, 2, la).astype(T) * T(7) + T(3)),
                         np.sort(rng.integers(0, 2, lb).astype(T) * T(7) + T(3)))
    # sawtooth of period 257 over the concatenation, each side then sorted
    saw = (np.arange(la + lb, dtype=np.int64) % 257).astype(T)
    out["sawtooth"] = (np.sort(saw[:la]), np.sort(saw[la:]))
    # 0 and MAX keys next to the zero word and the sentinels
    e = sorted_keys(rng, la + lb, kb)
    ea, eb = e[0::2][:la].copy(), e[1::2][:lb].copy()
    if la + lb > len(ea) + len(eb):  # unequal lengths: refill
        ea, eb = sorted_keys(rng, la, kb), sorted_keys(rng, lb, kb)
    for v in (ea, eb):
        if len(v) >= 4:
            v[:2] = 0
            v[-2:] = mx
    out["zero_and_max"] = (ea, eb)
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("corank"))


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("kb", (4, 8))
@pytest.mark.parametrize("shape", [(1320, 1320), (400, 900), (5280, 5280)])
def test_splits_valid_on_every_family(kb, it, shape, tmp):
    la, lb = shape
    for name, (a, b) in families(kb, la, lb, 1000 * kb + it).items():
        res = run_dump([(a, b)], kb, it, tmp=tmp)
        assert res["bad_probes"] == 0, name
        check_splits(a, b, it, res["pairs"][0])


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("kb", (4, 8))
def test_degenerate_pairs(kb, it, tmp):
    rng = np.random.default_rng(77 + kb + it)
    for la, lb in ((0, 700), (700, 0), (1, 700), (700, 1), (0, 0), (1, 1)):
        for a, b in ((sorted_keys(rng, la, kb), sorted_keys(rng, lb, kb)),
                     (np.zeros(la, DT[kb]), sorted_keys(rng, lb, kb)),
                     (np.full(la, np.iinfo(DT[kb]).max, DT[kb]), sorted_keys(rng, lb, kb))):
            # the level's bounds of a wider neighbour pair, so the seeded search runs
            res = run_dump([(a, b)], kb, it, tmp=tmp, extra=(700, 1400))
            assert res["bad_probes"] == 0
            check_splits(a, b, it, res["pairs"][0])


# The shipped level shapes: (key bytes, outputs per lane, [(la, lb) per level]).
# u32 16-way chunks (26 per lane, ~10816 .. 12864 keys in 16 segments), 8-way
# (18 per lane, ~7936 keys in 8), the u32 tile's levels 11..14 (34 per lane),
# u64 16-way chunks (18 per lane, ~6784 keys) and the u64 tile's levels 10..13
# (33 per lane); and the shapes the window was chosen on.
LEVEL_SHAPES = [
    (4, 26, [(676, 676), (1352, 1352), (2704, 2704), (5408, 5408), (804, 804), (6432, 6432)]),
    (4, 26, [(330, 330), (660, 660), (1320, 1320), (2640, 2640), (5280, 5280), (400, 900)]),
    (4, 18, [(992, 992), (1984, 1984), (3968, 3968)]),
    (4, 34, [(1024, 1024), (2048, 2048), (4096, 4096), (8192, 8192)]),
    (4, 32, [(8192, 8192)]),
    (8, 18, [(424, 424), (848, 848), (1696, 1696), (3392, 3392)]),
    (8, 33, [(512, 512), (1024, 1024), (2048, 2048), (4096, 4096)]),
]


@functools.lru_cache(maxsize=None)
def iid_pairs(kb, la, lb, n):
    rng = np.random.default_rng(la * 7919 + lb * 31 + kb)
    return tuple((sorted_keys(rng, la, kb), sorted_keys(rng, lb, kb)) for _ in range(n))


@pytest.mark.parametrize("kb,it,shapes", LEVEL_SHAPES)
def test_iid_fallback_cap(kb, it, shapes, tmp):
    """Fewer than 1 in 100 waves fall back on iid keys (a condition of the
    design, not a tuning target), and the seeded waves search in fewer steps."""
    for la, lb in shapes:
        lanes = (la + lb + it - 1) // it + 1
        n = max(8, -(-400 // (-(-lanes // 64))))  # >= 400 waves a shape
        pairs = iid_pairs(kb, la, lb, n)
        res = run_dump(list(pairs), kb, it, tmp=tmp)
        assert res["bad_probes"] == 0
        fb = np.concatenate([p["fallback"] for p in res["pairs"]])
        print(f"kb {kb} it {it} {la}+{lb}: w {res['w']} seeded {res['seeded']} waves {fb.size} fallbacks {int(fb.sum())} "
              f"steps/lane {np.mean(np.concatenate([p['steps'] for p in res['pairs']])):.2f}")
        assert fb.size >= 400
        assert fb.sum() * 100 < fb.size, (la, lb, int(fb.sum()), fb.size)
        if res["seeded"]:
            full_steps = int(np.log2(res["top_full"])) + 1
            seed_steps = int(np.log2(res["top_seed"])) + 1
            assert seed_steps < full_steps
            for p in res["pairs"][:4]:
                st = np.asarray(p["steps"]).reshape(-1)
                f = np.repeat(np.asarray(p["fallback"]), 64)[: st.size]
                assert np.all(st[f == 0] == seed_steps) and np.all(st[f == 1] == seed_steps + full_steps)
        for (a, b), p in zip(pairs[:3], res["pairs"][:3]):
            check_splits(a, b, it, p)


@pytest.mark.parametrize("kb,it,shape", [(4, 26, (5280, 5280)), (4, 26, (2640, 2640)), (4, 18, (3968, 3968)),
                                         (4, 32, (8192, 8192)), (8, 18, (3392, 3392))])
def test_sorted_pairs_fall_back(kb, it, shape, tmp):
    """A wholly below B, and the reverse: the guess is off by up to la / 2, so
    every wave of 64 lanes falls back; the splits are the full search's.  (The
    pair's last, partial wave holds only the diagonals next to the pair's end,
    where lo, hi and the guess meet: it may pass, and its splits hold too.)"""
    la, lb = shape
    fam = families(kb, la, lb, 5)
    for name in ("a_below_b", "b_below_a"):
        a, b = fam[name]
        res = run_dump([(a, b)], kb, it, tmp=tmp)
        assert res["seeded"]
        fb = res["pairs"][0]["fallback"]
        assert res["lanes"] // 64 >= 2 and all(fb[: res["lanes"] // 64]), (name, fb)
        check_splits(a, b, it, res["pairs"][0])


def test_sanitized_model(tmp):
    """The model under ASan + UBSan (its own executable, build/asan): same output."""
    assert os.path.exists(ASAN_DUMP), "sanitized model missing: make -C parallel-computing-mpi_amd/csrc asan"
    for kb, it, (la, lb) in ((4, 26, (400, 900)), (8, 18, (1, 700)), (4, 32, (0, 0))):
        a, b = families(kb, la, lb, 9)["iid"]
        assert run_dump([(a, b)], kb, it, exe=ASAN_DUMP, tmp=tmp) == run_dump([(a, b)], kb, it, tmp=tmp)
