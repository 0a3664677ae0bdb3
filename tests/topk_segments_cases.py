"""Layouts, key families and cached expectations of the segmented top-k tests --
numpy helpers only (no GPU, no pytest marks).  tests/test_gpu_topk_segments.py
runs them on the device; tests/test_topk_segments_abi.py holds what that file
relies on (the tied family really ties at the cut, for every (layout, k) used).

A layout is a list of segment lengths; the classes are misort.segment_class(len,
8): 5..13 up to the tile's 2^13 keys, ceil_log2(len) above.
"""
import functools

import numpy as np

import segment_layouts as L
import stream_order as SO
import topk_segments_oracle as TSO

U32 = np.uint32
ONES = U32(0xFFFFFFFF)


# ---- layouts -------------------------------------------------------------------------------------------

def short_lens():
    """Every length 0..70 and the ends of every tile class, shuffled; empty
    segments first, last and adjacent."""
    lens = list(range(71)) + [8191, 8192] + [(1 << lr) + d for lr in range(5, 13) for d in (-1, 0, 1)]
    lens = np.random.default_rng(11).permutation(lens).tolist()
    return [0, 0] + lens + [0, 0]


# 8193: a piece with one real record; 16385: class 15 and the piece that leaves early (pieces 3 of 0..3);
# 65537 with k = 1024: 16 k = 2^14 candidates, a pass from records to records
LONG_LENS = [8193, 0, 16384, 33, 16385, 40001, 1, 65536, 65537, 700]

LAYOUTS = {"short": short_lens(), "long": LONG_LENS}
KS = {"short": (1, 3, 32, 33, 64, 1024), "long": (1, 64, 1024)}


def offsets(layout, first=0):
    return L.offsets_of(LAYOUTS[layout], first)


# ---- key families: (rng, offs, largest) -> u32 bit patterns of offs[-1] keys -----------------------------

# the best key of every (type, direction) is in the pool, so k = 1 ties too: u32 smallest 0, u32 largest
# 0xFFFFFFFF, f32 smallest the pattern 0xFFFFFFFF, f32 largest 0x7FFFFFFF
TIE_POOL = np.array([0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000] + [v * 0x11111111 for v in range(1, 13)], dtype=U32)


def fam_tied(rng, offs, largest):
    """Three quarters of the keys from 16 values: the k-th best key has equals
    on both sides of the cut."""
    n = int(offs[-1])
    k = SO.rand(int(rng.integers(1 << 30)), n, U32)
    pick = rng.random(n) < 0.75
    k[pick] = TIE_POOL[rng.integers(0, TIE_POOL.size, int(pick.sum()))]
    return k


def fam_four(rng, offs, largest):
    return rng.integers(0, 4, size=int(offs[-1])).astype(U32) * U32(0x55555555)


def fam_equal(rng, offs, largest):
    ids, _, _ = L.seg_ids(offs)
    return (U32(0xCAFEF00D) + ids.astype(U32)).astype(U32)


def fam_half_sentinel(rng, offs, largest):
    """T is all-ones: the record's high half is the sentinel's, the position decides."""
    return np.full(int(offs[-1]), 0 if largest else ONES, dtype=U32)


def fam_half_sentinel_f32(rng, offs, largest):
    return np.full(int(offs[-1]), ONES if largest else U32(0x7FFFFFFF), dtype=U32)


def _best(largest, n):
    r = np.arange(n, dtype=U32) % U32(3)
    return ONES - r if largest else r


def fam_winners_last(rng, offs, largest):
    """The winners are the segment's last 1500 keys (the last piece and the end of the one before)."""
    k = rng.integers(1 << 8, 1 << 24, size=int(offs[-1])).astype(U32)
    for a, b in zip(offs[:-1], offs[1:]):
        n = min(int(b - a), 1500)
        k[b - n:b] = _best(largest, n)
    return k


def fam_winners_one_piece(rng, offs, largest):
    """All winners lie in one piece of 2^13 keys, the second where there is one."""
    k = rng.integers(1 << 8, 1 << 24, size=int(offs[-1])).astype(U32)
    for a, b in zip(offs[:-1], offs[1:]):
        ln = int(b - a)
        lo = 8192 if ln >= 8192 + 1500 else 0
        n = min(ln - lo, 1500)
        at = int(a) + lo + rng.permutation(min(ln - lo, 8192))[:n]
        k[at] = _best(largest, n)
    return k


def fam_f32(rng, offs, largest):
    """NaNs of both signs, +-0, +-inf, denormals among random floats."""
    return SO.f32_keys(int(rng.integers(1 << 30)), int(offs[-1])).view(U32).copy()


FAMILIES = {"tied": fam_tied, "four": fam_four, "equal": fam_equal, "half_sentinel": fam_half_sentinel,
            "winners_last": fam_winners_last, "winners_one_piece": fam_winners_one_piece, "f32": fam_f32,
            "half_sentinel_f32": fam_half_sentinel_f32}
F32_FAMILIES = ("f32", "half_sentinel_f32")


@functools.lru_cache(maxsize=None)
def keys_of(family, layout, largest):
    """The keys of a case (bit patterns, read-only): computed once."""
    offs = offsets(layout)
    rng = np.random.default_rng([sorted(FAMILIES).index(family), sorted(LAYOUTS).index(layout), int(largest)])
    keys = np.ascontiguousarray(FAMILIES[family](rng, offs, largest), dtype=U32)
    assert keys.shape == (int(offs[-1]),)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=64)
def want(family, layout, k, largest, f32):
    """(values, positions) the oracle gives: computed once, read-only."""
    out = TSO.topk_segments(keys_of(family, layout, largest), offsets(layout), k, largest, f32)
    for a in out:
        a.setflags(write=False)
    return out
