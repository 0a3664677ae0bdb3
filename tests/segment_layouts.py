"""Segment layouts and the host oracle of the segmented sort -- numpy helpers
only (no GPU, no pytest marks).

Two things live here.  The host side of tests/test_gpu_segments.py (offsets
from lengths, the key families, ``want``: every segment sorted on its own, on
bit patterns), and the named layouts of tests/test_gpu_segments_many.py: arrays
of segment lengths with more segments than one workgroup of the offset sweeps
takes.

A workgroup of k_seg_count / k_seg_scatter (segs.hip) takes ``WG`` = 2048
consecutive segments, in 8 trips of 256; segments i with the same ``i // WG``
(a span) share the workgroup's LDS counters and one global atomic per class.
Every layout function returns an int64 array of lengths, takes ``key_bytes``
(4 or 8) and is seeded: the same arguments give the same lengths.  Below,
t = misort.tile_log2(key_bytes) is the largest tile class; the class of a
length is misort.segment_class.  tests/test_segment_layouts.py pins what the
GPU file relies on (more than one span, the classes covered, the key totals).
"""
import numpy as np

import misort
from guard_bands import kmap

WG = 2048  # segments per workgroup of the offset sweeps: SEGS_NT * SEGS_ITER (segs.hip)
MAX_KEYS = {4: 1 << 22, 8: 1 << 21}  # per layout: a GPU case stays at a few seconds, host oracle included


# ---- offsets, oracle, key families ---------------------------------------------------

def offsets_of(lens, first=0):
    return np.concatenate([[first], first + np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def seg_ids(offs):
    lens = np.diff(offs)
    ids = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    pos = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(offs[:-1] - offs[0], lens)
    return ids, pos, np.repeat(lens, lens)


def want(k, offs, dt):
    """The oracle on bit patterns: k with every segment sorted (f64: by kmap)."""
    out = k.copy()
    a, b = int(offs[0]), int(offs[-1])
    ids, _, _ = seg_ids(offs)
    body = k[a:b]
    o = kmap(body.view(np.float64)) if dt == np.float64 else body
    order = np.lexsort((o, ids))
    out[a:b] = body[order]
    return out


def rand(rng, n, u):
    return rng.integers(0, np.iinfo(u).max, size=n, dtype=u, endpoint=True)


def fam_sentinels(rng, ids, pos, ln, u):
    k = rand(rng, ids.size, u)
    k[pos % 3 == 0] = np.iinfo(u).max  # a third of each segment: the padding value
    return k


def fam_opposed(rng, ids, pos, ln, u):
    """Every key of segment i lies above every key of segment i + 1."""
    top = int(ids.max()) + 1 if ids.size else 1
    assert top < (1 << 11)
    return ((top - ids) * (1 << 20) + rng.integers(0, 1 << 20, ids.size)).astype(u)


def fam_opposed_wide(rng, ids, pos, ln, u):
    """fam_opposed for up to 2^16 - 1 segments: ((nseg - id) << 16) | 16 random
    bits.  A segment sorted together with a neighbour, or written to a
    neighbour's place, shows."""
    top = int(ids.max()) + 1 if ids.size else 1
    assert top < (1 << 16)
    return (((top - ids) << 16) | rng.integers(0, 1 << 16, ids.size)).astype(u)


FAMILIES = {
    "random": lambda rng, ids, pos, ln, u: rand(rng, ids.size, u),
    "dups": lambda rng, ids, pos, ln, u: ((ids * 4 + rng.integers(0, 4, ids.size)).astype(u) * u(0x01000193)),
    "sentinels": fam_sentinels,
    "opposed": fam_opposed,
    "ascending": lambda rng, ids, pos, ln, u: (pos * 3 + ids * 7919).astype(u),
    "descending": lambda rng, ids, pos, ln, u: ((ln - pos) * 3 + ids * 7919).astype(u),
}
# (not in FAMILIES: the tests that run every family there keep their cases)
WIDE_FAMILIES = {"opposed_wide": fam_opposed_wide}


def make(family, seed, offs, n, u):
    """n keys (bit patterns): the family inside [offs[0], offs[-1]), random outside."""
    rng = np.random.default_rng(seed)
    k = rand(rng, n, u)
    ids, pos, ln = seg_ids(offs)
    fam = FAMILIES[family] if family in FAMILIES else WIDE_FAMILIES[family]
    k[int(offs[0]):int(offs[-1])] = fam(rng, ids, pos, ln, u)
    return k


# ---- lengths of a class ------------------------------------------------------------------

def class_lo(c):
    """The lengths of tile class c are (class_lo(c), 2^c]: class 5 starts at 1."""
    return 0 if c == 5 else 1 << (c - 1)


def _draw(rng, classes):
    """One length per entry of ``classes``, uniform over the class's range."""
    classes = np.asarray(classes, dtype=np.int64)
    lo = np.where(classes == 5, 0, np.int64(1) << (classes - 1))
    return rng.integers(lo + 1, (np.int64(1) << classes) + 1)


def _ends(classes, full):
    """The shortest length of each class, or (where ``full``) all 2^c keys."""
    classes = np.asarray(classes, dtype=np.int64)
    return np.where(full, np.int64(1) << classes, np.where(classes == 5, 0, np.int64(1) << (classes - 1)) + 1)


# ---- the layouts -----------------------------------------------------------------------------

BOUNDARY_NSEG = (255, 256, 257, 2047, 2048, 2049, 4095, 4097)  # around a trip, a workgroup, two workgroups


def boundary(nseg, key_bytes, seed=1):
    """nseg segments, a quarter of them empty, the rest of classes 5..9; the last
    one is not empty (offsets[nseg] is read by the sweep's last live lane)."""
    rng = np.random.default_rng([seed, nseg, key_bytes])
    lens = _draw(rng, rng.integers(5, 10, nseg))
    lens[rng.random(nseg) < 0.25] = 0
    if lens[-1] == 0:
        lens[-1] = 33
    return lens.astype(np.int64)


def long_lengths(key_bytes):
    """mixed's seven long lengths.  Classes t + 1 (four lengths: the shortest,
    the longest, the padding-free 2^(t + 1) and one in between) and t + 2 (two),
    and the shortest of class t + 3, so that there are three long classes."""
    t = misort.tile_log2(key_bytes)
    T = 1 << t
    return [T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 4 * T - 3, T + T // 2 + 3, 4 * T + 1]


def mixed(key_bytes, nseg=20011, long_at=(0, 2047, 2048, 10000, 20009, 20010, 12000), seed=2):
    """About 30 % empty segments; the others over every tile class 5..t, class c
    with weight 2^-(c - 5) (long-tailed: many short segments, few large ones);
    the shortest and the full length of every tile class twice in the first and
    twice in the last span; long_lengths() at ``long_at``."""
    t = misort.tile_log2(key_bytes)
    rng = np.random.default_rng([seed, nseg, key_bytes])
    w = 0.5 ** np.arange(t - 4)
    lens = _draw(rng, rng.choice(np.arange(5, t + 1), size=nseg, p=w / w.sum()))
    lens[rng.random(nseg) < 0.3] = 0
    for c in range(5, t + 1):
        lens[100 + c], lens[nseg - 100 - c] = class_lo(c) + 1, 1 << c
        lens[300 + c], lens[nseg - 300 - c] = 1 << c, class_lo(c) + 1
    assert len(long_at) == 7 and max(long_at) < nseg
    lens[list(long_at)] = long_lengths(key_bytes)
    return lens.astype(np.int64)


STRIPED_NSEG = 5 * WG + 77


def striped_by_workgroup(key_bytes):
    """Segment i has class 5 + (i // WG) % 5, the shortest and the full length of
    the class alternating: every workgroup feeds ONE class (all its lanes meet
    in that class's LDS counters), and class 5 comes from the first workgroup
    and the partial last one."""
    i = np.arange(STRIPED_NSEG)
    return _ends(5 + (i // WG) % 5, i % 2 == 1).astype(np.int64)


def striped_by_lane(key_bytes):
    """Segment i has class 5 + i % 8 % 5: lane t of every trip holds segment
    i = t (mod 8), so each of the 8 LDS counters of a class is fed by fixed
    lanes, and every workgroup feeds every class 5..9."""
    i = np.arange(STRIPED_NSEG)
    return _ends(5 + i % 8 % 5, (i // 8) % 2 == 1).astype(np.int64)


def sparse(key_bytes):
    """6000 segments, four of them not empty: most lanes, most trips and one
    whole workgroup but its last lane list nothing."""
    lens = np.zeros(6000, dtype=np.int64)
    lens[[0, 2047, 2048, 5999]] = [33, 1, 1 << misort.tile_log2(key_bytes), 700]
    return lens


def all_empty(key_bytes):
    return np.zeros(5000, dtype=np.int64)


def unit(key_bytes):
    """Lengths 1 and 2 alternating: the LR = 5 tile, R segments per tile, over
    many tiles."""
    return (1 + np.arange(40000) % 2).astype(np.int64)


# name -> (lengths(key_bytes), offsets[0], keys after offsets[nseg])
LAYOUTS = {f"boundary{n}": (lambda kb, n=n: boundary(n, kb), 0, 0) for n in BOUNDARY_NSEG}
LAYOUTS.update({
    "mixed": (mixed, 0, 0),
    "striped_by_workgroup": (striped_by_workgroup, 0, 0),
    "striped_by_lane": (striped_by_lane, 0, 0),
    "sparse": (sparse, 0, 0),
    "all_empty": (all_empty, 7, 9),
    "unit": (unit, 0, 0),
})


def layout(name, key_bytes):
    """(offsets, n) of a named layout."""
    lens, first, tail = LAYOUTS[name]
    offs = offsets_of(lens(key_bytes), first)
    return offs, int(offs[-1]) + tail


# ---- which workgroups feed a class -----------------------------------------------------------

def classes_of(lens, key_bytes):
    """misort.segment_class of every length (-1: empty)."""
    lens = np.asarray(lens, dtype=np.int64)
    uniq, inv = np.unique(lens, return_inverse=True)
    return np.array([misort.segment_class(int(x), key_bytes) for x in uniq], dtype=np.int64)[inv]


def class_spans(lens, key_bytes):
    """{class: the set of spans i // WG whose segments feed it}; empty segments
    feed none."""
    cls = classes_of(lens, key_bytes)
    span = np.arange(cls.size) // WG
    return {int(c): set(span[cls == c].tolist()) for c in np.unique(cls) if c >= 0}
