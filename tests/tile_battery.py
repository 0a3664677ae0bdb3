"""Adversarial key tiles for the SORT pass -- generators only (numpy, no GPU, no
pytest marks).

Every generator is a pure function ``gen(T, dtype, seed, tile=0, **params)``
returning exactly T keys of ``dtype`` (np.uint32 or np.uint64), the same keys
for the same arguments.  T is a SORT tile's key count (2^13, 2^14 or 2^15); R
is a run length (2^9, 2^10 or 2^11: the lengths at which a tile may switch from
a sorting network to in-LDS merges, today's and the neighbouring ones).

``tile`` is the tile's index in a multi-tile input.  Each generator mixes it
into at least one class of its keys, so the same generator at two tile
indices gives two different multisets: a kernel that sorts the wrong tile's
keys (a persistent grid prefetching the wrong tile) cannot produce the right
output.  The classes pinned to 0 and to the all-ones key stay pinned -- those
values are the point of the tile.  The only tiles a tile index cannot change
are 0-1 tiles that hold nothing but pinned values with given counts (all keys
MAX; one 0 and T - 1 MAX); ``battery`` drops exact repeats of an earlier
multiset.

``specs(T, dtype)`` lists the battery as (name, generator, params);
``battery(T, dtype, seed)`` builds it with tile index = position in specs;
``compose(tiles, tail)`` lays tiles out as one input whose last tile is cut.
"""
import hashlib
import re

import numpy as np

RUNS = (1 << 9, 1 << 10, 1 << 11)
ORDERS = ("first", "last", "alternating", "random", "one_run")
KSPECS = ("0", "1", "2", "31", "32", "33", "63", "64", "65", "R-1", "R", "R+1",
          "T/2-1", "T/2", "T/2+1", "T-R", "T-1", "T")
FEW = (2, 3, 5, 64)
ROTATIONS = ("1", "R-1", "R", "T/2", "T-1")


def key_bits(dtype):
    return np.dtype(dtype).itemsize * 8


def key_max(dtype):
    return int(np.iinfo(dtype).max)


def _rng(seed, tile, salt):
    return np.random.default_rng([int(seed) & 0xFFFFFFFF, int(tile), int(salt)])


def _ramp(v, dtype, tile):
    """Order-preserving map of the small integers v (0 <= v <= T) to keys: the
    tile index is added, and u64 keys carry the value in both words."""
    scale = 1 if key_bits(dtype) == 32 else 0x100000001
    return ((np.asarray(v).astype(np.uint64) + np.uint64(tile)) * np.uint64(scale)).astype(dtype)


def resolve(spec, T, R):
    """A symbolic count or shift ('R+1', 'T/2', '31') as an integer."""
    m = re.fullmatch(r"(T/2|T|R|\d+)(?:([+-])(R|\d+))?", spec)
    val = {"T/2": T // 2, "T": T, "R": R}
    a, b = (val[g] if g in val else int(g or 0) for g in (m.group(1), m.group(3)))
    return a - b if m.group(2) == "-" else a + b


# ------------------------------------------------------------------ 0-1 inputs

def zero_one_pairs(dtype):
    """(name, LO, HI, how the tile index is mixed in)."""
    b, M = key_bits(dtype), key_max(dtype)
    mid = 1 << (b - 1)
    pairs = [("0_1", 0, 1, "hi+"), ("0_max", 0, M, "lo_odd"), ("max-1_max", M - 1, M, "lo-"),
             ("mid-1_mid", mid - 1, mid, "hi+")]
    if b == 64:
        pairs.append(("lowones_highone", 0x00000000FFFFFFFF, 0x0000000100000000, "hi32+"))
    return pairs


def zero_one(T, dtype, seed, tile=0, pair=0, k=0, order="first", R=1 << 10):
    """k keys of value HI, T - k of value LO.

    Orders: 'first' / 'last' (all HI first / last), 'alternating' (HI, LO, HI,
    ... until one class runs out), 'random' (positions drawn from seed and
    tile), 'one_run' (the HI keys at random positions inside one aligned run
    of R keys; if k > R the LO keys are the ones inside one run; if neither
    class fits a run, the HI keys are one stretch starting at a run boundary).

    Tile index: 'hi+' HI + tile, 'lo-' LO - tile, 'hi32+' HI + (tile << 32),
    'lo_odd' (the pair (0, MAX), both values pinned): every second LO key
    holds `tile` instead of 0.  With k = 0 an unpinned LO carries it."""
    _, lo, hi, mix = zero_one_pairs(dtype)[pair]
    assert 0 <= k <= T and T % R == 0
    rng = _rng(seed, tile, 1)
    m = np.zeros(T, dtype=bool)  # True: HI
    if order == "first":
        m[:k] = True
    elif order == "last":
        m[T - k:] = True
    elif order == "alternating":
        if 2 * k <= T:
            m[0:2 * k:2] = True
        else:
            m[:] = True
            m[1:2 * (T - k):2] = False
    elif order == "random":
        m[rng.choice(T, size=k, replace=False)] = True
    elif order == "one_run":
        r0 = ((tile + seed) % (T // R)) * R
        if k <= R:
            m[r0 + rng.choice(R, size=k, replace=False)] = True
        elif T - k <= R:
            m[:] = True
            m[r0 + rng.choice(R, size=T - k, replace=False)] = False
        else:
            m[(r0 + np.arange(k)) % T] = True
    else:
        raise ValueError(order)
    if mix in ("hi+", "hi32+") and k == 0 and lo != 0:
        lo -= tile  # no HI key to carry it
    elif mix == "hi+":
        hi += tile
    elif mix == "lo-":
        lo -= tile
    elif mix == "hi32+":
        hi += tile << 32
    x = np.where(m, np.array(hi, dtype=dtype), np.array(lo, dtype=dtype)).astype(dtype)
    if mix == "lo_odd":
        x[np.flatnonzero(~m)[1::2]] = tile
    return x


# ------------------------------------------------------- few distinct values

def few_values(T, dtype, seed, tile=0, m=2):
    """m distinct values, 0 and MAX among them, at random positions.  The
    other m - 2 values carry the tile index; with m = 2 the count of MAX
    keys does."""
    M = key_max(dtype)
    rng = _rng(seed, tile, 2)
    if m == 2:
        x = np.zeros(T, dtype=dtype)
        x[rng.choice(T, size=1 + (T // 3 + 7919 * tile) % (T - 1), replace=False)] = M
        return x
    vals = [0, M] + [((j + 1) * (M // (m - 1))) ^ tile for j in range(m - 2)]
    idx = rng.integers(0, m, size=T)
    idx[rng.choice(T, size=m, replace=False)] = np.arange(m)  # every value present
    return np.array(vals, dtype=dtype)[idx]


# --------------------------------------------------------- sawtooth and stairs

def sawtooth(T, dtype, seed, tile=0, j=1, kind="saw"):
    """'saw': i mod 2^j; 'mirror': its descending mirror; 'stairs': i >> j
    (equal stretches of 2^j keys, aligned with every run boundary >= 2^j)."""
    i = np.arange(T, dtype=np.int64)
    if kind == "saw":
        v = i & ((1 << j) - 1)
    elif kind == "mirror":
        v = ((1 << j) - 1) - (i & ((1 << j) - 1))
    elif kind == "stairs":
        v = i >> j
    else:
        raise ValueError(kind)
    return _ramp(v, dtype, tile)


# --------------------------------------------------------------------- orders

def ascending(T, dtype, seed, tile=0):
    return _ramp(np.arange(T), dtype, tile)


def descending(T, dtype, seed, tile=0):
    return _ramp(np.arange(T)[::-1], dtype, tile)


def organ_pipe(T, dtype, seed, tile=0):
    i = np.arange(T)
    return _ramp(np.minimum(i, T - 1 - i), dtype, tile)


def bit_reversal(T, dtype, seed, tile=0):
    lt = T.bit_length() - 1
    i = np.arange(T, dtype=np.int64)
    v = np.zeros(T, dtype=np.int64)
    for b in range(lt):
        v |= ((i >> b) & 1) << (lt - 1 - b)
    return _ramp(v, dtype, tile)


def rotated(T, dtype, seed, tile=0, s=1):
    """Sorted keys rotated right by s."""
    return _ramp(np.roll(np.arange(T), s), dtype, tile)


def interleave(T, dtype, seed, tile=0, R=1 << 10):
    """Run r of R keys holds r, r + T/R, r + 2T/R, ...: merging the runs takes
    one key from each in turn."""
    i = np.arange(T, dtype=np.int64)
    return _ramp((i // R) + (i % R) * (T // R), dtype, tile)


# ------------------------------------------------------------ sentinels, halves

def sentinels_random(T, dtype, seed, tile=0):
    """Uniform keys with x[::11] = MAX and x[5::13] = 0."""
    x = _rng(seed, tile, 3).integers(0, key_max(dtype), size=T, dtype=dtype, endpoint=True)
    x[::11] = key_max(dtype)
    x[5::13] = 0
    return x


def around_half(T, dtype, seed, tile=0):
    """Keys within 32 of 2^(b-1) (the sign bit of a signed compare), many
    equal; the largest key carries the tile index."""
    mid = 1 << (key_bits(dtype) - 1)
    rng = _rng(seed, tile, 4)
    x = np.uint64(mid - 32) + rng.integers(0, 64, size=T, dtype=np.uint64)
    x[int(rng.integers(0, T))] = mid + 32 + tile
    return x.astype(dtype)


def u64_low_word(T, dtype, seed, tile=0, top=0):
    """One high word (its top bit = `top`, the tile index below it); only the
    low words differ."""
    assert key_bits(dtype) == 64
    low = _rng(seed, tile, 5).integers(0, 1 << 32, size=T, dtype=np.uint64)
    return (np.uint64(((top << 31) | (tile + 1)) << 32) | low).astype(dtype)


def u64_high_word(T, dtype, seed, tile=0):
    """Low word 0xFFFFFFFF everywhere; only the high words differ."""
    assert key_bits(dtype) == 64
    high = _rng(seed, tile, 6).integers(0, 1 << 32, size=T, dtype=np.uint64)
    high[0] = tile
    return ((high << np.uint64(32)) | np.uint64(0xFFFFFFFF)).astype(dtype)


def u64_opposed(T, dtype, seed, tile=0):
    """(k << 32) | (~k & 0xFFFFFFFF), k a shuffled ramp: the high word ascends
    where the low word descends."""
    assert key_bits(dtype) == 64
    k = (_rng(seed, tile, 7).permutation(T).astype(np.uint64) + np.uint64(tile)) * np.uint64(0x10001)
    return ((k << np.uint64(32)) | (~k & np.uint64(0xFFFFFFFF))).astype(dtype)


# -------------------------------------------------------------------- battery

def specs(T, dtype):
    """[(name, generator, params)]: the battery for tiles of T keys."""
    out = []
    np_ = len(zero_one_pairs(dtype))
    seen = set()
    for ki, ks in enumerate(KSPECS):
        for oi, order in enumerate(ORDERS):
            for ri, R in enumerate(RUNS if ("R" in ks or order == "one_run") else RUNS[1:2]):
                k = resolve(ks, T, R)
                pair = (ki + oi + ri) % np_
                key = (pair, k, order, R if order == "one_run" else 0)
                if key in seen:
                    continue
                seen.add(key)
                out.append((f"zero_one[{zero_one_pairs(dtype)[pair][0]},k={ks},{order},R={R}]", zero_one,
                            dict(pair=pair, k=k, order=order, R=R)))
    for m in FEW:
        out.append((f"few_values[m={m}]", few_values, dict(m=m)))
    for j in range(1, T.bit_length()):
        for kind in ("saw", "mirror", "stairs"):
            out.append((f"sawtooth[{kind},j={j}]", sawtooth, dict(j=j, kind=kind)))
    for name, fn in (("ascending", ascending), ("descending", descending), ("organ_pipe", organ_pipe),
                     ("bit_reversal", bit_reversal)):
        out.append((name, fn, {}))
    shifts = {}
    for ss in ROTATIONS:
        for R in (RUNS if "R" in ss else RUNS[1:2]):
            shifts.setdefault(resolve(ss, T, R), f"rotated[s={ss},R={R}]")
    for s, name in shifts.items():
        out.append((name, rotated, dict(s=s)))
    for R in RUNS:
        out.append((f"interleave[R={R}]", interleave, dict(R=R)))
    out.append(("sentinels_random", sentinels_random, {}))
    out.append(("around_half", around_half, {}))
    if key_bits(dtype) == 64:
        out.append(("u64_low_word[top=1]", u64_low_word, dict(top=1)))
        out.append(("u64_low_word[top=0]", u64_low_word, dict(top=0)))
        out.append(("u64_high_word", u64_high_word, {}))
        out.append(("u64_opposed", u64_opposed, {}))
    return out


def make(spec, T, dtype, seed, tile):
    _, fn, params = spec
    x = fn(T, dtype, seed, tile, **params)
    assert x.shape == (T,) and x.dtype == np.dtype(dtype)
    return x


def multiset_id(x):
    return hashlib.sha1(np.sort(x).tobytes()).digest()


def battery(T, dtype, seed=0):
    """[(name, tile)]: every spec at tile index = its position in specs; a
    tile whose multiset an earlier one already has (constant tiles of a pinned
    value) is left out."""
    out, seen = [], set()
    for i, sp in enumerate(specs(T, dtype)):
        x = make(sp, T, dtype, seed, i)
        h = multiset_id(x)
        if h in seen:
            continue
        seen.add(h)
        out.append((sp[0], x))
    return out


def cycle(T, dtype, seed, ntiles, families=None):
    """ntiles tiles: the specs in turn (only those whose name starts with one of
    `families`, if given), tile index = position."""
    sp = [s for s in specs(T, dtype) if families is None or s[0].startswith(tuple(families))]
    return [make(sp[i % len(sp)], T, dtype, seed, i) for i in range(ntiles)]


def compose(tiles, tail=None):
    """The tiles one after the other; the last one cut to its first `tail` keys."""
    tiles = list(tiles)
    if tail is not None:
        assert 0 < tail <= tiles[-1].size
        tiles[-1] = tiles[-1][:tail]
    return np.ascontiguousarray(np.concatenate(tiles))
