"""The segmented top-k's oracle -- numpy helpers only (no GPU, no pytest marks).

Everything works on key BIT PATTERNS (u32, 1-D) and int64 offsets.  Per segment
the order is that of the ascending record T(key) << 32 | position (topk_oracle.
tmap: T = K for the smallest keys, ~K for the largest, K the identity or the
order-preserving pattern of a float32), so equal keys come out in ascending
position order in both directions.  Row i of the (nseg, k) results holds the
first min(k, len) of segment i's stable argsort of T, then the fill: index
0xFFFFFFFF and the unmapped all-ones key.
"""
import numpy as np

from topk_oracle import tmap, tunmap

U32 = np.uint32
FILL_INDEX = U32(0xFFFFFFFF)


def fill_key(largest, f32):
    """The last key of the direction's order: u32 0xFFFFFFFF / 0, f32 pattern
    0x7FFFFFFF / 0xFFFFFFFF (smallest / largest)."""
    return U32(tunmap(np.array([0xFFFFFFFF], dtype=U32), largest, f32)[0])


def topk_segments(keys_bits, offs, k, largest, f32=False):
    """(key bit patterns, u32 positions), each (nseg, k)."""
    keys_bits = np.asarray(keys_bits, dtype=U32)
    offs = np.asarray(offs, dtype=np.int64)
    nseg = offs.size - 1
    lens = np.diff(offs)
    vals = np.full((nseg, k), fill_key(largest, f32), dtype=U32)
    idx = np.full((nseg, k), FILL_INDEX, dtype=U32)
    a, b = int(offs[0]), int(offs[-1])
    if b > a and k > 0:
        body = keys_bits[a:b]
        ids = np.repeat(np.arange(nseg, dtype=np.int64), lens)
        start = np.repeat(offs[:-1] - a, lens)
        order = np.lexsort((tmap(body, largest, f32), ids))  # stable: by segment, then T, then position
        rank = np.arange(b - a, dtype=np.int64) - start      # place inside the sorted segment
        keep = rank < k
        vals[ids[keep], rank[keep]] = body[order[keep]]
        idx[ids[keep], rank[keep]] = (order[keep] - start[keep]).astype(U32)
    return vals, idx


def topk_segments_loop(keys_bits, offs, k, largest, f32=False):
    """The same by a plain loop over the segments: what the oracle is held against."""
    keys_bits = np.asarray(keys_bits, dtype=U32)
    nseg = len(offs) - 1
    vals = np.full((nseg, k), fill_key(largest, f32), dtype=U32)
    idx = np.full((nseg, k), FILL_INDEX, dtype=U32)
    for i in range(nseg):
        seg = keys_bits[int(offs[i]):int(offs[i + 1])]
        t = tmap(seg, largest, f32).tolist()
        order = sorted(range(len(t)), key=lambda p: (t[p], p))[:k]
        for j, p in enumerate(order):
            vals[i, j], idx[i, j] = seg[p], p
    return vals, idx


def ties_at_the_cut(keys_bits, offs, k, largest, f32=False):
    """How many segments have their k-th and (k + 1)-th best mapped keys equal."""
    keys_bits = np.asarray(keys_bits, dtype=U32)
    hits = 0
    for i in range(len(offs) - 1):
        seg = keys_bits[int(offs[i]):int(offs[i + 1])]
        if seg.size > k:
            t = np.sort(tmap(seg, largest, f32))
            hits += int(t[k - 1] == t[k])
    return hits
