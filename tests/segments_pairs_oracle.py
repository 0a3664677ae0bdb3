"""Host oracle of the segmented key-value sort (misort_local_sort_segments_pairs)
-- numpy helpers only (no GPU, no pytest marks).

Every segment [offs[i], offs[i + 1]) of a pair of u32 bit-pattern arrays is
sorted on its own by (mapped key, value): one ``np.lexsort`` with the segment
index as the major key, which is per-segment because the segments are
contiguous and ascending.  The mapped key is kmap32_bits of sort_oracles.py (the
identity for u32 keys, the order-preserving pattern for f32).  For the argsort
the value of a pair is its position inside its segment.  ``loop_want`` is the
same thing as a plain Python loop over the segments;
tests/test_segments_pairs_abi.py holds the two against each other."""
import numpy as np

from segment_layouts import seg_ids
from sort_oracles import kmap32_bits

U32 = np.uint32


def positions(offs):
    """The position inside its segment of every element of [offs[0], offs[-1])."""
    return seg_ids(offs)[1].astype(U32)


def want(keys, offs, vals=None, f32=False, fringe_vals=None):
    """(keys, values) bit patterns after the call, out of place: inside
    [offs[0], offs[-1]) every segment sorted by (key, value); outside it the
    keys are the input's and the values the input's or, for the argsort
    (``vals`` None), ``fringe_vals`` (what the output held before: that part is
    not written)."""
    a, b = int(offs[0]), int(offs[-1])
    ids, pos, _ = seg_ids(offs)
    k = keys[a:b]
    v = pos.astype(U32) if vals is None else vals[a:b]
    order = np.lexsort((v, kmap32_bits(k, f32), ids))
    out_k = keys.copy()
    if vals is not None:
        out_v = vals.copy()
    elif fringe_vals is not None:
        out_v = np.array(fringe_vals, dtype=U32, copy=True)
    else:
        out_v = np.zeros(keys.size, dtype=U32)
    out_k[a:b] = k[order]
    out_v[a:b] = v[order]
    return out_k, out_v


def loop_want(keys, offs, vals=None, f32=False):
    """The sorted body [offs[0], offs[-1]) segment by segment, in plain Python:
    (keys, values) lists of ints."""
    out_k, out_v = [], []
    for i in range(len(offs) - 1):
        b, e = int(offs[i]), int(offs[i + 1])
        recs = []
        for c in range(e - b):
            key = int(keys[b + c])
            if f32:
                m = (~key & 0xFFFFFFFF) if key >> 31 else key | 0x80000000
            else:
                m = key
            recs.append((m, int(vals[b + c]) if vals is not None else c, key))
        recs.sort(key=lambda r: (r[0], r[1]))
        out_k += [r[2] for r in recs]
        out_v += [r[1] for r in recs]
    return out_k, out_v
