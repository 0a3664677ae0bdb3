"""Host oracles of the local sorts -- numpy helpers only (no GPU, no pytest
marks).  Each one is the oracle of one GPU test file, kept here so that other
files (tests/stream_order.py) compare with the same function instead of a copy:

    pairs_oracle, argsort_oracle   tests/test_gpu_pairs.py       32-bit keys with a payload
    order_of                       tests/test_gpu_pairs64.py     stable order of 64-bit keys
    want_rows                      tests/test_gpu_rows.py        every row on its own
    want_rows_pairs                tests/test_gpu_rows_pairs.py  every row's pairs by (key, value)

Every oracle works on bit patterns: K is the order-preserving unsigned pattern
of a key (the identity for unsigned keys; for floats the sign set inverted,
else the sign bit set), numpy sorts K, and the result is mapped back."""
import numpy as np

from guard_bands import kmap as kmap64, kunmap as kunmap64

U32, U64 = np.uint32, np.uint64


# ---- 32-bit keys with a payload (misort_local_sort_pairs) --------------------------------------

def kmap32(keys):
    """Order-preserving u32 pattern of the keys: u32 as they are; f32 with the
    sign set inverted, else the sign bit set."""
    if keys.dtype == np.float32:
        b = keys.view(np.uint32)
        return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return keys


def pairs_oracle(keys, vals):
    order = np.lexsort((vals, kmap32(keys)))
    return keys.view(np.uint32)[order], vals[order]


def argsort_oracle(keys):
    return np.argsort(kmap32(keys), kind="stable").astype(np.uint32)


# ---- 64-bit keys with a payload (misort_local_sort_pairs64) ------------------------------------

def order_of(keys):
    return np.argsort(kmap64(keys), kind="stable")


# ---- rows of keys (misort_local_sort_rows) ------------------------------------------------------

def want_rows(keys):
    """The oracle: bit patterns (rows, cols) of every row sorted on its own."""
    if keys.dtype == np.float64:
        return kunmap64(np.sort(kmap64(keys), axis=1))
    return np.sort(keys, axis=1)


# ---- rows of pairs (misort_local_sort_rows_pairs), on u32 bit patterns --------------------------

def kmap32_bits(b, f32):
    """Order-preserving u32 pattern of a key's bits."""
    if not f32:
        return b
    return np.where(b >> U32(31) != 0, ~b, b | U32(1 << 31)).astype(U32)


def kunmap32_bits(o, f32):
    if not f32:
        return o
    return np.where(o >> U32(31) != 0, o & U32(0x7FFFFFFF), ~o).astype(U32)


def want_rows_pairs(keys, vals=None, f32=False):
    """The oracle: (keys, values) bit patterns of every row sorted by (key, value)."""
    rows, cols = keys.shape
    v = np.broadcast_to(np.arange(cols, dtype=U64), (rows, cols)) if vals is None else vals.astype(U64)
    rec = np.sort(kmap32_bits(keys, f32).astype(U64) << U64(32) | v, axis=1)
    return kunmap32_bits((rec >> U64(32)).astype(U32), f32), (rec & U64(0xFFFFFFFF)).astype(U32)
