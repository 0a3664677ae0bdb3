"""The row-wise top-k's oracle and a numpy replay of its pass plan -- numpy
helpers only (no GPU, no pytest marks).

Both work on key BIT PATTERNS (u32, shape (rows, cols)).  The order is that of
the ascending record T(key) << 32 | column: T = K for the smallest keys, ~K for
the largest, K the identity or (f32) the order-preserving pattern of
sort_oracles.kmap32_bits.  Equal keys therefore come out in ascending column
order in both directions.
"""
import numpy as np

from sort_oracles import kmap32_bits, kunmap32_bits

U32, U64 = np.uint32, np.uint64
ONES = ~U64(0)  # the sentinel record


def tmap(bits, largest, f32):
    """T of the keys' bit patterns."""
    o = kmap32_bits(np.asarray(bits, dtype=U32), f32)
    return (~o).astype(U32) if largest else o


def tunmap(t, largest, f32):
    t = np.asarray(t, dtype=U32)
    return kunmap32_bits((~t).astype(U32) if largest else t, f32)


def topk_rows(keys_bits, k, largest, f32=False):
    """(key bit patterns, u32 columns), each (rows, k): per row the first k of
    the stable argsort of T."""
    keys_bits = np.asarray(keys_bits, dtype=U32)
    assert keys_bits.ndim == 2 and 0 <= k <= keys_bits.shape[1]
    order = np.argsort(tmap(keys_bits, largest, f32), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(keys_bits, order, axis=1), order.astype(U32)


def replay_plan(keys_bits, k, largest, f32, plan):
    """``plan`` (misort.topk_plan's tuples) on numpy: every pass cuts every row
    of m_in records into npieces blocks of 2^LR, padded with all-ones records,
    sorts each block and keeps its first k.  Returns what topk_rows returns."""
    keys_bits = np.asarray(keys_bits, dtype=U32)
    rows, cols = keys_bits.shape
    rec = tmap(keys_bits, largest, f32).astype(U64) << U64(32) | np.arange(cols, dtype=U64)[None, :]
    for m_in, lr, npieces, m_out in plan:
        assert rec.shape == (rows, m_in) and npieces << lr >= m_in and k <= 1 << lr
        x = np.full((rows, npieces << lr), ONES, dtype=U64)
        x[:, :m_in] = rec
        rec = np.sort(x.reshape(rows, npieces, 1 << lr), axis=2)[:, :, :k].reshape(rows, npieces * k)
        assert rec.shape[1] == m_out
    assert rec.shape == (rows, k)
    return tunmap((rec >> U64(32)).astype(U32), largest, f32), (rec & U64(0xFFFFFFFF)).astype(U32)
