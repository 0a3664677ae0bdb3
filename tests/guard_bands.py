"""Guard bands around a block of keys -- numpy helpers only (no GPU, no pytest
marks).

A kernel that pads ragged input with the all-ones key can store one padding
key at index n of its output, or at index -1 of a view that starts inside its
storage, and a comparison over [0, n) never sees it.  The buffer-contract tests
therefore lay every block out between two bands of a canary key that does not
occur in the data and compare the bands afterwards, bit for bit.

``guarded`` builds the layout on the host (the GPU tests upload ``base`` and
slice the same view out of the device tensor); ``assert_guards`` checks a host
copy of the whole base.  tests/test_guard_bands.py shows that the check bites.
"""
import numpy as np

U64 = np.uint64
TAIL = 64  # canary keys after the block


def canary_for(*arrays):
    """A key (of the arrays' unsigned dtype) that occurs in none of them."""
    dt = arrays[0].dtype
    assert dt in (np.uint32, np.uint64) and all(a.dtype == dt for a in arrays)
    c = 0xA5A5A5A5 if dt == np.uint32 else 0xA5A5A5A5A5A5A5A5
    while any(np.any(a == np.array(c, dtype=dt)) for a in arrays):
        c += 1
    return np.array(c, dtype=dt)


def guarded(n, dtype, lead, fill, body=None):
    """(base, view): ``base`` holds ``lead`` canaries, a block of n keys and
    TAIL canaries; ``view`` is the block, ``base[lead:lead + n]`` (a numpy view:
    writing it writes base).  ``fill`` is the canary key; the block starts as
    ``body`` (n keys) or, without one, as canaries too."""
    assert n >= 0 and lead >= 0
    base = np.full(lead + n + TAIL, fill, dtype=dtype)
    view = base[lead:lead + n]
    if body is not None:
        body = np.asarray(body)
        assert body.shape == (n,) and body.dtype == base.dtype
        view[:] = body
    return base, view


def assert_guards(base, n, lead, fill):
    """Raises AssertionError unless every key of ``base`` (a host array laid out
    by ``guarded``) outside [lead, lead + n) still equals the canary ``fill``;
    the message names the first changed key by its index relative to the block
    (-1: just before it, n: just after it)."""
    base = np.asarray(base)
    assert base.ndim == 1 and base.size == lead + n + TAIL, "not a guarded(n, ..., lead, ...) layout"
    bad = base != np.array(fill, dtype=base.dtype)
    bad[lead:lead + n] = False
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"guard band changed: key {i - lead} of a block of {n} (lead {lead}) holds "
                             f"{int(base[i]):#x}, the canary is {int(fill):#x}; {int(bad.sum())} guard keys differ")


def kmap(keys):
    """Order-preserving u64 pattern of 64-bit keys: u64 as they are; f64 with
    the sign set inverted, else the sign bit set."""
    if keys.dtype == np.float64:
        b = keys.view(np.uint64)
        return np.where(b >> U64(63) != 0, ~b, b | U64(1 << 63)).astype(np.uint64)
    return keys


def kunmap(o):
    """The f64 bit pattern of an ordered u64 pattern (the inverse of kmap on f64)."""
    return np.where(o >> U64(63) != 0, o & U64(0x7FFFFFFFFFFFFFFF), ~o).astype(np.uint64)
