"""The guard-band checker itself (guard_bands.py, CPU): it must pass a block
whose bands are untouched and raise for one altered key just before the block,
just after it, and at the far end of either band -- the places a kernel's
padding key or a shifted vector store would land."""
import numpy as np
import pytest

import guard_bands as G
import tile_battery as B

CASES = [(np.uint32, 64), (np.uint32, 1), (np.uint32, 3), (np.uint64, 32), (np.uint64, 1)]


def layout(dt, lead, n=1000):
    x = B.sentinels_random(n, dt, 7, lead)
    c = G.canary_for(x)
    base, view = G.guarded(n, dt, lead, c, x)
    return x, c, base, view


@pytest.mark.parametrize("dt,lead", CASES)
def test_untouched_bands_pass(dt, lead):
    x, c, base, view = layout(dt, lead)
    assert base.size == lead + x.size + G.TAIL and np.shares_memory(base, view)
    np.testing.assert_array_equal(view, x)
    G.assert_guards(base, x.size, lead, c)
    view[:] = np.sort(x)  # the block itself may change freely, padding values included
    view[-1] = np.iinfo(dt).max
    G.assert_guards(base, x.size, lead, c)
    empty_base, empty = G.guarded(0, dt, lead, c)
    assert empty.size == 0
    G.assert_guards(empty_base, 0, lead, c)


@pytest.mark.parametrize("dt,lead", CASES)
@pytest.mark.parametrize("where", ["before", "after", "far_left", "far_right"])
@pytest.mark.parametrize("value", ["max", "zero", "canary+1"])
def test_one_altered_guard_key_raises(dt, lead, where, value):
    x, c, base, _ = layout(dt, lead)
    n = x.size
    i = {"before": lead - 1, "after": lead + n, "far_left": 0, "far_right": base.size - 1}[where]
    base[i] = {"max": np.iinfo(dt).max, "zero": 0, "canary+1": int(c) + 1}[value]
    with pytest.raises(AssertionError, match="guard band changed"):
        G.assert_guards(base, n, lead, c)
    base[i] = c
    G.assert_guards(base, n, lead, c)


def test_message_names_the_key_relative_to_the_block():
    _, c, base, _ = layout(np.uint32, 3, n=10)
    base[3 + 10] = 0xFFFFFFFF  # one padding key at index n
    with pytest.raises(AssertionError, match=r"key 10 of a block of 10 \(lead 3\) holds 0xffffffff"):
        G.assert_guards(base, 10, 3, c)
    base[3 + 10] = c
    base[2] = 0
    with pytest.raises(AssertionError, match=r"key -1 of a block of 10"):
        G.assert_guards(base, 10, 3, c)


def test_wrong_layout_is_not_accepted():
    _, c, base, _ = layout(np.uint32, 3, n=10)
    with pytest.raises(AssertionError, match="layout"):
        G.assert_guards(base, 11, 3, c)


def test_canary_is_absent_from_every_array():
    x = np.array([0xA5A5A5A5, 0xA5A5A5A6, 5], dtype=np.uint32)
    y = np.array([0xA5A5A5A7], dtype=np.uint32)
    c = G.canary_for(x, y)
    assert c.dtype == np.uint32 and int(c) == 0xA5A5A5A8
    assert int(G.canary_for(np.zeros(3, np.uint64))) == 0xA5A5A5A5A5A5A5A5


def test_f64_key_map_roundtrip_and_order():
    bits = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000001,
                     0x3FF0000000000000, 0xBFF0000000000000], dtype=np.uint64)
    o = G.kmap(bits.view(np.float64))
    np.testing.assert_array_equal(G.kunmap(o), bits)
    # negative NaN < -inf < -1 < -denormal < -0 < +0 < +denormal < 1 < +inf < positive NaN
    order = [5, 3, 9, 7, 1, 0, 6, 8, 2, 4]
    np.testing.assert_array_equal(np.argsort(o), order)
    u = np.array([3, 1, 2], dtype=np.uint64)
    assert G.kmap(u) is u
