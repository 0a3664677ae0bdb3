"""The segment layouts themselves (segment_layouts.py, CPU): they must be what
tests/test_gpu_segments_many.py relies on, so that an edit of a generator
cannot silently shrink a case below the boundary it is there for -- more than
one workgroup of the offset sweeps (2048 segments), the classes covered and the
workgroups that feed each class's list, key totals that keep a GPU case short,
an oracle that would see a sweep that stopped after one workgroup, and
opposed_wide keys that do not interleave between neighbours."""
import numpy as np
import pytest

import misort
import segment_layouts as L

KB = (4, 8)


def lens_of(name, kb):
    return L.LAYOUTS[name][0](kb)


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_segment_counts_and_key_totals(name, kb):
    lens = lens_of(name, kb)
    assert lens.dtype == np.int64 and lens.ndim == 1 and (lens >= 0).all()
    np.testing.assert_array_equal(lens, lens_of(name, kb))  # seeded
    small = name.startswith("boundary") and int(name[len("boundary"):]) <= L.WG
    assert small or lens.size > L.WG
    assert int(lens.sum()) <= L.MAX_KEYS[kb]
    offs, n = L.layout(name, kb)
    assert offs.size == lens.size + 1 and n == int(offs[-1]) + L.LAYOUTS[name][2]
    np.testing.assert_array_equal(np.diff(offs), lens)


@pytest.mark.parametrize("kb", KB)
def test_boundary(kb):
    assert L.BOUNDARY_NSEG == (255, 256, 257, 2047, 2048, 2049, 4095, 4097)
    for nseg in L.BOUNDARY_NSEG:
        lens = L.boundary(nseg, kb)
        assert lens.size == nseg and lens[-1] > 0
        cls = L.classes_of(lens, kb)
        assert set(cls.tolist()) == {-1, 5, 6, 7, 8, 9}
        assert 0.15 < np.mean(lens == 0) < 0.35


@pytest.mark.parametrize("kb", KB)
def test_mixed(kb):
    t = misort.tile_log2(kb)
    lens = L.mixed(kb)
    assert lens.size == 20011
    assert 0.25 < np.mean(lens == 0) < 0.35
    spans = L.class_spans(lens, kb)
    assert set(spans) == set(range(5, t + 4))  # every tile class 5..t and three long classes
    for c in range(5, t + 1):
        assert len(spans[c]) >= 2, c
    for c in range(5, t):  # long-tailed: few large ones
        assert np.sum(L.classes_of(lens, kb) == c) > np.sum(L.classes_of(lens, kb) == c + 1), c
    T = 1 << t
    at = [0, 2047, 2048, 10000, 20009, 20010]
    assert lens[at].tolist() == [T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 4 * T - 3, T + T // 2 + 3]
    # (those six are two long classes; a seventh segment, the shortest of class t + 3, makes three)
    assert lens[12000] == 4 * T + 1 and sorted(np.flatnonzero(lens > T).tolist()) == sorted(at + [12000])
    cls = L.classes_of(lens, kb)
    # mixed lengths inside classes t + 1 and t + 2, one segment of exactly 2^(t + 1) keys
    assert sorted(lens[cls == t + 1].tolist()) == [T + 1, T + T // 2 + 3, 2 * T - 1, 2 * T]
    assert sorted(lens[cls == t + 2].tolist()) == [2 * T + 1, 4 * T - 3]
    assert lens[cls == t + 3].tolist() == [4 * T + 1]
    # the shortest and the full length of every tile class occur
    for c in range(5, t + 1):
        assert {L.class_lo(c) + 1, 1 << c} <= set(lens[cls == c].tolist()), c


@pytest.mark.parametrize("kb", KB)
def test_mixed_of_another_size_is_valid(kb):
    """The malformed-offsets cases start from 9001 segments."""
    t = misort.tile_log2(kb)
    lens = L.mixed(kb, nseg=9001, long_at=(0, 2047, 2048, 4000, 8990, 9000, 6000))
    assert lens.size == 9001 and int(lens.sum()) <= L.MAX_KEYS[kb]
    assert set(L.class_spans(lens, kb)) == set(range(5, t + 4))
    assert 9001 > 4 * L.WG and 8999 % L.WG >= 3 * 256  # index 8999: the fifth workgroup's partial fourth trip


@pytest.mark.parametrize("kb", KB)
def test_striped_by_workgroup(kb):
    """Span s feeds class 5 + s % 5 and no other.  With 5 * WG + 77 segments that
    is one whole workgroup per class, and for class 5 the partial sixth one as
    well: the one list here that two workgroups assemble (striped_by_lane and
    mixed have every list assembled by many)."""
    lens = L.striped_by_workgroup(kb)
    assert lens.size == 5 * L.WG + 77
    spans = L.class_spans(lens, kb)
    assert spans == {5: {0, 5}, 6: {1}, 7: {2}, 8: {3}, 9: {4}}
    assert any(len(s) >= 2 for s in spans.values())
    cls = L.classes_of(lens, kb)
    for c in range(5, 10):
        assert set(lens[cls == c].tolist()) == {L.class_lo(c) + 1, 1 << c}, c
    assert (lens[0:-1:2] < lens[1::2]).all()  # alternating: the shortest, then the full block


@pytest.mark.parametrize("kb", KB)
def test_striped_by_lane(kb):
    lens = L.striped_by_lane(kb)
    assert lens.size == 5 * L.WG + 77
    cls = L.classes_of(lens, kb)
    i = np.arange(lens.size)
    np.testing.assert_array_equal(cls, 5 + i % 8 % 5)
    # every class from every workgroup; the LDS counter of a lane is t & 7 = i & 7
    assert all(s == set(range(6)) for s in L.class_spans(lens, kb).values())
    for c in range(5, 10):
        assert set(lens[cls == c].tolist()) == {L.class_lo(c) + 1, 1 << c}, c
        for lane in set((i[cls == c] % 8).tolist()):
            assert set(lens[(cls == c) & (i % 8 == lane)].tolist()) == {L.class_lo(c) + 1, 1 << c}


@pytest.mark.parametrize("kb", KB)
def test_sparse_all_empty_unit(kb):
    lens = L.sparse(kb)
    assert lens.size == 6000
    assert {int(i): int(lens[i]) for i in np.flatnonzero(lens)} == \
        {0: 33, 2047: 1, 2048: 1 << misort.tile_log2(kb), 5999: 700}
    assert L.all_empty(kb).size == 5000 and not L.all_empty(kb).any()
    offs, n = L.layout("all_empty", kb)
    assert offs[0] == 7 and offs[-1] == 7 and n == 16
    lens = L.unit(kb)
    assert lens.size == 40000 and lens[:4].tolist() == [1, 2, 1, 2] and set(lens.tolist()) == {1, 2}


def test_class_spans():
    lens = np.zeros(3 * L.WG, dtype=np.int64)
    lens[[0, L.WG - 1, L.WG, 2 * L.WG + 5]] = [1, 33, 64, 40000]
    assert L.class_spans(lens, 4) == {5: {0}, 6: {0, 1}, 16: {2}}
    assert L.class_spans(lens, 8) == {5: {0}, 6: {0, 1}, 16: {2}}
    assert L.class_spans(np.zeros(10, dtype=np.int64), 4) == {}


@pytest.mark.parametrize("name,kb", [(n, 4) for n in L.LAYOUTS if n != "all_empty"] + [("mixed", 8)])
def test_oracle_sees_a_sweep_that_stops_after_one_workgroup(name, kb):
    u = np.uint32 if kb == 4 else np.uint64
    offs, n = L.layout(name, kb)
    k = L.make("random", 5, offs, n, u)
    w = L.want(k, offs, u)
    one = L.want(k, offs[:L.WG + 1], u)  # segments 2048.. left as they are
    if offs.size - 1 <= L.WG:
        np.testing.assert_array_equal(one, w)
    else:
        assert not np.array_equal(one, w)
        cut = int(offs[L.WG])
        np.testing.assert_array_equal(one[:cut], w[:cut])
        np.testing.assert_array_equal(one[cut:], k[cut:])


@pytest.mark.parametrize("u", [np.uint32, np.uint64], ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["mixed", "unit", "striped_by_lane"])
def test_opposed_wide_keys_of_adjacent_segments_do_not_interleave(name, u):
    offs, n = L.layout(name, np.dtype(u).itemsize)
    k = L.make("opposed_wide", 9, offs, n, u)
    ids, _, _ = L.seg_ids(offs)
    nseg = offs.size - 1
    np.testing.assert_array_equal(k >> u(16), (nseg - ids).astype(u))
    lens = np.diff(offs)
    live = np.flatnonzero(lens)
    lo = np.minimum.reduceat(k, (offs[:-1] - offs[0])[live])
    hi = np.maximum.reduceat(k, (offs[:-1] - offs[0])[live])
    assert (lo[:-1] > hi[1:]).all()  # every key of a segment above every key of the next non-empty one
    assert np.unique(k & u(0xFFFF)).size > 30000  # 16 random bits
    with pytest.raises(AssertionError):
        L.make("opposed_wide", 9, L.offsets_of(np.ones(1 << 16, dtype=np.int64)), 1 << 16, u)
