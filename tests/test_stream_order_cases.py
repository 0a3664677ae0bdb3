"""The case table of the stream-order tests against include/misort.h (no GPU).

Every prototype of the header that takes a ``void* stream`` is either run behind
pending work by a case of tests/stream_order.py, held to the assertion that the
call did not wait, or listed in NOT_ASYNCHRONOUS with the header's own sentence
that says why it is not.  An entry point added to the header without a case
fails here."""
import re

import numpy as np
import pytest

import segment_layouts as SL
import stream_order as SO


def uncovered(header):
    """Prototypes with a stream that have no case and no listed reason."""
    covered = {c.entry for c in SO.CASES} | set(SO.NOT_ASYNCHRONOUS)
    return [p for p in SO.stream_prototypes(header) if p not in covered]


def test_the_parser_finds_the_stream_prototypes():
    protos = SO.stream_prototypes()
    assert len(protos) == len(set(protos)) >= 15
    for must in ("misort_local_sort", "misort_parallel_bitonic_sort_oop", "misort_local_sort_pairs64",
                 "misort_local_sort_segments", "misort_merge_split_tail", "misort_fill_splitmix",
                 "misort_check_sort"):
        assert must in protos
    # no stream: the host-buffer path, the tooling, the pure host functions
    for must_not in ("misort_sort_host", "misort_codec_probe", "misort_pass_probe", "misort_plan",
                     "misort_synchronize"):
        assert must_not not in protos


def test_every_stream_prototype_has_a_case_or_a_reason():
    assert uncovered(SO.header_text()) == []


def test_a_new_stream_prototype_without_a_case_fails():
    new = ("\nint misort_local_sort_triples(misort_ctx* ctx, const void* d_in, void* d_out,\n"
           "                              int64_t n, void* stream);\n")
    header = SO.header_text().replace("#ifdef __cplusplus\n}", new + "#ifdef __cplusplus\n}")
    assert uncovered(header) == ["misort_local_sort_triples"]
    # ... and one without a stream asks for none
    assert uncovered(SO.header_text().replace("#ifdef __cplusplus\n}", new.replace(", void* stream", "") +
                                              "#ifdef __cplusplus\n}")) == []


def test_the_table_names_only_prototypes_of_the_header():
    protos = set(SO.stream_prototypes())
    assert {c.entry for c in SO.CASES} <= protos
    assert set(SO.NOT_ASYNCHRONOUS) <= protos
    # a listed call may have result-only cases, but never counts as asynchronous
    for c in SO.CASES:
        assert c.asynchronous == (c.entry not in SO.NOT_ASYNCHRONOUS)


def test_every_reason_is_the_headers_own_sentence():
    text = SO.squeeze(SO.header_text())
    for name, (why, sentence) in SO.NOT_ASYNCHRONOUS.items():
        assert why in ("host-waiting", "collective"), name
        assert SO.squeeze(sentence) in text, f"{name}: the header does not say {sentence!r}"
        assert re.search(SO.SAYS_IT_WAITS, sentence), f"{name}: {sentence!r} does not say that the call waits"
    for name, sentence in SO.SYNCHRONOUS_NO_STREAM.items():
        assert name not in SO.stream_prototypes() and SO.squeeze(sentence) in text, name
        assert re.search(SO.SAYS_IT_WAITS, sentence), name
    assert SO.squeeze(SO.COLLECTIVE_WAIT) in text
    assert "At P = 1 everything is enqueued on `stream`" in text  # why the lone-context cases assert the query
    assert "calls are asynchronous on it unless stated otherwise" in text


def test_the_multi_stream_rule_is_documented():
    text = SO.squeeze(SO.header_text())
    assert "Calls on different streams of one context must be ordered by the caller" in text
    import misort
    assert "different streams" in SO.squeeze(misort.Context.__doc__)


def test_the_asynchronous_entry_points_are_all_in_the_table():
    assert {c.entry for c in SO.CASES if c.asynchronous} == {
        "misort_local_sort", "misort_parallel_bitonic_sort", "misort_parallel_bitonic_sort_oop",
        "misort_local_sort_pairs", "misort_local_sort_pairs64", "misort_local_sort_rows",
        "misort_local_sort_rows_pairs", "misort_merge_split", "misort_merge_split_tail", "misort_fill_splitmix"}
    assert len({c.name for c in SO.REPEATED}) >= 14  # one shape per Python entry point for the stream variants


def test_the_segments_layout_has_tile_classes_and_a_long_class():
    import misort
    for kb in (4, 8):
        t = misort.tile_log2(kb)
        offs, n = SL.layout(SO.SEGMENTS_LAYOUT, kb)
        cls = set(SL.classes_of(np.diff(offs), kb).tolist())
        assert any(5 <= c <= t for c in cls) and any(c > t for c in cls) and -1 in cls
        # ... and no other named layout has a long class, so it is the smallest that does
        for other in SL.LAYOUTS:
            if other != SO.SEGMENTS_LAYOUT:
                o, _ = SL.layout(other, kb)
                assert max(SL.classes_of(np.diff(o), kb).tolist()) <= t, other


@pytest.mark.parametrize("cs", SO.CASES, ids=repr)
def test_a_case_is_consistent(cs):
    """Every expected pattern has its buffer's size, the real inputs differ from
    the poison, and no expected output equals what the buffer held before."""
    stage, call, expect, value_check = cs.build()
    assert set(expect) == set(stage) or cs.name.endswith("-new")
    for name, b in stage.items():
        n = int(np.prod(b.shape, dtype=np.int64))
        want = SO.bits(expect[name])
        assert want.size == n, name
        if b.host is not None:
            assert SO.bits(b.host).any(), f"{name}: the real data is all zeros, like the poison"
            assert not np.array_equal(want, np.zeros_like(want)), name
        else:
            assert not np.array_equal(want, SO.out_fill(n, b.dtype)), name
