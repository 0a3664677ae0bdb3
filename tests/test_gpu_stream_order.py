"""Every entry point with a stream, behind work that has not run yet
(tests/stream_order.py holds the harness, the case table and why).

The call's inputs hold poison when it is issued; a producer keeps the stream
busy, the real data is copied in behind it, the call is queued behind that, and
nothing but that stream is waited for.  A step of the call that is not ordered
on the caller's stream reads poison, or is overwritten by the late copy, and the
result differs from the oracle.  Calls the header declares asynchronous must
also return while the producer's event is still pending: that they did not wait,
and that the window was open, is asserted, never assumed.  Every comparison is
on bit patterns."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import segment_layouts as SL
import stream_order as SO
from sort_oracles import order_of, pairs_oracle, want_rows_pairs
from stream_order import F64, U32, U64, In, Out

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def calibration(ctx):
    cal = SO.calibrate()
    yield cal
    ms = cal["producer_ms"]
    if ms:
        print(f"\nstream_order: producer by {cal['kind']}, "
              f"{cal.get('cycles_per_ms', cal.get('ms_per_sort')):.6g} {'cycles/ms' if cal['kind'] == 'sleep' else 'ms/sort'}; "
              f"{len(ms)} producers asked for {SO.PRODUCER_MS} ms took min {min(ms):.1f} / median "
              f"{float(np.median(ms)):.1f} / max {max(ms):.1f} ms to their ready event")


@pytest.fixture(scope="module")
def side(ctx):
    """A stream that is neither torch's default nor the context's own."""
    return torch.cuda.Stream()


def check(cs, res, expect, value_check):
    SO.compare(res, expect, cs.name)
    if value_check:
        value_check(res.value)
    if cs.asynchronous:
        assert res.not_ready, f"{cs.name}: {SO.lost_sensitivity(res)}"


# ---- every entry point behind pending work -----------------------------------------------------------

@pytest.mark.parametrize("cs", SO.CASES, ids=repr)
def test_behind_pending_work(ctx, side, cs):
    SO.warm(ctx, cs, side)
    check(cs, *SO.run_case(ctx, cs, side))


@pytest.mark.parametrize("cs", SO.REPEATED, ids=repr)
def test_on_the_contexts_own_stream(ctx, cs):
    """stream = the context's own; the producer is queued through an ExternalStream of it."""
    own = torch.cuda.ExternalStream(ctx.native_stream)
    SO.warm(ctx, cs, own)
    check(cs, *SO.run_case(ctx, cs, own))


@pytest.mark.parametrize("cs", SO.REPEATED, ids=repr)
def test_on_the_current_stream(ctx, side, cs):
    """stream=None inside ``with torch.cuda.stream(st)``: the wrapper takes the current stream."""
    SO.warm(ctx, cs, side, "current")
    check(cs, *SO.run_case(ctx, cs, side, "current"))


@pytest.mark.parametrize("cs", SO.REPEATED, ids=repr)
def test_with_the_profiler(ctx, side, cs):
    """Profiled launches behind pending work: the same record kinds and counts as a synchronised run."""
    def launches():
        return {k: v[0] for k, v in ctx.profile_read().items() if v[0]}
    ctx.profile(True)
    try:
        SO.warm(ctx, cs, side)
        ctx.profile_reset()
        SO.warm(ctx, cs, side)  # the synchronised run
        want = launches()
        ctx.profile_reset()
        res, expect, value_check = SO.run_case(ctx, cs, side)
        got = launches()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    check(cs, res, expect, value_check)
    assert got == want


def test_negative_control_a_misordered_call_fails_the_comparison(ctx, side):
    """The producer and the staged copy on stream A, the call on stream B, nothing
    ordering them: the sort reads the poison.  Its output is the sorted poison
    (zeros) and differs from the oracle -- what a step of the library on the
    wrong stream would look like.  Only allocated memory is read.

    The control needs A and B on different hardware queues.  B is the module's
    side stream and A a near neighbour of it in torch's pool; the runtime deals
    streams to its queues in turn, so near neighbours differ.  Where they do
    not, the first assertion on the snapshot says so."""
    cs = SO.BY_NAME["local_sort-u32-oop"]
    SO.warm(ctx, cs, side)
    res, expect, _ = SO.run_case(ctx, cs, side, producer_stream=torch.cuda.Stream())
    assert res.not_ready, SO.lost_sensitivity(res)
    # the call saw the poison ...
    assert not res.snap["inp"].any(), (
        "the call on stream B ran after the copy queued on stream A although nothing orders them: the two "
        "streams share a hardware queue (GPU_MAX_HW_QUEUES caps them; a process with more streams than queues "
        "doubles up), so B was serialised behind A's producer.  That says nothing about the library; it means "
        "that a misordered step on such a pair of streams would pass the other tests of this file unseen.")
    for got in (res.snap["out"], res.live["out"]):
        assert not got.any()  # ... and sorted it
        assert not np.array_equal(got, expect["out"])
    with pytest.raises(AssertionError):
        SO.compare(res, expect, cs.name)
    np.testing.assert_array_equal(res.live["inp"], expect["inp"])  # the copy landed afterwards


# ---- sequences with no host wait ------------------------------------------------------------------------

N_BIG = (1 << 20) + 3
ROWS, COLS = 127, 8193  # the rows of 8193 keys that fit into N_BIG
SEED = 0x5EED0A11
SEG_LENS = [40, 0, 700, 1, 40000, 64, 9, 8193]
NA, NB = 100000, 99999


@functools.lru_cache(maxsize=None)
def chain_data(salt=0):
    """(stage, expected bit patterns per step) of the chain; computed once per
    ``salt``, which moves every seed: the same shapes with other data."""
    fill = O.splitmix(SEED + salt, N_BIG, U64)
    srt = np.sort(fill)
    rowsorted = fill.copy()
    rowsorted[:ROWS * COLS] = np.sort(fill[:ROWS * COLS].reshape(ROWS, COLS), axis=1).reshape(-1)
    small = SO.rand(1 + salt, 5000, U32)
    pk, pv = SO.tied_u32(2 + salt, SO.NPAIRS), SO.rand(3 + salt, SO.NPAIRS, U32)
    rk, rv = SO.tied_u32(4 + salt, (3, 10000)), SO.rand(5 + salt, (3, 10000), U32) & U32(7)
    fk = SO.f64_keys(6 + salt, SO.N64)
    offs = SL.offsets_of(SEG_LENS)
    sk = SL.make("dups", 7 + salt, offs, int(offs[-1]), U32)
    stage = {"A": Out(N_BIG, U64), "B": Out(N_BIG, U64), "idx": Out(N_BIG, U32),
             "small_in": In(small), "small_out": Out(small.size, U32),
             "pk": In(pk), "pv": In(pv), "pok": Out(pk.size, U32), "pov": Out(pk.size, U32),
             "rk": In(rk), "rv": In(rv), "rok": Out(rk.shape, U32), "rov": Out(rk.shape, U32),
             "cs": Out(NA, U64), "fk": In(fk), "fo": Out(fk.size, F64),
             "sk": In(sk), "offs": In(offs), "so": Out(sk.size, U32)}
    wpk, wpv = pairs_oracle(pk, pv)
    wrk, wrv = want_rows_pairs(rk, rv)
    want = {
        "fill": {"A": fill},
        "sort": {"A": fill, "B": srt},
        "rows": {"A": rowsorted, "B": srt},
        "argsort64": {"A": rowsorted, "idx": order_of(rowsorted).astype(U32)},
        "small": {"small_in": small, "small_out": np.sort(small)},
        "pairs": {"pk": pk, "pv": pv, "pok": wpk, "pov": wpv},
        "rows_pairs": {"rk": rk, "rv": rv, "rok": wrk, "rov": wrv},
        "compare_split": {"B": srt, "cs": O.compare_split(np.ascontiguousarray(srt[:NA]),
                                                          np.ascontiguousarray(srt[N_BIG - NB:]), 1)},
        "f64": {"fk": fk, "fo": SO.sorted_bits(fk)},
        "segments": {"sk": sk, "offs": offs, "so": SL.want(sk, offs, U32)},
    }
    return stage, want


def rows_view(t):
    return t["A"][:ROWS * COLS].view(ROWS, COLS)


STEPS = {  # name -> call(ctx, tensors, stream handle, salt); every step but the last is asynchronous
    "fill": lambda c, t, s, salt: c.fill_splitmix(t["A"], SEED + salt, 0, stream=s),
    "sort": lambda c, t, s, salt: c.local_sort(t["A"], t["B"], stream=s),
    "rows": lambda c, t, s, salt: c.sort_rows(rows_view(t), out=rows_view(t), stream=s),
    "argsort64": lambda c, t, s, salt: c.argsort64(t["A"], t["idx"], stream=s),
    "small": lambda c, t, s, salt: c.local_sort(t["small_in"], t["small_out"], stream=s),  # pong and fences, far smaller
    "pairs": lambda c, t, s, salt: c.sort_pairs(t["pk"], t["pv"], t["pok"], t["pov"], stream=s),
    "rows_pairs": lambda c, t, s, salt: c.sort_rows_pairs(t["rk"], t["rv"], t["rok"], t["rov"], stream=s),
    "compare_split": lambda c, t, s, salt: c.compare_split(t["B"][:NA], t["B"][N_BIG - NB:], 1, out=t["cs"], stream=s),
    "f64": lambda c, t, s, salt: c.local_sort(t["fk"], t["fo"], stream=s),
    "segments": lambda c, t, s, salt: c.sort_segments(t["sk"], t["offs"], out=t["so"], stream=s),  # waits: last
}
LARGE_TO_SMALL = ["fill", "sort", "rows", "argsort64", "small", "pairs", "rows_pairs", "compare_split", "f64",
                  "segments"]
SMALL_TO_LARGE = ["small", "rows_pairs", "f64", "pairs", "fill", "sort", "rows", "argsort64", "compare_split",
                  "segments"]


def run_chain(c, streams, order, pending_work=True, salt=0):
    """The chain on ``streams`` (step i on streams[i % len]; with two, every step
    waits for an event recorded after the step before it and its snapshot).
    Every step's tensors are cloned on its stream right after it.  Only the
    final waits for the streams wait on the host.  Returns (snapshots, the
    ready.query() right after the last asynchronous call returned, producer ms)."""
    stage, want = chain_data(salt)
    assert order[-1] == "segments" and sorted(order) == sorted(STEPS)
    live, staged = SO.allocate(stage)
    with torch.cuda.stream(streams[0]):
        pending = SO.queue_producer(live, staged, SO.PRODUCER_MS if pending_work else 0.01)
        prev = torch.cuda.Event()
        prev.record()
    snaps, not_ready = {}, None
    for i, name in enumerate(order):
        st = streams[i % len(streams)]
        if len(streams) > 1:
            st.wait_event(prev)
        if name == "segments":
            not_ready = pending.query() is False  # after the last asynchronous call
        with torch.cuda.stream(SO.elsewhere()):  # the calls get their stream as an argument only
            STEPS[name](c, live, st.cuda_stream, salt)
        with torch.cuda.stream(st):
            snaps[name] = {k: live[k].clone() for k in want[name]}
            if len(streams) > 1:
                prev = torch.cuda.Event()
                prev.record()
    for st in streams:
        st.synchronize()
    with torch.cuda.stream(streams[0]):
        host = {name: {k: SO.host_bits(v) for k, v in snap.items()} for name, snap in snaps.items()}
        streams[0].synchronize()
    return host, not_ready, pending.producer_ms()


def check_chain(host, order, salt=0):
    _, want = chain_data(salt)
    for name in order:
        for k, w in want[name].items():
            np.testing.assert_array_equal(host[name][k], SO.bits(w), err_msg=f"after {name}: {k}")


def test_chain_on_a_warm_context(ctx, side):
    """Ten calls of different entry points, key widths and sizes back to back on
    one stream behind the producer: pong, bounce, the record buffers, the fence
    and planning scratch and the merge passes' counters are reused with no host
    wait in between, and the host is ahead of the device all the way."""
    # grows every buffer (other data: the scratch must not be left holding this run's answers); checked too
    host, _, _ = run_chain(ctx, [side], LARGE_TO_SMALL, pending_work=False, salt=SO.WARM_SALT)
    check_chain(host, LARGE_TO_SMALL, SO.WARM_SALT)
    host, not_ready, ms = run_chain(ctx, [side], LARGE_TO_SMALL)
    check_chain(host, LARGE_TO_SMALL)
    assert not_ready, (f"the producer's event had completed after the chain's last asynchronous call returned: "
                       f"a call waited, or the producer ({ms:.1f} ms measured) is too short")


@pytest.mark.parametrize("order", [LARGE_TO_SMALL, SMALL_TO_LARGE], ids=["large_to_small", "small_to_large"])
def test_chain_on_a_fresh_context(side, order):
    """The context's buffers grow behind queued work (small to large: over and
    over).  Growing may wait for the device; the results must not change."""
    c = misort.Context(0)
    try:
        host, _, _ = run_chain(c, [side], order)
        check_chain(host, order)
    finally:
        c.close()


def test_chain_alternating_between_two_streams(ctx, side):
    """The chain's calls alternate between two streams of one context, ordered by
    events the test records and waits on: the context's buffers are shared, the
    merge scratch is per stream."""
    host, _, _ = run_chain(ctx, [side, torch.cuda.Stream()], LARGE_TO_SMALL)
    check_chain(host, LARGE_TO_SMALL)


# ---- with a communicator --------------------------------------------------------------------------------

def group_run(p, rank_fn):
    SO.calibrate()  # on this thread, before the ranks' threads need it
    g = misort.Group(p)
    try:
        return g.run(rank_fn)
    finally:
        g.close()


@pytest.mark.parametrize("malformed", [False, True], ids=["well_formed", "malformed"])
def test_sort_segments_with_a_communicator(ctx, malformed):
    """misort_local_sort_segments on a context of a 2-rank group, on the context's
    own stream with the producer pending: its one wait goes through the
    transport.  Malformed offsets (written by the producer: the poison is well
    formed) make every rank raise, and ``out`` is unchanged."""
    offs = SL.offsets_of(SEG_LENS)
    n = int(offs[-1])
    keys = [SL.make("dups", 200 + r, offs, n, U32) for r in range(2)]
    bad = offs.copy()
    bad[3], bad[4] = offs[4], offs[3]  # 741 before 740: offsets[3] > offsets[4]

    def rank_fn(r, c):
        own = torch.cuda.ExternalStream(c.native_stream)
        stage = {"inp": In(keys[r]), "offs": In(bad if malformed else offs), "out": Out(n, U32)}

        def call(t):
            if not malformed:
                c.sort_segments(t["inp"], t["offs"], out=t["out"], stream=c.native_stream)
                return None
            with pytest.raises(misort.MisortError) as e:
                c.sort_segments(t["inp"], t["offs"], out=t["out"], stream=c.native_stream)
            return e.value.code
        return SO.behind_pending_work(own, stage, call)

    for r, res in enumerate(group_run(2, rank_fn)):
        out = SO.out_fill(n, U32) if malformed else SL.want(keys[r], offs, U32)
        SO.compare(res, {"inp": keys[r], "offs": bad if malformed else offs, "out": out}, f"rank {r}")
        assert res.value == (-1 if malformed else None)


@pytest.mark.parametrize("p,dt", [(2, U32), (4, U32), (2, F64)], ids=["p2-u32", "p4-u32", "p2-f64"])
def test_parallel_bitonic_sort_with_a_communicator(ctx, p, dt):
    """Every rank's block is written by a producer pending on that rank's stream;
    the collective waits by contract, so there is no query assertion."""
    n = 100003
    x = O.generate_f64(n) if dt == F64 else O.splitmix(0xB170 + p, n, U32)
    want = O.parallel_bitonic_sort(x, p)
    sizes = [int(v) for v in misort.block_sizes(n, p)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    max_size = n // p + 1

    def rank_fn(r, c):
        own = torch.cuda.ExternalStream(c.native_stream)
        block = np.concatenate([x[offs[r]:offs[r + 1]], np.ones(max_size - sizes[r], x.dtype)])
        res = SO.behind_pending_work(own, {"buf": In(block)}, lambda t: SO._void(
            c.parallel_bitonic_sort(t["buf"], sizes[r], max_size, stream=c.native_stream)))
        return res, block

    for r, (res, block) in enumerate(group_run(p, rank_fn)):
        SO.compare(res, {"buf": np.concatenate([want[offs[r]:offs[r + 1]], block[sizes[r]:]])}, f"rank {r} of {p}")
