"""Stream order of the asynchronous entry points -- the harness and the case
table of tests/test_gpu_stream_order.py (no pytest in here; torch is imported
only where a GPU is used, so tests/test_stream_order_cases.py reads the table
on a machine without one).

include/misort.h promises that a call is asynchronous on ``stream``: it may be
queued behind work that has not run yet, and what follows it on the stream sees
its result.  ``behind_pending_work`` puts that to the test.  The call's inputs
hold *poison* when it is issued; a *producer* that keeps the stream busy for
PRODUCER_MS is queued first, then copies of the real data into the inputs, then
an event ``ready``.  The call is then given that stream, while torch's current
stream is another, idle one (``elsewhere``; only the ``stream=None`` variant
makes the stream current), ``ready.query()`` is read as soon as the call
returns, every tensor is cloned on the stream, and only that stream is waited
for.  An internal step on another stream (a bounce copy, a
conversion sweep, a record-forming kernel, a torch op of the wrapper) then
reads poison or is overwritten by the late copy, and the clones or the live
tensors differ from the oracle.  Poison is always a legal input of the same
call -- zeros: a sorted block, legal values, well-formed offsets with every
segment empty -- so a misordered step gives a wrong answer, never an access out
of bounds.

``ready.query() is False`` after the call returned is what the tests assert of
every call the header declares asynchronous: the call did not wait for the
stream, and the window in which a misordered step would have run early was
open.  PRODUCER_MS is the sensitivity knob behind it, not an asserted quantity.

CASES is the table: one Case per (entry point, shape, buffer layout); ``entry``
is the C prototype it runs.  NOT_ASYNCHRONOUS lists every prototype with a
``void* stream`` that the query assertion does not apply to, each with the
sentence of the header that says why; tests/test_stream_order_cases.py holds the
two against the header's prototypes.
"""
import functools
import os
import re

import numpy as np

import oracle_lib as O
import segment_layouts as SL
from guard_bands import kmap as kmap64, kunmap as kunmap64
from sort_oracles import argsort_oracle, order_of, pairs_oracle, want_rows, want_rows_pairs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "misort.h")

PRODUCER_MS = 50.0  # how long the producer keeps the stream busy: a sensitivity knob, never asserted
OUT_FILL = 0x5A     # every byte of an output before the call (the inputs' poison is zero)

U32, U64, F32, F64 = np.uint32, np.uint64, np.float32, np.float64
N32 = (1 << 17) + 9   # u32 keys: SORT tiles plus one multi-way pass
N64 = (1 << 16) + 3   # u64 / f64 keys: the same
NPAIRS = 131073       # pairs: the first multi-way pass of the u64 records


# ---- the header ----------------------------------------------------------------------------------------

def header_text():
    with open(HEADER) as f:
        return f.read()


def squeeze(text):
    """Comment text as one line: comment stars and runs of white space dropped."""
    return re.sub(r"\s+", " ", re.sub(r"(?m)^\s*/?\*+/?", " ", text)).strip()


def stream_prototypes(text=None):
    """The names of the header's prototypes that take a ``void* stream``, in order."""
    text = header_text() if text is None else text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(misort_\w+)\s*\(([^;{}]*?)\)\s*;", code)
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]


# Prototypes with a stream that are NOT held to the query assertion: name ->
# (why, the header's sentence).  The host-waiting ones keep every other assertion
# of their cases; the collectives wait by contract at P > 1 and the header
# tells callers not to rely on anything else at P = 1.  Every sentence must say
# that the call waits or is not asynchronous (SAYS_IT_WAITS).
SAYS_IT_WAITS = r"Not asynchronous|Synchronous|HOST WAIT"
NOT_ASYNCHRONOUS = {
    "misort_local_sort_segments": (
        "host-waiting", "ONE HOST WAIT PER CALL."),
    "misort_check_sort": (
        "host-waiting", "Synchronous; *errors is valid on every rank."),
    "misort_parallel_quick_sort": (
        "collective", "Not asynchronous: at P > 1 the host waits on `stream` several times in every round"),
    "misort_parallel_sample_sort": (
        "collective", "Not asynchronous: at P > 1 the host waits on `stream` (block sizes, samples and the "
                      "all-to-all-v counts are read back)"),
    "misort_parallel_sort_pairs": (
        "collective", "Not asynchronous: at P > 1 the host waits on `stream` as misort_parallel_bitonic_sort does"),
}
# Host-waiting without a stream parameter (the context's own stream): listed for
# completeness, there is nothing to queue it behind.
SYNCHRONOUS_NO_STREAM = {"misort_sort_host": "host h_out (this rank's block, parallel sort over the communicator). Synchronous."}
# misort_parallel_bitonic_sort(_oop) are in CASES on a lone context ("At P = 1
# everything is enqueued on `stream`"); with a communicator they wait:
COLLECTIVE_WAIT = "at P > 1 the host waits on the stream at the start (size exchange) and once per stage"


# ---- buffers of a call ---------------------------------------------------------------------------------

class In:
    """An input: ``host`` is the real data (any shape).  The device tensor holds
    poison (zeros) until the producer's copy lands; ``lead`` elements of storage
    precede it (1: a view that is not 16-byte aligned)."""

    def __init__(self, host, lead=0):
        self.host, self.lead = np.ascontiguousarray(host), lead
        self.shape, self.dtype = self.host.shape, self.host.dtype


class Out:
    """An output of ``shape`` elements of numpy ``dtype``, every byte OUT_FILL before the call."""

    def __init__(self, shape, dtype, lead=0):
        self.shape = (shape,) if np.isscalar(shape) else tuple(shape)
        self.dtype, self.lead, self.host = np.dtype(dtype), lead, None


def bits(a):
    """The bit patterns of a host array, flat, as the unsigned type of its width."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: U32, 8: U64}[a.dtype.itemsize])


def out_fill(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, OUT_FILL, np.uint8).view({4: U32, 8: U64}[np.dtype(dtype).itemsize])


def _storage(dtype):
    """Device storage of a numpy dtype: unsigned keys live in signed tensors."""
    return {np.dtype(U32): np.int32, np.dtype(U64): np.int64}.get(np.dtype(dtype), np.dtype(dtype).type)


def _torch_dtype(dtype):
    import torch
    return {np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32,
            np.float64: torch.float64}[_storage(dtype)]


def host_bits(t):
    """The bit patterns of a device tensor on the host, flat (no device-wide wait: the
    copy runs on the current stream, after work that the caller has waited for)."""
    import torch
    it = {4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it).reshape(-1).cpu().numpy().view({4: U32, 8: U64}[t.element_size()])


# ---- the producer --------------------------------------------------------------------------------------

_CAL = {}


def calibrate():
    """Once per session: how to keep a stream busy for a given time.  With
    torch.cuda._sleep, its cycles per millisecond (two events around one sleep);
    else the time of one torch sort of 2^22 keys, which the producer chains."""
    import torch
    if _CAL:
        return _CAL
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        probe = 20_000_000
        torch.cuda._sleep(1000)  # loads the kernel
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _CAL.update(kind="sleep", cycles_per_ms=probe / max(a.elapsed_time(b), 1e-3))
    else:
        busy = torch.randint(0, 1 << 30, (1 << 22,), dtype=torch.int32, device="cuda")
        busy.sort()
        torch.cuda.synchronize()
        a.record()
        for _ in range(4):
            busy.sort()
        b.record()
        b.synchronize()
        _CAL.update(kind="sorts", ms_per_sort=a.elapsed_time(b) / 4, busy=busy)
    _CAL["producer_ms"] = []  # every producer time measured since
    return _CAL


def keep_busy(ms):
    """Queues about ``ms`` milliseconds of work on torch's current stream."""
    import torch
    cal = calibrate()
    if cal["kind"] == "sleep":
        torch.cuda._sleep(int(ms * cal["cycles_per_ms"]))
    else:
        for _ in range(max(1, int(np.ceil(ms / cal["ms_per_sort"])))):
            cal["busy"].sort()


class Pending:
    """A producer in flight: ``ready`` is recorded after its copies."""

    def __init__(self, t0, ready, asked):
        self.t0, self.ready, self.asked = t0, ready, asked

    def query(self):
        """False while the producer, or a copy behind it, has not finished."""
        return self.ready.query()

    def producer_ms(self):
        """The measured time from the producer's start to ``ready`` (after a wait
        for it); kept for the session's report when PRODUCER_MS was asked for."""
        ms = self.t0.elapsed_time(self.ready)
        if self.asked == PRODUCER_MS:
            calibrate()["producer_ms"].append(ms)
        return ms


def allocate(stage):
    """(live, staged) device tensors of a stage: inputs as poison, outputs as
    OUT_FILL, the real data in staging tensors; waits for torch's current
    stream, on which it did this, and for nothing else."""
    import torch
    live, staged = {}, {}
    for name, b in stage.items():
        n = int(np.prod(b.shape, dtype=np.int64))
        base = torch.empty(b.lead + n, dtype=_torch_dtype(b.dtype), device="cuda")
        base.view(torch.uint8).fill_(0 if b.host is not None else OUT_FILL)
        live[name] = base[b.lead:b.lead + n].view(b.shape)
        if b.host is not None:
            staged[name] = torch.from_numpy(b.host.view(_storage(b.dtype))).cuda()
    torch.cuda.current_stream().synchronize()  # setup only
    return live, staged


def queue_producer(live, staged, ms=PRODUCER_MS):
    """On torch's current stream: the producer, the copies staged -> live, ``ready``."""
    import torch
    t0, ready = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    keep_busy(ms)
    for name, src in staged.items():
        live[name].copy_(src)
    ready.record()
    return Pending(t0, ready, ms)


_ELSEWHERE = []


def elsewhere():
    """An idle stream that no test queues work on: torch's current stream while
    a call with an explicit ``stream=`` is issued.  A torch op of the wrapper
    that runs on the current stream instead of ``stream`` lands here, ahead of
    the producer, and shows like any other misordered step."""
    import torch
    if not _ELSEWHERE:
        _ELSEWHERE.append(torch.cuda.Stream())
    return _ELSEWHERE[0]


class Result:
    """snap / live: {name: host bit patterns} of every tensor, cloned on the stream
    right after the call / read after the wait; not_ready: ``ready.query()`` was
    False when the call returned; producer_ms: measured; value: what the call returned."""


def behind_pending_work(stream, stage, call, producer_stream=None, ms=PRODUCER_MS, current="elsewhere"):
    """Runs ``call(live)``, which passes ``stream`` (a torch stream) to the
    library, behind a producer pending on that stream.  ``stream`` is torch's
    current stream only while the producer is queued and the clones are taken;
    the call itself is issued with ``elsewhere()`` current, or, with
    ``current="stream"`` (the calls that pass ``stream=None``), with ``stream``.
    ``stage`` is {name: In | Out}; ``call`` gets {name: device tensor} and may
    return {name: tensor} of outputs that it allocated, which are snapshotted
    with the rest.  ``producer_stream``: queue the producer and the copies
    there instead (the negative control: nothing then orders the call behind
    them)."""
    import torch
    live, staged = allocate(stage)
    with torch.cuda.stream(producer_stream or stream):
        pending = queue_producer(live, staged, ms)
    res = Result()
    with torch.cuda.stream(stream if current == "stream" else elsewhere()):
        res.value = call(live)
        res.not_ready = pending.query() is False
    with torch.cuda.stream(stream):
        if isinstance(res.value, dict):
            live.update(res.value)
        snap = {k: v.clone() for k, v in live.items()}
        stream.synchronize()
        if producer_stream is not None:
            producer_stream.synchronize()
        res.snap = {k: host_bits(v) for k, v in snap.items()}
        res.live = {k: host_bits(v) for k, v in live.items()}
        stream.synchronize()
    res.producer_ms = pending.producer_ms()
    return res


def lost_sensitivity(res):
    return (f"the producer's event had completed when the call returned: the call waited for the stream, or "
            f"the producer ({res.producer_ms:.1f} ms measured, {PRODUCER_MS} ms asked, calibration "
            f"{ {k: v for k, v in calibrate().items() if k in ('kind', 'cycles_per_ms', 'ms_per_sort')} }) "
            f"is too short to tell")


# ---- inputs ----------------------------------------------------------------------------------------------

def rand(seed, shape, dt):
    return np.random.default_rng(seed).integers(0, np.iinfo(dt).max, size=shape, dtype=dt, endpoint=True)


def tied_u32(seed, shape):
    """Random u32 keys, a third of them from 16 values: the values decide their order."""
    rng = np.random.default_rng(seed)
    k = rand(seed + 1, shape, U32)
    k[rng.random(shape) < 1 / 3] &= U32(0xF)
    return k


F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,  # +-0, +-inf, denormals
                        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], dtype=U32)  # NaNs
F64_SPECIAL = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x0000000000000001, 0x8000000000000001, 0x7FF8000000000000, 0xFFF8000000000000,
                        0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=U64)


def f32_keys(seed, shape):
    """float32 keys of both signs, a quarter of them +-0.0, +-inf, denormals and NaNs of both signs."""
    rng = np.random.default_rng(seed)
    k = (rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, shape)).astype(F32).view(U32)
    pick = rng.random(shape) < 0.25
    k[pick] = F32_SPECIAL[rng.integers(0, F32_SPECIAL.size, int(pick.sum()))]
    return k.view(F32)


def f64_keys(seed, shape, dups=False):
    """float64 keys of both signs with the specials; ``dups``: from 40 values only."""
    rng = np.random.default_rng(seed)
    k = (rng.standard_normal(shape) * 10.0 ** rng.integers(-300, 300, shape)).view(U64)
    if dups:
        pool = np.concatenate([F64_SPECIAL, k.reshape(-1)[:28]])
        return pool[rng.integers(0, pool.size, shape)].view(F64)
    pick = rng.random(shape) < 0.25
    k[pick] = F64_SPECIAL[rng.integers(0, F64_SPECIAL.size, int(pick.sum()))]
    return k.view(F64)


def few_few(seed, n):
    """u64 keys with 4 values in each half: stability is the whole test."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, n, dtype=U64) << U64(32) | rng.integers(0, 4, n, dtype=U64)


def keys_of(dt, seed, shape):
    return f64_keys(seed, shape) if dt == F64 else f32_keys(seed, shape) if dt == F32 else rand(seed, shape, dt)


def sorted_bits(x):
    """The local sort's oracle on bit patterns: numpy's sort of the ordered patterns."""
    if x.dtype == F64:
        return kunmap64(np.sort(kmap64(x.reshape(-1))))
    return np.sort(x.reshape(-1))


def sorted_block(dt, seed, n):
    """A sorted block of keys above zero (so that it differs from the poison)."""
    if dt == F64:
        return np.sort(np.abs(np.random.default_rng(seed).standard_normal(n)) + 1e-9)
    return np.sort(1 + rand(seed, n, dt) % dt(1 << 30))


def descents(a):
    """check_sort's count: positions i with a[i] > a[i + 1] (a NaN on either side is none)."""
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(a[:-1] > a[1:]))


# ---- the case table --------------------------------------------------------------------------------------

class Case:
    """name; entry: the C prototype; build(salt=0) -> (stage, call(ctx, tensors,
    stream), expect {name: bit patterns}, value_check or None), ``salt`` moves
    every seed: the same shapes with other data; rep: the one case of its Python
    entry point that the stream variants repeat."""

    def __init__(self, name, entry, build, rep=False):
        self.name, self.entry, self.rep = name, entry, rep
        self.build = functools.lru_cache(maxsize=None)(build)

    @property
    def asynchronous(self):
        return self.entry not in NOT_ASYNCHRONOUS

    def __repr__(self):
        return self.name


CASES = []


def case(name, entry, rep=False):
    def add(build):
        CASES.append(Case(name, entry, build, rep))
        return build
    return add


def _void(result):
    """A call whose outputs are all in the stage returns nothing to the harness."""
    return None


DT_NAME = {U32: "u32", U64: "u64", F32: "f32", F64: "f64"}
N_OF = {U32: N32, U64: N64, F64: N64}


def _local_sort(dt, mode):
    leads = {"oop": (0, 0), "view_in": (1, 0), "view_out": (0, 1), "view_both": (1, 1)}

    def build(salt=0):
        x = keys_of(dt, 11 + salt, N_OF[dt])
        if mode == "in_place":
            return ({"keys": In(x)}, lambda c, t, s: _void(c.local_sort(t["keys"], stream=s)),
                    {"keys": sorted_bits(x)}, None)
        li, lo = leads[mode]
        return ({"inp": In(x, li), "out": Out(x.size, dt, lo)},
                lambda c, t, s: _void(c.local_sort(t["inp"], t["out"], stream=s)),
                {"inp": bits(x), "out": sorted_bits(x)}, None)
    return build


for _dt in (U32, U64, F64):
    for _mode in ("oop", "in_place", "view_in", "view_out", "view_both"):
        case(f"local_sort-{DT_NAME[_dt]}-{_mode}", "misort_local_sort",
             rep=(_dt, _mode) == (U32, "view_both"))(_local_sort(_dt, _mode))


def _bitonic(dt, mode):
    def build(salt=0):
        n = N_OF[dt]
        x = keys_of(dt, 12 + salt, n + (5 if mode == "tail5" else 0))
        if mode == "out":
            return ({"inp": In(x), "out": Out(n, dt)},
                    lambda c, t, s: _void(c.parallel_bitonic_sort(t["inp"], out=t["out"], stream=s)),
                    {"inp": bits(x), "out": sorted_bits(x)}, None)
        want = np.concatenate([sorted_bits(x[:n]), bits(x[n:])])  # the 5 trailing keys stay
        return ({"keys": In(x)}, lambda c, t, s: _void(c.parallel_bitonic_sort(t["keys"], n, stream=s)),
                {"keys": want}, None)
    return build


for _dt in (U32, F64):
    for _mode in ("in_place", "out", "tail5"):
        case(f"parallel_bitonic_sort-{DT_NAME[_dt]}-{_mode}",
             "misort_parallel_bitonic_sort_oop" if _mode == "out" else "misort_parallel_bitonic_sort",
             rep=_dt == F64 and _mode != "tail5")(_bitonic(_dt, _mode))


def _pairs(dt, lead=0):
    def build(salt=0):
        keys = f32_keys(21 + salt, NPAIRS) if dt == F32 else tied_u32(21 + salt, NPAIRS)
        vals = rand(22 + salt, NPAIRS, U32)
        vals[np.random.default_rng(23 + salt).random(NPAIRS) < 0.5] &= U32(3)  # equal keys meet equal and unequal values
        wk, wv = pairs_oracle(keys, vals)
        return ({"keys": In(keys, lead), "vals": In(vals, lead), "ok": Out(NPAIRS, dt, lead), "ov": Out(NPAIRS, U32, lead)},
                lambda c, t, s: _void(c.sort_pairs(t["keys"], t["vals"], t["ok"], t["ov"], stream=s)),
                {"keys": bits(keys), "vals": vals, "ok": wk, "ov": wv}, None)
    return build


def _argsort(dt):
    def build(salt=0):
        keys = f32_keys(24 + salt, NPAIRS) if dt == F32 else rand(24 + salt, NPAIRS, U32) % U32(5)
        return ({"keys": In(keys), "idx": Out(NPAIRS, U32)},
                lambda c, t, s: _void(c.argsort(t["keys"], t["idx"], stream=s)),
                {"keys": bits(keys), "idx": argsort_oracle(keys)}, None)
    return build


case("sort_pairs-u32", "misort_local_sort_pairs")(_pairs(U32))
case("sort_pairs-f32", "misort_local_sort_pairs", rep=True)(_pairs(F32))
case("sort_pairs-u32-views", "misort_local_sort_pairs")(_pairs(U32, lead=1))
case("argsort-u32", "misort_local_sort_pairs")(_argsort(U32))
case("argsort-f32", "misort_local_sort_pairs", rep=True)(_argsort(F32))


def _pairs64(dt, vdt, keys_in_place=False):
    def build(salt=0):
        keys = f64_keys(31 + salt, N64, dups=True) if dt == F64 else few_few(31 + salt, N64)
        vals = rand(32 + salt, N64, vdt)
        order = order_of(keys)
        if keys_in_place:
            return ({"keys": In(keys), "vals": In(vals), "ov": Out(N64, vdt)},
                    lambda c, t, s: _void(c.sort_pairs64(t["keys"], t["vals"], t["keys"], t["ov"], stream=s)),
                    {"keys": bits(keys)[order], "vals": vals, "ov": vals[order]}, None)
        return ({"keys": In(keys), "vals": In(vals), "ok": Out(N64, dt), "ov": Out(N64, vdt)},
                lambda c, t, s: _void(c.sort_pairs64(t["keys"], t["vals"], t["ok"], t["ov"], stream=s)),
                {"keys": bits(keys), "vals": vals, "ok": bits(keys)[order], "ov": vals[order]}, None)
    return build


def _argsort64(dt):
    def build(salt=0):
        keys = f64_keys(33 + salt, N64, dups=True) if dt == F64 else few_few(33 + salt, N64)
        return ({"keys": In(keys), "idx": Out(N64, U32)},
                lambda c, t, s: _void(c.argsort64(t["keys"], t["idx"], stream=s)),
                {"keys": bits(keys), "idx": order_of(keys).astype(U32)}, None)
    return build


case("sort_pairs64-u64-v4", "misort_local_sort_pairs64")(_pairs64(U64, U32))
case("sort_pairs64-u64-v8", "misort_local_sort_pairs64")(_pairs64(U64, U64))
case("sort_pairs64-f64-v8", "misort_local_sort_pairs64", rep=True)(_pairs64(F64, U64))
case("sort_pairs64-u64-v4-keys_in_place", "misort_local_sort_pairs64")(_pairs64(U64, U32, keys_in_place=True))
case("argsort64-u64", "misort_local_sort_pairs64", rep=True)(_argsort64(U64))
case("argsort64-f64", "misort_local_sort_pairs64")(_argsort64(F64))


def _rows(dt, rows, cols, mode="oop"):
    def build(salt=0):
        x = keys_of(dt, 41 + salt, (rows, cols))
        want = bits(want_rows(x))
        if mode == "in_place":
            return ({"keys": In(x)}, lambda c, t, s: _void(c.sort_rows(t["keys"], out=t["keys"], stream=s)),
                    {"keys": want}, None)
        if mode == "new":  # the wrapper allocates the output
            return ({"inp": In(x)}, lambda c, t, s: {"out": c.sort_rows(t["inp"], stream=s)},
                    {"inp": bits(x), "out": want}, None)
        lead = 1 if mode == "view" else 0
        return ({"inp": In(x, lead), "out": Out((rows, cols), dt, lead)},
                lambda c, t, s: _void(c.sort_rows(t["inp"], out=t["out"], stream=s)),
                {"inp": bits(x), "out": want}, None)
    return build


for _dt, _r, _c, _mode, _rep in [
        (U32, 37, 1000, "oop", False), (U64, 5, 8192, "new", False),                       # the tile path
        (U32, 3, 40000, "oop", False), (U64, 3, 8193, "oop", False), (F64, 2, 8193, "oop", True),  # padded blocks
        (U32, 37, 1000, "in_place", False), (U64, 3, 8193, "in_place", False),
        (U32, 37, 999, "view", False), (U64, 3, 8193, "view", False)]:               # odd cols, one element in
    case(f"sort_rows-{DT_NAME[_dt]}-{_r}x{_c}-{_mode}", "misort_local_sort_rows", rep=_rep)(_rows(_dt, _r, _c, _mode))


def _rows_pairs(dt, rows, cols, in_place=False):
    def build(salt=0):
        f32 = dt == F32
        keys = f32_keys(51 + salt, (rows, cols)) if f32 else tied_u32(51 + salt, (rows, cols))
        vals = rand(52 + salt, (rows, cols), U32) & U32(7)
        wk, wv = want_rows_pairs(bits(keys).reshape(rows, cols), vals, f32)
        if in_place:
            return ({"keys": In(keys), "vals": In(vals)},
                    lambda c, t, s: _void(c.sort_rows_pairs(t["keys"], t["vals"], t["keys"], t["vals"], stream=s)),
                    {"keys": bits(wk), "vals": bits(wv)}, None)
        return ({"keys": In(keys), "vals": In(vals), "ok": Out((rows, cols), dt), "ov": Out((rows, cols), U32)},
                lambda c, t, s: _void(c.sort_rows_pairs(t["keys"], t["vals"], t["ok"], t["ov"], stream=s)),
                {"keys": bits(keys), "vals": bits(vals), "ok": bits(wk), "ov": bits(wv)}, None)
    return build


def _argsort_rows(dt, rows, cols):
    def build(salt=0):
        f32 = dt == F32
        keys = f32_keys(53 + salt, (rows, cols)) if f32 else rand(53 + salt, (rows, cols), U32) % U32(5)
        _, wi = want_rows_pairs(bits(keys).reshape(rows, cols), None, f32)
        return ({"keys": In(keys), "idx": Out((rows, cols), U32)},
                lambda c, t, s: _void(c.argsort_rows(t["keys"], t["idx"], stream=s)),
                {"keys": bits(keys), "idx": bits(wi)}, None)
    return build


for _dt in (U32, F32):
    for _r, _c in ((37, 1000), (3, 10000)):  # the tile path, padded blocks
        case(f"sort_rows_pairs-{DT_NAME[_dt]}-{_r}x{_c}", "misort_local_sort_rows_pairs",
             rep=(_dt, _r) == (F32, 3))(_rows_pairs(_dt, _r, _c))
        case(f"argsort_rows-{DT_NAME[_dt]}-{_r}x{_c}", "misort_local_sort_rows_pairs",
             rep=(_dt, _r) == (U32, 3))(_argsort_rows(_dt, _r, _c))
case("sort_rows_pairs-u32-37x1000-in_place", "misort_local_sort_rows_pairs")(_rows_pairs(U32, 37, 1000, in_place=True))


def _compare_split(dt, na, nb, keep_max, tail):
    def build(salt=0):
        a, b = sorted_block(dt, 61 + salt, na), sorted_block(dt, 62 + salt, nb)
        want = O.compare_split(a, b, keep_max)
        assert not np.array_equal(want, a)  # the merge changes the block
        return ({"local": In(a), "recv": In(b), "out": Out(na, dt)},
                lambda c, t, s: _void(c.compare_split(t["local"], t["recv"], keep_max, out=t["out"], stream=s,
                                                in_place_tail=tail)),
                {"local": bits(a), "recv": bits(b), "out": bits(want)}, None)
    return build


for _tail in (False, True):
    for _dt in (U32, F64):
        for _na, _nb in ((100000, 99999), (100000, 4096)):
            for _keep in (0, 1):
                case(f"compare_split{'-tail' if _tail else ''}-{DT_NAME[_dt]}-{_na}+{_nb}-keep{_keep}",
                     "misort_merge_split_tail" if _tail else "misort_merge_split",
                     rep=(_dt, _nb, _keep) == (F64, 4096, 1))(_compare_split(_dt, _na, _nb, _keep, _tail))


def _fill(dt):
    def build(salt=0):
        n, seed, g0 = N_OF[dt], 0x5EED0071 + salt, 12345 + salt
        junk = rand(71 + salt, n, dt) | dt(1)  # the producer writes the output too: a fill that ran early is overwritten
        return ({"out": In(junk)}, lambda c, t, s: _void(c.fill_splitmix(t["out"], seed, g0, stream=s)),
                {"out": O.splitmix(seed, n, dt, g0)}, None)
    return build


case("fill_splitmix-u32", "misort_fill_splitmix", rep=True)(_fill(U32))
case("fill_splitmix-u64", "misort_fill_splitmix")(_fill(U64))

SEGMENTS_LAYOUT = "mixed"  # the one named layout with tile classes and long classes


def _segments(dt, in_place):
    def build(salt=0):
        offs, n = SL.layout(SEGMENTS_LAYOUT, np.dtype(dt).itemsize)
        k = SL.make("random", 81 + salt, offs, n, dt)
        want = SL.want(k, offs, dt)
        if in_place:
            return ({"keys": In(k), "offs": In(offs)},
                    lambda c, t, s: _void(c.sort_segments(t["keys"], t["offs"], out=t["keys"], stream=s)),
                    {"keys": want, "offs": bits(offs)}, None)
        return ({"inp": In(k), "offs": In(offs), "out": Out(n, dt)},
                lambda c, t, s: _void(c.sort_segments(t["inp"], t["offs"], out=t["out"], stream=s)),
                {"inp": k, "offs": bits(offs), "out": want}, None)
    return build


for _dt in (U32, U64):
    for _ip in (False, True):
        case(f"sort_segments-{DT_NAME[_dt]}-{'in_place' if _ip else 'oop'}", "misort_local_sort_segments",
             rep=(_dt, _ip) == (U32, False))(_segments(_dt, _ip))


def _check_sort(dt):
    def build(salt=0):
        n = N_OF[dt]
        x = sorted_bits(keys_of(dt, 91 + salt, n)).view(dt).copy()
        at = np.random.default_rng(92 + salt).choice(n - 1, 777, replace=False)
        x[at], x[at + 1] = x[at + 1].copy(), x[at].copy()  # descents the host counts
        want = descents(x)
        assert want > 300

        def value_check(got):
            assert got == want, f"check_sort counted {got} descents, the data the producer writes has {want}"
        return ({"keys": In(x)}, lambda c, t, s: c.check_sort(t["keys"], stream=s), {"keys": bits(x)}, value_check)
    return build


case("check_sort-u32", "misort_check_sort", rep=True)(_check_sort(U32))
case("check_sort-f64", "misort_check_sort")(_check_sort(F64))


# The collectives on a lone context: results only (NOT_ASYNCHRONOUS says why).
def _quick(dt):
    def build(salt=0):
        x = keys_of(dt, 95 + salt, N_OF[dt])

        def call(c, t, s):
            _, n = c.parallel_quick_sort(t["inp"], out=t["out"], stream=s)
            return n

        def value_check(n):
            assert n == x.size
        return ({"inp": In(x), "out": Out(x.size, dt)}, call,
                {"inp": bits(x), "out": sorted_bits(x)}, value_check)
    return build


def _sample(dt):
    def build(salt=0):
        x = keys_of(dt, 96 + salt, N_OF[dt])
        return ({"inp": In(x), "out": Out(x.size, dt)},
                lambda c, t, s: _void(c.parallel_sample_sort(t["inp"], out=t["out"], stream=s)),
                {"inp": bits(x), "out": sorted_bits(x)}, None)
    return build


def _parallel_pairs(salt=0):
    keys, vals = tied_u32(97 + salt, NPAIRS), rand(98 + salt, NPAIRS, U32)
    wk, wv = pairs_oracle(keys, vals)
    return ({"keys": In(keys), "vals": In(vals), "ok": Out(NPAIRS, U32), "ov": Out(NPAIRS, U32)},
            lambda c, t, s: _void(c.parallel_sort_pairs(t["keys"], t["vals"], out_keys=t["ok"], out_values=t["ov"],
                                                  stream=s)),
            {"keys": keys, "vals": vals, "ok": wk, "ov": wv}, None)


case("parallel_quick_sort-u32-lone", "misort_parallel_quick_sort")(_quick(U32))
case("parallel_sample_sort-f64-lone", "misort_parallel_sample_sort")(_sample(F64))
case("parallel_sort_pairs-u32-lone", "misort_parallel_sort_pairs")(_parallel_pairs)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
REPEATED = [c for c in CASES if c.rep]  # one shape per Python entry point, for the stream variants


def run_case(ctx, cs, stream, stream_arg="explicit", producer_stream=None):
    """One case behind pending work: (Result, expect, value_check).
    ``stream_arg``: "explicit" passes the stream's handle while another stream
    is torch's current one; "current" passes None with the stream current."""
    stage, call, expect, value_check = cs.build()
    handle = None if stream_arg == "current" else stream.cuda_stream
    res = behind_pending_work(stream, stage, lambda t: call(ctx, t, handle), producer_stream,
                              current="stream" if stream_arg == "current" else "elsewhere")
    return res, expect, value_check


def compare(res, expect, what):
    """Snapshot and live tensors, bit for bit, against the expected patterns."""
    assert set(expect) == set(res.snap), (sorted(expect), sorted(res.snap))
    for name, want in expect.items():
        for kind, got in (("snapshot", res.snap[name]), ("live", res.live[name])):
            np.testing.assert_array_equal(got, bits(want), err_msg=f"{what}: {name} ({kind})")


WARM_SALT = 1000  # the warm-up's data: same shapes, other keys


def warm(ctx, cs, stream, stream_arg="explicit"):
    """The same call once on the same stream with the same shapes, inputs in
    place and the stream idle: scratch growth and first-use allocation, which
    may wait, are out of the way; the result is checked.  Its data is not the
    case's: the context's scratch (bounce, records, padded rows) would else be
    left holding the case's right answer, and a copy-out that ran early would
    deliver it."""
    import torch
    stage, call, expect, value_check = cs.build(WARM_SALT)
    live, staged = allocate(stage)
    with torch.cuda.stream(stream):
        for name, src in staged.items():
            live[name].copy_(src)
    with torch.cuda.stream(stream if stream_arg == "current" else elsewhere()):
        value = call(ctx, live, None if stream_arg == "current" else stream.cuda_stream)
    with torch.cuda.stream(stream):
        if isinstance(value, dict):
            live.update(value)
        stream.synchronize()
        res = Result()
        res.snap = res.live = {k: host_bits(v) for k, v in live.items()}
        stream.synchronize()
    compare(res, expect, f"{cs.name} (warm-up)")
    if value_check:
        value_check(value)
