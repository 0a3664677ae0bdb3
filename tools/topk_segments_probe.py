#!/usr/bin/env python3
"""Segmented top-k against its yardsticks: 2^27 u32 keys (random bit patterns) as
uniform segments of 64, 1000, 2^13, 2^17 and 2^20 keys whose offsets start one
element off alignment; k in 1, 8, 64, 1024 where k <= the length; the largest
keys; float32 keys once per shape at k = 64.  For each

* Context.topk_segments;
* Context.argsort_segments of the same data: what a caller ran until now (and
  then sliced), yardstick (a);
* Context.topk_rows on the same keys seen as rows: yardstick (b), what the
  segments cost over a call that needs no offsets.

And one ragged case: 2^25 keys in segments of 1 .. 2^18 keys, k = 64, against
topk_rows on the segments padded to the longest one (the padding itself is not
timed) and against argsort_segments.

The candidates alternate inside one process, run after run, on the context's own
stream, each run timed by HIP events on it: a warm-up of each, then --reps
rounds (median, minimum, maximum).  What was timed is held against topk_rows,
bit for bit.  Writes one JSON line to --out (default
profiles/topk_segments/topk_segments_probe.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402
import misort  # noqa: E402

LOG2_KEYS = 27
LENS = [64, 1000, 1 << 13, 1 << 17, 1 << 20]
KS = [1, 8, 64, 1024]
RAGGED_LOG2_KEYS, RAGGED_MAX_LOG2 = 25, 18


def alternated(fns, reps):
    """{name: {median, min, max} device ms}: one warm-up of every fn, then reps
    rounds in which they run one after the other."""
    for fn in fns.values():
        fn()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                   "max_over_median": max(v) / statistics.median(v)} for name, v in ms.items()}


def probe_uniform(ctx, store, nseg, ln, k, reps):
    """``store`` holds one element, then nseg segments of ln keys."""
    f32 = store.dtype == torch.float32
    keys = store[:1 + nseg * ln]
    rows = store[1:1 + nseg * ln].view(nseg, ln)
    offs = 1 + torch.arange(nseg + 1, dtype=torch.int64, device="cuda") * ln
    vals = torch.empty(nseg, k, dtype=store.dtype, device="cuda")
    idx = torch.empty(nseg, k, dtype=torch.int32, device="cuda")
    rvals, ridx = torch.empty_like(vals), torch.empty_like(idx)
    order = torch.empty(keys.numel(), dtype=torch.int32, device="cuda")
    res = {"len": ln, "nseg": nseg, "k": k, "dtype": "f32" if f32 else "u32",
           "passes": len(misort.topk_segments_plan(ln, k))}
    res.update(alternated({
        "topk_segments": lambda: ctx.topk_segments(keys, offs, k, out_values=vals, out_indices=idx),
        "argsort_segments": lambda: ctx.argsort_segments(keys, offs, out=order),
        "topk_rows": lambda: ctx.topk_rows(rows, k, out_values=rvals, out_indices=ridx),
    }, reps))
    res["over_argsort_segments_time"] = res["topk_segments"]["ms"] / res["argsort_segments"]["ms"]
    res["over_topk_rows_time"] = res["topk_segments"]["ms"] / res["topk_rows"]["ms"]
    assert torch.equal(idx, ridx) and torch.equal(vals.view(torch.int32), rvals.view(torch.int32)), (ln, k)
    return res


def probe_ragged(ctx, shift, reps, k=64):
    g = torch.Generator(device="cpu").manual_seed(25)
    total, top = 1 << (RAGGED_LOG2_KEYS - shift), 1 << (RAGGED_MAX_LOG2 - shift)
    lens = []
    while sum(lens) < total:
        lens.append(min(int(torch.randint(1, top + 1, (1,), generator=g)), total - sum(lens)))
    nseg, longest = len(lens), max(lens)
    offs = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).cuda()
    keys = torch.empty(total, dtype=torch.int32, device="cuda")
    ctx.fill_splitmix(keys, 0x5EED00D1)
    # the workaround: rows of the longest length, padded with the worst key of the direction (u32 0 for largest)
    padded = torch.zeros(nseg, longest, dtype=torch.int32, device="cuda")
    at = 0
    for i, ln in enumerate(lens):
        padded[i, :ln] = keys[at:at + ln]
        at += ln
    vals = torch.empty(nseg, k, dtype=torch.int32, device="cuda")
    idx = torch.empty(nseg, k, dtype=torch.int32, device="cuda")
    rvals, ridx = torch.empty_like(vals), torch.empty_like(idx)
    order = torch.empty(total, dtype=torch.int32, device="cuda")
    res = {"keys": total, "nseg": nseg, "longest": longest, "shortest": min(lens), "k": k, "dtype": "u32",
           "padded_keys": nseg * longest}
    res.update(alternated({
        "topk_segments": lambda: ctx.topk_segments(keys, offs, k, out_values=vals, out_indices=idx),
        "argsort_segments": lambda: ctx.argsort_segments(keys, offs, out=order),
        "topk_rows_padded": lambda: ctx.topk_rows(padded, k, out_values=rvals, out_indices=ridx),
    }, reps))
    res["over_argsort_segments_time"] = res["topk_segments"]["ms"] / res["argsort_segments"]["ms"]
    res["over_topk_rows_padded_time"] = res["topk_segments"]["ms"] / res["topk_rows_padded"]["ms"]
    full = torch.tensor([ln >= k for ln in lens], device="cuda")  # shorter ones: fill here, padding keys there
    assert torch.equal(idx[full], ridx[full]) and torch.equal(vals[full], rvals[full])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shift", type=int, default=0, help="halve the key counts this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_segments", "topk_segments_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("medians of at least 5 runs")
    if not torch.cuda.is_available():
        sys.exit("topk_segments_probe needs a GPU")
    ctx = misort.Context(0)
    res = []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for ln in LENS:
            nseg = max(1, (1 << (LOG2_KEYS - a.shift)) // ln)
            store = torch.empty(1 + nseg * ln, dtype=torch.int32, device="cuda")
            ctx.fill_splitmix(store, 0x5EED00D0 + ln)
            for k in (k for k in KS if k <= ln):
                res.append(probe_uniform(ctx, store, nseg, ln, k, a.reps))
                print(json.dumps(res[-1]), file=sys.stderr, flush=True)
            # float32 once per shape: finite keys of both signs
            fstore = (store >> 8).to(torch.float32)
            del store
            res.append(probe_uniform(ctx, fstore, nseg, ln, min(64, ln), a.reps))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
            del fstore
        ragged = probe_ragged(ctx, a.shift, a.reps)
        print(json.dumps(ragged), file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "topk_segments", "reps": a.reps, "log2_keys": LOG2_KEYS - a.shift,
                       "device": torch.cuda.get_device_name(0), "shapes": res, "ragged": ragged})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
