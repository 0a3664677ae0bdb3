#!/usr/bin/env python3
"""Row-wise top-k against its yardsticks: 2^27 u32 keys (random bit patterns) as
rows x cols arrays, cols in 64, 1000, 2^13, 2^17, 2^20; k in 1, 8, 64, 1024
where k <= cols; both directions; float32 keys once per shape.  For each

* Context.topk_rows;
* Context.argsort_rows of the same array: what a caller had to run before (and
  then slice), the yardstick;
* torch.topk(dim=-1, sorted=True) on the same tensor.

The three alternate inside one process, run after run, on the context's own
stream, each run timed by HIP events on it: a warm-up of each, then --reps
rounds (median, minimum, maximum).  A sample of rows of what was timed is held
against torch.  Writes one JSON line to --out (default
profiles/topk/topk_probe.json) and prints it."""
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
COLS = [64, 1000, 1 << 13, 1 << 17, 1 << 20]
KS = [1, 8, 64, 1024]


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
    return {name: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def probe(ctx, keys, k, largest, reps):
    rows, cols = keys.shape
    f32 = keys.dtype == torch.float32
    vals = torch.empty(rows, k, dtype=keys.dtype, device="cuda")
    idx = torch.empty(rows, k, dtype=torch.int32, device="cuda")
    order = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
    res = {"cols": cols, "rows": rows, "k": k, "largest": largest, "dtype": "f32" if f32 else "u32",
           "passes": len(misort.topk_plan(cols, k))}
    res.update(alternated({
        "topk_rows": lambda: ctx.topk_rows(keys, k, largest=largest, out_values=vals, out_indices=idx),
        "argsort_rows": lambda: ctx.argsort_rows(keys, out=order),
        "torch_topk": lambda: torch.topk(keys, k, dim=-1, largest=largest, sorted=True),
    }, reps))
    res["over_argsort_rows_time"] = res["topk_rows"]["ms"] / res["argsort_rows"]["ms"]
    res["over_torch_topk_time"] = res["topk_rows"]["ms"] / res["torch_topk"]["ms"]
    # what was timed is a top-k: a sample of rows has torch's values (u32 keys in
    # signed storage: compared through the unsigned order), and the indices gather them
    pick = torch.arange(0, rows, max(1, rows // 64), device="cuda")
    sample = keys[pick]
    if f32:
        want = torch.topk(sample, k, dim=-1, largest=largest).values
    else:
        lo = torch.iinfo(torch.int32).min
        want = torch.topk(sample ^ lo, k, dim=-1, largest=largest).values ^ lo
    assert torch.equal(vals[pick], want), (cols, k, largest)
    assert torch.equal(torch.gather(sample, -1, idx[pick].to(torch.int64)), want), (cols, k, largest)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shift", type=int, default=0, help="halve the key count this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "topk_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("medians of at least 5 runs")
    if not torch.cuda.is_available():
        sys.exit("topk_probe needs a GPU")
    ctx = misort.Context(0)
    res = []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for cols in COLS:
            rows = max(1, (1 << (LOG2_KEYS - a.shift)) // cols)
            keys = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
            ctx.fill_splitmix(keys, 0x5EED00D0 + cols)
            for k in (k for k in KS if k <= cols):
                for largest in (True, False):
                    res.append(probe(ctx, keys, k, largest, a.reps))
                    print(json.dumps(res[-1]), file=sys.stderr, flush=True)
            # float32 once per shape: finite keys of both signs
            fkeys = (keys >> 8).to(torch.float32)
            del keys
            res.append(probe(ctx, fkeys, min(64, cols), True, a.reps))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
            del fkeys
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "topk", "reps": a.reps, "log2_keys": LOG2_KEYS - a.shift,
                       "device": torch.cuda.get_device_name(0), "shapes": res})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
