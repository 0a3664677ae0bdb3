#!/usr/bin/env python3
"""Row-wise sort against its yardsticks: 2^28 u32 keys and 2^27 u64 keys as
rows x cols arrays (random bit patterns), for each shape

* Context.sort_rows, out of place;
* torch.sort(dim=-1) values on the same tensor (signed storage: the same work);
* pass_probe of the shipped tile_sort pass over the same key count (the floor
  of the one-pass path);
* local_sort of all rows * cols keys as ONE array (a row sort does fewer levels);
* for the two shapes with the longest rows, a host loop of local_sort per row;
* on the padded-block path, the pad and unpad kernels (the two `other` records)
  against a device-to-device torch copy that moves the same bytes.

Everything runs on the context's own stream, timed by HIP events on it: a
warm-up, then --reps timed runs each (medians).  Writes one JSON line to --out
(default profiles/rows/rows_probe.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402
import misort  # noqa: E402

# (cols, log2 rows at 2^28 keys); u64 shapes hold half the rows
SHAPES = [(64, 22), (1000, 18), (1 << 14, 14), ((1 << 14) - 1, 14), (1 << 16, 12), ((1 << 16) + 1, 12), (1 << 20, 8)]
ROW_LOOP_COLS = ((1 << 16) + 1, 1 << 20)


def timed(fn, reps):
    """Median and minimum device ms of fn() over reps runs, after one warm-up."""
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def other_records(ctx, fn, reps):
    """Median ms and bytes of the two `other` records of fn(): pad, unpad."""
    fn()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rec = [(ms, b) for kind, ms, b in ctx.profile_trace() if kind == "other"]
    ctx.profile(False)
    assert len(rec) == 2 * reps, len(rec)
    return [(statistics.median(ms for ms, _ in part), part[0][1]) for part in (rec[0::2], rec[1::2])]


def probe(ctx, dtype, cols, rows, reps):
    size = torch.empty(0, dtype=dtype).element_size()
    n = rows * cols
    keys = torch.empty(rows, cols, dtype=dtype, device="cuda")
    ctx.fill_splitmix(keys, 0x5EED0080 + cols)
    out = torch.empty_like(keys)
    flat_in, flat_out = keys.view(-1), out.view(-1)
    plan = misort.rows_plan(cols, size)
    res = {"key_bytes": size, "cols": cols, "rows": rows, "keys": n, "path": plan["path"],
           "tile_log2": plan["tile_log2"], "block_log2": plan["block_log2"], "passes": len(plan["passes"])}

    res["sort_rows_ms"], res["sort_rows_min_ms"] = timed(lambda: ctx.sort_rows(keys, out=out), reps)
    # what was timed is a row sort: it agrees with torch on a sample of rows
    # (signed storage sorts differently: compare as multisets through a sort of the unsigned order)
    pick = torch.arange(0, rows, max(1, rows // 64), device="cuda")
    want = torch.sort(keys[pick] ^ torch.iinfo(dtype).min, dim=-1).values ^ torch.iinfo(dtype).min
    assert torch.equal(out[pick], want)

    if plan["path"] == "tile" and cols == 1 << plan["tile_log2"]:
        # a row is a whole shipped tile: sort_rows ran the shipped SORT pass; the row tile itself
        os.environ["MISORT_ROWS_SHIPPED"] = "0"
        res["row_tile_ms"], res["row_tile_min_ms"] = timed(lambda: ctx.sort_rows(keys, out=out), reps)
        del os.environ["MISORT_ROWS_SHIPPED"]
        assert torch.equal(out[pick], want)
        res["row_tile_over_shipped_time"] = res["row_tile_ms"] / res["sort_rows_ms"]

    res["torch_sort_ms"], res["torch_sort_min_ms"] = timed(lambda: torch.sort(keys, dim=-1).values, reps)
    res["local_sort_all_ms"], res["local_sort_all_min_ms"] = timed(lambda: ctx.local_sort(flat_in, flat_out), reps)
    res["sort_rows_over_torch_time"] = res["sort_rows_ms"] / res["torch_sort_ms"]
    res["sort_rows_over_local_sort_all_time"] = res["sort_rows_ms"] / res["local_sort_all_ms"]

    if cols in ROW_LOOP_COLS:
        def row_loop():
            for r in range(rows):
                ctx.local_sort(keys[r], out[r])
        res["row_loop_ms"], res["row_loop_min_ms"] = timed(row_loop, min(reps, 3))
        res["sort_rows_over_row_loop_time"] = res["sort_rows_ms"] / res["row_loop_ms"]

    if plan["path"] == "blocks":
        (pad_ms, pad_b), (unpad_ms, unpad_b) = other_records(ctx, lambda: ctx.sort_rows(keys, out=out), reps)
        moved = (n + (rows << plan["block_log2"])) * size
        assert pad_b == moved and unpad_b == moved
        # a copy reads and writes its buffer once: moved / 2 bytes copied move `moved` bytes
        src = torch.empty(moved // (2 * size), dtype=dtype, device="cuda")
        dst = torch.empty_like(src)
        cp_ms, _ = timed(lambda: dst.copy_(src), reps)
        res.update({"pad_ms": pad_ms, "unpad_ms": unpad_ms, "pad_unpad_bytes_each": moved, "copy_same_bytes_ms": cp_ms,
                    "pad_over_copy_time": pad_ms / cp_ms, "unpad_over_copy_time": unpad_ms / cp_ms,
                    "local_sort_all_plus_sweeps_ms": res["local_sort_all_ms"] + pad_ms + unpad_ms})
        del src, dst

    # the shipped SORT pass over the same key count (it scrambles both buffers: last)
    hi = misort.plan(n, size)[0][1]
    res["tile_sort_pass_hi"] = hi
    res["tile_sort_pass_ms"] = ctx.pass_probe(flat_in, flat_out, "tile_sort", hi, 0, False, reps=reps)
    res["sort_rows_over_tile_sort_pass_time"] = res["sort_rows_ms"] / res["tile_sort_pass_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=int, default=0, help="halve the row counts this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows", "rows_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rows_probe needs a GPU")
    ctx = misort.Context(0)
    res = []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for dtype, less in ((torch.int32, 0), (torch.int64, 1)):
            for cols, lr in SHAPES:
                res.append(probe(ctx, dtype, cols, 1 << max(0, lr - less - a.shift), a.reps))
                print(json.dumps(res[-1]), file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "rows", "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": res})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
