#!/usr/bin/env python3
"""Row-wise key-value sort and argsort against their yardsticks: 2^27 pairs of
u32 keys (random bit patterns) as rows x cols arrays, for each shape

* Context.argsort_rows, and Context.sort_rows_pairs with a value array;
* (a) Context.sort_rows on a u64 tensor of the same rows x cols: the same
  network and passes, 16 bytes moved per element against 8 (argsort) or 16
  (with values); its run-to-run spread (max / median) is the bar the new calls
  are held against;
* (b) the composition a caller had to write before: keys.to(int64) << 32 |
  arange(cols) in torch, sort_rows on u64, a torch split;
* (c) torch.sort(dim=-1) and torch.argsort(dim=-1) on the same key tensor;
* on the one-pass path, the same two calls on the 8-byte kernel
  (MISORT_ROWS_PAIRS_W=2) where they took 16-byte accesses;
* on the padded-block path, the pad and unpad kernels (the two `other` records)
  against device-to-device torch copies that move the same counted bytes.

Everything runs on the context's own stream, timed by HIP events on it: a
warm-up, then --reps timed runs each (median, minimum, maximum).  Writes one
JSON line to --out (default profiles/rows_pairs/rows_pairs_probe.json) and
prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402
import misort  # noqa: E402

LOG2_PAIRS = 27
COLS = [64, 1000, 1 << 13, (1 << 13) + 1, 1 << 16, (1 << 16) + 1, 1 << 20]


def timed(fn, reps):
    """{median, min, max} device ms of fn() over reps runs, after one warm-up."""
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


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


def copy_ms(nbytes, reps):
    """A device copy that moves nbytes in all (reads half, writes half)."""
    src = torch.empty(int(nbytes) // 8, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), reps)["ms"]


def probe(ctx, cols, rows, reps):
    n = rows * cols
    keys = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
    vals = torch.empty_like(keys)
    ctx.fill_splitmix(keys, 0x5EED00A0 + cols)
    ctx.fill_splitmix(vals, 0x5EED00B0 + cols)
    out_k, out_v, idx = torch.empty_like(keys), torch.empty_like(keys), torch.empty_like(keys)
    plan = misort.rows_plan(cols, 8)
    res = {"cols": cols, "rows": rows, "pairs": n, "path": plan["path"], "block_log2": plan["block_log2"],
           "passes": len(plan["passes"])}

    res["argsort_rows"] = timed(lambda: ctx.argsort_rows(keys, out=idx), reps)
    res["sort_rows_pairs"] = timed(lambda: ctx.sort_rows_pairs(keys, vals, out_keys=out_k, out_values=out_v), reps)
    if plan["path"] == "tile" and cols % 4 == 0:
        # such rows took 16-byte accesses; the same calls on the 8-byte kernel
        os.environ["MISORT_ROWS_PAIRS_W"] = "2"
        res["argsort_rows_w2"] = timed(lambda: ctx.argsort_rows(keys, out=idx), reps)
        res["sort_rows_pairs_w2"] = timed(lambda: ctx.sort_rows_pairs(keys, vals, out_keys=out_k, out_values=out_v),
                                          reps)
        del os.environ["MISORT_ROWS_PAIRS_W"]
        ctx.argsort_rows(keys, out=idx)
        ctx.sort_rows_pairs(keys, vals, out_keys=out_k, out_values=out_v)
    # what was timed is a row argsort and a row key-value sort: a sample of rows agrees
    # with torch (signed storage: sorted through the unsigned order)
    pick = torch.arange(0, rows, max(1, rows // 64), device="cuda")
    lo = torch.iinfo(torch.int32).min
    want = torch.sort(keys[pick] ^ lo, dim=-1).values ^ lo
    assert torch.equal(torch.gather(keys[pick], -1, idx[pick].to(torch.int64)), want)
    assert torch.equal(out_k[pick], want)

    # (a) the same rows as u64 keys
    rec = torch.empty(rows, cols, dtype=torch.int64, device="cuda")
    rec_out = torch.empty_like(rec)
    ctx.fill_splitmix(rec, 0x5EED00C0 + cols)
    a = timed(lambda: ctx.sort_rows(rec, out=rec_out), reps)
    a["spread"] = a["max_ms"] / a["ms"]
    res["sort_rows_u64"] = a
    for name in ("argsort_rows", "sort_rows_pairs"):
        res[name]["over_sort_rows_u64_time"] = res[name]["ms"] / a["ms"]
        res[name]["within_spread"] = res[name]["ms"] <= a["max_ms"]

    # (b) zip in torch, sort_rows on u64, split in torch
    col = torch.arange(cols, dtype=torch.int64, device="cuda")

    def composed():
        torch.bitwise_or(keys.to(torch.int64) << 32, col, out=rec)
        ctx.sort_rows(rec, out=rec_out)
        return (rec_out & 0xFFFFFFFF).to(torch.int32)
    res["composed_argsort"] = timed(composed, reps)
    assert torch.equal(composed()[pick], idx[pick])
    res["argsort_rows"]["over_composed_time"] = res["argsort_rows"]["ms"] / res["composed_argsort"]["ms"]
    del rec, rec_out

    # (c) torch
    res["torch_sort"] = timed(lambda: torch.sort(keys, dim=-1), reps)
    res["torch_argsort"] = timed(lambda: torch.argsort(keys, dim=-1), reps)
    res["argsort_rows"]["over_torch_argsort_time"] = res["argsort_rows"]["ms"] / res["torch_argsort"]["ms"]
    res["sort_rows_pairs"]["over_torch_sort_time"] = res["sort_rows_pairs"]["ms"] / res["torch_sort"]["ms"]

    if plan["path"] == "blocks":
        block = rows << plan["block_log2"]
        for name, fn, want_b in (
                ("argsort_rows", lambda: ctx.argsort_rows(keys, out=idx), (4 * n + 8 * block, 8 * n + 4 * n)),
                ("sort_rows_pairs", lambda: ctx.sort_rows_pairs(keys, vals, out_keys=out_k, out_values=out_v),
                 (8 * n + 8 * block, 8 * n + 8 * n))):
            (pad_ms, pad_b), (unpad_ms, unpad_b) = other_records(ctx, fn, reps)
            assert (pad_b, unpad_b) == want_b, (pad_b, unpad_b, want_b)
            pad_cp, unpad_cp = copy_ms(pad_b, reps), copy_ms(unpad_b, reps)
            res[name].update({"pad_ms": pad_ms, "pad_bytes": pad_b, "pad_copy_ms": pad_cp,
                              "pad_over_copy_time": pad_ms / pad_cp, "unpad_ms": unpad_ms, "unpad_bytes": unpad_b,
                              "unpad_copy_ms": unpad_cp, "unpad_over_copy_time": unpad_ms / unpad_cp})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=int, default=0, help="halve the pair count this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_pairs", "rows_pairs_probe.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("medians of at least 5 runs")
    if not torch.cuda.is_available():
        sys.exit("rows_pairs_probe needs a GPU")
    ctx = misort.Context(0)
    res = []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for cols in COLS:
            res.append(probe(ctx, cols, max(1, (1 << (LOG2_PAIRS - a.shift)) // cols), a.reps))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "rows_pairs", "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": res})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
