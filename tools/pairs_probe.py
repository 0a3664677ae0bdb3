#!/usr/bin/env python3
"""Key-value sort against its two yardsticks, n = 2^26 and 2^28 pairs:

* zip_pairs / unzip_pairs (the profiler's `other` records of a sort_pairs and
  of an argsort) against a device-to-device torch copy of the same bytes;
* the whole sort_pairs and argsort against local_sort of n u64 keys.

Everything runs on the context's own stream, timed by HIP events on it: a
warm-up, then --reps timed runs each (medians).  Prints one JSON line:
python tools/pairs_probe.py > profiles/pairs/pairs_probe.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402
import misort  # noqa: E402


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
    """Median ms and bytes of the first and second `other` record of fn(): zip, unzip."""
    fn()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rec = [(ms, b) for kind, ms, b in ctx.profile_trace() if kind == "other"]
    ctx.profile(False)
    assert len(rec) == 2 * reps, len(rec)
    res = []
    for half in (rec[0::2], rec[1::2]):
        assert len({b for _, b in half}) == 1
        res.append((statistics.median(ms for ms, _ in half), half[0][1]))
    return res


def gbs(nbytes, ms):
    return nbytes / ms / 1e6


def probe(ctx, n, reps):
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty_like(keys)
    ctx.fill_splitmix(keys, 0x5EED0011)
    ctx.fill_splitmix(vals, 0x5EED0012)
    ok, ov = torch.empty_like(keys), torch.empty_like(vals)
    k64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(k64, 0x5EED0013)
    o64 = torch.empty_like(k64)

    pairs_ms, pairs_min = timed(lambda: ctx.sort_pairs(keys, vals, out_keys=ok, out_values=ov), reps)
    arg_ms, arg_min = timed(lambda: ctx.argsort(keys, out=ov), reps)
    u64_ms, u64_min = timed(lambda: ctx.local_sort(k64, o64), reps)
    (zip_ms, zip_b), (unzip_ms, unzip_b) = other_records(
        ctx, lambda: ctx.sort_pairs(keys, vals, out_keys=ok, out_values=ov), reps)
    (zipi_ms, zipi_b), (unzipv_ms, unzipv_b) = other_records(ctx, lambda: ctx.argsort(keys, out=ov), reps)
    # a copy reads and writes its buffer once: 8n bytes copied move the 16n of a
    # zip, 6n the 12n of an argsort's zip or unzip
    cp16_ms, _ = timed(lambda: o64.copy_(k64), reps)
    half = 3 * n // 4
    cp12_ms, _ = timed(lambda: o64[:half].copy_(k64[:half]), reps)
    assert zip_b == unzip_b == 16 * n and zipi_b == unzipv_b == 12 * n
    top = ok.view(torch.uint8).view(-1, 4)[:, 3]  # what was timed is a sort: the keys' top bytes ascend
    assert bool((top[1:] >= top[:-1]).all())
    return {
        "pairs": n,
        "sort_pairs_ms": pairs_ms, "sort_pairs_min_ms": pairs_min,
        "argsort_ms": arg_ms, "argsort_min_ms": arg_min,
        "local_sort_u64_ms": u64_ms, "local_sort_u64_min_ms": u64_min,
        "sort_pairs_over_u64": pairs_ms / u64_ms, "argsort_over_u64": arg_ms / u64_ms,
        "zip_ms": zip_ms, "unzip_ms": unzip_ms, "copy16_ms": cp16_ms,
        "zip_GBs": gbs(zip_b, zip_ms), "unzip_GBs": gbs(unzip_b, unzip_ms), "copy16_GBs": gbs(16 * n, cp16_ms),
        "zip_over_copy_rate": cp16_ms / zip_ms, "unzip_over_copy_rate": cp16_ms / unzip_ms,
        "zip_index_ms": zipi_ms, "unzip_values_ms": unzipv_ms, "copy12_ms": cp12_ms,
        "zip_index_GBs": gbs(zipi_b, zipi_ms), "unzip_values_GBs": gbs(unzipv_b, unzipv_ms),
        "copy12_GBs": gbs(12 * n, cp12_ms),
        "zip_index_over_copy_rate": cp12_ms / zipi_ms, "unzip_values_over_copy_rate": cp12_ms / unzipv_ms,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pairs_probe needs a GPU")
    ctx = misort.Context(0)
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        res = [probe(ctx, 1 << lg, a.reps) for lg in a.log2]
        torch.cuda.synchronize()
    ctx.close()
    print(json.dumps({"probe": "pairs", "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": res}))


if __name__ == "__main__":
    main()
