#!/usr/bin/env python3
"""64-bit key-value sort against its yardsticks, n = 2^26 and 2^28 pairs, f64 keys
(random bit patterns):

* k_zip_lo (the first `other` record of an argsort64) against a device-to-device
  torch copy of the same 16 bytes per key;
* k_gather_hi and k_emit (the second and third record) in ms and algorithmic
  GB/s, each beside torch gathers (src[idx.long()]) of the same element width
  over the same index stream: the first sort's order for gather_hi's keys, the
  first sort's ranks in output order for emit's records, the final order for
  emit's values;
* the whole argsort64 and sort_pairs64 (4- and 8-byte values) against twice
  local_sort of n u64 keys.

Everything runs on the context's own stream, timed by HIP events on it: a
warm-up, then --reps timed runs each (medians).  Writes one JSON line to --out
(default profiles/pairs64/pairs64_probe.json) and prints it."""
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
    """Median ms and bytes of the three `other` records of fn(): zip_lo, gather_hi, emit."""
    fn()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rec = [(ms, b) for kind, ms, b in ctx.profile_trace() if kind == "other"]
    ctx.profile(False)
    assert len(rec) == 3 * reps, len(rec)
    res = []
    for part in (rec[0::3], rec[1::3], rec[2::3]):
        assert len({b for _, b in part}) == 1
        res.append((statistics.median(ms for ms, _ in part), part[0][1]))
    return res


def gbs(nbytes, ms):
    return nbytes / ms / 1e6


def index_streams(ctx, keys, idx):
    """The index streams of the two gathers as int64 tensors: the first sort's
    order (gather_hi reads keys by it), and the first sort's ranks in output
    order (emit reads the first sort's records by it)."""
    b = keys.view(torch.int64)
    ordk = torch.where(b < 0, ~b, b ^ torch.iinfo(torch.int64).min)
    lo_order = ctx.argsort64(ordk & 0xFFFFFFFF).long()
    del ordk
    rank = torch.empty_like(lo_order)
    rank[lo_order] = torch.arange(lo_order.numel(), dtype=torch.int64, device=keys.device)
    return lo_order, rank[idx.long()]


def probe(ctx, n, reps):
    k64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(k64, 0x5EED0064)
    keys = k64.view(torch.float64)
    v4 = torch.empty(n, dtype=torch.int32, device="cuda")
    v8 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(v4, 0x5EED0065)
    ctx.fill_splitmix(v8, 0x5EED0066)
    ok, o4, o8 = torch.empty_like(keys), torch.empty_like(v4), torch.empty_like(v8)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    u64_in = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(u64_in, 0x5EED0067)
    u64_out = torch.empty_like(u64_in)

    arg_ms, arg_min = timed(lambda: ctx.argsort64(keys, out=idx), reps)
    p4_ms, p4_min = timed(lambda: ctx.sort_pairs64(keys, v4, out_keys=ok, out_values=o4), reps)
    p8_ms, p8_min = timed(lambda: ctx.sort_pairs64(keys, v8, out_keys=ok, out_values=o8), reps)
    u64_ms, u64_min = timed(lambda: ctx.local_sort(u64_in, u64_out), reps)
    (zip_ms, zip_b), (gat_ms, gat_b), (emi_ms, emi_b) = other_records(ctx, lambda: ctx.argsort64(keys, out=idx), reps)
    _, _, (em4_ms, em4_b) = other_records(
        ctx, lambda: ctx.sort_pairs64(keys, v4, out_keys=ok, out_values=o4), reps)
    _, _, (em8_ms, em8_b) = other_records(
        ctx, lambda: ctx.sort_pairs64(keys, v8, out_keys=ok, out_values=o8), reps)
    assert zip_b == 16 * n and gat_b == 24 * n and emi_b == 20 * n and em4_b == 32 * n and em8_b == 40 * n
    # what was timed is a sort: the keys come out in local_sort's order, bit for bit
    ctx.local_sort(keys, u64_out.view(torch.float64))
    assert torch.equal(ok.view(torch.int64), u64_out)

    # a copy reads and writes its buffer once: 8n bytes copied move the 16n of zip_lo
    cp_ms, _ = timed(lambda: u64_out.copy_(k64), reps)
    lo_order, rank = index_streams(ctx, keys, idx)
    final = idx.long()
    tg_keys_ms, _ = timed(lambda: k64[lo_order], reps)
    tg_recs_ms, _ = timed(lambda: k64[rank], reps)
    tg_v8_ms, _ = timed(lambda: v8[final], reps)
    tg_v4_ms, _ = timed(lambda: v4[final], reps)
    return {
        "pairs": n,
        "argsort64_ms": arg_ms, "argsort64_min_ms": arg_min,
        "sort_pairs64_v4_ms": p4_ms, "sort_pairs64_v4_min_ms": p4_min,
        "sort_pairs64_v8_ms": p8_ms, "sort_pairs64_v8_min_ms": p8_min,
        "local_sort_u64_ms": u64_ms, "local_sort_u64_min_ms": u64_min,
        "argsort64_over_2x_u64": arg_ms / (2 * u64_ms),
        "sort_pairs64_v4_over_2x_u64": p4_ms / (2 * u64_ms),
        "sort_pairs64_v8_over_2x_u64": p8_ms / (2 * u64_ms),
        "zip_lo_ms": zip_ms, "zip_lo_GBs": gbs(zip_b, zip_ms),
        "copy16_ms": cp_ms, "copy16_GBs": gbs(16 * n, cp_ms), "zip_lo_over_copy_rate": cp_ms / zip_ms,
        "gather_hi_ms": gat_ms, "gather_hi_GBs": gbs(gat_b, gat_ms),
        "torch_gather8_lo_order_ms": tg_keys_ms, "gather_hi_over_torch_time": gat_ms / tg_keys_ms,
        "emit_index_ms": emi_ms, "emit_index_GBs": gbs(emi_b, emi_ms),
        "torch_gather8_ranks_ms": tg_recs_ms, "emit_index_over_torch_time": emi_ms / tg_recs_ms,
        "emit_v4_ms": em4_ms, "emit_v4_GBs": gbs(em4_b, em4_ms),
        "torch_gather4_final_ms": tg_v4_ms, "emit_v4_over_torch_time": em4_ms / (tg_recs_ms + tg_v4_ms),
        "emit_v8_ms": em8_ms, "emit_v8_GBs": gbs(em8_b, em8_ms),
        "torch_gather8_final_ms": tg_v8_ms, "emit_v8_over_torch_time": em8_ms / (tg_recs_ms + tg_v8_ms),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs64", "pairs64_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pairs64_probe needs a GPU")
    ctx = misort.Context(0)
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        res = [probe(ctx, 1 << lg, a.reps) for lg in a.log2]
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "pairs64", "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": res})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
