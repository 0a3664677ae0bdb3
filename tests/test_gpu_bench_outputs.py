"""bench.py end to end on one GPU: a plain run times exactly --steps steps, runs
no CPU baseline, and `--dump-outputs DIR` writes the keys the last timed step
returned -- the whole sorted block when it is small, else the fixed sample of
bench.dump_indices -- exactly as float64 (u64 keys as 32-bit halves)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.gpu
# 2^22 u32: more keys than the dump holds (sampled); 2^16 u64: whole block, hi/lo halves
@pytest.mark.parametrize("dtype,logn", [("u32", 22), ("u64", 16)])
def test_plain_run_dumps_the_sorted_keys(tmp_path, dtype, logn):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    b = load_bench()
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dtype", dtype,
                        "--logn", str(logn), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == b.METRIC and line["unit"] == "Gkeys/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == dtype
    assert line["check_errors"] == 0 and line["cpu_baseline"] is None
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - (1 << logn) / (line["ms_per_step"] * 1e-3) / 1e9) <= 1e-9 * line["value"]

    n = 1 << logn
    want = O.local_sort(O.splitmix(b.SEED, n, np.uint32 if dtype == "u32" else np.uint64))[b.dump_indices(n)]
    files = sorted(os.listdir(d))
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    if dtype == "u32":
        assert files == ["sorted_keys.npy"]
        got = np.load(d / files[0])
        assert got.dtype == np.float64 and 2 < got.size <= b.DUMP_KEYS < n
        assert np.array_equal(got, want.astype(np.float64))
    else:
        assert files == ["sorted_keys_hi.npy", "sorted_keys_lo.npy"]
        hi, lo = np.load(d / files[0]), np.load(d / files[1])
        assert hi.dtype == lo.dtype == np.float64
        assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), want)
