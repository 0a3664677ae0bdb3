"""bench.py's launcher (CPU only): `--gpus N` without a torchrun environment
must start N ranks through torch.distributed.run as a child process, before
anything touches a GPU, and pass every argument through."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_needs_launch_only_without_world_size():
    b = load_bench()
    a = b.parse_args(["--gpus", "8"])
    assert b.needs_launch(a, env={})
    assert not b.needs_launch(a, env={"WORLD_SIZE": "8"})
    assert not b.needs_launch(b.parse_args([]), env={})
    assert not b.needs_launch(b.parse_args(["--gpus", "1"]), env={})


def test_launch_command_shape():
    b = load_bench()
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    cmd = b.launch_command(argv, 4, 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29511" in cmd
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == argv


def test_main_relaunches_without_touching_the_gpu(monkeypatch):
    b = load_bench()
    calls = []

    def fake_call(cmd, env=None):
        calls.append((cmd, env))
        return 7

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(b.subprocess, "call", fake_call)
    monkeypatch.setattr(b, "cpu_baseline", lambda *a: {"value": 0.1, "kind": "reference", "cores": 16})
    # if main went past the launcher it would build contexts: make that fatal
    import misort
    monkeypatch.setattr(misort, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    rc = b.main(["--gpus", "8", "--steps", "2", "--full"])
    assert rc == 7
    (cmd, env), = calls
    assert "--nproc-per-node=8" in cmd
    assert cmd[-5:] == ["--gpus", "8", "--steps", "2", "--full"]
    assert env["MASTER_ADDR"] == "127.0.0.1"
    # the host-core baseline was measured by the parent and handed over
    # (the file is removed once the ranks have finished)
    assert b.CPU_JSON_ENV in env and not os.path.exists(env[b.CPU_JSON_ENV])


def test_parent_cpu_baseline_reaches_rank0(monkeypatch, tmp_path):
    """The N > 1 line carries the host-core baseline: the parent measures it
    (no HIP call: misort.Context is fatal here) and rank 0 loads it."""
    b = load_bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cpu"] = b.load_cpu_json(env[b.CPU_JSON_ENV])
        return 0

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(b.subprocess, "call", fake_call)
    monkeypatch.setattr(b, "cpu_baseline", lambda *a: {"value": 0.12, "kind": "reference", "cores": 16})
    import misort
    monkeypatch.setattr(misort, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched")))
    assert b.main(["--gpus", "4", "--full"]) == 0
    assert seen["cpu"]["value"] == 0.12 and seen["cpu"]["kind"] == "reference"
    assert "launcher parent" in seen["cpu"]["measured_by"]
    assert b.load_cpu_json(None) is None and b.load_cpu_json(str(tmp_path / "missing.json")) is None


def test_plain_launch_runs_no_cpu_baseline(monkeypatch):
    """Without --full the launcher parent measures nothing: it only starts the ranks."""
    b = load_bench()
    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(b.subprocess, "call", lambda cmd, env=None: calls.append(env) or 0)
    monkeypatch.setattr(b, "cpu_baseline", lambda *a: (_ for _ in ()).throw(AssertionError("baseline run")))
    assert b.main(["--gpus", "2", "--steps", "3", "--warmup", "1"]) == 0
    (env,) = calls
    assert b.CPU_JSON_ENV not in env


def test_full_gates_the_extra_runs():
    b = load_bench()
    a = b.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (3, 2)
    a = b.parse_args(["--full", "--host-io", "--cpu-sweep", "--dump-outputs", "d"])
    assert a.full and a.host_io and a.cpu_sweep and a.dump_outputs == "d"
    for flag in ("--host-io", "--cpu-sweep"):
        try:
            b.parse_args([flag])
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(f"{flag} accepted without --full")


def test_dump_positions_and_arrays():
    """--dump-outputs writes the same positions in every run, both ends among
    them, within its size limit, and every key exactly as float64."""
    import numpy as np
    b = load_bench()
    assert np.array_equal(b.dump_indices(1000), np.arange(1000))
    assert b.dump_indices(0).size == 0
    n = 1 << 30
    i, j = b.dump_indices(n), b.dump_indices(n)
    assert np.array_equal(i, j) and i.dtype == np.int64
    assert i[0] == 0 and i[-1] == n - 1 and np.all(np.diff(i) > 0)
    assert b.DUMP_KEYS // 2 < i.size <= b.DUMP_KEYS
    assert 2 * 8 * b.DUMP_KEYS <= 64 << 20  # u64: two float64 arrays
    k = b.dump_indices(n // 8, b.DUMP_KEYS // 8)
    assert k.size <= b.DUMP_KEYS // 8 and k[-1] == n // 8 - 1
    u32 = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32)
    (name, arr), = b.dump_arrays("x", u32).items()
    assert name == "x" and arr.dtype == np.float64 and np.array_equal(arr.astype(np.uint32), u32)
    u64 = np.array([0, (1 << 64) - 1, (1 << 53) + 1, 0x0123456789ABCDEF], dtype=np.uint64)
    d = b.dump_arrays("x", u64)
    assert sorted(d) == ["x_hi", "x_lo"] and all(v.dtype == np.float64 for v in d.values())
    back = (d["x_hi"].astype(np.uint64) << np.uint64(32)) | d["x_lo"].astype(np.uint64)
    assert np.array_equal(back, u64)
    f64 = np.array([0.0, -0.0, 0.5, 1.0 - 2.0 ** -53])
    assert np.array_equal(b.dump_arrays("x", f64)["x"].view(np.uint64), f64.view(np.uint64))


def test_cpu_share_and_pow2():
    b = load_bench()
    n, why = b.cpu_share()
    assert n >= 1 and "sched_getaffinity" in why
    assert [b.pow2_floor(v) for v in (1, 2, 3, 8, 15, 16, 63, 64)] == [1, 2, 2, 8, 8, 16, 32, 64]
