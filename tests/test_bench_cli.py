"""bench.py's command line: what a plain run refuses, and the `--dump-outputs` writer (CPU: each check in a process of its own, so that importing bench.py
leaves this process's environment alone).  The GPU test runs a plain line with --dump-outputs end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*argv, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, BENCH, *argv], cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("argv,why", [(["--steps", "0"], "--steps must be at least 1"),
                                      (["--algo", "ppo", "--dump-outputs", "x"], "--dump-outputs covers the Rainbow line")])
def test_bench_refuses_before_touching_a_gpu(argv, why):
    r = _bench(*argv)
    assert r.returncode == 2 and why in r.stderr and not r.stdout.strip(), (r.returncode, r.stderr[-2000:])


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    """Integers and flags become float64, float32 stays float32; an array above 2^20 elements is written as the same 2^20 positions in every run."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); import bench; "
            "big = np.arange(3 << 20, dtype=np.float32).reshape(3, -1); "
            "bench.dump_outputs(sys.argv[2], {'actions': np.array([0, 5, 2], np.int32), 'done': np.array([1, 0], np.uint8), 'loss': np.float32([0.25]), "
            "'w': big, 'd': np.float64([1.5])})")
    for sub in ("a", "b"):
        r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / sub)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["actions", "d", "done", "loss", "w"]
    assert a["actions"].dtype == np.float64 and a["actions"].tolist() == [0, 5, 2] and a["done"].tolist() == [1, 0]
    assert a["loss"].dtype == np.float32 and a["d"].dtype == np.float64
    w = a["w"]
    assert w.dtype == np.float32 and w.shape == (1 << 20,) and len(np.unique(w)) == 1 << 20 and (np.diff(w) > 0).all() and w.max() < 3 << 20
    assert np.array_equal(w, np.load(tmp_path / "b" / "w.npy"))  # the same positions in a second process


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); import bench; "
            "bench.dump_outputs(sys.argv[2], {'p%d' % i: np.zeros(1 << 20) for i in range(9)})")  # 9 x 8 MB of float64
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / "o")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "more than" in r.stderr and not (tmp_path / "o").exists()


@pytest.mark.gpu
def test_plain_bench_line_with_dump_outputs(tmp_path):
    """A plain run prints the contract's line and nothing measured beside it; --dump-outputs holds the last timed step's actions, environment step, learner
    update and online parameters, all finite."""
    steps, inner = 3, 4
    r = _bench("--gpus", "1", "--envs", "512", "--capacity", "20000", "--steps", str(steps), "--warmup", "1", "--inner", str(inner),
               "--dump-outputs", str(tmp_path / "out"), timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("env-steps/sec") and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and abs(d["value"] * d["ms_per_step"] * 1e-3 - inner * 512) < 1e-6 * inner * 512
    assert d["roofline"] is None and not {"subfigures", "per_micro", "cpu_baseline", "strong_ref"} & set(d)
    out = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert {"actions", "rewards", "done", "next_obs", "loss", "td_target", "priorities", "q_online.fc1.weight"} <= set(out)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20 and out["actions"].shape == (512,) and out["q_online.fc1.weight"].shape == (1 << 20,)
    assert ((out["actions"] >= 0) & (out["actions"] < 6)).all() and (out["priorities"] >= 0).all()
