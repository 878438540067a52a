"""Probe: R2D2 on its device engine (device/r2d2.py) at E = 16 and E = 64 lanes next to the plugin path (one host environment, one batch-1
LSTM pass per step) on the same configuration: environment steps per second and updates per second, and the split of an engine lock-step into actor pass, ring
push, priority adds and trainer calls.

    python tools/r2d2_engine_probe.py --out profiles/r2d2_engine_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/r2d2_engine_probe.py --trace-loop   # a run of its own, no counters

Everything goes through `Runner.train()`: the engine arms under set_vector_envs(E) with train_interval = E (one update per lock-step, the engines' operating
point), the plugin arm under set_vector_envs(0) with train_interval = 1 (one update per step, the reference's default).  The three arms run in ONE process,
interleaved three times after one untimed call each; every timing ends in a device synchronise.  The phase split is a pass of its own with the engine's
`phase_times` switched on (it synchronises around every phase, so it is not the throughput run).

Two GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the
GPU; tools/agent57_engine_probe.py's scaffold):
  throughput  the three arms interleaved, 200 lock-steps (engine) or 200 steps (plugin) per timed call
  split       the phase split of 200 lock-steps at E = 16 and at E = 64

Configuration: r2d2.Config()'s defaults (batch 32, burn-in 5 + sequence 5 + 1, 512 units, dueling (512,), retrace) on Grid, with a proportional memory of 20 000
windows, a warm-up of 64 and no item compression."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LANES = (16, 64)
LIMITS = dict(throughput=300, split=200)  # seconds per child


def _runner(vector_envs):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import r2d2

    rl = r2d2.Config()
    rl.memory.set_proportional()
    rl.memory.capacity, rl.memory.warmup_size, rl.memory.compress = 20_000, 64, False
    runner = srl.Runner("Grid", rl)
    runner.set_device("cuda:0")
    runner.set_seed(1)
    runner.set_vector_envs(vector_envs)
    return runner


def _timed_train(runner, steps, interval):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = runner.train(max_steps=steps, train_interval=interval, enable_progress=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(seconds=dt, env_steps=st.total_step, updates=st.train_count, env_steps_per_s=st.total_step / dt, updates_per_s=st.train_count / dt)


def throughput(lock_steps, plugin_steps, rounds=3):
    arms = {f"engine_E{E}": (_runner(E), lock_steps * E, E) for E in LANES}
    arms["plugin"] = (_runner(0), plugin_steps, 1)
    for name, (runner, steps, interval) in arms.items():  # untimed: allocation, warm-up of the memory, MIOpen's solver search
        _timed_train(runner, steps, interval)
        assert (runner.vector_reason == "") == name.startswith("engine"), (name, runner.vector_reason)
    runs = {a: [] for a in arms}
    for _ in range(rounds):
        for name, (runner, steps, interval) in arms.items():
            runs[name].append(_timed_train(runner, steps, interval))
    res = dict(what="Runner.train() on the R2D2 device engine (one update per lock-step) and on the plugin path (one update per step), one process, interleaved",
               config=dict(env="Grid", batch_size=32, burnin=5, sequence_length=5, lstm_units=512, hidden_block="dueling (512,)", memory="Proportional, 20000, warm-up 64",
                           lock_steps_per_timed_call=lock_steps, plugin_steps_per_timed_call=plugin_steps))
    for name, rs in runs.items():
        res[name] = dict(runs=rs, env_steps_per_s_mean=sum(r["env_steps_per_s"] for r in rs) / len(rs), updates_per_s_mean=sum(r["updates_per_s"] for r in rs) / len(rs))
    for E in LANES:
        res[f"engine_E{E}"]["env_steps_per_s_over_plugin"] = res[f"engine_E{E}"]["env_steps_per_s_mean"] / res["plugin"]["env_steps_per_s_mean"]
    return res


def split(lock_steps):
    """The phase split: a pass of its own, synchronised around every phase (host ms per lock-step)."""
    res = dict(what="host ms per lock-step by phase, the engine synchronising around each: actor pass (environments included), ring push, priority adds, trainer call")
    for E in LANES:
        runner = _runner(E)
        _timed_train(runner, 20 * E, E)  # untimed: allocation, warm-up of the memory
        eng = runner._vector_actor.engine
        eng.phase_times = {}
        for _ in range(lock_steps):
            eng.step(1)
        total = sum(eng.phase_times.values())
        res[f"engine_E{E}"] = dict(lock_step_split_ms={k: 1e3 * v / lock_steps for k, v in eng.phase_times.items()},
                                   lock_step_split_share={k: v / total for k, v in eng.phase_times.items()})
        eng.phase_times = None
    return res


def ring_bytes_at_atari_capacity():
    """HBM of the lane rings at set_atari_config()'s capacity (1 000 000 windows of 40 + 80 + 1 steps, 84 x 84 frames, 512 units, 18 actions): host arithmetic."""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, R2D2LaneStore

    return {f"E{E}": dict(rows=LaneLedger.default_ring_len(E, 1_000_000, 121, 79), bytes=R2D2LaneStore.ring_bytes(E, 1_000_000, 121, 80, 18, 512, 84 * 84)) for E in LANES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="throughput,split")
    ap.add_argument("--lock-steps", type=int, default=200)
    ap.add_argument("--plugin-steps", type=int, default=200)
    ap.add_argument("--child", default=None, help="(internal) run one GPU step in this process and print its JSON")
    ap.add_argument("--trace-loop", action="store_true", help="40 engine lock-steps at E = 64 with one update each, for a profiler")
    a = ap.parse_args()
    if a.trace_loop:
        _timed_train(_runner(64), 40 * 64, 64)
        return
    if a.child:
        res = throughput(a.lock_steps, a.plugin_steps) if a.child == "throughput" else split(a.lock_steps)
        print("PROBE-JSON " + json.dumps(res))
        return
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}  # steps measured by an earlier call stay
    for step in a.steps.split(","):
        t0 = time.time()
        print("step %s (limit %d s)" % (step, LIMITS[step]), flush=True)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--lock-steps", str(a.lock_steps), "--plugin-steps", str(a.plugin_steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step], cwd=ROOT)
        except subprocess.TimeoutExpired:
            res[step] = dict(error="no result within %d s" % LIMITS[step])
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE-JSON ")]
        if p.returncode != 0 or not line:
            res[step] = dict(error="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            break
        res[step] = dict(json.loads(line[-1][len("PROBE-JSON "):]), wall_s=time.time() - t0)
    res["ring_bytes_at_atari_capacity"] = ring_bytes_at_atari_capacity()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    if any("error" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
