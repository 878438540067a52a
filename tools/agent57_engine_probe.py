"""Probe: Agent57 (the LSTM one) on its device engine (device/agent57.py) at E = 16 and E = 64 lanes next to the plugin path (one host
environment, two batch-1 LSTM passes per step) on the same configuration: environment steps per second and updates per second, and the split of an engine
lock-step into actor pass, ring push, priority adds and trainer calls.

    python tools/agent57_engine_probe.py --out profiles/agent57_engine_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/agent57_engine_probe.py --trace-loop   # a run of its own, no counters

Everything goes through `Runner.train()`: the engine arms under set_vector_envs(E) with train_interval = E (one update per lock-step, the engines' operating
point), the plugin arm under set_vector_envs(0) with train_interval = 1 (one update per step, the reference's default).  The three arms run in ONE process,
interleaved three times after one untimed call each; every timing ends in a device synchronise.  The phase split is a pass of its own with the engine's
`phase_times` switched on (it synchronises around every phase, so it is not the throughput run).

Two GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the
GPU; tools/agent57_lstm_probe.py's scaffold):
  throughput  the three arms interleaved, 300 lock-steps (engine) or 300 steps (plugin) per timed call: about 3 s each
  split       the phase split of 300 lock-steps at E = 16 and at E = 64

Configuration: the golden's small one (batch 8, burn-in 2 + sequence 3 + 1, 16 units) on `ProbeImg` below: 8 x 8 x 1 random frames, 4 actions, episodes of 20
steps."""
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


import numpy as np  # noqa: E402

from simple_distributed_rl_amd.base.define import SpaceTypes  # noqa: E402
from simple_distributed_rl_amd.base.env import registration  # noqa: E402
from simple_distributed_rl_amd.base.env.base import EnvBase  # noqa: E402
from simple_distributed_rl_amd.base.spaces.box import BoxSpace  # noqa: E402
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace  # noqa: E402


class ProbeImg(EnvBase):
    """Seeded random 8 x 8 x 1 frames in [0, 1], 4 actions, rewards in -2..2, terminated after `ep_len` steps."""

    def __init__(self, ep_len=20, seed=0):
        super().__init__()
        self.ep_len, self.rng = ep_len, np.random.default_rng(seed)

    action_space = property(lambda self: DiscreteSpace(4))
    observation_space = property(lambda self: BoxSpace((8, 8, 1), 0, 1, np.float32, SpaceTypes.GRAY_HW1))
    max_episode_steps = property(lambda self: 1000)
    player_num = property(lambda self: 1)

    def _frame(self):
        return self.rng.integers(0, 256, (8, 8, 1)).astype(np.float32) / 255

    def reset(self, **kw):
        self.t = 0
        return self._frame()

    def step(self, action):
        self.t += 1
        return self._frame(), float(self.rng.integers(-2, 3)), self.t >= self.ep_len, False

    def backup(self, **kw):
        return None

    def restore(self, d, **kw):
        pass


registration.register("ProbeImg", "agent57_engine_probe:ProbeImg", check_duplicate=False)  # (tools/ is on sys.path: the registry imports this file by name)


def _runner(vector_envs):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import agent57

    rl = agent57.Config(batch_size=8, actor_num=4, target_model_update_interval=5, lr_ext=0.001, lr_int=0.002, lstm_units=16, burnin=2, sequence_length=3)
    rl.window_length = 1
    rl.hidden_block.set_dueling_network((16,))
    rl.memory.capacity, rl.memory.warmup_size, rl.memory.compress = 20_000, 64, False
    rl.episodic_memory_capacity = 64
    runner = srl.Runner(srl.EnvConfig("ProbeImg", kwargs=dict(ep_len=20, seed=1)), rl)
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
    res = dict(what="Runner.train() on the Agent57 device engine (one update per lock-step) and on the plugin path (one update per step), one process, interleaved",
               config=dict(batch_size=8, burnin=2, sequence_length=3, lstm_units=16, frame=[8, 8, 1], episode_len=20, intrinsic_reward=True,
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
    """HBM of the lane rings at set_atari_config()'s capacity (100 000 windows of 40 + 80 + 1 steps, 84 x 84 frames, 512 units, 18 actions): host arithmetic."""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, LaneSequenceStore

    return {f"E{E}": dict(rows=LaneLedger.default_ring_len(E, 100_000, 121), bytes=LaneSequenceStore.ring_bytes(E, 100_000, 121, 18, 512, 84 * 84)) for E in LANES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="throughput,split")
    ap.add_argument("--lock-steps", type=int, default=300)
    ap.add_argument("--plugin-steps", type=int, default=300)
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
