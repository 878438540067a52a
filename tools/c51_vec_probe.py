"""C51 on CartPole-v1 on the MLP Q-network engine (device/mlpq.py:VectorQEngine with `categorical_atoms`), next to the DQN engine driven the same way in the same
process and to C51 on the plugin path.  The engine arms: E = 1024 lanes of the device CartPole, 32 updates per lock-step (one per 32 env steps,
tools/dqn_vec_probe.py's ratio), B = 32, the update replayed from its captured graph; c51.Config() as it is (hidden block (512,), 51 atoms) and dqn.Config() with
the same hidden block and the uniform memory.  The plugin arm: `Runner.train()` under set_vector_envs(0), one environment, one update per step.
The arms are INTERLEAVED: `--rounds` rounds, each running every arm for `--seconds`; per arm the median round is reported and every round is listed.
Prints one JSON line and writes it to profiles/c51_vec_probe.json.  The only yardstick for a time here is the DQN arm of the same run.

    python tools/c51_vec_probe.py [--seconds 4] [--rounds 3] [--only c51_engine] [--no-write]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import simple_distributed_rl_amd as srl  # noqa: E402
from simple_distributed_rl_amd.algorithms import c51, dqn  # noqa: E402
from simple_distributed_rl_amd.device import vector_runner as vr  # noqa: E402

LANES, UPDATES_PER_LOCKSTEP = 1024, 32


def c51_config():
    rl = c51.Config()
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 2048
    return rl


def dqn_config():
    rl = dqn.Config(batch_size=32, lr=0.001)
    rl.memory.set_replay_buffer()
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 2048
    return rl


class EngineArm:
    def __init__(self, rl_config):
        from simple_distributed_rl_amd.device.mlpq import VectorQEngine

        runner = srl.Runner("CartPole-v1", rl_config)
        runner.set_device("cuda:0")
        runner.setup_rl_config()
        kind = vr.engine_kind(runner.rl_config)
        cfg = (vr.c51_config_from if kind == "c51" else vr.mlp_config_from)(runner.rl_config, runner.env, LANES, 0)
        self.eng = eng = VectorQEngine(cfg, 0)
        while eng.replay.is_warmup_needed():
            eng.actor_step()
        eng.capture_graphs(actor=False, warm_actor=False)
        for _ in range(20):
            eng.step(learner_updates=UPDATES_PER_LOCKSTEP)
        torch.cuda.synchronize()
        self.about = {"path": "device", "lanes": LANES, "updates_per_lockstep": UPDATES_PER_LOCKSTEP, "batch_size": cfg.batch_size,
                      "categorical_atoms": cfg.categorical_atoms, "trunk": list(cfg.in_sizes + cfg.hidden_sizes)}

    def stretch(self, seconds: float):
        eng = self.eng
        torch.cuda.synchronize()
        u0, s0, t0 = eng.train_count, eng.total_env_steps, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(10):
                eng.step(learner_updates=UPDATES_PER_LOCKSTEP)
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"seconds": round(dt, 3), "env_steps_per_s": round((eng.total_env_steps - s0) / dt), "updates_per_s": round((eng.train_count - u0) / dt, 1)}

    def end(self):
        return {"loss": self.eng.info()["loss"]}


class PluginArm:
    def __init__(self, rl_config):
        rl_config.memory.warmup_size = 500
        self.runner = srl.Runner("CartPole-v1", rl_config)
        self.runner.set_device("cuda:0")
        self.runner.set_vector_envs(0)
        self.runner.train(timeout=2, enable_progress=False)  # warm: the replay past its warm-up
        self.about = {"path": "plugin", "lanes": 1, "batch_size": rl_config.batch_size, "reason": self.runner.vector_reason}

    def stretch(self, seconds: float):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = self.runner.train(timeout=seconds, enable_progress=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"seconds": round(dt, 3), "env_steps_per_s": round(st.total_step / dt), "updates_per_s": round(st.train_count / dt, 1)}

    def end(self):
        return {}


ARMS = {
    "c51_engine": lambda: EngineArm(c51_config()),
    "dqn_engine": lambda: EngineArm(dqn_config()),
    "c51_plugin": lambda: PluginArm(c51.Config()),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0, help="length of one arm's stretch in one round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=sorted(ARMS), default=None, help="one of the arms (e.g. under a kernel trace)")
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    arms = {k: f() for k, f in ARMS.items() if args.only in (None, k)}
    rounds = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, arm in arms.items():
            rounds[k].append(arm.stretch(args.seconds))
    out = {}
    for k, arm in arms.items():
        out[k] = dict(arm.about, updates_per_s=statistics.median(r["updates_per_s"] for r in rounds[k]),
                      env_steps_per_s=statistics.median(r["env_steps_per_s"] for r in rounds[k]), rounds=rounds[k], **arm.end())
    print(json.dumps(out))
    if not args.no_write and args.only is None:
        with open(os.path.join(ROOT, "profiles", "c51_vec_probe.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
