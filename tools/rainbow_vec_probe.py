"""Rainbow on CartPole-v1 on the MLP Q-network engine (device/mlpq.py:VectorQEngine with a dueling head and n-step items), next to the plugin path's Rainbow and
to the DQN engine at the same lane count.  `Runner.train()` does not route Rainbow on flat observations to the engine yet, so the engine runs are driven here:
E = 1024 lanes of the device CartPole, 32 updates per lock-step (one per 32 env steps, tools/dqn_vec_probe.py's ratio), the update replayed from its captured
graph.  Configs: rainbow.Config() (dueling (512,), n = 3, proportional replay), the same with the dueling block (64, 64), the same with `enable_noisy_dense`
(`rainbow_noisy`: NoisyLinear head, greedy acting; next to it the same config on the plugin path); DQN with the hidden block (64, 64).
Prints one JSON line and writes it to profiles/rainbow_vec_probe.json: env-steps/s and updates/s of each run, measured over a timed stretch after an untimed warm
one.  The plugin path runs one environment with one update per step: updates/s is the like-for-like figure.

    python tools/rainbow_vec_probe.py [--seconds 10] [--only rainbow_default] [--no-write]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import simple_distributed_rl_amd as srl  # noqa: E402
from simple_distributed_rl_amd.algorithms import dqn, rainbow  # noqa: E402
from simple_distributed_rl_amd.device import vector_runner as vr  # noqa: E402

LANES, UPDATES_PER_LOCKSTEP = 1024, 32


def rainbow_config(layer_sizes=(512,), noisy=False):
    rl = rainbow.Config(enable_noisy_dense=noisy)
    rl.hidden_block.set_dueling_network(layer_sizes)
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 2048
    return rl


def dqn_config():
    rl = dqn.Config(batch_size=32, lr=0.001, target_model_update_interval=200, discount=0.99)
    rl.memory.set_replay_buffer()
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 2048
    rl.hidden_block.set((64, 64))
    return rl


def run_engine(rl_config, seconds: float):
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    runner = srl.Runner("CartPole-v1", rl_config)
    runner.set_device("cuda:0")
    runner.setup_rl_config()
    if vr.engine_kind(runner.rl_config) == "rainbow":
        why = vr.why_not_flat_rainbow(runner.env, runner.rl_config, admit_noisy=True)
        assert why == "", why
    eng = VectorQEngine(vr.mlp_config_from(runner.rl_config, runner.env, LANES, 0), 0)
    while eng.replay.is_warmup_needed():
        eng.actor_step()
    eng.capture_graphs(actor=False, warm_actor=False)
    for _ in range(20):
        eng.step(learner_updates=UPDATES_PER_LOCKSTEP)
    torch.cuda.synchronize()
    u0, s0, t0 = eng.train_count, eng.total_env_steps, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            eng.step(learner_updates=UPDATES_PER_LOCKSTEP)
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    info = eng.info()
    return {"path": "device", "lanes": LANES, "updates_per_lockstep": UPDATES_PER_LOCKSTEP, "multisteps": eng.cfg.multisteps, "dueling_units": eng.cfg.dueling_units,
            "noisy": bool(eng.cfg.enable_noisy_dense),
            "trunk": list(eng.cfg.in_sizes + eng.cfg.hidden_sizes), "seconds": round(dt, 3), "env_steps_per_s": round((eng.total_env_steps - s0) / dt),
            "updates_per_s": round((eng.train_count - u0) / dt, 1), "loss": info["loss"]}


def run_plugin(rl_config, seconds: float):
    runner = srl.Runner("CartPole-v1", rl_config)
    runner.set_device("cuda:0")
    runner.train(timeout=2, enable_progress=False)  # warm: the replay past its warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = runner.train(timeout=seconds, enable_progress=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"path": "device" if runner.vector_reason == "" else "plugin", "lanes": 1, "seconds": round(dt, 3), "env_steps_per_s": round(st.total_step / dt),
            "updates_per_s": round(st.train_count / dt, 1)}


def plugin_config(noisy=False):
    rl = rainbow.Config(enable_noisy_dense=noisy)
    rl.memory.warmup_size = 500
    return rl


RUNS = {
    "rainbow_default": lambda s: run_engine(rainbow_config((512,)), s),
    "rainbow_64x64": lambda s: run_engine(rainbow_config((64, 64)), s),
    "dqn_64x64": lambda s: run_engine(dqn_config(), s),
    "rainbow_plugin": lambda s: run_plugin(plugin_config(), s),
    "rainbow_noisy": lambda s: run_engine(rainbow_config((512,), noisy=True), s),
    "rainbow_noisy_plugin": lambda s: run_plugin(plugin_config(noisy=True), s),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--only", choices=sorted(RUNS), default=None, help="one of the runs (e.g. under a kernel trace)")
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    out = {k: f(args.seconds) for k, f in RUNS.items() if args.only in (None, k)}
    print(json.dumps(out))
    if not args.no_write and args.only is None:
        with open(os.path.join(ROOT, "profiles", "rainbow_vec_probe.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
