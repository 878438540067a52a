"""DQN on CartPole-v1 through `Runner.train()` three ways: the device engine on the device CartPole (E = 1024 lanes), the device engine on host-stepped
copies of the environment (E = 64), and the plugin path (one environment, one update per step).  Config: tests/test_plugin_gpu.py's CartPole DQN (batch 32, (64, 64),
uniform replay).  Prints one JSON line: env-steps/s and updates/s of each, measured over a timed train() after an untimed warm one.  The runs learn at different
rates per env step (train_interval 32, 2 and 1): updates/s is the like-for-like figure.

    python tools/dqn_vec_probe.py [--seconds 10] [--only device_cartpole]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import simple_distributed_rl_amd as srl  # noqa: E402
from simple_distributed_rl_amd.algorithms import dqn  # noqa: E402
from simple_distributed_rl_amd.base.env import registration  # noqa: E402
from simple_distributed_rl_amd.envs.cartpole import CartPole  # noqa: E402


class HostCartPole(CartPole):
    """CartPole-v1 without the device batch environment: the engine steps E host copies."""

    device_vector = None


registration.register("HostCartPole-v1", __name__ + ":HostCartPole", {}, check_duplicate=False)


def config():
    rl = dqn.Config(batch_size=32, lr=0.001, target_model_update_interval=200, discount=0.99)
    rl.memory.set_replay_buffer()
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 500
    rl.epsilon_scheduler.set_linear(1.0, 0.05, 3000)
    rl.hidden_block.set((64, 64))
    return rl


def run(env_id: str, lanes, train_interval: int, seconds: float):
    runner = srl.Runner(env_id, config())
    runner.set_device("cuda:0")
    runner.set_vector_envs(lanes)
    runner.train(timeout=2, train_interval=train_interval, enable_progress=False)  # warm: replay past its warm-up, graphs captured
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = runner.train(timeout=seconds, train_interval=train_interval, enable_progress=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"path": "device" if runner.vector_reason == "" else "plugin", "lanes": lanes, "train_interval": train_interval, "seconds": round(dt, 3),
            "env_steps_per_s": round(st.total_step / dt), "updates_per_s": round(st.train_count / dt, 1)}


# name -> (environment id, lanes, train_interval): the device engine runs one update per `train_interval` env steps, the plugin path one per step
RUNS = {"device_cartpole": ("CartPole-v1", 1024, 32), "host_stepped": ("HostCartPole-v1", 64, 2), "plugin": ("CartPole-v1", "AUTO", 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--only", choices=sorted(RUNS), default=None, help="one of the three runs (e.g. under a kernel trace)")
    args = ap.parse_args()
    out = {k: run(*v, seconds=args.seconds) for k, v in RUNS.items() if args.only in (None, k)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
