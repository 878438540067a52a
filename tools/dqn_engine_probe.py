"""DQN (plain Q head, libsrlx dueling_type 3) against Rainbow (dueling 512) on the device engine at bench.py's operating point -- 1 024 environments, one update
per lock-step, 1 M replay, fast lock-step captured in graphs -- alternated in one process (rounds of `--steps` lock-steps each), same box, same method as bench.py.
Prints one JSON line: ms per lock-step, env-steps/s and updates/s per algorithm (median over rounds).

    python tools/dqn_engine_probe.py [--rounds 5] [--steps 256]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from simple_distributed_rl_amd.device.rainbow import RainbowDeviceConfig, RainbowEngine  # noqa: E402


def make(kind: str, E: int, capacity: int):
    if kind == "dqn":  # dqn.Config().set_atari_config() as device_config_from maps it (double DQN off, 1-step targets, uniform replay), one layer of 512
        cfg = RainbowDeviceConfig(n_envs=E, batch_size=32, memory_capacity=capacity, seed=0, multisteps=1, enable_double_dqn=False, hidden_units=512, plain_head=True,
                                  lr=0.00025, memory_alpha=0.0, memory_has_duplicate=False)
    else:  # bench.py's engine
        cfg = RainbowDeviceConfig(n_envs=E, batch_size=32, memory_capacity=capacity, seed=0)
    eng = RainbowEngine(cfg, 0, 200, overlap=True)
    assert eng.fast
    eng.prefill()
    for _ in range(8):
        eng.step(1)
    eng.capture_graphs()
    for _ in range(16):
        eng.step(1)
    torch.cuda.synchronize()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=256, help="lock-steps per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    engines = {k: make(k, args.envs, args.capacity) for k in ("dqn", "rainbow")}
    ms = {k: [] for k in engines}
    for _ in range(args.rounds):
        for k, eng in engines.items():
            trained0 = eng.train_count
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.step(1)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            assert eng.train_count - trained0 == args.steps
    out = {"envs": args.envs, "updates_per_lockstep": 1, "rounds": args.rounds, "lockstep_per_round": args.steps}
    for k, v in ms.items():
        m = statistics.median(v)
        out[k] = {"ms_per_lockstep": round(m, 4), "env_steps_per_s": round(args.envs / m * 1e3), "updates_per_s": round(1e3 / m, 1),
                  "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    out["dqn_over_rainbow"] = round(out["dqn"]["ms_per_lockstep"] / out["rainbow"]["ms_per_lockstep"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
