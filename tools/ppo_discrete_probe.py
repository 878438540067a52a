"""Probe: discrete-action PPO on the device engine (categorical head, CartPole) at E = 4096 -- steady-state throughput of the fused engine (HIP graphs and eager),
of the torch-autograd path (`fused=False`), of the continuous Pendulum engine next to it, the rollout launch alone for both heads, and the PPO plugin
(`Runner.train` with `ppo.Config` on CartPole-v1: one environment on the host).  Every timing ends in a device synchronise and starts after warm-up iterations.

    python tools/ppo_discrete_probe.py --out profiles/ppo_discrete_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/ppo_discrete_probe.py --kernels-only    # a run of its own: the tracer slows the loop
    python tools/ppo_discrete_probe.py --merge-kernel-stats DIR --out profiles/ppo_discrete_probe.json                       # kernel times into the same file
    python tools/ppo_discrete_probe.py --graphs-only [--tree TREE]     # the CartPole engine, fused with graphs, alone: one JSON line (ppo_discrete_check.py bench-ab)
    rocprofv3 ... -- python tools/ppo_discrete_probe.py --kernels-only --arm config     # the CartPole engine of a mapped ppo.Config (a staircase schedule that steps
                                                                                         # inside the run, baseline_type "normal"); --arm default: the engine as it was
The `cartpole_plugin_config_graphs` arm runs `vector_runner.ppo_config_from(ppo.Config(), CartPole-v1, E, seed)` as it is: the default staircase schedule
set_step(2000, 0.01) evaluated inside k_ppo_adam, the environment's 500-step limit.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_ppo_rollout", "k_ppo_minibatch", "k_ppo_reduce", "k_ppo_adam", "k_ppo_adv_baseline", "k_categorical_act", "k_cartpole_auto", "k_ppo_forward")
# a kernel's head, from its template argument: the rollout's task (k_ppo_rollout<PendulumNormal> / <CartPoleCategorical>), CAT of the others
HEADS = (("<categorical>", ("<true>", "CartPoleCategorical")), ("<normal>", ("<false>", "PendulumNormal")))
# (builds before the rollout became one template had two kernels)
OLD_NAMES = (("k_ppo_cat_rollout(", "k_ppo_rollout<CartPoleCategorical>("), ("k_ppo_rollout(", "k_ppo_rollout<PendulumNormal>("))


def _engine(discrete, fused, E, T=32):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    kw = dict(obs_dim=4, n_actions=2, episode_len=500) if discrete else {}
    return PPOEngine(PPODeviceConfig(n_envs=E, horizon=T, seed=1, **kw), 0, fused=fused)


def _config_engine(E, T=32, **config_kw):
    """PPOEngine of a ppo.Config on CartPole-v1, mapped by vector_runner.ppo_config_from (config_kw: ppo.Config fields; `schedule`: (decay_steps, decay_rate) of a
    staircase in place of the default one)."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.device import vector_runner as vr
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    schedule = config_kw.pop("schedule", None)
    rl = ppo.Config(**config_kw)
    if schedule:
        rl.lr_scheduler.set_step(*schedule)
    runner = srl.Runner("CartPole-v1", rl)
    runner.setup_rl_config()
    why = vr.why_not_ppo_engine(runner.env, runner.rl_config)
    assert why == "", why
    return PPOEngine(vr.ppo_config_from(runner.rl_config, runner.env, E, 1, horizon=T), 0, fused=True)


def _throughput(eng, graphs, iters):
    import torch

    for _ in range(3):
        eng.step()
    if graphs:
        eng.capture_graphs()
    for _ in range(3):
        eng.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c = eng.cfg
    return dict(iterations=iters, seconds=dt, env_steps_per_s=iters * c.n_envs * c.horizon / dt, updates_per_s=iters * c.epochs * c.minibatches / dt,
                us_per_iteration=1e6 * dt / iters)


def _rollout_us(eng, calls=30):
    """device time of `eng.rollout()` alone (events around `calls` back-to-back launches; the kernel itself: the rocprofv3 run)"""
    import torch

    for _ in range(3):
        eng.rollout()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        eng.rollout()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def _plugin(seconds):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.utils.common import set_seed

    set_seed(7, enable_gpu=True)
    rl = ppo.Config(batch_size=64, lr=0.002, train_num=20, discount=0.98, gae_discount=0.95, entropy_weight=0.01, train_every_epoch=True)
    rl.memory.warmup_size = 1000
    rl.lr_scheduler.set_constant()
    runner = srl.Runner("CartPole-v1", rl)
    runner.set_device("cuda:0")
    runner.train(max_train_count=40, enable_progress=False)  # warm-up: the first buffer and its updates
    c0 = runner.trainer.train_count
    t0 = time.perf_counter()
    st = runner.train(timeout=seconds, enable_progress=False)
    dt = time.perf_counter() - t0
    steps = getattr(st, "total_step", None)
    return dict(seconds=dt, env_steps_per_s=None if steps is None else steps / dt, updates_per_s=(runner.trainer.train_count - c0) / dt,
                note="srl.Runner('CartPole-v1', ppo.Config(batch_size=64, train_num=20, train_every_epoch=True)).train(): one host environment; this path's code is the "
                     "parent commit's")


def kernel_stats(directory):
    """{kernel<head>: calls, average / min / max us} of the PPO kernels in a rocprofv3 --stats output directory (or one *kernel_stats.csv)"""
    rows = {}
    for f in [directory] if os.path.isfile(directory) else glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Name"]
            for old, new in OLD_NAMES:
                name = name.replace(old, new)
            for k in KERNELS:
                if k + "(" in name or k + "<" in name:
                    if k == "k_ppo_adam":  # its template argument is the schedule, not the head: k_ppo_adam<true> evaluates one, k_ppo_adam<false> is the constant rate
                        key = k + ("<scheduled>" if "k_ppo_adam<true>" in name else "")
                    else:
                        key = k + next((head for head, marks in HEADS if any(m in name for m in marks)), "")
                        key += "+options" if k == "k_ppo_rollout" and ", true>" in name else ""  # (reward / state clips, action rescale compiled in)
                    rows[key] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def _merge(directory, out):
    rows = kernel_stats(directory)
    d = json.load(open(out)) if os.path.exists(out) else {}
    d["kernels_rocprofv3"] = dict(sorted(rows.items()), note="E = 4096, T = 32, rocprofv3 --kernel-trace --stats in a run of its own (eager launches)")
    json.dump(d, open(out, "w"), indent=1)
    print(json.dumps(d["kernels_rocprofv3"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ppo_discrete_probe.json")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--plugin-seconds", type=float, default=20.0)
    ap.add_argument("--kernels-only", action="store_true", help="a few eager iterations of both heads and of the step-wise kernels, for a profiler")
    ap.add_argument("--arm", choices=("default", "config"), default="default", help="--kernels-only: the engines as they were, or the CartPole engine of a mapped ppo.Config")
    ap.add_argument("--merge-kernel-stats", default=None)
    ap.add_argument("--graphs-only", action="store_true", help="the CartPole engine, fused with graphs: one JSON line, no record")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.merge_kernel_stats:
        return _merge(a.merge_kernel_stats, a.out)
    import torch

    if a.kernels_only and a.arm == "config":
        eng = _config_engine(a.envs, baseline_type="normal", schedule=(50, 0.5))  # 160 optimiser steps: the staircase steps three times
        for _ in range(10):
            eng.step()
        torch.cuda.synchronize()
        return
    if a.kernels_only:
        for discrete in (True, False):
            eng = _engine(discrete, None, a.envs)
            for _ in range(10):
                eng.step()
        eng = _engine(True, None, a.envs)
        eng._fused_rollout_ok = lambda: False  # the one-purpose kernels, step by step
        for _ in range(3):
            eng.step()
        torch.cuda.synchronize()
        return
    if a.graphs_only:
        print(json.dumps(_throughput(_engine(True, True, a.envs), True, a.iters)))
        return
    from simple_distributed_rl_amd import _native as N

    res = dict(device=str(N.device_info(0)), envs=a.envs, horizon=32, epochs=4, minibatches=4)
    res["cartpole_fused_graphs"] = _throughput(_engine(True, True, a.envs), True, a.iters)
    res["cartpole_plugin_config_graphs"] = dict(_throughput(_config_engine(a.envs), True, a.iters),
                                                note="vector_runner.ppo_config_from(ppo.Config(), CartPole-v1, E, 1): lr_scheduler set_step(2000, 0.01) inside k_ppo_adam")
    res["cartpole_fused_eager"] = _throughput(_engine(True, True, a.envs), False, a.iters)
    res["cartpole_unfused_eager"] = _throughput(_engine(True, False, a.envs), False, max(4, a.iters // 6))
    res["pendulum_fused_graphs"] = _throughput(_engine(False, True, a.envs), True, a.iters)
    res["rollout_launch_us"] = dict(cartpole=_rollout_us(_engine(True, True, a.envs)), pendulum=_rollout_us(_engine(False, True, a.envs)),
                                    note="k_ppo_rollout<CartPoleCategorical> / <PendulumNormal> + the counter kernel behind it, back to back, event-timed")
    if a.plugin_seconds > 0:
        res["plugin_cartpole"] = _plugin(a.plugin_seconds)
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    old.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(old, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
