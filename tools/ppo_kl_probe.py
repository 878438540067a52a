"""Probe: PPO's adaptive-KL surrogate (surrogate_type "kl") on the device engine at E = 4096, T = 32, CartPole and Pendulum, next to the clipped surrogate.

    python tools/ppo_kl_probe.py --out profiles/ppo_kl_probe.json            # env-steps/s and updates/s of "clip" and "kl" in the same run, rounds interleaved
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/ppo_kl_probe.py --kernels-only     # a run of its own: the tracer slows the loop
    python tools/ppo_kl_probe.py --merge-kernel-stats DIR --out profiles/ppo_kl_kernel_times.json                       # per-kernel times of every instantiation
    python tools/ppo_kl_probe.py --learning --out profiles/ppo_kl_learning.json   # CartPole under "kl" and under "clip", same iterations: mean episode return (a record)
    python tools/ppo_kl_probe.py --dump DIR [--tree TREE]    # the "clip" engines' state after a few iterations as DIR/<name>.npy: two builds compare bit for bit

Every timing ends in a device synchronise and starts after warm-up iterations; the engines replay their captured graphs."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(discrete, surrogate, E, T=32, **kw):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=2, episode_len=500) if discrete else {}
    return PPOEngine(PPODeviceConfig(n_envs=E, horizon=T, seed=1, surrogate_type=surrogate, **head, **kw), 0, fused=True)


def _warm(eng):
    for _ in range(3):
        eng.step()
    eng.capture_graphs()
    for _ in range(3):
        eng.step()


def _timed(eng, iters):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c = eng.cfg
    return dict(seconds=dt, env_steps_per_s=iters * c.n_envs * c.horizon / dt, updates_per_s=iters * c.epochs * c.minibatches / dt, us_per_iteration=1e6 * dt / iters)


def _throughput(E, iters, rounds):
    res = {}
    for discrete, env in ((True, "cartpole"), (False, "pendulum")):
        engines = {s: _engine(discrete, s, E) for s in ("clip", "kl")}
        for eng in engines.values():
            _warm(eng)
        runs = {s: [] for s in engines}
        for _ in range(rounds):  # interleaved: clip, kl, clip, kl, ...
            for s, eng in engines.items():
                runs[s].append(_timed(eng, iters))
        for s, eng in engines.items():
            key = "%s_%s" % (env, s)
            res[key] = dict(iterations=iters, rounds=runs[s], env_steps_per_s_mean=sum(r["env_steps_per_s"] for r in runs[s]) / rounds,
                            updates_per_s_mean=sum(r["updates_per_s"] for r in runs[s]) / rounds, info=eng.info())
        res[env + "_kl_over_clip_env_steps"] = res[env + "_kl"]["env_steps_per_s_mean"] / res[env + "_clip"]["env_steps_per_s_mean"]
    return res


def kernel_stats(directory):
    """{kernel with its template arguments: calls, average / min / max us} of the PPO kernels in a rocprofv3 --stats output directory"""
    rows = {}
    for f in [directory] if os.path.isfile(directory) else glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Name"].replace("(anonymous namespace)::", "")
            m = re.search(r"(k_ppo_[a-z_]+)(<[^>(]*>)?", name)
            if m:
                rows[m.group(1) + (m.group(2) or "")] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def _learning(E, iterations, every):
    import torch

    curves = {}
    for s in ("kl", "clip"):
        eng = _engine(True, s, E)
        _warm(eng)
        eng.pop_mean_episode_return()
        curve = []
        for it in range(iterations):
            eng.step()
            if (it + 1) % every == 0:
                torch.cuda.synchronize()
                curve.append(dict(iteration=it + 1, mean_episode_return=eng.pop_mean_episode_return(), **eng.info()))
        curves[s] = curve
    return dict(env="CartPole (episode_len 500)", envs=E, horizon=32, iterations=iterations, curves=curves,
                note="the reference's default hyper-parameters otherwise (adaptive_kl_target 0.01); a record, not a gate")


def _dump(path, E):
    """the "clip" engines (both heads) after four iterations, two eager and two replayed: parameters, Adam moments, the last rollout's buffers, the losses"""
    import numpy as np
    import torch

    os.makedirs(path, exist_ok=True)
    for discrete, env in ((True, "cartpole"), (False, "pendulum")):
        eng = _engine(discrete, "clip", E)
        eng.step()
        eng.step()
        eng.capture_graphs()
        eng.step()
        eng.step()
        torch.cuda.synchronize()
        for name in ("flat", "exp_avg", "exp_avg_sq", "b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_adv", "losses", "episode_return"):
            np.save(os.path.join(path, "%s_%s.npy" % (env, name)), getattr(eng, name).cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="eager iterations of both heads under both surrogates, for a profiler")
    ap.add_argument("--merge-kernel-stats", default=None)
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--learning-iterations", type=int, default=150)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.merge_kernel_stats:
        res = dict(sorted(kernel_stats(a.merge_kernel_stats).items()), note="E = %d, T = 32, rocprofv3 --kernel-trace --stats in a run of its own (eager launches)" % a.envs)
    else:
        import torch

        from simple_distributed_rl_amd import _native as N

        if a.dump:
            return _dump(a.dump, a.envs)
        if a.kernels_only:
            for discrete in (True, False):
                for s in ("clip", "kl"):
                    eng = _engine(discrete, s, a.envs)
                    for _ in range(10):
                        eng.step()
            torch.cuda.synchronize()
            return
        res = dict(device=str(N.device_info(0)), envs=a.envs, horizon=32, epochs=4, minibatches=4)
        res.update(_learning(1024, a.learning_iterations, 10) if a.learning else _throughput(a.envs, a.iters, a.rounds))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
