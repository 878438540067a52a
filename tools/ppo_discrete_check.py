"""The records of a PPO engine change that compare this build with its parent commit, and the categorical head's learning curve.  PARENT is a built checkout of the
parent commit (its own libsrlx.so); every sub-command runs on one MI355X.  `--records PREFIX` (before the sub-command; default profiles/ppo_discrete) names the
records: PREFIX_parity.json, PREFIX_bench_ab.json, PREFIX_kernel_times.json, PREFIX_learning.json (a sub-command's own --out overrides it).

    python tools/ppo_discrete_check.py parity-run --tree PARENT --out parent.pt      # seeded PPOEngines of both heads in that tree -> parameters, buffers, counters
    python tools/ppo_discrete_check.py parity-run --tree . --out new.pt
    python tools/ppo_discrete_check.py parity-compare parent.pt new.pt               # -> PREFIX_parity.json; exit status 1 unless every tensor is bit-identical
    python tools/ppo_discrete_check.py bench-ab --parent PARENT                      # bench.py --algo ppo and the CartPole engine (ppo_discrete_probe.py --graphs-only),
                                                                                     # alternating, three runs each -> PREFIX_bench_ab.json
    python tools/ppo_discrete_check.py kernel-times --parent DIR DIR --new DIR       # three `rocprofv3 --kernel-trace --stats` runs of ppo_discrete_probe.py --kernels-only
    python tools/ppo_discrete_check.py learning                                      # the curve tests/test_ppo_discrete_gpu.py::test_engine_learns_cartpole quotes
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, PPODeviceConfig fields, PPOEngine's `fused`): both heads, the libsrlx network and the torch-autograd path; EAGER iterations, then capture_graphs(), then GRAPH
# iterations
_CARTPOLE = dict(obs_dim=4, episode_len=500)
PARITY_CASES = (("default", dict(seed=7, n_envs=1024), None), ("action_dim_3", dict(seed=11, n_envs=512, action_dim=3, horizon=16), None),
                ("cartpole_2_actions", dict(seed=7, n_envs=1024, n_actions=2, **_CARTPOLE), None),
                ("cartpole_5_actions", dict(seed=11, n_envs=512, n_actions=5, horizon=16, **_CARTPOLE), None),
                ("unfused", dict(seed=3, n_envs=256, horizon=16), False), ("cartpole_unfused", dict(seed=3, n_envs=256, n_actions=2, horizon=16, **_CARTPOLE), False))
EAGER, GRAPH = 8, 8
# what a case records of its engine: the parameters, every rollout buffer, the counters and the optimiser's state
ENGINE_TENSORS = ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "_last_v", "_perms", "act_counter", "perm_counter", "episode_return", "finished_returns", "losses")
FUSED_TENSORS = ("flat", "flat_grad", "exp_avg", "exp_avg_sq", "opt_step", "partials")
ENV_TENSORS = ("state", "t", "obs", "counter", "episodes")


def parity_run(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import torch

    import simple_distributed_rl_amd

    assert os.path.abspath(simple_distributed_rl_amd.__file__).startswith(tree), simple_distributed_rl_amd.__file__
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    res = {}
    for name, kw, fused in PARITY_CASES:
        eng = PPOEngine(PPODeviceConfig(**kw), 0, fused=fused)
        assert eng.fused == (fused is None)
        for _ in range(EAGER):
            eng.step()
        eng.capture_graphs()  # (one whole iteration itself, as its warm-up)
        for _ in range(GRAPH):
            eng.step()
        torch.cuda.synchronize()
        t = {"parameters": torch.cat([p.detach().reshape(-1) for p in eng.net.parameters()])}
        t.update({k: getattr(eng, k) for k in ENGINE_TENSORS + (FUSED_TENSORS if eng.fused else ())})
        t.update({"env." + k: getattr(eng.env, k) for k in ENV_TENSORS if hasattr(eng.env, k)})
        res[name] = {k: v.detach().cpu() for k, v in t.items()}
        print(name, _sha(res[name]["parameters"]), flush=True)
    torch.save(res, out)


def _sha(t):
    return hashlib.sha256(t.contiguous().view(-1).view(dtype=__import__("torch").uint8).numpy().tobytes()).hexdigest()


def parity_compare(a_path, b_path, out):
    import torch

    a, b = torch.load(a_path), torch.load(b_path)
    res = dict(what="parameters, rollout buffers, counters, optimiser and environment state of seeded PPOEngines (both heads; fused: None = the libsrlx network, False = "
                    "torch autograd) in the parent commit's tree and in this build's; a tensor is identical when its bytes are",
               schedule="%d eager iterations, capture_graphs() (one iteration), %d graph-replayed iterations" % (EAGER, GRAPH), cases={})
    for name, kw, fused in PARITY_CASES:
        differing = sorted(k for k in set(a[name]) | set(b[name]) if k not in a[name] or k not in b[name] or _sha(a[name][k]) != _sha(b[name][k]))
        res["cases"][name] = dict(config=kw, fused=fused, tensors=len(b[name]), parameters=int(b[name]["parameters"].numel()), bit_identical=not differing,
                                  differing=differing, sha256_parameters=_sha(b[name]["parameters"]), sha256_b_adv=_sha(b[name]["b_adv"]))
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if all(c["bit_identical"] for c in res["cases"].values()) else 1


def bench_ab(parent, out, steps, warmup):
    trees = {"parent": os.path.abspath(parent), "new": ROOT}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = ["bench.py", "--algo", "ppo", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline"]
    probe = [os.path.join(ROOT, "tools", "ppo_discrete_probe.py"), "--graphs-only"]  # (this checkout's probe; --tree: the package it drives)
    val, upd, cart = {"parent": [], "new": []}, {"parent": [], "new": []}, {"parent": [], "new": []}
    for rep in range(3):
        for name in ("parent", "new"):
            for c in (cmd, probe + ["--tree", trees[name]]):
                r = subprocess.run([sys.executable] + c, cwd=trees[name], env=env, capture_output=True, text=True, timeout=170)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode != 0 or len(lines) != 1:
                    print(r.stdout[-2000:], r.stderr[-3000:])
                    return 1
                d = json.loads(lines[0])
                if c is cmd:
                    val[name].append(d["value"])
                    upd[name].append(d["learner_updates_per_s"])
                else:
                    cart[name].append(d["env_steps_per_s"])
                print(rep, name, d, flush=True)

    def verdict(p, n):
        r = dict(parent=p, new=n, parent_spread=max(p) - min(p), parent_slowest=min(p), new_median=statistics.median(n), bound=min(p) - (max(p) - min(p)))
        r["new_median_not_below_bound"] = r["new_median"] >= r["bound"]
        return r

    res = dict(command=" ".join(cmd) + ": the parent commit's tree and this build's, alternating in one session, three runs each", unit="env-steps/s",
               rule="the new median is not below the parent's slowest run minus the parent's own max - min spread", **verdict(val["parent"], val["new"]),
               parent_updates_per_s=upd["parent"], new_updates_per_s=upd["new"])
    res["categorical"] = dict(command="tools/ppo_discrete_probe.py --graphs-only --tree TREE: the CartPole engine, fused with graphs, E = 4096; run behind each bench.py run above",
                              **verdict(cart["parent"], cart["new"]))
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if res["new_median_not_below_bound"] and res["categorical"]["new_median_not_below_bound"] else 1


def kernel_times(parent_dirs, new_dir, out):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ppo_discrete_probe import kernel_stats

    p1, p2, n = (kernel_stats(d) for d in (*parent_dirs, new_dir))
    res = dict(what="average kernel times (us) of ppo_discrete_probe.py --kernels-only under rocprofv3 --kernel-trace --stats: the parent commit's build twice, this build once",
               rule="the new average is not above the parent's slower run plus the difference between the parent's two runs", kernels={})
    for k in ("k_ppo_rollout<normal>", "k_ppo_rollout<categorical>", "k_ppo_minibatch<normal>", "k_ppo_minibatch<categorical>"):
        a, b, c = p1[k]["average_us"], p2[k]["average_us"], n[k]["average_us"]
        res["kernels"][k] = dict(parent=[a, b], new=c, bound=max(a, b) + abs(a - b), new_not_above_bound=c <= max(a, b) + abs(a - b))
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if all(k["new_not_above_bound"] for k in res["kernels"].values()) else 1


def learning(out):
    sys.path.insert(0, ROOT)
    import torch

    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    kw = dict(obs_dim=4, n_actions=2, n_envs=1024, horizon=32, episode_len=500)  # tests/test_ppo_discrete_gpu.py: LEARNING; otherwise the defaults
    res = dict(config=kw, reading="mean return of the episodes finished in each 20 iterations, 200 iterations", curves={})
    for seed in (1, 2):
        eng = PPOEngine(PPODeviceConfig(seed=seed, **kw), 0)
        curve = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(200):
            eng.step()
            if (it + 1) % 20 == 0:
                curve.append(round(eng.pop_mean_episode_return(), 2))
        torch.cuda.synchronize()
        res["curves"]["seed_%d" % seed] = dict(curve=curve, rise_first_to_last=round(curve[-1] - curve[0], 2), seconds_for_the_200_iterations=round(time.perf_counter() - t0, 3))
        print(seed, curve, flush=True)
    res["smaller_rise"] = min(c["rise_first_to_last"] for c in res["curves"].values())
    json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default=os.path.join(ROOT, "profiles", "ppo_discrete"), help="prefix of the records' paths")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("parity-run")
    p.add_argument("--tree", required=True)
    p.add_argument("--out", required=True)
    p = sub.add_parser("parity-compare")
    p.add_argument("parent")
    p.add_argument("new")
    p.add_argument("--out", default=None)
    p = sub.add_parser("bench-ab")
    p.add_argument("--parent", required=True)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--out", default=None)
    p = sub.add_parser("kernel-times")
    p.add_argument("--parent", nargs=2, required=True)
    p.add_argument("--new", required=True)
    p.add_argument("--out", default=None)
    p = sub.add_parser("learning")
    p.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "parity-run":
        return parity_run(a.tree, a.out)
    out = a.out or "%s_%s.json" % (a.records, {"parity-compare": "parity"}.get(a.cmd, a.cmd.replace("-", "_")))
    if a.cmd == "parity-compare":
        return parity_compare(a.parent, a.new, out)
    if a.cmd == "bench-ab":
        return bench_ab(a.parent, out, a.steps, a.warmup)
    if a.cmd == "kernel-times":
        return kernel_times(a.parent, a.new, out)
    return learning(out)


if __name__ == "__main__":
    sys.exit(main())
