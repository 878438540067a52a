"""The records of the discrete-action PPO change that compare this build with its parent commit, and its learning curve.  PARENT is a built checkout of the parent
commit (its own libsrlx.so); every sub-command runs on one MI355X.

    python tools/ppo_discrete_check.py parity-run --tree PARENT --out parent.pt      # a seeded continuous PPOEngine in that tree -> its flat parameter vectors
    python tools/ppo_discrete_check.py parity-run --tree . --out new.pt
    python tools/ppo_discrete_check.py parity-compare parent.pt new.pt               # -> profiles/ppo_discrete_continuous_parity.json; exit status 1 unless bit-identical
    python tools/ppo_discrete_check.py bench-ab --parent PARENT                      # bench.py --algo ppo, alternating, three runs each -> profiles/ppo_discrete_bench_ab.json
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
# (name, PPODeviceConfig fields): n_actions stays 0 -- the continuous engine; EAGER iterations, then capture_graphs(), then GRAPH iterations
PARITY_CASES = (("default", dict(seed=7, n_envs=1024)), ("action_dim_3", dict(seed=11, n_envs=512, action_dim=3, horizon=16)))
EAGER, GRAPH = 8, 8


def parity_run(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import torch

    import simple_distributed_rl_amd

    assert os.path.abspath(simple_distributed_rl_amd.__file__).startswith(tree), simple_distributed_rl_amd.__file__
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    res = {}
    for name, kw in PARITY_CASES:
        eng = PPOEngine(PPODeviceConfig(**kw), 0)
        assert eng.fused
        for _ in range(EAGER):
            eng.step()
        eng.capture_graphs()  # (one whole iteration itself, as its warm-up)
        for _ in range(GRAPH):
            eng.step()
        torch.cuda.synchronize()
        res[name] = eng.flat.cpu()
        print(name, hashlib.sha256(res[name].numpy().tobytes()).hexdigest())
    torch.save(res, out)


def parity_compare(a_path, b_path, out):
    import torch

    a, b = torch.load(a_path), torch.load(b_path)
    res = dict(what="flat parameter vector of a seeded continuous PPOEngine (fused network) in the parent commit's tree and in this build's",
               schedule="%d eager iterations, capture_graphs() (one iteration), %d graph-replayed iterations" % (EAGER, GRAPH), cases={})
    for name, kw in PARITY_CASES:
        res["cases"][name] = dict(config=kw, parameters=int(a[name].numel()), bit_identical=bool(torch.equal(a[name], b[name])),
                                  max_abs_diff=float((a[name] - b[name]).abs().max()), sha256=hashlib.sha256(b[name].numpy().tobytes()).hexdigest())
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if all(c["bit_identical"] for c in res["cases"].values()) else 1


def bench_ab(parent, out, steps, warmup):
    trees = {"parent": os.path.abspath(parent), "new": ROOT}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = ["bench.py", "--algo", "ppo", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline"]
    val, upd = {"parent": [], "new": []}, {"parent": [], "new": []}
    for rep in range(3):
        for name in ("parent", "new"):
            r = subprocess.run([sys.executable] + cmd, cwd=trees[name], env=env, capture_output=True, text=True, timeout=170)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or len(lines) != 1:
                print(r.stdout[-2000:], r.stderr[-3000:])
                return 1
            d = json.loads(lines[0])
            val[name].append(d["value"])
            upd[name].append(d["learner_updates_per_s"])
            print(rep, name, d["value"], d["learner_updates_per_s"], flush=True)
    p, n = val["parent"], val["new"]
    res = dict(command=" ".join(cmd) + ": the parent commit's tree and this build's, alternating in one session, three runs each", unit="env-steps/s", parent=p, new=n,
               parent_updates_per_s=upd["parent"], new_updates_per_s=upd["new"], parent_spread=max(p) - min(p), parent_slowest=min(p), new_median=statistics.median(n),
               bound=min(p) - (max(p) - min(p)), rule="the new median is not below the parent's slowest run minus the parent's own max - min spread")
    res["new_median_not_below_bound"] = res["new_median"] >= res["bound"]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if res["new_median_not_below_bound"] else 1


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
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("parity-run")
    p.add_argument("--tree", required=True)
    p.add_argument("--out", required=True)
    p = sub.add_parser("parity-compare")
    p.add_argument("parent")
    p.add_argument("new")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_discrete_continuous_parity.json"))
    p = sub.add_parser("bench-ab")
    p.add_argument("--parent", required=True)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_discrete_bench_ab.json"))
    p = sub.add_parser("learning")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_discrete_learning.json"))
    a = ap.parse_args()
    if a.cmd == "parity-run":
        return parity_run(a.tree, a.out)
    if a.cmd == "parity-compare":
        return parity_compare(a.parent, a.new, a.out)
    if a.cmd == "bench-ab":
        return bench_ab(a.parent, a.out, a.steps, a.warmup)
    return learning(a.out)


if __name__ == "__main__":
    sys.exit(main())
