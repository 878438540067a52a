"""Probe: V-PPO's Trainer.train() on libsrlx's fused update ("srlx") next to the plain torch backend ("torch"), the measurement that decides
ppo_v.Trainer.update_backend's default.

    python tools/vppo_probe.py --out profiles/vppo_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o vppo --output-format csv -- python tools/vppo_probe.py --trace-loop     # a run of its own, no counters

Both arms run in ONE process.  Per shape: one untimed train() of each arm (allocation, the handle, torch's lazy initialisation), then three interleaved rounds
(srlx, torch, srlx, torch, ...) of CALLS whole train() calls each -- host batch assembly from a memory that hands out one fixed batch, the update, and the
`info` read that synchronises -- every round ending in a device synchronise.  The figure is milliseconds per train().
  default  ppo_v.Config() on CartPole: B 64, D 4, A 2, hidden 64-64, value 64, policy ()
  corner   the largest corner of the envelope: B 256, D 256, A 16, hidden 512-512-512, value 512-512, policy 512-512
The default rule: "srlx" iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean of the same run.
--trace-loop runs, at the default shape, one train() of each arm and then TRACE_CALLS of "srlx" followed by TRACE_CALLS of "torch": a kernel trace of it gives
the launches per train() of each arm (the libsrlx kernels are named k_vppo_*; everything else is torch's)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, TRACE_CALLS = 200, 100
# B, D, A, hidden, value, policy
SHAPES = dict(default=(64, 4, 2, (64, 64), (64,), ()), corner=(256, 256, 16, (512, 512, 512), (512, 512), (512, 512)))


class _FixedMemory:
    """Hands out one fixed batch of items [state, next_state, one-hot action, log_prob, reward, not_done, total_reward]."""

    def __init__(self, B, D, A, seed):
        import numpy as np

        rng = np.random.default_rng(seed)
        eye = np.identity(A, dtype=np.float32)
        self.items = [[rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32), eye[rng.integers(A)],
                       np.array([np.log(1.0 / A) + 0.05 * rng.standard_normal()], np.float32), float(rng.standard_normal()), int(rng.random() < 0.8),
                       float(rng.standard_normal())] for _ in range(B)]

    def sample(self):
        return self.items


def _trainer(shape, backend):
    import torch

    import vppo_cases as C
    from simple_distributed_rl_amd.algorithms import ppo_v

    B, D, A, hidden, value, policy = SHAPES[shape]
    cfg = C.make_config(D, 0, A, hidden, value, policy, device="cuda", batch_size=B)
    torch.manual_seed(1)
    tr = ppo_v.Trainer(cfg, ppo_v.Parameter(cfg), _FixedMemory(B, D, A, 2))
    tr.update_backend = backend
    tr.on_setup()
    return tr


def _loop(tr, calls):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        tr.train()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def measure(shape):
    arms = {a: _trainer(shape, a) for a in ("srlx", "torch")}
    for a, tr in arms.items():
        tr.train()
        assert tr.update_path == a, (a, tr.update_path, tr.why_not_srlx_update)
    runs = {a: [] for a in arms}
    for _ in range(3):
        for a, tr in arms.items():
            runs[a].append(_loop(tr, CALLS))
    B, D, A, hidden, value, policy = SHAPES[shape]
    res = dict(what=f"one whole Trainer.train() (host batch assembly and the info read included), ms, mean of {CALLS} calls per round",
               shape=dict(batch=B, obs_dim=D, actions=A, hidden_block=list(hidden), value_block=list(value), policy_block=list(policy)))
    res.update({a + "_ms": r for a, r in runs.items()})
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    res["srlx_over_torch"] = res["srlx_ms_mean"] / res["torch_ms_mean"]
    res["updates_per_s"] = {a: 1e3 / res[a + "_ms_mean"] for a in arms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vppo_probe.json"))
    ap.add_argument("--trace-loop", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        for a in ("srlx", "torch"):
            tr = _trainer("default", a)
            tr.train()
            _loop(tr, TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} train() calls per arm at the default shape")
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__)
    for shape in SHAPES:
        out[shape] = measure(shape)
        print(shape, {k: out[shape][k] for k in ("srlx_ms_mean", "torch_ms_mean", "srlx_over_torch")}, flush=True)
    out["default_rule"] = dict(rule="update_backend = 'srlx' iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean",
                               srlx=bool(out["default"]["srlx_ms_mean"] <= 1.10 * out["default"]["torch_ms_mean"]))
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
