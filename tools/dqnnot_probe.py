"""Probe: NoTarget_DQN's Trainer.train() on libsrlx's update ("srlx") and on the plain torch backend ("torch"): the measurement that decides
dqn_not.Trainer.update_backend's default.

    python tools/dqnnot_probe.py --out profiles/dqnnot_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o dqnnot --output-format csv -- python tools/dqnnot_probe.py --trace-loop [--shape b256]   # a run of its own, no counters

Both arms run in ONE process.  Per shape: one untimed train() of each arm (allocation, the handle, torch's lazy initialisation), then three interleaved rounds
(srlx, torch, srlx, ...) of CALLS whole train() calls each -- host batch assembly from a memory that hands out one fixed batch, the update, and the `info` read
that synchronises -- every round ending in a device synchronise.  The figure is milliseconds per train().
  default  dqn_not.Config() on CartPole: B 32, D 4, A 2, U 512
  b256     B 256, D 64, A 16, U 512
  b1024    B 1024, D 4, A 2, U 512
The default rule: "srlx" iff EVERY round's srlx time at the default shape is at most 1.10 times the same round's torch time.
--trace-loop runs, at --shape, one train() of each arm and then TRACE_CALLS of each arm in turn: a kernel trace of it gives the launches and the kernel time per
train() of each arm (the libsrlx kernels are named k_dqnnot_* and k_mlp_gemm_*; everything else is torch's).

The acting arm, the measurement that decides dqn_not.Parameter.act_backend's default:

    python tools/dqnnot_probe.py --act --out profiles/dqnnot_act_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o dqnnot_act --output-format csv -- python tools/dqnnot_probe.py --act --trace-loop   # a run of its own

Whole `Parameter.pred_q` calls on dqn_not.Config()'s network on CartPole-v1 (D 4, A 2, U 512) at n = 1 (what Worker.policy asks) and n = 1024, "srlx" against
"torch" on equal weights: one untimed call of each arm, then three interleaved rounds of ACT_CALLS calls each.  The rule is the same, at n = 1."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, TRACE_CALLS = 200, 100
ACT_CALLS, ACT_ROWS = 2000, (1, 1024)
SHAPES = {"default": (32, 4, 2, 512), "b256": (256, 64, 16, 512), "b1024": (1024, 4, 2, 512)}  # B, D, A, U
ARMS = ("srlx", "torch")


class _FixedMemory:
    """Hands out one fixed batch of items [state, next_state, action, reward, not_done, total_reward] with unit weights."""

    def __init__(self, B, D, A, seed):
        import numpy as np

        rng = np.random.default_rng(seed)
        self.items = [[rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32), int(rng.integers(A)), float(rng.standard_normal()),
                       int(rng.random() < 0.8), float(rng.standard_normal())] for _ in range(B)]
        self.weights = np.ones(B, np.float32)

    def sample(self):
        return self.items, self.weights, None


def _trainer(shape, backend):
    import torch

    import dqnnot_reference as R
    from simple_distributed_rl_amd.algorithms import dqn_not

    B, D, A, U = SHAPES[shape]
    cfg = R.make_config(D, U, A, device="cuda", batch_size=B)
    torch.manual_seed(1)
    tr = dqn_not.Trainer(cfg, dqn_not.Parameter(cfg), _FixedMemory(B, D, A, 2))
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
    arms = {a: _trainer(shape, a) for a in ARMS}
    for a, tr in arms.items():
        tr.train()
        assert tr.update_path == a, (a, tr.update_path, tr.why_not_srlx_update)
    runs = {a: [] for a in arms}
    for _ in range(3):
        for a, tr in arms.items():
            runs[a].append(_loop(tr, CALLS))
    B, D, A, U = SHAPES[shape]
    res = dict(what=f"one whole Trainer.train() (host batch assembly and the info read included), ms, mean of {CALLS} calls per round",
               shape=dict(batch=B, obs_dim=D, actions=A, base_units=U))
    res.update({a + "_ms": r for a, r in runs.items()})
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    res["srlx_over_torch_by_round"] = [s / t for s, t in zip(runs["srlx"], runs["torch"])]
    return res


def _actor(backend):
    """A GPU dqn_not.Parameter of dqn_not.Config() on CartPole-v1 (D 4, A 2, U 512) on one acting backend; both arms hold equal weights."""
    import torch

    import dqnnot_reference as R
    from simple_distributed_rl_amd.algorithms import dqn_not

    torch.manual_seed(1)
    p = dqn_not.Parameter(R.make_config(4, 512, 2, device="cuda"))
    p.act_backend = backend
    return p


def _act_loop(p, states, calls):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        p.pred_q(states)  # (ends in two device-to-host copies: every call is synchronous)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def measure_act(n):
    import numpy as np

    states = np.random.default_rng(3).standard_normal((n, 4)).astype(np.float32)
    arms = {a: _actor(a) for a in ARMS}
    for a, p in arms.items():
        p.pred_q(states)
        assert p.act_path == a, (a, p.act_path, p.why_not_srlx_act)
    runs = {a: [] for a in arms}
    for _ in range(3):
        for a, p in arms.items():
            runs[a].append(_act_loop(p, states, ACT_CALLS))
    res = dict(what=f"one whole Parameter.pred_q(states) (host-to-device copy of the states, the forward, q and v back as numpy), ms, mean of {ACT_CALLS} calls per round",
               shape=dict(rows=n, obs_dim=4, actions=2, base_units=512))
    res.update({a + "_ms": r for a, r in runs.items()})
    res["srlx_over_torch_by_round"] = [s / t for s, t in zip(runs["srlx"], runs["torch"])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/dqnnot_probe.json, with --act profiles/dqnnot_act_probe.json")
    ap.add_argument("--act", action="store_true", help="the acting arm (DESIGN.md 7z): whole pred_q calls at n = 1 and n = 1024, which decide Parameter.act_backend")
    ap.add_argument("--trace-loop", action="store_true")
    ap.add_argument("--shape", default="default", choices=list(SHAPES), help="the shape of --trace-loop")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "dqnnot_act_probe.json" if args.act else "dqnnot_probe.json")
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.act and args.trace_loop:  # (a kernel trace of it gives k_dqnnot_act's time at both row counts: the grid is 1, then 64)
        import numpy as np

        p = _actor("srlx")
        for n in ACT_ROWS:
            _act_loop(p, np.zeros((n, 4), np.float32), 1 + TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} pred_q calls on 'srlx' at each of n = {ACT_ROWS}")
        return
    if args.act:
        from simple_distributed_rl_amd import _native as N

        out = dict(device=N.device_info(0), torch=torch.__version__)
        for n in ACT_ROWS:
            out[f"n{n}"] = measure_act(n)
            print(n, {k: out[f"n{n}"][k] for k in ("srlx_ms", "torch_ms", "srlx_over_torch_by_round")}, flush=True)
        out["default_rule"] = dict(rule="act_backend = 'srlx' iff every round's srlx_ms <= 1.10 * torch_ms at n = 1",
                                   srlx=bool(all(r <= 1.10 for r in out["n1"]["srlx_over_torch_by_round"])))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.out)
        return
    if args.trace_loop:
        for a in ARMS:
            tr = _trainer(args.shape, a)
            tr.train()
            _loop(tr, TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} train() calls per arm at the {args.shape} shape")
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__)
    for shape in SHAPES:
        out[shape] = measure(shape)
        print(shape, {k: out[shape][k] for k in ("srlx_ms", "torch_ms", "srlx_over_torch_by_round")}, flush=True)
    out["default_rule"] = dict(rule="update_backend = 'srlx' iff every round's srlx_ms <= 1.10 * torch_ms at the default shape",
                               srlx=bool(all(r <= 1.10 for r in out["default"]["srlx_over_torch_by_round"])))
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
