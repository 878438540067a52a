"""Probe: V-PPO's Trainer.train() on libsrlx's fused update ("srlx"), on its layer-wise update on the float64 matrix cores ("srlx_gemm") and on the
plain torch backend ("torch"): the measurement that decides ppo_v.Trainer.update_backend's default and says on which side of the row path a shape
falls.

    python tools/vppo_probe.py --out profiles/vppo_gemm_probe.json
    python tools/vppo_probe.py --wide --out profiles/vppo_wide_probe.json      # batches above 256 on the gemm-only handle
    rocprofv3 --kernel-trace --stats -d DIR -o vppo --output-format csv -- python tools/vppo_probe.py --trace-loop [--shape corner]   # a run of its own, no counters

All arms run in ONE process.  Per shape: one untimed train() of each arm (allocation, the handle, torch's lazy initialisation), then three interleaved rounds
(srlx, srlx_gemm, torch, srlx, ...) of CALLS whole train() calls each -- host batch assembly from a memory that hands out one fixed batch, the update, and the
`info` read that synchronises -- every round ending in a device synchronise.  The figure is milliseconds per train().
  default  ppo_v.Config() on CartPole: B 64, D 4, A 2, hidden 64-64, value 64, policy ()
  b64-w256   B 64, D 4, A 2, every block 256 wide at the default's depths
  b256-w128  B 256, D 4, A 2, every block 128 wide at the default's depths
  corner   the largest corner of the envelope: B 256, D 256, A 16, hidden 512-512-512, value 512-512, policy 512-512
The default rule: "srlx" iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean of the same run.
--trace-loop runs, at --shape, one train() of each arm and then TRACE_CALLS of each arm in turn: a kernel trace of it gives the launches and the kernel time
per train() of each arm (the libsrlx kernels are named k_vppo_* and k_mlp_gemm_*; everything else is torch's).
--wide measures "srlx_gemm" against "torch" the same way (WIDE_CALLS calls per round) at B 512, 1024 and 4096 on ppo_v.Config()'s blocks and on 512-wide blocks,
where "srlx_gemm" is a gemm-only handle whose gradient launch is k_mlp_gemm_wgrad; and, at the corner (B 256), an ordinary handle on the gemm path
("srlx_gemm", gradient launch k_vppo_grad) against a gemm-only one ("srlx_gemm_only").  --trace-loop --shape corner-wgrad traces those two arms.

The acting arm (tools/act_probe.py), the measurement that decides ppo_v.Parameter.act_backend's default:

    python tools/vppo_probe.py --act --out profiles/vppo_act_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o vppo_act --output-format csv -- python tools/vppo_probe.py --act --trace-loop   # a run of its own

Whole Worker._dist calls for one state at ppo_v.Config()'s network on CartPole-v1 (default) and at the envelope's corner (512-wide blocks at full depth)."""
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
SHAPES = {"default": (64, 4, 2, (64, 64), (64,), ()), "b64-w256": (64, 4, 2, (256, 256), (256,), ()), "b256-w128": (256, 4, 2, (128, 128), (128,), ()),
          "corner": (256, 256, 16, (512, 512, 512), (512, 512), (512, 512))}
ARMS = ("srlx", "srlx_gemm", "torch")
WIDE_CALLS = 100
WIDE_SHAPES = {f"b{B}{tag}": (B, 4, 2, hidden, value, ()) for tag, hidden, value in (("", (64, 64), (64,)), ("-w512", (512, 512), (512,))) for B in (512, 1024, 4096)}
SHAPES.update(WIDE_SHAPES, **{"corner-wgrad": SHAPES["corner"]})
WIDE_ARMS = {name: ("srlx_gemm", "torch") for name in WIDE_SHAPES}
WIDE_ARMS["corner-wgrad"] = ("srlx_gemm", "srlx_gemm_only")


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
    tr.update_backend = "srlx_gemm" if backend == "srlx_gemm_only" else backend
    tr.on_setup()
    if backend == "srlx_gemm_only":  # (at B <= 256 the Trainer builds an ordinary handle: the probe puts a gemm-only one in its place before the first train())
        from simple_distributed_rl_amd.device.vppo import VppoUpdate

        tr._backend, tr._srlx = "srlx_gemm", VppoUpdate(tr.parameter, max_batch=B, gemm_only=True)
    return tr


def _loop(tr, calls):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        tr.train()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def measure(shape, arm_names=ARMS, calls=CALLS):
    arms = {a: _trainer(shape, a) for a in arm_names}
    for a, tr in arms.items():
        tr.train()
        assert tr.update_path == a.replace("_only", ""), (a, tr.update_path, tr.why_not_srlx_update)
    runs = {a: [] for a in arms}
    for _ in range(3):
        for a, tr in arms.items():
            runs[a].append(_loop(tr, calls))
    B, D, A, hidden, value, policy = SHAPES[shape]
    res = dict(what=f"one whole Trainer.train() (host batch assembly and the info read included), ms, mean of {calls} calls per round",
               shape=dict(batch=B, obs_dim=D, actions=A, hidden_block=list(hidden), value_block=list(value), policy_block=list(policy)))
    res.update({a + "_ms": r for a, r in runs.items()})
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    if arm_names is not ARMS:
        first, second = arm_names
        res[f"{first}_over_{second}_by_round"] = [x / y for x, y in zip(runs[first], runs[second])]
        return res
    res["srlx_over_torch"] = res["srlx_ms_mean"] / res["torch_ms_mean"]
    res["gemm_over_srlx_by_round"] = [g / r for g, r in zip(runs["srlx_gemm"], runs["srlx"])]
    res["gemm_over_torch_by_round"] = [g / t for g, t in zip(runs["srlx_gemm"], runs["torch"])]
    res["gemm_side_of_row_path"] = "faster" if all(x < 1 for x in res["gemm_over_srlx_by_round"]) else (
        "slower" if all(x > 1 for x in res["gemm_over_srlx_by_round"]) else "within the rounds' spread")
    res["updates_per_s"] = {a: 1e3 / res[a + "_ms_mean"] for a in arms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/vppo_probe.json, with --act profiles/vppo_act_probe.json")
    ap.add_argument("--act", action="store_true", help="the acting arm (DESIGN.md 7za): whole Worker._dist calls for one state, which decide Parameter.act_backend")
    ap.add_argument("--trace-loop", action="store_true")
    ap.add_argument("--wide", action="store_true", help="the shapes of WIDE_ARMS instead of the four of the docstring")
    ap.add_argument("--shape", default="default", choices=list(SHAPES), help="the shape of --trace-loop")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.act:
        import act_probe
        import vppo_cases as C
        from simple_distributed_rl_amd.algorithms import ppo_v

        shapes = {name: ((lambda s=SHAPES[name]: C.make_config(s[1], 0, s[2], *s[3:], device="cuda")), dict(zip(("obs_dim", "actions", "hidden", "value", "policy"), SHAPES[name][1:])))
                  for name in ("default", "corner")}
        return act_probe.run(args, ppo_v, shapes, "default", os.path.join(ROOT, "profiles", "vppo_act_probe.json"))
    args.out = args.out or os.path.join(ROOT, "profiles", "vppo_probe.json")
    if args.trace_loop:
        for a in WIDE_ARMS.get(args.shape, ARMS):
            tr = _trainer(args.shape, a)
            tr.train()
            _loop(tr, TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} train() calls per arm at the {args.shape} shape")
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__)
    for shape in (WIDE_ARMS if args.wide else ()):
        out[shape] = measure(shape, WIDE_ARMS[shape], WIDE_CALLS)
        print(shape, {k: v for k, v in out[shape].items() if k.endswith(("_ms", "_by_round"))}, flush=True)
    for shape in (() if args.wide else [s for s in SHAPES if s not in WIDE_ARMS]):
        out[shape] = measure(shape)
        print(shape, {k: out[shape][k] for k in ("srlx_ms", "srlx_gemm_ms", "torch_ms", "gemm_side_of_row_path")}, flush=True)
    if not args.wide:
        out["default_rule"] = dict(rule="update_backend = 'srlx' iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean",
                                   srlx=bool(out["default"]["srlx_ms_mean"] <= 1.10 * out["default"]["torch_ms_mean"]))
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
