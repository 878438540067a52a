"""Probe: discrete SAC's Trainer.train() on libsrlx's fused update ("srlx"), on its layer-wise path on the float64 matrix cores ("srlx_gemm")
and on the plain torch backend ("torch"), the measurement that decides sac.Trainer.update_backend's default.

    python tools/sacd_probe.py --out profiles/sacd_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o sacd --output-format csv -- python tools/sacd_probe.py --trace-loop [--shape corner] [--arms srlx_gemm]

The arms run in ONE process.  Per shape: one untimed train() of each arm (allocation, the handle, torch's lazy initialisation), then three interleaved rounds
(srlx, srlx_gemm, torch, srlx, ...) of CALLS whole train() calls each -- host batch assembly from a memory that hands out one fixed batch, the update, and the
`info` read that synchronises -- every round ending in a device synchronise.  The figure is milliseconds per train().
  default  sac.Config() on CartPole: B 32, D 4, A 2, policy 64-64-64, q 128-128-128
  wide     B 256, D 64, A 16, the same blocks
  corner   B 256, D 256, A 16, policy 512-512-512, q 512-512-512: the envelope's largest
The default rule: "srlx" iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean of the same run.
--trace-loop runs, at --shape, one train() and then TRACE_CALLS more of each arm of --arms in turn: a kernel trace of it gives the launches per train() of each
arm (the libsrlx kernels are named k_sacd_*; everything else is torch's)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, TRACE_CALLS = 200, 100
ARMS = ("srlx", "srlx_gemm", "torch")
SHAPES = dict(default=(32, 4, 2, (64, 64, 64), (128, 128, 128)), wide=(256, 64, 16, (64, 64, 64), (128, 128, 128)),
              corner=(256, 256, 16, (512, 512, 512), (512, 512, 512)))


class _FixedMemory:
    """Hands out one fixed batch of items [state, one-hot action, next_state, reward, terminated]."""

    def __init__(self, B, D, A, seed):
        import numpy as np

        rng = np.random.default_rng(seed)
        eye = np.identity(A, dtype=np.float32)
        self.items = [[rng.standard_normal(D).astype(np.float32), eye[rng.integers(A)], rng.standard_normal(D).astype(np.float32), float(rng.standard_normal()),
                       bool(rng.random() < 0.2)] for _ in range(B)]

    def sample(self):
        return self.items


def _trainer(shape, backend):
    import sacd_cases as C
    from simple_distributed_rl_amd.algorithms import sac

    B, D, A, pw, qw = SHAPES[shape]
    cfg = C.make_config(D, A, pw, qw, device="cuda", batch_size=B)
    tr = sac.Trainer(cfg, C.make_parameter(cfg, 1), _FixedMemory(B, D, A, 2))
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
    B, D, A, pw, qw = SHAPES[shape]
    res = dict(what=f"one whole Trainer.train() (host batch assembly and the info read included), ms, mean of {CALLS} calls per round",
               shape=dict(batch=B, obs_dim=D, actions=A, policy_block=list(pw), q_block=list(qw)))
    res.update({a + "_ms": r for a, r in runs.items()})
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    res["srlx_over_torch"] = res["srlx_ms_mean"] / res["torch_ms_mean"]
    res["gemm_over_srlx_by_round"] = [g / r for g, r in zip(runs["srlx_gemm"], runs["srlx"])]
    res["gemm_over_torch_by_round"] = [g / r for g, r in zip(runs["srlx_gemm"], runs["torch"])]
    res["gemm_faster_than_srlx_every_round"] = all(x < 1.0 for x in res["gemm_over_srlx_by_round"])
    res["updates_per_s"] = {a: 1e3 / res[a + "_ms_mean"] for a in arms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sacd_probe.json"))
    ap.add_argument("--trace-loop", action="store_true")
    ap.add_argument("--shape", default="default", choices=sorted(SHAPES))
    ap.add_argument("--arms", default=",".join(ARMS))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        for a in args.arms.split(","):
            tr = _trainer(args.shape, a)
            tr.train()
            assert tr.update_path == a, (a, tr.update_path, tr.why_not_srlx_update)
            _loop(tr, TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} train() calls per arm ({args.arms}) at the {args.shape} shape")
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__)
    for shape in SHAPES:
        out[shape] = measure(shape)
        print(shape, {k: out[shape][k] for k in ("srlx_ms", "srlx_gemm_ms", "torch_ms")}, flush=True)
    out["default_rule"] = dict(rule="update_backend = 'srlx' iff default.srlx_ms_mean <= 1.10 * default.torch_ms_mean",
                               srlx=bool(out["default"]["srlx_ms_mean"] <= 1.10 * out["default"]["torch_ms_mean"]))
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
