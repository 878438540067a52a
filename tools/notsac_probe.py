"""Probe: NoT_SAC's Trainer.train() on libsrlx's fused update ("srlx") next to the plain torch backend ("torch"), the measurement that decides
sac_not.Trainer.update_backend's default.

    python tools/notsac_probe.py --out profiles/notsac_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o notsac --output-format csv -- python tools/notsac_probe.py --trace-loop     # a run of its own, no counters

Both arms run in ONE process.  Per shape: one untimed train() of each arm (allocation, the handle, torch's lazy initialisation), then three interleaved rounds
(srlx, torch, srlx, torch, ...) of CALLS whole train() calls each -- host batch assembly from a memory that hands out one fixed batch, the noise draw, the
update, and the `info` read that synchronises -- every round ending in a device synchronise.  The figure is milliseconds per train().
  pendulum  sac_not.Config() on Pendulum-v1: B 64, D 3, Normal K 1, policy 512, q 512, act_emb 64
  cartpole  sac_not.Config() on CartPole-v1: B 64, D 4, Gumbel A 2, policy 512, q 512, act_emb 64
  large     B 256, D 256, Normal K 8, policy 512-512-512, q 512-512-512, act_emb 256: the envelope's largest corner
pendulum_rows16 and large_rows16 repeat two of them with the row kernels at 16 rows per workgroup (srlx_notsac_set_rows_per_workgroup) in place of the default.
The default rule: "srlx" iff pendulum.srlx_ms_mean <= 1.10 * pendulum.torch_ms_mean of the same run.
--trace-loop runs, at the pendulum shape, one train() of each arm and then TRACE_CALLS of "srlx" followed by TRACE_CALLS of "torch": a kernel trace of it
gives the launches per train() of each arm (the libsrlx kernels are named k_notsac_*; everything else is torch's)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, TRACE_CALLS = 200, 100
# B, D, head, n_out, policy, q, act_emb
SHAPES = dict(pendulum=(64, 3, 1, 1, (512,), (512,), 64), cartpole=(64, 4, 0, 2, (512,), (512,), 64),
              large=(256, 256, 1, 8, (512, 512, 512), (512, 512, 512), 256))


class _FixedMemory:
    """Hands out one fixed batch of items [state, next_state, action, reward, not_done, total_reward]."""

    def __init__(self, B, D, head, n_out, seed):
        import numpy as np

        rng = np.random.default_rng(seed)
        eye = np.identity(n_out, dtype=np.float32)
        act = (lambda: np.tanh(rng.standard_normal(n_out)).astype(np.float32)) if head else (lambda: eye[rng.integers(n_out)])
        self.items = [[rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32), act(), float(rng.standard_normal()),
                       int(rng.random() < 0.8), float(rng.standard_normal())] for _ in range(B)]

    def sample(self):
        return self.items


def _trainer(shape, backend, rpw=0):
    import torch

    import notsac_cases as C
    from simple_distributed_rl_amd.algorithms import sac_not

    B, D, head, n_out, policy, q, act_emb = SHAPES[shape]
    cfg = C.make_config(D, head, n_out, policy, q, act_emb, device="cuda", batch_size=B)
    torch.manual_seed(1)
    tr = sac_not.Trainer(cfg, sac_not.Parameter(cfg), _FixedMemory(B, D, head, n_out, 2))
    tr.update_backend = backend
    tr.on_setup()
    if backend == "srlx" and rpw:  # (the launch shape of the row kernels; never a bit: tests/test_notsac_gpu.py)
        assert tr._backend_for(B) == "srlx", tr.why_not_srlx_update
        tr._srlx.set_rows_per_workgroup(rpw)
    return tr


def _loop(tr, calls):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        tr.train()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def measure(shape, rpw=0):
    arms = {a: _trainer(shape, a, rpw) for a in ("srlx", "torch")}
    for a, tr in arms.items():
        tr.train()
        assert tr.update_path == a, (a, tr.update_path, tr.why_not_srlx_update)
    runs = {a: [] for a in arms}
    for _ in range(3):
        for a, tr in arms.items():
            runs[a].append(_loop(tr, CALLS))
    B, D, head, n_out, policy, q, act_emb = SHAPES[shape]
    res = dict(what=f"one whole Trainer.train() (host batch assembly, the noise draw and the info read included), ms, mean of {CALLS} calls per round",
               rows_per_workgroup=rpw or "default (one row per workgroup at B <= 256)", shape=dict(batch=B, obs_dim=D, head="Normal" if head else "Gumbel", n_out=n_out, policy_block=list(policy), q_block=list(q), act_emb_units=act_emb))
    res.update({a + "_ms": r for a, r in runs.items()})
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    res["srlx_over_torch"] = res["srlx_ms_mean"] / res["torch_ms_mean"]
    res["updates_per_s"] = {a: 1e3 / res[a + "_ms_mean"] for a in arms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notsac_probe.json"))
    ap.add_argument("--trace-loop", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        for a in ("srlx", "torch"):
            tr = _trainer("pendulum", a)
            tr.train()
            _loop(tr, TRACE_CALLS)
        print(f"trace loop: 1 + {TRACE_CALLS} train() calls per arm at the pendulum shape")
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__)
    for shape in SHAPES:
        out[shape] = measure(shape)
        print(shape, {k: out[shape][k] for k in ("srlx_ms_mean", "torch_ms_mean", "srlx_over_torch")}, flush=True)
    for shape in ("pendulum", "large"):  # the same arms with the row kernels at 16 rows per workgroup (B / 16 workgroups): what the default launch shape buys
        key = shape + "_rows16"
        out[key] = measure(shape, 16)
        print(key, {k: out[key][k] for k in ("srlx_ms_mean", "torch_ms_mean", "srlx_over_torch")}, flush=True)
    out["default_rule"] = dict(rule="update_backend = 'srlx' iff pendulum.srlx_ms_mean <= 1.10 * pendulum.torch_ms_mean",
                               srlx=bool(out["pendulum"]["srlx_ms_mean"] <= 1.10 * out["pendulum"]["torch_ms_mean"]))
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
