"""The acting arm of tools/vppo_probe.py and tools/notsac_probe.py (`--act`): the measurement that decides `Parameter.act_backend`'s default for
ppo_v and sac_not.

Whole `Worker._dist` calls for ONE environment state -- the host-to-device copy of the state, the policy's forward and the read of the distribution's loc or
logits back to the host, which makes every call synchronous as Worker.policy's own reads do -- "srlx" (one k_mlp_walk launch) against "torch" (the module's
forward) on equal weights in ONE process: one untimed call of each arm, then three interleaved rounds (srlx, torch, srlx, ...) of ACT_CALLS calls each, every
round ending in a device synchronise.  The figure is milliseconds per call.  The rule: "srlx" iff EVERY round's srlx time at the plugin's default shape is at
most 1.10 times the same round's torch time.  With --trace-loop: 1 + TRACE_CALLS calls on "srlx" at each shape, for a kernel trace in a run of its own."""
import json
import os
import time
import types

ACT_CALLS, TRACE_CALLS = 2000, 100
ARMS = ("srlx", "torch")


def _loop(worker, env, calls):
    import torch

    from simple_distributed_rl_amd.algorithms.ppo_v import CategoricalDist, NormalDist

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        d = worker._dist(env)
        (d.mean() if isinstance(d, NormalDist) else d.logits() if isinstance(d, CategoricalDist) else d.logits).cpu()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def _arm(module, config, backend):
    """A Worker of `module` over a seeded GPU Parameter on one acting backend; both arms hold equal weights."""
    import torch

    torch.manual_seed(1)
    p = module.Parameter(config)
    p.act_backend = backend
    w = module.Worker(config, p)
    w.on_setup(None, None)
    return w


def run(args, module, shapes, default_shape, default_out):
    """`shapes`: {name: (a function giving a fresh set-up GPU config, a dict describing the shape)}."""
    import numpy as np
    import torch

    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__,
               what=f"one whole Worker._dist(worker) for one state and the read of its loc / logits to the host, ms, mean of {ACT_CALLS} calls per round")
    for name, (make_config, described) in shapes.items():
        cfg = make_config()
        D = cfg.observation_space.shape[0]
        env = types.SimpleNamespace(state=np.random.default_rng(3).standard_normal(D).astype(np.float32))
        if args.trace_loop:
            _loop(_arm(module, cfg, "srlx"), env, 1 + TRACE_CALLS)
            continue
        arms = {a: _arm(module, make_config(), a) for a in ARMS}
        for a, w in arms.items():
            _loop(w, env, 1)
            assert w.parameter.act_path == a, (a, w.parameter.act_path, w.parameter.why_not_srlx_act)
        runs = {a: [] for a in arms}
        for _ in range(3):
            for a, w in arms.items():
                runs[a].append(_loop(w, env, ACT_CALLS))
        out[name] = dict(shape=described, **{a + "_ms": r for a, r in runs.items()}, srlx_over_torch_by_round=[s / t for s, t in zip(runs["srlx"], runs["torch"])])
        print(name, out[name], flush=True)
    if args.trace_loop:
        print(f"trace loop: 1 + {TRACE_CALLS} _dist calls on 'srlx' at each of {list(shapes)}")
        return
    out["default_rule"] = dict(rule=f"act_backend = 'srlx' iff every round's srlx_ms <= 1.10 * torch_ms at the {default_shape} shape",
                               srlx=bool(all(r <= 1.10 for r in out[default_shape]["srlx_over_torch_by_round"])))
    path = args.out or default_out
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
