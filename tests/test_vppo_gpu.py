"""V-PPO on the GPU: libsrlx's fused update (srlx_vppo_update, csrc/srlx_vppo.hip) and forward-only pass over the cases of tests/vppo_cases.py against the
float64 yardstick of tests/vppo_reference.py (which tests/test_vppo_pinned_cpu.py holds to the reference's own code), the plugin's Trainer on both backends,
and Runners on CartPole and Pendulum.  Bars (BASELINE's 1e-5): rtol 1e-5 / atol 1e-6 on v, n_v, new_logpi, the four losses, the norm and the
parameters after two updates; 1e-5 |g| + 1e-5 max |g| per tensor on every gradient before and after the clip; the parameters after two updates equal to
torch.optim.Adam (float32) on the kernel's own clipped gradients at rtol 1e-6.  No case and no element is left out of any comparison.
Every test prints what it measured as a fraction of its bar ("VPPO-ERR ...", shown with -s) before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo_v

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_cases as C  # noqa: E402
import vppo_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCALARS = ("loss_value", "loss_v_align", "loss_policy", "loss_e", "norm")


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu().reshape(-1)


def _frac(name, got, want):
    """max |got - want| as a fraction of the quantity's bar: rtol 1e-5 and, for a gradient tensor (g.* / raw.*) atol 1e-5 max |want|, for everything else atol
    1e-6.  <= 1 is np.testing.assert_allclose at that bar."""
    atol = 1e-5 * float(want.abs().max()) if name.startswith(("g.", "raw.")) else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _report(tag, got, want):
    """Prints every group's worst fraction of its bar, returns the quantities over their bar."""
    assert set(got) == set(want)
    fr = {name: _frac(name, got[name], want[name]) for name in got}
    groups = {}
    for name, v in fr.items():
        key = name.split("@")[0].split(".")[0] + ("@" + name.split("@")[1] if "@" in name else "")
        groups[key] = max(groups.get(key, 0.0), v)
    print(f"VPPO-ERR {tag} " + " ".join(f"{k}={v:.3f}" for k, v in groups.items()))
    return {k: v for k, v in fr.items() if not v <= 1.0}


def _quantities(k, out, raw, grads):
    """One update as {name@k: float64 CPU vector}.  `out`: the yardstick's dict, or the kernel's with its five scalars in out["scalars"]."""
    q = {f"{key}@{k}": _f64(out[key]) for key in ("v", "n_v", "new_logpi")}
    for j, key in enumerate(SCALARS):
        q[f"{key}@{k}"] = _f64(out["scalars"][j] if "scalars" in out else out[key])
    if raw is not None:
        q.update({f"raw.{j}@{k}": _f64(g) for j, g in enumerate(raw)})
    q.update({f"g.{j}@{k}": _f64(g) for j, g in enumerate(grads)})
    return q


def _dev(name, b):
    head = C.CASES[name][2]
    f = lambda x: x.float().cuda()  # noqa: E731
    return dict(state=f(b["state"]), n_state=f(b["n_state"]), action=f(b["action"]) if head else b["action"].int().cuda(), old_logpi=f(b["old_logpi"]),
                reward=f(b["reward"]), not_terminated=f(b["not_terminated"]), total_reward=f(b["total_reward"]))


def _update(u, cfg, d):
    out = u.update(d["state"], d["n_state"], d["action"], d["old_logpi"], d["reward"], d["not_terminated"], d["total_reward"], cfg.lr, cfg.discount,
                   cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy)
    torch.cuda.synchronize()
    return out


def _two_updates(name):
    """Two libsrlx updates on a fresh GPU parameter of the case; yields everything the tests look at."""
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    p = C.make_parameter(name, "cuda")
    cfg = p.config
    u = VppoUpdate(p, max_batch=C.CASES[name][0])
    # torch.optim.Adam (float32, on the GPU) on the kernel's own clipped gradients
    shadow = [t.detach().clone().requires_grad_(True) for t in p.net.parameters()]
    opt = torch.optim.Adam(shadow, lr=cfg.lr)
    steps = []
    for b in C.make_batches(name):
        out = _update(u, cfg, _dev(name, b))
        raw, grads = [g.clone() for g in u.raw_grads], [g.clone() for g in u.grads]
        for s, g in zip(shadow, grads):
            s.grad = g.clone()
        opt.step()
        steps.append(dict(out=out, raw=raw, grads=grads, after=[t.detach().clone() for t in p.net.parameters()]))
    return p, u, shadow, steps


@functools.lru_cache(maxsize=None)
def _measure(name):
    """Two libsrlx updates of the case measured against the yardstick, once per case (the tests below share it)."""
    refs = C.reference(name)
    p, u, shadow, steps = _two_updates(name)
    got, want = {}, {}
    for k, (st, ref) in enumerate(zip(steps, refs)):
        got.update(_quantities(k, st["out"], st["raw"], st["grads"]))
        want.update(_quantities(k, ref, ref["raw_grads"], ref["grads"]))
    got.update({f"p.{j}": _f64(t) for j, t in enumerate(steps[-1]["after"])})
    want.update({f"p.{j}": _f64(t) for j, t in enumerate(refs[-1]["params"])})
    bad = _report(name, got, want)
    adam = max(float(((_f64(a) - _f64(s)).abs() / (1e-6 * _f64(s).abs() + 1e-300)).max()) for a, s in zip(steps[-1]["after"], shadow))
    print(f"VPPO-ERR {name} params_vs_torch_adam={adam:.3f} steps={u.steps()} norm={[float(st['out']['scalars'][4]) for st in steps]}")
    return dict(bad=bad, adam=adam, steps=u.steps(), outs=[st["out"] for st in steps])


@pytest.mark.parametrize("name", C.NAMES)
def test_update_matches_float64_yardstick(name):
    """Two updates from fixed seeds: v, n_v, new_logpi, the four losses, the norm, every gradient tensor before and after the clip of both updates, and every
    parameter after the two updates, at the bars of the module docstring."""
    m = _measure(name)
    assert m["steps"] == 2
    assert not m["bad"], f"{name}: over the bar (fraction of it): {m['bad']}"
    if C.CASES[name][8] == 0.0:
        assert all(float(o["scalars"][3]) == 0.0 for o in m["outs"])  # loss_e is 0 unless entropy_weight > 0


@pytest.mark.parametrize("name", C.NAMES)
def test_adam_step_equals_torch_adam_on_the_kernels_own_gradients(name):
    assert _measure(name)["adam"] <= 1.0


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_only_call(name):
    """v bit for bit what the update writes for the same rows (v of the states, n_v of the next states), the head's outputs giving the update's new_logpi, and
    all of it within the bars of the float64 module; for 1, 15, 16 and 17 rows beside the case's B, with nothing written behind the last row."""
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    B, D, head, n_out = C.CASES[name][:4]
    p = C.make_parameter(name, "cuda")
    cfg = p.config
    y = C._yardstick(name, C.make_parameter(name))
    u = VppoUpdate(p, max_batch=B)
    d = _dev(name, C.make_batches(name)[0])
    v, heads = u.forward(d["state"])
    n_v, _ = u.forward(d["n_state"], want_head=False)
    torch.cuda.synchronize()
    worst = 0.0
    g = torch.Generator().manual_seed(NAMES_SEED + C.NAMES.index(name))
    lib = N.lib()
    for n in sorted({1, 15, 16, 17, B}):
        x = torch.randn(n, D, generator=g)
        with torch.no_grad():
            want_v, want_h = R.forward(y.net, x.double())
        xd = x.cuda()
        vv = torch.full((n + 1,), 7.0, device="cuda")
        h0, h1 = torch.full((n + 1, n_out), 7.0, device="cuda"), torch.full((n + 1, n_out), 7.0, device="cuda")
        N.check(lib.srlx_vppo_forward(u._h, n, N.tptr(xd), u.ls_lo, u.ls_hi, N.tptr(vv), N.tptr(h0), N.tptr(h1) if head else None, None))
        torch.cuda.synchronize()
        assert float(vv[n]) == 7.0 and bool((h0[n] == 7.0).all()) and bool((h1[n] == 7.0).all())
        worst = max(worst, _frac("v", _f64(vv[:n]), _f64(want_v)))
        if head:
            worst = max(worst, _frac("loc", _f64(h0[:n]), _f64(want_h[:, 0])), _frac("ls", _f64(h1[:n]), _f64(want_h[:, 1].clamp(u.ls_lo, u.ls_hi))))
        else:
            worst = max(worst, _frac("logits", _f64(h0[:n]), _f64(want_h)))
    out = _update(u, cfg, d)  # (last: it moves the parameters)
    assert torch.equal(v, out["v"]) and torch.equal(n_v, out["n_v"])
    with torch.no_grad():  # the update's new_logpi from the forward call's head outputs
        if head:
            dist = ppo_v.NormalDist(heads[0], heads[1])
            lp = dist.log_prob_sgp(d["action"]) if cfg.squashed_gaussian_policy else dist.log_prob(d["action"])
        else:
            lp = ppo_v.CategoricalDist(heads).log_prob(torch.nn.functional.one_hot(d["action"].long(), n_out).float())
    worst = max(worst, _frac("new_logpi", _f64(lp), _f64(out["new_logpi"])))
    print(f"VPPO-ERR forward {name} worst={worst:.3f}")
    assert worst <= 1.0


NAMES_SEED = 31


def test_two_fresh_handles_give_equal_bits():
    for name in ("wide-b33", "normal-k8"):
        a, b = _two_updates(name), _two_updates(name)
        for sa, sb in zip(a[3], b[3]):
            assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
            assert all(torch.equal(x, y) for key in ("raw", "grads", "after") for x, y in zip(sa[key], sb[key]))


def test_update_refuses_a_batch_above_max_batch_and_writes_nothing():
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    name = "mixed-b17"
    B = C.CASES[name][0]
    p = C.make_parameter(name, "cuda")
    u = VppoUpdate(p, max_batch=B - 1)
    before = [t.detach().clone() for t in p.net.parameters()]
    d = _dev(name, C.make_batches(name)[0])
    with pytest.raises(ValueError, match="above max_batch"):
        _update(u, p.config, d)
    out = torch.full((B,), 7.0, device="cuda")
    st = N.lib().srlx_vppo_update(u._h, B, N.tptr(d["state"]), N.tptr(d["n_state"]), N.tptr(d["action"]), N.tptr(d["old_logpi"]), N.tptr(d["reward"]),
                                  N.tptr(d["not_terminated"]), N.tptr(d["total_reward"]), C.LR, C.DISCOUNT, C.CLIP, 0.0, C.ALIGN, 10.0, 0, u.ls_lo, u.ls_hi,
                                  N.tptr(out), N.tptr(out), N.tptr(out), N.tptr(out), None)
    torch.cuda.synchronize()
    assert st == N.ERR_INVALID and b"vppo_update: batch" in N.lib().srlx_last_error()
    assert bool((out == 7.0).all()) and u.steps() == 0
    assert all(torch.equal(x, y) for x, y in zip(before, p.net.parameters()))
    assert all(not bool(g.any()) for g in u.grads + u.raw_grads)


# ---- Trainer and plugin -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _env_batch(env, B):
    """One sampled batch of a run the Worker produced on the CPU, as float64 tensors in the Trainer's layout."""
    import random

    random.seed(3), np.random.seed(3), torch.manual_seed(3)
    cfg = ppo_v.Config(batch_size=B, entropy_weight=0.1)
    cfg.memory.warmup_size = B
    runner = srl.Runner(env, cfg)
    runner.set_device("cpu")
    dist = runner.make_parameter().net.policy_dist_block
    if hasattr(dist, "loc_layers"):
        # A fresh network's scales reach 10 and its actions |a| = 11, where float32 has tanh(a) = 1 and the "torch" backend's correction is log(1e-10) against an
        # exact log(1 - tanh(a)^2) of -20: float32 evaluates 1 - tanh(a)^2 to about 1.2e-7 absolute.  The rollout's policy is therefore tamed (scale near 0.5,
        # |loc| small) and the test requires |a| <= 3: 1 - tanh^2 >= 1e-2, an error of 1.2e-5 in a log-probability whose bar is 1e-6 + 1e-5 |lp|, |lp| > 1.
        with torch.no_grad():
            dist.loc_layers[0].weight.mul_(2.0 ** -3)
            dist.log_scale_layers[0].weight.mul_(2.0 ** -6)
            dist.log_scale_layers[0].bias.fill_(float(np.log(0.5)))
    runner.rollout(max_memory=4 * B)
    cols = list(zip(*runner.memory.sample()))
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float64).reshape(B, -1))  # noqa: E731
    return dict(state=t(cols[0]), n_state=t(cols[1]), action=t(cols[2]), old_logpi=t(cols[3]), reward=t(cols[4]), not_terminated=t(cols[5]), total_reward=t(cols[6]))


ENVS = {"CartPole-v1": (4, 0, 2), "Pendulum-v1": (3, 1, 1)}


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("backend", ["srlx", "torch"])
def test_trainer_backends_follow_the_yardstick_on_an_environment_batch(backend, env):
    B = 8
    D, head, n_out = ENVS[env]
    b = _env_batch(env, B)
    cfg = C.make_config(D, head, n_out, (64, 64), (64,), (), device="cuda", batch_size=B, entropy_weight=0.1)
    torch.manual_seed(77)
    p = ppo_v.Parameter(cfg)
    y = R.Yardstick(p, cfg.lr, cfg.discount, cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy, C.ls_range(cfg))
    ref = y.update(b["state"], b["n_state"], b["action"] if head else b["action"].argmax(1), b["old_logpi"], b["reward"][:, 0], b["not_terminated"][:, 0],
                   b["total_reward"][:, 0])
    print(f"VPPO-ERR trainer-{backend}-{env} margin={ref['margin']:.2e} max|a|={float(b['action'].abs().max()):.2f}")
    assert not head or float(b["action"].abs().max()) <= 3.0  # (float32 resolves 1 - tanh(a)^2: see _env_batch)
    assert ref["margin"] >= 1e-3  # (the sampled batch is nowhere near a kink)
    tr = ppo_v.Trainer(cfg, p, None)
    tr.update_backend = backend
    tr.on_setup()
    args = [b[k].float().cuda() for k in ("state", "n_state", "action", "old_logpi", "reward", "not_terminated", "total_reward")]
    out = tr.train_on_batch(*args)
    torch.cuda.synchronize()
    assert tr.update_path == backend and tr.why_not_srlx_update == "" and tr.train_count == 1
    grads = tr._srlx.grads if backend == "srlx" else [t.grad for t in p.net.parameters()]
    bad = _report(f"trainer-{backend}-{env}", _quantities(0, out, None, grads), _quantities(0, ref, None, ref["grads"]))
    assert set(tr.info) == {"loss_value", "loss_v_align", "loss_policy", "loss_e"} and all(np.isfinite(v) for v in tr.info.values())
    assert tr.info["loss_value"] == pytest.approx(ref["loss_value"], rel=1e-5, abs=1e-6)
    assert not bad, bad
    tr.update_backend = "torch" if backend == "srlx" else "srlx"  # fixed for the Trainer's life at the first train()
    tr.train_on_batch(*args)
    assert tr.update_path == backend


def test_trainer_with_an_input_block_layer_outside_the_envelope_runs_torch_and_says_why():
    B = 8
    b = _env_batch("CartPole-v1", B)
    cfg = C.make_config(4, 0, 2, (64,), (64,), (), device="cuda", batch_size=B, in_block_layers=(48,))
    tr = ppo_v.Trainer(cfg, ppo_v.Parameter(cfg), None)
    tr.update_backend = "srlx"
    tr.on_setup()
    tr.train_on_batch(*[b[k].float().cuda() for k in ("state", "n_state", "action", "old_logpi", "reward", "not_terminated", "total_reward")])
    assert tr.update_path == "torch" and "outside the envelope" in tr.why_not_srlx_update and "(48, 64)" in tr.why_not_srlx_update
    assert all(np.isfinite(v) for v in tr.info.values())


@pytest.mark.parametrize("env", list(ENVS))
def test_runner_trains_and_evaluates_on_the_libsrlx_update(env, monkeypatch):
    monkeypatch.setattr(ppo_v.Trainer, "update_backend", "srlx")
    cfg = ppo_v.Config(batch_size=32)
    cfg.memory.warmup_size = 64
    runner = srl.Runner(env, cfg)
    runner.set_device("cuda:0")
    start = [t.detach().clone() for t in runner.make_parameter().net.parameters()]
    runner.train(max_train_count=30)
    tr = runner.trainer
    assert tr.train_count == 30 and tr.update_path == "srlx" and tr.why_not_srlx_update == ""
    assert {"loss_value", "loss_v_align", "loss_policy"} <= set(tr.info) and all(np.isfinite(v) for v in tr.info.values())
    assert not any(torch.equal(a, c) for a, c in zip(start, runner.parameter.net.parameters()))
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)


@pytest.mark.slow
def test_cartpole_learning_run_srlx_beside_torch():
    """Opt-in (SRLX_RUN_SLOW=1).  The same CartPole run (seed 1, 6000 steps, batch 64, lr 1e-3) on both backends, then 10 evaluation episodes each; the mean
    returns are printed ("VPPO-LEARN ...").  A record, not a gate: the only requirement is that both runs finish on their backend."""
    import random

    def run(backend, seed):
        ppo_v.Trainer.update_backend = backend
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        runner = srl.Runner("CartPole-v1", ppo_v.Config(lr=1e-3))
        runner.set_device("cuda:0")
        runner.set_seed(seed)
        runner.train(max_steps=6000)
        assert runner.trainer.update_path == backend
        return float(np.mean(runner.evaluate(max_episodes=10)))

    default = ppo_v.Trainer.update_backend
    try:
        torch_a, srlx_a = run("torch", 1), run("srlx", 1)
    finally:
        ppo_v.Trainer.update_backend = default
    print(f"VPPO-LEARN mean return over 10 episodes: torch seed 1 {torch_a:.1f}, srlx seed 1 {srlx_a:.1f}")
