"""Discrete SAC on the GPU: libsrlx's fused update (srlx_sacd_update, csrc/srlx_sacd.hip) and forward-only pass over the shapes of tests/sacd_cases.py against
the float64 yardstick of tests/sacd_reference.py (whose footing tests/test_sacd_cpu.py checks; parity with the TensorFlow reference is unpinned), the plugin's
Trainer on both backends, and a Runner on CartPole.  Bars (BASELINE's 1e-5): rtol 1e-5 / atol 1e-6 on y, q1, q2, entropy, the four losses and
alpha; 1e-5 |g| + 1e-5 max |g| per tensor on every gradient; the parameters after two updates equal to torch.optim.Adam (float32) on the kernel's own
gradients at rtol 1e-6 and to the yardstick's at rtol 1e-5 / atol 1e-6; a soft-synced target within 1 ulp of the float32 formula, a hard-synced one bit for bit.
Every test prints what it measured as a fraction of its bar ("SACD-ERR ...", shown with -s) before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import sac

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_cases as C  # noqa: E402
import sacd_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

TRAINED = ("policy", "q1_online", "q2_online")
CASES = [(i, auto) for i in range(len(C.SHAPES)) for auto in (True, False)]
CASE_IDS = [f"{C.shape_id(i)}-{'auto' if auto else 'fixed'}" for i, auto in CASES]


def _cfg(i, device, auto=True, **kw):
    B, D, A, pw, qw = C.SHAPES[i]
    return C.make_config(D, A, pw, qw, device=device, lr_policy=C.LR, lr_q=C.LR, lr_alpha=C.LR, discount=C.DISCOUNT, soft_target_update_tau=C.TAU,
                         entropy_alpha_auto_scale=auto, **kw)


def _batches(i):
    B, D, A, _, _ = C.SHAPES[i]
    return [C.make_batch(B, D, A, 100 * i + k) for k in range(2)]


def _snapshot(obj):
    return {name: [t.detach().clone() for t in getattr(obj, name).parameters()] for name in R.NETWORKS}


@functools.lru_cache(maxsize=None)
def _reference(i, auto, clip=False, dtype=torch.float64):
    """The yardstick's two updates (a hard sync, then a soft one) on the case's batches: computed once per case, shared, never modified.  With
    dtype=torch.float32 the same program in float32: how far float32 itself is from a bar (the figure quoted for the hard case below)."""
    A = C.SHAPES[i][2]
    p = C.make_parameter(_cfg(i, "cpu", auto), 1000 + i, clip_case=clip)
    y = R.Yardstick(p, C.LR, C.LR, C.LR, C.DISCOUNT, C.TAU, auto, -A, dtype=dtype)
    outs = []
    for k, b in enumerate(_batches(i)):
        out = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=k == 0)
        out["params"], out["log_alpha"] = _snapshot(y), float(y.log_alpha.detach())
        outs.append(out)
    return outs


def _dev(b):
    return dict(state=b["state"].float().cuda(), action=b["action"].int().cuda(), n_state=b["n_state"].float().cuda(), reward=b["reward"].float().cuda(),
                done=b["done"].to(torch.uint8).cuda(), onehot=b["onehot"].float().cuda())


def _update(u, b, lr, hard, auto, A):
    d = _dev(b)
    out = u.update(d["state"], d["action"], d["n_state"], d["reward"], d["done"], lr, lr, lr, hard, C.DISCOUNT, C.TAU, auto, -A)
    torch.cuda.synchronize()
    return out


SCALARS = ("q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha")


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu().reshape(-1)


def _update_quantities(k, out, grads, grad_log_alpha):
    """One update as {name@k: float64 CPU vector}.  `out`: the yardstick's dict, or the kernel's with its five scalars in out["scalars"]."""
    q = {f"{key}@{k}": _f64(out[key]) for key in ("y", "q1", "q2", "entropy")}
    for j, key in enumerate(SCALARS):
        q[f"{key}@{k}"] = _f64(out["scalars"][j] if "scalars" in out else out[key])
    for name in TRAINED:
        for j, g in enumerate(grads[name]):
            q[f"g_{name}.{j}@{k}"] = _f64(g)
    q[f"g_log_alpha@{k}"] = _f64(grad_log_alpha)
    return q


def _param_quantities(params, log_alpha):
    q = {f"p_{name}.{j}": _f64(t) for name in R.NETWORKS for j, t in enumerate(params[name])}
    q["p_log_alpha"] = _f64(log_alpha)
    return q


def _yardstick_quantities(outs):
    q = {}
    for k, o in enumerate(outs):
        q.update(_update_quantities(k, o, o["grads"], o["grads"]["log_alpha"]))
    q.update(_param_quantities(outs[-1]["params"], outs[-1]["log_alpha"]))
    return q


def _frac(name, got, want):
    """max |got - want| as a fraction of the quantity's bar: rtol 1e-5 and, for a gradient tensor (g_*) atol 1e-5 max |want|, for everything else atol 1e-6.
    <= 1 is np.testing.assert_allclose at that bar."""
    atol = 1e-5 * float(want.abs().max()) if name.startswith("g_") else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _report(tag, got, want):
    """Prints every group's worst fraction of its bar, returns the quantities over their bar."""
    fr = {name: _frac(name, got[name], want[name]) for name in got}
    groups = {}
    for name, v in fr.items():
        key = name.split("@")[0].split(".")[0] + ("@" + name.split("@")[1] if "@" in name else "")
        groups[key] = max(groups.get(key, 0.0), v)
    print(f"SACD-ERR {tag} " + " ".join(f"{k}={v:.3f}" for k, v in groups.items()))
    return {k: v for k, v in fr.items() if not v <= 1.0}


def _ulps(a, b):
    """Distance in float32 ulps between two float32 arrays."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _two_updates(i, auto, clip=False):
    """Two libsrlx updates on a fresh GPU parameter of the case; yields everything the tests look at."""
    from simple_distributed_rl_amd.device.sacd import SacdUpdate

    B, D, A, pw, qw = C.SHAPES[i]
    p = C.make_parameter(_cfg(i, "cuda", auto), 1000 + i, clip_case=clip)
    u = SacdUpdate(p, max_batch=B)
    # torch.optim.Adam (float32, on the GPU: the implementation whose roundings csrc/srlx_adam_math.h:adam_one_foreach states) on the kernel's own gradients
    shadow = {name: [t.detach().clone().requires_grad_(True) for t in getattr(p, name).parameters()] for name in TRAINED}
    shadow["log_alpha"] = [p.log_alpha.detach().clone().requires_grad_(True)]
    opts = {name: torch.optim.Adam(ts, lr=C.LR) for name, ts in shadow.items()}
    steps = []
    for k, b in enumerate(_batches(i)):
        before = _snapshot(p)
        out = _update(u, b, C.LR, k == 0, auto, A)
        grads = {name: [g.clone() for g in u.grads[name]] for name in TRAINED}
        gla = u.grad_log_alpha.clone()
        for name in TRAINED:
            for s, g in zip(shadow[name], grads[name]):
                s.grad = g.clone()
            opts[name].step()
        if auto:
            shadow["log_alpha"][0].grad = gla.clone()
            opts["log_alpha"].step()
        steps.append(dict(out=out, grads=grads, gla=gla, before=before, after=_snapshot(p), log_alpha=float(p.log_alpha)))
    return p, u, shadow, steps


@functools.lru_cache(maxsize=None)
def _measure(i, auto, clip=False):
    """Two libsrlx updates of the case measured against the yardstick, once per case (the tests below share it): the quantities over their bar, the distance
    from torch.optim.Adam on the kernel's own gradients, the soft sync's distance in ulps."""
    tag = ("clip-" if clip else "") + C.shape_id(i) + ("-auto" if auto else "-fixed")
    refs = _reference(i, auto, clip)
    p, u, shadow, steps = _two_updates(i, auto, clip)
    got = {}
    for k, st in enumerate(steps):
        got.update(_update_quantities(k, st["out"], st["grads"], st["gla"]))
    got.update(_param_quantities(steps[1]["after"], steps[1]["log_alpha"]))
    bad = _report(tag, got, _yardstick_quantities(refs))
    # the target sync of each update (step 5), from the tensors the kernel itself left
    sync_ulp, hard_is_copy = 0, True
    for k, st in enumerate(steps):
        for tname, oname in (("q1_target", "q1_online"), ("q2_target", "q2_online")):
            for t0, t1, w1 in zip(st["before"][tname], st["after"][tname], st["after"][oname]):
                if k == 0:
                    hard_is_copy &= torch.equal(t1, w1)
                else:
                    want = np.float32(1.0 - C.TAU) * t0.cpu().numpy() + np.float32(C.TAU) * w1.cpu().numpy()
                    sync_ulp = max(sync_ulp, int(_ulps(t1.cpu().numpy().reshape(-1), want.astype(np.float32).reshape(-1)).max()))
    # parameters after two updates against torch.optim.Adam (float32) on the kernel's own gradients: rtol 1e-6, no absolute term
    adam = 0.0
    for a, s in [(a, s) for name in TRAINED for a, s in zip(steps[1]["after"][name], shadow[name])] + [(steps[1]["log_alpha"], shadow["log_alpha"][0])]:
        a, s = _f64(a), _f64(s)
        adam = max(adam, float(((a - s).abs() / (1e-6 * s.abs() + 1e-300)).max()))
    print(f"SACD-ERR {tag} params_vs_torch_adam={adam:.3f} soft_sync_ulp={sync_ulp} hard_sync_is_copy={hard_is_copy} steps={u.steps()}")
    return dict(tag=tag, bad=bad, adam=adam, sync_ulp=sync_ulp, hard_is_copy=hard_is_copy, steps=u.steps(), log_alpha=steps[1]["log_alpha"],
                alpha_loss=float(steps[1]["out"]["scalars"][3]), y0=steps[0]["out"]["y"].cpu())


def _assert_update(i, auto, clip=False):
    m = _measure(i, auto, clip)
    assert m["steps"] == [2, 2, 2, 2 if auto else 0]
    if not auto:
        assert m["log_alpha"] == pytest.approx(np.log(0.2), rel=1e-6) and m["alpha_loss"] == 0.0
    assert m["hard_is_copy"] and m["sync_ulp"] <= 1 and m["adam"] <= 1.0, m
    bad = {k: v for k, v in m["bad"].items() if not k.startswith("p_")}
    assert not bad, f"{m['tag']}: over the bar (fraction of it): {bad}"
    b = _batches(i)[0]
    assert float(m["y0"][0]) == float(b["reward"][0].float())  # a done row has y = r


@pytest.mark.parametrize("i, auto", CASES, ids=CASE_IDS)
def test_update_matches_float64_yardstick(i, auto):
    """Two updates from fixed seeds (a hard sync, then a soft one; about a fifth of the rows done; a non-zero policy out layer; sac.Config()'s learning rates):
    y, q1, q2, entropy, the four losses, alpha and every gradient tensor of both updates at the bars of the module docstring; the parameters after the two
    updates equal to torch.optim.Adam (float32) on the kernel's own gradients at rtol 1e-6; the hard sync a copy, the soft sync within 1 ulp.  A done row has
    y = r."""
    _assert_update(i, auto)
    for ref in _reference(i, auto):  # no probability of the case is near the clip: 1e-7 cannot fall between the float32 and the float64 value
        assert not bool(((ref["probs"] >= 5e-8) & (ref["probs"] <= 2e-7)).any())


@pytest.mark.parametrize("i, auto", CASES + [(C.CLIP_SHAPE, None)], ids=CASE_IDS + ["forced-clip"])
def test_parameters_after_two_updates_match_float64_yardstick(i, auto):
    """Every tensor of the five networks and log_alpha after the two updates against the yardstick's float64 parameters at rtol 1e-5 / atol 1e-6, no slack.
    The hard case is B17-D256-A16-p32-q512: one first-layer weight of q2 has a first gradient of 8.3e-9 = 1.2e-7 max |g| (17 terms of about 1e-3 that cancel),
    and Adam's first step lr g / (|g| + eps) turns a relative error of such an entry into a parameter error of lr / 4 times it.  The yardstick's own float32 run
    is at 1.22 of the bar there; the kernels, which accumulate every sum in float64, at 0.25 (with float32 sums they were at 4.67)."""
    m = _measure(i, True, clip=True) if auto is None else _measure(i, auto)
    bad = {k: v for k, v in m["bad"].items() if k.startswith("p_")}
    assert not bad, f"{m['tag']}: over the bar (fraction of it): {bad}"


def test_forced_clip_case_follows_the_closed_form():
    """The forced-clip construction at shape 2: every row has one probability near 1e-9 (clipped: no alpha term in its gradient) and one near 2e-5 (inside)."""
    _assert_update(C.CLIP_SHAPE, True, clip=True)
    refs = _reference(C.CLIP_SHAPE, True, True)
    for ref in refs:
        pr = ref["probs"]
        assert bool(((pr < 5e-8).sum(1) == 1).all()) and bool((((pr > 2e-7) & (pr < 1e-4)).sum(1) == 1).all())
        assert not bool(((pr >= 5e-8) & (pr <= 2e-7)).any())
    print(f"SACD-ERR clip smallest_probability={float(refs[0]['probs'].min()):.3e}")


@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=C.shape_id)
def test_forward_only_call(i):
    """Logits and min(q1, q2) over every action, online and target, against the float64 modules; for 1, 15, 16 and 17 rows beside the case's B (16 / A items per
    workgroup), with nothing written behind the last row."""
    from simple_distributed_rl_amd.device.sacd import SacdUpdate

    B, D, A, pw, qw = C.SHAPES[i]
    p = C.make_parameter(_cfg(i, "cuda"), 1000 + i)
    p64 = R.Yardstick(C.make_parameter(_cfg(i, "cpu"), 1000 + i), 0, 0, 0, C.DISCOUNT, C.TAU, True, -A)
    u = SacdUpdate(p, max_batch=1)
    lib, worst = N.lib(), 0.0
    g = torch.Generator().manual_seed(i)
    for n in sorted({1, 15, 16, 17, B}):
        x = torch.randn(n, D, generator=g)
        with torch.no_grad():
            want_logits = p64.policy(x.double())
            want_q = [R.all_q(x.double(), A, p64.q1_online, p64.q2_online), R.all_q(x.double(), A, p64.q1_target, p64.q2_target)]
        xd = x.cuda()
        for target in (0, 1):
            logits, q = torch.full((n + 1, A), 7.0, device="cuda"), torch.full((n + 1, A), 7.0, device="cuda")
            N.check(lib.srlx_sacd_forward(u._h, n, N.tptr(xd), target, N.tptr(logits), N.tptr(q), None))
            torch.cuda.synchronize()
            assert bool((logits[n] == 7.0).all()) and bool((q[n] == 7.0).all())
            worst = max(worst, _frac("logits", _f64(logits[:n]), _f64(want_logits)), _frac("qmin", _f64(q[:n]), _f64(want_q[target])))
        only_q = u.forward(xd, target=True, want_logits=False)
        assert only_q[0] is None and torch.equal(only_q[1], q[:n])
    print(f"SACD-ERR forward {C.shape_id(i)} worst={worst:.3f}")
    assert worst <= 1.0


def test_two_fresh_handles_give_equal_bits():
    a, b = _two_updates(3, True), _two_updates(3, True)
    for sa, sb in zip(a[3], b[3]):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for name in TRAINED for x, y in zip(sa["grads"][name], sb["grads"][name])) and torch.equal(sa["gla"], sb["gla"])
        assert all(torch.equal(x, y) for name in R.NETWORKS for x, y in zip(sa["after"][name], sb["after"][name])) and sa["log_alpha"] == sb["log_alpha"]


def test_update_refuses_a_batch_above_max_batch_and_writes_nothing():
    from simple_distributed_rl_amd.device.sacd import SacdUpdate

    B, D, A, pw, qw = C.SHAPES[2]
    p = C.make_parameter(_cfg(2, "cuda"), 5)
    u = SacdUpdate(p, max_batch=B - 1)
    before = _snapshot(p)
    with pytest.raises(ValueError, match="above max_batch"):
        _update(u, _batches(2)[0], C.LR, True, True, A)
    d = _dev(_batches(2)[0])
    out = torch.full((B,), 7.0, device="cuda")
    st = N.lib().srlx_sacd_update(u._h, B, N.tptr(d["state"]), N.tptr(d["action"]), N.tptr(d["n_state"]), N.tptr(d["reward"]), N.tptr(d["done"]), C.LR, C.LR, C.LR,
                                  C.DISCOUNT, C.TAU, 1, 1, -float(A), N.tptr(out), N.tptr(out), N.tptr(out), N.tptr(out), N.tptr(out), None)
    torch.cuda.synchronize()
    assert st == N.ERR_INVALID and b"sacd_update: batch" in N.lib().srlx_last_error()
    assert bool((out == 7.0).all()) and u.steps() == [0, 0, 0, 0]
    assert all(torch.equal(x, y) for name in R.NETWORKS for x, y in zip(before[name], _snapshot(p)[name]))


# ---- Trainer and plugin -----------------------------------------------------------------------------------------------------------------------------------------
def _cartpole_batch(B):
    """One sampled batch of a CartPole run the Worker produced (random actions during start_steps)."""
    import random

    random.seed(3)
    np.random.seed(3)
    cfg = sac.Config(batch_size=B, start_steps=64)
    cfg.memory.warmup_size = 64
    runner = srl.Runner("CartPole-v1", cfg)
    runner.set_device("cpu")
    runner.rollout(max_memory=96)
    items = runner.memory.sample()
    state, onehot, n_state, reward, done = zip(*items)
    return dict(state=torch.tensor(np.asarray(state), dtype=torch.float64), onehot=torch.tensor(np.asarray(onehot), dtype=torch.float64),
                n_state=torch.tensor(np.asarray(n_state), dtype=torch.float64), reward=torch.tensor(np.asarray(reward), dtype=torch.float64),
                done=torch.tensor(np.asarray(done), dtype=torch.float64))


@pytest.mark.parametrize("backend", ["srlx", "torch"])
def test_trainer_backends_follow_the_yardstick_on_a_cartpole_batch(backend):
    B, A = 8, 2
    b = _cartpole_batch(B)
    cfg = C.make_config(4, A, (64, 64, 64), (128, 128, 128), device="cuda", batch_size=B)
    p = C.make_parameter(cfg, 77)
    y = R.Yardstick(p, cfg.lr_policy, cfg.lr_q, cfg.lr_alpha, cfg.discount, cfg.soft_target_update_tau, True, -A)
    ref = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=True)
    tr = sac.Trainer(cfg, p, None)
    tr.update_backend = backend
    tr.on_setup()
    if backend == "torch":  # autograd's gradients, as the optimisers read them
        grads = {}
        for name in TRAINED:
            for k, t in enumerate(getattr(p, name).parameters()):
                t.register_hook(lambda g, name=name, k=k: grads.setdefault(name, {}).__setitem__(k, g.clone()))
    out = tr.train_on_batch(b["state"].float().cuda(), b["onehot"].float().cuda(), b["n_state"].float().cuda(), b["reward"].float().cuda(),
                            b["done"].to(torch.uint8).cuda())
    torch.cuda.synchronize()
    assert tr.update_path == backend and tr.why_not_srlx_update == "" and tr.train_count == 1
    if backend == "srlx":
        got, gla = tr._srlx.grads, tr._srlx.grad_log_alpha
    else:
        got, gla = {name: [grads[name][k] for k in sorted(grads[name])] for name in TRAINED}, p.log_alpha.grad
    bad = _report(f"trainer-{backend}", _update_quantities(0, out, got, gla), _update_quantities(0, ref, ref["grads"], ref["grads"]["log_alpha"]))
    assert set(tr.info) == {"q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha"} and all(np.isfinite(v) for v in tr.info.values())
    assert tr.info["q1_loss"] == pytest.approx(float(ref["q1_loss"]), rel=1e-5, abs=1e-6)
    assert not bad, bad
    tr.update_backend = "torch" if backend == "srlx" else "srlx"  # fixed for the Trainer's life at the first train()
    tr.train_on_batch(b["state"].float().cuda(), b["onehot"].float().cuda(), b["n_state"].float().cuda(), b["reward"].float().cuda(), b["done"].to(torch.uint8).cuda())
    assert tr.update_path == backend


def test_trainer_with_an_input_block_layer_runs_torch_and_says_why():
    B, A = 8, 2
    b = _cartpole_batch(B)
    cfg = C.make_config(4, A, (64,), (64,), device="cuda", batch_size=B, in_block_layers=(32,))
    tr = sac.Trainer(cfg, C.make_parameter(cfg, 78), None)
    tr.update_backend = "srlx"
    tr.on_setup()
    tr.train_on_batch(b["state"].float().cuda(), b["onehot"].float().cuda(), b["n_state"].float().cuda(), b["reward"].float().cuda(), b["done"].to(torch.uint8).cuda())
    assert tr.update_path == "torch" and "input_block has layers of its own" in tr.why_not_srlx_update
    assert all(np.isfinite(v) for v in tr.info.values())


def _runner(backend, start_steps=64, warmup=64, **kw):
    cfg = sac.Config(start_steps=start_steps, **kw)
    cfg.memory.warmup_size = warmup
    runner = srl.Runner("CartPole-v1", cfg)
    runner.set_device("cuda:0")
    return runner


@pytest.mark.parametrize("backend", ["srlx", "torch"])
def test_runner_trains_and_evaluates_on_cartpole(backend, monkeypatch):
    monkeypatch.setattr(sac.Trainer, "update_backend", backend)
    runner = _runner(backend)
    runner.set_vector_envs(16)
    start = _snapshot(runner.make_parameter())
    runner.train(max_train_count=30)
    assert runner.vector_reason == "no device engine for algorithm 'SAC_Discrete'"
    tr, p = runner.trainer, runner.parameter
    assert tr.train_count == 30 and tr.update_path == backend
    assert set(tr.info) == {"q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha"} and all(np.isfinite(v) for v in tr.info.values())
    end = _snapshot(p)
    for name in TRAINED:
        assert not any(torch.equal(a, c) for a, c in zip(start[name], end[name])), name
    for tname, oname in (("q1_target", "q1_online"), ("q2_target", "q2_online")):  # the last update was a soft sync
        assert not any(torch.equal(a, c) for a, c in zip(end[tname], end[oname]))
    assert float(p.log_alpha.detach()) != pytest.approx(np.log(0.2), rel=1e-9)
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(r >= 1 for r in rewards)


@pytest.mark.slow
def test_cartpole_learning_run_srlx_beside_torch():
    """Opt-in (SRLX_RUN_SLOW=1).  The same CartPole run (seed 1, 3000 steps after 500 random ones, batch 32, lr 1e-3 for all three) on both backends, then 10
    evaluation episodes each.  No return threshold is invented: the bar of the libsrlx backend is the torch backend's own mean return from this same run, with
    the spread the torch backend shows between two seeds as slack; both returns are printed ("SACD-LEARN ...")."""
    import random

    def run(backend, seed):
        sac.Trainer.update_backend = backend
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        runner = _runner(backend, start_steps=500, warmup=500, lr_policy=1e-3, lr_q=1e-3, lr_alpha=1e-3)
        runner.set_seed(seed)
        runner.train(max_steps=3500)
        assert runner.trainer.update_path == backend
        return float(np.mean(runner.evaluate(max_episodes=10)))

    default = sac.Trainer.update_backend
    try:
        torch_a, torch_b, srlx_a = run("torch", 1), run("torch", 2), run("srlx", 1)
    finally:
        sac.Trainer.update_backend = default
    print(f"SACD-LEARN mean return over 10 episodes: torch seed 1 {torch_a:.1f}, torch seed 2 {torch_b:.1f}, srlx seed 1 {srlx_a:.1f}")
    assert srlx_a >= min(torch_a, torch_b) - abs(torch_a - torch_b)
