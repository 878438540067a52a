"""NoT_SAC on the GPU: libsrlx's fused update (srlx_notsac_update, csrc/srlx_notsac.hip) and forward-only pass over the cases of tests/notsac_cases.py against
the float64 yardstick of tests/notsac_reference.py (which tests/test_notsac_pinned_cpu.py holds to the reference's own code), the plugin's Trainer on the
libsrlx backend, and Runners on Pendulum and CartPole.  Bars (BASELINE's 1e-5): rtol 1e-5 / atol 1e-6 on q, target_q, next_action, pi_action,
the three losses, both norms and every parameter after each update; 1e-5 |g| + 1e-5 max |g| per tensor on every gradient of both networks before and after
its clip.  No case and no element is left out of any comparison.  Every test prints what it measured as a fraction of its bar ("NOTSAC-ERR ...", shown with
-s) before it asserts; the lines are appended to profiles/notsac_gpu_errors.log when SRLX_NOTSAC_LOG=1."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import sac_not

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import notsac_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

SCALARS = ("loss_q", "loss_q_align", "loss_policy", "norm_q", "norm_policy")
ROWS = ("q", "target_q", "next_action", "pi_action")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "notsac_gpu_errors.log")


def _say(line):
    print(line)
    if os.environ.get("SRLX_NOTSAC_LOG") == "1":
        with open(LOG, "a") as f:
            f.write(line + "\n")


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu().reshape(-1)


def _frac(name, got, want):
    """max |got - want| as a fraction of the quantity's bar: rtol 1e-5 and, for a gradient tensor (g.* / raw.*) atol 1e-5 max |want|, for everything else atol
    1e-6.  <= 1 is np.testing.assert_allclose at that bar."""
    atol = 1e-5 * float(want.abs().max()) if name.startswith(("g.", "raw.")) else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _report(tag, got, want):
    """Prints every group's worst fraction of its bar in one line, returns the quantities over their bar."""
    assert set(got) == set(want)
    fr = {name: _frac(name, got[name], want[name]) for name in got}
    groups = {}
    for name, v in fr.items():
        key = name.split("@")[0].split(".")[0]
        groups[key] = max(groups.get(key, 0.0), v)
    _say(f"NOTSAC-ERR {tag} " + " ".join(f"{k}={v:.3f}" for k, v in groups.items()))
    return {k: v for k, v in fr.items() if not v <= 1.0}


def _dev(name, b):
    head = C.spec(name)[2]
    f = lambda x: x.float().cuda()  # noqa: E731
    return dict(state=f(b["state"]), n_state=f(b["n_state"]), action=f(b["action"]) if head else b["action"].argmax(1).int().cuda(), reward=f(b["reward"]),
                not_terminated=f(b["not_terminated"]), total_reward=f(b["total_reward"]), noise=b["noise"].cuda())


def _update(u, cfg, d, lr=None):
    out = u.update(d["state"], d["n_state"], d["action"], d["reward"], d["not_terminated"], d["total_reward"], d["noise"], cfg.lr if lr is None else lr,
                   cfg.discount, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy)
    torch.cuda.synchronize()
    return out


def _two_updates(name, max_batch=None, rows=None, rpw=0):
    """Two libsrlx updates on a fresh GPU parameter of the case (`rows`: only the first so many rows of each batch; `rpw`: rows per workgroup of the row
    kernels, 0 for the library's default, which is ONE row per workgroup for every batch the update admits)."""
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    p = C.make_parameter(name, "cuda")
    u = NotSacUpdate(p, max_batch=max_batch or C.spec(name)[0])
    u.set_rows_per_workgroup(rpw)
    steps = []
    for b in C.make_batches(name):
        d = _dev(name, b)
        if rows is not None:
            d = {k: (v[:, :rows] if k == "noise" else v[:rows]).contiguous() for k, v in d.items()}
        out = _update(u, p.config, d)
        steps.append(dict(out=out, raw=[g.clone() for g in u.raw_grads], grads=[g.clone() for g in u.grads], after=[t.detach().clone() for t in u.params]))
    return p, u, steps


def _quantities(k, out, p_raw, q_raw, p_grads, q_grads, p_params, q_params):
    q = {f"{key}@{k}": _f64(out[key]) for key in ROWS}
    for j, key in enumerate(SCALARS):
        q[f"{key}@{k}"] = _f64(out["scalars"][j] if "scalars" in out else out[key])
    for tag, tensors in (("raw.p", p_raw), ("g.p", p_grads), ("raw.q", q_raw), ("g.q", q_grads), ("params.p", p_params), ("params.q", q_params)):
        q.update({f"{tag}{j}@{k}": _f64(t) for j, t in enumerate(tensors)})
    return q


@functools.lru_cache(maxsize=None)
def _measure(name, rpw=0):
    """Two libsrlx updates of the case at `rpw` rows per workgroup measured against the yardstick, once per case and launch shape."""
    refs = C.reference(name)
    p, u, steps = _two_updates(name, rpw=rpw)
    got, want = {}, {}
    for k, (st, ref) in enumerate(zip(steps, refs)):
        got.update(_quantities(k, st["out"], *u.split(st["raw"]), *u.split(st["grads"]), *u.split(st["after"])))
        want.update(_quantities(k, ref, ref["p_raw_grads"], ref["q_raw_grads"], ref["p_grads"], ref["q_grads"], ref["p_params"], ref["q_params"]))
    bad = _report(name + (f" rows-per-workgroup={rpw}" if rpw else ""), got, want)
    return dict(bad=bad, steps=u.steps(), outs=[st["out"] for st in steps], run=steps)


@pytest.mark.parametrize("rpw", [0, 16])
@pytest.mark.parametrize("name", C.NAMES)
def test_update_matches_float64_yardstick(name, rpw):
    """Two consecutive updates from fixed seeds: q, target_q, next_action, pi_action, the three losses, both raw norms, every gradient tensor of both networks
    before and after its clip, and every parameter after each step, at the bars of the module docstring; at the default launch shape (one row per workgroup)
    and at 16 rows per workgroup, where B = 17 and 33 leave a tail workgroup of one row and B = 1 and 15 a single partial one."""
    m = _measure(name, rpw)
    assert m["steps"] == 2
    assert not m["bad"], f"{name}: over the bar (fraction of it): {m['bad']}"


@pytest.mark.parametrize("rpw", [2, 4, 8, 16])
@pytest.mark.parametrize("name", C.NAMES)
def test_rows_per_workgroup_changes_no_bit_of_an_update(name, rpw):
    """Both updates of every case at 2, 4, 8 and 16 rows per workgroup against the default's one row per workgroup: every output, every gradient of both
    networks before and after its clip and every parameter, bit for bit."""
    one, many = _measure(name)["run"], _two_updates(name, rpw=rpw)[2]
    for sa, sb in zip(one, many):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for key in ("raw", "grads", "after") for x, y in zip(sa[key], sb[key]))


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_only_call(name):
    """The head's outputs and q(s, a) against the yardstick's forward for 1, 15, 16 and 17 rows beside the case's B, nothing written behind the last row; for
    257, 513 and 4097 rows, where rows share workgroups; q of the batch's own rows bit for bit what the update writes."""
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    B, D, head, n_out = C.spec(name)[:4]
    p = C.make_parameter(name, "cuda")
    y = C.yardstick(name, C.make_parameter(name))
    u = NotSacUpdate(p, max_batch=B)
    g = torch.Generator().manual_seed(31 + C.NAMES.index(name))
    lib = N.lib()
    worst = 0.0
    for n in sorted({1, 15, 16, 17, B}):
        x = torch.randn(n, D, generator=g)
        a = torch.softmax(torch.randn(n, n_out, generator=g), dim=1) if not head else torch.tanh(torch.randn(n, n_out, generator=g))
        want_h, want_q = y.forward(x.double(), a.double())
        xd, ad = x.cuda(), a.cuda()
        h0, h1 = torch.full((n + 1, n_out), 7.0, device="cuda"), torch.full((n + 1, n_out), 7.0, device="cuda")
        q = torch.full((n + 1,), 7.0, device="cuda")
        N.check(lib.srlx_notsac_forward(u._h, n, N.tptr(xd), u.ls_lo, u.ls_hi, N.tptr(h0), N.tptr(h1) if head else None, N.tptr(ad), N.tptr(q), None))
        torch.cuda.synchronize()
        assert float(q[n]) == 7.0 and bool((h0[n] == 7.0).all()) and bool((h1[n] == 7.0).all())
        worst = max(worst, _frac("q", _f64(q[:n]), _f64(want_q)))
        if head:
            worst = max(worst, _frac("loc", _f64(h0[:n]), _f64(want_h[0])), _frac("ls", _f64(h1[:n]), _f64(want_h[1])))
        else:
            worst = max(worst, _frac("logits", _f64(h0[:n]), _f64(want_h)))
    # more than 256 rows: the default launch shape is 2, 4 and 16 rows per workgroup, each with a tail workgroup of one row; against the yardstick and against
    # the bits of the same rows at one row per workgroup
    for n, rpw in ((257, 2), (513, 4), (4097, 16)):
        x = torch.randn(n, D, generator=g)
        a = torch.softmax(torch.randn(n, n_out, generator=g), dim=1) if not head else torch.tanh(torch.randn(n, n_out, generator=g))
        want_h, want_q = y.forward(x.double(), a.double())
        got = {}
        for shape in (0, 1, rpw):
            u.set_rows_per_workgroup(shape)
            got[shape] = u.forward(x.cuda(), a.cuda())
            torch.cuda.synchronize()
        u.set_rows_per_workgroup(0)
        heads, q = got[0]
        heads = heads if head else (heads,)
        for shape in (1, rpw):
            other = got[shape][0] if head else (got[shape][0],)
            assert torch.equal(q, got[shape][1]) and all(torch.equal(h, o) for h, o in zip(heads, other)), (n, shape)
        worst = max(worst, _frac("q", _f64(q), _f64(want_q)))
        for h, w in zip(heads, want_h if head else (want_h,)):
            worst = max(worst, _frac("head", _f64(h), _f64(w)))
    b = C.make_batches(name)[0]
    d = _dev(name, b)
    _, q = u.forward(d["state"], b["action"].float().cuda(), want_head=False)
    out = _update(u, p.config, d)  # (last: it moves the parameters)
    assert torch.equal(q, out["q"])
    _say(f"NOTSAC-ERR forward {name} worst={worst:.3f}")
    assert worst <= 1.0


def test_two_fresh_handles_give_equal_bits():
    for name in ("wide", "cat-a16-b17"):
        a, b = _two_updates(name), _two_updates(name)
        for sa, sb in zip(a[2], b[2]):
            assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
            assert all(torch.equal(x, y) for key in ("raw", "grads", "after") for x, y in zip(sa[key], sb[key]))


@pytest.mark.parametrize("name", ["b17-mixed", "cat-a16-b17"])
def test_a_rows_outputs_do_not_depend_on_the_rows_that_share_its_workgroup(name):
    """At 16 rows per workgroup (the default launch shape gives every row a workgroup of its own and could not fail this): B = 16, one full workgroup, against
    the first 16 rows of B = 17, a full workgroup and a tail of one row, and both against those rows alone in their workgroups; the per-row outputs of the first
    update, bit for bit."""
    full, part, alone = _two_updates(name, rpw=16), _two_updates(name, rows=16, rpw=16), _two_updates(name, rows=16, rpw=1)
    for key in ROWS:
        assert torch.equal(full[2][0]["out"][key][:16], part[2][0]["out"][key]), key
        assert torch.equal(alone[2][0]["out"][key], part[2][0]["out"][key]), key


def test_steps_count_and_the_learning_rate_reaches_adam():
    """Adam's first step moves a parameter by lr g / (|g| + eps): twice the learning rate, twice the move of every Q-network parameter (whose gradient does not
    depend on the rate; the policy's is taken through the Q-network already stepped at that rate, so only its bound is checked); lr 0 moves nothing."""
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    name = "k8-b33"
    d = _dev(name, C.make_batches(name)[0])
    moves = []
    for lr in (1e-4, 2e-4, 0.0):
        p = C.make_parameter(name, "cuda")
        u = NotSacUpdate(p, max_batch=33)
        before = [t.detach().clone() for t in u.params]
        assert u.steps() == 0
        _update(u, p.config, d, lr=lr)
        assert u.steps() == 1
        moves.append([torch.cat([(a.detach() - b).reshape(-1) for a, b in zip(*pair)]) for pair in zip(u.split(u.params), u.split(before))])
    assert float(moves[2][0].abs().max()) == 0.0 and float(moves[2][1].abs().max()) == 0.0
    # a move is read off float32 parameters: each difference carries up to one unit in the last place of the parameter, 2^-23 max |p|
    ulp = 2.0 ** -23 * max(1.0, max(float(t.abs().max()) for t in before))
    big = moves[0][1].abs() > 0.5e-4
    assert int(big.sum()) > 1000
    assert torch.allclose(moves[1][1][big], 2 * moves[0][1][big], rtol=1e-4, atol=3 * ulp)
    for k, lr in enumerate((1e-4, 2e-4)):
        assert 0.5 * lr < float(moves[k][0].abs().max()) <= lr + ulp and float(moves[k][1].abs().max()) <= lr + ulp


def test_trainer_schedule_reaches_the_libsrlx_update():
    name = "default-b16"
    p = C.make_parameter(name, "cuda")
    cfg = p.config
    cfg.lr_scheduler.set_step(1, 0.5)  # the rate halves after every step
    tr = sac_not.Trainer(cfg, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    b = C.make_batches(name)[0]
    args = (b["state"].float().cuda(), b["n_state"].float().cuda(), b["action"].float().cuda(), b["reward"].float().cuda().reshape(-1, 1),
            b["not_terminated"].float().cuda().reshape(-1, 1), b["total_reward"].float().cuda().reshape(-1, 1))
    assert tr._backend_for(16) == "srlx"
    seen, update = [], tr._srlx.update
    tr._srlx.update = lambda *a, **kw: (seen.append(a[7]), update(*a, **kw))[1]
    for k in range(2):
        tr.train_on_batch(*args, noise=b["noise"].cuda())
    assert tr.update_path == "srlx" and tr.why_not_srlx_update == "" and tr._srlx.steps() == 2
    assert seen == [cfg.lr * cfg.lr_scheduler.factor(0, cfg.lr), cfg.lr * cfg.lr_scheduler.factor(1, cfg.lr)] and seen[1] == pytest.approx(0.5 * seen[0])


def test_refusals():
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate
    from simple_distributed_rl_amd._native import SrlxError

    name = "b17-mixed"
    B = C.spec(name)[0]
    p = C.make_parameter(name, "cuda")
    u = NotSacUpdate(p, max_batch=B - 1)
    before = [t.detach().clone() for t in u.params]
    d = _dev(name, C.make_batches(name)[0])
    with pytest.raises(ValueError, match="above max_batch"):
        _update(u, p.config, d)
    for rows in (3, 32, -1):
        with pytest.raises(SrlxError, match="notsac_set_rows_per_workgroup"):
            u.set_rows_per_workgroup(rows)
    lib = N.lib()
    out = torch.full((B * 2,), 7.0, device="cuda")

    def raw_update(h):
        return lib.srlx_notsac_update(h, B, N.tptr(d["state"]), N.tptr(d["n_state"]), N.tptr(d["action"]), N.tptr(d["reward"]), N.tptr(d["not_terminated"]),
                                      N.tptr(d["total_reward"]), N.tptr(d["noise"]), C.LR, C.DISCOUNT, C.ALIGN, 10.0, 0, u.ls_lo, u.ls_hi, N.tptr(out), N.tptr(out),
                                      N.tptr(out), N.tptr(out), N.tptr(out), None)

    assert raw_update(u._h) == N.ERR_INVALID and b"notsac_update: batch" in lib.srlx_last_error()
    # a second bind of the wrong count leaves the handle as it was
    assert lib.srlx_notsac_bind(u._h, len(u.params) - 2, N._ptrs(u.params[:-2])) == N.ERR_INVALID and b"notsac_bind: " in lib.srlx_last_error()
    # an update before bind_adam
    import ctypes

    h = N.c_p()
    N.check(lib.srlx_notsac_create(ctypes.byref(h), u.D, u.head, u.n_out, len(u.policy_widths), N._int_array(u.policy_widths), len(u.q_widths),
                                   N._int_array(u.q_widths), u.act_emb, B, 0))
    N.check(lib.srlx_notsac_bind(h, len(u.params), N._ptrs(u.params)))
    N.check(lib.srlx_notsac_bind_grads(h, len(u.params), N._ptrs(u.grads), N._ptrs(u.raw_grads)))
    assert raw_update(h) == N.ERR_INVALID and b"bind the parameters, the gradient tensors and the Adam state first" in lib.srlx_last_error()
    lib.srlx_notsac_destroy(h)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and u.steps() == 0
    assert all(torch.equal(x, y) for x, y in zip(before, u.params))
    assert all(not bool(g.any()) for g in u.grads + u.raw_grads)
    _update(u, p.config, {k: (v[:, :B - 1] if k == "noise" else v[:B - 1]).contiguous() for k, v in d.items()})  # the handle still serves its own size
    assert u.steps() == 1


# ---- Trainer and plugin -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default-b16", "cat-default"])
def test_trainer_on_gpu_parameters_runs_the_libsrlx_update_and_follows_the_yardstick(name):
    ref = C.reference(name)[0]
    b = C.make_batches(name)[0]
    p = C.make_parameter(name, "cuda")
    tr = sac_not.Trainer(p.config, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    B = b["state"].shape[0]
    col = lambda x: x.float().cuda().reshape(B, 1)  # noqa: E731
    out = tr.train_on_batch(b["state"].float().cuda(), b["n_state"].float().cuda(), b["action"].float().cuda(), col(b["reward"]), col(b["not_terminated"]),
                            col(b["total_reward"]), noise=b["noise"].cuda())
    assert tr.update_path == "srlx" and tr.why_not_srlx_update == "" and tr.train_count == 1
    assert set(tr.info) == {"loss_q", "loss_q_align", "loss_policy"}
    for j, key in enumerate(SCALARS[:3]):
        assert tr.info[key] == pytest.approx(ref[key], rel=1e-5, abs=1e-6)
    assert _frac("pi_action", _f64(out["pi_action"]), _f64(ref["pi_action"])) <= 1.0
    tr.train_on_batch(b["state"].float().cuda(), b["n_state"].float().cuda(), b["action"].float().cuda(), col(b["reward"]), col(b["not_terminated"]),
                      col(b["total_reward"]))  # noise=None: drawn on the device
    assert tr.train_count == 2 and all(np.isfinite(v) for v in tr.info.values())


@pytest.mark.parametrize("env", ["Pendulum-v1", "CartPole-v1"])
def test_runner_trains_and_evaluates_on_the_libsrlx_update(env, monkeypatch):
    monkeypatch.setattr(sac_not.Trainer, "update_backend", "srlx")
    cfg = sac_not.Config(batch_size=32)
    cfg.memory.warmup_size = 64
    runner = srl.Runner(env, cfg)
    runner.set_device("cuda:0")
    tensors = lambda p: list(p.policy.parameters()) + list(p.qnet.parameters())  # noqa: E731
    start = [t.detach().clone() for t in tensors(runner.make_parameter())]
    ptrs = [t.data_ptr() for t in tensors(runner.parameter)]
    runner.train(max_train_count=30)
    tr = runner.trainer
    assert tr.train_count == 30 and tr.update_path == "srlx" and tr.why_not_srlx_update == ""
    assert set(tr.info) == {"loss_q", "loss_q_align", "loss_policy"} and all(np.isfinite(v) for v in tr.info.values())
    assert not any(torch.equal(a, c) for a, c in zip(start, tensors(runner.parameter)))
    assert ptrs == [t.data_ptr() for t in tensors(runner.parameter)]  # trained in place
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)


@pytest.mark.slow
@pytest.mark.parametrize("env, steps", [("Pendulum-v1", 6000), ("CartPole-v1", 6000)])
def test_learning_run_srlx_beside_torch(env, steps):
    """Opt-in (SRLX_RUN_SLOW=1).  The same run (seed 1, batch 64, lr 1e-3) on both backends, then 10 evaluation episodes each; the mean returns are written to
    profiles/notsac_learning.log.  A record, not a gate: the only requirement is that both runs finish on their backend."""
    import random

    def run(backend, seed):
        sac_not.Trainer.update_backend = backend
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        runner = srl.Runner(env, sac_not.Config(lr=1e-3))
        runner.set_device("cuda:0")
        runner.set_seed(seed)
        runner.train(max_steps=steps)
        assert runner.trainer.update_path == backend
        return float(np.mean(runner.evaluate(max_episodes=10)))

    default = sac_not.Trainer.update_backend
    try:
        torch_a, srlx_a = run("torch", 1), run("srlx", 1)
    finally:
        sac_not.Trainer.update_backend = default
    line = f"NOTSAC-LEARN {env} {steps} steps, mean return over 10 episodes: torch seed 1 {torch_a:.1f}, srlx seed 1 {srlx_a:.1f}"
    print(line)
    with open(os.path.join(os.path.dirname(LOG), "notsac_learning.log"), "a") as f:
        f.write(line + "\n")
