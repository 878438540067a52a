"""PPO's fused actor-critic kernels (csrc/srlx_ppo_net.hip: k_ppo_forward, k_ppo_rollout, k_ppo_minibatch, k_ppo_reduce, k_ppo_adam) over the envelope they admit --
observation length 1..8; Normal head: 1..4 action dimensions; categorical head: 2..8 actions -- at the row counts, sample counts and horizons where their loops,
tiles and LDS layouts change path.  The yardstick is the project's `ActorCritic` torch module in float64 and float64 autograd of the restated loss
(tests/test_ppo_gpu.py: _torch_loss; tests/ppo_cat_reference.py: torch_loss), torch.nn.utils.clip_grad_norm_ + torch.optim.Adam for the optimiser, and -- where
bit-equality of two paths is the claim -- the step-wise kernels for the one-launch rollout.  Tolerances are those of tests/test_ppo_net_gpu.py and
tests/test_ppo_discrete_gpu.py.  Every test prints the error it measured ("PPO-ERR ...", shown with -s) before it asserts."""
import copy
import math
import os
import sys
import types

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_cat_reference as R  # noqa: E402
import test_ppo_discrete_gpu as TD  # noqa: E402
import test_ppo_net_gpu as TN  # noqa: E402
from ppo_net_reference import KINK_MARGIN, kink_margin  # noqa: E402
from test_ppo_gpu import LS_RANGE, _torch_loss  # noqa: E402

pytestmark = pytest.mark.gpu

# (obs, A) of the Normal head; (obs, n) of the categorical head.  The first four of each run every sample count, the others (65, 16 385)
NORMAL = [
    (1, 1),  # every lower bound; w1 row stride 1
    (3, 4),  # Pendulum's width at the largest head
    (8, 1),
    (8, 4),  # every upper bound; the largest parameter count
    (2, 2),
    (7, 3),  # odd everything
]
CATEGORICAL = [
    (1, 2),  # lower bounds
    (4, 4),  # the last logit in the wloc slots
    (4, 5),  # the first logit in the wls slots
    (8, 8),  # upper bounds
    (3, 7),
]
GEOMETRIES = [(0, o, a) for o, a in NORMAL] + [(1, o, n) for o, n in CATEGORICAL]
CORNERS = [(0, o, a) for o, a in NORMAL[:4]] + [(1, o, n) for o, n in CATEGORICAL[:4]]
# a workgroup's 16 rows and its neighbours; 16 385 + 16: the launch's 1 024 workgroups take 16 384 rows per pass of the grid-stride loop -- workgroup 0 takes a
# second pass with a full group, workgroup 1 one with a single row
FORWARD_ROWS = (1, 15, 16, 17, 250, 16385 + 16)
# tiles of 64 samples, at most 256 workgroups: 1, 1, 1, 2, 3, 5 workgroups (k_ppo_reduce: four lanes per parameter, each sums every fourth partial); 16 385:
# workgroup 0 walks two tiles, the second holding one sample; 32 769: two tiles everywhere, three on workgroup 0
SAMPLES = (1, 63, 64, 65, 129, 257, 16385, 32769)
MINIBATCH = [(c, o, a, mb) for c, o, a in GEOMETRIES for mb in (SAMPLES if (c, o, a) in CORNERS else (65, 16385))]
PC, VC, VW, EW = 0.2, 0.2, 0.7, 0.01  # policy clip, value clip, value weight, entropy weight
SENTINEL = 7.0
LARGE = 16385  # sample counts from which a tensor's bar may come from float32 torch autograd's own error (_minibatch_case)


def _gid(case):
    return ("cat" if case[0] else "normal") + "-" + "-".join(str(x) for x in case[1:])


def _head(N, cat):
    lib, p = N.lib(), "srlx_ppo_cat_" if cat else "srlx_ppo_net_"
    fns = {k: getattr(lib, p + k) for k in ("param_count", "partials_floats", "forward", "minibatch", "adam", "rollout_max_horizon")}
    return types.SimpleNamespace(cat=bool(cat), name="categorical" if cat else "normal", net=TD._net if cat else TN._net, **fns)


def _rel(got, want):
    """max |got - want| / max |want| (NaN when a poisoned value came through)"""
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_geometries_outside_the_envelope_are_refused():
    """obs 0 and 9, A 0 and 5, n 1 and 9: the counts answer -1, the launchers a non-OK code (their arguments are checked first: nothing is launched)."""
    N, lib, torch, dev = TN._env()
    buf = torch.zeros(1 << 16, device=dev)
    rows, step = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    p, q, r = N.tptr(buf), N.tptr(rows), N.tptr(step)
    refused = 0
    for cat, bad in ((0, [(0, 1), (9, 1), (3, 0), (3, 5)]), (1, [(0, 2), (9, 2), (4, 1), (4, 9)])):
        h = _head(N, cat)
        for obs, size in bad:
            assert h.param_count(obs, size) == -1 and h.partials_floats(obs, size) == -1, (cat, obs, size)
            head_out = (p,) if cat else (p, p)
            ls = () if cat else LS_RANGE
            codes = (h.forward(16, obs, size, p, p, p, *head_out, None),
                     h.minibatch(16, q, obs, size, p, p, p, p, p, p, p, *ls, 1, 1, PC, 1, VC, VW, EW, p, p, p, None),
                     h.adam(obs, size, p, p, p, p, r, 3e-4, 0.9, 0.999, 1e-8, 0.5, 1.0, None))
            assert all(c != N.OK for c in codes), (cat, obs, size, codes)
            refused += len(codes)
    torch.cuda.synchronize()
    print("PPO-ERR refusals: %d launcher calls refused, buffers untouched: %s" % (refused, bool((buf == 0).all())))
    assert bool((buf == 0).all()) and step.tolist() == [0, 0]


# ---- forward -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GEOMETRIES, ids=_gid)
def test_forward_matches_float64(case):
    """Every output within 1e-5 (relative; absolute: 1e-5 of the tensor's largest entry) of the torch modules in float64 at FORWARD_ROWS; the row past the last one
    (every output is allocated with one guard row) keeps its sentinel.  The categorical entry point takes no log_scale buffer at all."""
    cat, obs, size = case
    N, lib, torch, dev = TN._env()
    h = _head(N, cat)
    net, flat = h.net(torch, dev, obs, size, 1)
    assert h.param_count(obs, size) == flat.numel()
    net64 = copy.deepcopy(net).double()
    g = torch.Generator().manual_seed(100 * obs + 10 * size + cat)
    checks = []
    for n in FORWARD_ROWS:
        x = torch.randn(n, obs, generator=g).to(dev)
        outs = [torch.full((n + 1,), SENTINEL, device=dev)] + [torch.full((n + 1, size), SENTINEL, device=dev) for _ in range(1 if cat else 2)]
        N.check(h.forward(n, obs, size, N.tptr(flat), N.tptr(x), *(N.tptr(t) for t in outs), None))
        torch.cuda.synchronize()
        with torch.no_grad():
            want = net64(x.double())
        for name, got, w in zip(("v", "logits" if cat else "loc", "log_scale"), outs, want):
            checks.append((n, name, got, w, _rel(got[:n].double(), w)))
    print("PPO-ERR forward %s obs=%d size=%d worst %.3g; per row count: %s" % (h.name, obs, size, max(c[4] for c in checks), " ".join(
        "%d:%.2g" % (n, max(c[4] for c in checks if c[0] == n)) for n in FORWARD_ROWS)))
    for n, name, got, w, _ in checks:
        torch.testing.assert_close(got[:n].double(), w, rtol=1e-5, atol=1e-5 * float(w.abs().max()), msg=lambda m: f"{name} at {n} rows: {m}")
        assert bool((got[n:] == SENTINEL).all()), (name, n, "the guard row was written")


# ---- one minibatch: gradients and losses ---------------------------------------------------------------------------------------------------------------------------
def _minibatch_case(cat, obs, size, mb, switches, gate=False):
    """One minibatch of `mb` samples, drawn through a shuffled rows table from buffers three times as long (and never shorter than 192 rows: 1 - 2 % of the rows lie
    at a ReLU kink, so at one sample three candidates would trip the filter's cap once in 25 cases) whose unused rows hold NaN, with a NaN-filled partials buffer;
    for every (base, clip, vclip) of `switches`: every parameter tensor's gradient and the three losses against float64 autograd.
    Tolerance: the project's standing one -- rtol 1e-5, atol 1e-5 of the tensor's largest entry (losses: rtol 1e-4, atol 1e-6).  At the large counts (LARGE and
    above) a tensor's entries can be a sum of tens of thousands of terms that cancels to 1e-5 of the terms' total, and then float32 rounding of the TERMS alone is
    beyond that bar; measured on an MI355X (profiles/ppo_envelope_gputest.log), categorical (obs, n) = (1, 2) at 32 769 samples, switches (0, 0, 0), logits bias
    (two entries, each the other's negative, 1.3e-5 where the terms' magnitudes sum to about 1): the kernel is 8.6e-10 from float64 against 1.3e-10 allowed.
    There -- and only at those counts -- a tensor may be as far from float64 as twice the distance of float32 torch autograd of the same loss on the same rows
    (the slack of tests/test_qnet_pinned.py's `wide` set); that distance is measured from torch, never from the kernel, and printed.
    gate: the log-scale clamp's bounds are the 30th and 70th percentile of the chosen rows' raw log-scales (float64), so the clamp and its gradient gate are active
    below, inside and above; rows with a raw log-scale within 1e-5 of a bound are dropped like the rows at a ReLU kink (which side they fall on is the yardstick's
    precision)."""
    N, lib, torch, dev = TN._env()
    h = _head(N, cat)
    net, flat = h.net(torch, dev, obs, size, 2)
    P = flat.numel()
    assert h.param_count(obs, size) == P
    net64 = copy.deepcopy(net).double()
    total = 3 * max(mb, 64)
    g = torch.Generator().manual_seed(7919 * mb + 64 * obs + 8 * size + cat)  # (a host generator: the same rows on every machine)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    b_obs, b_adv, b_vt = r(total, obs), r(total), r(total)
    b_act = torch.randint(0, size, (total,), generator=g, dtype=torch.int32).to(dev) if cat else r(total, size)
    order = torch.randperm(total, generator=g).to(dev)
    keep = kink_margin(torch, net, b_obs) > KINK_MARGIN
    ls_range, regions = LS_RANGE, None
    if gate:
        with torch.no_grad():
            ls64 = net64(b_obs.double())[2]
        chosen = order[keep[order]][:mb]
        q = torch.quantile(ls64[chosen].reshape(-1), torch.tensor([0.3, 0.7], dtype=torch.float64, device=dev))
        ls_range = tuple(float(t.float()) for t in q)  # (float32 values: the kernel and the yardstick clamp at the same numbers)
        keep &= ((ls64 - ls_range[0]).abs() > 1e-5).all(dim=1) & ((ls64 - ls_range[1]).abs() > 1e-5).all(dim=1)
    kept = int(keep.sum())
    assert 3 * kept > 2 * total, (kept, total)  # the filter keeps more than 2/3 of the candidate rows
    rows = order[keep[order]][:mb].contiguous()
    assert rows.numel() == mb
    if gate:
        ls_rows = ls64[rows]
        regions = [int((ls_rows < ls_range[0]).sum()), int(((ls_rows > ls_range[0]) & (ls_rows < ls_range[1])).sum()), int((ls_rows > ls_range[1]).sum())]
        assert min(regions) > 0, regions
    with torch.no_grad():
        if cat:
            v0, lg0 = net(b_obs)
            b_logp = torch.log_softmax(lg0, dim=-1).gather(1, b_act.long().view(-1, 1)).squeeze(1) + 0.3 * r(total)
        else:
            v0, loc0, ls0 = net(b_obs)
            ls_c = torch.clamp(ls0, ls_range[0], ls_range[1])
            b_logp = -0.5 * math.log(2 * math.pi) - ls_c - 0.5 * ((b_act - loc0) / torch.exp(ls_c)) ** 2 + 0.3 * r(total, size)
        b_val = v0 + 0.3 * r(total)
    b_logp, b_val = b_logp.contiguous(), b_val.contiguous()
    unused = torch.ones(total, dtype=torch.bool, device=dev)
    unused[rows] = False
    for t in (b_obs, b_adv, b_vt, b_val, b_logp):
        t[unused] = float("nan")  # a read of a row the table does not name poisons the result
    act_rows = b_act[rows]

    def loss_parts(model, dt, base, clip, vclip):  # the restated loss through `model` at precision dt
        logp_, adv_, vt_, val_ = (t[rows].to(dt) for t in (b_logp, b_adv, b_vt, b_val))
        if cat:
            v, lg = model(b_obs[rows].to(dt))
            return R.torch_loss(torch, lg, act_rows, logp_, adv_, v, vt_, val_, base, clip, PC, vclip, VC, VW, EW)
        v, loc, ls = model(b_obs[rows].to(dt))
        lsc = torch.clamp(ls, ls_range[0], ls_range[1])
        lp = -0.5 * math.log(2 * math.pi) - lsc - 0.5 * ((act_rows.to(dt) - loc) / torch.exp(lsc)) ** 2
        return _torch_loss(torch, lp, logp_, adv_, v, vt_, val_, base, clip, PC, vclip, VC, VW, EW)

    def grads_of(model, dt, base, clip, vclip):
        model.zero_grad()
        parts = loss_parts(model, dt, base, clip, vclip)
        sum(parts).backward()
        return torch.stack([p.detach() for p in parts]), [(name, p.grad.reshape(-1).double().clone()) for name, p in model.named_parameters()]

    partials = torch.empty(h.partials_floats(obs, size), device=dev)
    for base, clip, vclip in switches:
        partials.fill_(float("nan"))  # a reduce that reads a partial no workgroup wrote poisons the gradient
        grad, losses = torch.full((P,), float("nan"), device=dev), torch.full((3,), float("nan"), device=dev)
        ls_args = () if cat else ls_range
        N.check(h.minibatch(mb, N.tptr(rows), obs, size, N.tptr(flat), N.tptr(b_obs), N.tptr(b_act), N.tptr(b_logp), N.tptr(b_adv), N.tptr(b_vt), N.tptr(b_val), *ls_args,
                            base, clip, PC, vclip, VC, VW, EW, N.tptr(partials), N.tptr(grad), N.tptr(losses), None))
        torch.cuda.synchronize()
        want_losses, want_grads = grads_of(net64, torch.float64, base, clip, vclip)
        torch32 = [0.0] * len(want_grads)  # float32 torch autograd's own distance from float64, per tensor (large counts only)
        if mb >= LARGE:
            torch32 = [float((g32 - w).abs().max()) for (_, g32), (_, w) in zip(grads_of(net, torch.float32, base, clip, vclip)[1], want_grads)]
        off, tensors = 0, []
        for (name, want), t32 in zip(want_grads, torch32):
            got = grad[off : off + want.numel()].double()
            off += want.numel()
            tensors.append((name, got, want, _rel(got, want), t32))
        assert off == P
        worst = max(tensors, key=lambda t: t[3] if t[3] == t[3] else float("inf"))
        loss_err = float(((losses.double() - want_losses).abs() / want_losses.abs().clamp_min(1e-30)).max())
        print("PPO-ERR minibatch %s obs=%d size=%d mb=%d switches=%d%d%d%s kept %d/%d grad %.3g (%s) losses %.3g" % (
            h.name, obs, size, mb, base, clip, vclip, " clamp %s regions %s" % (ls_range, regions) if gate else "", kept, total, worst[3], worst[0], loss_err))
        for name, got, want, _, t32 in tensors:
            standing = 1e-5 * float(want.abs().max()) + 1e-12
            if 2 * t32 > standing:
                print("PPO-ERR   float32 torch autograd itself: %s |f32 - f64| %.3g, kernel |got - f64| %.3g, standing atol %.3g -> allowed %.3g" % (
                    name, t32, float((got - want).abs().max()), standing, 2 * t32))
        torch.testing.assert_close(losses.double(), want_losses, rtol=1e-4, atol=1e-6)
        for name, got, want, _, t32 in tensors:
            torch.testing.assert_close(got, want, rtol=1e-5, atol=max(1e-5 * float(want.abs().max()) + 1e-12, 2 * t32), msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("case", MINIBATCH, ids=_gid)
def test_minibatch_gradients_match_float64_autograd(case):
    """Loss switches (base, clip, vclip) = (1,1,1) and (0,0,0) at every count; (0,1,0) and (1,0,1) as well at 65 samples."""
    cat, obs, size, mb = case
    _minibatch_case(cat, obs, size, mb, [(1, 1, 1), (0, 0, 0)] + ([(0, 1, 0), (1, 0, 1)] if mb == 65 else []))


@pytest.mark.parametrize("obs,A,mb", [(3, 4, 65), (3, 4, 2000), (8, 1, 65), (8, 1, 2000)])
def test_log_scale_clamp_gates_its_gradient(obs, A, mb):
    """policy_normal's `pass ? ... : 0`: with the clamp's bounds inside the log-scales' spread (about 30 % of the entries below, 40 % inside, 30 % above), the
    float64 yardstick is torch.clamp inside the autograd graph; the stored log-probabilities are built with the same clamp."""
    _minibatch_case(0, obs, A, mb, [(1, 1, 1), (0, 0, 0)], gate=True)


# ---- clip + Adam ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("clip", ["active", "slack", "off"])
@pytest.mark.parametrize("cat,obs,size,P,wgs", [(0, 1, 1, 12803, 13), (0, 8, 4, 13641, 14), (1, 1, 2, 12803, 13), (1, 8, 8, 13641, 14)])
def test_clip_and_adam_five_steps(cat, obs, size, P, wgs, clip, scale):
    """Five consecutive steps on one state (k_ppo_adam: 1 024 parameters per workgroup, the last one partial) against torch.nn.utils.clip_grad_norm_ +
    torch.optim.Adam in float32: the clip active (max_grad_norm far below the norm), present but not biting (10 x the largest norm of the five gradients), and
    absent (max_grad_norm = 0: the torch side skips it); grad_scale 1 and 0.5 (the data-parallel mean).  The step counter advances, the arrival counter is back at
    zero after every step, and `grad` is left as it was."""
    N, lib, torch, dev = TN._env()
    h = _head(N, cat)
    net, flat = h.net(torch, dev, obs, size, 3)
    assert h.param_count(obs, size) == flat.numel() == P and (P + 1023) // 1024 == wgs
    g = torch.Generator().manual_seed(P + 10 * cat)
    g0, g1 = (1e-2 * torch.randn(P, generator=g)).to(dev), (1e-2 * torch.randn(P, generator=g)).to(dev)
    grads = [(g0 * (1.0 + k) + g1 * k).contiguous() for k in range(5)]
    norms = [float((gk.double() * scale).norm()) for gk in grads]
    max_norm = {"active": 0.01, "slack": 10.0 * max(norms), "off": 0.0}[clip]
    lr = 3e-4
    ref = flat.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=lr)
    mine = flat.clone()
    m, v2, step = torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    errs = []
    for k, gk in enumerate(grads):
        ref.grad = gk.clone() * scale
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
            assert norm > 10 * max_norm if clip == "active" else norm < max_norm, (norm, max_norm)
        opt.step()
        before = gk.clone()
        N.check(h.adam(obs, size, N.tptr(mine), N.tptr(gk), N.tptr(m), N.tptr(v2), N.tptr(step), lr, 0.9, 0.999, 1e-8, max_norm, scale, None))
        torch.cuda.synchronize()
        errs.append(float((mine - ref.detach()).abs().max()))
        assert step.tolist() == [k + 1, 0]
        assert torch.equal(gk, before)  # (every workgroup reads all of it for the norm; the data-parallel path reads it again)
    moved = float((mine - flat).abs().max())
    print("PPO-ERR adam %s obs=%d size=%d P=%d clip=%s (%.4g, norms %.4g..%.4g) grad_scale=%.1f max |mine - torch| per step %s, moved %.3g" % (
        h.name, obs, size, P, clip, max_norm, min(norms), max(norms), scale, " ".join("%.2g" % e for e in errs), moved))
    assert moved > lr  # five steps of about lr each
    torch.testing.assert_close(mine, ref.detach(), rtol=3e-7, atol=lr * 2e-5)  # (an ulp of the parameter, or 2e-5 of the step)
    assert step.tolist() == [5, 0]


# ---- the one-launch rollout, bit for bit against the step-wise kernels --------------------------------------------------------------------------------------------
def _cfg(cat, size, E, T, episode_len, seed=4):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig

    head = dict(obs_dim=4, n_actions=size) if cat else dict(action_dim=size)
    return PPODeviceConfig(n_envs=E, horizon=T, seed=seed, episode_len=episode_len, **head)


def _rollouts_agree(cfg, rollouts=2):
    """Two engines from one configuration, one on k_ppo_rollout, the other on the launches it fuses (network forward -> act -> environment step per step, then
    srlx_gae_scan): every buffer, the environments' state and counters, V(s_T) and the running episode returns are the same bits after each of `rollouts`
    consecutive rollouts; the finished episodes' sum to the float atomics' order.  Returns the fused engine."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    a, b = PPOEngine(cfg, 0), PPOEngine(cfg, 0)
    if a.cat:
        TD._give_the_logits_content(torch, a, b)
    assert torch.equal(a.flat, b.flat) and a.fused and b.fused and a._fused_rollout_ok()
    b._fused_rollout_ok = lambda: False  # the step-wise path on the libsrlx network
    T, ends = cfg.horizon, 0
    for it in range(rollouts):
        a.rollout()
        b.rollout()
        torch.cuda.synchronize()
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "episode_return"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
        assert torch.equal(a._last_v, b._last_v) and torch.equal(a.env.state, b.env.state) and torch.equal(a.env.t, b.env.t), it
        if a.cat:
            assert torch.equal(a.env.episodes, b.env.episodes), it
        else:
            assert int(a.env.counter.item()) == int(b.env.counter.item()) == T * (it + 1)
        assert int(a.act_counter.item()) == int(b.act_counter.item()) == T * (it + 1)
        ends += int(a.b_done.sum())
        assert float(a.finished_returns[1]) == float(b.finished_returns[1]) == float(ends)
        torch.testing.assert_close(a.finished_returns, b.finished_returns, rtol=1e-5, atol=1e-3)  # (float atomics: order differs)
        assert bool(torch.isfinite(a.b_adv).all()) and float(a.b_logp.max() - a.b_logp.min()) > 0
        for e in (a, b):
            e.b_obs[0].copy_(e.b_obs[T])  # (the step-wise path starts from b_obs[0], the fused one from env.obs)
    assert torch.equal(a.env.obs, a.b_obs[T])
    print("PPO-ERR rollout %s size=%d E=%d T=%d episode_len=%d: %d rollouts bit-equal; %d episode ends, finished sums differ by %.3g" % (
        a.head.__class__.__name__, a.head.size, cfg.n_envs, T, cfg.episode_len, rollouts, ends, float((a.finished_returns[0] - b.finished_returns[0]).abs())))
    return a, ends


@pytest.mark.parametrize("episode_len", [24, 1000])
@pytest.mark.parametrize("E", [16, 48])
@pytest.mark.parametrize("A", [2, 4])
def test_pendulum_rollout_with_several_action_dimensions(A, E, episode_len):
    """k_ppo_rollout<PendulumNormal> with A > 1 (zbuf [T][16][A], b_act / b_logp [T][E][A]) at one and three workgroups.  episode_len 24 = T: every episode ends
    exactly on the last step, so no lane bootstraps from V(s_T); episode_len 1000: no episode ends, every lane does."""
    _, _, torch, _ = TN._env()
    a, ends = _rollouts_agree(_cfg(0, A, E, 24, episode_len))
    assert a.b_act.shape == (24, E, A) and not torch.equal(a.b_act[..., 0], a.b_act[..., 1])
    if episode_len == 24:
        assert ends == 2 * E and bool(a.b_done[-1].all()) and int(a.b_done[:-1].sum()) == 0
        assert torch.equal(a.b_adv[-1], a.b_rew[-1] - a.b_val[-1])  # (no bootstrap: delta = r - V(s))
    else:
        assert ends == 0
        torch.testing.assert_close(a.b_adv[-1], (a.b_rew[-1] + 0.9 * a._last_v) - a.b_val[-1], rtol=1e-6, atol=1e-6)  # (delta = r + discount V(s_T) - V(s))
        assert float(a._last_v.abs().min()) > 0


@pytest.mark.parametrize("episode_len", [24, 11])
@pytest.mark.parametrize("E", [16, 48])
@pytest.mark.parametrize("n", [3, 5, 8])
def test_cartpole_rollout_with_more_than_two_actions(n, E, episode_len):
    """k_ppo_rollout<CartPoleCategorical> with n > 2 actions (the logits given content; 5 and 8: logit rows in the wls slots) at one and three workgroups;
    episode_len 24 = T: a lane that survives is truncated exactly on the last step; 11: every lane ends an episode inside the rollout."""
    _, _, torch, _ = TN._env()
    a, ends = _rollouts_agree(_cfg(1, n, E, 24, episode_len))
    assert a.b_act.shape == (24, E) and int(a.b_act.max()) > 1 and int(a.b_act.min()) == 0 and ends >= 2 * E * (24 // episode_len)
    assert float(a.b_logp.max() - a.b_logp.min()) > 0.5  # (a uniform policy would have every entry at log 1/n)


@pytest.mark.parametrize("cat,size", [(0, 3), (1, 7)])
def test_rollout_of_one_step(cat, size):
    """T = 1 at one workgroup: the only step is the last one (the GAE scan's bootstrap branch, record tables of one row)."""
    a, _ = _rollouts_agree(_cfg(cat, size, 16, 1, 11), rollouts=3)
    assert a.b_adv.shape == (1, 16)


# sizeof(FwdLds) = 4 * (3 * 64 * 64 weights + 1 356 small tensors + 16 * 8 inputs + 4 * 16 * 65 activations + 16 * 9 heads) = 72 304 bytes of the workgroup's 160 KiB;
# a step takes 16 environments * 4 bytes * (3 records + A draws; categorical: 3 records): (163 840 - 72 304) // 256 = 357, // 448 = 204, // 192 = 476
MAX_HORIZON = {(0, 1): 357, (0, 4): 204, (1, 2): 476, (1, 8): 476}


@pytest.mark.parametrize("cat,size", sorted(MAX_HORIZON), ids=lambda v: str(v))
def test_rollout_at_the_longest_horizon_and_refusal_beyond(cat, size):
    """T = srlx_ppo_*_rollout_max_horizon exactly (the LDS edge: the last step's records end at most one step's worth below 160 KiB) at one workgroup; T + 1 makes the
    engine take the step-wise path, and the library refuses the direct call with its horizon text before launching anything."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    h = _head(N, cat)
    T = h.rollout_max_horizon(size)
    assert T == MAX_HORIZON[(cat, size)]
    _rollouts_agree(_cfg(cat, size, 16, T, 11))
    over = PPOEngine(_cfg(cat, size, 16, T + 1, 11), 0)
    assert over.fused and not over._fused_rollout_ok()
    with pytest.raises(N.SrlxError, match="horizon"):
        over.head.rollout(over)
    torch.cuda.synchronize()
    assert int(over.act_counter.item()) == 0 and float(over.b_val.abs().max()) == 0 and float(over.finished_returns.abs().max()) == 0
