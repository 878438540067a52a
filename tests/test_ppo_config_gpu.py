"""GPU tests of what a ppo.Config asks of the PPO device engine beyond the network (csrc/srlx_ppo_net.hip, srlx_lr_math.h, device/ppo.py, device/vector_runner.py):
the learning-rate schedule evaluated inside k_ppo_adam (against torch.optim.Adam under a LambdaLR of `LRSchedulerConfig.factor`; through a captured update graph),
the batch baselines of the advantage (`srlx_ppo_adv_baseline` against float64 numpy; the fused engine against the torch-ops engine), reward clip / state clip /
action rescale inside the one-launch rollout (bit for bit against the step-wise path), and `ppo_config_from(ppo.Config(), ...)` end to end on both built-in
environments.  Bars: those of the tests whose fixtures these reuse (tests/test_ppo_envelope_gpu.py, tests/test_ppo_net_gpu.py) and the project's standing
float32 tolerance of 1e-5 (relative; absolute against a tensor's largest entry).  Every test prints what it measured ("PPO-CFG ...", shown with -s) before it
asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ppo_discrete_gpu as TD  # noqa: E402
import test_ppo_envelope_gpu as TE  # noqa: E402
import test_ppo_net_gpu as TN  # noqa: E402

pytestmark = pytest.mark.gpu

LR = 3e-4  # (test_clip_and_adam_five_steps)


def _schedules():
    from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig as S

    return {"step": S().set_step(2, 0.5), "exp": S().set_exp(3, 0.1), "cosine": S().set_cosine(4, 1e-5), "piecewise": S().set_piecewise([2, 4], [1e-3, 5e-4, 1e-4])}


def _sched_head(N, cat):
    h = TE._head(N, cat)
    h.adam_sched = getattr(N.lib(), ("srlx_ppo_cat_" if cat else "srlx_ppo_net_") + "adam_sched")
    return h


def _adam_fixture(N, torch, dev, cat, obs, size, P, wgs, steps):
    """The state and gradients of test_clip_and_adam_five_steps (tests/test_ppo_envelope_gpu.py), `steps` of them."""
    h = _sched_head(N, cat)
    net, flat = h.net(torch, dev, obs, size, 3)
    assert h.param_count(obs, size) == flat.numel() == P and (P + 1023) // 1024 == wgs
    g = torch.Generator().manual_seed(P + 10 * cat)
    g0, g1 = (1e-2 * torch.randn(P, generator=g)).to(dev), (1e-2 * torch.randn(P, generator=g)).to(dev)
    return h, flat, [(g0 * (1.0 + k) + g1 * k).contiguous() for k in range(steps)]


ADAM_GEOMETRIES = [(0, 1, 1, 12803, 13), (0, 8, 4, 13641, 14), (1, 1, 2, 12803, 13), (1, 8, 8, 13641, 14)]


# ---- the schedule inside k_ppo_adam ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["step", "exp", "cosine", "piecewise"])
@pytest.mark.parametrize("clip", ["active", "off"])
@pytest.mark.parametrize("cat,obs,size,P,wgs", ADAM_GEOMETRIES)
def test_scheduled_adam_seven_steps(cat, obs, size, P, wgs, clip, kind):
    """Seven consecutive steps through srlx_ppo_*_adam_sched against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam + LambdaLR(LRSchedulerConfig.factor): optimiser
    step k (0-based) runs at lr * factor(k), read by the kernel from its own step counter.  Each step starts from the torch side's parameters and moments (the bar
    is a fraction of THAT step, and the steps shrink by orders of magnitude: an earlier step's rounding must not be charged to a later one) and is held to that
    test's bar: rtol 3e-7 (an ulp of the parameter) plus 2e-5 of the scheduled step, lr * factor(k)."""
    N, lib, torch, dev = TN._env()
    h, flat, grads = _adam_fixture(N, torch, dev, cat, obs, size, P, wgs, 7)
    cfg = _schedules()[kind]
    sched = N.lr_schedule(cfg)
    max_norm = {"active": 0.01, "off": 0.0}[clip]
    ref = flat.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=LR)
    lam = cfg.apply_torch_scheduler(opt)
    mine, m, v2, step = flat.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    factors, errs, bars, close = [cfg.factor(k, LR) for k in range(7)], [], [], []
    assert len(set(factors)) >= 3  # (the schedule moves inside the seven steps)
    for k, gk in enumerate(grads):
        if k:
            mine.copy_(ref.detach()), m.copy_(opt.state[ref]["exp_avg"]), v2.copy_(opt.state[ref]["exp_avg_sq"])
        before = ref.detach().clone()
        ref.grad = gk.clone()
        if max_norm > 0:
            assert float(torch.nn.utils.clip_grad_norm_([ref], max_norm)) > 10 * max_norm
        assert abs(opt.param_groups[0]["lr"] - LR * factors[k]) <= 1e-15
        opt.step()
        lam.step()
        N.check(h.adam_sched(obs, size, N.tptr(mine), N.tptr(gk), N.tptr(m), N.tptr(v2), N.tptr(step), LR, ctypes.byref(sched), 0.9, 0.999, 1e-8, max_norm, 1.0, None))
        torch.cuda.synchronize()
        assert step.tolist() == [k + 1, 0]
        errs.append(float((mine - ref.detach()).abs().max()))
        bars.append(LR * factors[k] * 2e-5)
        close.append(bool(torch.isclose(mine, ref.detach(), rtol=3e-7, atol=bars[k]).all()))
        moved = float((ref.detach() - before).abs().max())
        # (the yardstick follows the schedule: an Adam step is about its rate, at most (1 - beta1) / sqrt(1 - beta2) = 3.2 times it)
        assert 0.5 * LR * factors[k] < moved < 3.5 * LR * factors[k], (k, moved)
    print("PPO-CFG adam_sched %s obs=%d size=%d P=%d clip=%s %s: factors %s; max |mine - torch| per step %s; 2e-5 of the step %s" % (
        h.name, obs, size, P, clip, kind, " ".join("%.3g" % f for f in factors), " ".join("%.2g" % e for e in errs), " ".join("%.2g" % b for b in bars)))
    assert all(close), close  # every step: |mine - torch| <= 2e-5 of the step + 3e-7 |torch|, element by element
    torch.testing.assert_close(mine, ref.detach(), rtol=3e-7, atol=bars[6])


@pytest.mark.parametrize("cat,obs,size,P,wgs", ADAM_GEOMETRIES)
def test_constant_schedule_is_the_plain_entry_point(cat, obs, size, P, wgs):
    """srlx_ppo_*_adam_sched under a constant schedule and srlx_ppo_*_adam: the same kernel, the same bits -- parameters and both moments after three steps, with the
    clip active and a data-parallel grad_scale."""
    from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig

    N, lib, torch, dev = TN._env()
    h, flat, grads = _adam_fixture(N, torch, dev, cat, obs, size, P, wgs, 3)
    sched = N.lr_schedule(LRSchedulerConfig())
    states = []
    for scheduled in (False, True):
        p, m, v2, step = flat.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        for gk in grads:
            head = (obs, size, N.tptr(p), N.tptr(gk), N.tptr(m), N.tptr(v2), N.tptr(step), LR)
            tail = (0.9, 0.999, 1e-8, 0.01, 0.5, None)
            N.check(h.adam_sched(*head, ctypes.byref(sched), *tail) if scheduled else h.adam(*head, *tail))
        torch.cuda.synchronize()
        states.append((p, m, v2, step))
    for a, b in zip(*states):
        assert torch.equal(a, b)
    assert states[0][3].tolist() == [3, 0] and float((states[0][0] - flat).abs().max()) > LR
    bad = N.lr_schedule(LRSchedulerConfig().set_step(2, 0.5))
    bad.decay_steps = 0
    p, m, v2, step = states[0]
    assert h.adam_sched(obs, size, N.tptr(p), N.tptr(grads[0]), N.tptr(m), N.tptr(v2), N.tptr(step), LR, ctypes.byref(bad), 0.9, 0.999, 1e-8, 0.0, 1.0, None) != 0
    assert b"schedule" in lib.srlx_last_error()


def _small_engine(torch, schedule, graphs, iterations=4, **kw):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    eng = PPOEngine(PPODeviceConfig(n_envs=64, horizon=8, epochs=1, minibatches=2, seed=11, lr_scheduler=schedule, **kw), 0)
    assert eng.fused and eng._fused_rollout_ok()
    snapshots = []
    for k in range(iterations):
        if k == 1 and graphs:
            eng.capture_graphs()  # (runs one whole iteration itself, as its warm-up)
        else:
            eng.step()
        torch.cuda.synchronize()
        snapshots.append(eng.flat.clone())
    return eng, snapshots


def test_the_schedule_survives_graph_capture():
    """set_step(3, 0.1) on E = 64, T = 8, one epoch of two minibatches (two optimiser steps per iteration): the engine that replays its captured update graph and the
    eager one hold the same bits after four iterations -- the rate is computed inside the launch from `opt_step[0]`, nothing of it is baked into the graph.  Against
    a constant-rate engine the parameters are the same after the first iteration (updates 0, 1) and differ after the second (update 3, the fourth, is the first at
    0.1 lr); under set_step(4, 0.1) the second iteration is still the constant engine's."""
    from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig as S

    N, lib, torch, dev = TN._env()
    eager, se = _small_engine(torch, S().set_step(3, 0.1), False)
    graph, sg = _small_engine(torch, S().set_step(3, 0.1), True)
    assert graph._update_graph is not None and eager._update_graph is None
    const, sc = _small_engine(torch, S(), False)
    later, sl = _small_engine(torch, S().set_step(4, 0.1), False, iterations=3)
    print("PPO-CFG graph capture: max |eager - graph| %.3g; |scheduled - constant| per iteration %s; |set_step(4) - constant| %s" % (
        float((eager.flat - graph.flat).abs().max()), " ".join("%.3g" % float((a - b).abs().max()) for a, b in zip(se, sc)),
        " ".join("%.3g" % float((a - b).abs().max()) for a, b in zip(sl, sc))))
    for a, b in zip(se, sg):
        assert torch.equal(a, b)
    assert torch.equal(eager.opt_step, graph.opt_step) and eager.opt_step.tolist() == [8, 0]
    assert torch.equal(eager.exp_avg, graph.exp_avg) and torch.equal(eager.exp_avg_sq, graph.exp_avg_sq) and torch.equal(eager.b_adv, graph.b_adv)
    assert torch.equal(se[0], sc[0]) and all(not torch.equal(a, b) for a, b in zip(se[1:], sc[1:]))
    assert torch.equal(sl[0], sc[0]) and torch.equal(sl[1], sc[1]) and not torch.equal(sl[2], sc[2])
    assert bool(torch.isfinite(graph.flat).all())


def test_torch_path_follows_the_schedule_through_a_lambda_lr():
    """fused=False applies `apply_torch_scheduler` to its Adam, as the plugin's trainer does: one update() of 16 optimiser steps under set_step(8, 0.1) from identical
    buffers, the fused engine against it at the bar of test_fused_engine_against_the_autograd_engine (tests/test_ppo_net_gpu.py); the same update at a constant
    rate moves the parameters about 16 / 8.8 times as far."""
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine
    from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig as S

    N, lib, torch, dev = TN._env()
    make = lambda sched, fused: PPOEngine(PPODeviceConfig(n_envs=512, horizon=16, seed=6, lr_scheduler=sched), 0, fused=fused)  # noqa: E731
    a, b, const = make(S().set_step(8, 0.1), True), make(S().set_step(8, 0.1), False), make(S(), True)
    assert b.lr_sch is not None and const.scheduled is False and a.scheduled
    a.rollout()
    torch.cuda.synchronize()
    for e in (b, const):
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv"):
            getattr(e, name).copy_(getattr(a, name))
    before = a.flat.clone()
    for e in (a, b, const):
        e.update()
    torch.cuda.synchronize()
    moved, moved_const = float((a.flat - before).abs().max()), float((const.flat - before).abs().max())
    flat_b = torch.cat([p.detach().reshape(-1) for p in b.net.parameters()])
    diff = (a.flat - flat_b).abs()
    print("PPO-CFG torch path schedule: moved %.3g (constant rate: %.3g), fused - torch max %.3g mean %.3g, torch lr now %.3g" % (
        moved, moved_const, float(diff.max()), float(diff.mean()), b.opt.param_groups[0]["lr"]))
    assert abs(b.opt.param_groups[0]["lr"] - 2e-4 * 0.1 ** 2) < 1e-15  # (16 steps taken: the next one is the third stair)
    assert float(diff.max()) < 0.03 * moved and float(diff.mean()) < 2e-4 * moved, (float(diff.max()), float(diff.mean()), moved)
    assert 1.3 * moved < moved_const < 2.5 * moved
    with pytest.raises(ValueError, match="capture_graphs"):
        b.capture_graphs()


# ---- baselines ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [1, 2, 255, 256, 257, 1025, 32768, 33793])  # (32 768: all of it staged in LDS; 33 793: 1 025 elements beyond the stage)
def test_adv_baseline_against_float64_numpy(mb):
    """srlx_ppo_adv_baseline over `mb` rows that are a shuffled subset of a larger buffer whose other entries are NaN (a read outside `rows` poisons the statistics,
    a write outside them is seen), advantages 100 + 1e-2 N(0, 1) (mean >> spread: a one-pass variance in float32 would cancel): "ave", "std" and "normal" against
    float64 numpy on the same float32 inputs at rtol 1e-5 / atol 1e-5 of the largest entry; two runs give the same bits; one sample under "normal" is exactly 0."""
    N, lib, torch, dev = TN._env()
    total = 2 * mb + 5
    g = torch.Generator().manual_seed(mb)
    rows = torch.randperm(total, generator=g)[:mb].contiguous()
    vals = (100.0 + 1e-2 * torch.randn(mb, generator=g)).float()
    adv = torch.full((total,), float("nan"))
    adv[rows] = vals
    adv_d, rows_d = adv.to(dev), rows.to(dev)
    x = vals.double().numpy()
    mean, sd = x.mean(), x.std() + 1e-8
    want = {"ave": x - mean, "std": x / sd, "normal": (x - mean) / sd}
    outside = torch.ones(total, dtype=torch.bool)
    outside[rows] = False
    for name, mode in N.PPO_BASELINE_MODES.items():
        outs = []
        for _ in range(2):
            out = torch.full((total,), float("nan"), device=dev)
            N.check(lib.srlx_ppo_adv_baseline(mb, N.tptr(rows_d), N.tptr(adv_d), mode, N.tptr(out), None))
            torch.cuda.synchronize()
            outs.append(out.cpu())
        got = outs[0][rows].double().numpy()
        top = float(np.abs(want[name]).max())
        err = float(np.abs(got - want[name]).max())
        print("PPO-CFG adv_baseline mb=%d %s: max |got - float64| %.3g, largest entry %.3g" % (mb, name, err, top))
        assert bool(torch.isnan(outs[0][outside]).all()), name  # (nothing written outside `rows`)
        assert torch.equal(outs[0][rows], outs[1][rows]), name
        np.testing.assert_allclose(got, want[name], rtol=1e-5, atol=1e-5 * top, err_msg=name)
        if mb == 1 and name == "normal":
            assert float(outs[0][rows][0]) == 0.0
    assert torch.equal(adv_d.cpu()[rows], vals)  # (the advantages themselves are untouched: v_target keeps reading them)
    assert lib.srlx_ppo_adv_baseline(mb, N.tptr(rows_d), N.tptr(adv_d), 4, N.tptr(out), None) != 0
    assert lib.srlx_ppo_adv_baseline(mb, N.tptr(rows_d), N.tptr(adv_d), 1, N.tptr(adv_d), None) != 0


@pytest.mark.parametrize("cat", [0, 1], ids=["normal-head", "categorical-head"])
@pytest.mark.parametrize("baseline", ["ave", "std", "normal"])
def test_engine_baselines_fused_against_torch(baseline, cat):
    """One update() (4 epochs x 4 minibatches) of the fused engine -- srlx_ppo_adv_baseline in front of every minibatch launch -- against the fused=False engine, which
    transforms each minibatch's advantages with torch ops, from identical buffers, at the bar of test_fused_engine_against_the_autograd_engine
    (tests/test_ppo_net_gpu.py): difference below 3 % of the movement at its largest and 2e-4 of it on average, losses within 1e-3.  And the baseline is really
    applied: the same update under baseline_type "none" ends elsewhere."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=2) if cat else {}
    make = lambda bt, fused: PPOEngine(PPODeviceConfig(n_envs=512, horizon=16, seed=6, baseline_type=bt, **head), 0, fused=fused)  # noqa: E731
    a, b, none = make(baseline, True), make(baseline, False), make("none", True)
    if cat:
        TD._give_the_logits_content(torch, a, b, none)
    assert a.b_adv_base is not None and none.b_adv_base is None and a.baseline == baseline
    a.rollout()
    torch.cuda.synchronize()
    for e in (b, none):
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv"):
            getattr(e, name).copy_(getattr(a, name))
    before, adv = a.flat.clone(), a.b_adv.clone()
    for e in (a, b, none):
        e.update()
    torch.cuda.synchronize()
    assert torch.equal(a.b_adv, adv)  # (the value target's advantages are untouched)
    moved = float((a.flat - before).abs().max())
    flat_b = torch.cat([p.detach().reshape(-1) for p in b.net.parameters()])
    diff = (a.flat - flat_b).abs()
    apart = float((a.flat - none.flat).abs().max())
    print("PPO-CFG engine baseline %s cat=%d: moved %.3g, fused - torch max %.3g mean %.3g, losses %s vs %s; against baseline none %.3g" % (
        baseline, cat, moved, float(diff.max()), float(diff.mean()), a.losses.tolist(), b.losses.tolist(), apart))
    assert moved > 1e-3
    assert float(diff.max()) < 0.03 * moved and float(diff.mean()) < 2e-4 * moved, (float(diff.max()), float(diff.mean()), moved)
    torch.testing.assert_close(a.losses, b.losses, rtol=1e-3, atol=1e-5)
    assert a.opt_step.tolist() == [16, 0]
    assert apart > 0.0


def test_baseline_aliases_and_unknown_types():
    """"v" is "advantage" (the same launches: the same bits after an iteration), "" is "none"; an unknown string raises where it used to mean "none"."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    def run(bt):
        eng = PPOEngine(PPODeviceConfig(n_envs=64, horizon=8, epochs=1, minibatches=2, seed=3, baseline_type=bt), 0)
        eng.step()
        torch.cuda.synchronize()
        return eng.flat.clone()

    adv, v, none, empty = run("advantage"), run("v"), run("none"), run("")
    assert torch.equal(adv, v) and torch.equal(none, empty) and not torch.equal(adv, none)
    for bad in ("median", "Advantage"):
        with pytest.raises(ValueError, match="baseline_type"):
            PPOEngine(PPODeviceConfig(n_envs=64, baseline_type=bad), 0)


# ---- the rollout's options -------------------------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("E", [16, 48])
def test_cartpole_rollout_with_reward_and_state_clip(E, T):
    """k_ppo_rollout<CartPoleCategorical> with reward_clip (0, 0.5) and state_clip (-0.03, 0.03) against the step-wise path (torch clamps around the step-wise
    kernels): every buffer, the environments and the bookkeeping bit for bit over two rollouts (tests/test_ppo_envelope_gpu.py: _rollouts_agree).  The first
    observation row is clipped like every other; the buffers hold the clipped reward; episode_return and the finished episodes' sum count the raw one; the
    environment's float64 state is not clipped."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig

    cfg = PPODeviceConfig(n_envs=E, horizon=T, seed=4, episode_len=5, obs_dim=4, n_actions=2, reward_clip=(0, 0.5), state_clip=(-0.03, 0.03))
    a, ends = TE._rollouts_agree(cfg, rollouts=2)
    assert a.env_opts is not None
    lo, hi = _f32(-0.03), _f32(0.03)
    assert float(a.b_obs.min()) == lo and float(a.b_obs.max()) == hi  # (some entry sits on either bound)
    # (row 0 of each rollout was compared inside _rollouts_agree: the step-wise path clamps it with torch; the initial draw is U(-0.05, 0.05))
    assert float(a.env.state.abs().max()) > 0.03
    assert bool((a.b_rew == 0.5).all())
    steps = 2 * T
    assert ends == E * (steps // 5)
    assert float(a.finished_returns[0]) == 5.0 * ends  # raw rewards of 1: five per finished episode, not 2.5
    assert bool((a.episode_return == float(steps % 5)).all())
    print("PPO-CFG cartpole options E=%d T=%d: %d episode ends, finished sum %.1f, |state| max %.3g, obs in [%.3g, %.3g]" % (
        E, T, ends, float(a.finished_returns[0]), float(a.env.state.abs().max()), float(a.b_obs.min()), float(a.b_obs.max())))


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("E", [16, 48])
def test_pendulum_rollout_with_action_rescale_and_clips(E, T):
    """k_ppo_rollout<PendulumNormal> with action_scale 2, reward_clip (-1, 0) and state_clip (-0.5, 0.5) against the step-wise path, bit for bit; then the rollout is
    replayed by hand on a fresh environment: fed 2 x the stored action it ends in the engine's state (the stored action is the policy's own, the environment saw
    twice it), its raw rewards and observations clamp to the buffers', and fed the stored action itself it ends elsewhere."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PendulumVecEnv, PPODeviceConfig

    cfg = PPODeviceConfig(n_envs=E, horizon=T, seed=4, episode_len=5, action_scale=2.0, reward_clip=(-1, 0), state_clip=(-0.5, 0.5))
    a, ends = TE._rollouts_agree(cfg, rollouts=1)
    assert a.env_opts is not None and a.rescale and ends == E * (T // 5)

    def replay(scale):
        env = PendulumVecEnv(E, 5, cfg.seed, dev)
        obs, rew, done = torch.empty((T, E, 3), device=dev), torch.empty((T, E), device=dev), torch.empty((T, E), dtype=torch.uint8, device=dev)
        for t in range(T):
            env.step((a.b_act[t, :, 0] * scale).contiguous(), obs[t], rew[t], done[t])
        torch.cuda.synchronize()
        return env, obs, rew, done

    env, obs, rew, done = replay(2.0)
    assert torch.equal(env.state, a.env.state) and torch.equal(env.t, a.env.t) and torch.equal(done, a.b_done)
    assert torch.equal(rew.clamp(-1.0, 0.0), a.b_rew) and float(rew.min()) < -1.0
    assert torch.equal(obs.clamp(-0.5, 0.5), a.b_obs[1:]) and float(obs.abs().max()) > 0.5
    assert float(a.b_obs.abs().max()) == 0.5 and float(PendulumVecEnv(E, 5, cfg.seed, dev).obs.abs().max()) > 0.5  # (the first row was compared inside _rollouts_agree)
    assert not torch.equal(replay(1.0)[0].state, a.env.state)
    raw_return = float(rew.sum())
    got = float(a.finished_returns[0] + a.episode_return.sum())
    print("PPO-CFG pendulum options E=%d T=%d: raw reward sum %.6g, engine's returns %.6g, clipped buffer sum %.6g" % (E, T, raw_return, got, float(a.b_rew.sum())))
    # (float32 sums of at most 384 negative terms in two orders: at most 384 x 6e-8 = 2.3e-5 relative apart)
    assert abs(got - raw_return) <= 5e-5 * abs(raw_return) and float(a.b_rew.sum()) > raw_return + 1.0


@pytest.mark.parametrize("cat", [0, 1], ids=["normal-head", "categorical-head"])
def test_ex_entry_points_with_everything_off_are_the_plain_ones(cat):
    """srlx_ppo_*_rollout_ex with an all-off srlx_ppo_env_opts_t against srlx_ppo_*_rollout: the same bits in every buffer over two rollouts at three workgroups."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=3) if cat else dict(action_dim=2)
    cfg = PPODeviceConfig(n_envs=48, horizon=8, seed=4, episode_len=5, **head)
    a, b = PPOEngine(cfg, 0), PPOEngine(cfg, 0)
    if cat:
        TD._give_the_logits_content(torch, a, b)
    assert a.env_opts is None and a._fused_rollout_ok() and b._fused_rollout_ok()
    b.env_opts = N.PPOEnvOpts(0, 0.0, 0.0, 0, 0.0, 0.0, 1.0, 0.0)  # -> the _ex entry point
    for it in range(2):
        a.rollout()
        b.rollout()
        torch.cuda.synchronize()
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "episode_return", "_last_v"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
        assert torch.equal(a.env.state, b.env.state) and torch.equal(a.env.obs, b.env.obs) and int(a.b_done.sum()) > 0
    bad = N.PPOEnvOpts(1, 1.0, 0.0, 0, 0.0, 0.0, 1.0, 0.0)  # a reward clip whose bounds are crossed: refused before anything is launched
    b.env_opts = bad
    with pytest.raises(N.SrlxError, match="lower bound"):
        b.rollout()
    if cat:
        b.env_opts = N.PPOEnvOpts(0, 0.0, 0.0, 0, 0.0, 0.0, 2.0, 0.0)
        with pytest.raises(N.SrlxError, match="Normal head"):
            b.rollout()
        with pytest.raises(ValueError, match="Normal head"):
            PPOEngine(PPODeviceConfig(n_envs=16, obs_dim=4, n_actions=2, action_scale=2.0), 0)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["CartPole-v1", "Pendulum-v1"])
def test_default_plugin_config_trains_on_the_engine_and_plays_through_the_plugin(env_name):
    """`ppo_config_from(ppo.Config(), env, 256, seed)` -- the staircase schedule, the environment's step limit, Pendulum's action scale of 2 -- runs on the fused
    engine, eagerly and through its graphs; the trained network goes to the plugin's Parameter, and `Runner.evaluate()` plays the environment with it."""
    N, lib, torch, dev = TN._env()
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.device import vector_runner as vr
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    runner = srl.Runner(env_name, ppo.Config())
    runner.set_device("cuda:0")
    runner.setup_rl_config()
    assert vr.why_not_ppo_engine(runner.env, runner.rl_config) == ""
    d = vr.ppo_config_from(runner.rl_config, runner.env, 256, 5, horizon=16)
    assert d.lr_scheduler.schedule_type == "step" and (d.action_scale == 2.0) == (env_name == "Pendulum-v1")
    eng = PPOEngine(d, 0)
    assert eng.fused and eng._fused_rollout_ok() and eng.scheduled and (eng.env_opts is not None) == (env_name == "Pendulum-v1")
    start = eng.flat.clone()
    eng.step()
    eng.capture_graphs()
    for _ in range(3):
        eng.step()
    torch.cuda.synchronize()
    info = eng.info()
    print("PPO-CFG end to end %s: %s, moved %.3g, optimiser steps %s" % (env_name, info, float((eng.flat - start).abs().max()), eng.opt_step.tolist()))
    assert all(np.isfinite(list(info.values()))) and bool(torch.isfinite(eng.flat).all())
    assert float((eng.flat - start).abs().max()) > 1e-3 and eng.opt_step.tolist() == [5 * 16, 0]
    eng.export_to(runner.parameter)
    x = torch.randn(64, d.obs_dim, device=dev)
    with torch.no_grad():
        out_p = runner.parameter.model.to(dev)(x)
    for mine, theirs in zip(eng.forward(x), out_p):
        torch.testing.assert_close(mine.view(-1), theirs.view(-1), rtol=1e-5, atol=1e-5)
    rewards = runner.evaluate(max_episodes=2, enable_progress=False)
    assert len(rewards) == 2 and np.all(np.isfinite(rewards))
