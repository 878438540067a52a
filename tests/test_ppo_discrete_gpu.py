"""GPU tests of discrete-action PPO on the device engine (csrc/srlx_ppo_math.h, srlx_ppo.hip, srlx_ppo_net.hip, device/ppo.py): the categorical act kernel and the
self-resetting CartPole against their host restatement (tests/ppo_cat_reference.py), the fused network with a categorical head against the torch modules and
autograd in float64, the one-launch rollout against the step-wise kernels (bit-exact), and the engine: fused against the torch-autograd path, determinism, HIP
graphs, two data-parallel ranks, the hand-over to the PPO plugin, learning.
float32 work: tolerance 1e-5 relative (to a tensor's largest entry where sums cancel), the bars of tests/test_ppo_net_gpu.py; the reference's PPO needs
TensorFlow -- parity UNPINNED, as for the whole PPO row."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_cat_reference as R  # noqa: E402
from ppo_net_reference import rows_off_the_kinks  # noqa: E402

pytestmark = pytest.mark.gpu


def _env():
    import torch

    from simple_distributed_rl_amd import _native as N

    return N, N.lib(), torch, torch.device("cuda:0")


def _act(N, lib, torch, dev, logits, seed, counter, deterministic=0):
    rows, n = logits.shape
    lg = torch.as_tensor(logits, device=dev).contiguous()
    a, lp = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, device=dev)
    c = torch.full((1,), counter, dtype=torch.int64, device=dev)
    N.check(lib.srlx_ppo_categorical_act(rows, n, N.tptr(lg), seed, N.tptr(c), deterministic, N.tptr(a), N.tptr(lp), None))
    torch.cuda.synchronize()
    return a.cpu().numpy(), lp.cpu().numpy(), int(c.item())


# ---- the act kernel ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8])
def test_categorical_act_against_the_reference(n):
    """Actions equal the restated rule on the kernel's own float32 logits, row for row, except where the uniform lies within 1e-6 of a cumulative boundary (the
    device's expf / logf may round such a row to the neighbouring action): those rows are skipped, and their share is at most 0.1 % (expected: about n * 2e-6)."""
    N, lib, torch, dev = _env()
    rows, seed, counter = 120_000, 1234, 7
    logits = (2.0 * np.random.default_rng(n).standard_normal((rows, n))).astype(np.float32)
    got_a, got_lp, c_after = _act(N, lib, torch, dev, logits, seed, counter)
    assert c_after == counter + 1
    want_a, u, cum = R.sample(logits, seed, counter)
    skip = R.near_boundary(u, cum)
    print("near-boundary share", n, float(skip.mean()), "mismatches among them", int((got_a != want_a)[skip].sum()))
    assert skip.mean() <= 1e-3
    assert np.array_equal(got_a[~skip], want_a[~skip])
    assert got_a.min() >= 0 and got_a.max() < n
    np.testing.assert_allclose(got_lp, R.logp_taken(logits, got_a), rtol=1e-5, atol=1e-5)
    # the same (seed, counter) draws the same actions; the next counter does not
    again, _, _ = _act(N, lib, torch, dev, logits, seed, counter)
    other, _, _ = _act(N, lib, torch, dev, logits, seed, counter + 1)
    assert np.array_equal(again, got_a) and not np.array_equal(other, got_a)


def test_categorical_act_floor_tie_and_frequencies():
    N, lib, torch, dev = _env()
    rows, seed = 120_000, 99
    # the floor: the row with the smallest uniform of 64 counters takes action 0 at a probability in (u, 1e-6): its log-probability lies below log(1e-6)
    best = min(((float(R.uniforms(seed, c, rows).min()), c) for c in range(64)))
    u_min, c_star = best
    r_star = int(R.uniforms(seed, c_star, rows).argmin())
    assert u_min < 3e-7  # (7.7e6 draws: the smallest is about 1.3e-7)
    logits = np.zeros((rows, 2), np.float32)
    logits[r_star, 0] = np.float32(np.log(3.0 * u_min))
    a, lp, _ = _act(N, lib, torch, dev, logits, seed, c_star)
    assert a[r_star] == 0 and lp[r_star] == np.float32(R.LOG_FLOOR) and np.log(3.0 * u_min) < R.LOG_FLOOR
    assert np.all(lp[np.arange(rows) != r_star] > R.LOG_FLOOR)
    # deterministic: the first maximum, no draw, the counter stays
    tie = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [-1.0, -2.0, -3.0, -0.5]], np.float32)
    a, lp, c_after = _act(N, lib, torch, dev, tie, seed, 5, deterministic=1)
    assert a.tolist() == [1, 0, 3] and c_after == 5
    np.testing.assert_allclose(lp, R.logp_taken(tie, a), rtol=1e-5, atol=1e-5)
    # frequencies at fixed logits: within 5 binomial sigma of softmax
    row = np.array([0.5, -0.3, 1.0], np.float32)
    a, _, _ = _act(N, lib, torch, dev, np.tile(row, (rows, 1)), seed, 11)
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    for k in range(3):
        assert abs((a == k).sum() - rows * p[k]) <= 5 * np.sqrt(rows * p[k] * (1 - p[k])), (k, (a == k).mean(), p[k])


# ---- the self-resetting CartPole --------------------------------------------------------------------------------------------------------------------------------
def _cartpole_inputs(torch, E, max_steps, seed=0):
    rng = np.random.default_rng(seed)
    s0 = np.stack([rng.uniform(-2.6, 2.6, E), rng.uniform(-3, 3, E), rng.uniform(-0.25, 0.25, E), rng.uniform(-3, 3, E)], 1)
    st0 = rng.integers(0, max_steps - 1, E).astype(np.int32)
    st0[:64] = max_steps - 1  # truncation
    ep0 = rng.integers(1, 5, E).astype(np.int32)
    return s0, st0, ep0


def _auto_step(N, lib, torch, s0, st0, ep0, actions, max_steps, seed):
    E = len(st0)
    state, steps, episodes = torch.tensor(s0, device="cuda"), torch.tensor(st0, device="cuda"), torch.tensor(ep0, device="cuda")
    obs, rew, done = torch.empty(E, 4, device="cuda"), torch.empty(E, device="cuda"), torch.empty(E, dtype=torch.uint8, device="cuda")
    act = torch.tensor(actions, device="cuda")
    N.check(lib.srlx_cartpole_autoreset_step(E, N.tptr(state), N.tptr(steps), N.tptr(episodes), N.tptr(act), max_steps, seed,
                                             N.tptr(obs), N.tptr(rew), N.tptr(done), None))
    torch.cuda.synchronize()
    return state, steps, episodes, obs, rew, done


def test_cartpole_autoreset_step_against_the_host_environment_and_k_cartpole():
    from simple_distributed_rl_amd.envs.cartpole import THETA_LIMIT, X_LIMIT

    N, lib, torch, dev = _env()
    E, max_steps, seed = 4096, 500, 3
    s0, st0, ep0 = _cartpole_inputs(torch, E, max_steps)
    for act in (0, 1):
        actions = np.full(E, act, np.int32)
        state, steps, episodes, obs, rew, done = _auto_step(N, lib, torch, s0, st0, ep0, actions, max_steps, seed)
        host = R.HostCartPoleAuto(s0, st0, ep0, max_steps, seed)
        stepped, after, term, trunc = host.step(actions)
        got, d = state.cpu().numpy(), done.cpu().numpy().astype(bool)
        away = np.minimum(np.abs(np.abs(stepped[:, 0]) - X_LIMIT), np.abs(np.abs(stepped[:, 2]) - THETA_LIMIT)) > 1e-9
        assert away.mean() > 0.99 and np.array_equal(d[away], (term | trunc)[away])
        assert trunc[:64].sum() > 10 and term.sum() > 100 and (~d).sum() > 1000  # the three kinds of lane are all there
        same = d == (term | trunc)
        np.testing.assert_allclose(got[same], after[same], rtol=1e-12, atol=1e-15)  # the stepped state, or the next episode's first one
        assert bool((rew == 1).all())
        assert np.array_equal(obs.cpu().numpy(), got.astype(np.float32))
        assert np.array_equal(steps.cpu().numpy()[~d], st0[~d] + 1) and not steps.cpu().numpy()[d].any()
        assert np.array_equal(episodes.cpu().numpy(), ep0 + d)
        assert np.abs(got[d]).max() <= 0.05
        # k_cartpole (srlx_cartpole_step) on the same inputs: the same bits on every lane that does not reset, the same done flag everywhere
        st_k, steps_k, ep_k = torch.tensor(s0, device="cuda"), torch.tensor(st0, device="cuda"), torch.tensor(ep0, device="cuda")
        obs_k, rew_k = torch.empty(E, 4, device="cuda"), torch.empty(E, device="cuda")
        term_k, done_k = torch.empty(E, dtype=torch.uint8, device="cuda"), torch.empty(E, dtype=torch.uint8, device="cuda")
        act_k, nr = torch.tensor(actions, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
        N.check(lib.srlx_cartpole_step(E, N.tptr(st_k), N.tptr(steps_k), N.tptr(ep_k), N.tptr(nr), N.tptr(act_k), max_steps, seed, N.tptr(obs_k), N.tptr(rew_k), N.tptr(term_k),
                                       N.tptr(done_k), None))
        torch.cuda.synchronize()
        keep = ~done.bool()
        assert torch.equal(done_k, done) and torch.equal(rew_k, rew)
        assert torch.equal(st_k[keep], state[keep]) and torch.equal(obs_k[keep], obs[keep]) and torch.equal(steps_k[keep], steps[keep])
        # ... and the reset k_cartpole would make for the lanes that ended is the one the self-resetting step made
        nr = done.clone()
        N.check(lib.srlx_cartpole_step(E, N.tptr(st_k), N.tptr(steps_k), N.tptr(ep_k), N.tptr(nr), N.tptr(act_k), max_steps, seed, N.tptr(obs_k), N.tptr(rew_k), N.tptr(term_k),
                                       N.tptr(done_k), None))
        torch.cuda.synchronize()
        assert torch.equal(st_k[~keep], state[~keep]) and torch.equal(ep_k[~keep], episodes[~keep])
    # resets: reproduced by the same seed, different under another
    a1 = _auto_step(N, lib, torch, s0, st0, ep0, actions, max_steps, 3)
    a2 = _auto_step(N, lib, torch, s0, st0, ep0, actions, max_steps, 3)
    a3 = _auto_step(N, lib, torch, s0, st0, ep0, actions, max_steps, 4)
    d = a1[5].bool()
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[0][~d], a3[0][~d]) and not torch.equal(a1[0][d], a3[0][d])
    assert float(a3[0][d].abs().max()) <= 0.05


# ---- the fused network with a categorical head ---------------------------------------------------------------------------------------------------------------------
def _net(torch, dev, obs, n, seed):
    from simple_distributed_rl_amd.device.ppo import ActorCritic, PPODeviceConfig

    torch.manual_seed(seed)
    net = ActorCritic(PPODeviceConfig(obs_dim=obs, n_actions=n)).to(dev)
    with torch.no_grad():
        torch.nn.init.orthogonal_(net.logits_layer.weight)  # (it starts at zero, as the biases do: give every tensor content)
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).contiguous()
    return net, flat


@pytest.mark.parametrize("obs,n,rows", [(4, 2, 1000), (5, 3, 77), (8, 8, 4096)])
def test_forward_against_the_torch_modules_in_float64(obs, n, rows):
    N, lib, torch, dev = _env()
    net, flat = _net(torch, dev, obs, n, 1)
    assert lib.srlx_ppo_cat_param_count(obs, n) == flat.numel()
    x = torch.randn(rows, obs, device=dev)
    v, logits = torch.empty(rows, device=dev), torch.empty(rows, n, device=dev)
    N.check(lib.srlx_ppo_cat_forward(rows, obs, n, N.tptr(flat), N.tptr(x), N.tptr(v), N.tptr(logits), None))
    torch.cuda.synchronize()
    with torch.no_grad():
        v64, lg64 = net.double()(x.double())
    for got, want in ((v, v64), (logits, lg64)):
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("base,clip,vclip", [(1, 1, 1), (0, 0, 0)])
@pytest.mark.parametrize("obs,n,mb", [(4, 2, 8192), (5, 3, 1234), (8, 8, 2000)])  # (8 actions: the second half of the policy-head slots)
def test_minibatch_gradients_against_autograd_in_float64(base, clip, vclip, obs, n, mb):
    """d loss / d every parameter of one minibatch (rows drawn from a larger buffer, a count that is no multiple of the 64-sample tile) against autograd of the same
    loss through the torch modules and log_softmax in float64; the three reported losses; then clip + Adam against torch's, two steps."""
    N, lib, torch, dev = _env()
    net, flat = _net(torch, dev, obs, n, 2)
    total = 3 * mb
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    b_obs, b_adv, b_vt = r(total, obs), r(total), r(total)
    b_act = torch.randint(0, n, (total,), device=dev, generator=g, dtype=torch.int32)
    with torch.no_grad():
        v0, lg0 = net(b_obs)
    b_logp = (torch.log_softmax(lg0, dim=-1).gather(1, b_act.long().view(-1, 1)).squeeze(1) + 0.3 * r(total)).contiguous()
    b_val = (v0 + 0.3 * r(total)).contiguous()
    # rows away from the ReLU kinks (the existing test's filter: a pre-activation within float32 rounding of zero takes the other branch in float64)
    cand = rows_off_the_kinks(torch, net, b_obs)
    assert cand.numel() > 2 * mb
    rows = cand[torch.randperm(cand.numel(), device=dev, generator=g)[:mb]].contiguous()
    pc, vc, vw, ew = 0.2, 0.2, 0.7, 0.01
    P = flat.numel()
    partials = torch.zeros(lib.srlx_ppo_cat_partials_floats(obs, n), device=dev)
    grad, losses = torch.zeros(P, device=dev), torch.zeros(3, device=dev)
    N.check(lib.srlx_ppo_cat_minibatch(mb, N.tptr(rows), obs, n, N.tptr(flat), N.tptr(b_obs), N.tptr(b_act), N.tptr(b_logp), N.tptr(b_adv), N.tptr(b_vt), N.tptr(b_val),
                                       base, clip, pc, vclip, vc, vw, ew, N.tptr(partials), N.tptr(grad), N.tptr(losses), None))
    torch.cuda.synchronize()
    d = torch.float64
    net64 = net.double()
    v, lg = net64(b_obs[rows].to(d))
    parts = R.torch_loss(torch, lg, b_act[rows], b_logp[rows].to(d), b_adv[rows].to(d), v, b_vt[rows].to(d), b_val[rows].to(d), base, clip, pc, vclip, vc, vw, ew)
    sum(parts).backward()
    torch.testing.assert_close(losses.double(), torch.stack([p.detach() for p in parts]), rtol=1e-4, atol=1e-6)
    off = 0
    for name, p in net64.named_parameters():
        got, want = grad[off : off + p.numel()].double(), p.grad.reshape(-1)
        off += p.numel()
        print(name, "max |got - want| / max |want|", float((got - want).abs().max() / want.abs().max()))
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")
    assert off == P
    # ---- clip + Adam ----
    ref = flat.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=3e-4)
    m, v2, step = torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    mine = flat.clone()
    for k in range(2):
        gk = grad.clone() * (1.0 + k)
        ref.grad = gk.clone() * 0.5  # (grad_scale 0.5: the sum over two ranks -> their mean)
        norm = torch.nn.utils.clip_grad_norm_([ref], 0.01)
        opt.step()
        N.check(lib.srlx_ppo_cat_adam(obs, n, N.tptr(mine), N.tptr(gk), N.tptr(m), N.tptr(v2), N.tptr(step), 3e-4, 0.9, 0.999, 1e-8, 0.01, 0.5, None))
        torch.cuda.synchronize()
        assert float(norm) > 0.01  # (the clip is active)
        torch.testing.assert_close(mine, ref.detach(), rtol=3e-7, atol=3e-4 * 2e-5)  # (an ulp of the parameter, or 2e-5 of the step)
    assert step.tolist() == [2, 0]


# ---- the engine --------------------------------------------------------------------------------------------------------------------------------------------------
def _cfg(E, T, seed, **kw):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig

    return PPODeviceConfig(n_envs=E, horizon=T, seed=seed, obs_dim=4, n_actions=2, **kw)


def _give_the_logits_content(torch, *engines):
    """`logits_layer` starts at zero (a uniform policy, every logit 0): an orthogonal weight and a random bias, the same in every engine, put real logits through
    the log-softmax and the inverse CDF from the first rollout on.  (A fused engine's module tensors are views of its flat vector: written in place.)"""
    first = engines[0].net.logits_layer
    with torch.no_grad():
        torch.nn.init.orthogonal_(first.weight, gain=2.0)
        first.bias.copy_(0.5 * torch.randn_like(first.bias))
        for e in engines[1:]:
            e.net.logits_layer.weight.copy_(first.weight)
            e.net.logits_layer.bias.copy_(first.bias)
    assert float(first.weight.detach().abs().max()) > 0.1


def test_one_launch_rollout_equals_the_stepwise_kernels():
    """k_ppo_rollout<CartPoleCategorical> against the launches it fuses (network forward -> srlx_ppo_categorical_act -> srlx_cartpole_autoreset_step per step, then srlx_gae_scan),
    same seeds: every buffer, both counters (the action stream's, the lanes' episode counts), the environments' state and the episode bookkeeping -- bit for bit;
    every lane ends an episode inside the rollout (episode_len 11 < T).  The policy is not uniform (the logits layer is given content), and the third rollout
    runs on parameters that two updates have moved."""
    N, lib, torch, dev = _env()
    from simple_distributed_rl_amd.device.ppo import CartPoleAutoVecEnv, PPOEngine

    cfg = _cfg(272, 24, 4, episode_len=11)
    a, b = PPOEngine(cfg, 0), PPOEngine(cfg, 0)
    _give_the_logits_content(torch, a, b)
    assert torch.equal(a.flat, b.flat)
    assert a.fused and b.fused and a.cat and a._fused_rollout_ok() and isinstance(a.env, CartPoleAutoVecEnv)
    assert a.b_act.dtype == torch.int32 and a.b_act.shape == (24, 272) and a.b_logp.shape == (24, 272) and a.b_obs.shape == (25, 272, 4)
    b._fused_rollout_ok = lambda: False  # the step-wise path on the libsrlx network
    for it in range(3):
        a.rollout()
        b.rollout()
        torch.cuda.synchronize()
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "episode_return"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
        assert torch.equal(a._last_v, b._last_v) and torch.equal(a.env.state, b.env.state) and torch.equal(a.env.t, b.env.t) and torch.equal(a.env.episodes, b.env.episodes)
        assert int(a.act_counter.item()) == int(b.act_counter.item()) == cfg.horizon * (it + 1)
        assert bool((a.env.episodes >= 1 + 2 * (it + 1)).all())  # (the first episode's reset counts one; at least two ends per 24 steps)
        assert float(a.finished_returns[1]) == float(b.finished_returns[1]) == float((a.env.episodes - 1).sum())
        torch.testing.assert_close(a.finished_returns, b.finished_returns, rtol=1e-5, atol=1e-3)  # (float atomics: order differs)
        assert int(a.b_done.sum()) > 0 and 0 < float(a.b_act.float().mean()) < 1
        spread = float(a.b_logp.max() - a.b_logp.min())
        print("rollout", it, "log-probabilities span", spread)
        assert spread > 0.5  # (a uniform policy would have every entry at log 0.5)
        if it > 0:  # the next rollout runs on trained parameters: the same update on both sides (deterministic: the same bits)
            a.update()
            b.update()
            assert torch.equal(a.flat, b.flat)
        for e in (a, b):
            e.b_obs[0].copy_(e.b_obs[cfg.horizon])  # (the step-wise path starts from b_obs[0], the fused one from env.obs)
    assert torch.equal(a.env.obs, a.b_obs[cfg.horizon])


@pytest.mark.parametrize("v_target", ["gae", "return"])
def test_fused_engine_against_the_autograd_engine(v_target):
    """Three whole iterations of the fused engine against the torch-modules / log_softmax / autograd / torch.optim.Adam engine from the same parameters (the logits
    layer given content: the policy is not uniform) and seeds, at the bars of the continuous counterpart (tests/test_ppo_net_gpu.py).
    Rollouts: an environment whose draws all fall on the same side of the cumulative boundaries in both engines has the same trajectory, and its records agree to
    float32 rounding of the networks' sums; a draw whose uniform lies within the two engines' difference in cumulative probability (1e-6 at equal parameters, up
    to the parameters' difference after updates) may flip, after which that environment's trajectories differ -- at most a few of the 8192 draws of a rollout,
    so at least 99 % of the environments must match.  Every update then runs on IDENTICAL buffers and the environments are aligned again; the parameters are not:
    both engines keep their own, and their difference is held against the movement since the start (Adam divides by sqrt(v): an entry whose gradients are
    rounding residue may step differently -- bounded by a few % of the movement)."""
    N, lib, torch, dev = _env()
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    cfg = _cfg(512, 16, 6, v_target=v_target)
    a, b = PPOEngine(cfg, 0, fused=True), PPOEngine(cfg, 0, fused=False)
    _give_the_logits_content(torch, a, b)
    with torch.no_grad():
        for p, q in zip(a.net.parameters(), b.net.parameters()):
            assert torch.equal(p, q)  # (same seed, same initialisation)
    assert a.flat.data_ptr() == next(a.net.parameters()).data_ptr()  # the module's tensors are views of the flat vector
    start = a.flat.clone()
    for it in range(3):
        a.rollout()
        b.rollout()
        torch.cuda.synchronize()
        lanes = (a.b_act == b.b_act).all(dim=0)
        spread = float(a.b_logp.max() - a.b_logp.min())
        print("iteration", it, "environments with identical action sequences:", int(lanes.sum()), "of", cfg.n_envs, "; log-probabilities span", spread)
        assert spread > 0.5 and 0 < float(a.b_act.float().mean()) < 1  # (a uniform policy would have every entry at log 0.5)
        assert float(lanes.float().mean()) >= 0.99
        assert torch.equal(a.b_rew[:, lanes], b.b_rew[:, lanes]) and torch.equal(a.b_done[:, lanes], b.b_done[:, lanes])
        for name in ("b_logp", "b_val", "b_adv"):
            torch.testing.assert_close(getattr(a, name)[:, lanes], getattr(b, name)[:, lanes], rtol=2e-4, atol=2e-4, msg=lambda m: f"{name}: {m}")
        # the update on IDENTICAL buffers; the environments and their bookkeeping aligned for the next rollout
        for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "episode_return", "finished_returns"):
            getattr(b, name).copy_(getattr(a, name))
        for name in ("state", "t", "episodes", "obs"):
            getattr(b.env, name).copy_(getattr(a.env, name))
        a.update()
        b.update()
        torch.cuda.synchronize()
        for e in (a, b):
            e.b_obs[0].copy_(e.b_obs[cfg.horizon])
        moved = float((a.flat - start).abs().max())
        assert moved > 1e-3 * (it + 1)  # 16 steps of about lr each per iteration
        flat_b = torch.cat([p.detach().reshape(-1) for p in b.net.parameters()])
        diff = (a.flat - flat_b).abs()
        print("iteration", it, "moved", moved, "diff max", float(diff.max()), "diff mean", float(diff.mean()))
        assert float(diff.max()) < 0.03 * moved and float(diff.mean()) < 2e-4 * moved, (it, float(diff.max()), float(diff.mean()), moved)
        torch.testing.assert_close(a.losses, b.losses, rtol=1e-3, atol=1e-5)
        assert a.opt_step.tolist() == [cfg.epochs * cfg.minibatches * (it + 1), 0]


def test_engine_gates_determinism_and_graphs():
    N, lib, torch, dev = _env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    with pytest.raises(ValueError):
        PPOEngine(PPODeviceConfig(n_envs=64, n_actions=2), 0)  # CartPole has four observation dimensions
    with pytest.raises(ValueError):
        PPOEngine(PPODeviceConfig(n_envs=64, obs_dim=4, n_actions=2, hidden_sizes=(32, 32)), 0, fused=True)
    other = PPOEngine(PPODeviceConfig(n_envs=64, horizon=8, obs_dim=4, n_actions=2, hidden_sizes=(32, 32), epochs=1, minibatches=2), 0)
    assert not other.fused  # (other blocks: the torch modules, log_softmax and srlx_ppo_loss_logpi)
    other.step()
    long = PPOEngine(PPODeviceConfig(n_envs=32, horizon=600, obs_dim=4, n_actions=2, epochs=1, minibatches=2), 0)  # per-step records beyond the rollout kernel's LDS
    assert long.fused and not long._fused_rollout_ok() and lib.srlx_ppo_cat_rollout_max_horizon(2) < 600
    long.step()  # (the step-wise kernels on the libsrlx network)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(long.flat).all()) and int(long.act_counter.item()) == 600 and all(bool(torch.isfinite(p).all()) for p in other.net.parameters())

    def run(graphs):
        eng = PPOEngine(_cfg(1024, 16, 9), 0)
        assert eng.fused and eng._fused_rollout_ok()
        for k in range(7):
            if k == 2 and graphs:
                eng.capture_graphs()  # (runs one whole iteration itself, as its warm-up)
                continue
            eng.step()
        torch.cuda.synchronize()
        return eng

    a, b, c = run(False), run(False), run(True)
    for name in ("flat", "b_adv", "b_act", "b_obs", "exp_avg_sq", "episode_return", "finished_returns"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name  # two engines, one seed: bit-identical
    assert torch.equal(a.env.state, b.env.state) and torch.equal(a.env.episodes, b.env.episodes)
    assert torch.equal(a.flat, c.flat) and torch.equal(a.b_adv, c.b_adv) and torch.equal(a.b_act, c.b_act)  # eager launches == graph replays, bit for bit
    assert bool(torch.isfinite(a.flat).all()) and all(np.isfinite(list(a.info().values())))


def test_engine_hip_graphs():
    """The assertions of tests/test_ppo_gpu.py::test_ppo_engine_hip_graphs on the discrete engine: environments advance, parameters move, losses stay finite,
    episodes finish (CartPole episodes last at most episode_len = 200 steps: at least two per environment in 400 steps)."""
    N, lib, torch, dev = _env()
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    eng = PPOEngine(_cfg(512, 25, 2), 0)
    for _ in range(2):
        eng.step()
    eng.capture_graphs()
    before = [p.detach().clone() for p in eng.net.parameters()]
    obs0 = eng.b_obs[0].clone()
    eng.pop_mean_episode_return()
    for _ in range(16):
        eng.step()
    torch.cuda.synchronize()
    assert int(eng.finished_returns[1].item()) >= 2 * 512
    mean_return = eng.pop_mean_episode_return()
    assert np.isfinite(mean_return) and 1 <= mean_return <= 200
    assert all(np.isfinite(list(eng.info().values())))
    assert any(float((p.detach() - q).abs().max()) > 0 for p, q in zip(eng.net.parameters(), before))
    assert not torch.equal(eng.b_obs[0], obs0)


_DP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SRLX_ROOT"])
from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, DistributedPPO, CartPoleAutoVecEnv
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"], rank=int(os.environ["RANK"]), world_size=2)
dp = DistributedPPO(PPODeviceConfig(n_envs=256, horizon=16, epochs=2, minibatches=2, seed=5, obs_dim=4, n_actions=2), 0)
assert dp.engine.fused and dp.engine.cat and isinstance(dp.engine.env, CartPoleAutoVecEnv)
for _ in range(3):
    dp.step()
flat = torch.cat([p.detach().reshape(-1) for p in dp.engine.net.parameters()]).cpu()
obs = dp.engine.b_obs[0].cpu()
both = [torch.empty_like(flat) for _ in range(2)]
dist.all_gather(both, flat)
obs2 = [torch.empty_like(obs) for _ in range(2)]
dist.all_gather(obs2, obs)
assert torch.equal(both[0], both[1]), "parameters diverged across ranks"
assert not torch.equal(obs2[0], obs2[1]), "ranks must run different environments"
assert torch.isfinite(flat).all()
print("rank", dist.get_rank(), "ok")
"""


def test_data_parallel_two_ranks_one_gpu(tmp_path):
    """2 ranks (sharing the GPU, gloo rendezvous) keep identical parameters through averaged gradients while stepping different CartPole environments."""
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER)
    port = str(29500 + os.getpid() % 150)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(os.environ, SRLX_ROOT=ROOT, RANK=str(r), PORT=port), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)


def test_trained_policy_is_evaluated_through_the_plugin():
    """Train briefly on the engine, hand the weights to the PPO plugin's Parameter, and `Runner.evaluate()` plays CartPole-v1 with them on the plugin path; the plugin's
    weights go back into an engine unchanged."""
    N, lib, torch, dev = _env()
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.device.ppo import PPOEngine

    eng = PPOEngine(_cfg(256, 16, 3, episode_len=500), 0)
    for _ in range(5):
        eng.step()
    runner = srl.Runner("CartPole-v1", ppo.Config())
    runner.set_device("cuda:0")
    eng.export_to(runner.parameter)
    x = torch.randn(64, 4, device=dev)
    v_e, lg_e = eng.forward(x)
    with torch.no_grad():
        v_p, lg_p = runner.parameter.model.to(dev)(x)
    torch.testing.assert_close(lg_e, lg_p, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(v_e, v_p.view(-1), rtol=1e-5, atol=1e-5)
    rewards = runner.evaluate(max_episodes=3, enable_progress=False)
    assert len(rewards) == 3 and np.all(np.isfinite(rewards)) and min(rewards) >= 1
    fresh = PPOEngine(_cfg(256, 16, 99), 0)
    assert not torch.equal(fresh.flat, eng.flat)
    fresh.load_from(runner.parameter)
    assert torch.equal(fresh.flat, eng.flat)


LEARNING = dict(n_envs=1024, horizon=32, seed=1, episode_len=500)  # otherwise the reference's default hyper-parameters (ppo/config.py:43-110)
MARGIN = 80.0


@pytest.mark.slow
def test_engine_learns_cartpole():
    """The discrete engine with the reference's default hyper-parameters improves the mean episode return of 1024 CartPole environments (step limit 500): 6.5 M
    environment steps in about 0.2 s.  Measured with this build (profiles/ppo_discrete_learning.json, mean return of the episodes finished in each 20
    iterations): seed 1: 25.8, 173.4, 298.7, 290.1, 218.3, 203.4, 227.2, 297.8, 267.5, 193.1; seed 2: 27.3, 191.8, 244.9, 310.4, 257.2, 294.3, 269.8, 237.6,
    263.8, 238.7.  The smaller rise from the first to the last reading is 167; the margin is under half of it."""
    N, lib, torch, dev = _env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    eng = PPOEngine(PPODeviceConfig(obs_dim=4, n_actions=2, **LEARNING), 0)
    first = last = None
    for it in range(200):
        eng.step()
        if (it + 1) % 20 == 0:
            last = eng.pop_mean_episode_return()
            first = last if first is None else first
            print("iteration", it + 1, "mean episode return", last)
    assert all(np.isfinite(list(eng.info().values()))), eng.info()
    assert last > first + MARGIN, (first, last)
