"""surrogate_type "kl" without a GPU: what `vector_runner` answers with and without `admit_kl`, PPODeviceConfig's new fields, and the float64 restatement of the two
KL divergences (tests/ppo_kl_reference.py) against independent formulas."""
import dataclasses
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_kl_reference as K  # noqa: E402


def _pair(env_name, rl):
    import simple_distributed_rl_amd as srl

    runner = srl.Runner(env_name, rl)
    runner.setup_rl_config()
    return runner.env, runner.rl_config


def test_two_argument_answer_is_unchanged_and_admit_kl_opens_it():
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.device import vector_runner as vr

    for name in ("CartPole-v1", "Pendulum-v1"):
        env, c = _pair(name, ppo.Config(surrogate_type="kl", adaptive_kl_target=0.02))
        assert "unknown surrogate_type 'kl'" in vr.why_not_ppo_engine(env, c)
        assert vr.why_not_ppo_engine(env, c, admit_kl=True) == ""
        try:
            vr.ppo_config_from(c, env, 64, 3)
        except ValueError as e:
            assert "unknown surrogate_type 'kl'" in str(e)
        else:
            raise AssertionError("ppo_config_from mapped \"kl\" without admit_kl")
        d = vr.ppo_config_from(c, env, 64, 3, admit_kl=True)
        assert d.surrogate_type == "kl" and d.adaptive_kl_target == 0.02 and d.adaptive_kl_beta == 0.5
        env, c = _pair(name, ppo.Config(surrogate_type="klx"))
        assert "unknown surrogate_type 'klx'" in vr.why_not_ppo_engine(env, c, admit_kl=True)
        env, c = _pair(name, ppo.Config())  # other surrogates: the keyword changes nothing
        assert dataclasses.asdict(vr.ppo_config_from(c, env, 64, 3, admit_kl=True)) == dataclasses.asdict(vr.ppo_config_from(c, env, 64, 3))
    assert "adaptive_kl_target" in vr.PPO_REFUSED_FIELDS  # (the tuples stay as they are until the route flips)


PARENT_DEFAULTS = dict(
    n_envs=4096, horizon=32, epochs=4, minibatches=4, episode_len=200, obs_dim=3, action_dim=1, hidden_sizes=(64, 64), value_sizes=(64,), policy_sizes=(64,), discount=0.9,
    gae_discount=0.9, baseline_type="advantage", v_target="gae", surrogate_type="clip", policy_clip_range=0.2, enable_value_clip=True, value_clip_range=0.2, lr=0.0002,
    value_loss_weight=1.0, entropy_weight=0.01, global_gradient_clip_norm=0.5, stable_gradients_scale_range=(1e-10, 10), seed=0, n_actions=0, reward_clip=None, state_clip=None,
    action_scale=1.0, action_offset=0.0)


def test_device_config_keeps_every_old_default():
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig

    d = PPODeviceConfig()
    for k, v in PARENT_DEFAULTS.items():
        assert getattr(d, k) == v, k
    assert d.lr_scheduler.schedule_type == ""
    names = [f.name for f in dataclasses.fields(d)]
    assert sorted(set(names) - set(PARENT_DEFAULTS) - {"lr_scheduler"}) == ["adaptive_kl_beta", "adaptive_kl_target"]
    assert (d.adaptive_kl_target, d.adaptive_kl_beta) == (0.01, 0.5)


def test_plugin_config_documents_kl_and_parameter_keeps_beta():
    from simple_distributed_rl_amd.algorithms import ppo

    c = ppo.Config(surrogate_type="kl")
    assert c.adaptive_kl_target == 0.01 and K.BETA_START == 0.5


def test_normal_kl_is_torch_distributions():
    g = torch.Generator().manual_seed(0)
    m1, m2 = torch.randn(500, 3, generator=g, dtype=torch.float64), torch.randn(500, 3, generator=g, dtype=torch.float64)
    ls1, ls2 = 2 * torch.randn(500, 3, generator=g, dtype=torch.float64), 2 * torch.randn(500, 3, generator=g, dtype=torch.float64)
    ls1[0], ls2[0] = math.log(1e-10), math.log(10)  # the clamp's own bounds
    ls1[1], ls2[1] = math.log(10), math.log(1e-3)
    want = torch.distributions.kl_divergence(torch.distributions.Normal(m1, torch.exp(ls1)), torch.distributions.Normal(m2, torch.exp(ls2)))
    got = K.kl_normal(torch, m1, ls1, m2, ls2)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert float(K.kl_normal(torch, m1, ls1, m1, ls1).abs().max()) <= 2.0 ** -52  # (exp(2 ls) exp(-2 ls) is 1 to one rounding)


def test_categorical_kl_is_the_clipped_sum():
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((200, 5))
    logits[0] = [30.0, 0.0, 0.0, 0.0, 0.0]  # new probabilities of 1e-13: below the clip
    old = rng.dirichlet(np.ones(5), size=200)
    old[1] = [0.0, 0.5, 0.5, 0.0, 0.0]  # old probabilities of exactly 0
    new = np.exp(logits - logits.max(1, keepdims=True))
    new /= new.sum(1, keepdims=True)
    want = np.zeros(200)
    for i in range(200):
        for k in range(5):
            q, p = min(max(old[i, k], 1e-10), 1.0), min(max(new[i, k], 1e-10), 1.0)
            want[i] += q * math.log(q / p)
    got = K.kl_categorical(torch, torch.as_tensor(old), torch.as_tensor(new))
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-15)
    # the gradient formula of csrc/srlx_ppo_math.h against autograd: d kl / d logit_j = g_j P_j - P_j sum_k g_k P_k, g_k = -q_k / p_k where the clip passes
    lg = torch.as_tensor(logits, dtype=torch.float64).requires_grad_()
    P = torch.softmax(lg, dim=-1)
    K.kl_categorical(torch, torch.as_tensor(old), P).sum().backward()
    Pn = P.detach().numpy()
    g = np.where((Pn >= 1e-10) & (Pn <= 1.0), -np.clip(old, 1e-10, 1.0) / np.clip(Pn, 1e-10, 1.0), 0.0)
    formula = g * Pn - Pn * (g * Pn).sum(1, keepdims=True)
    np.testing.assert_allclose(lg.grad.numpy(), formula, rtol=1e-9, atol=1e-12)
    assert float(np.abs(formula[0]).max()) > 0 and Pn[0, 1] < 1e-12


def test_beta_adaptation_rule():
    assert K.adapt_beta(0.5, 1.0, 2.25) == 0.25 and K.adapt_beta(0.5, 1.0, 1 / 2.25) == 1.0 and K.adapt_beta(8.0, 1.0, 1 / 2.25) == 16.0
    assert K.adapt_beta(16.0, 1.0, 1 / 2.25) == 16.0 and K.adapt_beta(0.5, 1.0, 1.0) == 0.5


def test_standard_normal_logits_stay_out_of_the_probability_band():
    """The GPU tests drop rows with a new probability between 1e-11 and 1e-9 (which side of the 1e-10 clip they fall on is the yardstick's precision); with the
    logits those tests draw (a network's output, standard normal here, at most 8 of them) no row is near it."""
    g = torch.Generator().manual_seed(5)
    p = torch.softmax(torch.randn(100000, 8, generator=g, dtype=torch.float64), dim=-1)
    assert float(p.min()) > 1e-9
