"""Discrete-action PPO on the device engine, the parts that need no GPU: the categorical network's geometry in libsrlx (the library loads without a device, as
tests/test_abi.py shows), the host restatement of its loss (tests/ppo_cat_reference.py) against torch autograd and the oracle, and the weight exchange with the
PPO plugin's network.  The reference's PPO needs TensorFlow: parity UNPINNED, as for the whole PPO row.
Two tests here, `test_reference_seeds_equal_autograd_and_losses_equal_the_oracle` and `test_sampling_rule_of_the_reference`, validate the YARDSTICK alone (the helper
against torch autograd and the oracle): they touch no symbol of the feature beyond this module's imports (`PPOEngine.export_to` among them), so their bodies would
pass without it; what they protect is every GPU comparison that is made against that helper.  The other tests need the new symbols or the new config field."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hot_path_oracle as H  # noqa: E402
import ppo_cat_reference as R  # noqa: E402

from simple_distributed_rl_amd import _native as N  # noqa: E402
from simple_distributed_rl_amd.device.ppo import ActorCritic, PPODeviceConfig, PPOEngine  # noqa: E402


def test_default_config_is_still_the_continuous_engine():
    cfg = PPODeviceConfig()
    assert cfg.n_actions == 0 and cfg.obs_dim == 3 and cfg.action_dim == 1
    net = ActorCritic(cfg)
    assert hasattr(net, "loc_layer") and hasattr(net, "log_scale_layer") and not hasattr(net, "logits_layer")
    assert len(net(torch.zeros(2, 3))) == 3
    assert N.lib().srlx_ppo_net_param_count(3, 1) == 12931 == sum(p.numel() for p in net.parameters())


@pytest.mark.parametrize("obs,n", [(4, 2), (1, 2), (5, 3), (8, 8), (3, 5)])
def test_param_count_and_partials_follow_the_module(obs, n):
    lib = N.lib()
    net = ActorCritic(PPODeviceConfig(obs_dim=obs, n_actions=n))
    assert hasattr(net, "logits_layer") and not hasattr(net, "loc_layer")
    names = [k for k, _ in net.named_parameters()]
    assert names[-2:] == ["logits_layer.weight", "logits_layer.bias"] and names[0] == "hidden_block.0.weight"
    P = sum(p.numel() for p in net.parameters())
    assert lib.srlx_ppo_cat_param_count(obs, n) == P == 64 * obs + 64 + 3 * (64 * 64 + 64) + 64 + 1 + 64 * n + n
    assert lib.srlx_ppo_cat_partials_floats(obs, n) == 256 * ((P + 3 + 3) & ~3)  # the existing formula: 256 workgroups x (P + 3 loss sums, rounded to 16 bytes)
    v, logits = net(torch.zeros(7, obs))
    assert v.shape == (7,) and logits.shape == (7, n)


def test_geometry_outside_the_envelope_is_refused():
    lib = N.lib()
    for obs, n in ((0, 2), (9, 2), (4, 1), (4, 0), (4, 9)):
        assert lib.srlx_ppo_cat_param_count(obs, n) == -1 and lib.srlx_ppo_cat_partials_floats(obs, n) == -1, (obs, n)
    assert lib.srlx_ppo_cat_rollout_max_horizon(1) == -1 and lib.srlx_ppo_cat_rollout_max_horizon(9) == -1
    assert 32 <= lib.srlx_ppo_cat_rollout_max_horizon(2) <= 1024


def _case(B, n, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    logits, a = 2.0 * f(B, n), rng.integers(0, n, B).astype(np.int32)
    olp = (R.log_softmax32(logits)[np.arange(B), a] + 0.3 * f(B)).astype(np.float32)
    adv, v, vt = f(B), f(B), f(B)
    ov = (v + 0.3 * f(B)).astype(np.float32)
    return logits, a, olp, adv, v, vt, ov


@pytest.mark.parametrize("base,clip,vclip", [(1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0)])
@pytest.mark.parametrize("B,n", [(512, 2), (300, 3), (257, 8)])
def test_reference_seeds_equal_autograd_and_losses_equal_the_oracle(base, clip, vclip, B, n):
    logits, a, olp, adv, v, vt, ov = _case(B, n, B + n + base)
    pc, vc, vw, ew = 0.2, 0.2, 0.7, 0.01
    losses, d_logits, d_v = R.losses_and_seeds64(logits, a, olp, adv, v, vt, ov, base, clip, pc, vclip, vc, vw, ew)
    d = torch.float64
    t = lambda x: torch.as_tensor(x).to(d)  # noqa: E731
    lg, vg = t(logits).requires_grad_(), t(v).requires_grad_()
    parts = R.torch_loss(torch, lg, torch.as_tensor(a), t(olp), t(adv), vg, t(vt), t(ov), base, clip, pc, vclip, vc, vw, ew)
    sum(parts).backward()
    np.testing.assert_allclose(np.array(losses), np.array([float(p.detach()) for p in parts]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(d_logits, lg.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(d_v, vg.grad.numpy(), rtol=1e-10, atol=1e-15)
    # the oracle's compute_train_loss at K = 1 on the taken action's log-probability (float32 arithmetic)
    lp32 = R.log_softmax32(logits)[np.arange(B), a][:, None]
    want = H.ppo_loss(lp32, olp[:, None], adv, v, vt, ov, base, clip, pc, vclip, vc, vw, ew)
    np.testing.assert_allclose(np.array(losses), np.array(want, np.float64), rtol=1e-5, atol=1e-7)


def test_sampling_rule_of_the_reference():
    """The restated rule on its own: the inverse CDF over float32 probabilities, the fall-back to the last action, the floor, the first maximum; and the share of
    rows within 1e-6 of a cumulative boundary (the rows the GPU test may skip) stays far below its 0.1 % cap for the inputs that test uses."""
    logits = np.array([[0.0, 0.0, 0.0], [5.0, -5.0, 0.0], [-30.0, 0.0, -30.0]], np.float32)
    a, u, cum = R.sample(logits, 11, 3)
    assert cum.shape == (3, 3) and np.all(np.diff(cum, axis=1) >= 0) and np.allclose(cum[:, -1], 1.0, atol=1e-6)
    for i in range(3):
        want = next((k for k in range(3) if float(cum[i, k]) > u[i]), 2)
        assert a[i] == want
    assert R.sample(logits, 11, 3)[0].tolist() == a.tolist() and np.array_equal(R.uniforms(11, 3, 3), u)
    assert R.logp_taken(np.array([[0.0, -40.0]], np.float32), np.array([1]))[0] == np.float32(R.LOG_FLOOR)
    assert R.mode(np.array([[1.0, 3.0, 3.0, 2.0]], np.float32))[0] == 1
    for n in (2, 3, 8):
        rows = 120_000
        lg = (2.0 * np.random.default_rng(n).standard_normal((rows, n))).astype(np.float32)
        _, u, cum = R.sample(lg, 1234, 7)
        share = R.near_boundary(u, cum).mean()
        assert share <= 1e-3 and share <= 10 * n * 2e-6 + 5e-5, (n, share)  # expected about n * 2e-6


def test_plugin_network_round_trip():
    """engine network -> plugin `ppo.Parameter` -> another engine network: identical state, and the two architectures agree in float64 to 1e-12."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo

    torch.manual_seed(3)
    cfg = PPODeviceConfig(obs_dim=4, n_actions=2)
    net = ActorCritic(cfg)
    with torch.no_grad():
        assert not net.logits_layer.weight.any()  # the policy starts uniform (categorical_dist_block.py:147)
        torch.nn.init.orthogonal_(net.logits_layer.weight)
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    runner = srl.Runner("CartPole-v1", ppo.Config())
    parameter = runner.parameter
    assert set(k.split(".")[0] for k in parameter.model.state_dict()) == {"hidden_block", "value_block", "value_out", "policy_block", "policy_out"}
    PPOEngine.export_to(types.SimpleNamespace(net=net), parameter)
    x = torch.randn(33, 4, dtype=torch.float64)
    with torch.no_grad():
        v_e, lg_e = net.double()(x)
        v_p, lg_p = parameter.model.double()(x)
    assert float((v_e - v_p.view(-1)).abs().max()) <= 1e-12 and float((lg_e - lg_p).abs().max()) <= 1e-12
    parameter.model.float()
    # through the plugin's own backup / restore, then back into a fresh engine network
    other = srl.Runner("CartPole-v1", ppo.Config()).parameter
    other.restore(parameter.backup())
    back = ActorCritic(cfg)
    PPOEngine.load_from(types.SimpleNamespace(net=back), other)
    for (k, p), (_, q) in zip(net.float().state_dict().items(), back.state_dict().items()):
        assert torch.equal(p, q), k
    with pytest.raises(ValueError):  # another head size does not fit
        PPOEngine.export_to(types.SimpleNamespace(net=ActorCritic(PPODeviceConfig(obs_dim=4, n_actions=3))), parameter)
