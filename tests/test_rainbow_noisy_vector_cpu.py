"""Rainbow with NoisyLinear layers on flat observations, the parts that need no GPU: the float64 yardstick (tests/rainbow_noisy_reference.py) against the
reference's recorded Trainer.train() with its recorded noise, its pick_items within the cap on every envelope shape of the GPU tests, the noisy EngineMLPQNet
against the plugin's module tree, the mapping of rainbow.Config(enable_noisy_dense=True) onto VectorQConfig, and the new libsrlx symbols."""
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import rainbow
from simple_distributed_rl_amd.device import vector_runner as vr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rainbow_noisy_recipe as NC  # noqa: E402
import rainbow_noisy_reference as M  # noqa: E402


def _recorded(name):
    """The three effective sets and the s_0 eps of a recorded case, from the recipe's parameters and the golden's noise."""
    z = np.load(os.path.join(HERE, "golden", "train_step_rainbow_noisy_vec.npz"))
    case, mk, sk, (mu, sig), (mu_t, sig_t), it = M.golden_inputs(name)
    eps = {label: [None if s is None else torch.tensor(z[f"{name}.{label}.{k}"]) for k, s in zip(mk, sk)] for label in ("eps_next", "eps_target", "eps_s0")}
    return z, case, mk, sk, mu, sig, M.effective(mu, sig, eps["eps_next"]), M.effective(mu_t, sig_t, eps["eps_target"]), eps["eps_s0"], it


@pytest.mark.parametrize("name", list(NC.CASES))
def test_float64_reference_matches_the_reference_trainer(name):
    """tests/rainbow_noisy_reference.py against ONE recorded Trainer.train() of the reference's Rainbow with enable_noisy_dense per case, under the noise the
    reference drew, at the bars of test_rainbow_vector_cpu.py: target, online Q of s_0, loss and priorities within rel 1e-5; every p.grad (mu and sigma) within
    rel 1e-5 with an absolute slack of 1e-5 * max |g|; every parameter after Adam within rel 1e-5 (+ 1e-7), except entries whose reference gradient is below
    1e-4 * max |g| (the first Adam step is about lr * g / |g|: only the bound 2 lr holds there)."""
    z, case, mk, sk, mu, sig, eff_next, eff_target, eps0, it = _recorded(name)
    g = lambda k: z[f"{name}.{k}"]  # noqa: E731
    lr = float(g("lr"))
    out = M.learner_step(mu, sig, eps0, eff_next, eff_target, it.states.double(), it.act.long(), it.rew.double(), it.term.double(), it.w.double(),
                         float(g("discount")), case["retrace_h"], case["double_dqn"], False, case["dueling_type"])
    np.testing.assert_allclose(out.q0.numpy(), g("q0"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.target.numpy(), g("target_q"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.loss, float(g("loss")), rtol=1e-5)
    np.testing.assert_allclose(out.priorities.numpy(), g("priorities"), rtol=1e-5, atol=1e-5 * float(np.abs(g("target_q")).max()))
    keys = mk + [k for k in sk if k is not None]
    params = mu + [s for s in sig if s is not None]
    grads = out.grads + [s for s in out.sigma_grads if s is not None]
    assert sorted(keys) == sorted(k for k, _ in NC.keys_shapes(case))
    after = M.adam_steps(params, [grads], lr)[0][0]
    for k, grad, aft in zip(keys, grads, after):
        gr, gmax = g("grad." + k), float(np.abs(g("grad." + k)).max())
        np.testing.assert_allclose(grad.numpy(), gr, rtol=1e-5, atol=1e-5 * gmax, err_msg=k)
        want = g("after." + k)
        firm = np.abs(gr) >= 1e-4 * gmax
        np.testing.assert_allclose(aft.numpy()[firm], want[firm], rtol=1e-5, atol=1e-7, err_msg=k)
        assert np.abs(aft.numpy()[~firm] - want[~firm]).max(initial=0.0) <= 2 * lr * (1 + 1e-3), k


def test_recorded_draws_are_three_independent_normal_draws_and_mix_retrace_branches():
    """What the golden must contain: three different noise tensors per noisy tensor with standard-normal moments over the whole record, and, under the recorded noise, taken actions at steps >= 1 that equal the selecting arg-max for some items only."""
    for name in NC.CASES:
        z, case, mk, sk, mu, sig, eff_next, eff_target, eps0, it = _recorded(name)
        noisy = [k for k, s in zip(mk, sk) if s is not None]
        assert len(noisy) == 2 * (len(case["layer_sizes"]) - 1) + 8
        allv = []
        for k in noisy:
            a, b, c = (z[f"{name}.{lb}.{k}"] for lb in ("eps_next", "eps_target", "eps_s0"))
            assert a.shape == z[f"{name}.grad.{k}"].shape and not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
            allv += [a.ravel(), b.ravel(), c.ravel()]
        allv = np.concatenate(allv).astype(np.float64)
        assert abs(allv.mean()) <= 5 / np.sqrt(allv.size) and abs(allv.var() - 1) <= 5 * np.sqrt(2 / allv.size)
        sel = []
        M.target_q(eff_next, eff_target, it.states[:, 1:].double(), it.act.long(), it.rew.double(), it.term.double(), 0.99, case["retrace_h"], case["double_dqn"],
                   False, case["dueling_type"], sel)
        hit = it.act[:, 1:].long() == sel[0].argmax(-1)[:, 1:]
        assert bool(hit.any()) and bool((~hit).any()), name


@pytest.mark.parametrize("D, ins, hid, H, A, dtype, n", M.ENVELOPE, ids=[f"{e[0]}-{'x'.join(map(str, e[1] + e[2])) or 'none'}-{e[3]}-{e[4]}-n{e[6]}" for e in M.ENVELOPE])
@pytest.mark.parametrize("double_dqn", [True, False], ids=["double", "single"])
def test_pick_items_stays_within_its_cap(D, ins, hid, H, A, dtype, n, double_dqn):
    """pick_items over three effective sets asserts its own cap (at most 15 % of 400 candidates discarded) and that both Huber branches, terminal and
    non-terminal items and both retrace branches occur; here on every envelope shape with torch.randn stand-in noise at the reference's initial sigma."""
    g = torch.Generator().manual_seed(5)
    (mu, sig), (mu_t, sig_t) = M.init_params(D, ins, hid, H, A, 11), M.init_params(D, ins, hid, H, A, 12)
    draw = lambda ps, ss: [None if s is None else torch.randn(p.shape, generator=g) for p, s in zip(ps, ss)]  # noqa: E731
    on0, on_next, tg = M.effective(mu, sig, draw(mu, sig)), M.effective(mu, sig, draw(mu, sig)), M.effective(mu_t, sig_t, draw(mu_t, sig_t))
    it = M.pick_items(on0, on_next, tg, D, A, n, dtype, 0.99, 1.0, double_dqn, False, 3)
    assert it.idx.shape == (M.KEEP, n + 1) and it.act.shape == (M.KEEP, n)


@pytest.mark.parametrize("in_sizes, layer_sizes, dtype", [((), (512,), "average"), ((32,), (64, 64), ""), ((), (64, 96), "average")])
def test_noisy_engine_net_speaks_the_noisy_rainbow_module_tree(in_sizes, layer_sizes, dtype):
    """State_dict keys in the plugin network's order, values through load / store unchanged, `kernel_sigmas()` None exactly for the `in_sizes` layers, the
    reference's initial sigma 0.5 / sqrt(in), and a forward pass that draws fresh noise per call and equals the plugin's at sigma = 0."""
    from simple_distributed_rl_amd.algorithms.dqn import build_qnetwork
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    c = rainbow.Config(enable_noisy_dense=True)
    c.input_block.value.set(in_sizes)
    c.hidden_block.set_dueling_network(layer_sizes, dueling_type=dtype)
    r = srl.Runner("CartPole-v1", c)
    r.setup_rl_config()
    torch.manual_seed(4)
    ref = build_qnetwork(r.rl_config)
    net = EngineMLPQNet(4, in_sizes, layer_sizes[:-1], 2, layer_sizes[-1], dtype, noisy=True)
    assert list(net.reference_state_dict()) == list(ref.state_dict())
    mus, sigmas = net.kernel_parameters(), net.kernel_sigmas()
    assert len(mus) == len(sigmas) == 2 * (len(in_sizes) + len(layer_sizes) - 1) + 8
    assert [s is None for s in sigmas] == [l < len(in_sizes) for l in range(len(mus) // 2) for _ in range(2)]
    for l in range(len(in_sizes), len(mus) // 2):
        fan_in = mus[2 * l].shape[1]
        for s, m in zip(sigmas[2 * l:2 * l + 2], mus[2 * l:2 * l + 2]):
            assert s.shape == m.shape and bool((s == np.float32(0.5 / np.sqrt(fan_in))).all())
            assert float(m.detach().abs().max()) <= 1 / np.sqrt(fan_in)
    for p in ref.parameters():  # (distinct values everywhere: a swapped pair would show)
        torch.nn.init.uniform_(p, -0.5, 0.5)
    net.load_reference_state_dict(ref.state_dict())
    sd = net.reference_state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    x = torch.randn(9, 4)
    with torch.no_grad():
        assert not torch.equal(net(x), net(x))  # noise drawn anew on every forward
        for s in [s for s in sigmas if s is not None]:
            s.zero_()
        ref.load_state_dict(net.reference_state_dict())
        assert float((net(x) - ref(x)).abs().max()) <= 1e-6 * float(ref(x).abs().max())
    plain = EngineMLPQNet(4, in_sizes, layer_sizes[:-1], 2, layer_sizes[-1], dtype)
    assert plain.kernel_sigmas() == [None] * len(plain.kernel_parameters()) and all(k.endswith((".weight", ".bias")) for k in plain.reference_state_dict())


def test_noisy_rainbow_config_mapping():
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    assert VectorQConfig().enable_noisy_dense is False
    r = srl.Runner("CartPole-v1", rainbow.Config(enable_noisy_dense=True))
    r.setup_rl_config()
    assert "no noisy dense layers" in vr.why_not_flat_rainbow(r.env, r.rl_config)
    assert vr.why_not_flat_rainbow(r.env, r.rl_config, admit_noisy=True) == ""
    d = vr.mlp_config_from(r.rl_config, r.env, 64, 3)
    assert d.enable_noisy_dense is True and (d.dueling_units, d.multisteps, d.hidden_sizes, d.in_sizes) == (512, 3, (), ())
    r = srl.Runner("CartPole-v1", rainbow.Config())
    r.setup_rl_config()
    assert vr.mlp_config_from(r.rl_config, r.env, 64, 3).enable_noisy_dense is False
    assert vr.why_not_flat_rainbow(r.env, r.rl_config, admit_noisy=True) == ""
    bad = rainbow.Config(enable_noisy_dense=True, multisteps=8)  # (the rest of the envelope still holds with the keyword)
    r = srl.Runner("CartPole-v1", bad)
    r.setup_rl_config()
    assert "multisteps of at most 7" in vr.why_not_flat_rainbow(r.env, r.rl_config, admit_noisy=True)


def test_new_symbols_resolve():
    lib = N.lib()
    for name in ("srlx_mlpq_bind_noisy", "srlx_mlpq_bind_noisy_grads", "srlx_mlpq_bind_noisy_adam", "srlx_mlpq_noisy_draw", "srlx_mlpq_noisy_eps"):
        assert name in N.SIGNATURES and hasattr(lib, name), name
    # the argument checks that need no device: a NULL handle is an error with a message
    assert lib.srlx_mlpq_bind_noisy(None, None, 0) != 0 and b"mlpq_bind_noisy" in lib.srlx_last_error()
    assert lib.srlx_mlpq_noisy_draw(None, None, None) != 0 and b"mlpq_noisy_draw" in lib.srlx_last_error()
