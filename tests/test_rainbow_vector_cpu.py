"""Rainbow on flat observations, the parts that need no GPU: the float64 yardstick (tests/rainbow_vec_reference.py) against the reference's recorded
Trainer.train(), pick_items within its cap on every envelope shape of the GPU tests, the dueling EngineMLPQNet against the plugin's module tree, the mapping of
rainbow.Config onto VectorQConfig, every reason `why_not_flat_rainbow` gives, and the argument checks of srlx_mlpq_create_dueling (they run before any device
call)."""
import ctypes
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
import rainbow_vec_recipe as R  # noqa: E402
import rainbow_vec_reference as M  # noqa: E402

ENVELOPE, golden_inputs = M.ENVELOPE, M.golden_inputs


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_reference_matches_the_reference_trainer(name):
    """tests/rainbow_vec_reference.py against ONE recorded Trainer.train() of the reference's Rainbow per case (tests/golden/train_step_rainbow_vec.npz, inputs
    from tests/rainbow_vec_recipe.py), at the bars of the GPU golden test: target, online Q of s_0, loss and priorities within rel 1e-5; every p.grad within rel
    1e-5 with an absolute slack of 1e-5 * max |g|; every parameter after Adam within rel 1e-5 (+ 1e-7), except entries whose reference gradient is below
    1e-4 * max |g| (the first Adam step is about lr * g / |g|: only the bound 2 lr holds there)."""
    z = np.load(os.path.join(HERE, "golden", "train_step_rainbow_vec.npz"))
    case, keys, on, tg, it = golden_inputs(name)
    g = lambda k: z[f"{name}.{k}"]  # noqa: E731
    lr = float(g("lr"))
    out = M.learner_step(on, tg, it.states.double(), it.act.long(), it.rew.double(), it.term.double(), it.w.double(), float(g("discount")), case["retrace_h"],
                         case["double_dqn"], False, case["dueling_type"])
    np.testing.assert_allclose(out.q0.numpy(), g("q0"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.target.numpy(), g("target_q"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.loss, float(g("loss")), rtol=1e-5)
    np.testing.assert_allclose(out.priorities.numpy(), g("priorities"), rtol=1e-5, atol=1e-5 * float(np.abs(g("target_q")).max()))
    after = M.adam_steps(on, [out.grads], lr)[0][0]
    for k, grad, aft in zip(keys, out.grads, after):
        gr, gmax = g("grad." + k), float(np.abs(g("grad." + k)).max())
        np.testing.assert_allclose(grad.numpy(), gr, rtol=1e-5, atol=1e-5 * gmax, err_msg=k)
        want = g("after." + k)
        firm = np.abs(gr) >= 1e-4 * gmax
        np.testing.assert_allclose(aft.numpy()[firm], want[firm], rtol=1e-5, atol=1e-7, err_msg=k)
        assert np.abs(aft.numpy()[~firm] - want[~firm]).max(initial=0.0) <= 2 * lr * (1 + 1e-3), k


def test_recipe_items_end_inside_the_window_and_mix_retrace_branches():
    """What the golden's items must contain: an episode that ends at step 1 with padding behind it, and taken actions at steps >= 1 that equal the selecting
    network's arg-max for some steps and not for others -- in every multi-step case, so that retrace coefficients of 0 and of retrace_h ** m both occur."""
    for name, case in R.CASES.items():
        _, _, on, tg, it = golden_inputs(name)
        n = case["n"]
        if n == 1:
            assert float(it.term.sum()) == 1.0
            continue
        for b in R.ENDS:
            assert it.term[b].tolist() == [0.0] + [1.0] * (n - 1) and float(it.rew[b, 2:].abs().sum()) == 0.0
            assert all(torch.equal(it.states[b, m], it.states[b, 2]) for m in range(3, n + 1))
        sel = []
        M.target_q(on, tg, it.states[:, 1:].double(), it.act.long(), it.rew.double(), it.term.double(), 0.99, case["retrace_h"], case["double_dqn"], False,
                   case["dueling_type"], sel)
        hit = it.act[:, 1:].long() == sel[0].argmax(-1)[:, 1:]
        assert 0.3 < float(hit.float().mean()) < 0.9, name
        assert bool(hit.all(1).any()) and bool((~hit[:, 0]).any()), name
        assert 0.15 < float(sel[0].argmax(-1).float().mean()) < 0.85, name  # (the arg-max depends on the observation)


@pytest.mark.parametrize("D, trunk, H, A, dtype, n", ENVELOPE, ids=[f"{e[0]}-{'x'.join(map(str, e[1])) or 'none'}-{e[2]}-{e[3]}-n{e[5]}" for e in ENVELOPE])
def test_pick_items_stays_within_its_cap(D, trunk, H, A, dtype, n):
    """pick_items asserts its own cap (at most 15 % of 400 candidates discarded) and that both Huber branches, terminal and non-terminal items and both retrace
    branches occur; here on every envelope shape, with retrace_h 1 and double DQN."""
    on, tg = M.init_params(D, trunk, H, A, 11), M.init_params(D, trunk, H, A, 12)
    it = M.pick_items(on, tg, D, A, n, dtype, 0.99, 1.0, True, False, 3)
    assert it.idx.shape == (M.KEEP, n + 1) and it.act.shape == (M.KEEP, n)
    full = float((it.chain == n).float().mean())
    print(f"RAINBOW-VEC pick_items D={D} trunk={trunk} H={H} A={A} n={n}: full retrace chains {full:.2f}")


@pytest.mark.parametrize("in_sizes, layer_sizes, dtype", [((), (512,), "average"), ((32,), (64, 64), "average"), ((32,), (96, 64, 128), ""), ((), (64, 96), "")])
def test_dueling_engine_net_speaks_the_rainbow_module_tree(in_sizes, layer_sizes, dtype):
    from simple_distributed_rl_amd.algorithms.dqn import build_qnetwork
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    c = rainbow.Config()
    c.input_block.value.set(in_sizes)
    c.hidden_block.set_dueling_network(layer_sizes, dueling_type=dtype)
    r = srl.Runner("CartPole-v1", c)
    r.setup_rl_config()
    torch.manual_seed(4)
    ref = build_qnetwork(r.rl_config)
    for p in ref.parameters():  # (zero-initialised biases would hide a swapped pair)
        torch.nn.init.uniform_(p, -0.5, 0.5)
    net = EngineMLPQNet(4, in_sizes, layer_sizes[:-1], 2, layer_sizes[-1], dtype).load_reference_state_dict(ref.state_dict())
    sd = net.reference_state_dict()
    assert list(sd) == list(ref.state_dict())
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    x = torch.randn(33, 4, dtype=torch.float64)
    with torch.no_grad():
        want = ref.double()(x)
        got = net.double()(x)
        mine = M.forward([p.detach() for p in net.kernel_parameters()], x, dtype)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((mine - want).abs().max()) <= 1e-12 * float(want.abs().max())
    ps = net.kernel_parameters()
    n_trunk = len(in_sizes) + len(layer_sizes) - 1
    H = layer_sizes[-1]
    assert len(ps) == 2 * n_trunk + 8
    assert [tuple(p.shape) for p in ps[2 * n_trunk:]] == [(H, ps[2 * n_trunk].shape[1]), (H,), (1, H), (1,), (H, ps[2 * n_trunk].shape[1]), (H,), (2, H), (2,)]


def test_rainbow_config_mapping():
    r = srl.Runner("CartPole-v1", rainbow.Config())
    r.setup_rl_config()
    assert vr.why_not_flat_rainbow(r.env, r.rl_config) == ""
    d = vr.mlp_config_from(r.rl_config, r.env, 256, 7)
    assert (d.obs_dim, d.in_sizes, d.hidden_sizes, d.dueling_units, d.dueling_type, d.n_actions, d.n_envs, d.seed) == (4, (), (), 512, "average", 2, 256, 7)
    assert (d.multisteps, d.retrace_h, d.batch_size, d.enable_double_dqn) == (3, 1.0, 32, True)
    c = rainbow.Config(multisteps=5, retrace_h=0.5, enable_double_dqn=False)
    c.input_block.value.set((32,))
    c.hidden_block.set_dueling_network((64, 96), dueling_type="")
    c.memory.set_proportional(alpha=0.6, beta_initial=0.5)
    r = srl.Runner("CartPole-v1", c)
    r.setup_rl_config()
    assert vr.why_not_flat_rainbow(r.env, r.rl_config) == ""
    d = vr.mlp_config_from(r.rl_config, r.env, 16, 0)
    assert (d.in_sizes, d.hidden_sizes, d.dueling_units, d.dueling_type, d.multisteps, d.retrace_h) == ((32,), (64,), 96, "", 5, 0.5)
    assert (d.memory_alpha, d.memory_beta_initial, d.enable_double_dqn) == (0.6, 0.5, False)
    one = rainbow.Config(multisteps=1)  # Rainbow_no_multisteps
    r = srl.Runner("CartPole-v1", one)
    r.setup_rl_config()
    assert vr.mlp_config_from(r.rl_config, r.env, 16, 0).multisteps == 1 and vr.mlp_config_from(r.rl_config, r.env, 16, 0).dueling_units == 512


def test_vector_q_config_defaults_are_the_dqn_engine():
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    d = VectorQConfig()
    assert (d.dueling_units, d.dueling_type, d.multisteps, d.retrace_h) == (0, "average", 1, 1.0)


@pytest.mark.parametrize("change, env_id, reason", [
    (lambda c: setattr(c, "enable_noisy_dense", True), "CartPole-v1", "no noisy dense layers"),
    (lambda c: c.hidden_block.set_dueling_network((512,), dueling_type="max"), "CartPole-v1", "dueling types 'average' and ''"),
    (lambda c: c.hidden_block.set((64, 64)), "CartPole-v1", "an MLP hidden block stays on the plugin path"),
    (lambda c: c.hidden_block.set_dueling_network((64, 64, 64, 64)), "CartPole-v1", "at most 2 dense layers in front of the head"),
    (lambda c: (c.input_block.value.set((32, 32)), c.hidden_block.set_dueling_network((64, 64))), "CartPole-v1", "at most 2 dense layers in front of the head"),
    (lambda c: c.hidden_block.set_dueling_network((48,)), "CartPole-v1", "32..512 units in multiples of 32"),
    (lambda c: c.hidden_block.set_dueling_network((1024,)), "CartPole-v1", "32..512 units in multiples of 32"),
    (lambda c: c.hidden_block.set_dueling_network((16, 64)), "CartPole-v1", "32..512 units in multiples of 32"),
    (lambda c: c.hidden_block.set_dueling_network((64,), activation="tanh"), "CartPole-v1", "all of ReLU layers"),
    (lambda c: c.hidden_block.set_dueling_network((64, 64), use_bias=False), "CartPole-v1", "use_bias=False"),
    (lambda c: setattr(c, "multisteps", 8), "CartPole-v1", "multisteps of at most 7"),
    (lambda c: setattr(c, "window_length", 2), "CartPole-v1", "window_length 1"),
    (lambda c: setattr(c, "batch_size", 512), "CartPole-v1", "batches of at most 256"),
    (lambda c: c.memory.set_rankbased(), "CartPole-v1", "no device replay for memory"),
    (lambda c: None, "Grid", "observations are not single-channel image frames"),
])
def test_uncovered_rainbow_shapes_give_their_reason(change, env_id, reason):
    c = rainbow.Config()
    change(c)
    r = srl.Runner(env_id, c)
    r.setup_rl_config()
    assert reason in vr.why_not_flat_rainbow(r.env, r.rl_config)


def _create(D, trunk, H, dtype, A, rows, batch, nstep):
    h = N.c_p()
    widths = (ctypes.c_int * 3)(*(list(trunk) + [0, 0, 0])[:3])
    return N.lib().srlx_mlpq_create_dueling(ctypes.byref(h), D, len(trunk), ctypes.cast(widths, N.c_p), H, dtype, A, rows, batch, nstep, 0), h


# every bound of the envelope, one step outside it on each side: (D, trunk, H, dueling_type, A, max_rows, max_batch, max_nstep)
_OUTSIDE = [
    (0, (64,), 64, 0, 2, 16, 8, 3), (257, (64,), 64, 0, 2, 16, 8, 3),  # D 1..256
    (4, (64, 64, 64), 64, 0, 2, 16, 8, 3),  # 0..2 trunk layers
    (4, (0,), 64, 0, 2, 16, 8, 3), (4, (544,), 64, 0, 2, 16, 8, 3), (4, (48,), 64, 0, 2, 16, 8, 3), (4, (64, 16), 64, 0, 2, 16, 8, 3),  # trunk widths
    (4, (), 0, 0, 2, 16, 8, 3), (4, (), 544, 0, 2, 16, 8, 3), (4, (), 80, 0, 2, 16, 8, 3),  # H 32..512 in multiples of 32
    (4, (), 64, -1, 2, 16, 8, 3), (4, (), 64, 2, 2, 16, 8, 3),  # dueling_type 0 / 1
    (4, (), 64, 0, 1, 16, 8, 3), (4, (), 64, 0, 33, 16, 8, 3),  # A 2..32
    (4, (), 64, 0, 2, 0, 8, 3), (4, (), 64, 0, 2, 16, -1, 3), (4, (), 64, 0, 2, 16, 257, 3),  # max_rows >= 1, max_batch 0..256
    (4, (), 64, 0, 2, 16, 8, 0), (4, (), 64, 0, 2, 16, 8, 8),  # max_nstep 1..7
]


@pytest.mark.parametrize("args", _OUTSIDE, ids=[str(i) for i in range(len(_OUTSIDE))])
def test_create_dueling_rejects_what_is_outside_the_envelope(args):
    """One step outside each bound: SRLX_ERR_ARG (-1) and a NULL handle, decided before any device call (this test runs without a GPU)."""
    st, h = _create(*args)
    assert st == -1 and not h.value, (args, st)
    assert "mlpq_create_dueling" in N.lib().srlx_last_error().decode()


@pytest.mark.parametrize("args", [(1, (), 32, 0, 2, 1, 0, 1), (256, (512, 512), 512, 1, 32, 1 << 20, 256, 7)], ids=["lower", "upper"])
def test_create_dueling_passes_the_envelope_checks_at_its_bounds(args):
    """On the bounds themselves the argument checks pass: with a GPU the handle is created; without one the call fails at the device, with another message."""
    st, h = _create(*args)
    if st == 0:
        assert h.value
        N.check(N.lib().srlx_mlpq_destroy(h))
    else:
        assert not h.value and "mlpq_create_dueling" not in N.lib().srlx_last_error().decode()
