"""DQN on flat observations on the device engine (libsrlx srlx_mlpq_* / srlx_cartpole_step, device/mlpq.py): the MLP forward against torch float64, the fused
epsilon-greedy policy, the learner step against float64 autograd + torch's Adam, bit-reproducibility, the batch CartPole against envs/cartpole.py, and Runner.train()
end to end."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N

pytestmark = pytest.mark.gpu

SHAPES = [(4, (64, 64), 2), (4, (512,), 2), (17, (96, 32), 5)]


def _net(D, widths, A, seed=0):
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    torch.manual_seed(seed)
    net = EngineMLPQNet(D, (), widths, A).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.uniform_(-0.3, 0.3)
    return net


@pytest.mark.parametrize("D, widths, A", SHAPES)
def test_mlp_forward_matches_torch_float64(D, widths, A):
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    net = _net(D, widths, A)
    h = MLPQHandle(net, 4096)
    ref = _net(D, widths, A).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    for rows in (1, 33, 1024, 4096):
        x = torch.randn(rows, D, device="cuda")
        q = torch.zeros(rows, A, device="cuda")
        h.forward(rows, x, q=q)
        # the same rows through an offset table (the store's layout: row r at an arbitrary element offset)
        perm = torch.randperm(rows, device="cuda")
        q2 = torch.zeros(rows, A, device="cuda")
        h.forward(rows, x.data_ptr(), offsets=(perm * D).to(torch.int64), q=q2)
        with torch.no_grad():
            want = ref(x.double())
        torch.cuda.synchronize()
        err = float((q.double() - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()), (rows, err)
        assert torch.equal(q2, q[perm])


def test_fused_policy_selection():
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, A, E = 4, 5, 4096
    net = _net(D, (64,), A, seed=3)
    h = MLPQHandle(net, E)
    x = torch.randn(E, D, device="cuda")
    q = torch.zeros(E, A, device="cuda")
    acts = torch.zeros(E, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    # epsilon 0: argmax of the row
    h.forward(E, x, q=q, eps=torch.zeros(E, device="cuda"), seed=11, counter=counter, actions=acts)
    assert torch.equal(acts.long(), q.argmax(1))
    # = the stand-alone selection (srlx_policy_epsilon_greedy on srlx_rng_uniform(seed, counter, 2 E)) at epsilon 0.3, bit for bit
    eps = torch.full((E,), 0.3, device="cuda")
    counter.fill_(7)
    h.forward(E, x, q=q, eps=eps, seed=11, counter=counter, actions=acts)
    u = torch.zeros(2 * E, dtype=torch.float64, device="cuda")
    c2 = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    lib = N.lib()
    N.check(lib.srlx_rng_uniform(11, N.tptr(c2), 2 * E, N.tptr(u), N.torch_stream_ptr()))
    want = torch.zeros(E, dtype=torch.int32, device="cuda")
    N.check(lib.srlx_policy_epsilon_greedy(E, A, N.tptr(q), N.tptr(eps), N.tptr(u), None, N.tptr(want), N.torch_stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(acts, want)
    # epsilon 1: uniform over the actions (chi-square over ~10^6 draws), a fixed seed reproduces the actions
    ones = torch.ones(E, device="cuda")
    counts = torch.zeros(A, dtype=torch.int64, device="cuda")
    first = None
    for c in range(245):
        counter.fill_(c)
        h.forward(E, x, eps=ones, seed=5, counter=counter, actions=acts)
        counts += torch.bincount(acts.long(), minlength=A)
        if c == 0:
            first = acts.clone()
    n = float(counts.sum())
    chi2 = float((((counts.double() - n / A) ** 2) / (n / A)).sum())
    assert chi2 < 18.47, (chi2, counts.tolist())  # p = 0.001 at 4 degrees of freedom
    counter.fill_(0)
    h.forward(E, x, eps=ones, seed=5, counter=counter, actions=acts)
    assert torch.equal(acts, first)


def _reference():
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mlpq_reference

    return mlpq_reference


@pytest.mark.parametrize("widths", [(64, 64), (512,)])
@pytest.mark.parametrize("double_dqn", [True, False])
@pytest.mark.parametrize("B", [32, 256])
def test_learner_step_matches_float64_autograd_and_torch_adam(widths, double_dqn, B):
    """Target, loss and priorities within rel 1e-5 of float64 autograd; gradients within rel 1e-5 with an absolute slack of 1e-5 * max |g| of the tensor (entries
    that are sums of cancelling per-item terms); the post-Adam parameters equal torch.optim.Adam (float32) stepping on the kernel's own gradients to 1e-6."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, A, lr = 4, 2, 1e-3
    net, tgt = _net(D, widths, A, seed=1), _net(D, widths, A, seed=2)
    before = [p.detach().clone() for p in net.kernel_parameters()]
    h = MLPQHandle(net, 64, max_batch=B, lr=lr)
    ht = MLPQHandle(tgt, 64)
    g = torch.Generator(device="cuda").manual_seed(B)
    obs = torch.randn(2 * B, D, device="cuda", generator=g)
    off = torch.stack([torch.arange(B) * 2 * D, (torch.arange(B) * 2 + 1) * D], 1).to(torch.int64).cuda()
    act = torch.randint(0, A, (B, 1), device="cuda", generator=g, dtype=torch.int32)
    rew = torch.rand(B, 1, device="cuda", generator=g) * 2 - 1
    term = (torch.rand(B, 1, device="cuda", generator=g) < 0.2).float()
    term[3] = 1.0  # at least one terminal item
    w = torch.rand(B, device="cuda", generator=g) * 0.5 + 0.5
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    q0, target, loss, pri = torch.zeros(B, A, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(B, device="cuda")
    h.train_step(ht, B, obs.data_ptr(), off, act, rew, term, w, 0.99, double_dqn, False, steps, q0, target, loss, pri)
    torch.cuda.synchronize()
    o = obs.double().cpu().view(B, 2, D)
    ref = _reference().learner_step([b.double().cpu() for b in before], [p.detach().double().cpu() for p in tgt.kernel_parameters()], o[:, 0], o[:, 1],
                                    act.long().cpu().view(-1), rew.double().cpu().view(-1), term.double().cpu().view(-1), w.double().cpu(), 0.99, double_dqn)
    t_ref, l_ref, p_ref, q_ref, g_ref = ref.target, ref.loss, ref.priorities, ref.q0, ref.grads
    np.testing.assert_allclose(q0.double().cpu(), q_ref.cpu(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(target.double().cpu(), t_ref.cpu(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pri.double().cpu(), p_ref.cpu(), rtol=1e-5, atol=1e-6)
    assert float(loss) == pytest.approx(l_ref, rel=1e-5)
    grads = [p.grad.detach().clone() for p in net.kernel_parameters()]
    for gk, gr in zip(grads, g_ref):
        np.testing.assert_allclose(gk.double().cpu(), gr.cpu(), rtol=1e-5, atol=1e-5 * float(gr.abs().max()) + 1e-12)
    shadow = [b.clone().requires_grad_(True) for b in before]
    opt = torch.optim.Adam(shadow, lr=lr)
    for s, gk in zip(shadow, grads):
        s.grad = gk
    opt.step()
    for p, s in zip(net.kernel_parameters(), shadow):
        np.testing.assert_allclose(p.detach().cpu(), s.detach().cpu(), rtol=1e-6, atol=1e-7)


def _engine(seed=4, capacity=64 * 20):
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig, VectorQEngine

    cfg = VectorQConfig(batch_size=32, lr=1e-3, target_model_update_interval=10, memory_capacity=capacity, memory_warmup_size=256, hidden_sizes=(64, 64),
                        n_envs=64, seed=seed, epsilon=0.1)
    return VectorQEngine(cfg, 0)


def test_two_engines_with_one_seed_are_bit_identical():
    """50+ updates with the ring wrapping (20 lock-steps of capacity) and CartPole episodes ending; then the update as a captured graph."""
    out = []
    for _ in range(2):
        eng = _engine()
        for _ in range(60):
            eng.step(learner_updates=1)
        eng.capture_graphs(warm_actor=False)
        for _ in range(10):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        assert eng.train_count >= 50
        assert int(eng.env.episodes.sum()) > 64  # episodes ended and restarted
        out.append(([p.detach().clone() for p in eng.q_online.kernel_parameters()], eng.priorities.clone(), eng.loss.clone()))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def _cartpole_kernel(state, steps, episodes, needs_reset, actions, max_steps, seed):
    E = state.shape[0]
    d = "cuda"
    obs, rew = torch.zeros(E, 4, device=d), torch.zeros(E, device=d)
    term, done = torch.zeros(E, dtype=torch.uint8, device=d), torch.zeros(E, dtype=torch.uint8, device=d)
    N.check(N.lib().srlx_cartpole_step(E, N.tptr(state), N.tptr(steps), N.tptr(episodes), N.tptr(needs_reset), N.tptr(actions), max_steps, ctypes.c_uint64(seed),
                                       N.tptr(obs), N.tptr(rew) if needs_reset is not None else None, N.tptr(term) if needs_reset is not None else None,
                                       N.tptr(done) if needs_reset is not None else None, N.torch_stream_ptr()))
    torch.cuda.synchronize()
    return obs, rew, term, done


def test_device_cartpole_matches_the_host_environment():
    from simple_distributed_rl_amd.envs.cartpole import THETA_LIMIT, X_LIMIT, CartPole

    E, max_steps = 4096, 500
    rng = np.random.default_rng(0)
    s0 = np.stack([rng.uniform(-2.6, 2.6, E), rng.uniform(-3, 3, E), rng.uniform(-0.25, 0.25, E), rng.uniform(-3, 3, E)], 1)
    st0 = rng.integers(0, max_steps, E).astype(np.int32)
    st0[:64] = max_steps - 1  # truncation
    for a in (0, 1):
        state = torch.tensor(s0, device="cuda")
        steps = torch.tensor(st0, device="cuda")
        episodes = torch.zeros(E, dtype=torch.int32, device="cuda")
        obs, rew, term, done = _cartpole_kernel(state, steps, episodes, torch.zeros(E, dtype=torch.uint8, device="cuda"),
                                                torch.full((E,), a, dtype=torch.int32, device="cuda"), max_steps, 1)
        got = state.cpu().numpy()
        env = CartPole()
        for i in range(E):
            env.state, env.steps = s0[i].copy(), int(st0[i])
            o, r, te, tr = env.step(a)
            np.testing.assert_allclose(got[i], env.state, rtol=1e-12, atol=1e-15)
            assert np.array_equal(obs[i].cpu().numpy(), o) or np.allclose(obs[i].cpu().numpy(), o, rtol=1e-6)
            x, th = env.state[0], env.state[2]
            if min(abs(abs(x) - X_LIMIT), abs(abs(th) - THETA_LIMIT)) > 1e-9:
                assert bool(term[i]) == te and bool(done[i]) == (te or tr), i
            assert float(rew[i]) == r
    # resets: in range, reproduced by seed, another seed differs
    def resets(seed):
        state = torch.zeros(E, 4, dtype=torch.float64, device="cuda")
        steps, episodes = torch.full((E,), 7, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.int32, device="cuda")
        obs, *_ = _cartpole_kernel(state, steps, episodes, None, None, max_steps, seed)
        assert int(steps.abs().sum()) == 0 and bool((episodes == 1).all())
        return state, obs

    s1, o1 = resets(3)
    s2, _ = resets(3)
    s3, _ = resets(4)
    assert float(s1.abs().max()) <= 0.05 and torch.equal(s1, s2) and not torch.equal(s1, s3)
    assert torch.equal(o1, s1.float())
    # a lane that ended delivers only its next episode's first observation on the next lock-step
    state, steps = s1.clone(), torch.zeros(E, dtype=torch.int32, device="cuda")
    episodes = torch.ones(E, dtype=torch.int32, device="cuda")
    nr = torch.zeros(E, dtype=torch.uint8, device="cuda")
    nr[::3] = 1
    obs, rew, term, done = _cartpole_kernel(state, steps, episodes, nr, torch.ones(E, dtype=torch.int32, device="cuda"), max_steps, 3)
    m = nr.bool()
    assert bool((rew[m] == 0).all()) and bool((done[m] == 0).all()) and bool((steps[m] == 0).all()) and bool((episodes[m] == 2).all())
    assert float(state[m].abs().max()) <= 0.05 and not torch.equal(state[m], s1[m])
    assert bool((rew[~m] == 1).all()) and bool((steps[~m] == 1).all())


def _cartpole_cfg():
    from simple_distributed_rl_amd.algorithms import dqn

    rl = dqn.Config(batch_size=32, lr=0.001, target_model_update_interval=200, discount=0.99)
    rl.memory.set_replay_buffer()
    rl.memory.capacity, rl.memory.warmup_size = 100_000, 500
    rl.epsilon_scheduler.set_linear(1.0, 0.05, 3000)
    rl.hidden_block.set((64, 64))
    return rl


def test_runner_trains_cartpole_on_the_device():
    from simple_distributed_rl_amd.device.mlpq import CartPoleVecEnv, VectorQEngine
    from simple_distributed_rl_amd.utils.common import set_seed

    set_seed(3, enable_gpu=True)
    runner = srl.Runner("CartPole-v1", _cartpole_cfg())
    runner.set_device("cuda:0")
    runner.set_vector_envs(256)
    t0 = time.time()
    st = runner.train(max_train_count=6000, train_interval=8, enable_progress=False)
    assert runner.vector_reason == ""
    eng = runner._vector_actor.engine
    assert isinstance(eng, VectorQEngine) and isinstance(eng.env, CartPoleVecEnv)
    assert st.train_count >= 6000 and st.trainer.train_count >= 6000
    rewards = runner.evaluate(max_episodes=10, enable_progress=False)
    assert len(rewards) == 10 and np.mean(rewards) > 60, rewards
    assert time.time() - t0 < 300


class HostBox:
    """A host-stepped flat-observation environment with no device_vector: episodes of 7 steps, Box(3), 3 actions."""


def _register_host_box():
    from simple_distributed_rl_amd.base.env import registration
    from simple_distributed_rl_amd.base.env.base import EnvBase
    from simple_distributed_rl_amd.base.spaces.box import BoxSpace
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    class _HostBox(EnvBase):
        def __init__(self):
            super().__init__()
            self.t = 0

        action_space = property(lambda self: DiscreteSpace(3))
        observation_space = property(lambda self: BoxSpace((3,), -10.0, 10.0, np.float32))
        player_num = property(lambda self: 1)
        max_episode_steps = property(lambda self: 7)

        def reset(self, *, seed=None, **kwargs):
            self.t = 0
            return np.zeros(3, np.float32)

        def step(self, action):
            self.t += 1
            return np.array([self.t, int(action), 1.0], np.float32), float(action), False, self.t >= 7

        def backup(self, **kw):
            return self.t

        def restore(self, d, **kw):
            self.t = d

    globals()["HostBox"] = _HostBox
    registration.register("HostBox-test", __name__ + ":HostBox", {}, check_duplicate=False)


def test_host_stepped_box_env_runs_on_the_engine():
    from simple_distributed_rl_amd.algorithms import dqn
    from simple_distributed_rl_amd.device.vector_runner import HostVecEnv

    _register_host_box()
    rl = dqn.Config(batch_size=16, target_model_update_interval=10)
    rl.memory.set_replay_buffer()
    rl.memory.capacity, rl.memory.warmup_size = 2000, 64
    rl.hidden_block.set((32,))
    runner = srl.Runner("HostBox-test", rl)
    runner.set_device("cuda:0")
    runner.set_vector_envs(16)
    st = runner.train(max_steps=16 * 40, enable_progress=False)
    assert runner.vector_reason == ""
    eng = runner._vector_actor.engine
    assert isinstance(eng.env, HostVecEnv) and eng.env.float_obs
    assert st.total_step == 16 * 40 and st.train_count > 0
    # 40 lock-steps of 16 lanes, episodes of 7 steps + one reset-only lock-step each: 5 episodes per lane, 35 environment steps
    assert st.episode_count == 16 * 5 and st.shared_vars["env_steps_exact"] == 16 * 35


def test_auto_keeps_cartpole_dqn_on_the_plugin_path():
    from simple_distributed_rl_amd.utils.common import set_seed

    set_seed(3, enable_gpu=True)
    runner = srl.Runner("CartPole-v1", _cartpole_cfg())
    runner.set_device("cuda:0")
    runner.train(max_train_count=50, enable_progress=False)
    assert "set_vector_envs(n)" in runner.vector_reason
    assert runner.trainer.train_count > 0 and runner._vector_actor is None


def _golden():
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import dqn_vec_recipe as R

    return R, np.load(os.path.join(here, "golden", "train_step_dqn_vec.npz"))


@pytest.mark.parametrize("shape_key", ["h64x64", "h512"])
@pytest.mark.parametrize("double_dqn", [True, False])
def test_learner_step_against_the_reference_trainer(shape_key, double_dqn):
    """One srlx_mlpq_train_step against ONE Trainer.train() of the reference's DQN (oracle/gen_golden_dqn_vec.py; weights and batch from tests/dqn_vec_recipe.py):
    target, online Q of s_0, loss and priorities within rel 1e-5; every p.grad within rel 1e-5 with an absolute slack of 1e-5 * max |g| of the tensor (entries that
    are sums of cancelling per-item terms); every parameter after Adam within rel 1e-5 (+ 1e-7), except entries whose reference gradient is below 1e-4 * max |g|:
    there the first Adam step (about lr * g / |g|) turns on the sign and size of a cancelling sum, and only the bound 2 lr holds."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    R, z = _golden()
    hidden, name = R.SHAPES[shape_key], R.case_name(shape_key, double_dqn)
    g = lambda k: z[f"{name}.{k}"]  # noqa: E731
    net = EngineMLPQNet(R.D, (), hidden, R.A).cuda().load_reference_state_dict({k: torch.tensor(v) for k, v in R.recipe_state_dict(hidden, R.SEED_ONLINE).items()})
    tgt = EngineMLPQNet(R.D, (), hidden, R.A).cuda().load_reference_state_dict({k: torch.tensor(v) for k, v in R.recipe_state_dict(hidden, R.SEED_TARGET).items()})
    assert [(k, tuple(v.shape)) for k, v in net.reference_state_dict().items()] == R.keys_shapes(hidden)
    lr = float(g("lr"))
    h = MLPQHandle(net, 64, max_batch=R.B, lr=lr)
    ht = MLPQHandle(tgt, 64)
    s0, s1, actions, reward, undone, weights = R.make_items()
    B = R.B
    obs = torch.tensor(np.stack([s0, s1], 1).reshape(2 * B, R.D), device="cuda")
    off = torch.stack([torch.arange(B) * 2 * R.D, (torch.arange(B) * 2 + 1) * R.D], 1).to(torch.int64).cuda()
    act = torch.tensor(actions, device="cuda").view(B, 1)
    rew = torch.tensor(reward, device="cuda").view(B, 1)
    term = torch.tensor(1.0 - undone, device="cuda").view(B, 1)
    w = torch.tensor(weights, device="cuda")
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    q0, target, loss, pri = torch.zeros(B, R.A, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(B, device="cuda")
    h.train_step(ht, B, obs.data_ptr(), off, act, rew, term, w, float(g("discount")), double_dqn, False, steps, q0, target, loss, pri)
    torch.cuda.synchronize()
    np.testing.assert_allclose(q0.cpu().numpy(), g("q0"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(target.cpu().numpy(), g("target_q"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss), float(g("loss")), rtol=1e-5)
    np.testing.assert_allclose(pri.cpu().numpy(), g("priorities"), rtol=1e-5, atol=1e-5 * float(np.abs(g("target_q")).max()))
    ps = dict(zip([k for k, _ in R.keys_shapes(hidden)], net.kernel_parameters()))
    for k, p in ps.items():
        gr, gmax = g("grad." + k), float(np.abs(g("grad." + k)).max())
        np.testing.assert_allclose(p.grad.cpu().numpy(), gr, rtol=1e-5, atol=1e-5 * gmax, err_msg=k)
        after, want = p.detach().cpu().numpy(), g("after." + k)
        firm = np.abs(gr) >= 1e-4 * gmax
        np.testing.assert_allclose(after[firm], want[firm], rtol=1e-5, atol=1e-7, err_msg=k)
        assert np.abs(after[~firm] - want[~firm]).max(initial=0.0) <= 2 * lr * (1 + 1e-3), k


def test_engine_trains_with_a_batch_above_the_fused_draw():
    """B = 128: the draw and the gather run as two launches (srlx_per_sample_keyed + srlx_store_gather_train on the float32 ring).  The gathered offsets address
    ring rows whose online Q equals what the update reported for s_0, and every item's action / terminal flag is well-formed."""
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig, VectorQEngine

    cfg = VectorQConfig(batch_size=128, lr=1e-3, target_model_update_interval=5, memory_capacity=64 * 30, memory_warmup_size=512, hidden_sizes=(64, 64),
                        n_envs=64, seed=6, epsilon=0.5)
    eng = VectorQEngine(cfg, 0)
    before = [p.detach().clone() for p in eng.q_online.kernel_parameters()]
    for _ in range(40):
        eng.actor_step()
        if not eng.replay.is_warmup_needed():
            q_before = [p.detach().clone() for p in eng.q_online.kernel_parameters()]
            eng.learner_step()
    torch.cuda.synchronize()
    assert eng.train_count >= 30 and eng.replay.B == 128
    info = eng.info()
    assert math.isfinite(info["loss"]) and info["loss"] > 0
    r = eng.replay
    b = r.batch
    assert bool((b.indices >= r.capacity - 1).all()) and bool((b.indices < 2 * r.capacity - 1).all())
    assert len(set(b.indices.tolist())) == 128  # the uniform replay draws without replacement
    assert bool(((b.actions >= 0) & (b.actions < 2)).all()) and bool(((b.terminated == 0) | (b.terminated == 1)).all())
    # the s_0 rows the offsets point at, through the pre-update weights of the last update, give the Q the update reported
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    net = EngineMLPQNet(4, (), (64, 64), 2).cuda()
    with torch.no_grad():
        for p, v in zip(net.kernel_parameters(), q_before):
            p.copy_(v)
    q = torch.zeros(128, 2, device="cuda")
    MLPQHandle(net, 128).forward(128, r.obs_base, offsets=r.frame_off_all[:, 0, 0].contiguous(), q=q)
    torch.cuda.synchronize()
    assert torch.equal(q, eng.q0)
    assert not all(torch.equal(a, c) for a, c in zip(before, eng.q_online.kernel_parameters()))
