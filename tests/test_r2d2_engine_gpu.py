"""The device engine of R2D2 (device/r2d2.py) on the GPU at E = 4, burn-in 2, S = 3, H = 16, dueling (32,), batch 4, on the small corridor of
tests/r2d2_lanes_reference.py: window counts against the ledger, the stored (action, mu) against the policy mirror, the stored recurrent state against a fresh
forward, the batch the trainer receives against `SequenceBatch.from_items` of the host model's windows, seeded determinism, and the route through
`Runner.train()`."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, A = 4, 4
ENV_KW = dict(n_actions=A, starts=(1, 3, 0, 4, 2), budgets=(9, 1, 4, 9, 2))


def _config(warmup=4, **kw):
    from simple_distributed_rl_amd.algorithms import r2d2

    c = r2d2.Config(batch_size=4, burnin=2, sequence_length=3, lstm_units=16, epsilon=0.5, target_model_update_interval=5, **kw)
    c.hidden_block.set_dueling_network((32,))
    c.memory.set_proportional()
    c.memory.capacity, c.memory.warmup_size = 256, warmup
    return c


def _engine(seed, warmup=4, masked=True, **engine_kw):
    import simple_distributed_rl_amd as srl
    from r2d2_lanes_reference import register_corridor
    from simple_distributed_rl_amd.base.context import RunContext
    from simple_distributed_rl_amd.base.env.registration import make
    from simple_distributed_rl_amd.device.r2d2 import MaskedHostVecEnv, R2D2Engine
    from simple_distributed_rl_amd.device.vector_runner import HostVecEnv
    from simple_distributed_rl_amd.utils.common import set_seed

    register_corridor()
    set_seed(seed, enable_gpu=True)
    rl = _config(warmup)
    env_config = srl.EnvConfig("R2D2Corridor-v0", kwargs=dict(ENV_KW))
    rl.setup(make(env_config))
    ctx = RunContext()
    ctx.seed = seed

    def batch_env(ring):
        env = (MaskedHostVecEnv if masked else HostVecEnv)(env_config, E, ring.dev, seed, float_obs=True)
        env.setup(ctx)
        return env

    return R2D2Engine(rl, E, 0, seed=seed, env=batch_env, context=ctx, **engine_kw)


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "no-masks"])
def test_memory_length_is_the_ledgers_window_count_and_training_runs(masked):
    eng = _engine(seed=5, masked=masked)
    assert eng.masked == masked
    led, predicted, ended = eng.store.ledger, 0, 0
    for _ in range(30):
        first = eng._first_host.copy()
        eng.step(1)
        done = eng._first_host  # (this lock-step's done lanes are the next one's first lanes)
        predicted += int(led.window_counts(first, done).sum())
        ended += int(done.sum())
        assert eng.memory.length() == predicted == led.serial
    assert ended >= 2 and predicted == 30 * E - (ended - int(eng._first_host.sum())) + (eng.S - 1) * ended  # the lanes' steps + S - 1 flush windows per ended episode
    assert eng.train_count >= 20 and np.isfinite(eng.info()["loss"])
    assert eng.parameter.q_online.lstm_path == "srlx"
    assert (eng.store.any_invalid, eng.mask is not None) == (masked, masked)


def _rings(eng):
    st = eng.store
    return [x.cpu().numpy().copy() for x in (st.frames, st.scalars, st.invalid, st.hidden)]


def test_stored_action_and_mu_equal_the_mirror_and_the_stored_state_a_fresh_forward():
    from r2d2_lanes_reference import policy_mirror

    eng = _engine(seed=7, warmup=250, lane_epsilon=[0.0, 0.1, 0.5, 1.0])  # (training held off: the network stays what it was while the lanes acted)
    eng.record = []
    steps = 30
    for _ in range(steps):
        eng.step(1)
    assert eng.train_count == 0 and eng.store.ledger.ring_len > steps + 1  # (nothing was overwritten)
    frames, scalars, invalid, hidden = _rings(eng)
    assert any(r["mask"].any() for r in eng.record)
    net, checked = eng.parameter.q_online, 0
    for n, r in enumerate(eng.record):
        np.testing.assert_array_equal(r["eps"], np.array([0.0, 0.1, 0.5, 1.0], np.float32))
        want_a, want_mu = policy_mirror(r["q"], r["eps"], r["u"], r["mask"])
        np.testing.assert_array_equal(r["actions"], want_a)
        np.testing.assert_array_equal(r["mu"].view(np.uint32), want_mu.view(np.uint32))
        p = n + 1  # the position this lock-step pushed
        for e in range(E):
            age = int(scalars[p, e, 4])
            assert (age == 0) == bool(r["first"][e])
            if age == 0:
                assert scalars[p, e, 1].view(np.float32) == np.float32(1.0 / A) and not hidden[p, e].any()
                continue
            assert scalars[p, e, 0] == want_a[e] and scalars[p, e, 1].view(np.uint32) == want_mu[e].view(np.uint32)
            np.testing.assert_array_equal(invalid[p, e], r["next_mask"][e])
            # (h, c) before o_p: a fresh forward from the zero state over the episode's observations so far, o_{p - age} .. o_{p - 1}
            obs = torch.from_numpy(frames[p - age : p, e, : eng.store.frame_elems]).to(eng.dev).view(1, age, *eng.obs_shape)
            with torch.no_grad():
                net.eval()
                _, (h, c) = net(obs, net.get_initial_state(1, eng.dev))
            np.testing.assert_allclose(h[0, 0].cpu().numpy(), hidden[p, e, 0], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(c[0, 0].cpu().numpy(), hidden[p, e, 1], rtol=1e-5, atol=1e-5)
            checked += 1
    assert checked > steps * E // 2


def _model_windows(eng):
    """The host model fed with what the engine's lock-steps recorded; its windows in serial order."""
    from r2d2_lanes_reference import R2D2LanesModel

    rec = eng.record
    model = R2D2LanesModel(E, eng.L, eng.S, A, eng.H, eng.obs_shape, eng.store.seed)
    z = np.zeros(E, np.float32)
    assert model.push(rec[0]["obs"], z, z, z, z, np.zeros((E, 2, eng.H), np.float32), np.ones(E, bool), np.zeros(E, bool), invalid=rec[0]["mask"]) == []
    windows = []
    for r in rec:
        windows += model.push(r["next_obs"], r["actions"], r["mu"], r["reward"], r["terminated"], r["hidden"], r["first"], r["done"].astype(bool) & ~r["first"],
                              invalid=r["next_mask"])
    return windows


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "no-masks"])
def test_the_trainer_receives_from_items_of_the_host_models_windows(masked):
    from r2d2_lanes_reference import as_item
    from simple_distributed_rl_amd.algorithms import r2d2

    eng = _engine(seed=9, warmup=4, masked=masked)
    eng.record = []
    seen = []
    inner_gather, inner_train = eng.store.gather_serials, eng.trainer._train_on_batch

    def gather_serials(serials):
        seen.append([list(int(s) for s in serials)])
        return inner_gather(serials)

    def train_on_batch(sb, w):
        seen[-1].append(sb)
        return inner_train(sb, w)

    eng.store.gather_serials, eng.trainer._train_on_batch = gather_serials, train_on_batch
    for _ in range(25):
        eng.step(1)
    torch.cuda.synchronize()
    windows = _model_windows(eng)
    assert len(windows) == eng.store.ledger.serial and len(seen) >= 20 and eng.train_count == len(seen)
    flush = 0
    for serials, sb in seen:
        assert len(serials) == 4
        want = r2d2.SequenceBatch.from_items([as_item(windows[s]) for s in serials], A, eng.dev)
        flush += sum(windows[s]["desc"][2] > 0 for s in serials)
        for f in ("states", "actions", "probs", "rewards", "dones"):
            a, b = getattr(sb, f), getattr(want, f)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f
        for a, b in zip(sb.hidden_states, want.hidden_states):
            assert a.shape == b.shape and torch.equal(a, b)
        if not masked:
            assert sb.invalid_actions is None and want.invalid_actions is None
        elif want.invalid_actions is None:  # (no sampled window has an invalid action: the ring hands out the all-zero mask, which masks nothing)
            assert not sb.invalid_actions.any()
        else:
            assert torch.equal(sb.invalid_actions, want.invalid_actions)
    assert flush > 0  # flush windows were sampled


def test_two_engines_with_one_seed_agree_bit_for_bit():
    def run():
        eng = _engine(seed=11, warmup=40)
        actions = []
        while eng.replay.is_warmup_needed():  # up to the first update
            eng.step(0)
            actions.append(eng.actions.cpu().numpy().copy())
        random.seed(11)
        serials = list(eng.memory.memory.sample(4, 0)[0])
        return np.array(actions), _rings(eng), serials, eng.store.ledger.t

    a1, r1, s1, t1 = run()
    a2, r2, s2, t2 = run()
    assert t1 == t2 and len(a1) >= 5
    np.testing.assert_array_equal(a1, a2)
    r1[0], r2[0] = r1[0][..., :3], r2[0][..., :3]  # (a frame row is 3 floats of a stride of 4: the fourth is never written)
    for x, y in zip(r1, r2):
        np.testing.assert_array_equal(x[:t1], y[:t1])  # (rows no lock-step has written are torch.empty)
    assert s1 == s2


# ---- the route -------------------------------------------------------------------------------------------------------------------------------------------------------
def _runner(vector_envs, config=None):
    import simple_distributed_rl_amd as srl
    from r2d2_lanes_reference import register_corridor
    from simple_distributed_rl_amd.utils.common import set_seed

    register_corridor()
    set_seed(2, enable_gpu=True)
    runner = srl.Runner(srl.EnvConfig("R2D2Corridor-v0", kwargs=dict(ENV_KW)), config or _config())
    runner.set_device("cuda:0")
    runner.set_seed(2)
    runner.set_vector_envs(vector_envs)
    return runner


def test_runner_trains_on_the_engine_under_explicit_lanes_and_evaluates_on_the_plugin_path():
    from simple_distributed_rl_amd.device.r2d2 import R2D2Engine

    runner = _runner(E)
    before = {k: v.detach().clone() for k, v in runner.parameter.q_online.state_dict().items()}
    st = runner.train(max_train_count=3, enable_progress=False)
    assert runner.vector_reason == "" and st.train_count == 3 and st.end_reason == "max_train_count over."
    eng = runner._vector_actor.engine
    assert isinstance(eng, R2D2Engine) and eng.masked and eng.train_count == 3
    after = runner.parameter.q_online.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)  # the Runner's Parameter was trained in place
    assert st.total_step % E == 0 and st.total_step >= E  # whole lock-steps of E lanes (the first one's 4 windows already fill the warm-up of 4)
    rewards = runner.evaluate(max_episodes=2, enable_progress=False)  # the plugin path plays the trained Parameter
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)
    # a second train() continues on the same engine and memory
    held = eng.memory.length()
    st = runner.train(max_train_count=2, enable_progress=False)
    assert runner._vector_actor.engine is eng and eng.memory.length() > held and st.train_count == 2 and runner.vector_reason == ""


def test_runner_keeps_the_plugin_path_under_auto():
    runner = _runner("AUTO")
    st = runner.train(max_train_count=2, enable_progress=False)
    assert st.train_count == 2 and runner.vector_reason == "no device engine for algorithm 'R2D2'"
    assert runner._vector_actor is None


def test_train_mp_keeps_r2d2_off_the_engine(monkeypatch):
    """Both destinations of `Runner.train_mp()` are intercepted: entering the engine's fails the test, the plugin's ends the run at once."""
    from simple_distributed_rl_amd.base.run import play_mp, play_mp_memory
    from simple_distributed_rl_amd.device import mp_runner
    from simple_distributed_rl_amd.device import vector_runner as vr

    class ReachedPlugin(Exception):
        pass

    def engine_path(*a, **kw):
        raise AssertionError("train_mp handed R2D2 to train_mp_on_engine")

    def plugin_path(*a, **kw):
        raise ReachedPlugin()

    monkeypatch.setattr(mp_runner, "train_mp_on_engine", engine_path)
    monkeypatch.setattr(play_mp_memory, "train", plugin_path)
    monkeypatch.setattr(play_mp, "train", plugin_path)
    runner = _runner(E)
    for mp_memory in (True, False):
        with pytest.raises(ReachedPlugin):
            runner.train_mp(actor_num=1, max_train_count=1, enable_mp_memory=mp_memory, enable_progress=False)
        assert runner.vector_reason == vr.R2D2_MP_REASON


def test_runner_refuses_lane_counts_the_engine_cannot_serve_with_their_reasons():
    c = _config()
    c.memory.capacity = 10  # 4 lanes of sequence length 3 emit up to 12 windows in one lock-step
    runner = _runner(E, c)
    st = runner.train(max_train_count=1, enable_progress=False)
    assert st.train_count == 1 and "more than memory.capacity 10" in runner.vector_reason and runner._vector_actor is None
    runner = _runner(257)
    st = runner.train(max_train_count=1, enable_progress=False)
    assert st.train_count == 1 and "at most 256 rows" in runner.vector_reason and runner._vector_actor is None


@pytest.mark.slow
def test_r2d2_engine_learns_the_grid():
    """Opt-in (SRLX_RUN_SLOW=1): the plugin run's own bar on the engine -- 3000 updates on Grid reach a mean evaluation return above 0.3 over 20 episodes."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import r2d2
    from simple_distributed_rl_amd.utils.common import set_seed

    set_seed(1, enable_gpu=True)
    c = r2d2.Config(batch_size=32, burnin=2, sequence_length=4, lstm_units=32, lr=0.001, target_model_update_interval=200, discount=0.95)
    c.hidden_block.set_dueling_network((64,))
    c.memory.set_proportional()
    c.memory.capacity, c.memory.warmup_size = 10_000, 200
    r = srl.Runner("Grid", c)
    r.set_device("cuda:0")
    r.set_vector_envs(16)
    r.train(max_train_count=3000, enable_progress=False)
    assert r.vector_reason == ""
    rewards = r.evaluate(max_episodes=20, enable_progress=False)
    print(f"R2D2-ENGINE-LEARN Grid: mean return {np.mean(rewards):.3f} over 20 episodes after 3000 updates on 16 lanes")
    assert np.mean(rewards) > 0.3, rewards
