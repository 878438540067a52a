"""The device engine of Agent57 (the LSTM one; device/agent57.py) on the GPU, with the golden's small configuration on TinyImg and on
CartPole-v1's flat observations at E = 4: window counts against the ledger, finite losses, recurrent-state alignment of the stored windows, seeded
determinism, and the route through `Runner.train()`.  (tests/test_agent57_engine_gpu.py is the Agent57_light engine's file.)"""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E = 4
ENVS = {"TinyImg": dict(ep_len=5, seed=3), "CartPole-v1": {}}


def _config(intrinsic, warmup=8):
    from simple_distributed_rl_amd.algorithms import agent57

    rl = agent57.Config(batch_size=8, actor_num=4, target_model_update_interval=5, lr_ext=0.001, lr_int=0.002, lstm_units=16, burnin=2, sequence_length=3,
                        enable_intrinsic_reward=intrinsic)
    rl.window_length = 1
    rl.memory.capacity, rl.memory.warmup_size = 1000, warmup
    rl.hidden_block.set_dueling_network((16,))
    rl.episodic_memory_capacity = 64
    return rl


def _register():
    from simple_distributed_rl_amd.base.env import registration
    from test_plugin_surface import TinyImg  # noqa: F401

    registration.register("TinyImg", "test_plugin_surface:TinyImg", check_duplicate=False)


def _engine(env_id, intrinsic, seed, warmup=8, env_kw=None):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.base.context import RunContext
    from simple_distributed_rl_amd.base.env.registration import make
    from simple_distributed_rl_amd.device.agent57 import Agent57Engine
    from simple_distributed_rl_amd.device.vector_runner import HostVecEnv
    from simple_distributed_rl_amd.utils.common import set_seed

    _register()
    set_seed(seed, enable_gpu=True)
    rl = _config(intrinsic, warmup)
    env_config = srl.EnvConfig(env_id, kwargs=dict(ENVS[env_id] if env_kw is None else env_kw))
    rl.setup(make(env_config))
    ctx = RunContext()
    ctx.seed = seed

    def batch_env(ring):
        env = HostVecEnv(env_config, E, ring.dev, seed, float_obs=True)
        env.setup(ctx)
        return env

    return Agent57Engine(rl, E, 0, seed=seed, env=batch_env, context=ctx)


@pytest.mark.parametrize("env_id", list(ENVS))
@pytest.mark.parametrize("intrinsic", [False, True], ids=["ext", "ext+int"])
def test_memory_length_is_the_ledgers_window_count_and_training_runs(env_id, intrinsic):
    eng = _engine(env_id, intrinsic, seed=5)
    led, predicted, ended = eng.store.ledger, 0, 0
    for _ in range(30):
        first = eng._first_host.copy()
        eng.step(1)
        done = eng._first_host  # (this lock-step's done lanes are the next one's first lanes)
        predicted += int(led.window_counts(first, done).sum())
        ended += int(done.sum())
        assert eng.memory.length() == predicted == led.serial
    assert ended >= 2 and predicted > 30 * E - 2 * ended  # flush windows were counted
    assert eng.train_count >= 20
    info = eng.info()
    keys = ("ext_loss", "int_loss", "emb_loss", "lifelong_loss") if intrinsic else ("ext_loss",)
    for k in keys:
        assert np.isfinite(info[k]), k


@pytest.mark.parametrize("env_id", list(ENVS))
def test_stored_recurrent_state_lines_up_with_the_stored_inputs(env_id):
    """Two windows of one lane with no episode boundary between them, the second starting j steps later: the online network run from the first window's stored
    state over its first j inputs must arrive at the second window's stored state (1e-5 relative: the acting pass ran at batch E, this one runs at batch 1)."""
    kw = dict(ep_len=40, seed=3) if env_id == "TinyImg" else None
    eng = _engine(env_id, True, seed=7, warmup=900, env_kw=kw)  # (training held off: the networks stay what they were while the lanes acted)
    L, j = eng.L, 2
    lane, ages = None, None
    for _ in range(40):
        eng.step(1)
        ages = eng.store.ledger.age
        if (ages >= L + j).any():  # a lane whose episode is old enough for two windows j steps apart whose heads lie after its first observation
            lane = int(np.argmax(ages >= L + j))
            break
    assert lane is not None and eng.train_count == 0
    t = eng.store.ledger.t - 1
    sb = eng.store.gather(np.array([[lane, t - j, 0], [lane, t, 0]], np.int64))
    p = eng.parameter
    onehot = eng.action_eye[sb.act_idx]
    actor = eng.actor_eye[sb.actor].unsqueeze(1).expand(2, L, -1)
    assert int(sb.actor[0]) == int(sb.actor[1])
    in_ = [x[0:1, :j] for x in (sb.states, sb.r_ext.unsqueeze(-1), sb.r_int.unsqueeze(-1), onehot, actor)]
    for net, h, c in ((p.q_ext_online, sb.h_ext, sb.c_ext), (p.q_int_online, sb.h_int, sb.c_int)):
        assert h[0].abs().sum() > 0  # (an unpadded head: a state the network produced)
        with torch.no_grad():
            net.eval()
            _, (h_n, c_n) = net(in_, (h[0:1].unsqueeze(0).contiguous(), c[0:1].unsqueeze(0).contiguous()))
        np.testing.assert_allclose(h_n[0, 0].cpu().numpy(), h[1].cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c_n[0, 0].cpu().numpy(), c[1].cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_two_engines_with_one_seed_agree_bit_for_bit():
    def run():
        eng = _engine("TinyImg", True, seed=11)
        actions = []
        while eng.replay.is_warmup_needed():  # up to the first update
            eng.step(0)
            actions.append(eng.actions.cpu().numpy().copy())
        random.seed(11)
        serials = list(eng.memory.memory.sample(8, 0)[0])
        st = eng.store
        rings = [x.cpu().numpy().copy() for x in (st.frames, st.scalars, st.invalid, st.hidden)]
        return np.array(actions), rings, serials, st.ledger.t

    a1, r1, s1, t1 = run()
    a2, r2, s2, t2 = run()
    assert t1 == t2 and len(a1) >= 2
    np.testing.assert_array_equal(a1, a2)
    for x, y in zip(r1, r2):
        np.testing.assert_array_equal(x[:t1], y[:t1])  # (rows no lock-step has written are torch.empty)
    assert s1 == s2


def _runner(vector_envs):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.utils.common import set_seed

    _register()
    set_seed(2, enable_gpu=True)
    runner = srl.Runner(srl.EnvConfig("TinyImg", kwargs=dict(ep_len=5, seed=1)), _config(True))
    runner.set_device("cuda:0")
    runner.set_seed(2)
    runner.set_vector_envs(vector_envs)
    return runner


def test_runner_trains_on_the_engine_under_explicit_lanes():
    runner = _runner(E)
    before = {k: v.detach().clone() for k, v in runner.parameter.q_ext_online.state_dict().items()}
    st = runner.train(max_train_count=3, enable_progress=False)
    assert runner.vector_reason == "" and st.train_count >= 3 and st.end_reason == "max_train_count over."
    after = runner.parameter.q_ext_online.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)  # the Runner's Parameter was trained in place
    assert st.total_step % E == 0 and st.total_step >= 2 * E  # whole lock-steps of E lanes (train_interval 1 owes E updates per lock-step once 8 windows are in)
    rewards = runner.evaluate(max_episodes=2, enable_progress=False)  # the plugin path plays the trained Parameter
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)


def test_runner_keeps_the_plugin_path_under_auto():
    runner = _runner("AUTO")
    st = runner.train(max_train_count=2, enable_progress=False)
    assert st.train_count == 2
    assert "set_vector_envs(n)" in runner.vector_reason and "Agent57" in runner.vector_reason


def test_train_mp_keeps_agent57_off_the_engine(monkeypatch):
    """`Runner.train_mp()` hands non-DQN engine kinds to `train_mp_on_engine`; Agent57's engine is one process on one GPU, so the run must reach the plugin's
    multi-process path with the stated reason.  Both destinations are intercepted: entering the engine's fails the test, the plugin's ends the run at once."""
    from simple_distributed_rl_amd.base.run import play_mp, play_mp_memory
    from simple_distributed_rl_amd.device import mp_runner
    from simple_distributed_rl_amd.device import vector_runner as vr

    class ReachedPlugin(Exception):
        pass

    def engine_path(*a, **kw):
        raise AssertionError("train_mp handed Agent57 to train_mp_on_engine")

    def plugin_path(*a, **kw):
        raise ReachedPlugin()

    monkeypatch.setattr(mp_runner, "train_mp_on_engine", engine_path)
    monkeypatch.setattr(play_mp_memory, "train", plugin_path)
    monkeypatch.setattr(play_mp, "train", plugin_path)
    runner = _runner(E)
    assert vr.why_not_vector(runner.context, runner.env, _set_up(runner)) == ""  # (nothing but the guard keeps this pair off the engine)
    for mp_memory in (True, False):
        with pytest.raises(ReachedPlugin):
            runner.train_mp(actor_num=1, max_train_count=1, enable_mp_memory=mp_memory, enable_progress=False)
        assert runner.vector_reason == vr.AGENT57_MP_REASON


def _set_up(runner):
    runner.setup_rl_config()
    runner.context.setup_device()
    return runner.rl_config


def test_runner_refuses_more_lanes_than_the_memory_holds_with_a_reason():
    runner = _runner(E)
    runner.rl_config.memory.capacity = 20  # 4 lanes of window 6 emit up to 24 windows in one lock-step
    st = runner.train(max_train_count=1, enable_progress=False)
    assert st.train_count == 1 and "more than memory.capacity 20" in runner.vector_reason
