"""The V-PPO device engine's Normal head on the GPU (device/vppo_engine.py: VppoNormalEngine): device Pendulum, E = 16 lanes, batches of 8, warm-up
32.  What the lanes drew against the mirror (tests/vppo_normal_reference.py), the environments against the mirror's Pendulum, the item ring against the mirror
replayed from the record, the first ratio, one update against the plugin's own `train_on_batch` on a cloned Parameter, two fresh engines against each other, the
trained Parameter played by the Runner, a host-stepped Pendulum-v1, the refusals' text, and the categorical engine as it was."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd.algorithms import ppo_v

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_normal_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

E, B, WARMUP, STEPS = 16, 8, 32, 5  # episodes of 5 steps: 60 lock-steps close ten of them per lane
ITEM_VIEWS = ("item_s", "item_s2", "item_action", "item_logp", "item_reward", "item_not_terminated", "item_total")
F32 = np.float32


def _runner(seed=0, env="Pendulum-v1", **kw):
    cfg = ppo_v.Config(batch_size=B, **kw)
    cfg.memory.warmup_size = WARMUP
    cfg.memory.capacity = 2000
    runner = srl.Runner(env, cfg)
    runner.set_device("cuda:0")
    torch.manual_seed(seed)
    runner.make_parameter()
    return runner


def _engine(seed=0, n_envs=E, env=None, max_episode_steps=STEPS, **kw):
    from simple_distributed_rl_amd.device.vppo_engine import VppoNormalEngine

    runner = _runner(seed, **kw)
    eng = VppoNormalEngine(runner.rl_config, n_envs, seed=seed, parameter=runner.make_parameter(), env=env, max_episode_steps=max_episode_steps)
    assert eng.parameter is runner.make_parameter()
    return runner, eng


def _params(p):
    return [t.detach().clone() for t in p.net.parameters()]


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _replay_record(eng):
    """The mirror's lanes fed the engine's record."""
    lanes = M.NormalLanes(eng.E, eng.K, eng.replay.capacity, eng.cfg.discount, eng.replay.R - 2, eng.first_obs.cpu().numpy())
    for rec in eng.record:
        lanes.push(rec["actions"], rec["logp"], rec["reward"], rec["terminated"], rec["done"], rec["next_obs"])
    return lanes


def test_lanes_draw_the_mirrors_actions_and_the_ring_is_the_mirrors():
    runner, eng = _engine(seed=3, epsilon=0.3)
    assert eng.K == 1 and eng.D == 3 and eng.replay.action_dim == 1 and eng.low.tolist() == [-2.0] and eng.high.tolist() == [2.0]
    eng.record = []
    steps = 60
    for _ in range(steps):
        eng.actor_step()
    torch.cuda.synchronize()
    assert eng.lock_steps == steps and eng.total_env_steps == steps * E and int(eng.policy_counter.item()) == steps
    net64 = copy.deepcopy(eng.parameter.net).double().cpu()
    obs = [eng.first_obs.cpu().numpy()] + [r["next_obs"] for r in eng.record[:-1]]
    pend = M.PendulumLanes(E, STEPS, eng.seed)
    assert int(_ulps(pend.reset(), obs[0]).max()) <= 1
    randoms, worst_a, differ, worst_state = 0, 0, 0, 0.0
    for t, rec in enumerate(eng.record):
        assert rec["counter"] == t
        with torch.no_grad():
            dist = net64(torch.from_numpy(obs[t]).double())[1]
        np.testing.assert_allclose(rec["loc"], dist.mean().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(np.exp(rec["log_scale"].astype(np.float64)), dist.stddev().numpy(), rtol=1e-5, atol=1e-6)
        u0, ua, ub = M.uniforms(eng.seed ^ 0xAC7, t, E, 1)
        np.testing.assert_allclose(rec["z"], M.box_muller(ua, ub), rtol=1e-12, atol=1e-14)
        # (the scale: the device's own float32 exponential of the kernel's log-scale, as in tests/test_vppo_act_normal_gpu.py: _device_exp)
        dev_scale = torch.exp(torch.from_numpy(rec["log_scale"]).cuda()).cpu().numpy()
        actions, random, l, ls, sd, _ = M.act(rec["loc"], rec["log_scale"], eng.seed ^ 0xAC7, t, 0.3, 0.5, z=rec["z"], scale=dev_scale)
        assert np.array_equal(random, u0 < 0.3)
        d = _ulps(rec["actions"], actions)
        worst_a, differ = max(worst_a, int(d.max())), differ + int((d > 0).sum())
        # on the epsilon branch the scale is a constant: the action and the log-probability are the mirror's to the bit given the kernel's z
        assert np.array_equal(_i32(rec["actions"][random]), _i32(actions[random]))
        assert np.array_equal(_i32(rec["logp"][random]), _i32(M.logp_f32(rec["actions"], l, ls, sd, True)[random]))
        assert int(_ulps(rec["env_actions"], M.env_action(rec["actions"], [-2.0], [2.0], True)).max()) <= 1
        assert bool((np.abs(rec["env_actions"]) <= 2.0).all())
        randoms += int(random.sum())
        # the environments: the mirror's Pendulum carries its own float64 state through the whole run, fed the engine's torques
        m_obs, m_reward, m_term, m_done = pend.step(rec["env_actions"][:, 0], rec["first"])
        assert np.array_equal(m_done, rec["done"]) and not rec["terminated"].any()
        assert int(_ulps(m_obs, rec["next_obs"]).max()) <= 1 and int(_ulps(m_reward, rec["reward"]).max()) <= 1
    torch.cuda.synchronize()
    state = eng.env.state.cpu().numpy()
    worst_state = float(np.abs(state - np.array(pend.state)).max())
    assert worst_state <= 1e-11, "sixty steps of drift apart (each step within 1e-12; resets every six lock-steps restart it)"
    assert 0 < randoms < steps * E
    lanes = _replay_record(eng)
    added, err = eng.replay.count()
    assert err == 0 and added == lanes.ring.added == E * STEPS * (steps // (STEPS + 1))
    n = lanes.ring.length()
    for name, w in zip(ITEM_VIEWS, lanes.slots()):
        got = eng.replay.view(name).numpy()[:n]
        assert np.array_equal(_i32(got), _i32(w.reshape(got.shape))), name
    print(f"VPPO-NORMAL-ENGINE {added} items from {steps} lock-steps, {randoms} noise draws; {differ} of {steps * E} actions differ from the mirror (worst {worst_a} ulp, "
          f"bar 1); state {worst_state:.3e} from the mirror's after {steps} lock-steps")
    assert worst_a <= 1, "an action more than one float32 ulp from the mirror fed the kernel's own loc, log-scale and z"


def test_first_ratio_is_one_and_one_learner_step_is_the_plugins_update_on_the_same_batch():
    runner, eng = _engine(seed=7, epsilon=0.0)  # every draw from the head: a noise draw's stored log-probability is the noise distribution's, not the head's
    assert eng.learner_step() is False and eng.train_count == 0
    while eng.replay.is_warmup_needed():
        eng.actor_step()
    clone = ppo_v.Parameter(eng.cfg)
    clone.net.load_state_dict(copy.deepcopy(eng.parameter.net.state_dict()))
    assert eng.learner_step() is True and eng.train_count == 1 and eng.trainer.update_path == "srlx"
    torch.cuda.synchronize()
    r = eng.replay
    assert r.actions.dtype == torch.float32 and tuple(r.actions.shape) == (B, 1) and tuple(r.old_logpi.shape) == (B, 1)
    tr = ppo_v.Trainer(eng.cfg, clone, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    out = tr.train_on_batch(r.states[:B], r.next_states[:B], r.actions[:B], r.old_logpi[:B], r.rewards[:B], r.not_terminated[:B], r.total_rewards[:B])
    torch.cuda.synchronize()
    assert tr.update_path == "srlx"
    for a, b in zip(_params(eng.parameter), _params(clone)):
        assert torch.equal(a, b)
    assert eng.trainer.info == tr.info and set(eng.info()) == set(tr.info) | {"train_count", "memory", "env_steps"}
    # with unchanged parameters the stored log-probability IS the update's: every ratio of the first batch is exactly 1 where the store did not floor it
    floor = float(np.float32(np.log(1e-6)))
    old, new = r.old_logpi[:B].view(-1), out["new_logpi"].view(-1)
    live = old > floor
    ratio = torch.exp(new - old)
    print(f"VPPO-NORMAL-ENGINE first batch: {int(live.sum())} of {B} elements above the floor, ratio - 1 max {float((ratio[live] - 1).abs().max()):.1e}")
    assert int(live.sum()) >= B // 2 and torch.equal(new[live], old[live]) and bool((ratio[live] == 1.0).all()), "the first ratio is exactly 1"


def test_two_fresh_engines_with_one_seed_give_equal_actions_and_parameters():
    runs = []
    for _ in range(2):
        runner, eng = _engine(seed=11)
        eng.record = []
        for _ in range(50):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        runs.append((np.stack([r["actions"] for r in eng.record]), _params(eng.parameter), eng.train_count))
    assert runs[0][2] == runs[1][2] > 0
    assert np.array_equal(_i32(runs[0][0]), _i32(runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_runner_plays_the_parameter_the_engine_trained():
    runner, eng = _engine(seed=13)
    start = _params(eng.parameter)
    while eng.train_count < 30:
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    info = eng.info()
    assert info["train_count"] == 30 and all(np.isfinite(v) for v in info.values())
    assert {"loss_value", "loss_v_align", "loss_policy"} <= set(info)
    end = _params(runner.parameter)
    assert not any(torch.equal(a, b) for a, b in zip(start, end))
    rewards = runner.evaluate(max_episodes=1)  # srl.Runner("Pendulum-v1", ppo_v.Config(...)): the plugin path plays the Parameter the engine trained in place
    assert len(rewards) == 1 and np.isfinite(rewards[0]) and rewards[0] < 0


def test_host_stepped_pendulum_runs_sixty_lock_steps():
    from simple_distributed_rl_amd.base.context import RunContext
    from simple_distributed_rl_amd.device.vector_runner import EpisodeLedger, FloatActionHostVecEnv

    def batch_env(replay):
        env = FloatActionHostVecEnv(srl.EnvConfig("Pendulum-v1", {"max_steps": 7}), 4, replay.dev, 0, float_obs=True)
        env.setup(RunContext())
        return env

    runner, eng = _engine(seed=17, n_envs=4, env=batch_env, max_episode_steps=7, epsilon=0.5)
    eng.ledger = EpisodeLedger(4, eng.dev)
    eng.record = []
    for _ in range(60):
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    info = eng.info()
    assert info["env_steps"] == 240 and all(np.isfinite(v) for v in info.values())
    lanes = _replay_record(eng)
    assert eng.replay.R == 7 + 3, "an EnvRun's episode can last max_episode_steps + 1 steps: the ring holds that many and s'"
    assert eng.replay.count() == (lanes.ring.added, 0) and lanes.ring.added > 0
    n = lanes.ring.length()
    for name, w in zip(ITEM_VIEWS, lanes.slots()):
        got = eng.replay.view(name).numpy()[:n]
        assert np.array_equal(_i32(got), _i32(w.reshape(got.shape))), name
    # the host environments took the rescaled float32 rows: their rewards are Pendulum's for those torques (every reward is under 0 but the resets' zeros)
    assert all(bool((rec["reward"][~rec["first"]] < 0).all()) and bool((rec["reward"][rec["first"]] == 0).all()) for rec in eng.record)
    assert info["train_count"] > 0
    eng.env.teardown()


def test_engine_refusals_in_why_nots_words():
    from simple_distributed_rl_amd.device.vector_runner import why_not_vppo_engine
    from simple_distributed_rl_amd.device.vppo_engine import VppoEngine, VppoNormalEngine

    runner = _runner()
    runner.rl_config.batch_size = 512
    runner.rl_config.policy_block.set((48,))
    why = why_not_vppo_engine(runner.env, runner.rl_config, n_envs=5000, admit_normal=True)
    assert len(why.split("; ")) == 3
    with pytest.raises(ValueError) as e:
        VppoNormalEngine(runner.rl_config, 5000, parameter=runner.make_parameter())
    assert str(e.value) == f"VppoNormalEngine cannot run this configuration: {why}"
    # the categorical engine keeps refusing a continuous action space in the words it always had
    runner = _runner()
    with pytest.raises(ValueError, match="the Normal head's acting kernel is not built"):
        VppoEngine(runner.rl_config, 4, parameter=runner.make_parameter(), max_episode_steps=200)
    # and the Normal engine a discrete one
    cart = _runner(env="CartPole-v1")
    with pytest.raises(ValueError, match="a discrete action space is VppoEngine's"):
        VppoNormalEngine(cart.rl_config, 4, parameter=cart.make_parameter(), max_episode_steps=500)


def test_categorical_engine_on_cartpole_is_what_it_was():
    """Two fresh categorical engines on CartPole give equal records, rings and parameters (tests/test_vppo_engine_gpu.py, untouched, holds them to the mirror): the
    store's kernels now carry a K, and at K = 1 nothing may have moved."""
    from simple_distributed_rl_amd.device.vppo_engine import VppoEngine

    runs = []
    for _ in range(2):
        runner = _runner(11, env="CartPole-v1", epsilon=0.3)
        eng = VppoEngine(runner.rl_config, E, seed=11, parameter=runner.make_parameter())
        eng.record = []
        for _ in range(60):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        assert eng.K == 0 and eng.A == 2 and eng.actions.dtype == torch.int32 and eng.replay.action_dim == 0
        assert tuple(eng.replay.view("item_action").shape) == (2000,) and eng.replay.view("item_action").dtype == torch.int32
        runs.append(([np.stack([r[k] for r in eng.record]) for k in ("actions", "logp", "logits", "cdf", "reward", "done")],
                     [eng.replay.view(v).numpy() for v in ITEM_VIEWS], _params(eng.parameter), eng.train_count, eng.replay.count()))
    assert runs[0][3] == runs[1][3] > 0 and runs[0][4] == runs[1][4] and runs[0][4][0] > 0 and runs[0][4][1] == 0
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert np.array_equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


@pytest.mark.slow
def test_pendulum_learning_on_sixteen_lanes_beside_the_plugin_path():
    """Opt-in (SRLX_RUN_SLOW=1).  A record, not a gate on a return: ppo_v.Config() with warm-up 500 on the plugin path (seed 1, 6000 steps) and on the engine (16
    lanes, one update per lock-step, 6000 updates, seed 1), then 5 evaluation episodes each.  Printed as "VPPO-NORMAL-ENGINE-LEARN ..."; the engine only has to
    finish with finite losses."""
    import random

    from simple_distributed_rl_amd.device.vppo_engine import VppoNormalEngine

    def make(seed):
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        cfg = ppo_v.Config()
        cfg.memory.warmup_size = 500
        runner = srl.Runner("Pendulum-v1", cfg)
        runner.set_device("cuda:0")
        runner.set_seed(seed)
        return runner

    def plugin(seed):
        runner = make(seed)
        runner.train(max_steps=6000)
        return float(np.mean(runner.evaluate(max_episodes=5)))

    def engine(seed):
        runner = make(seed)
        eng = VppoNormalEngine(runner.rl_config, 16, seed=seed, parameter=runner.make_parameter())
        while eng.train_count < 6000:
            eng.step(learner_updates=1)
        assert all(np.isfinite(v) for v in eng.info().values())
        return float(np.mean(runner.evaluate(max_episodes=5)))

    plugin_a, engine_a = plugin(1), engine(1)
    print(f"VPPO-NORMAL-ENGINE-LEARN mean return over 5 episodes: plugin seed 1 {plugin_a:.1f}, engine (16 lanes) seed 1 {engine_a:.1f}")
