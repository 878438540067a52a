"""The SAC-Discrete device engine on the GPU (device/sacd_engine.py): device CartPole, E = 16 lanes, batches of 8, blocks (32,), 32 random steps,
warm-up 32.  What the lanes drew against the mirror (tests/sacd_engine_reference.py), the ring against the recorded transitions, one update against the plugin's
own `train_on_batch` on a cloned Parameter, two fresh engines against each other, the trained Parameter played by the Runner, a host-stepped environment."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd.algorithms import sac

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_engine_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

E, B, START, WARMUP = 16, 8, 32, 32
NETWORKS = ("policy", "q1_online", "q1_target", "q2_online", "q2_target")


def _runner(seed=0, **kw):
    cfg = sac.Config(batch_size=B, start_steps=START, **kw)
    cfg.policy_block.set((32,))
    cfg.q_block.set((32,))
    cfg.memory.warmup_size = WARMUP
    runner = srl.Runner("CartPole-v1", cfg)
    runner.set_device("cuda:0")
    torch.manual_seed(seed)
    runner.make_parameter()
    return runner


def _engine(seed=0, n_envs=E, live_policy=False, env=None, **kw):
    """A fresh engine around a fresh Runner's Parameter.  live_policy: the policy's out layer gets seeded non-zero weights (a fresh one is zero: every logit 0,
    which would hide the network from a test of the actions)."""
    from simple_distributed_rl_amd.device.sacd_engine import SacdEngine

    runner = _runner(seed, **kw)
    p = runner.make_parameter()
    if live_policy:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            w = p.policy.out_layer.weight
            w.copy_(torch.randn(w.shape, generator=g).to(w.device))
    eng = SacdEngine(runner.rl_config, n_envs, seed=seed, parameter=p, env=env)
    assert eng.parameter is runner.make_parameter()
    return runner, eng


def _bits(p):
    return [t.detach().clone() for name in NETWORKS for t in getattr(p, name).parameters()] + [p.log_alpha.detach().clone()]


def _clone_parameter(cfg, p):
    q = sac.Parameter(cfg)
    for name in NETWORKS:
        getattr(q, name).load_state_dict(copy.deepcopy(getattr(p, name).state_dict()))
    with torch.no_grad():
        q.log_alpha.copy_(p.log_alpha)
    return q


def _observations(eng):
    """obs[t]: what the lanes saw at lock-step t, from the record."""
    obs = [eng.first_obs.cpu().numpy()]
    for rec in eng.record[:-1]:
        obs.append(rec["next_obs"])
    return obs


def test_lanes_draw_the_mirrors_actions_and_the_counter_advances_once_per_lock_step():
    runner, eng = _engine(seed=3, live_policy=True)
    eng.record = []
    steps = 6
    for _ in range(steps):
        eng.actor_step()
    torch.cuda.synchronize()
    assert eng.random_until == 2 and eng.lock_steps == steps and eng.total_env_steps == steps * E
    policy64 = copy.deepcopy(eng.parameter.policy).double().cpu()
    live = 0
    for t, (rec, obs) in enumerate(zip(eng.record, _observations(eng))):
        assert rec["counter"] == t
        with torch.no_grad():
            want = policy64(torch.from_numpy(obs).double()).numpy()
        np.testing.assert_allclose(rec["logits"], want, rtol=1e-5, atol=1e-6)
        actions, scores = M.act(rec["logits"], eng.seed ^ 0xAC7, t, eng.random_until, 2)
        np.testing.assert_allclose(rec["scores"], scores, rtol=1e-12, atol=1e-12)
        assert float(M.top_two_gap(scores).min()) > 1e-9
        assert np.array_equal(rec["actions"], actions), f"lock-step {t}"
        if t < 2:
            assert np.array_equal(actions, M.random_actions(M.uniforms(eng.seed ^ 0xAC7, t, E, 2), 2))
        else:
            assert np.array_equal(actions, M.first_argmax(scores))
            live += int(np.abs(rec["logits"]).max() > 0)
    assert live == steps - 2, "the logits of the sampling phase are the network's"
    assert int(eng.policy_counter.item()) == steps


def test_every_drawn_row_is_one_recorded_transition_of_one_lane():
    runner, eng = _engine(seed=5)
    eng.record = []
    for _ in range(48):
        eng.actor_step()
    torch.cuda.synchronize()
    obs = _observations(eng)
    recorded, terminals = {}, 0
    for t, rec in enumerate(eng.record):
        for e in range(E):
            if rec["first"][e]:  # the lock-step only delivered a new episode's first observation: no item
                continue
            key = (obs[t][e].tobytes(), int(rec["actions"][e]), np.float32(rec["reward"][e]).tobytes(), rec["next_obs"][e].tobytes(), int(rec["terminated"][e] != 0))
            recorded[key] = (t, e)
            terminals += int(rec["terminated"][e] != 0)
    assert terminals > 0, "no episode ended in 48 lock-steps of CartPole"
    assert eng.replay.length() == 48 * E
    seen_terminal, rows = 0, 0
    for _ in range(48):
        state, onehot, n_state, reward, done, actions = (x.cpu().numpy() for x in eng.draw_batch())
        eng.replay.check_draws()
        assert np.array_equal(onehot, (np.arange(2)[None, :] == actions[:, None]).astype(np.float32))
        for b in range(B):
            key = (state[b].tobytes(), int(actions[b]), np.float32(reward[b]).tobytes(), n_state[b].tobytes(), int(done[b]))
            assert key in recorded, f"row {b} is no recorded transition"
            t, e = recorded[key]
            if done[b]:  # s' is the ending step's own next observation, never the next episode's first frame
                seen_terminal += 1
                assert eng.record[t]["done"][e] and (t + 1 == len(eng.record) or eng.record[t + 1]["first"][e])
                assert n_state[b].tobytes() == eng.record[t]["next_obs"][e].tobytes()
            rows += 1
    print(f"SACD-ENGINE ring: {rows} drawn rows matched {len(recorded)} recorded transitions, {seen_terminal} of them terminal ({terminals} recorded)")
    assert seen_terminal > 0


def test_one_learner_step_is_the_plugins_update_on_the_same_five_tensors():
    runner, eng = _engine(seed=7, live_policy=True)
    assert eng.learner_step() is False and eng.train_count == 0
    for _ in range(3):
        eng.actor_step()
    clone = _clone_parameter(eng.cfg, eng.parameter)
    assert eng.learner_step() is True and eng.train_count == 1 and eng.trainer.update_path == "srlx"
    torch.cuda.synchronize()
    tr = sac.Trainer(eng.cfg, clone, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    reward = eng.replay.batch.rewards.view(-1)
    tr.train_on_batch(eng.states, eng.onehot, eng.next_states, reward, eng.done)  # (no `actions`: the argmax round trip gives the same int32 actions)
    torch.cuda.synchronize()
    assert tr.update_path == "srlx"
    for a, b in zip(_bits(eng.parameter), _bits(clone)):
        assert torch.equal(a, b)
    assert eng.trainer.info == tr.info and set(eng.info()) == set(tr.info) | {"train_count", "memory", "env_steps"}
    assert eng.info()["memory"] == 3 * E and eng.info()["env_steps"] == 3 * E


def test_two_fresh_engines_with_one_seed_give_equal_actions_and_parameters():
    runs = []
    for _ in range(2):
        runner, eng = _engine(seed=11)
        eng.record = []
        for _ in range(12):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        runs.append((np.stack([r["actions"] for r in eng.record]), _bits(eng.parameter), eng.train_count))
    assert runs[0][2] == runs[1][2] == 11  # (the warm-up of 32 items is two lock-steps: the second one already trains)
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_runner_plays_the_parameter_the_engine_trained():
    runner, eng = _engine(seed=13)
    start = _bits(eng.parameter)
    while eng.train_count < 30:
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    info = eng.info()
    assert info["train_count"] == 30 and all(np.isfinite(v) for v in info.values())
    assert {"q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha"} <= set(info)
    end = _bits(runner.parameter)
    assert not any(torch.equal(a, b) for a, b in zip(start, end))
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(r >= 1 for r in rewards)


def test_host_stepped_environment_runs_forty_lock_steps():
    from simple_distributed_rl_amd.base.context import RunContext
    from simple_distributed_rl_amd.device.vector_runner import EpisodeLedger, HostVecEnv

    def batch_env(replay):
        env = HostVecEnv(srl.EnvConfig("CartPole-v1"), 4, replay.dev, 0, float_obs=True)
        env.setup(RunContext())
        return env

    runner, eng = _engine(seed=17, n_envs=4, env=batch_env)
    eng.ledger = EpisodeLedger(4, eng.dev)
    assert eng.random_until == 8
    for _ in range(40):
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    info = eng.info()
    assert info["env_steps"] == 160 and info["train_count"] == 40 - 8 + 1 and all(np.isfinite(v) for v in info.values())
    assert len(eng.ledger.drain()) > 0
    eng.env.teardown()


def test_engine_refuses_a_config_outside_the_envelope_in_why_nots_words():
    from simple_distributed_rl_amd.device.sacd_engine import SacdEngine
    from simple_distributed_rl_amd.device.vector_runner import why_not_sacd_engine

    runner = _runner()
    runner.rl_config.batch_size = 512
    runner.rl_config.policy_block.set((48,))
    why = why_not_sacd_engine(runner.env, runner.rl_config, n_envs=5000)
    assert len(why.split("; ")) == 3
    with pytest.raises(ValueError) as e:
        SacdEngine(runner.rl_config, 5000, parameter=runner.make_parameter())
    assert str(e.value) == f"SacdEngine cannot run this configuration: {why}"


@pytest.mark.slow
def test_cartpole_learning_on_sixteen_lanes_beside_the_plugin_path():
    """Opt-in (SRLX_RUN_SLOW=1).  The hyper-parameters of test_sacd_gpu.py's test_cartpole_learning_run_srlx_beside_torch (500 random steps, warm-up 500, batch
    32, lr 1e-3 for all three, 3000 updates after them) on the plugin path (seeds 1 and 2) and on the engine (16 lanes, one update per lock-step, seed 1), then
    10 evaluation episodes each.  No return threshold is invented: the engine's bar is the plugin path's own mean return from this same run, less the
    seed-to-seed spread measured here.  Printed as "SACD-ENGINE-LEARN ..."."""
    import random

    from simple_distributed_rl_amd.device.sacd_engine import SacdEngine

    def make(seed):
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
        cfg = sac.Config(start_steps=500, lr_policy=1e-3, lr_q=1e-3, lr_alpha=1e-3)
        cfg.memory.warmup_size = 500
        runner = srl.Runner("CartPole-v1", cfg)
        runner.set_device("cuda:0")
        runner.set_seed(seed)
        return runner

    def plugin(seed):
        runner = make(seed)
        runner.train(max_steps=3500)
        return float(np.mean(runner.evaluate(max_episodes=10)))

    def engine(seed):
        runner = make(seed)
        eng = SacdEngine(runner.rl_config, 16, seed=seed, parameter=runner.make_parameter())
        while eng.train_count < 3000:
            eng.step(learner_updates=1)
        return float(np.mean(runner.evaluate(max_episodes=10)))

    plugin_a, plugin_b, engine_a = plugin(1), plugin(2), engine(1)
    print(f"SACD-ENGINE-LEARN mean return over 10 episodes: plugin seed 1 {plugin_a:.1f}, plugin seed 2 {plugin_b:.1f}, engine (16 lanes) seed 1 {engine_a:.1f}")
    assert engine_a >= min(plugin_a, plugin_b) - abs(plugin_a - plugin_b)
