"""The V-PPO device engine without a GPU: the mirror of srlx_vppo_act and of the episode store (tests/vppo_engine_reference.py) held to hand-worked
literals and, field by field, to what `ppo_v.Worker.on_step` adds to a Memory; every sentence of `why_not_vppo_engine` on a config that trips exactly that
reason; the route (`engine_kind`) as it was; the new entry points' declaration and export."""
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_engine_reference as M  # noqa: E402

from simple_distributed_rl_amd.algorithms import ppo_v  # noqa: E402
from simple_distributed_rl_amd.base.define import SpaceTypes  # noqa: E402
from simple_distributed_rl_amd.base.spaces.box import BoxSpace  # noqa: E402
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace  # noqa: E402
from simple_distributed_rl_amd.device.vector_runner import engine_kind, why_not_vppo_engine  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the acting rule ------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_cdf_and_inverse_cdf_literals():
    z = np.array([[0.0, math.log(3.0)], [1.0, 1.0]], np.float32)
    c = M.cdf(z)
    # row 0: max = log 3 (as a float32), weights exp(-log 3) = 1/3 and 1; row 1: 1 and 1
    l3 = float(np.float32(math.log(3.0)))
    assert c[0].tolist() == [math.exp(-l3), math.exp(-l3) + 1.0] and c[1].tolist() == [1.0, 2.0]
    # u1 c_last against the boundaries: 0.2 * 1.3333 = 0.267 < 0.3333 -> 0; 0.3 * 1.3333 = 0.4 -> 1; a tie (0.5 * 2 = 1.0 < 1.0 is false) -> the next action
    assert M.inverse_cdf(c[[0, 0, 1, 1]], np.array([0.2, 0.3, 0.5, 0.4999])).tolist() == [0, 1, 1, 0]
    np.testing.assert_allclose(M.boundary_gap(c[[1]], np.array([0.25])), [0.25], rtol=0, atol=1e-15)


def test_mirror_inverse_cdf_falls_back_to_the_last_action():
    c = np.array([[0.5, 1.0]])
    assert M.inverse_cdf(c, np.array([1.0])).tolist() == [1]  # (a value the generator never gives: 1.0 < 1.0 is false for every k)


def test_mirror_uniform_branch_literals():
    top = 1.0 - 2.0 ** -53
    assert M.uniform_actions(np.array([0.49, 0.5, 0.0, top]), 2).tolist() == [0, 1, 0, 1]
    assert M.uniform_actions(np.array([top]), 16).tolist() == [15] and M.uniform_actions(np.array([1.0]), 3).tolist() == [2]
    assert M.uniform_logp(2) == np.float32(-0.6931471805599453) and M.uniform_logp(16) == np.float32(math.log(1.0 / 16))


def test_mirror_act_takes_each_branch_by_the_rows_first_uniform():
    u0, u1 = M.uniforms(7, 3, 2)
    np.testing.assert_allclose(np.stack([u0, u1], 1).reshape(-1), [0.04136613, 0.7773777, 0.86880186, 0.2478679], rtol=0, atol=5e-9)  # the oracle at (7, 3)
    z = np.zeros((2, 2), np.float32)
    a, random, c = M.act(z, 7, 3, 0.1)
    assert random.tolist() == [True, False] and a.tolist() == [1, 0]  # floor(0.777 * 2) = 1; 0.2479 * 2 = 0.496 < 1 -> 0
    assert M.act(z, 7, 3, 0.0)[1].tolist() == [False, False] and M.act(z, 7, 3, 1.0)[1].tolist() == [True, True]
    assert M.act(z, 7, 3, 0.0)[0].tolist() == [1, 0]  # 0.777 * 2 = 1.55: not under c_0 = 1 -> 1


# ---- the trackings and the ring ---------------------------------------------------------------------------------------------------------------------------------
def _step(i):
    return (np.float32([i]), np.float32([i + 1]), i % 2, np.float32(-0.5 - i), np.float32(1.0), np.float32(1.0))


def test_mirror_three_step_episode_returns_in_reversed_order():
    items = M.close_episode([_step(0), _step(1), _step(2)], 0.5)
    assert [float(it[0][0]) for it in items] == [2.0, 1.0, 0.0]  # the last step first
    assert [float(it[6]) for it in items] == [1.0, 1.5, 1.75]  # 1; 1 + 0.5 * 1; 1 + 0.5 * 1.5
    items = M.close_episode([_step(0), _step(1), _step(2)], 0.95)
    assert [it[6] for it in items] == [np.float32(1.0), np.float32(1.95), np.float32(1.0 + 0.95 * 1.95)]
    assert all(it[6].dtype == np.float32 for it in items)


def test_mirror_ring_wraps_as_replay_buffer_add_does():
    from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBuffer

    ring, ref = M.Ring(3), ReplayBuffer(batch_size=1, capacity=3, warmup_size=1, compress=False)
    for x in range(8):
        ring.add(x), ref.add(x)
        assert ring.buffer == ref.buffer and ring.idx == ref.idx and ring.length() == ref.length()
    assert ring.buffer == [6, 7, 5] and ring.added == 8  # item q in slot q % 3


def test_mirror_one_close_longer_than_the_ring_keeps_its_last_capacity_items():
    obs = np.zeros((1, 1), np.float32)
    lanes = M.Lanes(1, 3, 1.0, 10, obs)
    for i in range(5):
        lanes.push([i], [-1.0], [float(i)], [0], [1 if i == 4 else 0], np.float32([[i + 1]]))
    s, s2, a, lp, r, nt, tot = lanes.slots()
    # the walk adds steps 4, 3, 2, 1, 0 as items 0..4; slots q % 3 hold items 3, 4, 2 = steps 1, 0, 2
    assert a.tolist() == [1, 0, 2] and tot.tolist() == [10.0, 10.0, 9.0] and lanes.ring.added == 5
    assert s[:, 0].tolist() == [1.0, 0.0, 2.0] and s2[:, 0].tolist() == [2.0, 1.0, 3.0]


def test_mirror_lanes_follow_the_needs_reset_protocol_and_the_lane_order():
    lanes = M.Lanes(2, 8, 0.5, 4, np.float32([[10], [20]]))
    lanes.push([0, 1], [-20.0, -1.0], [1.0, 2.0], [1, 0], [1, 1], np.float32([[11], [21]]))  # both close: lane 0's item first
    assert lanes.slots()[0][:, 0].tolist() == [10.0, 20.0] and lanes.slots()[3].tolist() == [M.LOG_FLOOR, np.float32(-1.0)]
    assert lanes.slots()[5].tolist() == [0.0, 1.0] and lanes.needs_reset == [True, True]
    lanes.push([1, 1], [-1.0, -1.0], [9.0, 9.0], [0, 0], [0, 0], np.float32([[12], [22]]))  # only the new first observations
    assert lanes.ring.added == 2 and lanes.track == [[], []] and lanes.needs_reset == [False, False]
    lanes.push([1, 0], [-1.0, -1.0], [3.0, 4.0], [0, 0], [0, 1], np.float32([[13], [23]]))
    assert lanes.slots()[0][:, 0].tolist() == [10.0, 20.0, 22.0] and lanes.slots()[1][2, 0] == 23.0 and len(lanes.track[0]) == 1


def test_mirror_over_long_episode_sets_the_error():
    lanes = M.Lanes(1, 8, 0.5, 2, np.float32([[0]]))
    for i in range(2):
        lanes.push([0], [-1.0], [1.0], [0], [0], np.float32([[i + 1]]))
    assert lanes.error == 0
    lanes.push([0], [-1.0], [1.0], [0], [0], np.float32([[3]]))
    assert lanes.error == 1 and lanes.ring.added == 0
    lanes.push([0], [-1.0], [1.0], [0], [1], np.float32([[4]]))  # the rest of the dropped episode does not close
    assert lanes.ring.added == 0 and lanes.needs_reset == [True]
    lanes.push([0], [-1.0], [9.0], [0], [0], np.float32([[5]]))  # the new first observation
    lanes.push([0], [-1.0], [2.5], [1], [1], np.float32([[6]]))
    assert lanes.ring.added == 1 and lanes.slots()[6].tolist() == [2.5] and lanes.slots()[0][0, 0] == 5.0 and lanes.error == 1


def test_mirror_floyd_literals():
    assert M.floyd(5, 2, [0.9, 0.1]) == [3, 0]  # j = 3: floor(0.9 * 4) = 3; j = 4: floor(0.1 * 5) = 0
    assert M.floyd(5, 2, [0.9, 0.7]) == [3, 4]  # j = 4: floor(0.7 * 5) = 3, taken -> 4
    assert M.floyd(3, 3, [0.5, 0.2, 0.1]) == [0, 1, 2]  # B == N: j = 0 -> 0; j = 1: floor(0.4) = 0, taken -> 1; j = 2: floor(0.3) = 0, taken -> 2
    assert sorted(M.floyd(4, 4, [0.0, 0.99, 0.5, 0.3])) == [0, 1, 2, 3]
    for N, B in ((7, 7), (64, 64), (300, 256), (10, 1)):
        got = M.draw(5, 2, N, B)
        assert len(set(got)) == B and min(got) >= 0 and max(got) < N


# ---- the Worker itself ------------------------------------------------------------------------------------------------------------------------------------------
class _Run:
    """What `ppo_v.Worker.on_step` asks of a WorkerRun."""

    def __init__(self):
        self._context = SimpleNamespace(training=True)
        self.rows = []

    def add_tracking(self, d):
        self.rows.append(d)

    def get_trackings(self):
        return [list(d.values()) for d in self.rows]


def test_mirror_adds_what_the_worker_adds_on_a_scripted_episode():
    cfg = ppo_v.Config(discount=0.9)
    added = []
    w = ppo_v.Worker(cfg, None, SimpleNamespace(add=added.append))
    run = _Run()
    w._set_worker_run(run)
    rng = np.random.default_rng(3)
    n = 5
    obs = rng.standard_normal((n + 1, 3)).astype(np.float32)
    acts = [1, 0, 3, 2, 1]
    logps = np.float32([-0.3, -20.0, math.log(1e-6), -13.0, -1.25])  # both sides of the floor, and the floor itself
    rewards = [1.0, -0.5, 0.25, 2.0, 1.0]
    lanes = M.Lanes(1, 16, 0.9, 10, obs[:1])
    for i in range(n):
        run.state, run.next_state, run.reward, run.terminated, run.done = obs[i], obs[i + 1], rewards[i], i == n - 1, i == n - 1
        w.action, w.log_prob = np.eye(4, dtype=np.float32)[acts[i]], np.float32([logps[i]])
        w.on_step(run)
        lanes.push([acts[i]], [logps[i]], [rewards[i]], [int(i == n - 1)], [int(i == n - 1)], obs[i + 1:i + 2])
    assert len(added) == n == lanes.ring.added
    s, s2, a, lp, r, nt, tot = lanes.slots()
    for k, item in enumerate(added):
        assert np.array_equal(item[0], s[k]) and np.array_equal(item[1], s2[k]) and int(np.argmax(item[2])) == a[k]
        assert np.float32(item[3][0]) == lp[k] and np.float32(item[4]) == r[k] and np.float32(item[5]) == nt[k]
        assert np.float32(item[6]) == tot[k], (k, item[6], tot[k])
    assert lp.tolist() == [np.float32(-1.25), np.float32(-13.0), M.LOG_FLOOR, M.LOG_FLOOR, np.float32(-0.3)]


# ---- why_not_vppo_engine ----------------------------------------------------------------------------------------------------------------------------------------
def _env(A=2, shape=(4,), players=1, action_space=None, steps=500):
    return SimpleNamespace(player_num=players, action_space=DiscreteSpace(A) if action_space is None else action_space, max_episode_steps=steps,
                           observation_space=BoxSpace(shape, -np.inf, np.inf, np.float32, SpaceTypes.CONTINUOUS))


def _cfg(**kw):
    c = ppo_v.Config(**kw)
    c._rl_act_space = DiscreteSpace(2)
    return c


def _one(reason):
    assert reason and "; " not in reason, reason
    return reason


def test_why_not_is_empty_for_the_default_config_on_cartpole_and_the_route_is_as_it_was():
    import simple_distributed_rl_amd as srl

    runner = srl.Runner("CartPole-v1", ppo_v.Config())
    runner.set_device("cpu")
    runner.setup_rl_config()
    assert why_not_vppo_engine(runner.env, runner.rl_config) == ""
    assert why_not_vppo_engine(runner.env, runner.rl_config, n_envs=16) == ""
    assert why_not_vppo_engine(_env(), _cfg(), n_envs=4096) == ""
    assert engine_kind(ppo_v.Config()) is None


def test_why_not_names_each_reason_on_its_own():
    from simple_distributed_rl_amd.algorithms import dqn
    from simple_distributed_rl_amd.rl.memories.priority_replay_buffer import PriorityReplayBufferConfig

    assert why_not_vppo_engine(_env(), dqn.Config()) == "'DQN' is not a V-PPO config"
    assert _one(why_not_vppo_engine(_env(players=2), _cfg())) == "multi-player environment"
    box = BoxSpace((1,), -1.0, 1.0, np.float32, SpaceTypes.CONTINUOUS)
    assert _one(why_not_vppo_engine(_env(action_space=box), _cfg())).startswith("a continuous action space: the Normal head's acting kernel is not built")
    assert _one(why_not_vppo_engine(_env(A=17), _cfg())).startswith("17 actions: outside the envelope (D 1..256")
    assert _one(why_not_vppo_engine(_env(shape=(257,)), _cfg())).startswith("257 observation elements: outside the envelope")
    assert _one(why_not_vppo_engine(_env(shape=(4, 4)), _cfg())).startswith("the actor-critic reads flat BoxSpace((D,)) observations")
    c = _cfg()
    c._obs_processors = [(object(), None, _env().observation_space)]  # (processor, space before, space after)
    assert _one(why_not_vppo_engine(_env(), c)) == "observation processors are served by the plugin path"
    assert _one(why_not_vppo_engine(_env(), _cfg(window_length=2))) == "the network reads one observation (window_length 1)"
    c = _cfg()
    c.hidden_block.set((64, 48))
    assert _one(why_not_vppo_engine(_env(), c)).startswith("input_block + hidden_block (64, 48): outside the envelope")
    c = _cfg()
    c.input_block.value.set((64, 64))  # four trunk layers with the hidden block's two
    assert _one(why_not_vppo_engine(_env(), c)).startswith("input_block + hidden_block (64, 64, 64, 64): outside the envelope")
    c = _cfg()
    c.value_block.set((64, 64, 64))
    assert _one(why_not_vppo_engine(_env(), c)).startswith("value_block (64, 64, 64): outside the envelope")
    c = _cfg()
    c.policy_block.set((16,))
    assert _one(why_not_vppo_engine(_env(), c)).startswith("policy_block (16,): outside the envelope")
    c = _cfg()
    c.policy_block.set((64,), activation="tanh")
    assert _one(why_not_vppo_engine(_env(), c)) == "policy_block is not an MLP of ReLU layers (Linear layers with biases)"
    c = _cfg()
    c.value_block.set((64,), use_bias=False)
    assert _one(why_not_vppo_engine(_env(), c)) == "the value_block sets ['use_bias'] (the kernels' layers are Linear with bias + ReLU)"
    c = _cfg()
    c.lr_scheduler.schedule_type = "linear"
    assert _one(why_not_vppo_engine(_env(), c)) == "the lr schedule 'linear' is not one the host evaluates per step"
    assert _one(why_not_vppo_engine(_env(), _cfg(batch_size=257))) == "batch size 257 above max_batch 256"
    assert _one(why_not_vppo_engine(_env(), _cfg(memory=PriorityReplayBufferConfig()))).startswith("V-PPO draws uniformly from the ReplayBuffer memory")
    assert _one(why_not_vppo_engine(_env(steps=None), _cfg())).startswith("no known max_episode_steps")
    assert _one(why_not_vppo_engine(_env(steps=0), _cfg())).startswith("no known max_episode_steps")
    assert _one(why_not_vppo_engine(_env(steps=4094), _cfg())) == "max_episode_steps 4094 above the tracking ring's 4093"
    assert why_not_vppo_engine(_env(steps=4093), _cfg()) == ""
    c = _cfg()
    c.memory.capacity, c.memory.warmup_size = 400, 100
    assert _one(why_not_vppo_engine(_env(), c)).startswith("max_episode_steps 500 above the memory's capacity 400")
    for n in (0, 4097, 1.5):
        assert _one(why_not_vppo_engine(_env(), _cfg(), n_envs=n)) == f"{n!r} lanes are outside the engine's 1..4096"


def test_why_not_joins_every_reason():
    why = why_not_vppo_engine(_env(A=17, players=2, steps=None), _cfg(batch_size=300), n_envs=0)
    assert len(why.split("; ")) == 5 and why.startswith("multi-player environment; 17 actions")


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------------------------
NEW = ("srlx_vppo_act", "srlx_vppo_lanes_create", "srlx_vppo_lanes_destroy", "srlx_vppo_lanes_reset", "srlx_vppo_lanes_push", "srlx_vppo_lanes_sample",
       "srlx_vppo_lanes_count", "srlx_vppo_lanes_views", "srlx_vppo_lanes_read")


def test_entry_points_are_declared_bound_and_exported():
    from simple_distributed_rl_amd import _native as N

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srlx.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in N.SIGNATURES and hasattr(N.lib(), name), name


def test_refusals_that_need_no_device():
    import ctypes

    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    assert lib.srlx_vppo_act(None, 1, None, 0, None, 0.1, None, None, None, None, None) == N.ERR_INVALID and b"vppo_act: NULL handle" in lib.srlx_last_error()
    h = N.c_p()
    for args, word in (((0, 4, 500, 100, 0.9), b"0 lanes"), ((4097, 4, 500, 100, 0.9), b"4097 lanes"), ((1, 0, 500, 100, 0.9), b"observation length 0"),
                       ((1, 257, 500, 100, 0.9), b"observation length 257"), ((1, 4, 0, 100, 0.9), b"max_episode_steps 0"),
                       ((1, 4, 4095, 100, 0.9), b"max_episode_steps 4095"), ((1, 4, 500, 0, 0.9), b"capacity 0"), ((1, 4, 500, 100, 1.5), b"discount 1.5")):
        st = lib.srlx_vppo_lanes_create(ctypes.byref(h), *args, 0)
        assert st == N.ERR_INVALID and not h and b"vppo_lanes_create" in lib.srlx_last_error() and word in lib.srlx_last_error(), (args, lib.srlx_last_error())
    for call in (lambda: lib.srlx_vppo_lanes_push(None, *[None] * 8), lambda: lib.srlx_vppo_lanes_sample(None, 1, 0, *[None] * 9),
                 lambda: lib.srlx_vppo_lanes_reset(None, None, None)):
        assert call() == N.ERR_INVALID and b"vppo_lanes" in lib.srlx_last_error()


def test_train_on_batch_takes_int32_actions():
    import inspect

    sig = inspect.signature(ppo_v.Trainer.train_on_batch)
    assert list(sig.parameters)[-1] == "actions" and sig.parameters["actions"].default is None
