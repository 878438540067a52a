"""The V-PPO device engine's Normal head without a GPU: the mirror of srlx_vppo_act_normal, of the lanes' Pendulum and of the K-wide episode store
(tests/vppo_normal_reference.py) held to hand-worked literals, to `ppo_v.Worker.on_step` field by field on a scripted continuous episode, to envs/pendulum.py bit
for bit; the Box-Muller draws of one whole counter held to the moments of a standard normal; every new sentence of `why_not_vppo_engine(admit_normal=True)` and
the old answers unchanged; the new entry points' declaration, export and the refusals that need no device."""
import ctypes
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_normal_reference as M  # noqa: E402

from simple_distributed_rl_amd.algorithms import ppo_v  # noqa: E402
from simple_distributed_rl_amd.base.define import SpaceTypes  # noqa: E402
from simple_distributed_rl_amd.base.spaces.box import BoxSpace  # noqa: E402
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace  # noqa: E402
from simple_distributed_rl_amd.base.spaces.np_array import NpArraySpace  # noqa: E402
from simple_distributed_rl_amd.device.vector_runner import engine_kind, why_not_vppo_engine  # noqa: E402
from simple_distributed_rl_amd.rl.functions import compute_normal_logprob, compute_normal_logprob_sgp  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32


# ---- the acting rule ------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_uniform_layout_is_two_k_plus_one_per_row():
    from hot_path_oracle import rng_uniform

    flat = rng_uniform(np.uint64(7), 3, 2 * 7)  # K = 3: 7 uniforms per row
    u0, ua, ub = M.uniforms(7, 3, 2, 3)
    assert u0.tolist() == [flat[0], flat[7]]
    assert ua.tolist() == [[flat[1], flat[3], flat[5]], [flat[8], flat[10], flat[12]]]
    assert ub.tolist() == [[flat[2], flat[4], flat[6]], [flat[9], flat[11], flat[13]]]
    # K = 1 at (7, 3): the oracle's first values (tests/test_vppo_engine_cpu.py pins them)
    u0, ua, ub = M.uniforms(7, 3, 1, 1)
    np.testing.assert_allclose([u0[0], ua[0, 0], ub[0, 0]], [0.04136613, 0.7773777, 0.86880186], rtol=0, atol=5e-9)


def test_mirror_box_muller_literals():
    # Ua = 0: log 1 = 0 -> z = 0 whatever Ub; Ub = 0: cos 0 = 1 -> z = sqrt(-2 log(1 - Ua)); Ub = 0.5: the same with the other sign
    assert M.box_muller(0.0, 0.3) == 0.0
    r = math.sqrt(-2.0 * math.log(1.0 - 0.75))  # sqrt(2 log 4) = 1.6651...
    assert M.box_muller(0.75, 0.0) == r and abs(r - 1.6651092223153954) < 1e-15
    assert M.box_muller(0.75, 0.5) == -r
    assert abs(M.box_muller(0.75, 0.25)) < 2e-16 * r  # cos(pi / 2) in float64: 6e-17
    top = 1.0 - 2.0 ** -53  # the generator's largest value: 1 - Ua = 2^-53, finite
    assert M.box_muller(top, 0.0) == math.sqrt(2.0 * 53 * math.log(2.0))


def test_mirror_branch_action_and_logp_literals():
    loc, ls = F32([[0.5, -1.0]]), F32([[0.0, math.log(2.0)]])
    random, l, s, sd = M.branch(loc, ls, np.array([0.2]), 0.1, 0.5)
    assert not random[0] and l.tolist() == loc.tolist() and sd.tolist() == [[1.0, 2.0]] and s.dtype == F32 and sd.dtype == F32
    a = M.action_of(l, sd, np.array([[1.0, -0.25]]))
    assert a.tolist() == [[1.5, -1.5]] and a.dtype == F32  # 0.5 + 1 * 1; -1 + 2 * -0.25
    lp = M.logp_f32(a, l, s, sd, False)
    # u = 1 and -0.25: -0.9189385 - 0 - 0.5; -0.9189385 - log 2 - 0.5 * 0.0625
    want = [F32(F32(-M.HALF_LOG_2PI - F32(0.0)) - F32(0.5)), F32(F32(-M.HALF_LOG_2PI - F32(math.log(2.0))) - F32(0.03125))]
    assert lp[0].tolist() == want and lp.dtype == F32
    np.testing.assert_allclose(lp, compute_normal_logprob(a.astype(np.float64), loc.astype(np.float64), sd.astype(np.float64)), rtol=1e-6, atol=1e-7)
    # the epsilon branch: loc 0, scale the noise scale, on EVERY element of the row
    random, l, s, sd = M.branch(loc, ls, np.array([0.05]), 0.1, 0.5)
    assert random[0] and l.tolist() == [[0.0, 0.0]] and sd.tolist() == [[0.5, 0.5]] and s.tolist() == [[F32(math.log(0.5))] * 2]
    assert M.action_of(l, sd, np.array([[1.0, -3.0]])).tolist() == [[0.5, -1.5]]
    # squashed: the correction is the row's sum and comes off every element
    corr = M.squash_correction(a)
    want = math.log(1.0 - math.tanh(1.5) ** 2) * 2  # tanh is odd: both elements give the same term
    assert abs(float(corr[0]) - want) < 1e-6 and corr.dtype == F32
    lps = M.logp_f32(a, loc, ls, F32([[1.0, 2.0]]), True)
    assert lps[0].tolist() == [F32(lp[0, 0] - corr[0]), F32(lp[0, 1] - corr[0])]
    assert M.squash_correction(F32([[13.0]]))[0] == F32(math.log(1e-10))  # 1 - tanh(13)^2 = 2e-11: floored


def test_mirror_env_action_literals():
    low, high = F32([-2.0, 0.0]), F32([2.0, 10.0])
    assert M.env_action(F32([[0.0, 0.0]]), low, high, True).tolist() == [[0.0, 5.0]]
    assert M.env_action(F32([[40.0, -40.0]]), low, high, True).tolist() == [[2.0, 0.0]]  # tanh saturates at +-1 in float64
    assert M.env_action(F32([[0.5, -3.0]]), low, high, False).tolist() == [[1.0, 0.0]]  # -2 + 1.5 / 2 * 4; 0 + (-2 / 2) * 10 clipped
    got = M.env_action(F32([[0.3, 0.3]]), low, high, True)
    space = NpArraySpace(2, low, high)
    assert got[0].tolist() == space.rescale_from(np.tanh(np.float64(F32(0.3))) * np.ones(2), src_low=-1, src_high=1).tolist()
    assert M.env_action(F32([[0.3, 1.7]]), low, high, False)[0].tolist() == space.sanitize(space.rescale_from(F32([0.3, 1.7]))).tolist()


def test_box_muller_moments_over_one_whole_counter():
    """65 536 rows x 8 elements of one counter: N = 524 288 draws.  The mean of N standard normals has standard deviation 1 / sqrt(N), their sample variance
    sqrt(2 / N): five of each."""
    n, K = 65536, 8
    _, ua, ub = M.uniforms(0x5EED0ACE, 11, n, K)
    z = M.box_muller(ua, ub).reshape(-1)
    N = z.size
    mean, var = float(z.mean()), float(z.var())
    print(f"VPPO-NORMAL z over N={N}: mean {mean:.3e} (bar {5 / math.sqrt(N):.3e}), variance - 1 {var - 1:.3e} (bar {5 * math.sqrt(2 / N):.3e}), "
          f"min {z.min():.3f}, max {z.max():.3f}")
    assert N == 524288 and np.isfinite(z).all()
    assert abs(mean) < 5 / math.sqrt(N)
    assert abs(var - 1.0) < 5 * math.sqrt(2.0 / N)


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


def _scripted(squashed):
    K, n = 2, 5
    cfg = ppo_v.Config(discount=0.9, squashed_gaussian_policy=squashed)
    added = []
    w = ppo_v.Worker(cfg, None, SimpleNamespace(add=added.append))
    run = _Run()
    w._set_worker_run(run)
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((n + 1, 3)).astype(F32)
    loc = rng.standard_normal((n, K)).astype(F32)
    ls = (0.5 * rng.standard_normal((n, K))).astype(F32)
    ls[1] = [-4.0, 0.2]  # a scale of 0.018: with z = 7 on it the log-probability lies under log(1e-6) on one element of the row and above it on the other
    z = rng.standard_normal((n, K))
    z[1] = [7.0, 0.1]
    u0 = np.array([0.5, 0.5, 0.01, 0.5, 0.5])  # step 2 takes the epsilon branch
    rewards = [1.0, -0.5, 0.25, 2.0, 1.0]
    random, l, s, sd = M.branch(loc, ls, u0, 0.1, cfg.policy_noise_normal_scale)
    actions = M.action_of(l, sd, z)
    logp = M.logp_f32(actions, l, s, sd, squashed)
    lanes = M.NormalLanes(1, K, 16, 0.9, 10, obs[:1])
    for i in range(n):
        run.state, run.next_state, run.reward, run.terminated, run.done = obs[i], obs[i + 1], rewards[i], i == n - 1, i == n - 1
        # what Worker.policy leaves behind for this draw: the action, and its float64 log-probability from the loc and scale it drew with
        w.action = actions[i].astype(np.float64)
        f = compute_normal_logprob_sgp if squashed else compute_normal_logprob
        w.log_prob = f(w.action, l[i].astype(np.float64), sd[i].astype(np.float64))
        w.on_step(run)
        lanes.push(actions[i:i + 1], logp[i:i + 1], [rewards[i]], [int(i == n - 1)], [int(i == n - 1)], obs[i + 1:i + 2])
    return added, lanes, random, logp


def test_mirror_adds_what_the_worker_adds_on_a_scripted_continuous_episode():
    for squashed in (True, False):
        added, lanes, random, logp = _scripted(squashed)
        assert len(added) == 5 == lanes.ring.added and random.tolist() == [False, False, True, False, False]
        s, s2, a, lp, r, nt, tot = lanes.slots()
        assert a.shape == (5, 2) and lp.shape == (5, 2)
        for k, item in enumerate(added):
            assert np.array_equal(item[0], s[k]) and np.array_equal(item[1], s2[k]) and np.array_equal(F32(item[2]), a[k])
            # the Worker's float64 log-probability beside the mirror's float32 form: the project's bars
            np.testing.assert_allclose(lp[k], np.asarray(item[3], np.float64), rtol=1e-5, atol=1e-6)
            assert F32(item[4]) == r[k] and F32(item[5]) == nt[k] and F32(item[6]) == tot[k], (k, item[6], tot[k])
        # item 3 is step 1 (the walk is reversed): floored on element 0 only, each element on its own
        assert lp[3, 0] == M.LOG_FLOOR and lp[3, 1] > M.LOG_FLOOR and logp[1, 0] < M.LOG_FLOOR
        assert float(added[3][3][0]) == math.log(1e-6) and float(added[3][3][1]) > math.log(1e-6)


def test_mirror_logp_restatements_are_the_projects_functions():
    rng = np.random.default_rng(5)
    x, loc, scale = rng.standard_normal((4, 3)), rng.standard_normal((4, 3)), np.exp(0.3 * rng.standard_normal((4, 3)))
    assert np.array_equal(M.compute_normal_logprob(x, loc, scale), compute_normal_logprob(x, loc, scale))
    np.testing.assert_allclose(M.compute_normal_logprob_sgp(x, loc, scale), compute_normal_logprob_sgp(x, loc, scale), rtol=1e-15, atol=0)


# ---- the Pendulum -----------------------------------------------------------------------------------------------------------------------------------------------
def test_pendulum_mirror_is_envs_pendulum_bit_for_bit():
    from simple_distributed_rl_amd.envs.pendulum import Pendulum

    env = Pendulum()
    rng = np.random.default_rng(9)
    for th, thdot in [(0.0, 0.0), (math.pi, 0.0), (-math.pi, 8.0), (3.5, -8.0), (-7.0, 1.0), (100.0, 0.3)] + [tuple(x) for x in rng.uniform(-9, 9, (40, 2))]:
        for torque in (0.0, 2.0, -2.0, 5.0, -5.0, float(F32(rng.uniform(-2, 2)))):
            env.restore((float(th), float(thdot), 0))
            obs, reward, term, trunc = env.step(np.array([torque], F32))
            m_th, m_thdot, m_reward = M.pendulum_step(float(th), float(thdot), float(F32(torque)))
            assert (env.th, env.thdot, reward) == (m_th, m_thdot, m_reward) and term is False
            assert np.array_equal(obs, M.pendulum_obs(m_th, m_thdot))
    # the remainder takes the divisor's sign: th = -4 is 2 pi - 4 = 2.28 from the top, not -4
    assert abs(M.pendulum_step(-4.0, 0.0, 0.0)[2] + (2 * math.pi - 4.0) ** 2) < 1e-14
    assert M.pendulum_step(0.0, 9.0, 3.0)[1] == 8.0 and M.pendulum_step(0.0, 0.0, 3.0)[1] == 3.0 * 2.0 * 0.05  # the speed and the torque are clipped


def test_pendulum_mirror_reset_and_needs_reset_protocol():
    th, thdot = M.pendulum_reset(5, 2, 0)
    assert -math.pi <= th < math.pi and -1.0 <= thdot < 1.0
    assert M.pendulum_reset(5, 2, 1) != (th, thdot) and M.pendulum_reset(5, 3, 0) != (th, thdot) and M.pendulum_reset(6, 2, 0) != (th, thdot)
    p = M.PendulumLanes(3, 2, 5)
    first = p.reset()
    assert first.shape == (3, 3) and first.dtype == F32 and p.episodes == [1, 1, 1]
    assert np.array_equal(first[2], M.pendulum_obs(*M.pendulum_reset(5, 2, 0)))
    obs, r, term, done = p.step(F32([0.5, 0.0, -0.5]), [False] * 3)
    assert done.tolist() == [0, 0, 0] and not term.any() and (r < 0).all()
    obs, r, term, done = p.step(F32([0.5, 0.0, -0.5]), [False] * 3)
    assert done.tolist() == [1, 1, 1] and p.steps == [2, 2, 2]
    obs, r, term, done = p.step(F32([9.0, 9.0, 9.0]), [True, False, True])  # lanes 0 and 2 only receive a first observation
    assert np.array_equal(obs[0], M.pendulum_obs(*M.pendulum_reset(5, 0, 1))) and r[0] == 0 and done[0] == 0 and p.steps == [0, 3, 0] and p.episodes == [2, 1, 2]
    assert done[1] == 1 and r[1] < 0


# ---- the K-wide store -------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_normal_lanes_floor_each_element_and_keep_the_lane_order():
    lanes = M.NormalLanes(2, 2, 8, 0.5, 4, F32([[10], [20]]))
    lanes.push(F32([[0.1, 0.2], [0.3, 0.4]]), F32([[-20.0, -1.0], [-2.0, -30.0]]), [1.0, 2.0], [1, 0], [1, 1], F32([[11], [21]]))  # both close: lane 0's first
    s, s2, a, lp, r, nt, tot = lanes.slots()
    assert s[:, 0].tolist() == [10.0, 20.0] and a.tolist() == [[F32(0.1), F32(0.2)], [F32(0.3), F32(0.4)]]
    assert lp.tolist() == [[M.LOG_FLOOR, F32(-1.0)], [F32(-2.0), M.LOG_FLOOR]] and nt.tolist() == [0.0, 1.0] and lanes.needs_reset == [True, True]
    lanes.push(F32([[9, 9], [9, 9]]), F32([[-1, -1], [-1, -1]]), [9.0, 9.0], [0, 0], [0, 0], F32([[12], [22]]))  # only the new first observations
    assert lanes.ring.added == 2 and lanes.track == [[], []]
    for i in range(3):
        lanes.push(F32([[i, i], [i, i]]), F32([[-1, -1], [-1, -1]]), [1.0, 1.0], [0, 0], [0, int(i == 2)], F32([[13 + i], [23 + i]]))
    s, s2, a, lp, r, nt, tot = lanes.slots()
    assert lanes.ring.added == 5 and a[2:, 0].tolist() == [2.0, 1.0, 0.0] and tot[2:].tolist() == [1.0, 1.5, 1.75]


# ---- why_not_vppo_engine ----------------------------------------------------------------------------------------------------------------------------------------
def _env(action_space, shape=(3,), steps=200):
    return SimpleNamespace(player_num=1, action_space=action_space, max_episode_steps=steps,
                           observation_space=BoxSpace(shape, -np.inf, np.inf, np.float32, SpaceTypes.CONTINUOUS))


def _cfg(**kw):
    c = ppo_v.Config(**kw)
    c._rl_act_space = NpArraySpace(1, -2.0, 2.0)
    return c


def _one(reason):
    assert reason and "; " not in reason, reason
    return reason


def test_why_not_admits_pendulum_with_admit_normal_and_keeps_todays_answer_without():
    import simple_distributed_rl_amd as srl

    runner = srl.Runner("Pendulum-v1", ppo_v.Config())
    runner.set_device("cpu")
    runner.setup_rl_config()
    old = "a continuous action space: the Normal head's acting kernel is not built, it stays on the plugin path"
    assert why_not_vppo_engine(runner.env, runner.rl_config) == old and why_not_vppo_engine(runner.env, runner.rl_config, 16) == old
    assert why_not_vppo_engine(runner.env, runner.rl_config, n_envs=16, admit_normal=True) == ""
    assert why_not_vppo_engine(_env(NpArraySpace(8, -1.0, 1.0)), _cfg(), admit_normal=True) == ""
    assert why_not_vppo_engine(_env(BoxSpace((2,), np.float32([-1, 0]), np.float32([1, 5]), np.float32, SpaceTypes.CONTINUOUS)), _cfg(), admit_normal=True) == ""
    assert engine_kind(ppo_v.Config()) is None
    # the categorical answers do not depend on the switch
    cart = srl.Runner("CartPole-v1", ppo_v.Config())
    cart.set_device("cpu")
    cart.setup_rl_config()
    assert why_not_vppo_engine(cart.env, cart.rl_config, admit_normal=True) == "" == why_not_vppo_engine(cart.env, cart.rl_config)
    disc = SimpleNamespace(player_num=1, action_space=DiscreteSpace(17), max_episode_steps=500,
                           observation_space=BoxSpace((4,), -np.inf, np.inf, np.float32, SpaceTypes.CONTINUOUS))
    assert why_not_vppo_engine(disc, _cfg(), admit_normal=True) == why_not_vppo_engine(disc, _cfg())


def test_why_not_names_each_new_reason_on_its_own():
    box = lambda *a, **k: BoxSpace(*a, dtype=np.float32, stype=SpaceTypes.CONTINUOUS, **k)  # noqa: E731
    assert _one(why_not_vppo_engine(_env(NpArraySpace(9, -1.0, 1.0)), _cfg(), admit_normal=True)).startswith("9 action elements: outside the envelope (D 1..256")
    assert _one(why_not_vppo_engine(_env(box((2, 2), -1.0, 1.0)), _cfg(), admit_normal=True)).startswith("a continuous action space that is not a flat vector")
    assert _one(why_not_vppo_engine(_env(box((84, 84), 0.0, 1.0, )), _cfg(), admit_normal=True)).startswith("a continuous action space that is not a flat vector")
    assert _one(why_not_vppo_engine(_env(NpArraySpace(2)), _cfg(), admit_normal=True)).startswith("a continuous action space with an infinite bound")
    assert _one(why_not_vppo_engine(_env(box((1,), -1.0, np.inf)), _cfg(), admit_normal=True)).startswith("a continuous action space with an infinite bound")
    assert _one(why_not_vppo_engine(_env(NpArraySpace(1, 1.0, -1.0)), _cfg(), admit_normal=True)) == "a continuous action space whose low is above its high"
    # the reasons that do not depend on the head read as they always did
    assert _one(why_not_vppo_engine(_env(NpArraySpace(1, -2.0, 2.0), shape=(257,)), _cfg(), admit_normal=True)).startswith("257 observation elements: outside")
    assert _one(why_not_vppo_engine(_env(NpArraySpace(1, -2.0, 2.0), steps=None), _cfg(), admit_normal=True)).startswith("no known max_episode_steps")
    assert _one(why_not_vppo_engine(_env(NpArraySpace(1, -2.0, 2.0)), _cfg(batch_size=257), admit_normal=True)) == "batch size 257 above max_batch 256"
    why = why_not_vppo_engine(_env(NpArraySpace(9, -1.0, 1.0), steps=None), _cfg(batch_size=300), n_envs=0, admit_normal=True)
    assert len(why.split("; ")) == 4 and why.startswith("9 action elements")


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------------------------
NEW = ("srlx_vppo_act_normal", "srlx_vppo_lanes_create_normal", "srlx_vppo_lanes_push_normal", "srlx_vppo_lanes_sample_normal", "srlx_pendulum_lane_step")


def test_new_entry_points_are_declared_bound_and_exported():
    from simple_distributed_rl_amd import _native as N

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srlx.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in N.SIGNATURES and hasattr(N.lib(), name), name
    from simple_distributed_rl_amd.device.mlpq import PendulumLaneVecEnv  # noqa: F401
    from simple_distributed_rl_amd.device.vector_runner import FloatActionHostVecEnv, HostVecEnv
    from simple_distributed_rl_amd.device.vppo import VppoUpdate
    from simple_distributed_rl_amd.device.vppo_engine import VppoEngine, VppoNormalEngine

    assert issubclass(VppoNormalEngine, VppoEngine) and issubclass(FloatActionHostVecEnv, HostVecEnv) and callable(VppoUpdate.act_normal)
    acts = np.float32([[0.5, -1.0], [2.0, 3.0]])
    assert FloatActionHostVecEnv._lane_action(None, acts, 1).tolist() == [2.0, 3.0] and HostVecEnv._lane_action(None, np.int32([4, 7]), 1) == 7


def test_new_refusals_that_need_no_device():
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    st = lib.srlx_vppo_act_normal(None, 1, None, 0, None, 0.1, 0.5, 1, -1.0, 1.0, *[None] * 9)
    assert st == N.ERR_INVALID and b"vppo_act_normal: NULL handle" in lib.srlx_last_error()
    h = N.c_p()
    for args, word in (((0, 3, 200, 100, 0.9, 1), b"0 lanes"), ((4097, 3, 200, 100, 0.9, 1), b"4097 lanes"), ((1, 0, 200, 100, 0.9, 1), b"observation length 0"),
                       ((1, 3, 0, 100, 0.9, 1), b"max_episode_steps 0"), ((1, 3, 4095, 100, 0.9, 1), b"max_episode_steps 4095"), ((1, 3, 200, 0, 0.9, 1), b"capacity 0"),
                       ((1, 3, 200, 100, 1.5, 1), b"discount 1.5"), ((1, 3, 200, 100, 0.9, 0), b"0 action elements"), ((1, 3, 200, 100, 0.9, 9), b"9 action elements")):
        st = lib.srlx_vppo_lanes_create_normal(ctypes.byref(h), *args, 0)
        assert st == N.ERR_INVALID and not h and b"vppo_lanes_create_normal" in lib.srlx_last_error() and word in lib.srlx_last_error(), (args, lib.srlx_last_error())
    assert lib.srlx_vppo_lanes_create_normal(None, 1, 3, 200, 100, 0.9, 1, 0) == N.ERR_INVALID and b"NULL handle pointer" in lib.srlx_last_error()
    assert lib.srlx_vppo_lanes_push_normal(None, *[None] * 8) == N.ERR_INVALID and b"vppo_lanes_push_normal: NULL handle" in lib.srlx_last_error()
    assert lib.srlx_vppo_lanes_sample_normal(None, 1, 0, *[None] * 9) == N.ERR_INVALID and b"vppo_lanes_sample_normal: NULL handle" in lib.srlx_last_error()
    for args in ((0, None, None, None, None, None, 200, 0, None, None, None, None, None), (4, None, None, None, None, None, 200, 0, None, None, None, None, None)):
        assert lib.srlx_pendulum_lane_step(*args) == N.ERR_INVALID and b"pendulum_lane_step" in lib.srlx_last_error()
