"""srlx_pendulum_lane_step on the GPU (csrc/srlx_vppo_lanes.hip, device/mlpq.py: PendulumLaneVecEnv) against the Pendulum of
tests/vppo_normal_reference.py, which tests/test_vppo_normal_engine_cpu.py holds to envs/pendulum.py bit for bit.  Every step is fed the device's own previous
state.  Bars: the state within 1e-12 of the mirror's (a step is a dozen float64 operations on values under 10 around one sin: the device's sin and the host's
are each within an ulp or two of the true value, 2e-15 on 15 sin th, and 1e-12 is hundreds of that); observations and reward within one float32 ulp (each is one
rounding of a float64 value that differs by at most that much)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_normal_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED = 0xBEEF


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _env(E, max_steps, seed=SEED):
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.mlpq import PendulumLaneVecEnv

    needs_reset = torch.zeros(E, dtype=torch.uint8, device="cuda")
    replay = SimpleNamespace(obs_uint8=False, F=3, E=E, seed=seed, dev=torch.device("cuda:0"), needs_reset_ptr=N.tptr(needs_reset))
    return PendulumLaneVecEnv(replay, max_steps=max_steps), needs_reset


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("E,max_steps,T", [(1, 1, 6), (5, 3, 14), (65, 200, 205), (5, 200, 30)], ids=["E1-steps1", "E5-steps3", "E65-steps200", "E5-wild-torques"])
def test_steps_resets_and_done_match_the_mirror(E, max_steps, T):
    env, needs_reset = _env(E, max_steps)
    first = _host(env.reset())
    # the reset of every lane (NULL torques): episode 0 of each lane, keyed as documented
    want_state = np.array([M.pendulum_reset(SEED, e, 0) for e in range(E)])
    assert np.array_equal(_host(env.state), want_state), "the first states are not the documented keyed draws, bit for bit"
    assert int(_ulps(first, np.stack([M.pendulum_obs(*s) for s in want_state])).max()) <= 1
    assert _host(env.episodes).tolist() == [1] * E and _host(env.steps).tolist() == [0] * E
    g = np.random.default_rng(E + max_steps)
    wild = max_steps == 200 and E == 5
    worst_state, worst_obs, worst_reward, resets = 0.0, 0, 0, 0
    done_prev = np.zeros(E, np.uint8)
    for t in range(T):
        torques = (g.uniform(-6, 6, E) if wild else g.uniform(-2, 2, E)).astype(F32)
        if wild and t == 3:
            env.state.copy_(torch.tensor([[-7.0, 8.0], [100.0, -8.0], [3.5, 7.9], [-3.2, -7.9], [0.0, 0.0]], dtype=torch.float64))  # far from the top, at the speed clip
        before, steps_before, episodes_before = _host(env.state), _host(env.steps), _host(env.episodes)
        needs_reset.copy_(torch.from_numpy(done_prev))
        obs, reward, term, done = (_host(x) for x in env.step(torch.from_numpy(torques).cuda()))
        state, steps_after, episodes_after = _host(env.state), _host(env.steps), _host(env.episodes)
        for e in range(E):
            if done_prev[e]:  # the lock-step only delivers the next episode's first observation
                th, thdot = M.pendulum_reset(SEED, e, int(episodes_before[e]))
                assert (state[e, 0], state[e, 1]) == (th, thdot) and reward[e] == 0 and done[e] == 0 and term[e] == 0
                assert steps_after[e] == 0 and episodes_after[e] == episodes_before[e] + 1
                resets += 1
                want_r, want_done = F32(0), 0
            else:
                th, thdot, r = M.pendulum_step(float(before[e, 0]), float(before[e, 1]), float(torques[e]))
                worst_state = max(worst_state, abs(state[e, 0] - th), abs(state[e, 1] - thdot))
                want_r, want_done = F32(r), int(steps_before[e] + 1 >= max_steps)
                assert steps_after[e] == steps_before[e] + 1 and episodes_after[e] == episodes_before[e] and done[e] == want_done and term[e] == 0
                worst_reward = max(worst_reward, int(_ulps(reward[e:e + 1], np.array([want_r]))[0]))
            worst_obs = max(worst_obs, int(_ulps(obs[e], M.pendulum_obs(th, thdot)).max()))
        done_prev = done
    print(f"PENDULUM-LANES E{E} max_steps {max_steps}: {T} lock-steps, {resets} lane resets; state {worst_state:.3e} (bar 1e-12), obs {worst_obs} ulp, reward "
          f"{worst_reward} ulp (bars 1)")
    assert worst_state <= 1e-12 and worst_obs <= 1 and worst_reward <= 1
    assert resets >= (T - 1) // (max_steps + 1) * E and (resets > 0 or T <= max_steps)


def test_null_torques_reset_every_lane_and_refusals():
    from simple_distributed_rl_amd import _native as N

    env, needs_reset = _env(5, 3)
    env.reset()
    a = _host(env.state)
    env.reset()  # every lane's NEXT episode
    b = _host(env.state)
    assert np.array_equal(b, np.array([M.pendulum_reset(SEED, e, 1) for e in range(5)])) and not np.array_equal(a, b)
    assert _host(env.episodes).tolist() == [2] * 5
    lib = N.lib()
    t = torch.zeros(5, dtype=torch.float32, device="cuda")
    # a step without the scalar outputs is refused before any launch
    st = lib.srlx_pendulum_lane_step(5, N.tptr(env.state), N.tptr(env.steps), N.tptr(env.episodes), N.tptr(needs_reset), N.tptr(t), 3, SEED, N.tptr(env.next_obs), None,
                                     None, None, None)
    assert st == N.ERR_INVALID and b"pendulum_lane_step" in lib.srlx_last_error()
    assert np.array_equal(_host(env.state), b)
