"""The yardstick of the V-PPO engine's Normal head (srlx_vppo_act_normal, the K-wide episode store, srlx_pendulum_lane_step), written as another
program: numpy arrays and Python floats where the kernels have threads, Python lists where they have rings, the keyed uniforms from the oracle's restatement of
the counter generator (oracle/hot_path_oracle.py: rng_uniform).  It reads nothing from the library.  The store is the categorical mirror's
(tests/vppo_engine_reference.py: Ring, close_episode, floyd, draw) with K-wide actions and log-probabilities in front of it."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hot_path_oracle import rng_u64, rng_uniform, u53  # noqa: E402
from vppo_engine_reference import LOG_FLOOR, Lanes, close_episode, draw  # noqa: E402,F401

F32 = np.float32
HALF_LOG_2PI = F32(0.91893853320467274178)  # 0.5 log(2 pi) as the float32 the update holds
SQUASH_FLOOR = 1e-10
PENDULUM_KEY = 0x50454E44554C554D  # "PENDULUM"


# ---- acting ---------------------------------------------------------------------------------------------------------------------------------------------------
def uniforms(seed, counter, n_rows, K):
    """(U0 [n], Ua [n][K], Ub [n][K]): row r reads the generator at (2 K + 1) r (U0), + 1 + 2 j (Ua of element j) and + 2 + 2 j (Ub)."""
    u = rng_uniform(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), counter, (2 * K + 1) * n_rows).reshape(n_rows, 2 * K + 1)
    return u[:, 0], u[:, 1::2], u[:, 2::2]


def box_muller(ua, ub):
    """One standard normal per pair, float64: sqrt(-2 log(1 - Ua)) cos(2 pi Ub)."""
    ua, ub = np.asarray(ua, np.float64), np.asarray(ub, np.float64)
    return np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(2.0 * np.pi * ub)


def scale_of(log_scale):
    """exp of a float32 log-scale as a float32 (the float64 exp rounded once: the correctly rounded value)."""
    return np.exp(np.asarray(log_scale, F32).astype(np.float64)).astype(F32)


def branch(loc, log_scale, u0, epsilon, noise_scale, scale=None):
    """(random mask [n], loc, log-scale, scale [n][K] float32) the draw uses: the head's, or (0, log(noise), noise) on every element of a row with U0 < epsilon.
    `scale`: the head's float32 exp(log_scale) where the caller has the device's own (the kernels call the device's expf, which is within an ulp of the correctly
    rounded `scale_of` and not always equal to it); None: `scale_of`."""
    loc, log_scale = np.asarray(loc, F32), np.asarray(log_scale, F32)
    random = np.asarray(u0) < epsilon
    r = random[:, None]
    head_scale = scale_of(log_scale) if scale is None else np.asarray(scale, F32)
    return (random, np.where(r, F32(0.0), loc).astype(F32), np.where(r, F32(math.log(noise_scale)), log_scale).astype(F32),
            np.where(r, F32(noise_scale), head_scale).astype(F32))


def action_of(loc, sd, z):
    """np.random.normal(loc, scale) on the draw z, float64, rounded to the float32 the item holds: the value BEFORE tanh."""
    return (np.asarray(loc, F32).astype(np.float64) + np.asarray(sd, F32).astype(np.float64) * np.asarray(z, np.float64)).astype(F32)


def squash_correction(actions):
    """sum_i log(clip(1 - tanh(a_i)^2, 1e-10, 1)) per row in float64 (a running sum in element order), rounded to float32."""
    a = np.asarray(actions, F32).astype(np.float64)
    out = np.empty(len(a), F32)
    for r in range(len(a)):
        s = 0.0
        for x in a[r]:
            th = math.tanh(float(x))
            s = s + math.log(min(max(1.0 - th * th, SQUASH_FLOOR), 1.0))
        out[r] = F32(s)
    return out


def logp_f32(actions, loc, log_scale, sd, squashed):
    """The update's float32 form on the stored float32 action, every operation rounded to float32: u = (a - loc) / sd;
    (-0.5 log 2 pi - ls - 0.5 (u u)) - corr."""
    a, loc, ls, sd = (np.asarray(x, F32) for x in (actions, loc, log_scale, sd))
    corr = squash_correction(a)[:, None] if squashed else F32(0.0)
    u = ((a - loc) / sd).astype(F32)
    return (((-HALF_LOG_2PI - ls).astype(F32) - (F32(0.5) * (u * u).astype(F32)).astype(F32)).astype(F32) - corr).astype(F32)


def compute_normal_logprob(x, loc, scale):
    """rl/functions.py: compute_normal_logprob restated in float64."""
    x, loc, scale = (np.asarray(v, np.float64) for v in (x, loc, scale))
    return -0.5 * math.log(2.0 * math.pi) - np.log(scale) - 0.5 * (((x - loc) / scale) ** 2)


def compute_normal_logprob_sgp(x, loc, scale):
    """rl/functions.py: compute_normal_logprob_sgp restated in float64 (x before tanh; the correction summed over the elements, subtracted from each)."""
    x = np.asarray(x, np.float64)
    return compute_normal_logprob(x, loc, scale) - np.sum(np.log(np.clip(1.0 - np.tanh(x) ** 2, SQUASH_FLOOR, 1.0)), axis=-1, keepdims=True)


def env_action(actions, low, high, squashed):
    """NpArraySpace.rescale_from of tanh(a) (squashed) or a (plain) from [-1, 1] onto [low, high] in float64, rounded to float32, clipped to the bounds."""
    a = np.asarray(actions, F32).astype(np.float64)
    low, high = np.asarray(low, F32), np.asarray(high, F32)
    x = np.tanh(a) if squashed else a
    e = (low.astype(np.float64) + (x + 1.0) / 2.0 * (high.astype(np.float64) - low.astype(np.float64))).astype(F32)
    return np.clip(e, low, high).astype(F32)


def act(loc, log_scale, seed, counter, epsilon, noise_scale, z=None, scale=None):
    """srlx_vppo_act_normal for rows whose head outputs are given: (actions f32, random mask, loc, log-scale, scale used, z).  `z`: the kernel's own draws, where the
    comparison is about what follows them; `scale`: as in `branch`."""
    n, K = np.asarray(loc).shape
    u0, ua, ub = uniforms(seed, counter, n, K)
    if z is None:
        z = box_muller(ua, ub)
    random, l, ls, sd = branch(loc, log_scale, u0, epsilon, noise_scale, scale)
    return action_of(l, sd, z), random, l, ls, sd, z


# ---- the Pendulum ---------------------------------------------------------------------------------------------------------------------------------------------
def pendulum_step(th, thdot, torque):
    """envs/pendulum.py: step on Python floats, line for line: (th, thdot, reward)."""
    u = min(max(float(torque), -2.0), 2.0)
    ang = ((th + math.pi) % (2 * math.pi)) - math.pi
    reward = -(ang * ang + 0.1 * thdot * thdot + 0.001 * u * u)
    thdot = min(max(thdot + (3 * 10.0 / (2 * 1.0) * math.sin(th) + 3.0 / (1.0 * 1.0 * 1.0) * u) * 0.05, -8.0), 8.0)
    th = th + thdot * 0.05
    return th, thdot, reward


def pendulum_obs(th, thdot):
    return np.array([math.cos(th), math.sin(th), thdot], F32)


def pendulum_reset(seed, lane, episode):
    """The first state of `lane`'s episode number `episode`: th = -pi + 2 pi U_0, thdot = -1 + 2 U_1, keyed by (seed ^ "PENDULUM", lane << 32 | episode, k)."""
    key = np.uint64(((lane << 32) | (episode & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF)
    u = u53(rng_u64(np.uint64((seed ^ PENDULUM_KEY) & 0xFFFFFFFFFFFFFFFF), key, np.arange(2, dtype=np.uint64)))
    return -math.pi + (2.0 * math.pi) * float(u[0]), -1.0 + 2.0 * float(u[1])


class PendulumLanes:
    """E pendulums under the needs_reset protocol: `step(torques, needs_reset)` -> (obs [E][3], reward, terminated, done)."""

    def __init__(self, E, max_steps, seed):
        self.E, self.max_steps, self.seed = E, max_steps, seed
        self.state = [(0.0, 0.0)] * E
        self.steps, self.episodes = [0] * E, [0] * E

    def _reset_lane(self, e):
        self.state[e] = pendulum_reset(self.seed, e, self.episodes[e])
        self.episodes[e] += 1
        self.steps[e] = 0

    def reset(self):
        for e in range(self.E):
            self._reset_lane(e)
        return np.stack([pendulum_obs(*s) for s in self.state])

    def step(self, torques, needs_reset):
        reward, done = np.zeros(self.E, F32), np.zeros(self.E, np.uint8)
        for e in range(self.E):
            if needs_reset[e]:
                self._reset_lane(e)
                continue
            th, thdot, r = pendulum_step(*self.state[e], float(F32(torques[e])))
            self.state[e] = (th, thdot)
            self.steps[e] += 1
            reward[e], done[e] = F32(r), int(self.steps[e] >= self.max_steps)
        return np.stack([pendulum_obs(*s) for s in self.state]), reward, np.zeros(self.E, np.uint8), done


# ---- the trackings and the ring ---------------------------------------------------------------------------------------------------------------------------------
class NormalLanes(Lanes):
    """The categorical mirror's lanes with a float32 action of K elements and K log-probabilities per step, each floored on its own."""

    def __init__(self, E, K, capacity, discount, max_episode_steps, first_obs):
        super().__init__(E, capacity, discount, max_episode_steps, first_obs)
        self.K = K

    def push(self, actions, logp, rewards, terminated, done, next_obs):
        actions, logp = np.asarray(actions, F32).reshape(self.E, self.K), np.asarray(logp, F32).reshape(self.E, self.K)
        for e in range(self.E):  # the closing lanes append in lane order
            nxt = np.asarray(next_obs[e], F32).copy()
            if self.needs_reset[e]:
                self.track[e] = []
            elif self.track[e] is None:
                pass
            else:
                self.track[e].append((self.obs[e], nxt, actions[e].copy(), np.maximum(logp[e], LOG_FLOOR), F32(rewards[e]), F32(0.0 if terminated[e] else 1.0)))
                if len(self.track[e]) > self.max_steps:
                    self.error, self.track[e] = 1, None
                elif done[e]:
                    for item in close_episode(self.track[e], self.discount):
                        self.ring.add(item)
                    self.track[e] = []
            self.obs[e] = nxt
            self.needs_reset[e] = bool(done[e])

    def slots(self):
        """The item ring in slot order as arrays: s, s', action [n][K], logp [n][K], reward, not_terminated, total."""
        b = self.ring.buffer
        cols = list(zip(*b)) if b else [[]] * 7
        return tuple(np.array(c, F32) for c in cols)
