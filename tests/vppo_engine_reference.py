"""The yardstick of the V-PPO engine's launches outside the update (srlx_vppo_act, srlx_vppo_lanes_push / _sample), written as another program:
numpy arrays and Python floats where the kernels have threads, Python lists where they have rings, the keyed uniforms from the oracle's restatement of the
counter generator (oracle/hot_path_oracle.py: rng_uniform).  It reads nothing from the library."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from hot_path_oracle import rng_uniform  # noqa: E402

LOG_FLOOR = np.float32(math.log(1e-6))  # Worker.on_step's floor, as the float32 the item holds


# ---- acting ---------------------------------------------------------------------------------------------------------------------------------------------------
def uniforms(seed, counter, n_rows):
    """(U0, U1) per row: what srlx_rng_uniform(seed, counter, 2 n_rows) writes at 2 r and 2 r + 1."""
    u = rng_uniform(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), counter, 2 * n_rows).reshape(n_rows, 2)
    return u[:, 0], u[:, 1]


def cdf(logits):
    """Running sums, in action order, of exp(z - max z) in float64."""
    z = np.asarray(logits, np.float32).astype(np.float64)
    w = np.exp(z - z.max(axis=1, keepdims=True))
    c = np.empty_like(w)
    for r in range(len(w)):
        acc = 0.0
        for k in range(w.shape[1]):
            acc = acc + float(w[r, k])
            c[r, k] = acc
    return c


def inverse_cdf(c, u1):
    """The first k with u1 c_{A-1} < c_k; A - 1 when there is none."""
    out = np.empty(len(c), np.int32)
    for r in range(len(c)):
        thr = float(u1[r]) * float(c[r, -1])
        out[r] = next((k for k in range(c.shape[1]) if thr < c[r, k]), c.shape[1] - 1)
    return out


def boundary_gap(c, u1):
    """How far each row's u1 c_{A-1} lies from the nearest boundary, relative to c_{A-1}."""
    thr = (np.asarray(u1) * c[:, -1])[:, None]
    return (np.abs(c - thr) / c[:, -1:]).min(axis=1)


def uniform_actions(u1, A):
    """sample_action(): min(A - 1, floor(u1 A))."""
    return np.minimum(A - 1, np.floor(np.asarray(u1, np.float64) * A).astype(np.int64)).astype(np.int32)


def act(logits, seed, counter, epsilon):
    """(actions, random mask, cdf) of srlx_vppo_act for rows whose logits are given."""
    n, A = np.asarray(logits).shape
    u0, u1 = uniforms(seed, counter, n)
    c = cdf(logits)
    random = u0 < epsilon
    return np.where(random, uniform_actions(u1, A), inverse_cdf(c, u1)).astype(np.int32), random, c


def uniform_logp(A):
    return np.float32(math.log(1.0 / A))


# ---- the trackings and the ring ---------------------------------------------------------------------------------------------------------------------------------
class Ring:
    """ReplayBuffer.add (rl/memories/replay_buffer.py:72-78) on a list of slots."""

    def __init__(self, capacity):
        self.capacity, self.buffer, self.idx, self.added = capacity, [], 0, 0

    def add(self, item):
        if len(self.buffer) < self.capacity:
            self.buffer.append(item)
        else:
            self.buffer[self.idx] = item
        self.idx = (self.idx + 1) % self.capacity
        self.added += 1

    def length(self):
        return len(self.buffer)


def close_episode(trackings, discount):
    """Worker.on_step's walk: the episode's items in reversed order, each with the discounted return to the episode's end (a Python float chain, rounded to
    float32 where the item is stored).  A tracking is (s, s', action, logp, reward, not_terminated)."""
    out, total = [], 0.0
    for b in reversed(trackings):
        total = float(b[4]) + discount * total
        out.append(tuple(b) + (np.float32(total),))
    return out


class Lanes:
    """E lanes' trackings in front of one Ring, driven like the store: `push` per lock-step."""

    def __init__(self, E, capacity, discount, max_episode_steps, first_obs):
        self.E, self.discount, self.max_steps = E, float(discount), max_episode_steps
        self.ring = Ring(capacity)
        self.obs = [np.asarray(first_obs[e], np.float32).copy() for e in range(E)]
        self.track = [[] for _ in range(E)]
        self.needs_reset = [False] * E
        self.error = 0

    def push(self, actions, logp, rewards, terminated, done, next_obs):
        for e in range(self.E):  # the closing lanes append in lane order
            nxt = np.asarray(next_obs[e], np.float32).copy()
            if self.needs_reset[e]:  # the lock-step only delivers the new first observation
                self.track[e] = []
            elif self.track[e] is None:  # the rest of an episode that outlived the ring is dropped with it
                pass
            else:
                self.track[e].append((self.obs[e], nxt, int(actions[e]), max(np.float32(logp[e]), LOG_FLOOR), np.float32(rewards[e]),
                                      np.float32(0.0 if terminated[e] else 1.0)))
                if len(self.track[e]) > self.max_steps:
                    self.error, self.track[e] = 1, None
                elif done[e]:
                    for item in close_episode(self.track[e], self.discount):
                        self.ring.add(item)
                    self.track[e] = []
            self.obs[e] = nxt
            self.needs_reset[e] = bool(done[e])

    def slots(self):
        """The item ring in slot order as arrays: s, s', action, logp, reward, not_terminated, total."""
        b = self.ring.buffer
        cols = list(zip(*b)) if b else [[]] * 7
        return (np.array(cols[0], np.float32), np.array(cols[1], np.float32), np.array(cols[2], np.int32), np.array(cols[3], np.float32),
                np.array(cols[4], np.float32), np.array(cols[5], np.float32), np.array(cols[6], np.float32))


# ---- the draw -------------------------------------------------------------------------------------------------------------------------------------------------
def floyd(N, B, U):
    """B distinct values of [0, N) by Floyd's algorithm on the uniforms U [B], in the order they are chosen."""
    chosen = []
    for i, j in enumerate(range(N - B, N)):
        t = min(j, int(math.floor(float(U[i]) * (j + 1))))
        chosen.append(j if t in chosen else t)
    return chosen


def draw(seed, draw_index, N, B):
    return floyd(N, B, rng_uniform(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), draw_index, B))
