"""The schedules and the case table of tests/test_vppo_lanes_envelope_{cpu,gpu}.py: V-PPO's episode store (csrc/srlx_vppo_lanes.hip) over the
envelope `create` admits.  The mirror stays tests/vppo_engine_reference.py: Lanes and tests/vppo_normal_reference.py: NormalLanes; this module only feeds them.
Needs no GPU and reads nothing from the library.

In the kernel's terms: a closing lane of n steps numbers its items j = 0..n-1 from its LAST step; its threads walk j in strides of 256.  Of the S items one
lock-step adds, the first max(0, S - capacity) of the sequence are dropped; `cut` below is the j at which that boundary falls inside one lane's episode."""
import ctypes
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_engine_reference as MC  # noqa: E402
import vppo_normal_reference as MN  # noqa: E402

F32 = np.float32
FLOOR = F32(math.log(1e-6))
STRIDE = 256  # threads of a closing workgroup


def schedule(E, D, T, key, lengths, K=0, reward_scale=False):
    """T lock-steps of hand-fed fields as stacked arrays [T][E]...: lane e plays episodes whose lengths cycle through `lengths` from index e % len(lengths), each
    followed by the lock-step that only delivers the next first observation (whose other fields are noise the store must ignore).  Log-probabilities on both sides
    of log(1e-6), lane 0's (element 0) on two lock-steps of four at the float just under the floor and at the floor itself; a lane's closing steps alternate
    between termination and truncation (lane e's i-th close terminates when i + e is even), so that two closes anywhere hold both; `reward_scale` multiplies every
    reward by 1e4, 1 or 1e-4 at random.  K = 0: int32 actions [T][E] and log-probabilities [T][E]; K > 0: float32 [T][E][K] both.
    Returns (first observations [E][D], plan)."""
    g = np.random.default_rng(key)
    done = np.zeros((T, E), np.uint8)
    for e in range(E):
        t, i = 0, e % len(lengths)
        while t + lengths[i] - 1 < T:
            t += lengths[i]
            done[t - 1, e] = 1
            t += 1  # the first observation of the next episode
            i = (i + 1) % len(lengths)
    wide = (T, E, K) if K else (T, E)
    logp = np.where(g.random(wide) < 0.3, -14.0 - g.random(wide), -3.0 * g.random(wide)).astype(F32)
    lane0 = logp[:, 0, 0] if K else logp[:, 0]  # (views)
    lane0[0::4], lane0[1::4] = np.nextafter(FLOOR, F32(-20)), FLOOR  # the other two lock-steps of four keep their random values: one lane alone holds both sides
    if K > 1:
        logp[:, 0, K - 1] = F32(-0.25)  # one row floored on one element and not on another
    rewards = g.standard_normal((T, E)).astype(F32)
    if reward_scale:
        rewards = (rewards * g.choice(np.array([1e4, 1.0, 1e-4], F32), (T, E))).astype(F32)
    plan = dict(actions=g.standard_normal(wide).astype(F32) if K else g.integers(0, 5, wide).astype(np.int32), logp=logp, rewards=rewards,
                terminated=(done & ((np.cumsum(done, axis=0) + np.arange(E) + 1) % 2 == 0)).astype(np.uint8), done=done, next_obs=g.standard_normal((T, E, D)).astype(F32))
    return g.standard_normal((E, D)).astype(F32), plan


def mirror_of(E, K, capacity, discount, steps, first):
    return MN.NormalLanes(E, K, capacity, discount, steps, first) if K else MC.Lanes(E, capacity, discount, steps, first)


def inputs(c):
    """(first observations, plan, a fresh mirror) of a Case or a Draw: one key per table entry, the same in both test files."""
    if isinstance(c, Case):
        first, plan = schedule(c.E, c.D, c.T, 1000 + CASES.index(c), c.lengths, c.K, c.reward_scale)
        return first, plan, mirror_of(c.E, c.K, c.capacity, c.discount, c.steps, first)
    first, plan = schedule(c.E, c.D, c.T, 2000 + DRAWS.index(c), [1], c.K)
    return first, plan, mirror_of(c.E, c.K, c.capacity, 0.95, 1, first)


def push(mirror, plan, t):
    """One lock-step into the mirror; returns [(lane, n)] of the episodes it closes, in lane order (read off the mirror's own trackings before the push)."""
    done = plan["done"][t]
    closing = [(e, len(mirror.track[e]) + 1) for e in np.nonzero(done)[0] if not mirror.needs_reset[e] and mirror.track[e] is not None]
    mirror.push(plan["actions"][t], plan["logp"][t], plan["rewards"][t], plan["terminated"][t], done, plan["next_obs"][t])
    return closing


class Seen:
    """What a run met, for the `VPPO-LANES-ENV` line and the CPU file's assertions."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.longest = self.closes = self.big_s = self.cut = self.cut_of = self.highest_lane = 0
        self.lane0_idle = False  # some lock-step closed lanes while lane 0 did not close

    def note(self, closing):
        if not closing:
            return
        S = sum(n for _, n in closing)
        self.longest = max(self.longest, max(n for _, n in closing))
        self.closes, self.big_s = max(self.closes, len(closing)), max(self.big_s, S)
        self.highest_lane = max(self.highest_lane, closing[-1][0])
        self.lane0_idle |= closing[0][0] != 0
        before = 0
        for _, n in closing:
            j = S - self.capacity - before  # the first j of this lane that survives
            if 0 < j < n and j > self.cut:
                self.cut, self.cut_of = j, n
            before += n


# name, lanes, observation length, action elements (0: categorical), max_episode_steps, capacity, episode lengths, lock-steps, discount, reward_scale,
# `every`: compare after every lock-step that closes a lane (False: once, after the last), and what the schedule must reach (asserted on the mirror alone by
# tests/test_vppo_lanes_envelope_cpu.py): longest episode at least, most closes in one lock-step at least, largest S above the capacity, the cut (see above) at
# least, the highest closing lane at least, added above the capacity.
Case = namedtuple("Case", "name E D K steps capacity lengths T discount reward_scale every longest closes s_over cut lane added_over")


def _case(name, E, D, K, steps, capacity, lengths, T, discount=0.95, reward_scale=False, every=True, longest=1, closes=1, s_over=False, cut=0, lane=0,
          added_over=True):
    return Case(name, E, D, K, steps, capacity, lengths, T, discount, reward_scale, every, longest, closes, s_over, cut, lane, added_over)


_STRIDE_LENGTHS = [600, 257, 256, 255, 1]
_TWO = 2 * 4095 + 1  # two whole 4094-step episodes and the lock-step behind the second
CASES = [
    # 1. episodes across the 256-thread stride (a third trip at 600): lane 0 starts at 600, lane 1 at 257, so lane 1 closes while lane 0 does not
    _case("stride-D5", 2, 5, 0, 600, 1000, _STRIDE_LENGTHS, 2800, longest=600, lane=1),
    _case("stride-D4-K3", 2, 4, 3, 600, 1000, _STRIDE_LENGTHS, 2800, longest=600, lane=1),
    # 2. the envelope's longest episode: R = 4096, both LDS arrays full, the second episode wraps the tracking ring.  Capacity 4000 cuts the one lane's close at
    # j = 94 (inside the first stride: the episode's step 4000); capacity 3700 is there for a cut inside the second stride, j = 394
    _case("longest-cap8192", 1, 4, 0, 4094, 8192, [4094], _TWO, longest=4094, added_over=False),
    _case("longest-cap4000", 1, 4, 0, 4094, 4000, [4094], _TWO, longest=4094, s_over=True, cut=94),
    _case("longest-cap3700", 1, 4, 0, 4094, 3700, [4094], _TWO, longest=4094, s_over=True, cut=394),
    _case("longest-cap8192-K8", 1, 4, 8, 4094, 8192, [4094], _TWO, longest=4094, added_over=False),
    _case("longest-cap4000-K8", 1, 4, 8, 4094, 4000, [4094], _TWO, longest=4094, s_over=True, cut=94),
    _case("longest-cap3700-K8", 1, 5, 8, 4094, 3700, [4094], _TWO, longest=4094, s_over=True, cut=394),
    # 3. the discount at both ends on rewards of mixed magnitude
    _case("discount0", 1, 3, 0, 300, 1000, [300], 2 * 301 + 1, discount=0.0, reward_scale=True, longest=300, added_over=False),
    _case("discount1", 1, 3, 0, 300, 1000, [300], 2 * 301 + 1, discount=1.0, reward_scale=True, longest=300, added_over=False),
    _case("discount1-longest", 1, 4, 0, 4094, 8192, [4094], _TWO, discount=1.0, reward_scale=True, longest=4094, added_over=False),
    # 4. many lanes: the prefix loop's second trip (lane 256 closes), every lane closing in one lock-step, S > capacity spread over more than 256 lanes
    _case("lanes-E257-D1", 257, 1, 0, 3, 256, [3, 1, 2], 14, longest=3, closes=257, s_over=True, lane=256),
    _case("lanes-E300-D1", 300, 1, 0, 3, 256, [3, 1, 2], 14, longest=3, closes=257, s_over=True, lane=299),
    _case("lanes-E257-D3-K8", 257, 3, 8, 3, 256, [3, 1, 2], 14, longest=3, closes=257, s_over=True, lane=256),
    _case("lanes-E300-D3-K8", 300, 3, 8, 3, 256, [3, 1, 2], 14, longest=3, closes=257, s_over=True, lane=299),
    _case("lanes-E4096-D4", 4096, 4, 0, 2, 16384, [2, 1], 12, longest=2, closes=4096, lane=4095),
    # 5. the engine's own Pendulum shape: every lane closes 200 steps in one lock-step, S = 204 800 into 100 000 slots; compared once, after the close
    _case("pendulum-E1024", 1024, 3, 1, 201, 100_000, [200], 201, every=False, longest=200, closes=1024, s_over=True, lane=1023),
]
CASE_IDS = [c.name for c in CASES]

# `sample` at its edges (test 6): name, observation length, action elements, capacity, lanes of one-step episodes, lock-steps, batch, outputs offset by one float
Draw = namedtuple("Draw", "name D K capacity E T B offset")
DRAWS = [
    Draw("D4-offset", 4, 0, 64, 4, 100, 64, 1),  # the scalar gather at D % 4 == 0, on a wrapped ring
    Draw("D256-K8-offset-B256", 256, 8, 300, 8, 80, 256, 1),
    Draw("D256-K8-B256", 256, 8, 300, 8, 80, 256, 0),
    Draw("B-equals-N-equals-capacity-256", 4, 0, 256, 8, 64, 256, 0),
    Draw("D8", 8, 3, 64, 4, 40, 33, 0),
    Draw("D12", 12, 0, 64, 4, 40, 33, 0),
    Draw("D8-offset", 8, 0, 64, 4, 40, 33, 1),
    Draw("D12-K8-offset", 12, 8, 64, 4, 40, 33, 1),
    Draw("added-40x-capacity", 5, 0, 16, 8, 160, 16, 0),
]
DRAW_IDS = [d.name for d in DRAWS]

# srlx_pendulum_lane_step past one workgroup (test 8): lanes, max_steps, lock-steps
PENDULUMS = [(257, 3, 10), (1000, 3, 10), (65536, 2, 3)]

# srlx_vppo_lanes_create at the ends of its envelope (test 7): LOW holds every size at its minimum (K None: the categorical entry point); each entry of REFUSED and
# ACCEPTED changes one argument.  All maxima together would ask for tens of gigabytes.
LOW = dict(E=1, D=1, steps=1, capacity=1, discount=0.0, K=None)
REFUSED = [dict(E=0), dict(E=4097), dict(D=0), dict(D=257), dict(steps=0), dict(steps=4095), dict(capacity=0), dict(capacity=2 ** 24 + 1), dict(discount=-0.1),
           dict(discount=1.1), dict(discount=float("nan")), dict(K=0), dict(K=9)]
ACCEPTED = [dict(), dict(E=4096), dict(D=256), dict(steps=4094), dict(capacity=2 ** 24), dict(discount=1.0), dict(K=1), dict(K=8)]
REFUSED_IDS = [f"{k}={v}" for kw in REFUSED for k, v in kw.items()]
ACCEPTED_IDS = ["minimum"] + [f"{k}={v}" for kw in ACCEPTED for k, v in kw.items()]


def create(lib, **kw):
    """(status, handle) of srlx_vppo_lanes_create, or _create_normal where K is given, on LOW with `kw` over it."""
    a = dict(LOW, **kw)
    h = ctypes.c_void_p()
    if a["K"] is None:
        return lib.srlx_vppo_lanes_create(ctypes.byref(h), a["E"], a["D"], a["steps"], a["capacity"], a["discount"], 0), h
    return lib.srlx_vppo_lanes_create_normal(ctypes.byref(h), a["E"], a["D"], a["steps"], a["capacity"], a["discount"], a["K"], 0), h


def assert_create_refuses(kw):
    """ERR_INVALID, no handle, and the entry point named in srlx_last_error(); action_dim is the Normal entry point's alone, every other argument is refused by both."""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    for a, name in [(kw, b"vppo_lanes_create_normal:")] if "K" in kw else [(kw, b"vppo_lanes_create:"), (dict(kw, K=3), b"vppo_lanes_create_normal:")]:
        st, h = create(lib, **a)
        err = lib.srlx_last_error()
        assert st == N.ERR_INVALID and not h.value and name in err and b"unavailable" not in err and b"failed" not in err, (st, err)
