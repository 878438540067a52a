"""srlx_episode_account (csrc/srlx_episode.hip) over the envelope it admits.  The kernel is ONE workgroup of 1024 threads (16 waves) that walks the E
lanes in chunks of 1024, so E sits on and either side of a wave (64) and of a chunk (1024), and at 2049 = two chunks and one lane.  The model is the
host loop of tests/test_runner_vector_gpu.py: test_episode_ledger_matches_a_host_model -- a float32 running return per lane, finished episodes appended
in lane order, episode number k in ring slot k % ring_cap.  After EVERY launch: ep_return (bit patterns) and ep_len of every lane, the whole ring with a
sentinel pair behind it, and the four totals.  Rewards are multiples of 1/64, for which every float32 return and the float64 return_sum are exact in any
order of summation; then one pass of random float32 rewards, where return_sum is held to the bound of a float64 sum of n terms in any order.

Ring overflow: more episodes ending in one launch than the ring holds leaves the newest ring_cap of them, in lane order, and the same bytes on a second run
(before this test several threads wrote one slot in no defined order)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from simple_distributed_rl_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = (F32(-1234.5), F32(4321.0))
UNWRITTEN = F32(-77.0)


class Ledger:
    """The device state of one ledger, the ring one pair longer than ring_cap, beside its host model."""

    def __init__(self, E, cap, episodes0=0, steps0=0, return0=0.0, length0=0):
        self.E, self.cap, self.lib = E, cap, N.lib()
        self.ep_return = torch.zeros(E, dtype=torch.float32, device="cuda")
        self.ep_len = torch.zeros(E, dtype=torch.int32, device="cuda")
        ring = np.full((cap + 1, 2), UNWRITTEN, F32)
        ring[cap] = SENTINEL
        self.ring = torch.from_numpy(ring).cuda()
        totals = np.array([episodes0, steps0, 0, length0], np.int64)
        totals[2:3].view(np.float64)[0] = return0
        self.totals = torch.from_numpy(totals).cuda()
        # the model
        self.m_return, self.m_len, self.m_ring = np.zeros(E, F32), np.zeros(E, np.int32), ring.copy()
        self.m_episodes, self.m_steps, self.m_length = episodes0, steps0, length0
        self.m_terms = [float(return0)]  # what return_sum sums
        self.book = []

    def launch(self, rewards, done, skip):
        r, d = torch.from_numpy(rewards).cuda(), torch.from_numpy(done).cuda()
        s = None if skip is None else torch.from_numpy(skip).cuda()
        N.check(self.lib.srlx_episode_account(self.E, N.tptr(r), N.tptr(d), N.tptr(s), N.tptr(self.ep_return), N.tptr(self.ep_len), N.tptr(self.ring), self.cap,
                                              N.tptr(self.totals), None))
        torch.cuda.synchronize()

    def model(self, rewards, done, skip):
        """env_run.py:334-352 + core_play.py:200-214 for E lanes; returns how many episodes ended."""
        ended = 0
        for e in range(self.E):
            if skip is not None and skip[e]:
                continue
            self.m_steps += 1
            self.m_return[e] = F32(self.m_return[e] + rewards[e])
            self.m_len[e] += 1
            if done[e]:
                rec = (self.m_return[e], F32(self.m_len[e]))
                self.m_ring[self.m_episodes % self.cap] = rec  # one after the other: the newest of a slot survives
                self.book.append(rec)
                self.m_terms.append(float(rec[0]))
                self.m_length += int(self.m_len[e])
                self.m_episodes += 1
                self.m_return[e], self.m_len[e] = 0, 0
                ended += 1
        return ended

    def step(self, rewards, done, skip=None):
        self.launch(rewards, done, skip)
        return self.model(rewards, done, skip)

    def read_totals(self):
        t = self.totals.cpu().numpy()
        return int(t[0]), int(t[1]), float(t[2:3].view(np.float64)[0]), int(t[3])

    def compare(self, exact_sum=True, what=""):
        assert np.array_equal(self.ep_return.cpu().numpy().view(np.int32), self.m_return.view(np.int32)), f"{what}: running returns"
        assert np.array_equal(self.ep_len.cpu().numpy(), self.m_len), f"{what}: running lengths"
        ring = self.ring.cpu().numpy()
        assert tuple(ring[self.cap]) == SENTINEL, f"{what}: a store past the ring"
        assert np.array_equal(ring.view(np.int32), self.m_ring.view(np.int32)), f"{what}: ring records"
        episodes, steps, rsum, lsum = self.read_totals()
        assert (episodes, steps, lsum) == (self.m_episodes, self.m_steps, self.m_length), what
        want = math.fsum(self.m_terms)
        if exact_sum:
            assert rsum == want, f"{what}: return_sum {rsum!r} for {want!r}"
        else:
            # a float64 sum of n terms in ANY order is within (n - 1) * 2^-53 * sum|x| of the true sum to first order; n * 2^-52 * sum|x| bounds it with all
            # higher-order terms for every n here (derived, not measured)
            n = len(self.m_terms)
            bound = n * 2.0 ** -52 * math.fsum(abs(x) for x in self.m_terms)
            print(f"EPISODE-ENV {what}: return_sum off by {abs(rsum - want):.3e}, bound {bound:.3e} over {n} terms")
            assert abs(rsum - want) <= bound, (rsum, want, bound)


def _sixty_fourths(rng, E):
    return (rng.integers(-128, 129, E) / 64).astype(F32)


def _mask(rng, E, p):
    return (rng.random(E) < p).astype(np.uint8)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_lock_steps_match_the_host_model(E):
    cap = E + 3  # no launch ends more than the ring holds; the run wraps the ring several times
    rng = np.random.default_rng(E)
    # totals continue from a ledger in mid-run: an episode count that is no multiple of the ring's capacity
    led = Ledger(E, cap, episodes0=3 * cap + 5, steps0=1000, return0=2.5, length0=77)
    none, every = np.zeros(E, np.uint8), np.ones(E, np.uint8)
    last = none.copy()
    last[E - 1] = 1  # the last lane of the last chunk
    skip_not_last = _mask(rng, E, 0.3)
    skip_not_last[E - 1] = 0
    skip_last = _mask(rng, E, 0.3)
    skip_last[E - 1] = 1
    plan = [("no lane done", none, None), ("some done, some skipped", _mask(rng, E, 0.3), _mask(rng, E, 0.2)), ("every lane done", every, None),
            ("the last lane done", last, None), ("every lane done, some skipped", every, skip_last), ("no lane done, some skipped", none, _mask(rng, E, 0.5)),
            ("some done", _mask(rng, E, 0.5), None), ("every lane done again", every, None), ("the last lane done, others skipped", last, skip_not_last),
            ("every lane skipped", every, every)]
    ended = []
    for name, done, skip in plan:
        ended.append(led.step(_sixty_fourths(rng, E), done, skip))
        led.compare(True, f"E {E}, {name}")
    assert ended[0] == 0 and ended[2] == E and ended[3] == 1 and ended[4] == E - int(skip_last.sum()) and ended[5] == 0 and ended[7] == E and ended[8] == 1
    assert ended[9] == 0 and led.m_episodes - (3 * cap + 5) > (2 * cap if E > 1 else 3), "the ring wrapped"
    # one pass with random float32 rewards: the running returns are single float32 adds (exact against the model); return_sum within the derived bound
    led.step((rng.standard_normal(E) * 100).astype(F32), none, None)
    led.compare(False, f"E {E}, random rewards, no lane done")
    led.step((rng.standard_normal(E) * 100).astype(F32), _mask(rng, E, 0.5), _mask(rng, E, 0.1))
    led.compare(False, f"E {E}, random rewards, some done")
    led.step(rng.standard_normal(E).astype(F32), every, None)
    led.compare(False, f"E {E}, random rewards, every lane done")


def _overflow_run(E, cap, with_skip):
    rng = np.random.default_rng(E + cap)
    led = Ledger(E, cap, episodes0=7)
    none, every = np.zeros(E, np.uint8), np.ones(E, np.uint8)
    lanes = (np.arange(E) / 64).astype(F32)  # a different return in every lane
    led.step(lanes, none, None)
    led.compare(True, "warm-up")
    skip = None
    if with_skip:
        skip = _mask(rng, E, 0.1)
        skip[[0, E - 1]] = (1, 0)
    ended = led.step(lanes, every, skip)
    assert ended > cap and (ended == E) == (not with_skip)
    led.compare(True, f"E {E}, cap {cap}: {ended} episodes end in one launch")
    # the newest `cap` episodes of the launch, in lane order, in the slots their episode numbers name
    newest = led.book[-cap:]
    ring = led.ring.cpu().numpy()
    for k, rec in zip(range(led.m_episodes - cap, led.m_episodes), newest):
        assert tuple(ring[k % cap]) == rec
    assert [float(r[0]) for r in newest] == sorted(float(r[0]) for r in newest), "lane order"
    # E > cap with FEWER than cap episodes ending: nothing is held back, the count goes on from where the overflow left it
    few = none.copy()
    few[[0, E // 2, E - 1]] = 1
    assert led.step(_sixty_fourths(rng, E), few, None) == 3
    led.compare(True, "three episodes after the overflow")
    ended = led.step(_sixty_fourths(rng, E), every, None)
    assert ended == E
    led.compare(True, "a second overflow")
    return led.ring.cpu().numpy().tobytes(), led.read_totals()


@pytest.mark.parametrize("with_skip", [False, True], ids=["all-lanes", "some-skipped"])
@pytest.mark.parametrize("E,cap", [(130, 64), (2049, 1000)])
def test_ring_overflow_keeps_the_newest_and_is_reproducible(E, cap, with_skip):
    first = _overflow_run(E, cap, with_skip)
    second = _overflow_run(E, cap, with_skip)
    assert first[0] == second[0], "equal ring bytes on two runs"
    assert first[1] == second[1]


def test_refusals_write_nothing():
    E, cap = 65, 8
    led = Ledger(E, cap, episodes0=5, steps0=9, return0=1.25, length0=3)
    r = torch.ones(E, dtype=torch.float32, device="cuda")
    d = torch.ones(E, dtype=torch.uint8, device="cuda")
    good = [E, N.tptr(r), N.tptr(d), None, N.tptr(led.ep_return), N.tptr(led.ep_len), N.tptr(led.ring), cap, N.tptr(led.totals), None]
    bad = {"n_envs 0": (0, 0), "n_envs negative": (0, -1), "ring_cap 0": (7, 0), "ring_cap negative": (7, -1), "rewards NULL": (1, None), "done NULL": (2, None),
           "ep_return NULL": (4, None), "ep_len NULL": (5, None), "ring NULL": (6, None), "totals NULL": (8, None)}
    for name, (k, value) in bad.items():
        args = list(good)
        args[k] = value
        assert led.lib.srlx_episode_account(*args) != N.OK, name
    with pytest.raises(N.SrlxError):
        args = list(good)
        args[7] = 0
        N.check(led.lib.srlx_episode_account(*args))
    torch.cuda.synchronize()
    led.compare(True, "after the refusals")
    N.check(led.lib.srlx_episode_account(*good))  # and the same arguments, whole, are taken
    torch.cuda.synchronize()
    led.model(np.ones(E, F32), np.ones(E, np.uint8), None)
    led.compare(True, "the accepted call")
