"""The schedules of tests/test_vppo_lanes_envelope_gpu.py checked where there is no GPU: every case of tests/vppo_lanes_cases.py runs through the mirror alone
and must reach the edge it is there for -- conditions on the inputs, so that the GPU comparison cannot pass on a schedule that misses its subject."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_lanes_cases as C  # noqa: E402


def _walk(c):
    first, plan, mirror = C.inputs(c)
    seen = C.Seen(c.capacity)
    t0 = time.perf_counter()
    for t in range(c.T):
        seen.note(C.push(mirror, plan, t))
    return plan, mirror, seen, time.perf_counter() - t0


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_schedule_reaches_what_the_case_is_for(c):
    plan, mirror, seen, wall = _walk(c)
    R = c.steps + 2
    print(f"VPPO-LANES-ENV {c.name}: {mirror.ring.added} items through {c.T} lock-steps (R {R}), longest episode {seen.longest}, up to {seen.closes} closes in "
          f"one, largest S {seen.big_s} against capacity {c.capacity}, cut at j {seen.cut} of {seen.cut_of}, mirror {wall:.2f} s")
    assert mirror.error == 0, "the error word"
    # (the Pendulum shape is the engine's own: one episode per lane, 201 lock-steps in 203 rows)
    assert (c.T > R) == (c.name != "pendulum-E1024"), "the tracking ring does not wrap"
    assert seen.longest >= c.longest and seen.longest <= c.steps and seen.closes >= c.closes and seen.highest_lane >= c.lane
    assert (seen.big_s > c.capacity) == c.s_over
    assert seen.cut >= c.cut and (c.cut == 0 or seen.cut < seen.cut_of)
    assert (mirror.ring.added > c.capacity) == c.added_over
    assert plan["terminated"].any() and (plan["done"] & ~plan["terminated"] & 1).any(), "terminations and truncations among the closing steps"
    lp = np.stack([np.asarray(item[3], np.float32).reshape(-1) for item in mirror.ring.buffer])
    assert (lp == C.FLOOR).any() and (lp > C.FLOOR).any() and (lp >= C.FLOOR).all(), "stored log-probabilities on both sides of the floor"
    if c.reward_scale:
        r = np.abs(np.array([item[4] for item in mirror.ring.buffer], np.float64))
        assert (r > 1e3).any() and (r < 1e-3).any(), "rewards of mixed magnitude"


def test_the_cases_together_reach_every_edge():
    """Which case holds which edge (the issue's list), asserted on the table so that dropping a case fails here."""
    by = {c.name: c for c in C.CASES}
    assert by["stride-D5"].D % 4 and not by["stride-D4-K3"].D % 4 and by["stride-D4-K3"].K == 3  # both closes, past two strides
    assert all(by[n].longest > 2 * C.STRIDE for n in ("stride-D5", "stride-D4-K3"))
    assert {256, 257, 255, 1} <= set(by["stride-D5"].lengths)  # the stride's own length, one either side, and 1
    assert by["longest-cap4000"].longest == by["longest-cap8192-K8"].longest == 4094 == by["longest-cap4000"].steps  # R = 4096: the LDS arrays full
    assert by["longest-cap3700"].cut > C.STRIDE and by["longest-cap3700-K8"].cut > C.STRIDE  # keep_from inside a lane's second stride
    assert by["longest-cap3700-K8"].D % 4  # ... and in the scalar close's n * D loop
    assert (by["discount0"].discount, by["discount1"].discount, by["discount1-longest"].discount) == (0.0, 1.0, 1.0)
    assert all(by[n].closes > C.STRIDE and by[n].s_over and by[n].lane >= C.STRIDE for n in ("lanes-E257-D1", "lanes-E300-D1", "lanes-E257-D3-K8", "lanes-E300-D3-K8"))
    assert by["lanes-E4096-D4"].E == by["lanes-E4096-D4"].closes == 4096
    p = by["pendulum-E1024"]
    assert (p.E, p.D, p.K, p.lengths, p.capacity, p.T) == (1024, 3, 1, [200], 100_000, 201) and p.E * 200 > p.capacity


def test_lane_zero_idles_while_others_close():
    """Lane 0's workgroup carries the count over whether it closes or not: the stride cases close lane 1 alone, the many-lane cases close others without lane 0."""
    for name in ("stride-D5", "lanes-E257-D1", "lanes-E4096-D4"):
        c = next(x for x in C.CASES if x.name == name)
        assert _walk(c)[2].lane0_idle, name


@pytest.mark.parametrize("d", C.DRAWS, ids=C.DRAW_IDS)
def test_draw_cases_fill_their_rings(d):
    first, plan, mirror = C.inputs(d)
    for t in range(d.T):
        C.push(mirror, plan, t)
    n = mirror.ring.length()
    assert mirror.ring.added == d.E * d.T // 2 and d.B <= n <= d.capacity and d.B <= 256 and mirror.error == 0
    if d.name.startswith("B-equals"):
        assert d.B == n == d.capacity == mirror.ring.added == 256
    if d.name.startswith("added"):
        assert mirror.ring.added == 40 * d.capacity
    draws = [C.MC.draw(0xD0A, i, n, d.B) for i in range(3)]
    assert all(len(set(x)) == d.B and min(x) >= 0 and max(x) < n for x in draws) and (d.B == n or draws[0] != draws[1])


@pytest.mark.parametrize("kw", C.REFUSED, ids=C.REFUSED_IDS)
def test_create_refuses_before_any_device_call(kw):
    """The refusals of tests/test_vppo_lanes_envelope_gpu.py where there is no device: the message is the argument's, never the device's."""
    C.assert_create_refuses(kw)
