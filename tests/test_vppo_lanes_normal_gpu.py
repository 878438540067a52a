"""V-PPO's episode store with K float32 action elements per step on the GPU (csrc/srlx_vppo_lanes.hip, device/vppo_lanes.py): the scripted schedules
of tests/test_vppo_lanes_gpu.py at K 1, 3 and 8 against the mirror of tests/vppo_normal_reference.py, bit for bit after every lock-step, over every slot the ring
holds and every drawn item; and each kind of handle refusing the other kind's push and sample."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_normal_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

ITEM_VIEWS = ("item_s", "item_s2", "item_action", "item_logp", "item_reward", "item_not_terminated", "item_total")
FLOOR = np.float32(math.log(1e-6))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _store(E, D, K, steps, capacity, B, discount=0.95, seed=9):
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    return VppoLanes(E, D, steps, capacity, B, 1, discount, seed=seed, action_dim=K)


def _schedule(E, D, K, steps, T, k, lengths=None):
    """T lock-steps of hand-fed fields: episode lengths cycle through `lengths` per lane (1 and `steps` among them), log-probabilities on both sides of
    log(1e-6) on different elements of one row, rewards that are no round numbers, terminations on some of the closing steps."""
    g = np.random.default_rng(k)
    lengths = lengths or [1, steps, 2, 3]
    plan, left, first = [], [0] * E, [False] * E
    nxt = [e % len(lengths) for e in range(E)]
    for e in range(E):
        left[e] = lengths[nxt[e]]
    for t in range(T):
        done = np.zeros(E, np.uint8)
        for e in range(E):
            if first[e]:
                first[e] = False
                nxt[e] = (nxt[e] + 1) % len(lengths)
                left[e] = lengths[nxt[e]]
                continue
            left[e] -= 1
            if left[e] == 0:
                done[e], first[e] = 1, True
        term = (done & (g.random(E) < 0.5)).astype(np.uint8)
        logp = np.where(g.random((E, K)) < 0.3, -14.0 - g.random((E, K)), -3.0 * g.random((E, K))).astype(np.float32)
        # lane 0: the floor itself or the float just under it on element 0, and (K > 1) a value well above it on the last element of the same row
        logp[0, 0] = FLOOR if t % 2 else np.nextafter(FLOOR, np.float32(-20))
        if K > 1:
            logp[0, K - 1] = np.float32(-0.25)
            if E > 1:
                logp[E - 1, 0], logp[E - 1, 1] = np.float32(-2.0), np.float32(-17.5)
        plan.append(dict(actions=g.standard_normal((E, K)).astype(np.float32), logp=logp, rewards=g.standard_normal(E).astype(np.float32), terminated=term,
                         done=done, next_obs=g.standard_normal((E, D)).astype(np.float32)))
    return g.standard_normal((E, D)).astype(np.float32), plan


def _run(store, mirror, plan, counter=None):
    for p in plan:
        d = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
        store.push(d["actions"], d["logp"], d["rewards"], d["terminated"], d["done"], d["next_obs"], bump=counter)
        mirror.push(p["actions"], p["logp"], p["rewards"], p["terminated"], p["done"], p["next_obs"])


def _compare_ring(store, mirror):
    added, err = store.count()
    assert added == mirror.ring.added and err == mirror.error, (added, mirror.ring.added, err)
    n = mirror.ring.length()
    assert store.length() == n
    want = mirror.slots()
    for name, w in zip(ITEM_VIEWS, want):
        got = store.view(name).numpy()
        if n:
            assert np.array_equal(_bits(got[:n]), _bits(w.reshape(got[:n].shape))), name
        assert not got[n:].any(), f"{name}: a store past the ring's length"
    return n


@pytest.mark.parametrize("E,D,K,steps,capacity,T", [(1, 1, 1, 4, 7, 40), (3, 4, 3, 5, 7, 45), (5, 5, 8, 6, 64, 80), (65, 256, 3, 3, 64, 12), (3, 4, 8, 5, 64, 45),
                                                    (5, 5, 1, 6, 7, 50)],
                         ids=["E1-D1-K1-cap7", "E3-D4-K3-cap7", "E5-D5-K8-cap64", "E65-D256-K3-cap64", "E3-D4-K8-cap64", "E5-D5-K1-cap7"])
def test_push_and_close_match_the_mirror(E, D, K, steps, capacity, T):
    """Episodes of length 1 and of max_episode_steps, several lanes closing in one lock-step, wraps of both capacities, the floor on both sides on different
    elements of one row; checked after every lock-step."""
    first, plan = _schedule(E, D, K, steps, T, 100 * E + D + K)
    store = _store(E, D, K, steps, capacity, 1)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.NormalLanes(E, K, capacity, 0.95, steps, first)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    closes = 0
    for t, p in enumerate(plan):
        _run(store, mirror, [p], counter)
        closes = max(closes, int(p["done"].sum()))
        _compare_ring(store, mirror)
        assert np.array_equal(store.view("needs_reset").numpy(), np.array(mirror.needs_reset, np.uint8))
        assert np.array_equal(store.view("length").numpy() * (1 - p["done"]), np.array([len(x) for x in mirror.track], np.int32) * (1 - p["done"]))
    assert int(counter.item()) == T and mirror.ring.added > capacity and mirror.error == 0
    assert E == 1 or closes > 1, "no lock-step closed several lanes"
    lp = mirror.slots()[3]
    assert lp.shape[1] == K and bool((lp == FLOOR).any()) and bool((lp >= FLOOR).all())
    assert bool((lp > FLOOR).any()) or (E == 1 and K == 1), "(one lane of one element: every log-probability of the schedule stands at the floor's edge)"
    if K > 1:
        assert bool(((lp == FLOOR).any(axis=1) & (lp > FLOOR).any(axis=1)).any()), "no stored row floored on one element and not on another"
    row = store.view("obs").numpy()[T % store.R]
    assert np.array_equal(_bits(row), _bits(plan[-1]["next_obs"])), "the current row is the last next_obs, dense [E][D]"
    # the tracking ring's views are [R][E][K]: the last lock-step's actions stand in its row as they were pushed, its log-probabilities floored
    last = (T - 1) % store.R
    stored = ~np.array([bool(x) for x in _first_lanes(plan)])
    assert np.array_equal(_bits(store.view("action").numpy()[last][stored]), _bits(plan[-1]["actions"][stored]))
    assert np.array_equal(_bits(store.view("logp").numpy()[last][stored]), _bits(np.maximum(plan[-1]["logp"], FLOOR)[stored]))
    print(f"VPPO-LANES-NORMAL E{E} D{D} K{K} cap{capacity}: {mirror.ring.added} items through {T} lock-steps, up to {closes} closes in one, hbm {store.hbm_bytes()} bytes")


def _first_lanes(plan):
    """The lanes whose LAST lock-step of the plan only delivered a first observation: those whose step before it was done."""
    return plan[-2]["done"] if len(plan) > 1 else np.zeros_like(plan[-1]["done"])


def test_one_lockstep_adds_more_than_the_capacity():
    """S > capacity from one lane (an episode of 9 into 7 slots) and from several lanes closing together (3 x 4 into 7): the ring holds the last 7 of the
    sequence, as the sequential ring would."""
    for E, K, steps, lengths in ((1, 3, 9, [9]), (3, 8, 4, [4])):
        first, plan = _schedule(E, 4, K, steps, 2 * steps + 3, 77 + E, lengths=lengths)
        store = _store(E, 4, K, steps, 7, 1)
        store.reset_all(torch.from_numpy(first).cuda())
        mirror = M.NormalLanes(E, K, 7, 0.95, steps, first)
        _run(store, mirror, plan)
        assert _compare_ring(store, mirror) == 7 and mirror.ring.added == 2 * E * steps


def test_over_long_episode_sets_the_sticky_error():
    K = 3
    first, plan = _schedule(1, 4, K, 3, 6, 5, lengths=[100])
    store = _store(1, 4, K, 3, 16, 1)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.NormalLanes(1, K, 16, 0.95, 3, first)
    _run(store, mirror, plan[:3])
    assert store.count() == (0, 0)
    _run(store, mirror, plan[3:4])
    assert store.count() == (0, 1) and mirror.error == 1
    _run(store, mirror, plan[4:])
    assert store.count()[1] == 1, "the error is sticky"
    assert int(store.view("length")[0]) == -1
    end = dict(plan[5], done=np.ones(1, np.uint8))
    _run(store, mirror, [end])
    assert store.count() == (0, 1) and mirror.ring.added == 0
    _run(store, mirror, [plan[4], end])  # the new first observation, then a one-step episode
    assert store.count() == (1, 1) and mirror.ring.added == 1
    assert float(store.view("item_total")[0]) == float(end["rewards"][0])
    assert np.array_equal(_bits(store.view("item_action").numpy()[0]), _bits(end["actions"][0]))
    with pytest.raises(RuntimeError, match="max_episode_steps"):
        store.check()
    store.reset_all(torch.from_numpy(first).cuda())
    assert store.count() == (0, 0)


@pytest.mark.parametrize("D,K,capacity,fill,B", [(4, 3, 64, 40, 1), (4, 8, 64, 64, 64), (5, 3, 300, 300, 256), (1, 1, 7, 7, 7), (256, 8, 64, 33, 33), (4, 3, 64, 200, 64)],
                         ids=["B1-K3", "B64-full-K8", "B256-D5-K3", "B7-equals-length-K1", "B33-equals-length-D256-K8", "B64-wrapped-K3"])
def test_sample_draws_the_mirrors_slots_and_gathers_their_items(D, K, capacity, fill, B):
    """One-step episodes on one lane fill the ring with `fill` items; three draws in a row (the draw index is the key) with guard rows behind every output."""
    first, plan = _schedule(1, D, K, 1, 2 * fill, 31 + B, lengths=[1])
    store = _store(1, D, K, 1, capacity, B + 1, seed=0xD0A)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.NormalLanes(1, K, capacity, 0.95, 1, first)
    _run(store, mirror, plan)
    n = _compare_ring(store, mirror)
    assert n == min(fill, capacity) and n >= B
    want_items = mirror.slots()
    bufs = (store.states, store.next_states, store.actions, store.old_logpi, store.rewards, store.not_terminated, store.total_rewards, store.slots)
    assert store.actions.dtype == torch.float32 and tuple(store.actions.shape) == (B + 1, K) and tuple(store.old_logpi.shape) == (B + 1, K)
    for draw in range(3):
        for t in bufs:
            t.fill_(7)
        out = store.sample(B)
        torch.cuda.synchronize()
        slots = out[7].cpu().numpy()
        want = M.draw(0xD0A, draw, n, B)
        assert slots.tolist() == want and len(set(want)) == B
        for got, w in zip(out[:7], want_items):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(w[want].reshape(got.shape)))
        for t in bufs:
            assert bool((t[B:] == 7).all()), "a store past B"
    assert store.count()[1] == 0


def test_each_kind_of_handle_refuses_the_other_kinds_push_and_sample():
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    lib = N.lib()
    normal, cat = _store(2, 4, 3, 2, 16, 2), VppoLanes(2, 4, 2, 16, 2, 1, 0.95)
    assert normal.K == 3 and normal.action_dim == 3 and cat.K == 1 and cat.action_dim == 0 and cat.actions.dtype == torch.int32
    z = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = N.tptr(z)
    for fn, h, name, word in ((lib.srlx_vppo_lanes_push, normal, b"vppo_lanes_push:", b"srlx_vppo_lanes_push_normal"),
                              (lib.srlx_vppo_lanes_push_normal, cat, b"vppo_lanes_push_normal:", b"srlx_vppo_lanes_push)")):
        assert fn(h._h, p, p, p, p, p, p, None, None) == N.ERR_INVALID
        assert name in lib.srlx_last_error() and word in lib.srlx_last_error(), lib.srlx_last_error()
    for fn, h, name, word in ((lib.srlx_vppo_lanes_sample, normal, b"vppo_lanes_sample:", b"srlx_vppo_lanes_sample_normal"),
                              (lib.srlx_vppo_lanes_sample_normal, cat, b"vppo_lanes_sample_normal:", b"srlx_vppo_lanes_sample)")):
        assert fn(h._h, 1, 0, p, p, p, p, p, p, p, p, None) == N.ERR_INVALID
        assert name in lib.srlx_last_error() and word in lib.srlx_last_error(), lib.srlx_last_error()
    for h in (normal, cat):
        assert h.count() == (0, 0) and h.lock_steps == 0, "a refused call moved the store"
    assert lib.srlx_vppo_lanes_sample_normal(normal._h, 0, 0, p, p, p, p, p, p, p, p, None) == N.ERR_INVALID and b"batch 0" in lib.srlx_last_error()
    assert lib.srlx_vppo_lanes_push_normal(normal._h, None, p, p, p, p, p, None, None) == N.ERR_INVALID and b"NULL argument" in lib.srlx_last_error()
