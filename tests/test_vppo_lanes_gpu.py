"""V-PPO's episode store on the GPU (csrc/srlx_vppo_lanes.hip, device/vppo_lanes.py): push, close and sample against the mirror of
tests/vppo_engine_reference.py, bit for bit, on scripted schedules.  Every comparison covers every slot the ring holds and every drawn item."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_engine_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

ITEM_VIEWS = ("item_s", "item_s2", "item_action", "item_logp", "item_reward", "item_not_terminated", "item_total")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _store(E, D, steps, capacity, B, discount=0.95, seed=9):
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    return VppoLanes(E, D, steps, capacity, B, 1, discount, seed=seed)


def _schedule(E, D, steps, T, k, lengths=None):
    """T lock-steps of hand-fed fields: episode lengths cycle through `lengths` per lane (1 and `steps` among them), log-probabilities on both sides of
    log(1e-6), rewards that are no round numbers, terminations on some of the closing steps."""
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
        logp = np.where(g.random(E) < 0.3, -14.0 - g.random(E), -3.0 * g.random(E)).astype(np.float32)
        logp[0] = np.float32(math.log(1e-6)) if t % 2 else np.nextafter(np.float32(math.log(1e-6)), np.float32(-20))
        plan.append(dict(actions=g.integers(0, 5, E).astype(np.int32), logp=logp, rewards=g.standard_normal(E).astype(np.float32), terminated=term, done=done,
                         next_obs=g.standard_normal((E, D)).astype(np.float32)))
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


@pytest.mark.parametrize("E,D,steps,capacity,T", [(1, 1, 4, 7, 40), (3, 4, 5, 7, 45), (5, 5, 6, 64, 80), (65, 256, 3, 64, 12), (3, 4, 5, 64, 45)],
                         ids=["E1-D1-cap7", "E3-D4-cap7", "E5-D5-cap64", "E65-D256-cap64", "E3-D4-cap64"])
def test_push_and_close_match_the_mirror(E, D, steps, capacity, T):
    """Episodes of length 1 and of max_episode_steps, several lanes closing in one lock-step (every lane starts the same cycle two lanes apart), wraps of both
    capacities, the floor on both sides; checked after every lock-step."""
    first, plan = _schedule(E, D, steps, T, 100 * E + D)
    store = _store(E, D, steps, capacity, 1)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.Lanes(E, capacity, 0.95, steps, first)
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
    row = store.view("obs").numpy()[T % store.R]
    assert np.array_equal(_bits(row), _bits(plan[-1]["next_obs"])), "the current row is the last next_obs, dense [E][D]"
    print(f"VPPO-LANES E{E} D{D} cap{capacity}: {mirror.ring.added} items through {T} lock-steps, up to {closes} closes in one, hbm {store.hbm_bytes()} bytes")


def test_one_lockstep_adds_more_than_the_capacity():
    """S > capacity from one lane (an episode of 9 into 7 slots) and from several lanes closing together (3 x 4 into 7): the ring holds the last 7 of the
    sequence, as the sequential ring would."""
    for E, steps, lengths in ((1, 9, [9]), (3, 4, [4])):
        first, plan = _schedule(E, 4, steps, 2 * steps + 3, 77 + E, lengths=lengths)
        store = _store(E, 4, steps, 7, 1)
        store.reset_all(torch.from_numpy(first).cuda())
        mirror = M.Lanes(E, 7, 0.95, steps, first)
        _run(store, mirror, plan)
        assert _compare_ring(store, mirror) == 7 and mirror.ring.added == 2 * E * steps


def test_over_long_episode_sets_the_sticky_error():
    first, plan = _schedule(1, 4, 3, 6, 5, lengths=[100])
    store = _store(1, 4, 3, 16, 1)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.Lanes(1, 16, 0.95, 3, first)
    _run(store, mirror, plan[:3])
    assert store.count() == (0, 0)
    _run(store, mirror, plan[3:4])
    assert store.count() == (0, 1) and mirror.error == 1
    _run(store, mirror, plan[4:])
    assert store.count()[1] == 1, "the error is sticky"
    # the rest of the dropped episode never closes (its returns would be cut short at the drop); the lane's next episode does
    assert int(store.view("length")[0]) == -1
    end = dict(plan[5], done=np.ones(1, np.uint8))
    _run(store, mirror, [end])
    assert store.count() == (0, 1) and mirror.ring.added == 0
    _run(store, mirror, [plan[4], end])  # the new first observation, then a one-step episode
    assert store.count() == (1, 1) and mirror.ring.added == 1
    assert float(store.view("item_total")[0]) == float(end["rewards"][0])
    with pytest.raises(RuntimeError, match="max_episode_steps"):
        store.check()
    store.reset_all(torch.from_numpy(first).cuda())
    assert store.count() == (0, 0)


@pytest.mark.parametrize("D,capacity,fill,B", [(4, 64, 40, 1), (4, 64, 64, 64), (5, 300, 300, 256), (1, 7, 7, 7), (256, 64, 33, 33), (4, 64, 200, 64)],
                         ids=["B1", "B64-full", "B256-D5", "B7-equals-length", "B33-equals-length-D256", "B64-wrapped"])
def test_sample_draws_the_mirrors_slots_and_gathers_their_items(D, capacity, fill, B):
    """One-step episodes on one lane fill the ring with `fill` items; three draws in a row (the draw index is the key) with guard rows behind every output."""
    first, plan = _schedule(1, D, 1, 2 * fill, 31 + B, lengths=[1])
    store = _store(1, D, 1, capacity, B + 1, seed=0xD0A)
    store.reset_all(torch.from_numpy(first).cuda())
    mirror = M.Lanes(1, capacity, 0.95, 1, first)
    _run(store, mirror, plan)
    n = _compare_ring(store, mirror)
    assert n == min(fill, capacity) and n >= B
    want_items = mirror.slots()
    bufs = (store.states, store.next_states, store.actions, store.old_logpi, store.rewards, store.not_terminated, store.total_rewards, store.slots)
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


def test_a_draw_larger_than_the_ring_sets_the_error():
    first, plan = _schedule(1, 4, 1, 6, 3, lengths=[1])
    store = _store(1, 4, 1, 16, 8)
    store.reset_all(torch.from_numpy(first).cuda())
    _run(store, M.Lanes(1, 16, 0.95, 1, first), plan)
    assert store.count() == (3, 0) and store.is_warmup_needed() is True, "the gate waits for a whole batch, whatever warmup_size says"
    store.sample(8)
    assert store.count() == (3, 2)
    with pytest.raises(RuntimeError, match="more items"):
        store.check()


def test_the_warmup_gate_stops_reading_once_open():
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    first, plan = _schedule(2, 4, 1, 8, 4, lengths=[1])
    store = VppoLanes(2, 4, 1, 16, 2, 4, 0.95)
    store.reset_all(torch.from_numpy(first).cuda())
    reads = []
    count = store.count
    store.count = lambda: reads.append(1) or count()
    mirror = M.Lanes(2, 16, 0.95, 1, first)
    _run(store, mirror, plan[:2])
    assert store.is_warmup_needed() and len(reads) == 1
    _run(store, mirror, plan[2:])
    assert not store.is_warmup_needed() and len(reads) == 2
    assert not store.is_warmup_needed() and len(reads) == 2
    assert store.obs_uint8 is False and store.F == 4 and store.E == 2 and store.needs_reset_ptr.value
