"""V-PPO's episode store and the lane Pendulum on the GPU over the envelope they admit (csrc/srlx_vppo_lanes.hip, device/vppo_lanes.py):
k_vppo_lanes_store, _close<VEC>, _pick, _gather<VEC> and k_pendulum_lanes where their strided loops take a second and a sixteenth trip, where the LDS arrays are
full, where more than 256 lanes close at once and where one lock-step adds more than the ring holds.  The cases and their schedules are
tests/vppo_lanes_cases.py's (tests/test_vppo_lanes_envelope_cpu.py asserts that each reaches its edge); the mirrors are tests/vppo_engine_reference.py: Lanes and
tests/vppo_normal_reference.py: NormalLanes, unmodified.  The store moves data and runs one float64 chain under -ffp-contract=off, so every comparison is bit
for bit: all seven item views over every slot the ring holds, `added`, the error word, needs_reset and the lanes' lengths, and zeros past the ring's length."""
import ctypes
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_lanes_cases as C  # noqa: E402
import vppo_normal_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
ITEM_VIEWS = ("item_s", "item_s2", "item_action", "item_logp", "item_reward", "item_not_terminated", "item_total")
FIELDS = ("actions", "logp", "rewards", "terminated", "done", "next_obs")
SEED = 0xD0A


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _store(E, D, K, steps, capacity, B, discount=0.95, seed=SEED):
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    return VppoLanes(E, D, steps, capacity, B, 1, discount, seed=seed, action_dim=K)


def _upload(plan):
    """Each field once, [T][E]...; a push takes slices."""
    return {k: torch.from_numpy(plan[k]).cuda() for k in FIELDS}


def _push(store, dev, t):
    store.push(*(dev[k][t] for k in FIELDS))


def _compare(store, mirror, done):
    added, err = store.count()
    assert (added, err) == (mirror.ring.added, mirror.error) and err == 0, (added, mirror.ring.added, err)
    n = mirror.ring.length()
    assert store.length() == n
    for name, w in zip(ITEM_VIEWS, mirror.slots()):
        got = store.view(name).numpy()
        assert np.array_equal(_bits(got[:n]), _bits(w.reshape(got[:n].shape))), name
        assert not _bits(got[n:]).any(), f"{name}: a store past the ring's length"
    assert np.array_equal(store.view("needs_reset").numpy(), np.array(mirror.needs_reset, np.uint8))
    # (a closed lane's length stays for the close to read until the lane's next lock-step: compared on the lanes that did not close)
    assert np.array_equal(store.view("length").numpy() * (1 - done), np.array([len(x) for x in mirror.track], np.int32) * (1 - done))


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_push_and_close_match_the_mirror(c):
    first, plan, mirror = C.inputs(c)
    t0 = time.perf_counter()
    store = _store(c.E, c.D, c.K, c.steps, c.capacity, 1, c.discount)
    store.reset_all(torch.from_numpy(first).cuda())
    dev = _upload(plan)
    seen, compares = C.Seen(c.capacity), 0
    for t in range(c.T):
        _push(store, dev, t)
        closing = C.push(mirror, plan, t)
        seen.note(closing)
        if (closing and c.every) or t == c.T - 1:
            _compare(store, mirror, plan["done"][t])
            compares += 1
    assert seen.longest >= c.longest and seen.closes >= c.closes and (seen.big_s > c.capacity) == c.s_over and seen.cut >= c.cut
    row = store.view("obs").numpy()[c.T % store.R]
    assert np.array_equal(_bits(row), _bits(plan["next_obs"][-1])), "the current row is the last next_obs, dense [E][D]"
    print(f"VPPO-LANES-ENV {c.name}: {mirror.ring.added} items added through {c.T} lock-steps, longest episode {seen.longest}, up to {seen.closes} closes in one, "
          f"largest S {seen.big_s} against capacity {c.capacity}, {compares} comparisons, {time.perf_counter() - t0:.2f} s")


# ---- sample -------------------------------------------------------------------------------------------------------------------------------------------------------
def _outputs(store, B, offset):
    """Buffers for one draw, each with `offset` guard elements in front and a guard row and a guard element behind: (whole buffers, the views the kernel gets)."""
    D, K = store.D, store.K
    widths = (D, D, K, K, 1, 1, 1, 1)
    dtypes = (torch.float32, torch.float32, store._action_dtype, torch.float32, torch.float32, torch.float32, torch.float32, torch.int64)
    whole = [torch.full((offset + B * w + w + 1,), 7, dtype=dt, device="cuda") for w, dt in zip(widths, dtypes)]
    return whole, [b[offset:offset + B * w] for b, w in zip(whole, widths)]


def _draw(store, B, offset):
    from simple_distributed_rl_amd import _native as N

    whole, views = _outputs(store, B, offset)
    assert all((v.data_ptr() - b.data_ptr()) == offset * v.element_size() and b.data_ptr() % 16 == 0 for b, v in zip(whole, views))
    N.check(store._sample(store._h, B, ctypes.c_uint64(SEED), *(N.tptr(v) for v in views), N.torch_stream_ptr()))
    torch.cuda.synchronize()
    for b, v in zip(whole, views):
        b = b.cpu().numpy()
        assert (b[:offset] == 7).all() and (b[offset + v.numel():] == 7).all(), "a store outside the B rows"
    return [v.cpu().numpy() for v in views]


def _fill(store, d):
    first, plan, mirror = C.inputs(d)
    store.reset_all(torch.from_numpy(first).cuda())
    dev = _upload(plan)
    for t in range(d.T):
        _push(store, dev, t)
        C.push(mirror, plan, t)
    _compare(store, mirror, plan["done"][-1])
    return mirror


@pytest.mark.parametrize("d", C.DRAWS, ids=C.DRAW_IDS)
def test_sample_at_its_edges(d):
    """Through the raw entry point, so that the outputs can stand one float off a 16-byte boundary (the scalar gather at D % 4 == 0, which VppoLanes' own aligned
    buffers never reach).  Three draws in a row; then reset_all and a refill, after which the draw index is 0 again."""
    t0 = time.perf_counter()
    store = _store(d.E, d.D, d.K, 1, d.capacity, 1)
    for again in range(2):
        mirror = _fill(store, d)
        n, want_items = mirror.ring.length(), mirror.slots()
        for draw in range(3 if not again else 1):
            out = _draw(store, d.B, d.offset)
            want = C.MC.draw(SEED, draw, n, d.B)
            assert out[7].tolist() == want and len(set(want)) == d.B
            for got, w in zip(out[:7], want_items):
                assert np.array_equal(_bits(got), _bits(w[want].reshape(got.shape)))
    assert store.count() == (mirror.ring.added, 0)
    print(f"VPPO-LANES-ENV sample {d.name}: B {d.B} of N {n} (added {mirror.ring.added}, capacity {d.capacity}), D {d.D} K {d.K} offset {d.offset}, "
          f"{time.perf_counter() - t0:.2f} s")


# ---- create and sample: refusals and acceptances --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", C.REFUSED, ids=C.REFUSED_IDS)
def test_create_refuses_what_lies_outside_the_envelope(kw):
    """Every other argument at its minimum, so the refusal is the named argument's.  (tests/test_vppo_lanes_envelope_cpu.py makes the same calls where there is no
    device at all: the sizes are checked before any device call.)"""
    C.assert_create_refuses(kw)


@pytest.mark.parametrize("kw", C.ACCEPTED, ids=C.ACCEPTED_IDS)
def test_create_accepts_each_upper_end_alone(kw):
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    st, h = C.create(lib, **kw)
    assert st == N.OK and h.value, lib.srlx_last_error()
    added, err = N.c_i64(-1), ctypes.c_int32(-1)
    assert lib.srlx_vppo_lanes_count(h, ctypes.byref(added), ctypes.byref(err), None) == N.OK and (added.value, err.value) == (0, 0)
    assert lib.srlx_vppo_lanes_destroy(h) == N.OK


def test_sample_refuses_a_batch_past_256_or_past_the_capacity():
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    z = torch.full((4096,), 7, dtype=torch.float32, device="cuda")
    p = N.tptr(z)
    for K, capacity, batch, name in ((0, 300, 257, b"vppo_lanes_sample:"), (0, 4, 5, b"vppo_lanes_sample:"), (3, 300, 257, b"vppo_lanes_sample_normal:"),
                                     (3, 4, 5, b"vppo_lanes_sample_normal:")):
        store = _store(1, 4, K, 1, capacity, 1)
        assert store._sample(store._h, batch, ctypes.c_uint64(0), p, p, p, p, p, p, p, p, None) == N.ERR_INVALID
        err = lib.srlx_last_error()
        assert err.startswith(name) and b"batch %d" % batch in err, err
        assert store.count() == (0, 0)
    torch.cuda.synchronize()
    assert bool((z == 7).all()), "a refused draw wrote"


# ---- srlx_pendulum_lane_step past one workgroup -------------------------------------------------------------------------------------------------------------------
P_SEED = 0xBEEF


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _env(E, max_steps):
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.mlpq import PendulumLaneVecEnv

    needs_reset = torch.zeros(E, dtype=torch.uint8, device="cuda")
    replay = SimpleNamespace(obs_uint8=False, F=3, E=E, seed=P_SEED, dev=torch.device("cuda:0"), needs_reset_ptr=N.tptr(needs_reset))
    return PendulumLaneVecEnv(replay, max_steps=max_steps), needs_reset


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("E,max_steps,T", C.PENDULUMS, ids=[f"E{e}" for e, _, _ in C.PENDULUMS])
def test_pendulum_lanes_past_one_workgroup(E, max_steps, T):
    """The bars of tests/test_pendulum_lanes_gpu.py: every step is fed the device's own previous state; the state within 1e-12 of the mirror's, observation and
    reward within one float32 ulp, the reset draws bit-equal."""
    t0 = time.perf_counter()
    env, needs_reset = _env(E, max_steps)
    first = _host(env.reset())
    want_state = np.array([M.pendulum_reset(P_SEED, e, 0) for e in range(E)])
    assert np.array_equal(_host(env.state), want_state), "the first states are not the documented keyed draws, bit for bit"
    assert int(_ulps(first, np.stack([M.pendulum_obs(*s) for s in want_state])).max()) <= 1
    assert (_host(env.episodes) == 1).all() and (_host(env.steps) == 0).all()
    g = np.random.default_rng(E + max_steps)
    worst_state, worst_obs, worst_reward, resets = 0.0, 0, 0, 0
    done_prev = np.zeros(E, np.uint8)
    for t in range(T):
        torques = g.uniform(-2.5, 2.5, E).astype(F32)  # (past the clip at 2 on some lanes)
        before, steps_before, episodes_before = _host(env.state), _host(env.steps), _host(env.episodes)
        needs_reset.copy_(torch.from_numpy(done_prev))
        obs, reward, term, done = (_host(x) for x in env.step(torch.from_numpy(torques).cuda()))
        state, steps_after, episodes_after = _host(env.state), _host(env.steps), _host(env.episodes)
        want, want_r = np.empty((E, 2)), np.zeros(E, F32)
        for e in range(E):
            if done_prev[e]:  # the lock-step only delivers the next episode's first observation
                want[e] = M.pendulum_reset(P_SEED, e, int(episodes_before[e]))
            else:
                th, thdot, r = M.pendulum_step(float(before[e, 0]), float(before[e, 1]), float(torques[e]))
                want[e], want_r[e] = (th, thdot), F32(r)
        rs = done_prev.astype(bool)
        assert np.array_equal(state[rs], want[rs]), "a reset draw is not the keyed one, bit for bit"
        assert not reward[rs].any() and not done[rs].any() and not term.any()
        assert np.array_equal(steps_after, np.where(rs, 0, steps_before + 1)) and np.array_equal(episodes_after, episodes_before + rs)
        assert np.array_equal(done[~rs], (steps_before[~rs] + 1 >= max_steps).astype(np.uint8))
        resets += int(rs.sum())
        if (~rs).any():
            worst_state = max(worst_state, float(np.abs(state[~rs] - want[~rs]).max()))
            worst_reward = max(worst_reward, int(_ulps(reward[~rs], want_r[~rs]).max()))
        worst_obs = max(worst_obs, int(_ulps(obs, np.stack([M.pendulum_obs(*s) for s in want])).max()))
        done_prev = done
    print(f"VPPO-LANES-ENV pendulum E{E} max_steps {max_steps}: {T} lock-steps, {resets} lane resets; state {worst_state:.3e} (bar 1e-12), obs {worst_obs} ulp, "
          f"reward {worst_reward} ulp (bars 1), {time.perf_counter() - t0:.2f} s")
    assert worst_state <= 1e-12 and worst_obs <= 1 and worst_reward <= 1
    assert resets == T // (max_steps + 1) * E, "every lane resets at each lock-step behind its max_steps-th step"


def test_pendulum_lanes_refuses_65537_lanes():
    from simple_distributed_rl_amd import _native as N

    env, needs_reset = _env(4, 3)
    env.reset()
    a = _host(env.state)
    lib = N.lib()
    t = torch.zeros(4, dtype=torch.float32, device="cuda")
    args = (N.tptr(env.state), N.tptr(env.steps), N.tptr(env.episodes), N.tptr(needs_reset), N.tptr(t), 3, P_SEED, N.tptr(env.next_obs), N.tptr(env.rewards),
            N.tptr(env.terminated), N.tptr(env.done), None)
    assert lib.srlx_pendulum_lane_step(65537, *args) == N.ERR_INVALID and lib.srlx_last_error().startswith(b"pendulum_lane_step")
    assert lib.srlx_pendulum_lane_step(0, *args) == N.ERR_INVALID
    assert np.array_equal(_host(env.state), a) and (_host(env.episodes) == 1).all()
