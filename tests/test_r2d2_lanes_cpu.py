"""R2D2's lane sequence ring and the engine's route, the parts that need no GPU: the host model of the window rules against what the plugin's own
`r2d2.Worker` adds to its memory, the numpy mirror of `srlx_r2d2_policy` against `rl.functions`, `LaneLedger` with a flush-window count (serial order, `_lo`, the
ring-length derivation by brute force and by a constructed stream), every reason of `why_not_r2d2_engine`, and the argument checks of the three entry points."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


# ---- the host model against the Worker ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("burnin,S", [(0, 1), (0, 3), (2, 1), (2, 3)])
def test_host_model_equals_what_the_worker_adds(burnin, S):
    """The plugin's Worker plays seeded episodes on CPU parameters (a terminated one, truncated ones, one of a single step); its recorded per-step values go
    through the host model as lock-steps of one lane, and every window must equal the item the Worker added, field by field and exactly."""
    import simple_distributed_rl_amd as srl
    from r2d2_lanes_reference import R2D2LanesModel, register_corridor
    from r2d2_reference import worker_case
    from simple_distributed_rl_amd.algorithms import r2d2

    register_corridor()
    A, H = 4, 16
    c = r2d2.Config(batch_size=4, burnin=burnin, sequence_length=S, lstm_units=H, epsilon=0.5)
    c.hidden_block.set_dueling_network((32,))
    c.memory.capacity, c.memory.warmup_size = 256, 4
    env = srl.EnvConfig("R2D2Corridor-v0", kwargs=dict(n_actions=A, starts=(1, 3, 0, 4, 2), budgets=(9, 1, 4, 9, 2)))
    records, adds, _ = worker_case(c, env, seed=3, episodes=10)
    L = burnin + S + 1
    lengths = [len(r.a) for r in records]
    assert all(r.done for r in records) and 1 in lengths and max(lengths) >= 4
    assert any(r.terminated[-1] for r in records) and any(not r.terminated[-1] for r in records)  # a terminated end and a truncated one
    assert any(len(lst) for r in records for lst in r.invalid)  # the state-dependent invalid action was met

    def mask(lst):
        m = np.zeros(A, np.uint8)
        m[list(lst)] = 1
        return m

    model, windows = R2D2LanesModel(1, L, S, A, H, (3,), seed=9), []
    z = np.zeros(1, np.float32)
    for r in records:
        assert model.push([r.s[0]], [0], z, z, [0], np.zeros((1, 2, H), np.float32), first=[True], done=[False], invalid=[mask(r.invalid[0])]) == []
        for i in range(len(r.a)):
            windows += model.push([r.s[i + 1]], [r.a[i]], [r.prob[i]], [r.reward[i]], [r.terminated[i]], np.asarray(r.hidden[i + 1], np.float32)[None], first=[False],
                                  done=[i == len(r.a) - 1], invalid=[mask(r.invalid[i + 1])])
    assert len(windows) == len(adds) == sum(n + S - 1 for n in lengths)
    real = pads = 0
    for j, (w, (item, priority)) in enumerate(zip(windows, adds)):
        assert priority is None
        np.testing.assert_array_equal(w["states"], np.asarray(item["states"], np.float32), err_msg=f"states {j}")
        np.testing.assert_array_equal(w["probs"], np.asarray(item["probs"], np.float32), err_msg=f"probs {j}")
        np.testing.assert_array_equal(w["rewards"], np.asarray(item["rewards"], np.float32), err_msg=f"rewards {j}")
        np.testing.assert_array_equal(w["dones"], np.asarray(item["dones"], np.uint8), err_msg=f"dones {j}")
        np.testing.assert_array_equal(w["invalid"], np.array([mask(lst) for lst in item["invalid_actions"]]), err_msg=f"invalid {j}")
        np.testing.assert_array_equal(w["hidden"], np.asarray(item["hidden_states"], np.float32), err_msg=f"hidden {j}")
        keep = ~w["is_pad"]
        np.testing.assert_array_equal(w["actions"][keep], np.asarray(item["actions"])[keep], err_msg=f"actions {j}")
        np.testing.assert_array_equal(w["probs"][w["is_pad"]], np.full(int(w["is_pad"].sum()), np.float32(1.0 / A)))
        real, pads = real + int(keep.sum()), pads + int(w["is_pad"].sum())
        k = w["desc"][2]
        if k:
            np.testing.assert_array_equal(w["dones"][S - k:], 1)  # the dones of flush pads
    assert real > 0 and (pads > 0 or S == 1)  # (at S = 1 the one transition of a window is always a real one)


# ---- the policy mirror ----------------------------------------------------------------------------------------------------------------------------------------------
def _policy_rows(rng, n, A):
    for i in range(n):
        q = rng.integers(-2, 3, A).astype(np.float32) if i % 2 else rng.standard_normal(A).astype(np.float32)  # (small integers: ties)
        invalid = (rng.random(A) < 0.35).astype(np.uint8) if i % 3 else np.zeros(A, np.uint8)
        if invalid.all():
            invalid[rng.integers(A)] = 0
        yield q, invalid


@pytest.mark.parametrize("A", [1, 2, 3, 7])
def test_policy_mirror_equals_the_functions_it_restates(A, monkeypatch):
    from r2d2_lanes_reference import policy_probs, policy_row
    from simple_distributed_rl_amd.rl import functions as funcs

    rng = np.random.default_rng(40 + A)
    checked_masked = checked_tied = 0
    for q, invalid in _policy_rows(rng, 120, A):
        lst = np.nonzero(invalid)[0].tolist()
        for eps32 in (np.float32(0.0), np.float32(0.1), np.float32(1.0)):
            eps = float(eps32)  # (the kernel reads epsilon as float32: the functions get that value)
            want = funcs.calc_epsilon_greedy_probs(q, lst, eps, A)
            assert policy_probs(q, eps32, invalid) == want
            for u in (float(rng.random()), 1.0 - 2.0**-53, 2.0**-60):  # u > 0
                monkeypatch.setattr(random, "random", lambda u=u: u)
                a_want = funcs.random_choice_by_probs(want)
                a, mu, bounds = policy_row(q, eps32, u, invalid)
                if want[a_want] > 0:  # (at a tiny u the reference can return a zero-weight action 0; the mirror skips invalid ones)
                    assert a == a_want and mu == np.float32(want[a]), (q, lst, eps, u)
                assert not invalid[a]
        checked_masked += bool(lst)
        checked_tied += int((q[invalid == 0] == q[invalid == 0].max()).sum() > 1)
    assert (checked_masked > 10 and checked_tied > 3) or A == 1  # (the comparison met masks and ties)


def test_policy_mirror_departures():
    from r2d2_lanes_reference import policy_row

    q = np.array([3.0, 1.0, 2.0], np.float32)
    assert policy_row(q, 0.1, 0.0, np.array([1, 0, 0], np.uint8))[0] == 1  # u = 0: the first VALID action, never the invalid action 0
    a, mu, bounds = policy_row(q, 0.1, 0.5, np.array([1, 1, 1], np.uint8))
    assert (a, mu, bounds) == (0, np.float32(1.0), [])  # no valid action
    a, mu, _ = policy_row(q, 0.0, 0.999, np.array([1, 0, 0], np.uint8))
    assert a == 2 and mu == np.float32(1.0)  # the unmasked maximum is invalid: greedy over the rest


# ---- LaneLedger with a flush count ----------------------------------------------------------------------------------------------------------------------------------
def _episode_masks(lengths_per_lane):
    """(first, done) masks per lock-step for lanes that play the given episode lengths back to back, until the first lane runs out."""
    E = len(lengths_per_lane)
    cursor, remaining = [0] * E, [0] * E
    first = np.ones(E, bool)
    while True:
        done = np.zeros(E, bool)
        for e in range(E):
            if first[e]:
                if cursor[e] >= len(lengths_per_lane[e]):
                    return
                remaining[e] = lengths_per_lane[e][cursor[e]]
                cursor[e] += 1
            else:
                remaining[e] -= 1
                done[e] = remaining[e] == 0
        yield first.copy(), done
        first = done


@pytest.mark.parametrize("S", [1, 3])
def test_ledger_flush_count_serial_order_and_lo(S):
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger

    E, L = 3, S + 3
    led = LaneLedger(E, 64, L, flush=S - 1)
    assert led.flush == S - 1
    want_next, age = 0, np.zeros(E, int)
    for t, (first, done) in enumerate(_episode_masks([[1, 3, 2, 5, 1, 1, 7], [2, 2, 2, 2, 2, 2, 2], [6, 1, 1, 4, 9]])):
        assert led.push(first) == t
        age = np.where(first, 0, age + 1)
        serials = led.emit(done)
        counts = [0 if first[e] else 1 + (S - 1) * int(done[e]) for e in range(E)]
        np.testing.assert_array_equal(led.window_counts(first, done), counts)
        assert serials.tolist() == list(range(want_next, want_next + sum(counts)))
        want_next += sum(counts)
        want = [(e, t, k) for e in range(E) for k in range(counts[e])]  # lane-major; the step's window, then its S - 1 flush windows
        assert [tuple(r) for r in led.descriptors(serials).tolist()] == want
        np.testing.assert_array_equal(led._lo[serials % 64], [t - min(L - 1 - k, age[e]) for e, _, k in want])
    assert led.serial == want_next


def test_ledger_default_flush_is_the_window_and_its_defaults_keep_their_bits():
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, LaneSequenceStore, R2D2LaneStore

    for E, C, L in [(1, 12, 2), (3, 40, 6), (16, 100_000, 11), (64, 1_000_000, 121)]:
        c = -(-C // E)
        led = LaneLedger(E, C, L)
        assert led.flush == L - 1 and led.ring_len == c + 2 * L == LaneLedger.default_ring_len(E, C, L)
        assert LaneLedger.min_ring_len(E, C, L) == (C - 2) // E + L + 2 == LaneLedger.min_ring_len(E, C, L, flush=1) <= c + L + 1
        assert LaneLedger.min_ring_len(E, C, L, flush=0) == 2 * c + L and LaneLedger.default_ring_len(E, C, L, flush=0) == 2 * c + 2 * L - 1
        np.testing.assert_array_equal(led.window_counts([False, False, True], [True, False, False]), [L, 1, 0])
    with pytest.raises(ValueError):
        LaneLedger(4, 4 * 6 - 1, 6)  # the default count: one lock-step's windows are E L
    assert LaneLedger(4, 4 * 3, 6, flush=2).seq_capacity == 12  # E (1 + flush)
    with pytest.raises(ValueError):
        LaneLedger(4, 4 * 3 - 1, 6, flush=2)
    with pytest.raises(ValueError, match="flush"):
        LaneLedger(4, 100, 6, flush=6)
    # ring_bytes: host arithmetic over the default ring
    assert LaneSequenceStore.ring_bytes(3, 40, 6, 4, 16, 5) == (14 + 12) * 3 * (4 * 8 + 32 + 4 + 16 * 16)
    assert R2D2LaneStore.ring_bytes(3, 40, 6, 3, 4, 16, 5) == (14 + 12) * 3 * (4 * 8 + 32 + 4 + 8 * 16)
    assert R2D2LaneStore.ring_bytes(3, 40, 4, 1, 4, 16, 5) == (2 * 14 + 2 * 4 - 1) * 3 * (4 * 8 + 32 + 4 + 8 * 16)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("E,C,burnin", [(1, 12, 0), (3, 40, 2), (4, 24, 2), (7, 100, 1)])
def test_ring_at_the_derived_length_never_refuses_random_episode_streams(E, C, burnin, S):
    """Seeded random episode lengths from 1 up (episodes of one step often, and in runs), at the default ring length and at the derivation's minimum; every live
    window's oldest referenced position is checked against what the ring still holds, by brute force."""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger

    L = burnin + S + 1
    for ring_len in (None, LaneLedger.min_ring_len(E, C, L, S - 1)):
        rng = np.random.default_rng(E * 1000 + C + S)
        lengths = [rng.choice([1, 1, 1, 1, 2, 3, L - 1, L, L + 1, 3 * L], 600).tolist() for _ in range(E)]
        for e in range(E):  # runs of one-step episodes behind a long one: the slowest emission behind the farthest reference
            for at in range(5, 600, 60):
                lengths[e][at : at + 1 + 2 * C // E + 4] = [3 * L] + [1] * (2 * C // E + 4)
        led = LaneLedger(E, C, L, ring_len, flush=S - 1)
        live, age = [], np.zeros(E, int)
        for t, (first, done) in enumerate(_episode_masks(lengths)):
            led.push(first)  # never refuses
            assert all(lo > t - led.ring_len for lo in live), t  # what this push overwrote was referenced by no live window
            age = np.where(first, 0, age + 1)
            desc = led.descriptors(led.emit(done))
            live += [t_ - min(L - 1 - k, age[e]) for e, t_, k in desc.tolist()]
            live = live[-C:]
        assert t > 3 * led.ring_len


@pytest.mark.parametrize("E,C", [(2, 8), (3, 10), (1, 6)])
@pytest.mark.parametrize("S", [1, 3])
def test_ledger_refuses_at_one_row_less_than_the_derived_minimum(S, E, C):
    """Constructed streams that reach the bound (the class docstring's).  S > 1 (a flush count >= 1): the last lane plays one long episode, the others end an
    episode of L + 2 steps together and then play long ones; the windows behind the last lane's window of that lock-step are as few as a stream can make them.
    S = 1 (no flush windows): every lane ends an episode of L + 2 steps at the same lock-step and then plays episodes of one step, one window per lane per TWO
    lock-steps.  (3, 10): E divides C - 1, where the bound for S > 1 is one row below ceil(C / E) + L + 1.)"""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, LedgerError

    L, c = S + 3, -(-C // E)
    T_min = LaneLedger.min_ring_len(E, C, L, S - 1)
    assert T_min == ((C - 2) // E + L + 2 if S > 1 else 2 * c + L)
    if (E, C) == (2, 8):
        assert T_min == (4 + L + 1 if S > 1 else 2 * 4 + L)
    lengths = [[L + 2, 400]] * (E - 1) + [[400]] if S > 1 else [[L + 2] + [1] * 200] * E

    def run(T):
        led = LaneLedger(E, C, L, ring_len=T, flush=S - 1)
        for first, done in _episode_masks(lengths):
            before = (led.t, led.serial, led.age.copy(), led._t.copy(), led._lo.copy())
            try:
                led.push(first)
            except LedgerError as e:
                assert "would overwrite position" in str(e) and f"{LaneLedger.default_ring_len(E, C, L, S - 1)} rows never refuse" in str(e)
                assert all(np.array_equal(a, b) for a, b in zip(before, (led.t, led.serial, led.age, led._t, led._lo)))  # refused before anything changed
                return led.t
            led.emit(done)
        return None

    assert run(T_min) is None
    assert run(T_min - 1) is not None


# ---- reasons ---------------------------------------------------------------------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, n=4, discrete=True, players=1):
        from simple_distributed_rl_amd.base.spaces.box import BoxSpace
        from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

        self.action_space = DiscreteSpace(n) if discrete else BoxSpace((1,), -1, 1)
        self.player_num = players


def _config(**kw):
    from simple_distributed_rl_amd.algorithms import r2d2

    c = r2d2.Config(batch_size=4, lstm_units=16, burnin=2, sequence_length=3, **kw)
    c.window_length = 1
    return c


def test_every_reason_of_why_not_r2d2_engine():
    from simple_distributed_rl_amd.algorithms import dqn
    from simple_distributed_rl_amd.device import vector_runner as vr

    c = _config()
    assert vr.engine_kind(c) is None  # (the route is a question of its own: nothing else learns of it)
    assert vr.why_not_r2d2_engine(_Env(), c) == "the run is not on a GPU device"
    c._set_device("cuda:0")
    assert vr.why_not_r2d2_engine(_Env(), c) == ""
    assert "discrete action spaces" in vr.why_not_r2d2_engine(_Env(discrete=False), c)
    assert "multi-player" in vr.why_not_r2d2_engine(_Env(players=2), c)
    assert "outside the lane gather's 1..64" in vr.why_not_r2d2_engine(_Env(n=65), c)
    for change, reason in ((lambda c: c.memory.set_rankbased(), "no device replay for memory 'RankBased'"),
                           (lambda c: c.memory.set_rankbased_linear(), "no device replay for memory 'RankBasedLinear'"),
                           (lambda c: setattr(c.memory, "enable_demo_memory", True), "demo memory"),
                           (lambda c: setattr(c, "window_length", 4), "window_length 1"),
                           (lambda c: setattr(c, "burnin", 600), "outside the lane gather's 2..513"),
                           (lambda c: setattr(c, "lstm_units", 2048), "outside the lane gather's 1..1024"),
                           (lambda c: setattr(c, "batch_size", 2048), "outside the lane gather's 1..1024")):
        c = _config()
        c._set_device("cuda:0")
        change(c)
        assert reason in vr.why_not_r2d2_engine(_Env(), c), reason
    c = _config()
    c._set_device("cuda:0")
    c._obs_processors = [(object(), None, None)]
    assert "observation processors" in vr.why_not_r2d2_engine(_Env(), c)
    # the reasons that depend on the lane count, when the caller has one
    c = _config()
    c._set_device("cuda:0")
    c.memory.capacity = 50  # sequence length 3: 16 lanes emit up to 48 windows in a lock-step, 17 up to 51
    assert vr.why_not_r2d2_engine(_Env(), c, n_envs=16) == "" and vr.why_not_r2d2_engine(_Env(), c) == ""
    assert "more than memory.capacity 50" in vr.why_not_r2d2_engine(_Env(), c, n_envs=17)
    c.memory.capacity = 100_000
    assert vr.why_not_r2d2_engine(_Env(), c, n_envs=256) == ""
    assert "at most 256 rows" in vr.why_not_r2d2_engine(_Env(), c, n_envs=257)
    # every reason at once, joined with "; "
    c = _config()
    c.window_length, c.lstm_units = 4, 2048
    c.memory.set_rankbased()
    why = vr.why_not_r2d2_engine(_Env(discrete=False, players=2), c).split("; ")
    assert len(why) == 6 and why[0] == "the run is not on a GPU device"
    assert vr.why_not_r2d2_engine(_Env(), dqn.Config()) == "'DQN' is not an r2d2.Config"
    assert "train_mp() keeps it on the plugin path" in vr.R2D2_MP_REASON


def test_runner_without_a_gpu_keeps_r2d2_on_the_plugin_path():
    import simple_distributed_rl_amd as srl
    from r2d2_lanes_reference import register_corridor

    register_corridor()
    c = _config()
    c.memory.warmup_size = 1000
    runner = srl.Runner(srl.EnvConfig("R2D2Corridor-v0"), c)
    runner.set_device("CPU")
    runner.set_vector_envs(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the plugin's trainer says so itself: its arithmetic is libsrlx's)
        runner.train(max_steps=5)
    assert runner.vector_reason == "the run is not on a GPU device"


def test_lane_memory_takes_serials_and_refuses_items_backup_and_restore():
    from simple_distributed_rl_amd.algorithms import r2d2
    from simple_distributed_rl_amd.device.r2d2 import LaneMemory

    class Store:
        class ledger:
            seq_capacity = 100

    c = _config()
    c.memory.capacity, c.memory.warmup_size = 100, 8  # (the default ReplayBuffer memory: the proportional tree lives on the GPU)
    plain = r2d2.Memory(c)
    assert not hasattr(plain, "add_serial")  # the plugin path's memory is what it was
    mem = LaneMemory(c)
    with pytest.raises(RuntimeError, match="no lane ring"):
        mem.add_serial(0)
    Store.ledger.seq_capacity = 99
    with pytest.raises(ValueError, match="capacity"):
        mem.attach_lane_store(Store())
    Store.ledger.seq_capacity = 100
    mem.attach_lane_store(Store())
    mem.add_serial(0)
    assert mem.length() == 1
    with pytest.raises(RuntimeError, match="pushed there"):
        mem.add({"states": []})
    with pytest.raises(RuntimeError, match="no backup format"):
        mem.call_backup()
    with pytest.raises(RuntimeError, match="no restore yet"):
        mem.call_restore([None, None])
    assert mem.length() == 1
    with pytest.raises(RuntimeError, match="already holds"):
        mem.attach_lane_store(Store())


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_r2d2_entry_points_validate_their_arguments_before_they_touch_a_device():
    """Every bad argument of srlx.h's envelope returns SRLX_ERR_INVALID and a message that names the entry point.  (No call here is valid, so none reaches a
    launch.)"""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    for name, n_args in (("srlx_r2d2_policy", 9), ("srlx_r2d2_lane_push", 22), ("srlx_r2d2_lane_gather", 24)):
        assert name in N.SIGNATURES and hasattr(lib, name) and len(N.SIGNATURES[name][1]) == n_args
    ok = dict(B=8, L=6, S=3, A=4, H=16, E=3, T=18, frame_elems=64, frame_stride=64, t=5)
    g_names = ("desc", "ring_frames", "ring_scalars", "ring_invalid", "ring_hidden", "states", "actions", "probs", "rewards", "dones", "invalid", "h", "c")
    shared = [dict(A=0), dict(A=65), dict(H=0), dict(H=1025), dict(E=0), dict(E=65537), dict(frame_elems=0),
              dict(frame_elems=(1 << 20) + 1, frame_stride=(1 << 20) + 4), dict(frame_stride=63), dict(T=(1 << 31) // 3 + 1)]
    bad = shared + [dict(B=0), dict(B=-1), dict(B=1025), dict(L=1), dict(L=514, T=600), dict(S=0), dict(S=6), dict(T=5)] + [{n: None} for n in g_names]
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in g_names]
        st = lib.srlx_r2d2_lane_gather(c["B"], c["L"], c["S"], c["A"], c["H"], c["E"], c["T"], c["frame_elems"], c["frame_stride"], 7, *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_r2d2_lane_gather" in lib.srlx_last_error(), change
    p_names = ("frames", "action", "mu", "reward", "done", "invalid", "h", "c", "first", "ring_frames", "ring_scalars", "ring_invalid", "ring_hidden")
    bad = shared + [dict(T=1), dict(t=-1)] + [{n: None} for n in p_names if n != "invalid"]  # (push's invalid mask may be NULL)
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in p_names]
        st = lib.srlx_r2d2_lane_push(c["E"], c["A"], c["H"], c["frame_elems"], c["frame_stride"], c["T"], c["t"], 7, *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_r2d2_lane_push" in lib.srlx_last_error(), change
    q_names = ("q", "eps", "u", "invalid", "actions", "mu")
    bad = [dict(E=0), dict(E=-3), dict(E=65537), dict(A=0), dict(A=65)] + [{n: None} for n in q_names if n != "invalid"]  # (the mask may be NULL)
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in q_names]
        st = lib.srlx_r2d2_policy(c["E"], c["A"], *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_r2d2_policy" in lib.srlx_last_error(), change
