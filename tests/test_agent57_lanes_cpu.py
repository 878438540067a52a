"""Agent57's lane sequence ring and the engine's route, the parts that need no GPU: the host model of the padding rules against the reference's
recorded items, `LaneLedger`'s serial order, counts and refusals, the reasons of `why_not_agent57_engine` and of the two `Runner` paths that keep the plugin,
and the argument checks of the two entry points."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture_replay(push):
    """Replays tests/golden/rollout_items_agent57.npz (14 steps, episodes of 4, L = 6, H = 16, one environment) as lock-steps of ONE lane: `push(step)` is called
    per log record with the `scripted_lockstep` fields and returns whatever the consumer makes of it.  The recurrent vectors are pushed where the fixture
    records them: an item's vectors are those of its head position, so a first pass with zero vectors finds every window's head, and the replay proper pushes
    at position p the vectors of the item whose (unpadded) head p is.  Returns (fixture, [push results])."""
    from agent57_lanes_reference import LanesModel

    z = np.load(os.path.join(GOLDEN, "rollout_items_agent57.npz"))
    L, S, A, H, shape = 6, 3, 4, 16, (8, 8, 1)
    n_items = len(z["item_actor"])

    def steps(hidden_at):
        episode = -1
        for i in range(len(z["frames"])):
            first = z["env_actions"][i] < 0
            episode += int(first)
            term = bool(z["env_terminated"][i])
            actor = int(z["item_actor"][min(episode * (4 + L - 1), n_items - 1)])  # (every episode of 4 steps makes 4 + L - 1 items)
            yield dict(frames=(z["frames"][i].reshape((1,) + shape).astype(np.float32) / 255), action=np.array([max(int(z["env_actions"][i]), 0)], np.int32),
                       r_ext=z["env_rewards"][i : i + 1].astype(np.float32), r_int=np.zeros(1, np.float32), undone=np.array([0.0 if term else 1.0], np.float32),
                       actor=np.array([actor], np.int32), hidden=hidden_at.get(i, np.zeros((4, H), np.float32)).reshape(1, 4, H), invalid=None,
                       first=np.array([first]), done=np.array([term]))

    probe = LanesModel(1, L, S, A, H, shape, seed=0)
    heads = []
    for st in steps({}):
        heads += [(w["head"], bool(w["is_pad"][0]) and not w["states"][0].any()) for w in probe.push(**st)]
    hidden_at = {}
    for j, (head, padded) in enumerate(heads[:n_items]):
        if not padded and head >= 0:
            hidden_at[head] = np.stack([z["item_h_ext"][j, 0], z["item_c_ext"][j, 0], z["item_h_int"][j, 0], z["item_c_int"][j, 0]])
    return z, [push(st) for st in steps(hidden_at)]


def assert_windows_equal_fixture(z, windows):
    n = len(z["item_actor"])
    assert n <= len(windows) <= n + 1  # (the rollout's step budget ends the run after its last environment step, before that step's window is added)
    real = 0
    for j, w in enumerate(windows[:n]):
        np.testing.assert_array_equal(w["states"], z["item_states"][j], err_msg=f"states {j}")
        np.testing.assert_array_equal(w["r_ext"], z["item_rewards_ext"][j], err_msg=f"r_ext {j}")
        np.testing.assert_array_equal(w["r_int"], z["item_rewards_int"][j], err_msg=f"r_int {j}")
        np.testing.assert_array_equal(w["dones"], z["item_dones"][j], err_msg=f"dones {j}")
        assert w["actor"] == z["item_actor"][j], j
        want_hidden = np.stack([z["item_h_ext"][j, 0], z["item_c_ext"][j, 0], z["item_h_int"][j, 0], z["item_c_int"][j, 0]])
        np.testing.assert_array_equal(w["hidden"], want_hidden, err_msg=f"hidden {j}")
        keep = ~w["is_pad"]
        real += int(keep.sum())
        np.testing.assert_array_equal(w["actions"][keep], z["item_actions"][j][keep], err_msg=f"actions {j}")
    assert real > n  # (the comparison of the real actions is not vacuous)


def test_host_model_equals_the_reference_items():
    """The padding rules pinned on the reference: every window of the host model equals the reference worker's recorded item exactly; actions at every entry
    that is not a pad."""
    from agent57_lanes_reference import LanesModel

    model = LanesModel(1, 6, 3, 4, 16, (8, 8, 1), seed=11)
    z, out = fixture_replay(lambda st: model.push(**st))
    assert_windows_equal_fixture(z, [w for ws in out for w in ws])


def test_pad_action_restates_the_projects_generator():
    from oracle import hot_path_oracle as H
    from simple_distributed_rl_amd.device.sequence_store import pad_action

    lanes, pos = np.arange(5)[:, None], np.arange(-7, 40)[None, :]
    want = H.rng_u64(0x1234, lanes.astype(np.uint64), pos.astype(np.int64).astype(np.uint64)) % np.uint64(3)
    np.testing.assert_array_equal(pad_action(0x1234, lanes, pos, 3), want.astype(np.int64))


# ---- LaneLedger -----------------------------------------------------------------------------------------------------------------------------------------------
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


def test_ledger_serial_order_and_counts():
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger

    E, L = 3, 4
    led = LaneLedger(E, 64, L)
    want_next = 0
    for t, (first, done) in enumerate(_episode_masks([[1, 3, 2, 5], [2, 2, 2, 2, 2], [6, 1, 1, 4]])):
        assert led.push(first) == t
        serials = led.emit(done)
        counts = [0 if first[e] else 1 + (L - 1) * int(done[e]) for e in range(E)]
        np.testing.assert_array_equal(led.window_counts(first, done), counts)
        assert serials.tolist() == list(range(want_next, want_next + sum(counts)))  # serials follow the lock-steps
        want_next += sum(counts)
        want = [(e, t, k) for e in range(E) for k in range(counts[e])]  # lane-major; the step's window, then its flush windows
        assert [tuple(r) for r in led.descriptors(serials).tolist()] == want
    assert led.serial == want_next > 64
    with pytest.raises(Exception, match="not among the last 64"):
        led.descriptors([led.serial - 65])
    with pytest.raises(Exception, match="not among the last 64"):
        led.descriptors([led.serial])


def test_ledger_protocol_errors():
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger

    with pytest.raises(ValueError):
        LaneLedger(4, 4 * 6 - 1, 6)  # one lock-step's windows must fit
    led = LaneLedger(2, 32, 4)
    with pytest.raises(ValueError, match="position 0"):
        led.push([True, False])
    led.push([True, True])
    with pytest.raises(RuntimeError):
        led.push([False, False])  # the previous lock-step's emit is missing
    led.emit([False, False])
    led.push([False, False])
    led.emit([True, False])
    with pytest.raises(ValueError, match="must be first"):
        led.push([False, False])


@pytest.mark.parametrize("E,C,L", [(1, 12, 2), (3, 40, 6), (4, 24, 6), (7, 100, 5)])
def test_default_ring_never_refuses_random_episode_streams(E, C, L):
    """Seeded random episode lengths from 1 up, at the default ring length and at the derivation's minimum ceil(C / E) + L + 1; every live window's oldest
    referenced position is checked against what the ring still holds, by brute force."""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger

    for ring_len in (None, -(-C // E) + L + 1):
        rng = np.random.default_rng(E * 1000 + C)
        lengths = [rng.choice([1, 1, 2, 3, L - 1, L, L + 1, 3 * L], 400).tolist() for _ in range(E)]
        led = LaneLedger(E, C, L, ring_len)
        assert led.ring_len == (LaneLedger.default_ring_len(E, C, L) if ring_len is None else ring_len)
        live, age = [], np.zeros(E, int)
        for t, (first, done) in enumerate(_episode_masks(lengths)):
            led.push(first)  # never refuses
            assert all(lo > t - led.ring_len for lo in live), t  # what this push overwrote was referenced by no live window
            age = np.where(first, 0, age + 1)
            desc = led.descriptors(led.emit(done))
            live += [t_ - min(L - 1 - k, age[e]) for e, t_, k in desc.tolist()]
            live = live[-C:]
        assert t > 3 * led.ring_len


def test_ledger_refuses_before_any_write_at_a_ring_one_row_too_short():
    """A constructed stream: E = 2 lanes, L = 4, C = 8, both lanes in one long episode.  Every lock-step emits 2 windows, so the 8 live windows span 4 lock-steps
    and the oldest references L - 1 = 3 positions before its own: the push at position t needs positions >= t - 4 - 3 kept, T >= 8.  T = 8 runs; T = 7 refuses,
    and the refused ledger is unchanged."""
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, LedgerError

    def run(T, steps=40):
        led = LaneLedger(2, 8, 4, ring_len=T)
        led.push([True, True])
        led.emit([False, False])
        for _ in range(steps):
            led.push([False, False])
            led.emit([False, False])
        return led

    assert run(8).t == 41
    led = LaneLedger(2, 8, 4, ring_len=7)
    led.push([True, True])
    led.emit([False, False])
    refused_at = None
    for t in range(1, 40):
        before = (led.t, led.serial, led.age.copy(), led._t.copy(), led._lo.copy())
        try:
            led.push([False, False])
        except LedgerError as e:
            refused_at = t
            assert "would overwrite position" in str(e)
            after = (led.t, led.serial, led.age, led._t, led._lo)
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            break
        led.emit([False, False])
    # windows of lock-steps t - 4 .. t - 1 are live at push t; the oldest references position t - 4 - 3 once the episode is that old: first at t = 7 (position 0)
    assert refused_at == 7


# ---- reasons ---------------------------------------------------------------------------------------------------------------------------------------------------
class _Env:
    player_num = 1

    def __init__(self, n=4, discrete=True, players=1):
        from simple_distributed_rl_amd.base.spaces.box import BoxSpace
        from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

        self.action_space = DiscreteSpace(n) if discrete else BoxSpace((1,), -1, 1)
        self.player_num = players


def _config(**kw):
    from simple_distributed_rl_amd.algorithms import agent57

    c = agent57.Config(batch_size=8, actor_num=4, lstm_units=16, burnin=2, sequence_length=3, **kw)
    c.window_length = 1
    return c


def test_every_reason_of_why_not_agent57_engine():
    from simple_distributed_rl_amd.algorithms import dqn, ppo
    from simple_distributed_rl_amd.device import vector_runner as vr

    c = _config()
    assert vr.engine_kind(c) == "agent57"
    assert vr.why_not_agent57_engine(_Env(), c) == "the run is not on a GPU device"  # (a config no run has put on a device)
    c._set_device("cuda:0")
    assert vr.why_not_agent57_engine(_Env(), c) == ""
    assert "discrete action spaces" in vr.why_not_agent57_engine(_Env(discrete=False), c)
    assert "multi-player" in vr.why_not_agent57_engine(_Env(players=2), c)
    assert "outside the lane gather's 1..64" in vr.why_not_agent57_engine(_Env(n=65), c)
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
        assert reason in vr.why_not_agent57_engine(_Env(), c), reason
    c = _config()
    c._set_device("cuda:0")
    c._obs_processors = [(object(), None, None)]
    assert "observation processors" in vr.why_not_agent57_engine(_Env(), c)
    # the reasons that depend on the lane count, when the caller has one
    c = _config()
    c._set_device("cuda:0")
    c.memory.capacity = 100  # window 6: 16 lanes emit up to 96 windows in a lock-step, 17 up to 102
    assert vr.why_not_agent57_engine(_Env(), c, n_envs=16) == "" and vr.why_not_agent57_engine(_Env(), c) == ""
    assert "more than memory.capacity 100" in vr.why_not_agent57_engine(_Env(), c, n_envs=17)
    c.memory.capacity = 100_000
    assert vr.why_not_agent57_engine(_Env(), c, n_envs=256) == ""
    assert "at most 256 rows" in vr.why_not_agent57_engine(_Env(), c, n_envs=257)
    # every reason at once, joined as why_not_ppo_engine joins them
    c = _config()
    c.window_length, c.lstm_units = 4, 2048
    c.memory.set_rankbased()
    why = vr.why_not_agent57_engine(_Env(discrete=False, players=2), c).split("; ")
    assert len(why) == 6 and why[0] == "the run is not on a GPU device"
    assert vr.why_not_agent57_engine(_Env(), dqn.Config()) == "'DQN' is not an agent57.Config"
    # the answers other algorithms get are as they were
    assert vr.engine_kind(ppo.Config()) is None and vr.engine_kind(dqn.Config()) == "dqn"
    assert vr.auto_lanes_reason(_Env(), ppo.Config(), "AUTO") == ""


def test_auto_and_train_mp_reasons():
    from simple_distributed_rl_amd.device import vector_runner as vr

    c = _config()
    why = vr.auto_lanes_reason(_Env(), c, "AUTO")
    assert "set_vector_envs(n)" in why and "plugin path" in why
    assert vr.auto_lanes_reason(_Env(), c, 4) == ""
    assert "train_mp() keeps it on the plugin path" in vr.AGENT57_MP_REASON


def test_runner_without_a_gpu_keeps_agent57_on_the_plugin_path():
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.base.env import registration
    from test_plugin_surface import TinyImg  # noqa: F401

    registration.register("TinyImg", "test_plugin_surface:TinyImg", check_duplicate=False)
    c = _config(enable_intrinsic_reward=False)
    c.memory.set_replay_buffer()
    c.memory.warmup_size = 1000
    runner = srl.Runner(srl.EnvConfig("TinyImg", kwargs=dict(ep_len=3)), c)
    runner.set_device("CPU")
    runner.set_vector_envs(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the plugin's trainer says so itself: its arithmetic is libsrlx's)
        runner.train(max_steps=5)
    assert runner.vector_reason == "the run is not on a GPU device"


def test_memory_takes_a_lane_store_only_in_device_mode_and_empty():
    from simple_distributed_rl_amd.algorithms import agent57

    class Store:
        class ledger:
            seq_capacity = 100

    c = _config()
    c.memory.set_replay_buffer()  # (the proportional memory's tree lives on the GPU)
    c.memory.capacity, c.memory.warmup_size = 100, 8
    host = agent57.Memory(c)
    with pytest.raises(ValueError, match="'host'"):
        host.attach_lane_store(Store())
    with pytest.raises(RuntimeError, match="no lane ring"):
        host.add_serial(0)

    DeviceMemory = lambda c: agent57.Memory(c, sequence_store="device")  # noqa: E731
    assert agent57.Memory.sequence_store == "host"  # (the keyword is this memory's alone)
    mem = DeviceMemory(c)
    Store.ledger.seq_capacity = 99
    with pytest.raises(ValueError, match="capacity"):
        mem.attach_lane_store(Store())
    Store.ledger.seq_capacity = 100
    mem.attach_lane_store(Store())
    mem.add_serial(0)
    assert mem.length() == 1
    with pytest.raises(RuntimeError, match="pushed there"):
        mem.add([None] * 9)
    with pytest.raises(RuntimeError, match="no restore yet"):
        mem.call_restore([None, None, None])
    assert mem.length() == 1  # (refused before anything was changed)
    full = DeviceMemory(c)
    full.memory.add(0, None)
    with pytest.raises(RuntimeError, match="already holds"):
        full.attach_lane_store(Store())


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------------------------
def test_lane_entry_points_validate_their_arguments_before_they_touch_a_device():
    """Every bad argument of srlx.h's envelope returns SRLX_ERR_INVALID and a message that names the entry point.  (No call here is valid, so none reaches a
    launch.)"""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    ok = dict(B=8, L=6, S=3, A=4, H=16, E=3, T=18, frame_elems=64, frame_stride=64, t=5)
    g_names = ("desc", "ring_frames", "ring_scalars", "ring_invalid", "ring_hidden", "states", "actions", "r_ext", "r_int", "dones", "invalid", "actor", "h_ext", "c_ext",
               "h_int", "c_int")
    shared = [dict(A=0), dict(A=65), dict(H=0), dict(H=1025), dict(E=0), dict(E=65537), dict(frame_elems=0),
              dict(frame_elems=(1 << 20) + 1, frame_stride=(1 << 20) + 4), dict(frame_stride=63), dict(T=(1 << 31) // 3 + 1)]
    bad = shared + [dict(B=0), dict(B=-1), dict(B=1025), dict(L=1), dict(L=514, T=600), dict(S=0), dict(S=6), dict(T=5)] + [{n: None} for n in g_names]
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in g_names]
        st = lib.srlx_seq_lane_gather(c["B"], c["L"], c["S"], c["A"], c["H"], c["E"], c["T"], c["frame_elems"], c["frame_stride"], 7, *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_seq_lane_gather" in lib.srlx_last_error(), change
    p_names = ("frames", "action", "r_ext", "r_int", "undone", "actor", "invalid", "h_ext", "c_ext", "h_int", "c_int", "first", "ring_frames", "ring_scalars",
               "ring_invalid", "ring_hidden")
    bad = shared + [dict(T=1), dict(t=-1)] + [{n: None} for n in p_names if n != "invalid"]  # (push's invalid mask may be NULL)
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in p_names]
        st = lib.srlx_seq_lane_push(c["E"], c["A"], c["H"], c["frame_elems"], c["frame_stride"], c["T"], c["t"], 7, *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_seq_lane_push" in lib.srlx_last_error(), change
