"""Agent57's device sequence store, the parts that need no GPU: the host ledger against a brute-force rebuild of every live sequence, its
behaviour on a long-lived frame object and on items that share nothing, srlx_seq_gather's argument checks, and the plugin switch's refusals."""
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SEQ_CAPACITY = 7


def _scripted_stream(L, lengths, shape, seed=0):
    """The frame lists `agent57.Worker` emits (on_reset / _shift / _add_memory restated): one add per step, L - 1 flush adds padded with the shared all-zero
    dummy after the episode's end; consecutive lists share their frame OBJECTS."""
    rng = np.random.default_rng(seed)
    dummy = np.zeros(shape, np.float32)
    fresh = lambda: (rng.random(shape) + 0.5).astype(np.float32)  # noqa: E731
    for n in lengths:
        recent = [dummy] * (L - 1) + [fresh()]
        for _ in range(n):
            recent = recent[1:] + [fresh()]
            yield recent[:]
        for _ in range(L - 1):
            recent = recent[1:] + [dummy]
            yield recent[:]


def _replay_against_brute_force(stream, L, frame_capacity=None):
    """Applies every plan to a numpy ring and, after every add, rebuilds ALL live sequences from ring + table and compares with deep copies of the items."""
    from simple_distributed_rl_amd.device.sequence_store import SequenceLedger

    led = SequenceLedger(SEQ_CAPACITY, L, frame_capacity)
    ring, live = None, {}
    for frames in stream:
        want = np.array([np.asarray(f, np.float32).reshape(-1) for f in frames])  # the deep copy, taken before the plan
        if ring is None:
            ring = np.full((led.frame_capacity, want.shape[1]), np.nan, np.float32)
        serial = led.serial
        plan = led.plan(frames)
        assert plan.serial == serial and plan.seq_slot == serial % SEQ_CAPACITY and plan.table.dtype == np.int32 and plan.table.shape == (L,)
        for slot, frame in plan.uploads:
            assert 0 <= slot < led.frame_capacity
            ring[slot] = np.asarray(frame, np.float32).reshape(-1)
        live[plan.seq_slot] = (plan.table.copy(), want)  # (the slot's previous sequence is no longer live)
        for table, orig in live.values():
            got = np.where((table >= 0)[:, None], ring[np.maximum(table, 0)], np.float32(0))
            np.testing.assert_array_equal(got, orig)
    return led


@pytest.mark.parametrize("L", [2, 6])
@pytest.mark.parametrize("pattern", ["ones", "mixed"])
def test_ledger_keeps_every_live_sequence_intact_on_the_scripted_stream(L, pattern):
    frame_capacity = SEQ_CAPACITY + 2 * L
    if pattern == "ones":
        lengths = [1] * (3 * frame_capacity // 2 + 4)  # two uploads per episode: past three wraps of the frame ring
    else:
        lengths = [2, L - 1, L, L + 3, 1, 40] * 4
    led = _replay_against_brute_force(_scripted_stream(L, lengths, (3,)), L)
    assert led.frame_capacity == frame_capacity
    adds = sum(n + L - 1 for n in lengths)
    assert led.serial == adds
    assert led.uploads > 3 * frame_capacity
    assert led.uploads == sum(n + 1 for n in lengths) <= adds + 2 * len(lengths)  # one upload per distinct non-zero frame


@pytest.mark.parametrize("L", [2, 6])
def test_ledger_keeps_every_live_sequence_intact_on_the_real_worker_stream(L):
    """Items of the real CPU worker (TinyImg, no intrinsic reward) with `memory.add` intercepted."""
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=False, ep_len=5, seed=3)
    rl.burnin, rl.sequence_length = (0, 1) if L == 2 else (2, 3)
    runner.set_seed(7)
    items = []
    runner.memory.add = lambda batch, priority=None, serialized=False: items.append(batch)
    steps = 4 * (SEQ_CAPACITY + 2 * L)
    runner.rollout(max_steps=steps)
    assert len(items) >= steps and all(len(it[0]) == L for it in items)
    led = _replay_against_brute_force((it[0] for it in items), L)
    episodes = steps // 5 + 1
    assert 3 * led.frame_capacity < led.uploads <= len(items) + 2 * episodes


def test_ledger_uploads_a_long_lived_object_again_before_its_slot_is_reused():
    """The same ndarray object as every observation for three times the frame ring, then the same object between fresh frames: no stale slot either way."""
    L = 6
    F = SEQ_CAPACITY + 2 * L
    obj = np.full((3,), 0.25, np.float32)
    led = _replay_against_brute_force(([obj] * L for _ in range(3 * F)), L)
    assert led.uploads == 1
    rng = np.random.default_rng(1)

    def mixed():
        recent = [obj] * L
        for i in range(12 * F):
            recent = recent[1:] + [obj if i % 2 else (rng.random(3) + 0.5).astype(np.float32)]
            yield recent[:]

    led = _replay_against_brute_force(mixed(), L, frame_capacity=4 * F)
    assert led.refresh_age == (4 * F - SEQ_CAPACITY - 2) // 2 < 2 * F
    assert led.uploads >= 6 * F + 3  # 6 F fresh frames: the long-lived object went up at the start and at least twice more (once per refresh_age uploads)


def test_ledger_refuses_items_that_share_no_frames_before_a_live_sequence_is_corrupted():
    from simple_distributed_rl_amd.device.sequence_store import LedgerError

    L = 6
    stream = (pickle.loads(pickle.dumps(frames)) for frames in _scripted_stream(L, [40], (3,)))
    with pytest.raises(LedgerError, match="share no frame objects"):
        _replay_against_brute_force(stream, L)  # (every add before the refusal was checked against the brute force)
    # with L slots per add the same stream is held
    stream = (pickle.loads(pickle.dumps(frames)) for frames in _scripted_stream(L, [40], (3,)))
    _replay_against_brute_force(stream, L, frame_capacity=(SEQ_CAPACITY + 1) * L)


def test_ledger_plan_changes_nothing_when_it_refuses():
    from simple_distributed_rl_amd.device.sequence_store import LedgerError, SequenceLedger

    L = 2
    led = SequenceLedger(SEQ_CAPACITY, L)
    fresh = lambda: [np.ones(3, np.float32), np.ones(3, np.float32)]  # noqa: E731
    with pytest.raises(LedgerError):
        for _ in range(100):
            before = (led.serial, led.uploads)
            led.plan(fresh())
    assert (led.serial, led.uploads) == before
    with pytest.raises(ValueError):
        SequenceLedger(SEQ_CAPACITY, L, frame_capacity=SEQ_CAPACITY + 2 * L - 1)
    with pytest.raises(ValueError):
        led.plan([np.ones(3, np.float32)] * 3)


def test_record_layout_matches_libsrlx_and_packs_what_the_trainer_would_build():
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.sequence_store import RecordLayout

    lib = N.lib()
    for L, S, A, H in ((2, 1, 1, 1), (6, 3, 5, 16), (121, 80, 18, 512), (513, 512, 64, 1024)):
        assert lib.srlx_seq_record_dwords(L, S, A, H) == RecordLayout(L, S, A, H).dwords
    for L, S, A, H in ((1, 1, 2, 16), (514, 3, 2, 16), (6, 6, 2, 16), (6, 0, 2, 16), (6, 3, 0, 16), (6, 3, 65, 16), (6, 3, 2, 0), (6, 3, 2, 1025)):
        assert lib.srlx_seq_record_dwords(L, S, A, H) == -1
    lay = RecordLayout(6, 3, 5, 16)
    rng = np.random.default_rng(0)
    eye = np.identity(5, dtype=int)
    acts = rng.integers(0, 5, 6)
    item = [None, [eye[a] for a in acts], list(rng.random(6)), list(rng.random(6)), [1, 1, 0], 3, [[], [4, 0], [2]],
            [rng.random((1, 16)).astype(np.float32), rng.random((1, 16)).astype(np.float32)], [rng.random((1, 16)).astype(np.float32), rng.random((1, 16)).astype(np.float32)]]
    row = np.full(lay.dwords, -7, np.int32)
    table = np.array([-1, 3, 4, 5, 6, -1], np.int32)
    assert lay.pack(row, table, item) is True
    f32 = row.view(np.float32)
    np.testing.assert_array_equal(row[:6], table)
    np.testing.assert_array_equal(row[6:12], acts)
    np.testing.assert_array_equal(f32[12:18], np.asarray(item[2], np.float32))
    np.testing.assert_array_equal(f32[18:24], np.asarray(item[3], np.float32))
    np.testing.assert_array_equal(f32[24:27], [1, 1, 0])
    assert row[27] == 3
    np.testing.assert_array_equal(f32[28:92], np.concatenate([item[7][0][0], item[7][1][0], item[8][0][0], item[8][1][0]]))
    want = np.zeros((3, 5), np.uint8)
    want[1, 4] = want[1, 0] = want[2, 2] = 1
    np.testing.assert_array_equal(row.view(np.uint8)[4 * 92 : 4 * 92 + 15].reshape(3, 5), want)
    item[6] = [[], [], []]
    assert lay.pack(row, table, item) is False and not row.view(np.uint8)[4 * 92 : 4 * 92 + 15].any()


def test_seq_gather_validates_its_arguments_before_it_touches_a_device():
    """Every bad argument of srlx.h's envelope returns a status and a message that names the entry point.  (No call here is valid, so none reaches a launch.)"""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    ok = dict(B=8, L=6, S=3, A=4, H=16, frame_elems=64, frame_stride=64, frame_capacity=19, seq_capacity=7, record_stride=int(lib.srlx_seq_record_dwords(6, 3, 4, 16)))
    names = ("slots", "ring", "records", "states", "actions", "r_ext", "r_int", "dones", "invalid", "actor", "h_ext", "c_ext", "h_int", "c_int")
    bad = [dict(B=0), dict(B=-1), dict(B=1025), dict(L=1), dict(L=0), dict(L=514), dict(S=0), dict(S=6), dict(S=7), dict(A=0), dict(A=65), dict(H=0), dict(H=1025),
           dict(frame_elems=0), dict(frame_elems=(1 << 20) + 1, frame_stride=(1 << 20) + 4), dict(frame_stride=63), dict(frame_capacity=0), dict(frame_capacity=1 << 31),
           dict(seq_capacity=0), dict(record_stride=ok["record_stride"] - 1)] + [{n: None} for n in names]
    for change in bad:
        c = dict(ok, **change)
        ptrs = [None if n in change else N.c_p(4096) for n in names]
        st = lib.srlx_seq_gather(c["B"], c["L"], c["S"], c["A"], c["H"], c["frame_elems"], c["frame_stride"], c["frame_capacity"], c["seq_capacity"],
                                 c["record_stride"], *ptrs, None)
        assert st == N.ERR_INVALID, change
        assert b"srlx_seq_gather" in lib.srlx_last_error(), change


@pytest.mark.parametrize("shape,L,S,A,H", [((3,), 2, 1, 2, 16), ((7, 9, 1), 6, 3, 5, 48)], ids=["3-2-1-2-16", "7x9x1-6-3-5-48"])
def test_from_items_equals_the_restated_host_assembly(shape, L, S, A, H):
    """SequenceBatch.from_items on the CPU against `_host_assemble` (test_agent57_seqstore_gpu.py's restatement of the trainer's list branch): a single item
    without invalid actions, repeated items, 64 items; every tensor equal in dtype, shape and bits, and `any_invalid`."""
    import torch

    from simple_distributed_rl_amd.device.sequence_store import SequenceBatch
    from test_agent57_seqstore_gpu import _host_assemble, _items

    items = list(_items(L, S, A, H, shape, [2, L + 3, 1, 5] * 4 + [1], tail=2))
    quiet = [i for i, it in enumerate(items) if not any(lst for lst in it[6])]
    assert quiet and len(quiet) < len(items)
    rng = np.random.default_rng(5)
    any_seen = set()
    for picks in ([quiet[0]], [6, 0, 0, 2, 5], rng.integers(0, len(items), 64).tolist()):
        batch = [items[i] for i in picks]
        want, want_any = _host_assemble(batch, S, A, "cpu")
        got = SequenceBatch.from_items(batch, S, A, "cpu")
        assert len(got) == len(picks) and got.any_invalid is want_any
        any_seen.add(want_any)
        assert set(got.tensors()) == set(want)
        for k, v in got.tensors().items():
            assert v.dtype == want[k].dtype and v.shape == want[k].shape and v.device.type == "cpu", k
            assert torch.equal(v, want[k]), k
    assert any_seen == {False, True}


def test_invalid_mask_helper_agrees_with_the_loop_it_replaces():
    from simple_distributed_rl_amd.device.sequence_store import fill_invalid_mask

    def loop(n, A, lists):
        m, any_ = np.zeros((n, A), np.uint8), False
        for i, lst in enumerate(lists):
            for a in lst:
                m[i, a] = 1
                any_ = True
        return m, any_

    A = 5
    for lists in ([[], [4, 0], [2], []], [[3, 3, 3]], [[A - 1]], [[], [0, 1, 2, 3, 4], [], [4, 4, 0]], [np.array([1, 4]), ()]):
        want, want_any = loop(len(lists), A, lists)
        got = np.full((len(lists), A), 0xA5, np.uint8)  # (the helper clears what the mask held)
        assert fill_invalid_mask(got, lists) is True and want_any
        np.testing.assert_array_equal(got, want)
    for lists in ([[]], [[], [], []], []):
        got = np.full((3, A), 0xA5, np.uint8)
        assert fill_invalid_mask(got, lists) is False and not got.any()


@pytest.fixture
def sequence_store_switch():
    from simple_distributed_rl_amd.algorithms import agent57

    was = agent57.Memory.sequence_store
    yield agent57.Memory
    agent57.Memory.sequence_store = was


def test_memory_switch_refuses_what_the_device_store_cannot_serve(sequence_store_switch):
    from test_agent57_cpu import _agent57_runner

    Memory = sequence_store_switch
    assert Memory.sequence_store == "host"
    Memory.sequence_store = "bogus"
    runner, rl = _agent57_runner(None, intrinsic=False)
    with pytest.raises(ValueError, match="bogus"):
        runner.make_memory()
    Memory.sequence_store = "device"
    for name, setter in (("RankBased", "set_rankbased"), ("RankBasedLinear", "set_rankbased_linear")):
        runner, rl = _agent57_runner(None, intrinsic=False)
        getattr(rl.memory, setter)()
        with pytest.raises(ValueError, match=rf"the {name} memory"):
            runner.make_memory()
    runner, rl = _agent57_runner(None, intrinsic=False)
    rl.memory.enable_demo_memory = True
    with pytest.raises(ValueError, match="enable_demo_memory"):
        runner.make_memory()
    # a run without a GPU: the usual no-fallback error, at the first add (the memory is built before the run's device is known)
    runner, rl = _agent57_runner(None, intrinsic=False)
    mem = runner.make_memory()
    item = [[np.ones((8, 8, 1), np.float32)] * 6]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mem.add(item, None)
    with pytest.raises(RuntimeError, match="serialized add"):
        mem.add(*mem.serialize(item, None), serialized=True)
    assert mem.length() == 0 and mem.is_warmup_needed()


def test_host_memory_is_the_default_and_keeps_the_reference_backup_layout():
    from simple_distributed_rl_amd.algorithms import agent57
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=False)
    mem = runner.make_memory()
    assert type(mem) is agent57.Memory and mem.sequence_store == "host"
    mem.add(["an item"], None)
    assert mem.length() == 1 and len(mem.call_backup()) == 2
