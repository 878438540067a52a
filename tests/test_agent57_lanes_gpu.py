"""Agent57's lane sequence ring on the GPU: srlx_seq_lane_push + srlx_seq_lane_gather against the host model of the worker's list logic
(tests/agent57_lanes_reference.py), bit for bit -- the kernels only copy -- over a ring short enough to be overwritten several times, every flush offset,
padding on either side and on both, repeated windows, both copy paths; and the reference's recorded rollout replayed through one lane."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, L, S, H, C = 3, 6, 3, 16, 18  # burnin 2 + S 3 + 1; C = E L, the smallest memory a lock-step's windows fit


def _push(store, st, dev):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    hid = st["hidden"]
    store.push(t(st["frames"]), t(st["action"]), t(st["r_ext"]), t(st["r_int"]), t(st["undone"]), t(st["actor"]), t(hid[:, 0]), t(hid[:, 1]), t(hid[:, 2]),
               t(hid[:, 3]), first=st["first"], invalid=None if st["invalid"] is None else t(st["invalid"]))
    return store.emit(st["done"])


def _assert_batch_equals(batch, windows):
    got = {k: v.cpu().numpy() for k, v in batch.tensors().items()}
    for b, w in enumerate(windows):
        where = f"row {b}, window {w['desc']}"
        np.testing.assert_array_equal(got["states"][b], w["states"], err_msg=where)
        np.testing.assert_array_equal(got["act_idx"][b], w["actions"], err_msg=where)
        np.testing.assert_array_equal(got["r_ext"][b], w["r_ext"], err_msg=where)
        np.testing.assert_array_equal(got["r_int"][b], w["r_int"], err_msg=where)
        np.testing.assert_array_equal(got["dones"][b], w["dones"], err_msg=where)
        np.testing.assert_array_equal(got["invalid"][b], w["invalid"], err_msg=where)
        assert got["actor"][b] == w["actor"], where
        for i, k in enumerate(("h_ext", "c_ext", "h_int", "c_int")):
            np.testing.assert_array_equal(got[k][b], w["hidden"][i], err_msg=where + " " + k)
    assert got["states"].dtype == np.float32 and got["act_idx"].dtype == np.int64 and got["actor"].dtype == np.int64 and got["invalid"].dtype == np.uint8


@pytest.mark.parametrize("A,shape", [(3, (5,)), (4, (5,)), (3, (64,)), (4, (8, 8, 1))], ids=["A3-dword", "A4-dword", "A3-float4", "A4-float4"])
def test_push_and_gather_equal_the_host_model(A, shape):
    from agent57_lanes_reference import LanesModel, scripted_stream
    from simple_distributed_rl_amd.device.sequence_store import LaneSequenceStore

    dev = torch.device("cuda:0")
    store = LaneSequenceStore(dev, E, C, L, S, A, H, shape, seed=0xA57 + A)
    T = store.ledger.ring_len
    assert T == C // E + 2 * L
    model = LanesModel(E, L, S, A, H, shape, seed=store.seed)
    live, seen_k, seen_pad, firsts_on_row0, n_steps = [], set(), set(), 0, 0
    for st in scripted_stream(7 + A, E, L, A, H, shape, cycles=2):
        t = store.ledger.t
        firsts_on_row0 += int(t % T == 0 and st["first"].any())
        serials = _push(store, st, dev)
        windows = model.push(st["frames"], st["action"], st["r_ext"], st["r_int"], st["undone"], st["actor"], st["hidden"], st["first"], st["done"], st["invalid"])
        assert len(windows) == len(serials)
        assert [w["desc"] for w in windows] == [tuple(r) for r in store.ledger.descriptors(serials).tolist()]
        live = (live + list(zip(serials.tolist(), windows)))[-C:]
        n_steps += 1
        if not live:
            continue
        picks = live + [live[0], live[len(live) // 2], live[0]]  # every live window (old ones after the ring has moved on), and one window three times
        _assert_batch_equals(store.gather_serials([s for s, _ in picks]), [w for _, w in picks])
        for w in windows:
            before, after = bool(w["is_pad"][0]) and not w["states"][0].any(), w["desc"][2] > 0
            seen_k.add(w["desc"][2])
            seen_pad.add((before, after))
    assert n_steps > 3 * T  # every ring row was overwritten at least twice
    assert seen_k == set(range(L))
    assert seen_pad == {(False, False), (True, False), (False, True), (True, True)}
    assert firsts_on_row0 >= 2  # position 0, and a lane that begins an episode on the ring's first row after a wrap
    with pytest.raises(Exception, match="not among the last"):
        store.gather_serials([store.ledger.serial - C - 1])
    with pytest.raises(RuntimeError, match="no backup format"):
        store.backup()


def test_descriptors_outside_the_ring_read_nothing():
    from agent57_lanes_reference import scripted_stream
    from simple_distributed_rl_amd.device.sequence_store import LaneSequenceStore

    dev = torch.device("cuda:0")
    store = LaneSequenceStore(dev, E, C, L, S, 3, H, (5,), seed=1)
    for i, st in enumerate(scripted_stream(1, E, L, 3, H, (5,), cycles=1)):
        _push(store, st, dev)
        if i == 8:
            break
    batch = store.gather(np.array([[E, 3, 0], [-1, 3, 0], [0, -1, 0], [0, 3, L], [0, 3, -1]], np.int64))
    for k, v in batch.tensors().items():
        assert not v.cpu().numpy().any(), k


def test_fixture_replay_through_one_lane():
    """The reference worker's recorded rollout (rollout_items_agent57.npz) pushed through the kernels at E = 1: every gathered window equals the recorded item."""
    from agent57_lanes_reference import LanesModel
    from simple_distributed_rl_amd.device.sequence_store import LaneSequenceStore
    from test_agent57_lanes_cpu import assert_windows_equal_fixture, fixture_replay

    dev = torch.device("cuda:0")
    store = LaneSequenceStore(dev, 1, 64, 6, 3, 4, 16, (8, 8, 1), seed=5)
    model = LanesModel(1, 6, 3, 4, 16, (8, 8, 1), seed=store.seed)  # (tells which action entries are pads)

    def push(st):
        serials = _push(store, st, dev)
        pads = [w["is_pad"] for w in model.push(**st)]
        if not len(serials):
            return []
        got = {k: v.cpu().numpy() for k, v in store.gather_serials(serials).tensors().items()}
        return [dict(states=got["states"][b], actions=got["act_idx"][b], is_pad=pads[b], r_ext=got["r_ext"][b], r_int=got["r_int"][b], dones=got["dones"][b],
                     actor=int(got["actor"][b]), hidden=np.stack([got[k][b] for k in ("h_ext", "c_ext", "h_int", "c_int")])) for b in range(len(serials))]

    z, out = fixture_replay(push)
    assert_windows_equal_fixture(z, [w for ws in out for w in ws])
