"""R2D2's lane sequence ring on the GPU: srlx_r2d2_policy against its numpy mirror, and srlx_r2d2_lane_push + srlx_r2d2_lane_gather against the
host model of the worker's list logic (tests/r2d2_lanes_reference.py, footed on the plugin's Worker by tests/test_r2d2_lanes_cpu.py).  Everything here is bit
for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEV = "cuda:0"


# ---- srlx_r2d2_policy ----------------------------------------------------------------------------------------------------------------------------------------------
def _run_policy(q, eps, u, invalid):
    from simple_distributed_rl_amd import _native as N

    E, A = q.shape
    d = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    tq, te, tu, ti = d(q), d(eps), d(u), d(invalid)
    actions = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    mu = torch.full((E,), -7.0, dtype=torch.float32, device=DEV)
    N.check(N.lib().srlx_r2d2_policy(E, A, N.tptr(tq), N.tptr(te), N.tptr(tu), N.tptr(ti), N.tptr(actions), N.tptr(mu), N.torch_stream_ptr()))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), mu.cpu().numpy()


def _policy_case(E, A, masked, seed):
    """Random rows (half of them small integers: ties), then, where E leaves room, the forced rows: every action valid and tied; the unmasked maximum invalid;
    one valid action; no valid action; eps 0 and 1; u = 0 and u = 1 - 2^-53; u on every cumulative boundary the mirror computes, and one ulp to either side."""
    from r2d2_lanes_reference import policy_row

    rng = np.random.default_rng(seed)
    q = rng.standard_normal((E, A)).astype(np.float32)
    q[::2] = rng.integers(-1, 2, (len(q[::2]), A)).astype(np.float32)
    eps = rng.choice(np.array([0.0, 0.1, 0.4, 1.0], np.float32), E)
    u = rng.random(E)
    invalid = (rng.random((E, A)) < 0.3).astype(np.uint8) if masked else None
    r = 0

    def force(row_q=None, row_inv=None, row_eps=None, row_u=None):
        nonlocal r
        if r >= E - 6:  # (the last six rows stay random: the boundary rows below are copies of them)
            return
        if row_q is not None:
            q[r] = row_q
        if row_inv is not None and masked:
            invalid[r] = row_inv
        if row_eps is not None:
            eps[r] = row_eps
        if row_u is not None:
            u[r] = row_u
        r += 1

    if E > 64:
        top = np.zeros(A, np.uint8)
        force(row_q=np.full(A, 0.25, np.float32), row_inv=np.zeros(A, np.uint8))  # every action valid and tied
        base = rng.standard_normal(A).astype(np.float32)
        top[int(np.argmax(base))] = 1
        force(row_q=base, row_inv=top if A > 1 else None)  # the unmasked maximum is invalid
        one = np.ones(A, np.uint8)
        one[A // 2] = 0
        force(row_inv=one)  # one valid action
        force(row_inv=np.ones(A, np.uint8))  # no valid action
        for e_ in (0.0, 1.0):
            for u_ in (0.0, 1.0 - 2.0**-53, 0.37):
                force(row_eps=e_, row_u=u_)
                force(row_q=np.zeros(A, np.float32), row_eps=e_, row_u=u_)
        for src in range(E - 6, E):  # each of the first eight cumulative boundaries of the last six rows, and its neighbours, on a copy of the row
            inv = None if invalid is None else invalid[src].copy()
            for b in policy_row(q[src], eps[src], 0.5, inv)[2][:8]:
                for u_ in (b, np.nextafter(b, 0.0), min(np.nextafter(b, 2.0), 1.0 - 2.0**-53)):
                    force(row_q=q[src].copy(), row_inv=inv, row_eps=eps[src], row_u=min(u_, 1.0 - 2.0**-53))
    return q, eps, u, invalid


@pytest.mark.parametrize("masked", [False, True], ids=["null-mask", "masks"])
@pytest.mark.parametrize("A", [1, 2, 3, 64])
@pytest.mark.parametrize("E", [1, 5, 257])
def test_policy_equals_the_mirror_bit_for_bit(E, A, masked):
    from r2d2_lanes_reference import policy_mirror

    q, eps, u, invalid = _policy_case(E, A, masked, seed=E * 100 + A)
    want_a, want_mu = policy_mirror(q, eps, u, invalid)
    got_a, got_mu = _run_policy(q, eps, u, invalid)
    np.testing.assert_array_equal(got_a, want_a)
    np.testing.assert_array_equal(got_mu.view(np.uint32), want_mu.view(np.uint32))
    if masked:  # an all-zero mask is a NULL mask
        zero_a, zero_mu = _run_policy(q, eps, u, np.zeros_like(invalid))
        null_a, null_mu = _run_policy(q, eps, u, None)
        np.testing.assert_array_equal(zero_a, null_a)
        np.testing.assert_array_equal(zero_mu.view(np.uint32), null_mu.view(np.uint32))
        valid_rows = ~invalid.all(axis=1)
        assert not invalid[np.arange(E), got_a][valid_rows].any()  # never an invalid action
        assert (got_a[~valid_rows] == 0).all() and (got_mu[~valid_rows] == 1).all()
    again_a, again_mu = _run_policy(q, eps, u, invalid)
    np.testing.assert_array_equal(again_a, got_a)
    np.testing.assert_array_equal(again_mu.view(np.uint32), got_mu.view(np.uint32))


# ---- push + gather -------------------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("states", "actions", "probs", "rewards", "dones", "invalid", "hidden")


def _batch_arrays(sb, S, A):
    B = sb.actions.shape[0]
    inv = np.zeros((B, S + 1, A), np.uint8) if sb.invalid_actions is None else sb.invalid_actions.cpu().numpy()
    hidden = torch.stack([sb.hidden_states[0][0], sb.hidden_states[1][0]], dim=1).cpu().numpy()  # [B][2][H]
    return dict(states=sb.states.cpu().numpy(), actions=sb.actions.cpu().numpy(), probs=sb.probs.cpu().numpy(), rewards=sb.rewards.cpu().numpy(),
                dones=sb.dones.cpu().numpy(), invalid=inv, hidden=hidden)


def _assert_rows_equal(got, row, want, what):
    for f in FIELDS:
        a, b = got[f][row], np.asarray(want[f])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, f, a, b)


@pytest.mark.parametrize("A,frame_shape,masks", [(3, (5,), "all"), (4, (64,), "all"), (3, (64,), "none"), (4, (5,), "none"), (3, (5,), "third"), (4, (8, 8), "third")])
@pytest.mark.parametrize("burnin,S", [(0, 1), (0, 3), (2, 1), (2, 3)])
def test_push_and_gather_equal_the_host_model(burnin, S, A, frame_shape, masks):
    from r2d2_lanes_reference import R2D2LanesModel, scripted_stream
    from simple_distributed_rl_amd.device.sequence_store import LaneLedger, R2D2LaneStore

    E, H, L, seed = 3, 16, burnin + S + 1, 0x51
    C = 2 * E * max(S, 2) + 1
    T = LaneLedger.min_ring_len(E, C, L, S - 1)  # the proven minimum
    store = R2D2LaneStore(DEV, E, C, L, S, A, H, frame_shape, seed=seed, ring_len=T)
    assert store.ledger.ring_len == T and (store.frame_elems % 4 == 0) == (frame_shape != (5,))
    model = R2D2LanesModel(E, L, S, A, H, frame_shape, seed)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    windows, seen_k, seen_pad = [], set(), set()
    for n, st in enumerate(scripted_stream(7 + S, E, L, S, A, H, frame_shape, cycles=3)):
        inv = st["invalid"] if masks == "all" or (masks == "third" and n >= 2) else None
        store.push(dev(st["frames"]), dev(st["action"]), dev(st["mu"]), dev(st["reward"]), dev(st["terminated"]), dev(st["hidden"][:, 0]), dev(st["hidden"][:, 1]),
                   first=st["first"], invalid=None if inv is None else dev(inv))
        serials = store.emit(st["done"])
        new = model.push(st["frames"], st["action"], st["mu"], st["reward"], st["terminated"], st["hidden"], st["first"], st["done"], invalid=inv)
        assert [w["desc"] for w in new] == [tuple(r) for r in store.ledger.descriptors(serials).tolist()]
        windows += new
        live = list(range(max(0, len(windows) - C), len(windows)))
        if not live:
            continue
        live += [live[len(live) // 2]] * 2  # one window three times in the batch
        sb = store.gather_serials(live)
        assert (sb.invalid_actions is None) == (masks == "none" or (masks == "third" and n < 2))
        got = _batch_arrays(sb, S, A)
        for row, s in enumerate(live):
            _assert_rows_equal(got, row, windows[s], (n, s, windows[s]["desc"]))
        for w in new:
            seen_k.add(w["desc"][2])
            before, after = not w["states"][0].any(), not w["states"][-1].any()
            seen_pad.add(("before" if before else "") + ("after" if after else ""))
    assert store.ledger.t > 3 * T  # the ring was overwritten three times
    assert seen_k == set(range(S)) and seen_pad >= ({""} | ({"before"} if L > 2 else set()) | ({"after", "beforeafter"} if S > 1 else set()))
    if masks != "none":
        assert any(w["invalid"].any() for w in windows)
    # descriptors outside the ranges yield zeros; two identical calls give identical bits
    t = store.ledger.t - 1
    bad = np.array([[-1, t, 0], [E, t, 0], [0, -1, 0], [0, t, -1], [0, t, S], [1, t, 0]], np.int64)
    a, b = (_batch_arrays(store.gather(bad), S, A) for _ in range(2))
    for f in FIELDS:
        assert not a[f][:5].any(), f
        assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), f
    assert a["states"][5].any()


def test_store_refuses_bad_push_arguments_before_the_ledger_moves():
    from simple_distributed_rl_amd.device.sequence_store import R2D2LaneStore

    E, A, H = 2, 3, 16
    store = R2D2LaneStore(DEV, E, 32, 6, 3, A, H, (5,), seed=1)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
    good = dict(frames=z(E, 5), action=z(E, dt=torch.int32), mu=z(E), reward=z(E), done=z(E, dt=torch.uint8), h=z(E, H), c=z(E, H))
    for k, v in (("frames", z(E, 6)), ("action", z(E, dt=torch.int64)), ("mu", z(E + 1)), ("done", z(E)), ("h", z(E, H).cpu()), ("c", z(H, E).t())):
        with pytest.raises(ValueError, match=f"push argument {k}"):
            store.push(**dict(good, **{k: v}), first=[True, True])
    with pytest.raises(ValueError, match="push argument invalid"):
        store.push(**good, first=[True, True], invalid=z(E, A + 1, dt=torch.uint8))
    assert store.ledger.t == 0 and store.any_invalid is False
    assert store.push(**good, first=[True, True]) == 0
    with pytest.raises(ValueError, match="envelope"):
        R2D2LaneStore(DEV, E, 32, 6, 3, 65, H, (5,))
