"""srlx_sacd_act and srlx_sacd_ring_batch on the GPU (csrc/srlx_sacd.hip) against tests/sacd_engine_reference.py (whose footing
tests/test_sacd_engine_cpu.py checks).  Bars: the logits bit for bit srlx_sacd_forward(target = 0)'s and within rtol 1e-5 / atol 1e-6 of the float64 torch module
(test_sacd_gpu.py's forward bar); the scores within rtol 1e-12 / atol 1e-12 of the mirror fed the kernel's own logits (the device's float64 log is within a few
ulp of numpy's and -log(u) lies in (1e-6, 13.9], so two nested logs leave an absolute error near 2e-15: 1e-12 is about 500 times that); the actions the first
argmax of the kernel's own scores exactly, and the mirror's on every row whose top-two score gap exceeds 1e-9 -- and no row may fall under that gap.
Every test prints what it measured ("SACD-ACT ...", shown with -s) before it asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_cases as C  # noqa: E402
import sacd_engine_reference as M  # noqa: E402
import sacd_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (D, A, policy widths): every D of {1, 4, 255, 256}, every A of {2, 3, 16}, every block of {(32,), (64, 64, 64), (512, 32)}
CASES = [(1, 2, (32,)), (4, 3, (64, 64, 64)), (255, 16, (512, 32)), (256, 2, (512, 32)), (4, 16, (32,)), (256, 3, (64, 64, 64))]
ROWS = (1, 15, 16, 17, 33)
# beside the issue's rows: the launch cuts a workgroup's rows to 1, 2, 4, 8, 16 by the row count (srlx_param_tail.h: rows_per_workgroup); 300, 1000, 1030 and
# 2049 rows reach 2, 4, 8 and 16 rows per workgroup, three of them with a partly filled last workgroup
MANY_ROWS = (300, 1000, 1030, 2049)
SEED, RANDOM_UNTIL = 0x5AC0FFEE, 5


def _id(case):
    D, A, pw = case
    return f"D{D}-A{A}-p{'x'.join(map(str, pw))}"


def _handle(case, k):
    """A bound handle (max_batch = 1: acting needs no scratch) over seeded parameters whose policy out layer is NOT zero, and their float64 CPU copy."""
    from simple_distributed_rl_amd.device.sacd import SacdUpdate

    D, A, pw = case
    p = C.make_parameter(C.make_config(D, A, pw, (32,), device="cuda"), 2000 + k)
    assert float(p.policy.out_layer.weight.detach().abs().max()) > 0
    p64 = R.Yardstick(C.make_parameter(C.make_config(D, A, pw, (32,), device="cpu"), 2000 + k), 0, 0, 0, C.DISCOUNT, C.TAU, True, -A)
    return SacdUpdate(p, max_batch=1), p64


def _ring(n, D, k, table=True):
    """A ring of n + 3 rows and a table of n offsets (in floats) that permutes rows and repeats one; table=False: dense rows, no table."""
    g = torch.Generator().manual_seed(k)
    ring = torch.randn(n + 3, D, generator=g)
    if not table:
        return ring, None, ring[:n].clone()
    idx = torch.randperm(n + 3, generator=g)[:n]
    if n > 1:
        idx[-1] = idx[0]
    return ring, idx * D, ring[idx].clone()


def _act(u, n, ring_d, off_d, counter, want_logits=True, want_scores=True, random_until=RANDOM_UNTIL):
    """One launch with a guard row behind every output; returns host arrays (None where not asked for)."""
    A = u.A
    c = torch.tensor([counter], dtype=torch.int64, device="cuda")
    actions = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    logits = torch.full((n + 1, A), 7.0, dtype=torch.float32, device="cuda") if want_logits else None
    scores = torch.full((n + 1, A), 7.0, dtype=torch.float64, device="cuda") if want_scores else None
    u.act(n, ring_d, off_d, SEED, c, random_until, actions, logits=logits, scores=scores)
    torch.cuda.synchronize()
    assert int(c.item()) == counter, "the counter is read, not advanced"
    assert int(actions[n]) == -7 and (logits is None or bool((logits[n] == 7.0).all())) and (scores is None or bool((scores[n] == 7.0).all())), "a store past n_rows"
    return (actions[:n].cpu().numpy(), None if logits is None else logits[:n].cpu().numpy(), None if scores is None else scores[:n].cpu().numpy())


def _check_rows(u, p64, case, n, k, table, stats):
    D, A, pw = case
    ring, off, x = _ring(n, D, k, table)
    ring_d, off_d = ring.cuda(), None if off is None else off.cuda()
    counter = RANDOM_UNTIL + 3
    actions, logits, scores = _act(u, n, ring_d, off_d, counter)
    # the logits: srlx_sacd_forward's bits, and the float64 module's values
    fwd, _ = u.forward(x.cuda(), want_q=False)
    torch.cuda.synchronize()
    assert np.array_equal(logits.view(np.int32), fwd.cpu().numpy().view(np.int32)), "logits differ from srlx_sacd_forward(target = 0) in some bit"
    with torch.no_grad():
        want = p64.policy(x.double()).numpy()
    stats["logits"] = max(stats["logits"], float((np.abs(logits - want) / (1e-6 + 1e-5 * np.abs(want))).max()))
    np.testing.assert_allclose(logits, want, rtol=1e-5, atol=1e-6)
    # the scores: the mirror on the kernel's own logits
    m_actions, m_scores = M.act(logits, SEED, counter, RANDOM_UNTIL, A)
    stats["scores"] = max(stats["scores"], float((np.abs(scores - m_scores) / (1e-12 + 1e-12 * np.abs(m_scores))).max()))
    np.testing.assert_allclose(scores, m_scores, rtol=1e-12, atol=1e-12)
    # the actions: the first maximum of the kernel's own scores; the mirror's wherever the gap is wide -- and it is wide everywhere
    assert np.array_equal(actions, M.first_argmax(scores))
    gap = M.top_two_gap(m_scores)
    stats["gap"] = min(stats["gap"], float(gap.min()))
    assert float(gap.min()) > 1e-9, f"a row's top-two score gap {gap.min():.3e} is under 1e-9: pick another seed (no row may be skipped)"
    assert np.array_equal(actions, m_actions)
    # the random phase on both sides of random_until; every optional output NULL
    for c in (RANDOM_UNTIL - 1, RANDOM_UNTIL):
        a_full, lg, sc = _act(u, n, ring_d, off_d, c)
        want_a, want_s = M.act(lg, SEED, c, RANDOM_UNTIL, A)
        assert np.array_equal(a_full, want_a), f"counter {c}"
        assert np.array_equal(lg.view(np.int32), logits.view(np.int32)), "the logits are written in both phases"
        np.testing.assert_allclose(sc, want_s, rtol=1e-12, atol=1e-12)
        a_bare, _, _ = _act(u, n, ring_d, off_d, c, want_logits=False, want_scores=False)
        assert np.array_equal(a_bare, a_full)
        a_one, lg_one, _ = _act(u, n, ring_d, off_d, c, want_scores=False)
        assert np.array_equal(a_one, a_full) and np.array_equal(lg_one.view(np.int32), logits.view(np.int32))
    assert set(M.random_actions(M.uniforms(SEED, RANDOM_UNTIL - 1, n, A), A).tolist()) <= set(range(A))
    # equal inputs, equal bits
    again = _act(u, n, ring_d, off_d, counter)
    assert np.array_equal(again[0], actions) and np.array_equal(again[1].view(np.int32), logits.view(np.int32)) and np.array_equal(again[2].view(np.int64), scores.view(np.int64))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_act_over_the_row_edges(k):
    """1, 15, 16, 17 and 33 rows through an offset table that permutes rows and repeats one, and through a NULL table."""
    case = CASES[k]
    u, p64 = _handle(case, k)
    stats = dict(logits=0.0, scores=0.0, gap=np.inf)
    for n in ROWS:
        for table in (True, False):
            _check_rows(u, p64, case, n, 100 * k + n, table, stats)
    print(f"SACD-ACT {_id(case)} logits={stats['logits']:.3f} of the bar, scores={stats['scores']:.3e} of the bar, smallest top-two gap={stats['gap']:.3e}")


def test_act_over_every_rows_per_workgroup_cut():
    case = CASES[1]
    u, p64 = _handle(case, 1)
    stats = dict(logits=0.0, scores=0.0, gap=np.inf)
    for n in MANY_ROWS:
        _check_rows(u, p64, case, n, 7000 + n, True, stats)
    print(f"SACD-ACT many rows {_id(case)} logits={stats['logits']:.3f} of the bar, scores={stats['scores']:.3e} of the bar, smallest top-two gap={stats['gap']:.3e}")


def test_act_random_phase_covers_every_action_and_zero_random_until_never_draws_it():
    case = CASES[4]  # A = 16
    u, _ = _handle(case, 4)
    ring, off, _ = _ring(33, case[0], 5)
    a, _, _ = _act(u, 33, ring.cuda(), off.cuda(), 0)
    want, _ = M.act(np.zeros((33, 16), np.float32), SEED, 0, RANDOM_UNTIL, 16)
    assert np.array_equal(a, want) and len(set(a.tolist())) > 8
    a0, lg, _ = _act(u, 33, ring.cuda(), off.cuda(), 0, random_until=0)
    assert np.array_equal(a0, M.act(lg, SEED, 0, 0, 16)[0])


def test_act_on_a_wide_handle_after_a_narrower_one_was_created():
    """The kernel's dynamic-LDS cap is per function, not per handle: a handle created later with narrower rows (still above 64 KB) must not lower it under
    what the earlier, wider handle launches with."""
    wide = (256, 2, (512, 32))
    u, p64 = _handle(wide, 3)
    narrow, _ = _handle((256, 2, (288,)), 9)
    stats = dict(logits=0.0, scores=0.0, gap=np.inf)
    _check_rows_act_only(u, p64, wide, 17, 31, stats)
    _check_rows_act_only(narrow, None, (256, 2, (288,)), 17, 32, stats)


def _check_rows_act_only(u, p64, case, n, k, stats):
    """srlx_sacd_act alone (no srlx_sacd_forward launch): logits against the float64 module when given, actions against the mirror."""
    D, A, pw = case
    ring, off, x = _ring(n, D, k)
    actions, logits, scores = _act(u, n, ring.cuda(), off.cuda(), RANDOM_UNTIL)
    if p64 is not None:
        with torch.no_grad():
            np.testing.assert_allclose(logits, p64.policy(x.double()).numpy(), rtol=1e-5, atol=1e-6)
    m_actions, m_scores = M.act(logits, SEED, RANDOM_UNTIL, RANDOM_UNTIL, A)
    np.testing.assert_allclose(scores, m_scores, rtol=1e-12, atol=1e-12)
    assert float(M.top_two_gap(m_scores).min()) > 1e-9 and np.array_equal(actions, m_actions)


def test_act_refusals_name_the_entry_point():
    from simple_distributed_rl_amd.device.sacd import _int_array

    lib = N.lib()
    u, _ = _handle(CASES[0], 0)
    x = torch.zeros((4, 1), device="cuda")
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    ok = dict(h=u._h, n=4, obs=N.tptr(x), off=None, counter=N.tptr(c), until=1, actions=N.tptr(a))
    fresh = N.c_p()
    N.check(lib.srlx_sacd_create(ctypes.byref(fresh), 1, 2, 1, _int_array((32,)), 1, _int_array((32,)), 1, 0))
    try:
        for change, word in ((dict(h=None), b"NULL handle"), (dict(h=fresh), b"unbound"), (dict(n=0), b"0 rows"), (dict(n=65537), b"65537 rows"),
                             (dict(until=-1), b"random_until"), (dict(obs=None), b"NULL"), (dict(counter=None), b"NULL"), (dict(actions=None), b"NULL")):
            k = dict(ok, **change)
            st = lib.srlx_sacd_act(k["h"], k["n"], k["obs"], k["off"], SEED, k["counter"], k["until"], k["actions"], None, None, None)
            msg = lib.srlx_last_error()
            assert st == N.ERR_INVALID and b"sacd_act" in msg and word in msg, (change, msg)
        torch.cuda.synchronize()
        assert bool((a == -7).all()), "a refused call wrote actions"
    finally:
        lib.srlx_sacd_destroy(fresh)


# ---- srlx_sacd_ring_batch -----------------------------------------------------------------------------------------------------------------------------------------
def _ring_batch_case(B, D, A, aligned, base_shift=0):
    from simple_distributed_rl_amd.device.sacd import ring_batch

    g = torch.Generator().manual_seed(B * 1000 + D * 10 + A)
    rows = 64
    full = torch.arange(rows * D + 8, dtype=torch.float32) * 0.5 - 3.0  # hand-filled: element i holds i / 2 - 3, so a wrong index shows
    ring = full[base_shift:]  # (base_shift = 1: a base pointer 4 bytes off a 16-byte boundary)
    hi = rows * D - D - base_shift
    if aligned:
        hi = hi // 4 * 4
    off = torch.randint(0, hi + 1, (B, 2), generator=g)
    if aligned:
        off = off // 4 * 4
    off[0, 0], off[0, 1] = 0, hi  # both ends of the ring
    actions = torch.randint(0, A, (B, 1), generator=g, dtype=torch.int32)
    actions[0, 0] = A - 1
    rewards = torch.randn(B, 1, generator=g)
    terminated = (torch.rand(B, 1, generator=g) < 0.3).float()
    terminated[0, 0] = 1.0
    ring_d = full.cuda()[base_shift:]
    s = torch.full((B + 1, D), 7.0, device="cuda")
    n = torch.full((B + 1, D), 7.0, device="cuda")
    oh = torch.full((B + 1, A), 7.0, device="cuda")
    dn = torch.full((B + 1,), 7, dtype=torch.uint8, device="cuda")
    ring_batch(B, D, A, ring_d, off.cuda(), actions.cuda(), rewards.cuda(), terminated.cuda(), s, n, oh, dn)
    torch.cuda.synchronize()
    ws, wn, woh, wdn = M.ring_batch(ring.numpy(), off.numpy(), actions.numpy(), terminated.numpy(), D, A)
    assert np.array_equal(s[:B].cpu().numpy().view(np.int32), ws.view(np.int32)) and np.array_equal(n[:B].cpu().numpy().view(np.int32), wn.view(np.int32))
    assert np.array_equal(oh[:B].cpu().numpy(), woh) and np.array_equal(dn[:B].cpu().numpy(), wdn)
    assert bool((s[B] == 7.0).all()) and bool((n[B] == 7.0).all()) and bool((oh[B] == 7.0).all()) and int(dn[B]) == 7, "a store past B"


@pytest.mark.parametrize("B", [1, 7, 256])
def test_ring_batch_is_the_mirrors_indexing(B):
    for D in (1, 4, 255):
        for A in (2, 16):
            _ring_batch_case(B, D, A, aligned=False)
    # D = 4: the 16-byte path (every offset a multiple of 4) and the base pointer that forbids it
    _ring_batch_case(B, 4, 2, aligned=True)
    _ring_batch_case(B, 4, 2, aligned=True, base_shift=1)
    _ring_batch_case(B, 256, 16, aligned=True)


def test_ring_batch_refusals_write_nothing():
    lib = N.lib()
    t = torch.full((64,), 7.0, device="cuda")
    i64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    u8 = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    ok = [N.tptr(t), N.tptr(i64), N.tptr(i32), N.tptr(t), N.tptr(t), N.tptr(t), N.tptr(t), N.tptr(t), N.tptr(u8)]
    for B, D, A in ((0, 4, 2), (257, 4, 2), (8, 0, 2), (8, 257, 2), (8, 4, 1), (8, 4, 17)):
        assert lib.srlx_sacd_ring_batch(B, D, A, *ok, None) == N.ERR_INVALID and b"sacd_ring_batch" in lib.srlx_last_error(), (B, D, A)
    for k in range(9):
        args = list(ok)
        args[k] = None
        assert lib.srlx_sacd_ring_batch(8, 4, 2, *args, None) == N.ERR_INVALID and b"sacd_ring_batch: NULL" in lib.srlx_last_error(), k
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((u8 == 7).all())
