"""srlx_vppo_act on the GPU (csrc/srlx_vppo.hip) against tests/vppo_engine_reference.py (whose footing tests/test_vppo_engine_cpu.py checks).
Bars: the logits bit for bit srlx_vppo_forward's; the running sums within 1e-12 relative of the mirror fed the kernel's own logits (each weight is one float64
exp of an argument in [-88, 0] x 2: the device's exp and numpy's are each within an ulp or two of the true value, 4e-16 relative, and a sum of <= 16 positive
terms keeps the relative error of its terms plus 16 roundings, under 1e-14: 1e-12 is a hundred times that); the actions the first boundary above U1 c_{A-1} of
the kernel's own sums AND of the mirror's on every row, with no row's U1 c_{A-1} within 1e-9 c_{A-1} of a boundary; the sampled log-probability bit for bit the
new_logpi of one srlx_vppo_update on the same rows and actions.  Every test prints what it measured ("VPPO-ACT ...", shown with -s) before it asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo_v

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_cases as C  # noqa: E402
import vppo_engine_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

# (D, A, trunk, value block, policy block): policy block depth 0, 1, 2; A 2, 3, 16; the last is the wide corner
CASES = [(4, 2, (32,), (32,), ()), (4, 3, (32, 32), (), (32,)), (5, 16, (32,), (32,), (32, 32)), (1, 2, (64, 32), (), ()), (256, 16, (512,), (), (512,))]
ROWS = (1, 15, 16, 17, 33)
MANY_ROWS = (300, 1000, 1030, 2049)  # 2, 4, 8 and 16 rows per workgroup, each with a partly filled last workgroup (1000: the cut of the measured E = 1024)
SEED = 0x5EED0ACE


def _id(case):
    D, A, tw, vw, pw = case
    return f"D{D}-A{A}-t{'x'.join(map(str, tw))}-p{'x'.join(map(str, pw)) or '0'}"


def _handle(case, k, max_batch=1):
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    D, A, tw, vw, pw = case
    torch.manual_seed(3000 + k)
    p = ppo_v.Parameter(C.make_config(D, 0, A, tw, vw, pw, device="cuda"))
    g = torch.Generator().manual_seed(4000 + k)
    with torch.no_grad():
        for t in p.net.parameters():
            if t.dim() == 1:
                t.copy_((torch.randn(t.shape, generator=g) * 0.1).to(t.device))
    return VppoUpdate(p, max_batch=max_batch)


def _act(u, x_d, counter, epsilon, want_logits=True, want_cdf=True):
    """One launch with a guard row behind every output; returns host arrays (None where not asked for)."""
    n, A = x_d.shape[0], u.n_out
    c = torch.tensor([counter], dtype=torch.int64, device="cuda")
    actions = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    logp = torch.full((n + 1,), 7.0, dtype=torch.float32, device="cuda")
    logits = torch.full((n + 1, A), 7.0, dtype=torch.float32, device="cuda") if want_logits else None
    cdf = torch.full((n + 1, A), 7.0, dtype=torch.float64, device="cuda") if want_cdf else None
    u.act(n, x_d, SEED, c, epsilon, actions, logp, logits=logits, cdf=cdf)
    torch.cuda.synchronize()
    assert int(c.item()) == counter, "the counter is read, not advanced"
    assert int(actions[n]) == -7 and float(logp[n]) == 7.0 and (logits is None or bool((logits[n] == 7.0).all())) and (cdf is None or bool((cdf[n] == 7.0).all())), \
        "a store past n_rows"
    return (actions[:n].cpu().numpy(), logp[:n].cpu().numpy(), None if logits is None else logits[:n].cpu().numpy(), None if cdf is None else cdf[:n].cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _check_rows(u, case, n, k, stats, update_max=256):
    D, A, tw, vw, pw = case
    x = (0.5 * torch.randn(n, D, generator=torch.Generator().manual_seed(k))).cuda()
    counter = 11
    actions, logp, logits, cdf = _act(u, x, counter, 0.0)
    _, fwd = u.forward(x, want_v=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(logits), _bits(fwd.cpu().numpy())), "logits differ from srlx_vppo_forward in some bit"
    m_actions, m_random, m_cdf = M.act(logits, SEED, counter, 0.0)
    stats["cdf"] = max(stats["cdf"], float((np.abs(cdf - m_cdf) / np.abs(m_cdf)).max()))
    np.testing.assert_allclose(cdf, m_cdf, rtol=1e-12, atol=0)
    u1 = M.uniforms(SEED, counter, n)[1]
    gap = min(float(M.boundary_gap(cdf, u1).min()), float(M.boundary_gap(m_cdf, u1).min()))
    stats["gap"] = min(stats["gap"], gap)
    assert gap > 1e-9, f"a row's U1 c_last lies {gap:.3e} c_last from a boundary: pick another seed (no row may be skipped)"
    assert not m_random.any() and np.array_equal(actions, M.inverse_cdf(cdf, u1)) and np.array_equal(actions, m_actions)
    # epsilon 1: every row the uniform action; epsilon 0.5: both branches, as the mirror's U0 < epsilon says
    a1, lp1, lg1, _ = _act(u, x, counter, 1.0)
    assert np.array_equal(a1, M.uniform_actions(u1, A)) and bool((lp1 == M.uniform_logp(A)).all()) and np.array_equal(_bits(lg1), _bits(logits))
    ah, lph, _, cdfh = _act(u, x, counter, 0.5)
    mh, rh, _ = M.act(logits, SEED, counter, 0.5)
    assert np.array_equal(ah, mh) and np.array_equal(_bits(cdfh), _bits(cdf))
    assert np.array_equal(_bits(lph), _bits(np.where(rh, M.uniform_logp(A), logp).astype(np.float32)))
    if n >= 15:
        assert rh.any() and not rh.all(), "epsilon 0.5 took one branch only"
    # optional outputs NULL; equal inputs, equal bits
    ab, lpb, _, _ = _act(u, x, counter, 0.0, want_logits=False, want_cdf=False)
    assert np.array_equal(ab, actions) and np.array_equal(_bits(lpb), _bits(logp))
    ao, lpo, lgo, _ = _act(u, x, counter, 0.0, want_cdf=False)
    assert np.array_equal(ao, actions) and np.array_equal(_bits(lpo), _bits(logp)) and np.array_equal(_bits(lgo), _bits(logits))
    # the log-probability of EVERY row: new_logpi of srlx_vppo_update on the same rows and actions, in chunks of the update's 256 (a handle of its own over the
    # same seeded parameters, updated at lr 0: Adam's step is then p - 0, and the parameters are checked to have kept their bits)
    v = _handle(case, stats["k"], max_batch=min(n, update_max))
    for a, b in zip(u.params, v.params):
        assert torch.equal(a, b)
    for i0 in range(0, n, update_max):
        xs, acts = x[i0:i0 + update_max], torch.from_numpy(actions[i0:i0 + update_max]).cuda()
        B = xs.shape[0]
        z = torch.zeros(B, device="cuda")
        out = v.update(xs, xs, acts, torch.from_numpy(logp[i0:i0 + B]).cuda().view(B, 1), z, z, z, 0.0, 0.95, 0.1, 0.0, 0.1, 10.0, False)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["new_logpi"].view(-1).cpu().numpy()), _bits(logp[i0:i0 + B])), f"rows {i0}..: logp differs from the update's new_logpi"
        for a, b in zip(u.params, v.params):
            assert torch.equal(a, b), "an update at lr 0 moved a parameter"


@pytest.mark.parametrize("k", range(len(CASES) - 1), ids=[_id(c) for c in CASES[:-1]])
def test_act_over_the_row_edges(k):
    case = CASES[k]
    u = _handle(case, k)
    stats = dict(cdf=0.0, gap=np.inf, k=k)
    for n in ROWS:
        _check_rows(u, case, n, 100 * k + n, stats)
    print(f"VPPO-ACT {_id(case)} cdf={stats['cdf']:.3e} relative (bar 1e-12), smallest boundary gap={stats['gap']:.3e}")


def test_act_over_every_rows_per_workgroup_cut():
    case = CASES[0]  # D 4, 32-wide blocks
    u = _handle(case, 0)
    stats = dict(cdf=0.0, gap=np.inf, k=0)
    for n in MANY_ROWS:
        _check_rows(u, case, n, 7000 + n, stats)
    print(f"VPPO-ACT many rows {_id(case)} cdf={stats['cdf']:.3e} relative (bar 1e-12), smallest boundary gap={stats['gap']:.3e}")


def test_act_wide_corner_and_the_lds_cap_order():
    """The kernel's dynamic-LDS cap is per function, not per handle: a handle created later with narrower rows must not lower it under what the earlier, wider
    handle launches with (98 432 bytes at 512-wide rows)."""
    wide = CASES[-1]
    u = _handle(wide, 4)
    narrow = _handle(CASES[0], 0)
    stats = dict(cdf=0.0, gap=np.inf, k=4)
    _check_rows(u, wide, 17, 31, stats)
    _check_rows(narrow, CASES[0], 17, 32, dict(stats, k=0))
    print(f"VPPO-ACT wide {_id(wide)} cdf={stats['cdf']:.3e} relative (bar 1e-12), smallest boundary gap={stats['gap']:.3e}")


def test_act_refusals_name_the_entry_point():
    from simple_distributed_rl_amd.device.vppo import _int_array

    lib = N.lib()
    u = _handle(CASES[0], 0)
    normal = ppo_v.Parameter(C.make_config(3, 1, 2, (32,), (), (), device="cuda"))
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    un = VppoUpdate(normal, max_batch=1)
    x = torch.zeros((4, 4), device="cuda")
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    ok = dict(h=u._h, n=4, obs=N.tptr(x), counter=N.tptr(c), eps=0.1, actions=N.tptr(a), logp=N.tptr(lp))
    fresh = N.c_p()
    N.check(lib.srlx_vppo_create(ctypes.byref(fresh), 4, 0, 2, 1, _int_array((32,)), 0, _int_array(()), 0, _int_array(()), 1, 0))
    try:
        for change, word in ((dict(h=None), b"NULL handle"), (dict(h=fresh), b"unbound"), (dict(h=un._h), b"categorical"), (dict(n=0), b"0 rows"),
                             (dict(n=65537), b"65537 rows"), (dict(eps=-0.1), b"epsilon"), (dict(eps=1.5), b"epsilon"), (dict(eps=float("nan")), b"epsilon"),
                             (dict(obs=None), b"NULL"), (dict(counter=None), b"NULL"), (dict(actions=None), b"NULL"), (dict(logp=None), b"NULL")):
            k = dict(ok, **change)
            st = lib.srlx_vppo_act(k["h"], k["n"], k["obs"], SEED, k["counter"], k["eps"], k["actions"], k["logp"], None, None, None)
            msg = lib.srlx_last_error()
            assert st == N.ERR_INVALID and b"vppo_act" in msg and word in msg, (change, msg)
        torch.cuda.synchronize()
        assert bool((a == -7).all()) and bool((lp == 7.0).all()), "a refused call wrote its outputs"
    finally:
        lib.srlx_vppo_destroy(fresh)
