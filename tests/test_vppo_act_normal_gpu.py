"""srlx_vppo_act_normal on the GPU (csrc/srlx_vppo.hip) against tests/vppo_normal_reference.py (whose footing tests/test_vppo_normal_engine_cpu.py
checks).  Bars: loc and clamped log-scale bit for bit srlx_vppo_forward's; z within 1e-12 relative of the mirror (absolute 1e-14 where |z| < 1e-2: a cosine near its
zero); the action within one float32 ulp of the mirror fed the kernel's own loc, log-scale and z; on the policy branch the log-probability of every element bit for
bit the new_logpi of srlx_vppo_update on the same rows and actions; on the epsilon branch bit for bit the mirror's float32 form given the action; the environment's
action within one ulp of the mirror's and inside the bounds.  Every test prints what it measured ("VPPO-ACT-NORMAL ...", shown with -s) before it asserts.

The action's bar and the scale.  The mirror forms sd = exp(ls) from the kernel's own log-scale.  With the host's (correctly rounded) exponential the bar is
missed -- measured on one MI355X: 286 of 6 664 actions differ, by up to 62 ulp -- and every one of those is reproduced to the bit by moving the mirror's scale
one float32 ulp: the kernel's scale is the device's expf (the update's, which is why the log-probabilities agree to the bit), which lies within an ulp of the
correctly rounded value, and where loc and sd z cancel one ulp of the scale is many of the sum.  So the mirror is fed the DEVICE's float32 exponential of that
log-scale (`_device_exp`); everything else of it stays on the host.  Then 0 of 6 664 differ.  Each test prints both figures."""
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
import vppo_normal_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

# (D, K, trunk, value block, policy block): D 1, 3, 256; K 1, 2, 8; trunk (32,) and (64, 64); policy block () and (32,); the last is the wide corner
CASES = [(3, 1, (64, 64), (64,), ()), (1, 2, (32,), (), (32,)), (256, 8, (32,), (), ()), (3, 8, (64, 64), (), (32,)), (256, 8, (512,), (), (512,))]
ROWS = (1, 15, 16, 17, 33)
MANY_ROWS = (300, 1000, 1030, 2049)  # 2, 4, 8 and 16 rows per workgroup, each with a partly filled last workgroup
SEED = 0x5EED0ACE
NOISE = 0.5
F32 = np.float32


def _id(case):
    D, K, tw, vw, pw = case
    return f"D{D}-K{K}-t{'x'.join(map(str, tw))}-p{'x'.join(map(str, pw)) or '0'}"


def _handle(case, k, max_batch=1, forced=False, **kw):
    """A Normal handle over seeded parameters (equal for equal `k`).  `forced` (K = 4): log-scale weights scaled by 2^-6 and a bias of (-1.5, 0, 1.5, 0.2), which a
    clamp of (log 0.5, log 2) meets below, inside, above and inside."""
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    D, K, tw, vw, pw = case
    torch.manual_seed(3000 + k)
    p = ppo_v.Parameter(C.make_config(D, 1, K, tw, vw, pw, device="cuda", **kw))
    g = torch.Generator().manual_seed(4000 + k)
    with torch.no_grad():
        for t in p.net.parameters():
            if t.dim() == 1:
                t.copy_((torch.randn(t.shape, generator=g) * 0.1).to(t.device))
        if forced:
            dist = p.net.policy_dist_block
            dist.log_scale_layers[0].weight.mul_(2.0 ** -6)
            dist.log_scale_layers[0].bias.copy_(torch.tensor([-1.5, 0.0, 1.5, 0.2]).to(t.device))
    return VppoUpdate(p, max_batch=max_batch)


def _bounds(K):
    j = np.arange(K, dtype=F32)
    return (-2.0 - 0.5 * j).astype(F32), (2.0 + 0.25 * j).astype(F32)


def _act(u, x_d, counter, epsilon, squashed, optional=True):
    """One launch with a guard row behind every output; returns a dict of host arrays (the optional ones only when asked for)."""
    n, K = x_d.shape[0], u.n_out
    c = torch.tensor([counter], dtype=torch.int64, device="cuda")
    low, high = (torch.from_numpy(b).cuda() for b in _bounds(K))
    f = lambda dt=torch.float32: torch.full((n + 1, K), 7.0, dtype=dt, device="cuda")  # noqa: E731
    out = dict(actions=f(), logp=f(), env=f())
    if optional:
        out.update(loc=f(), log_scale=f(), z=f(torch.float64))
    u.act_normal(n, x_d, SEED, c, epsilon, NOISE, squashed, low, high, out["actions"], out["logp"], out["env"], loc=out.get("loc"), log_scale=out.get("log_scale"),
                 z=out.get("z"))
    torch.cuda.synchronize()
    assert int(c.item()) == counter, "the counter is read, not advanced"
    for name, t in out.items():
        assert bool((t[n] == 7.0).all()), f"{name}: a store past n_rows"
    return {k: t[:n].cpu().numpy() for k, t in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _ulps(a, b):
    """The distance between two float32 arrays in units in the last place (the integers that order the floats)."""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _device_exp(log_scale):
    """exp of float32 log-scales as the DEVICE's float32 math library gives it, through torch (another program's call of it).  The kernels' scale is the device's
    expf(ls); it lies within an ulp of the correctly rounded exponential a host computes and differs from it on about one element in 25, and in loc + sd z, where
    the terms can cancel, one ulp of the scale becomes many ulps of the action (measured with the host's exponential: up to 62).  So the mirror is fed the device's
    exponential of the kernel's own log-scale; every other operation of the mirror stays on the host."""
    return torch.exp(torch.from_numpy(np.ascontiguousarray(log_scale, F32)).cuda()).cpu().numpy()


def _check_z(z, m_z, stats):
    small = np.abs(m_z) < 1e-2
    rel = np.abs(z - m_z)[~small] / np.abs(m_z)[~small]
    stats["z"] = max(stats["z"], float(rel.max(initial=0.0)))
    stats["z_abs"] = max(stats["z_abs"], float(np.abs(z - m_z)[small].max(initial=0.0)))
    assert float(rel.max(initial=0.0)) <= 1e-12 and float(np.abs(z - m_z)[small].max(initial=0.0)) <= 1e-14


def _check_rows(u, case, n, k, stats, squashed, update_max=256):
    D, K, tw, vw, pw = case
    x = (0.5 * torch.randn(n, D, generator=torch.Generator().manual_seed(k))).cuda()
    counter = 11
    low, high = _bounds(K)
    got = _act(u, x, counter, 0.0, squashed)
    _, (h0, h1) = u.forward(x, want_v=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got["loc"]), _bits(h0.cpu().numpy())), "locs differ from srlx_vppo_forward in some bit"
    assert np.array_equal(_bits(got["log_scale"]), _bits(h1.cpu().numpy())), "log-scales differ from srlx_vppo_forward in some bit"
    # the draw
    u0, ua, ub = M.uniforms(SEED, counter, n, K)
    _check_z(got["z"], M.box_muller(ua, ub), stats)
    m_actions, m_random, l, ls, sd, _ = M.act(got["loc"], got["log_scale"], SEED, counter, 0.0, NOISE, z=got["z"], scale=_device_exp(got["log_scale"]))
    d = _ulps(got["actions"], m_actions)
    stats["act_diff"] += int((d > 0).sum())
    stats["act_ulps"] = max(stats["act_ulps"], int(d.max()))
    stats["elements"] += d.size
    assert not m_random.any()
    # (a figure, not a bar: the same comparison with the host's correctly rounded exponential as the mirror's scale)
    h = _ulps(got["actions"], M.act(got["loc"], got["log_scale"], SEED, counter, 0.0, NOISE, z=got["z"])[0])
    stats["host_diff"] += int((h > 0).sum())
    stats["host_ulps"] = max(stats["host_ulps"], int(h.max()))
    # the environment's action
    m_env = M.env_action(got["actions"], low, high, squashed)
    de = _ulps(got["env"], m_env)
    stats["env_ulps"] = max(stats["env_ulps"], int(de.max()))
    # epsilon 1: every row on the noise branch; the log-probability is the mirror's float32 form given the kernel's action, bit for bit
    g1 = _act(u, x, counter, 1.0, squashed)
    a1, r1, l1, ls1, sd1, _ = M.act(got["loc"], got["log_scale"], SEED, counter, 1.0, NOISE, z=got["z"])
    d1 = _ulps(g1["actions"], a1)
    stats["eps_act_ulps"] = max(stats["eps_act_ulps"], int(d1.max()))
    lp1 = M.logp_f32(g1["actions"], l1, ls1, sd1, squashed)
    stats["eps_logp_diff"] += int((_bits(g1["logp"]) != _bits(lp1)).sum())
    # epsilon 0.5: both branches, as the mirror's U0 < epsilon says
    gh = _act(u, x, counter, 0.5, squashed)
    rh = u0 < 0.5
    want_a = np.where(rh[:, None], g1["actions"], got["actions"])
    want_lp = np.where(rh[:, None], g1["logp"], got["logp"])
    want_env = np.where(rh[:, None], g1["env"], got["env"])
    # optional outputs NULL; equal inputs, equal bits
    gb = _act(u, x, counter, 0.0, squashed, optional=False)
    print(f"VPPO-ACT-NORMAL {_id(case)} n={n} squashed={squashed}: {int((d > 0).sum())} of {d.size} actions differ from the mirror (worst {int(d.max())} ulp), "
          f"env worst {int(de.max())} ulp, epsilon-branch actions worst {int(d1.max())} ulp, epsilon-branch logp {int((_bits(g1['logp']) != _bits(lp1)).sum())} differ")
    assert int(de.max()) <= 1 and bool((got["env"] >= low).all()) and bool((got["env"] <= high).all())
    assert r1.all() and int(d1.max()) <= 1
    assert np.array_equal(_bits(g1["logp"]), _bits(lp1)), "the epsilon branch's log-probability differs from the mirror's float32 form given the action"
    assert np.array_equal(_bits(g1["loc"]), _bits(got["loc"])) and np.array_equal(_bits(g1["z"]), _bits(got["z"]))
    assert int(_ulps(g1["env"], M.env_action(g1["actions"], low, high, squashed)).max()) <= 1
    for name, want in (("actions", want_a), ("logp", want_lp), ("env", want_env)):
        assert np.array_equal(_bits(gh[name]), _bits(want)), f"epsilon 0.5: {name}"
    if n >= 15:
        assert rh.any() and not rh.all(), "epsilon 0.5 took one branch only"
    for name in ("actions", "logp", "env"):
        assert np.array_equal(_bits(gb[name]), _bits(got[name])), name
    # the log-probability of EVERY element of EVERY row: new_logpi of srlx_vppo_update on the same rows and the kernel's own actions, in chunks of the update's 256
    # (a handle of its own over the same seeded parameters, updated at lr 0: Adam's step is then p - 0, and the parameters are checked to have kept their bits)
    v = _handle(case, stats["k"], max_batch=min(n, update_max), **stats.get("kw", {}))
    for a, b in zip(u.params, v.params):
        assert torch.equal(a, b)
    for i0 in range(0, n, update_max):
        xs = x[i0:i0 + update_max]
        B = xs.shape[0]
        acts, old = torch.from_numpy(got["actions"][i0:i0 + B]).cuda(), torch.from_numpy(got["logp"][i0:i0 + B]).cuda()
        zero = torch.zeros(B, device="cuda")
        out = v.update(xs, xs, acts, old, zero, zero, zero, 0.0, 0.95, 0.1, 0.0, 0.1, 10.0, squashed)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["new_logpi"].cpu().numpy()), _bits(got["logp"][i0:i0 + B])), f"rows {i0}..: logp differs from the update's new_logpi"
        for a, b in zip(u.params, v.params):
            assert torch.equal(a, b), "an update at lr 0 moved a parameter"
    return got


def _stats(k, **kw):
    return dict(z=0.0, z_abs=0.0, act_diff=0, host_diff=0, host_ulps=0, act_ulps=0, env_ulps=0, eps_act_ulps=0, eps_logp_diff=0, elements=0, k=k, kw=kw)


def _report(name, s):
    print(f"VPPO-ACT-NORMAL {name}: z {s['z']:.3e} relative (bar 1e-12), {s['z_abs']:.3e} absolute near 0 (bar 1e-14); {s['act_diff']} of {s['elements']} actions "
          f"differ from the mirror, worst {s['act_ulps']} ulp (bar 1) [with the host's exponential as the scale: {s['host_diff']} differ, worst {s['host_ulps']} "
          f"ulp]; env worst {s['env_ulps']} ulp (bar 1)")
    # (asserted last: every other property of every size has been checked by now)
    assert s["act_ulps"] <= 1, "an action more than one float32 ulp from the mirror fed the kernel's own loc, log-scale and z"


@pytest.mark.parametrize("k", range(len(CASES) - 1), ids=[_id(c) for c in CASES[:-1]])
def test_act_normal_over_the_row_edges(k):
    case = CASES[k]
    u = _handle(case, k)
    stats = _stats(k)
    for i, n in enumerate(ROWS):
        _check_rows(u, case, n, 100 * k + n, stats, squashed=bool((i + k) % 2))
    _check_rows(u, case, 17, 100 * k + 18, stats, squashed=bool(k % 2))  # both heads of the rule at one size
    _report(_id(case), stats)


def test_act_normal_over_every_rows_per_workgroup_cut():
    case = CASES[0]  # ppo_v.Config() on Pendulum
    u = _handle(case, 0)
    stats = _stats(0)
    for i, n in enumerate(MANY_ROWS):
        _check_rows(u, case, n, 7000 + n, stats, squashed=i % 2 == 0)
    _report("many rows " + _id(case), stats)


def test_act_normal_wide_corner_and_the_lds_cap_order():
    """The kernel's dynamic-LDS cap is per function, not per handle: a handle created later with narrower rows must not lower it under what the earlier, wider
    handle launches with (98 432 bytes at 512-wide rows).  Wide, narrow, wide."""
    wide = CASES[-1]
    u = _handle(wide, 4)
    stats = _stats(4)
    _check_rows(u, wide, 17, 31, stats, squashed=True)
    narrow = _handle(CASES[0], 0)
    _check_rows(narrow, CASES[0], 17, 32, _stats(0), squashed=True)
    _check_rows(u, wide, 17, 33, stats, squashed=False)
    _report("wide " + _id(wide), stats)


def test_act_normal_log_scales_past_both_clamp_ends():
    """A log-scale Linear whose weights are scaled down and whose bias stands below, inside, above and inside a clamp of (log 0.5, log 2): the kernel's log-scale
    is the clamp's end to the bit, and the log-probability still the update's."""
    case = (4, 4, (64,), (), (32,))
    kw = dict(stable_gradients_scale_range=C.NARROW_SCALE_RANGE, forced=True)
    u = _handle(case, 9, **kw)
    stats = _stats(9, **kw)
    got = _check_rows(u, case, 33, 55, stats, squashed=True)
    lo, hi = F32(np.log(0.5)), F32(np.log(2.0))
    ls = got["log_scale"]
    assert bool((ls[:, 0] == lo).all()) and bool((ls[:, 2] == hi).all())
    assert bool(((ls[:, 1] > lo) & (ls[:, 1] < hi)).all()) and bool(((ls[:, 3] > lo) & (ls[:, 3] < hi)).all())
    _report("clamped " + _id(case), stats)


def test_act_normal_refusals_name_the_entry_point():
    from simple_distributed_rl_amd.device.vppo import VppoUpdate, _int_array

    lib = N.lib()
    u = _handle(CASES[0], 0)
    cat = VppoUpdate(ppo_v.Parameter(C.make_config(3, 0, 2, (32,), (), (), device="cuda")), max_batch=1)
    x = torch.zeros((4, 3), device="cuda")
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    low, high = torch.full((1,), -2.0, device="cuda"), torch.full((1,), 2.0, device="cuda")
    outs = [torch.full((4, 1), 7.0, device="cuda") for _ in range(5)]
    z = torch.full((4, 1), 7.0, dtype=torch.float64, device="cuda")
    ok = dict(h=u._h, n=4, obs=N.tptr(x), counter=N.tptr(c), eps=0.1, noise=0.5, sq=1, lo=-1.0, hi=1.0, low=N.tptr(low), high=N.tptr(high), actions=N.tptr(outs[0]),
              logp=N.tptr(outs[1]), env=N.tptr(outs[2]), loc=N.tptr(outs[3]), ls=N.tptr(outs[4]), z=N.tptr(z))
    fresh = N.c_p()
    N.check(lib.srlx_vppo_create(ctypes.byref(fresh), 3, 1, 1, 1, _int_array((32,)), 0, _int_array(()), 0, _int_array(()), 1, 0))
    try:
        for change, word in ((dict(h=None), b"NULL handle"), (dict(h=fresh), b"unbound"), (dict(h=cat._h), b"Normal head"), (dict(n=0), b"0 rows"),
                             (dict(n=65537), b"65537 rows"), (dict(eps=-0.1), b"epsilon"), (dict(eps=1.5), b"epsilon"), (dict(eps=float("nan")), b"epsilon"),
                             (dict(noise=0.0), b"noise scale"), (dict(noise=-1.0), b"noise scale"), (dict(noise=float("inf")), b"noise scale"),
                             (dict(noise=float("nan")), b"noise scale"), (dict(sq=2), b"squashed"), (dict(lo=1.0, hi=-1.0), b"ordered"), (dict(obs=None), b"NULL"),
                             (dict(counter=None), b"NULL"), (dict(low=None), b"NULL"), (dict(high=None), b"NULL"), (dict(actions=None), b"NULL"),
                             (dict(logp=None), b"NULL"), (dict(env=None), b"NULL"), (dict(loc=None), b"together"), (dict(ls=None), b"together")):
            k = dict(ok, **change)
            st = lib.srlx_vppo_act_normal(k["h"], k["n"], k["obs"], SEED, k["counter"], k["eps"], k["noise"], k["sq"], k["lo"], k["hi"], k["low"], k["high"], k["actions"],
                                          k["logp"], k["env"], k["loc"], k["ls"], k["z"], None)
            msg = lib.srlx_last_error()
            assert st == N.ERR_INVALID and b"vppo_act_normal" in msg and word in msg, (change, msg)
        # srlx_vppo_act keeps refusing a Normal handle as it did
        a = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        st = lib.srlx_vppo_act(u._h, 4, N.tptr(x), SEED, N.tptr(c), 0.1, N.tptr(a), N.tptr(outs[0]), None, None, None)
        assert st == N.ERR_INVALID and b"vppo_act: the acting kernel serves the categorical head" in lib.srlx_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in outs + [z]) and bool((a == -7).all()), "a refused call wrote its outputs"
    finally:
        lib.srlx_vppo_destroy(fresh)
