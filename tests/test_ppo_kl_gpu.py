"""PPO's adaptive-KL surrogate (surrogate_type "kl") on the GPU: the step-wise loss kernels (srlx_ppo_loss_categorical_kl / srlx_ppo_loss_normal_kl), the fused
minibatch (k_ppo_minibatch<CAT, true> + k_ppo_reduce_kl), the adaptation of beta in device memory, the KL rollout, the engine on both paths, captured graphs, and the
plugin trainer.  The yardstick is float64 torch autograd of tests/ppo_kl_reference.py's restatement -- through the project's `ActorCritic` module where the kernel
holds the network.  Tolerance: the project's standing one (tests/test_ppo_envelope_gpu.py) -- rtol 1e-5, atol 1e-5 of the tensor's largest entry; losses rtol 1e-4,
atol 1e-6; a tensor may be as far from float64 as twice float32 torch autograd's own distance on the same rows (measured from torch, never from the kernel, and
printed).  Rows at a ReLU kink, rows with a raw log-scale within 1e-5 of a clamp bound and rows with a new probability between 1e-11 and 1e-9 are dropped (which
side they fall on is the yardstick's precision); the filter must keep more than 2/3 of the candidates.  The old distribution is the new one's inputs + 0.5 randn, so
that kl_mean is no cancellation residue (asserted: >= 1e-3 in float64).  Every test prints what it measured ("PPO-KL ...", shown with -s) before it asserts."""
import copy
import dataclasses
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_cat_reference as R  # noqa: E402
import ppo_kl_reference as K  # noqa: E402
import test_ppo_discrete_gpu as TD  # noqa: E402
import test_ppo_net_gpu as TN  # noqa: E402
from ppo_net_reference import KINK_MARGIN, kink_margin  # noqa: E402
from test_ppo_gpu import LS_RANGE, _torch_loss  # noqa: E402

pytestmark = pytest.mark.gpu

VC, VW, EW = 0.2, 0.7, 0.01  # value clip, value weight, entropy weight
SWITCHES = [(1, 1), (0, 0), (0, 1), (1, 0)]  # (baseline_advantage, enable_value_clip)
SENTINEL = 7.0
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def _check(torch, what, pairs, losses, want_losses):
    """pairs: (name, got, want float64, float32 torch autograd's own distance).  Prints, then asserts the standing tolerance."""
    worst = max(float((g.double() - w).abs().max()) / (float(w.abs().max()) or 1.0) for _, g, w, _ in pairs)
    loss_err = float(((losses.double() - want_losses).abs() / want_losses.abs().clamp_min(1e-30)).max())
    print("PPO-KL %s: worst tensor %.3g of its largest entry, losses %.3g relative (kl_mean f64 %.6g, kernel %.6g)" % (what, worst, loss_err, float(want_losses[3]), float(losses[3])))
    for name, got, want, t32 in pairs:
        standing = 1e-5 * float(want.abs().max()) + 1e-12
        if 2 * t32 > standing:
            print("PPO-KL   float32 torch autograd itself: %s |f32 - f64| %.3g, kernel |got - f64| %.3g, standing atol %.3g -> allowed %.3g" % (
                name, t32, float((got.double() - want).abs().max()), standing, 2 * t32))
    torch.testing.assert_close(losses.double(), want_losses, rtol=1e-4, atol=1e-6)
    for name, got, want, t32 in pairs:
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=max(1e-5 * float(want.abs().max()) + 1e-12, 2 * t32), msg=lambda m: f"{what} {name}: {m}")


def _leaf_grads(torch, loss_fn, leaves, dt):
    """sum of the first three parts of loss_fn(*leaves at dt) differentiated at the leaves: (parts [4], grads)"""
    xs = [t.detach().to(dt).requires_grad_() for t in leaves]
    parts = loss_fn(dt, *xs)
    sum(parts[:3]).backward()
    return torch.stack([p.detach().double() for p in parts]), [x.grad.double() for x in xs]


# ---- 1. the step-wise loss kernels against float64 autograd ------------------------------------------------------------------------------------------------------------
def _cat_inputs(torch, dev, n, B, same=False, salt=0):
    g = torch.Generator().manual_seed(1000 * n + B + (5 if same else 0) + 100003 * salt)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    total = 3 * max(B, 64)
    logits = r(total, n)
    P64 = torch.softmax(logits.double(), dim=-1)
    keep = ~((P64 > 1e-11) & (P64 < 1e-9)).any(dim=1)
    assert 3 * int(keep.sum()) > 2 * total
    logits = logits[torch.nonzero(keep).reshape(-1)[:B]].contiguous()
    act = torch.randint(0, n, (B,), generator=g, dtype=torch.int32)
    crafted = B >= 67 and not same
    old_probs = torch.softmax(logits if same else logits + 0.5 * r(B, n), dim=-1)
    if crafted:  # row 0: a logit gap of 30 -- every other new probability is 1e-13, below the clip (its value 1e-10, no gradient through it) under ordinary old ones
        logits[0] = 0.0
        logits[0, 0] = 30.0
        act[0] = 0
    lsm = torch.log_softmax(logits, dim=-1)
    if crafted:
        old_probs[1, 0] = 0.0  # row 1: an old probability of exactly 0 (clipped to 1e-10)
    old_lp = lsm.gather(1, act.long().view(-1, 1)).squeeze(1) + (0.0 if same else 1.0) * 0.3 * r(B)
    adv, vt, v = r(B), r(B), r(B)
    ov = v + 0.3 * r(B)
    return [t.to(dev).contiguous() for t in (logits, act, old_lp, old_probs, adv, v, vt, ov)]


def _launch_cat(N, lib, torch, dev, n, inp, base, vclip, beta, target):
    logits, act, old_lp, old_probs, adv, v, vt, ov = inp
    B = logits.shape[0]
    beta_t, losses = torch.full((1,), beta, device=dev), torch.full((5,), float("nan"), device=dev)
    g_logits, g_v = torch.full((B + 1, n), SENTINEL, device=dev), torch.full((B + 1,), SENTINEL, device=dev)  # (one guard row each)
    N.check(lib.srlx_ppo_loss_categorical_kl(B, n, N.tptr(logits), N.tptr(act), N.tptr(old_lp), N.tptr(old_probs), N.tptr(adv), N.tptr(v), N.tptr(vt), N.tptr(ov), base, vclip, VC,
                                             VW, EW, target, N.tptr(beta_t), N.tptr(losses), N.tptr(g_logits), N.tptr(g_v), None))
    torch.cuda.synchronize()
    assert bool((g_logits[B:] == SENTINEL).all()) and float(g_v[B]) == SENTINEL
    return losses, float(beta_t.item()), g_logits[:B], g_v[:B]


@pytest.mark.parametrize("B", [1, 67, 257])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_stepwise_categorical_kl_loss(n, B):
    """logits [B][n] -> losses, kl_mean and the seeds d loss / d logits, d loss / d v; at B >= 67 row 0 has a logit gap of 30 and row 1 an old probability of 0.
    The target is the yardstick's kl_mean, so beta stays."""
    N, lib, torch, dev = TN._env()
    for salt in range(8):  # the input rule: a draw whose float64 kl_mean is a cancellation residue (possible at one row) is drawn again -- judged on the yardstick alone
        inp = _cat_inputs(torch, dev, n, B, salt=salt)
        logits, act, old_lp, old_probs, adv, v, vt, ov = inp
        if float(K.kl_categorical(torch, old_probs.double(), torch.softmax(logits.double(), -1)).mean()) >= 2e-3:
            break
    if B >= 67:
        assert float(torch.softmax(logits[0].double(), -1)[1]) < 2e-13 and float(old_probs[1, 0]) == 0.0
    for base, vclip in SWITCHES:
        fn = lambda dt, lg, vv: K.torch_loss_categorical(torch, lg, act, old_lp.to(dt), old_probs.to(dt), adv.to(dt), vv, vt.to(dt), ov.to(dt), base, vclip, VC, VW, EW, 0.5)  # noqa: E731
        want_l, (w_lg, w_v) = _leaf_grads(torch, fn, (logits, v), torch.float64)
        _, (f_lg, f_v) = _leaf_grads(torch, fn, (logits, v), torch.float32)
        assert float(want_l[3]) >= 1e-3
        losses, beta, g_lg, g_v = _launch_cat(N, lib, torch, dev, n, inp, base, vclip, 0.5, float(want_l[3]))
        _check(torch, "stepwise categorical n=%d B=%d switches=%d%d" % (n, B, base, vclip),
               [("d_logits", g_lg, w_lg, float((f_lg - w_lg).abs().max())), ("d_v", g_v, w_v, float((f_v - w_v).abs().max()))], losses[:4], want_l)
        assert beta == 0.5 and float(losses[4]) == 0.5
    if B >= 67:
        assert float(w_lg[0, 1:].abs().max()) < 1e-12 and float(g_lg[0, 1:].abs().max()) < 1e-12  # (the clip's zero gradient: what is left carries the factor p_k = 1e-13)


def _normal_inputs(torch, dev, A, B, same=False, salt=0):
    g = torch.Generator().manual_seed(2000 * A + B + (5 if same else 0) + 100003 * salt)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    total = 3 * max(B, 64)
    loc, ls = r(total, A), r(total, A)
    q = torch.quantile(ls.double().reshape(-1), torch.tensor([0.3, 0.7], dtype=torch.float64))
    ls_range = tuple(float(t.float()) for t in q)  # (float32 values: the kernel and the yardstick clamp at the same numbers)
    keep = ((ls.double() - ls_range[0]).abs() > 1e-5).all(dim=1) & ((ls.double() - ls_range[1]).abs() > 1e-5).all(dim=1)
    assert 3 * int(keep.sum()) > 2 * total
    rows = torch.nonzero(keep).reshape(-1)[:B]
    loc, ls = loc[rows].contiguous(), ls[rows].contiguous()
    if B >= 67:
        regions = [int((ls < ls_range[0]).sum()), int(((ls > ls_range[0]) & (ls < ls_range[1])).sum()), int((ls > ls_range[1]).sum())]
        assert min(regions) > 0, regions  # below, inside and above the clamp
    lsc = torch.clamp(ls, *ls_range)
    action = loc + torch.exp(lsc) * r(B, A)
    old_loc = loc.clone() if same else loc + 0.5 * r(B, A)
    old_ls = lsc.clone() if same else torch.clamp(ls + 0.5 * r(B, A), *ls_range)  # (recorded as clamped at acting time)
    old_lp = -HALF_LOG_2PI - lsc - 0.5 * ((action - loc) / torch.exp(lsc)) ** 2 + (0.0 if same else 1.0) * 0.3 * r(B, A)
    adv, vt, v = r(B), r(B), r(B)
    ov = v + 0.3 * r(B)
    return ls_range, [t.to(dev).contiguous() for t in (loc, ls, action, old_lp, old_loc, old_ls, adv, v, vt, ov)]


def _launch_normal(N, lib, torch, dev, A, ls_range, inp, base, vclip, beta, target):
    loc, ls, action, old_lp, old_loc, old_ls, adv, v, vt, ov = inp
    B = loc.shape[0]
    beta_t, losses = torch.full((1,), beta, device=dev), torch.full((5,), float("nan"), device=dev)
    g_loc, g_ls, g_v = torch.full((B + 1, A), SENTINEL, device=dev), torch.full((B + 1, A), SENTINEL, device=dev), torch.full((B + 1,), SENTINEL, device=dev)
    N.check(lib.srlx_ppo_loss_normal_kl(B, A, N.tptr(loc), N.tptr(ls), ls_range[0], ls_range[1], N.tptr(action), N.tptr(old_lp), N.tptr(old_loc), N.tptr(old_ls), N.tptr(adv),
                                        N.tptr(v), N.tptr(vt), N.tptr(ov), base, vclip, VC, VW, EW, target, N.tptr(beta_t), N.tptr(losses), N.tptr(g_loc), N.tptr(g_ls), N.tptr(g_v),
                                        None))
    torch.cuda.synchronize()
    assert bool((g_loc[B:] == SENTINEL).all()) and bool((g_ls[B:] == SENTINEL).all()) and float(g_v[B]) == SENTINEL
    return losses, float(beta_t.item()), g_loc[:B], g_ls[:B], g_v[:B]


@pytest.mark.parametrize("B", [1, 67, 257])
@pytest.mark.parametrize("A", [1, 4])
def test_stepwise_normal_kl_loss(A, B):
    """(loc, log_scale) [B][A] -> losses, kl_mean and the seeds; the clamp's bounds are the 30th / 70th percentile of the raw log-scales, so the KL term's gate
    (d kl / d ls2 reaches the raw log-scale inside the range only) is active below, inside and above."""
    N, lib, torch, dev = TN._env()
    for salt in range(8):  # (the input rule, as in the categorical test)
        ls_range, inp = _normal_inputs(torch, dev, A, B, salt=salt)
        loc, ls, action, old_lp, old_loc, old_ls, adv, v, vt, ov = inp
        if float(K.kl_normal(torch, old_loc.double(), old_ls.double(), loc.double(), torch.clamp(ls.double(), *ls_range)).mean()) >= 2e-3:
            break
    for base, vclip in SWITCHES:
        fn = lambda dt, lc, l_, vv: K.torch_loss_normal(torch, lc, l_, ls_range, action.to(dt), old_lp.to(dt), old_loc.to(dt), old_ls.to(dt), adv.to(dt), vv, vt.to(dt),  # noqa: E731
                                                        ov.to(dt), base, vclip, VC, VW, EW, 0.5)
        want_l, want = _leaf_grads(torch, fn, (loc, ls, v), torch.float64)
        _, f32 = _leaf_grads(torch, fn, (loc, ls, v), torch.float32)
        assert float(want_l[3]) >= 1e-3
        losses, beta, *got = _launch_normal(N, lib, torch, dev, A, ls_range, inp, base, vclip, 0.5, float(want_l[3]))
        _check(torch, "stepwise normal A=%d B=%d switches=%d%d clamp %s" % (A, B, base, vclip, ls_range),
               [(name, gt, w, float((f - w).abs().max())) for name, gt, w, f in zip(("d_loc", "d_log_scale", "d_v"), got, want, f32)], losses[:4], want_l)
        assert beta == 0.5 and float(losses[4]) == 0.5
        outside = (ls < ls_range[0]) | (ls > ls_range[1])
        assert float(got[1][outside].abs().max() if bool(outside.any()) else 0.0) == 0.0  # (outside the clamp nothing reaches the raw log-scale)


@pytest.mark.parametrize("head", ["categorical", "normal"])
def test_stepwise_old_equals_new(head):
    """Every row's old distribution is its new one (and its stored log-probability the new one): |kl_mean| <= 1e-6, and the seeds are the "" surrogate's -- float64
    autograd of the loss without any KL term -- within the standing tolerance, at beta 8."""
    N, lib, torch, dev = TN._env()
    B = 67
    for base, vclip in SWITCHES:
        if head == "categorical":
            inp = _cat_inputs(torch, dev, 3, B, same=True)
            logits, act, old_lp, old_probs, adv, v, vt, ov = inp
            fn = lambda dt, lg, vv: R.torch_loss(torch, lg, act, old_lp.to(dt), adv.to(dt), vv, vt.to(dt), ov.to(dt), base, 0, 0.2, vclip, VC, VW, EW) + (lg.sum() * 0,)  # noqa: E731
            leaves = (logits, v)
            losses, beta, *got = _launch_cat(N, lib, torch, dev, 3, inp, base, vclip, 8.0, 1.0)
            names = ("d_logits", "d_v")
        else:
            ls_range, inp = _normal_inputs(torch, dev, 2, B, same=True)
            loc, ls, action, old_lp, old_loc, old_ls, adv, v, vt, ov = inp

            def fn(dt, lc, l_, vv):
                lsc = torch.clamp(l_, *ls_range)
                lp = -HALF_LOG_2PI - lsc - 0.5 * ((action.to(dt) - lc) / torch.exp(lsc)) ** 2
                return _torch_loss(torch, lp, old_lp.to(dt), adv.to(dt), vv, vt.to(dt), ov.to(dt), base, 0, 0.2, vclip, VC, VW, EW) + (lc.sum() * 0,)

            leaves = (loc, ls, v)
            losses, beta, *got = _launch_normal(N, lib, torch, dev, 2, ls_range, inp, base, vclip, 8.0, 1.0)
            names = ("d_loc", "d_log_scale", "d_v")
        want_l, want = _leaf_grads(torch, fn, leaves, torch.float64)
        _, f32 = _leaf_grads(torch, fn, leaves, torch.float32)
        print("PPO-KL old == new %s switches=%d%d: kl_mean %.3g" % (head, base, vclip, float(losses[3])))
        assert abs(float(losses[3])) <= 1e-6
        want_l[3] = losses[3].double()  # (checked above; the other three against the "" surrogate's)
        _check(torch, "old == new " + head, [(nm, gt, w, float((f - w).abs().max())) for nm, gt, w, f in zip(names, got, want, f32)], losses[:4], want_l)
        assert beta == 4.0  # kl_mean < target / 1.5


# ---- 2. + 3. the fused minibatch against float64 autograd of the whole network; the adaptation of beta ------------------------------------------------------------------
_FUSED = {}


def _fused_fixture(cat, obs, size, mb):
    """One minibatch of `mb` samples drawn through a shuffled rows table from buffers three times as long (never shorter than 192 rows) whose unused rows hold NaN,
    the old distribution's buffers included.  Built once per case and left unchanged; returns launch(base, vclip, beta, target) and yardstick(base, vclip, beta)."""
    key = (cat, obs, size, mb)
    if key not in _FUSED:
        for salt in range(8):  # the input rule: a draw whose float64 kl_mean is a cancellation residue (possible at one sample) is drawn again -- judged on the yardstick alone
            _FUSED[key] = _build_fused(cat, obs, size, mb, salt)
            if float(_FUSED[key].yardstick(1, 1, 0.5)[0][3]) >= 2e-3:
                break
    return _FUSED[key]


def _build_fused(cat, obs, size, mb, salt):
    N, lib, torch, dev = TN._env()
    net, flat = (TD._net if cat else TN._net)(torch, dev, obs, size, 2)
    P = flat.numel()
    net64 = copy.deepcopy(net).double()
    total = 3 * max(mb, 64)
    g = torch.Generator().manual_seed(7919 * mb + 64 * obs + 8 * size + cat + 1 + 100003 * salt)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    b_obs, b_adv, b_vt = r(total, obs), r(total), r(total)
    b_act = torch.randint(0, size, (total,), generator=g, dtype=torch.int32).to(dev) if cat else r(total, size)
    order = torch.randperm(total, generator=g).to(dev)
    keep = kink_margin(torch, net, b_obs) > KINK_MARGIN
    with torch.no_grad():
        out64 = net64(b_obs.double())
        if cat:
            P64 = torch.softmax(out64[1], dim=-1)
            keep &= ~((P64 > 1e-11) & (P64 < 1e-9)).any(dim=1)
            v0, lg0 = net(b_obs)
            b_logp = torch.log_softmax(lg0, dim=-1).gather(1, b_act.long().view(-1, 1)).squeeze(1) + 0.3 * r(total)
            old = [torch.softmax(lg0 + 0.5 * r(total, size), dim=-1).contiguous()]
        else:
            keep &= ((out64[2] - LS_RANGE[0]).abs() > 1e-5).all(dim=1) & ((out64[2] - LS_RANGE[1]).abs() > 1e-5).all(dim=1)
            v0, loc0, ls0 = net(b_obs)
            ls_c = torch.clamp(ls0, *LS_RANGE)
            b_logp = -HALF_LOG_2PI - ls_c - 0.5 * ((b_act - loc0) / torch.exp(ls_c)) ** 2 + 0.3 * r(total, size)
            old = [(loc0 + 0.5 * r(total, size)).contiguous(), torch.clamp(ls0 + 0.5 * r(total, size), *LS_RANGE).contiguous()]
        b_val = (v0 + 0.3 * r(total)).contiguous()
    b_logp = b_logp.contiguous()
    kept = int(keep.sum())
    assert 3 * kept > 2 * total, (kept, total)
    rows = order[keep[order]][:mb].contiguous()
    assert rows.numel() == mb
    unused = torch.ones(total, dtype=torch.bool, device=dev)
    unused[rows] = False
    for t in [b_obs, b_adv, b_vt, b_val, b_logp] + old:
        t[unused] = float("nan")  # a read of a row the table does not name poisons the result
    act_rows = b_act[rows]
    lib_p = "srlx_ppo_cat_" if cat else "srlx_ppo_net_"
    n_partials = getattr(lib, lib_p + "kl_partials_floats")(obs, size)
    assert n_partials == 256 * ((P + 4 + 3) // 4 * 4) and getattr(lib, lib_p + "partials_floats")(obs, size) == 256 * ((P + 3 + 3) // 4 * 4)
    partials = torch.empty(n_partials, device=dev)

    def loss_parts(model, dt, base, vclip, beta):
        logp_, adv_, vt_, val_ = (t[rows].to(dt) for t in (b_logp, b_adv, b_vt, b_val))
        old_ = [t[rows].to(dt) for t in old]
        if cat:
            v, lg = model(b_obs[rows].to(dt))
            return K.torch_loss_categorical(torch, lg, act_rows, logp_, old_[0], adv_, v, vt_, val_, base, vclip, VC, VW, EW, beta)
        v, loc, ls = model(b_obs[rows].to(dt))
        return K.torch_loss_normal(torch, loc, ls, LS_RANGE, act_rows.to(dt), logp_, old_[0], old_[1], adv_, v, vt_, val_, base, vclip, VC, VW, EW, beta)

    def grads_of(model, dt, base, vclip, beta):
        model.zero_grad()
        parts = loss_parts(model, dt, base, vclip, beta)
        sum(parts[:3]).backward()
        return torch.stack([p.detach().double() for p in parts]), [(name, p.grad.reshape(-1).double().clone()) for name, p in model.named_parameters()]

    def yardstick(base, vclip, beta):
        want_l, want = grads_of(net64, torch.float64, base, vclip, beta)
        t32 = [float((g32 - w).abs().max()) for (_, g32), (_, w) in zip(grads_of(net, torch.float32, base, vclip, beta)[1], want)]
        return want_l, want, t32

    def launch(base, vclip, beta, target):
        partials.fill_(float("nan"))  # a reduce that reads a partial no workgroup wrote poisons the gradient
        grad, losses, beta_t = torch.full((P,), float("nan"), device=dev), torch.full((5,), float("nan"), device=dev), torch.full((1,), beta, device=dev)
        head = (N.tptr(old[0]),) if cat else (N.tptr(old[0]), N.tptr(old[1]), *LS_RANGE)
        fn = lib.srlx_ppo_cat_minibatch_kl if cat else lib.srlx_ppo_net_minibatch_kl
        N.check(fn(mb, N.tptr(rows), obs, size, N.tptr(flat), N.tptr(b_obs), N.tptr(b_act), N.tptr(b_logp), N.tptr(b_adv), N.tptr(b_vt), N.tptr(b_val), *head, base, vclip, VC, VW, EW,
                   target, N.tptr(beta_t), N.tptr(partials), N.tptr(grad), N.tptr(losses), None))
        torch.cuda.synchronize()
        return losses, float(beta_t.item()), grad

    return types.SimpleNamespace(launch=launch, yardstick=yardstick, P=P, kept=kept, total=total, torch=torch)


FUSED_GEOMETRIES = [(1, 4, 2), (1, 1, 8), (1, 8, 3), (0, 3, 1), (0, 8, 4)]


@pytest.mark.parametrize("mb", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("cat,obs,size", FUSED_GEOMETRIES, ids=lambda v: str(v))
def test_fused_kl_minibatch_against_float64_autograd(cat, obs, size, mb):
    """Every parameter tensor's gradient, the three losses and kl_mean at beta 0.5 and 8, baseline and value clip both on and both off; the target is the
    yardstick's kl_mean, so beta stays."""
    fx = _fused_fixture(cat, obs, size, mb)
    torch = fx.torch
    for beta in (0.5, 8.0):
        for base, vclip in ((1, 1), (0, 0)):
            want_l, want, t32 = fx.yardstick(base, vclip, beta)
            assert float(want_l[3]) >= 1e-3
            losses, beta_after, grad = fx.launch(base, vclip, beta, float(want_l[3]))
            off, pairs = 0, []
            for (name, w), t in zip(want, t32):
                pairs.append((name, grad[off : off + w.numel()], w, t))
                off += w.numel()
            assert off == fx.P
            _check(torch, "fused %s obs=%d size=%d mb=%d beta=%g switches=%d%d kept %d/%d" % ("categorical" if cat else "normal", obs, size, mb, beta, base, vclip, fx.kept, fx.total),
                   pairs, losses[:4], want_l)
            assert beta_after == beta and float(losses[4]) == beta


@pytest.mark.parametrize("cat,obs,size", [(1, 4, 2), (0, 3, 1)], ids=lambda v: str(v))
def test_beta_adapts_in_the_reduction_launch(cat, obs, size):
    """ppo.py:279-287 through srlx_ppo_*_minibatch_kl, the target set from the yardstick's float64 kl_mean: a factor 1.5 away from either threshold, so float32
    rounding of kl_mean does not choose the branch.  Exact equalities."""
    fx = _fused_fixture(cat, obs, size, 65)
    kl = float(fx.yardstick(1, 1, 0.5)[0][3])
    got = []
    for target, beta, want in ((2.25 * kl, 0.5, 0.25), (kl / 2.25, 0.5, 1.0), (kl / 2.25, 8.0, 16.0), (kl / 2.25, 16.0, 16.0), (kl, 0.5, 0.5)):
        losses, beta_after, _ = fx.launch(1, 1, beta, target)
        got.append((target / kl, beta, beta_after, float(losses[4]), want, K.adapt_beta(beta, kl, target)))
    print("PPO-KL beta adaptation (target / kl, beta, after, losses[4], want, reference):", got)
    for _, _, after, reported, want, ref in got:
        assert after == want == reported == ref


def test_beta_stops_halving_at_the_smallest_normal_float():
    """A float32 beta that went on halving would lose bits below 1.18e-38 and then reach 0, from which no doubling returns: the halving stops at FLT_MIN, through
    both entry points, and the doubling still works from there."""
    N, lib, torch, dev = TN._env()
    flt_min = float(np.finfo(np.float32).tiny)
    fx = _fused_fixture(1, 4, 2, 65)
    kl = float(fx.yardstick(1, 1, 0.5)[0][3])
    inp = _cat_inputs(torch, dev, 3, 67)
    for launch in (lambda beta, target: fx.launch(1, 1, beta, target)[1], lambda beta, target: _launch_cat(N, lib, torch, dev, 3, inp, 1, 1, beta, target)[1]):
        assert launch(2 * flt_min, 1e3) == flt_min  # the last exact halving
        assert launch(flt_min, 1e3) == flt_min      # ... and no further
        assert launch(flt_min, kl / 1e3) == 2 * flt_min


# ---- 4. the rollout ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("E", [16, 48])
@pytest.mark.parametrize("cat,size", [(0, 2), (1, 3)])
def test_kl_rollout_records_the_acting_distribution(cat, size, E, T):
    """k_ppo_rollout<Task, false, true> from the start state of the plain rollout: every output they share is the same bits, and the recorded distribution is what
    the step-wise path (network forward -> srlx_ppo_*_act_dist per step) records -- over two consecutive rollouts, episodes ending inside them (episode_len 3)."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=size) if cat else dict(action_dim=size)
    cfg = PPODeviceConfig(n_envs=E, horizon=T, seed=4, episode_len=3, surrogate_type="kl", **head)
    a, b, c = PPOEngine(cfg, 0), PPOEngine(dataclasses.replace(cfg, surrogate_type="clip"), 0), PPOEngine(cfg, 0)
    if cat:
        TD._give_the_logits_content(torch, a, b, c)
    assert a.fused and a._fused_rollout_ok() and b._fused_rollout_ok() and a.kl and not b.kl and b.old_dist is None
    c._fused_rollout_ok = lambda: False  # the step-wise path on the libsrlx network
    for t in a.old_dist + c.old_dist:
        t.fill_(float("nan"))
    for it in range(2):
        for e in (a, b, c):
            e.rollout()
        torch.cuda.synchronize()
        for other in (b, c):
            for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv", "episode_return", "_last_v"):
                assert torch.equal(getattr(a, name), getattr(other, name)), (it, name)
            assert torch.equal(a.env.state, other.env.state) and torch.equal(a.env.t, other.env.t) and torch.equal(a.env.obs, a.b_obs[T])
            assert torch.equal(a.env.episodes, other.env.episodes) if cat else int(a.env.counter.item()) == int(other.env.counter.item()) == T * (it + 1)
            assert int(a.act_counter.item()) == int(other.act_counter.item()) == T * (it + 1)
            assert float(a.finished_returns[1]) == float(other.finished_returns[1])
            torch.testing.assert_close(a.finished_returns, other.finished_returns, rtol=1e-5, atol=1e-3)  # (float atomics: order differs)
        for x, y in zip(a.old_dist, c.old_dist):
            assert x.shape == (T, E, size) and torch.equal(x, y) and bool(torch.isfinite(x).all()), it
        if cat:
            torch.testing.assert_close(a.old_dist[0].sum(-1), torch.ones(T, E, device=dev), rtol=1e-5, atol=1e-5)
            taken = a.old_dist[0].gather(2, a.b_act.long().unsqueeze(-1)).squeeze(-1)
            torch.testing.assert_close(taken, torch.exp(a.b_logp), rtol=1e-6, atol=0)  # (no log-probability of this policy is near the floor)
            assert float(a.old_dist[0].max() - a.old_dist[0].min()) > 0.05  # (not the uniform policy)
        else:
            assert float(a.old_dist[1].min()) >= a.ls_range[0] - 1e-6 and float(a.old_dist[1].max()) <= a.ls_range[1] + 1e-6
            assert not torch.equal(a.old_dist[0], a.b_act)
        for e in (a, b, c):
            e.b_obs[0].copy_(e.b_obs[T])
    print("PPO-KL rollout %s size=%d E=%d T=%d: shared outputs and the recorded distribution bit-equal over 2 rollouts, %d episode ends" % (
        "categorical" if cat else "normal", size, E, T, int(a.finished_returns[1])))


# ---- 5. the engine ----------------------------------------------------------------------------------------------------------------------------------------------------
def _record_betas(engine, store):
    """wraps the head's minibatch / loss entry so that beta is copied (on the device) after every minibatch update"""
    name = "minibatch" if engine.fused else "loss_and_seeds"
    inner = getattr(engine.head, name)

    def wrapped(*a, **k):
        out = inner(*a, **k)
        store.append(engine.kl_beta.clone())
        return out

    setattr(engine.head, name, wrapped)


@pytest.mark.parametrize("cat", [0, 1])
def test_engine_fused_against_autograd_under_kl(cat):
    """One whole iteration at E = 48, T = 4, two minibatches (96 samples each: a full tile and a partial one) of the fused engine against the torch-modules /
    autograd / torch.optim.Adam engine, with the comparison and bars of tests/test_ppo_net_gpu.py and tests/test_ppo_discrete_gpu.py; beta after each of the 8
    minibatch updates is the same number on both paths."""
    N, lib, torch, dev = TN._env()
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=2) if cat else {}
    cfg = PPODeviceConfig(n_envs=48, horizon=4, minibatches=2, seed=6, surrogate_type="kl", **head)
    a, b = PPOEngine(cfg, 0, fused=True), PPOEngine(cfg, 0, fused=False)
    if cat:
        TD._give_the_logits_content(torch, a, b)
    betas_a, betas_b = [], []
    _record_betas(a, betas_a)
    _record_betas(b, betas_b)
    a.rollout()
    b.rollout()
    torch.cuda.synchronize()
    if cat:
        lanes = (a.b_act == b.b_act).all(dim=0)
        assert float(lanes.float().mean()) >= 0.99
    else:
        lanes = torch.ones(48, dtype=torch.bool, device=dev)
        torch.testing.assert_close(a.b_act, b.b_act, rtol=2e-4, atol=2e-4)
    for name in ("b_logp", "b_val", "b_adv"):
        torch.testing.assert_close(getattr(a, name)[:, lanes], getattr(b, name)[:, lanes], rtol=2e-4, atol=2e-4, msg=lambda m: f"{name}: {m}")
    for x, y in zip(a.old_dist, b.old_dist):
        torch.testing.assert_close(x[:, lanes], y[:, lanes], rtol=2e-4, atol=2e-4)
    for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done", "b_adv"):  # the update on IDENTICAL buffers
        getattr(b, name).copy_(getattr(a, name))
    for x, y in zip(a.old_dist, b.old_dist):
        y.copy_(x)
    before = a.flat.clone()
    a.update()
    b.update()
    torch.cuda.synchronize()
    moved = float((a.flat - before).abs().max())
    flat_b = torch.cat([p.detach().reshape(-1) for p in b.net.parameters()])
    diff = (a.flat - flat_b).abs()
    seq_a, seq_b = [float(t) for t in betas_a], [float(t) for t in betas_b]
    print("PPO-KL engine %s: moved %.3g, diff max %.3g mean %.3g; losses fused %s torch %s; beta fused %s torch %s" % (
        "categorical" if cat else "normal", moved, float(diff.max()), float(diff.mean()), a.losses.tolist(), b.losses.tolist(), seq_a, seq_b))
    assert moved > 0.5 * 8 * cfg.lr  # 8 steps of about lr each
    assert float(diff.max()) < 0.03 * moved and float(diff.mean()) < 2e-4 * moved, (float(diff.max()), float(diff.mean()), moved)
    torch.testing.assert_close(a.losses, b.losses, rtol=1e-3, atol=1e-5)
    assert len(seq_a) == 8 and seq_a == seq_b and a.opt_step.tolist() == [8, 0]
    info = a.info()
    assert set(info) == {"policy_loss", "value_loss", "entropy_loss", "kl_mean", "kl_beta"} and info["kl_beta"] == seq_a[-1] and np.isfinite(list(info.values())).all()
    assert set(PPOEngine(dataclasses.replace(cfg, surrogate_type="clip"), 0).info()) == {"policy_loss", "value_loss", "entropy_loss"}


@pytest.mark.parametrize("env_name", ["CartPole-v1", "Pendulum-v1"])
def test_engine_exchanges_beta_with_the_plugin_and_refuses_data_parallel(env_name):
    N, lib, torch, dev = TN._env()
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo
    from simple_distributed_rl_amd.device import vector_runner as vr
    from simple_distributed_rl_amd.device.ppo import DistributedPPO, PPOEngine

    runner = srl.Runner(env_name, ppo.Config(surrogate_type="kl", adaptive_kl_target=0.03))
    runner.set_device("cuda:0")
    runner.setup_rl_config()
    d = vr.ppo_config_from(runner.rl_config, runner.env, 32, 5, horizon=4, minibatches=2, admit_kl=True)
    assert d.surrogate_type == "kl" and d.adaptive_kl_target == 0.03
    eng = PPOEngine(d, 0)
    assert eng.fused and eng.kl and float(eng.kl_beta.item()) == 0.5
    eng.step()
    eng.kl_beta.fill_(4.0)
    eng.export_to(runner.parameter)
    assert runner.parameter.adaptive_kl_beta == 4.0
    runner.parameter.adaptive_kl_beta = 0.125
    eng.load_from(runner.parameter)
    assert float(eng.kl_beta.item()) == 0.125
    with pytest.raises(ValueError, match="data-parallel"):
        DistributedPPO(d, 0)
    with pytest.raises(ValueError, match="data-parallel"):
        PPOEngine(d, 0, flat_grad_sync=lambda flat: 1.0)
    with pytest.raises(ValueError, match="data-parallel"):
        PPOEngine(d, 0, grad_sync=lambda net: None, fused=False)


# ---- 6. captured graphs follow beta -------------------------------------------------------------------------------------------------------------------------------------
GRAPH_TARGET, GRAPH_LR = 1e-3, 3e-3  # at this rate a minibatch update moves the policy by a KL around the target: beta moves in both directions


def _six_iterations(torch, cat, fused, graphs):
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig, PPOEngine

    head = dict(obs_dim=4, n_actions=2) if cat else {}
    eng = PPOEngine(PPODeviceConfig(n_envs=64, horizon=8, epochs=2, minibatches=2, seed=11, lr=GRAPH_LR, surrogate_type="kl", adaptive_kl_target=GRAPH_TARGET, **head), 0, fused=fused)
    betas = []
    for k in range(6):
        if k == 1 and graphs:
            eng.capture_graphs()  # (runs one whole iteration itself, as its warm-up)
        else:
            eng.step()
        torch.cuda.synchronize()
        betas.append(float(eng.kl_beta.item()))
    return eng, betas


@pytest.mark.parametrize("cat,fused", [(0, True), (1, True), (0, False)])
def test_captured_graphs_follow_beta(cat, fused):
    """Two engines, one seed: one eager, one replaying its captured rollout and update graphs from the second iteration on.  beta is device state that the update's
    own launches adapt, so nothing of it is baked into the graph: the beta sequences are the same numbers and the parameters the same bits
    (tests/test_ppo_config_gpu.py: test_the_schedule_survives_graph_capture).  On the fused path, and once on the torch path."""
    N, lib, torch, dev = TN._env()
    eager, be = _six_iterations(torch, cat, fused, False)
    graph, bg = _six_iterations(torch, cat, fused, True)
    assert graph._update_graph is not None and eager._update_graph is None
    changes = sum(1 for x, y in zip([0.5] + be, be) if x != y)
    pe, pg = (torch.cat([p.detach().reshape(-1) for p in e.net.parameters()]) for e in (eager, graph))
    print("PPO-KL graphs %s %s: beta eager %s graph %s; max |eager - graph| %.3g" % ("categorical" if cat else "normal", "fused" if fused else "torch", be, bg, float((pe - pg).abs().max())))
    assert changes >= 2, be
    assert be == bg
    assert torch.equal(pe, pg) and bool(torch.isfinite(pg).all())
    assert torch.equal(eager.losses, graph.losses)


# ---- 7. the plugin path -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["CartPole-v1", "Pendulum-v1"])
def test_plugin_trainer_runs_the_kl_surrogate(env_name):
    N, lib, torch, dev = TN._env()
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo

    rl = ppo.Config(surrogate_type="kl", batch_size=16, train_num=2, train_every_epoch=True)
    rl.memory.warmup_size = 48
    runner = srl.Runner(env_name, rl)
    runner.set_device("cuda:0")
    runner.train(max_train_count=4, enable_progress=False)
    trainer, parameter = runner.trainer, runner.parameter
    info = trainer.info
    print("PPO-KL plugin %s: train_count %d info %s beta %r" % (env_name, trainer.train_count, dict(info), parameter.adaptive_kl_beta))
    assert trainer.train_count >= 4
    assert all(k in info and math.isfinite(info[k]) for k in ("policy_loss", "value_loss", "entropy_loss", "kl_mean", "kl_beta"))
    assert parameter.adaptive_kl_beta == float(trainer.kl_beta.item()) == info["kl_beta"]
    assert parameter.adaptive_kl_beta in [0.5 * 2.0 ** k for k in range(-8, 6)]
    backup = parameter.call_backup(serialized=True)
    kept = parameter.adaptive_kl_beta
    parameter.adaptive_kl_beta = 123.0
    parameter.call_restore(backup)
    assert parameter.adaptive_kl_beta == kept
    from simple_distributed_rl_amd.base.exception import UndefinedError

    with pytest.raises(UndefinedError):
        bad = srl.Runner(env_name, ppo.Config(surrogate_type="klx"))
        bad.set_device("cuda:0")
        bad.train(max_train_count=1, enable_progress=False)
