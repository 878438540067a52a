"""Rainbow with NoisyLinear layers on flat observations on the device (libsrlx srlx_mlpq_bind_noisy and the noisy paths of srlx_mlpq_forward / _train_nstep /
_publish, csrc/srlx_mlpq.hip; device/mlpq.py:VectorQEngine with `enable_noisy_dense`) over the envelope shapes of tests/rainbow_noisy_reference.py, against its
float64 yardstick (pinned on the reference's recorded Trainer.train() by tests/test_rainbow_noisy_vector_cpu.py).  srlx_mlpq_noisy_draw / _noisy_eps tell a test
the noise of a step before it runs, so every comparison is against float64 arithmetic on mu + sigma * eps of the very draws the kernels use; parity with the
reference's own noise stream is statistical (the generator test).  Every test prints the error it measured ("RAINBOW-NOISY-ERR ...", shown with -s) before it
asserts."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rainbow_noisy_reference as M  # noqa: E402

ENVELOPE = M.ENVELOPE

pytestmark = pytest.mark.gpu

DISCOUNT = 0.99
D_ON, D_TG = 6, 11  # the draw ids the learner tests start from (online: D_ON = the s_1..s_n pass, D_ON + 1 = the s_0 pass; target: D_TG)


def _sid(i):
    D, ins, hid, H, A, dtype, n = ENVELOPE[i]
    return f"{D}-{'x'.join(str(w) for w in ins + hid) or 'none'}-{H}-{A}-{dtype or 'naive'}-n{n}"


def _per_group(n):
    return 16 // (n + 1)  # items one workgroup of the learner kernel takes


@functools.lru_cache(maxsize=None)
def _params(i):
    """((mu, sigma) online, (mu, sigma) target) in float64 (float32 values): the reference's initial sigma 0.5 / sqrt(in) times a factor in [0.5, 1.5] that
    differs in every element, so that a shifted or swapped eps shows."""
    D, ins, hid, H, A, _, _ = ENVELOPE[i]
    g = torch.Generator().manual_seed(i)
    out = []
    for seed in (3000 + i, 4000 + i):
        mu, sig = M.init_params(D, ins, hid, H, A, seed)
        sig = [None if s is None else (s.float() * (0.5 + torch.rand(s.shape, generator=g))).double() for s in sig]
        out.append((mu, sig))
    return tuple(out)


def _net(i, mu, sig, noisy=True):
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    D, ins, hid, H, A, dtype, _ = ENVELOPE[i]
    net = EngineMLPQNet(D, ins, hid, A, H, dtype, noisy=noisy).cuda()
    with torch.no_grad():
        for p, v in zip(net.kernel_parameters(), mu):
            p.copy_(v.float())
        for p, v in zip(net.kernel_sigmas(), sig):
            if p is not None:
                p.copy_(v.float())
    return net


def _handle(i, which, **kw):
    """A handle over fresh copies of the online (which = 0) or target (1) tensors of shape i; its noise key depends on the shape and the role only."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    mu, sig = _params(i)[which]
    net = _net(i, mu, sig)
    return net, MLPQHandle(net, kw.pop("max_rows", 16), noise_seed=(77 if which == 0 else 99) + 1000 * i, **kw)


def _eps(h, draw):
    out = [None if s is None else h.eps(draw, k) for k, s in enumerate(h.sigmas)]
    torch.cuda.synchronize()
    return [None if e is None else e.cpu() for e in out]


@functools.lru_cache(maxsize=None)
def _sets(i, d_on=D_ON, d_tg=D_TG):
    """(online effective set of the s_0 draw, of the s_1..s_n draw, target effective set, eps of the s_0 draw) in float64, for handles of `_handle`'s keys
    whose counters stand at d_on / d_tg."""
    (mu, sig), (mu_t, sig_t) = _params(i)
    _, h = _handle(i, 0)
    _, ht = _handle(i, 1)
    eps0 = _eps(h, d_on + 1)
    return M.effective(mu, sig, eps0), M.effective(mu, sig, _eps(h, d_on)), M.effective(mu_t, sig_t, _eps(ht, d_tg)), eps0


@functools.lru_cache(maxsize=None)
def _items(i, double_dqn, retrace_h, rescale):
    D, _, _, _, A, dtype, n = ENVELOPE[i]
    on0, on_next, tg, _ = _sets(i)
    return M.pick_items(on0, on_next, tg, D, A, n, dtype, DISCOUNT, retrace_h, double_dqn, rescale, 100 * i + 4 * int(double_dqn) + 2 * int(retrace_h == 1.0) + int(rescale))


def _batch(it, D, B):
    """The first B items on the device.  Only the rows these items use are placed, on the even row slots of a NaN-filled buffer in a shuffled order: a read of
    any other row poisons the result."""
    P = it.rows.shape[0]
    slot = torch.randperm(P, generator=torch.Generator().manual_seed(B)) * 2
    buf = torch.full((2 * P, D), float("nan"))
    used = it.idx[:B].reshape(-1).unique()
    buf[slot[used]] = it.rows[used].float()
    off = (slot[it.idx[:B]] * D).to(torch.int64).contiguous()
    return types.SimpleNamespace(obs=buf.cuda(), off=off.cuda(), act=it.act[:B].int().contiguous().cuda(), rew=it.rew[:B].float().contiguous().cuda(),
                                 term=it.term[:B].float().contiguous().cuda(), w=it.w[:B].float().cuda())


def _outputs(B, A):
    """q0, target, loss, priorities with one guard row past the batch."""
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    return f(B + 1, A), f(B + 1), f(1), f(B + 1)


def _step(h, ht, B, n, b, retrace_h, double_dqn, rescale, steps, out):
    h.train_nstep(ht, B, n, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, retrace_h, double_dqn, rescale, steps, *out)
    torch.cuda.synchronize()


def _grads(net):
    return [p.grad.detach().clone() for p in net.kernel_parameters()], [None if s is None else s.grad.detach().clone() for s in net.kernel_sigmas()]


def _live(ts):
    return [t for t in ts if t is not None]


# ---- 1. the generator -----------------------------------------------------------------------------------------------------------------------------------------
def test_generator_moments_and_independence():
    """srlx_mlpq_noisy_eps on the 512 x 512 tensors of the upper-bound shape (N = 262 144 elements; rainbow.Config()'s own shape has no 512 x 512 tensor: its
    largest is 2 x 512), over four draws, each bound five standard errors of its estimator: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N); the correlation
    between two consecutive draws of one tensor, between two tensors of one draw (the second trunk layer's weight and v_layers.0's), and between elements 2 j
    and 2 j + 1 (the two halves of one Box-Muller evaluation), each <= 5 / sqrt(N).  The same (seed, draw, tensor) gives the same bits twice; another seed,
    draw or tensor gives other bits."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i = 2
    (mu, sig), _ = _params(i)
    _, h = _handle(i, 0)
    N_el = 512 * 512
    assert h.params[2].numel() == N_el and h.params[4].numel() == N_el
    se = 1.0 / np.sqrt(N_el)
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])  # noqa: E731
    draws = [h.eps(d, 2).double().cpu().numpy().ravel() for d in (0, 1, 2, 1 << 40)]
    other = [h.eps(d, 4).double().cpu().numpy().ravel() for d in (0, 1, 2, 1 << 40)]
    for k, (e, o) in enumerate(zip(draws, other)):
        nxt = draws[(k + 1) % 4]
        figs = dict(mean=abs(e.mean()), var=abs(e.var() - 1.0), draws=abs(corr(e, nxt)), tensors=abs(corr(e, o)), halves=abs(corr(e[0::2], e[1::2])))
        print(f"RAINBOW-NOISY-ERR generator draw {k}: " + " ".join(f"{a}={b:.3e}" for a, b in figs.items()) + f" (5 se = {5 * se:.3e}, var bound {5 * np.sqrt(2) * se:.3e})")
        assert np.isfinite(e).all() and figs["mean"] <= 5 * se and figs["var"] <= 5 * np.sqrt(2.0) * se
        assert figs["draws"] <= 5 * se and figs["tensors"] <= 5 * se and figs["halves"] <= 5 * se
    assert torch.equal(h.eps(1, 2), h.eps(1, 2)) and np.array_equal(h.eps(1, 2).cpu().numpy().ravel(), draws[1].astype(np.float32))
    h2 = MLPQHandle(_net(i, mu, sig), 16, noise_seed=h.noise_seed + 1)
    assert not torch.equal(h.eps(1, 2), h2.eps(1, 2)) and not torch.equal(h.eps(1, 2), h.eps(1, 4)) and not torch.equal(h.eps(1, 2), h.eps(2, 2))
    # an odd-length tensor (A = 3 biases, shape 3): the last Box-Muller pair's second half is not written past the tensor's end
    _, h3 = _handle(3, 0)
    k = len(h3.params) - 1
    assert h3.params[k].numel() == 3 and bool(torch.isfinite(h3.eps(4, k)).all())
    with pytest.raises(N.SrlxError, match="not a noisy tensor"):  # (shape 4's first layer is the plain input value block's)
        _handle(4, 0)[1].eps(0, 0)


# ---- 2. forward -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ENVELOPE)), ids=_sid)
def test_forward_draws_fresh_noise_per_call(i):
    """With the next draw set to d, 1, 16, 17 and 250 rows: Q within 1e-5 * max |Q| of the float64 forward pass on mu + sigma * eps(d); the counter reads d + 1
    afterwards; a second call on the same rows gives other Q; with the draw set back to d the first call's bits return; the fused actions at eps = 0 are the first
    arg-max of the launch's own Q rows."""
    D, _, _, _, A, dtype, _ = ENVELOPE[i]
    (mu, sig), _ = _params(i)
    _, h = _handle(i, 0, max_rows=256)
    g = torch.Generator().manual_seed(i)
    worst = 0.0
    assert h.next_draw() == 0
    for rows in (1, 16, 17, 250):
        d = 3 + rows
        x = torch.randn(rows, D, generator=g)
        xd = x.cuda()
        q, q2, q3 = (torch.zeros(rows, A, device="cuda") for _ in range(3))
        acts = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        zero = torch.zeros(rows, device="cuda")
        counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        h.set_next_draw(d)
        h.forward(rows, xd, q=q, eps=zero, seed=11, counter=counter, actions=acts)
        assert h.next_draw() == d + 1
        h.forward(rows, xd, q=q2)
        assert h.next_draw() == d + 2
        h.set_next_draw(d)
        h.forward(rows, xd, q=q3)
        torch.cuda.synchronize()
        want = M.forward(M.effective(mu, sig, _eps(h, d)), x.double(), dtype)
        err = float((q.double().cpu() - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (rows, err)
        assert not torch.equal(q2, q) and torch.equal(q3, q), rows
        assert torch.equal(acts.long(), q.argmax(1)), rows  # (torch's arg-max returns the first maximum; ties do not occur on these rows)
        assert bool((q.topk(2, dim=1).values.diff(dim=1) != 0).all())
    print(f"RAINBOW-NOISY-ERR forward {_sid(i)} worst_rel={worst:.3e}")


# ---- 3. the learner step --------------------------------------------------------------------------------------------------------------------------------------
def _batch_sizes(n):
    P = _per_group(n)
    return sorted({1, P, P + 1, 256})


LEARN_CASES = [(i, dd, 1.0, False) for i in range(len(ENVELOPE)) for dd in (True, False)] + [(3, True, 0.5, False), (5, True, 1.0, True)]


@pytest.mark.parametrize("i, double_dqn, retrace_h, rescale", LEARN_CASES,
                         ids=[f"{_sid(i)}-{'double' if dd else 'single'}-h{h}-{'rescale' if rs else 'plain'}" for i, dd, h, rs in LEARN_CASES])
def test_learner_step_matches_float64_reference(i, double_dqn, retrace_h, rescale):
    """One srlx_mlpq_train_nstep (gradients only) on noisy handles whose counters stand at known ids, on the first B items of pick_items, B = 1, P, P + 1 (P = the
    items of one workgroup at this n) and 256, against rainbow_noisy_reference.learner_step on the three effective sets of those ids: Q of s_0, target and
    priorities at rtol 1e-5 / atol 1e-6, the loss at rel 1e-5, every mu and sigma gradient at rtol 1e-5 with an absolute slack of 1e-5 * max |g| of the tensor.
    Nothing is written past row B of the outputs; the online counter advances by 2 and the target's by 1; at B = P + 1 a second run from the same ids gives the
    same bits."""
    D, _, _, _, A, dtype, n = ENVELOPE[i]
    (mu, sig), _ = _params(i)
    _, eff_next, eff_tg, eps0 = _sets(i)
    it = _items(i, double_dqn, retrace_h, rescale)
    _, ht = _handle(i, 1)
    for B in _batch_sizes(n):
        net, h = _handle(i, 0, max_batch=B, max_nstep=n)
        h.set_next_draw(D_ON), ht.set_next_draw(D_TG)
        b = _batch(it, D, B)
        q0, target, loss, pri = out = _outputs(B, A)
        _step(h, ht, B, n, b, retrace_h, double_dqn, rescale, None, out)
        assert (h.next_draw(), ht.next_draw()) == (D_ON + 2, D_TG + 1)
        ref = M.learner_step(mu, sig, eps0, eff_next, eff_tg, it.rows[it.idx[:B]], it.act[:B], it.rew[:B], it.term[:B], it.w[:B], DISCOUNT, retrace_h, double_dqn,
                             rescale, dtype)
        gm, gs = _grads(net)
        got, want = gm + _live(gs), ref.grads + _live(ref.sigma_grads)
        gerr = max(float((gk.double().cpu() - gr).abs().max()) / float(gr.abs().max()) for gk, gr in zip(got, want))
        print(f"RAINBOW-NOISY-ERR learner {_sid(i)} B={B} dd={int(double_dqn)} h={retrace_h} rs={int(rescale)} "
              f"q0={float((q0[:B].double().cpu() - ref.q0).abs().max()):.3e} target={float((target[:B].double().cpu() - ref.target).abs().max()):.3e} "
              f"loss_rel={abs(float(loss) - ref.loss) / ref.loss:.3e} grad_rel={gerr:.3e}")
        assert float(q0[B].min()) == 7.0 and float(q0[B].max()) == 7.0 and float(target[B]) == 7.0 and float(pri[B]) == 7.0
        np.testing.assert_allclose(q0[:B].double().cpu(), ref.q0, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(target[:B].double().cpu(), ref.target, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(pri[:B].double().cpu(), ref.priorities, rtol=1e-5, atol=1e-6)
        assert float(loss) == pytest.approx(ref.loss, rel=1e-5)
        for k, (gk, gr) in enumerate(zip(got, want)):
            np.testing.assert_allclose(gk.double().cpu(), gr, rtol=1e-5, atol=1e-5 * float(gr.abs().max()) + 1e-12, err_msg=f"B={B} tensor {k} of mu + sigma")
        if B == _per_group(n) + 1:
            net2, h2 = _handle(i, 0, max_batch=256, max_nstep=7)
            h2.set_next_draw(D_ON), ht.set_next_draw(D_TG)
            out2 = _outputs(B, A)
            _step(h2, ht, B, n, b, retrace_h, double_dqn, rescale, None, out2)
            gm2, gs2 = _grads(net2)
            assert all(torch.equal(a, c) for a, c in zip(list(out) + gm + _live(gs), list(out2) + gm2 + _live(gs2)))


# ---- 4. sigma = 0 is the plain handle -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 3, 4], ids=_sid)
def test_zero_sigma_is_bit_equal_to_the_plain_dueling_handle(i):
    """A noisy handle with every sigma 0 and a plain dueling handle on the same mu, the same batch at B = P + 1 and B = 256 with one Adam step: Q of s_0, target,
    loss, priorities, every mu gradient and every post-Adam mu are the same bits; the sigma gradients equal g_mu * eps of the s_0 draw (float32 product)."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, _, A, dtype, n = ENVELOPE[i]
    (mu, sig), (mu_t, sig_t) = _params(i)
    zeros = lambda ss: [None if s is None else torch.zeros_like(s) for s in ss]  # noqa: E731
    it = M.pick_items(mu, mu, mu_t, D, A, n, dtype, DISCOUNT, 1.0, True, False, 900 + i)
    for B in (_per_group(n) + 1, 256):
        b = _batch(it, D, B)
        got = []
        for noisy in (True, False):
            net, tgt = _net(i, mu, zeros(sig), noisy), _net(i, mu_t, zeros(sig_t), noisy)
            h, ht = MLPQHandle(net, 16, max_batch=B, lr=1e-3, max_nstep=n, noise_seed=5), MLPQHandle(tgt, 16, noise_seed=6)
            if noisy:
                h.set_next_draw(D_ON)
            out = _outputs(B, A)
            steps = torch.zeros(1, dtype=torch.int64, device="cuda")
            _step(h, ht, B, n, b, 1.0, True, False, steps, out)
            gm, gs = _grads(net)
            got.append(list(out) + gm + [p.detach().clone() for p in net.kernel_parameters()] + h.exp_avg + h.exp_avg_sq)
            if noisy:
                assert all(bool((t == 0).all()) for t in _live(tgt.kernel_sigmas()))
                for k, s in enumerate(gs):
                    if s is not None:
                        assert torch.equal(s, gm[k] * h.eps(D_ON + 1, k)), (B, k)
                        assert float(s.abs().max()) > 0
        assert not torch.equal(got[0][0], torch.full_like(got[0][0], 7.0))
        assert all(torch.equal(a, c) for a, c in zip(*got)), B


# ---- 5. Adam --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [3, 4], ids=_sid)
def test_adam_over_six_steps(i):
    """Six consecutive updates (B = 100, steps_taken 0..5 in a device tensor) on fresh pick_items batches, the draw ids running on from D_ON / D_TG.  After every
    step mu and sigma equal torch.optim.Adam (float32) stepping on the kernel's own gradients (rtol 1e-6, atol 1e-7) and the float64 Adam (rtol 1e-5, atol
    1e-7).  The same inputs with write_grads=False (Adam only): mu, sigma, exp_avg and exp_avg_sq of both bit-identical."""
    D, _, _, _, A, dtype, n = ENVELOPE[i]
    B, lr, n_steps = 100, 1e-3, 6
    (mu, sig), (mu_t, sig_t) = _params(i)
    _, ht = _handle(i, 1)
    net, h = _handle(i, 0, max_batch=B, lr=lr, max_nstep=n)
    h.set_next_draw(D_ON), ht.set_next_draw(D_TG)
    tensors = lambda nt: nt.kernel_parameters() + _live(nt.kernel_sigmas())  # noqa: E731

    start = mu + _live(sig)
    shadow = [v.float().cuda().requires_grad_(True) for v in start]
    opt = torch.optim.Adam(shadow, lr=lr)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    batches, grads_per_step = [], []
    worst32 = worst64 = 0.0
    for k in range(n_steps):
        cur_mu = [p.detach().double().cpu() for p in net.kernel_parameters()]
        cur_sig = [None if s is None else s.detach().double().cpu() for s in net.kernel_sigmas()]
        on0 = M.effective(cur_mu, cur_sig, _eps(h, D_ON + 2 * k + 1))
        on_next = M.effective(cur_mu, cur_sig, _eps(h, D_ON + 2 * k))
        tg = M.effective(mu_t, sig_t, _eps(ht, D_TG + k))
        batches.append(_batch(M.pick_items(on0, on_next, tg, D, A, n, dtype, DISCOUNT, 1.0, True, False, 500 + 10 * i + k), D, B))
        assert int(steps) == k and (h.next_draw(), ht.next_draw()) == (D_ON + 2 * k, D_TG + k)
        _step(h, ht, B, n, batches[k], 1.0, True, False, steps, _outputs(B, A))
        steps += 1
        gm, gs = _grads(net)
        grads_per_step.append(gm + _live(gs))
        for s, gk in zip(shadow, grads_per_step[k]):
            s.grad = gk.clone()
        opt.step()
        want64 = M.adam_steps(start, [[g.cpu() for g in gs_] for gs_ in grads_per_step], lr)[0][k]
        for p, s, w64 in zip(tensors(net), shadow, want64):
            worst32 = max(worst32, float((p.detach() - s.detach()).abs().max()))
            worst64 = max(worst64, float((p.detach().double().cpu() - w64).abs().max()))
            np.testing.assert_allclose(p.detach().cpu(), s.detach().cpu(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
            np.testing.assert_allclose(p.detach().double().cpu(), w64, rtol=1e-5, atol=1e-7, err_msg=f"step {k}")
    print(f"RAINBOW-NOISY-ERR adam {_sid(i)} steps={n_steps} max_abs_vs_torch_f32={worst32:.3e} max_abs_vs_f64={worst64:.3e}")
    assert not any(torch.equal(s.detach().double().cpu(), v) for s, v in zip(_live(net.kernel_sigmas()), _live(sig)))  # the sigmas moved
    net2, h2 = _handle(i, 0, max_batch=B, lr=lr, write_grads=False, max_nstep=n)
    h2.set_next_draw(D_ON), ht.set_next_draw(D_TG)
    steps.zero_()
    for k in range(n_steps):
        _step(h2, ht, B, n, batches[k], 1.0, True, False, steps, _outputs(B, A))
        steps += 1
    assert all(torch.equal(a, c) for a, c in zip(tensors(net), tensors(net2)))
    for a, c in ((h.exp_avg, h2.exp_avg), (h.exp_avg_sq, h2.exp_avg_sq), (_live(h.exp_avg_sigma), _live(h2.exp_avg_sigma)),
                 (_live(h.exp_avg_sq_sigma), _live(h2.exp_avg_sq_sigma))):
        assert all(torch.equal(x, y) for x, y in zip(a, c))


# ---- 6. publish, 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_publish_copies_every_mu_and_sigma():
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    for i in (2, 4):  # 12 + 12 tensors; a plain layer in front
        (mu, sig), (mu_t, sig_t) = _params(i)
        src, hs = _handle(i, 0)
        dst, hd = _handle(i, 1)
        both = lambda nt: nt.kernel_parameters() + _live(nt.kernel_sigmas())  # noqa: E731
        assert not any(torch.equal(a, c) for a, c in zip(both(src), both(dst)))
        hs.publish_to(hd)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(both(src), both(dst)))
        assert all(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(both(src), mu + _live(sig)))
        plain = MLPQHandle(_net(i, mu_t, sig_t, noisy=False), 16)
        before = [p.detach().clone() for p in plain.params]
        for a, c in ((hs, plain), (plain, hs)):
            with pytest.raises(N.SrlxError, match="mlpq_publish: a noisy source needs a noisy destination"):
                a.publish_to(c)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(before, plain.params)) and all(torch.equal(a, c) for a, c in zip(both(src), both(dst)))


def test_refusals_give_a_message_and_launch_nothing():
    """A noisy bind on a plain handle, a head layer without sigmas, a noisy trunk layer in front of a plain one, noisy / plain handles mixed in train_nstep,
    srlx_mlpq_train_step on a noisy handle, training with neither sigma gradients nor sigma Adam state: an error with its message; outputs preset to a sentinel
    and the gradients keep what they held."""
    import ctypes

    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    lib = N.lib()
    i, B = 4, 4
    D, ins, hid, H, A, dtype, n = ENVELOPE[i]
    (mu, sig), (mu_t, sig_t) = _params(i)
    table = lambda ts: ctypes.cast((N.c_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]), N.c_p)  # noqa: E731
    plain_dqn = MLPQHandle(EngineMLPQNet(D, (), (32,), A).cuda(), 16)
    some = [torch.zeros(4, device="cuda")] * 4
    with pytest.raises(N.SrlxError, match="no NoisyLinear form"):
        N.check(lib.srlx_mlpq_bind_noisy(plain_dqn.h, table(some), 0))
    net = _net(i, mu, sig)
    s = net.kernel_sigmas()
    assert s[0] is None and s[2] is not None and len(s) == 12
    bare = MLPQHandle(_net(i, mu, sig, noisy=False), 16)
    with pytest.raises(N.SrlxError, match="head layer 1 has no sigma"):
        N.check(lib.srlx_mlpq_bind_noisy(bare.h, table(s[:6] + [None, None] + s[8:]), 0))
    with pytest.raises(N.SrlxError, match="one of its two sigma"):
        N.check(lib.srlx_mlpq_bind_noisy(bare.h, table(s[:5] + [None] + s[6:]), 0))
    with pytest.raises(N.SrlxError, match="plain trunk layer 1 behind a noisy one"):
        N.check(lib.srlx_mlpq_bind_noisy(bare.h, table([s[2], s[3], None, None] + s[4:]), 0))
    with pytest.raises(N.SrlxError, match="not a noisy handle"):
        bare.next_draw()
    # training
    h = MLPQHandle(net, 16, max_batch=B, max_nstep=n, noise_seed=1)
    ht = MLPQHandle(_net(i, mu_t, sig_t), 16, noise_seed=2)
    ht_plain = MLPQHandle(_net(i, mu_t, sig_t, noisy=False), 16)
    net_p = _net(i, mu, sig, noisy=False)
    h_plain = MLPQHandle(net_p, 16, max_batch=B, max_nstep=n)
    on0, on_next, tg, _ = _sets(i)
    b = _batch(_items(i, True, 1.0, False), D, B)
    for t in net.kernel_parameters() + _live(net.kernel_sigmas()) + net_p.kernel_parameters():
        t.grad.fill_(3.0)
    out = _outputs(B, A)
    args = (B, n, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, 1.0, True, False, None)
    with pytest.raises(N.SrlxError, match="a noisy online handle needs a noisy target"):
        h.train_nstep(ht_plain, *args, *out)
    with pytest.raises(N.SrlxError, match="a noisy online handle needs a noisy target"):
        h_plain.train_nstep(ht, *args, *out)
    with pytest.raises(N.SrlxError, match="a noisy handle trains through srlx_mlpq_train_nstep"):
        h.train_step(ht, B, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, True, False, None, *out)
    N.check(lib.srlx_mlpq_bind_noisy_grads(h.h, None))
    with pytest.raises(N.SrlxError, match="neither sigma gradients nor sigma Adam state"):
        h.train_nstep(ht, *args, *out)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)
    assert all(bool((t.grad == 3.0).all()) for t in net.kernel_parameters() + _live(net.kernel_sigmas()) + net_p.kernel_parameters())
    assert (h.next_draw(), ht.next_draw()) == (0, 0)
    N.check(lib.srlx_mlpq_bind_noisy_grads(h.h, h._sgtab))
    h.train_nstep(ht, *args, *out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0][:B]).all()) and not bool((out[0][:B] == 7.0).any()) and (h.next_draw(), ht.next_draw()) == (2, 1)


# ---- 8. the engine, 9. the hand-over --------------------------------------------------------------------------------------------------------------------------
def _noisy_cfg(**kw):
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    base = dict(batch_size=32, lr=1e-3, target_model_update_interval=10, memory_capacity=64 * 20, memory_warmup_size=256, hidden_sizes=(), dueling_units=64,
                multisteps=3, n_envs=64, seed=4, epsilon=0.1, memory_alpha=0.6, enable_noisy_dense=True)
    base.update(kw)
    return VectorQConfig(**base)


def test_two_noisy_engines_with_one_seed_are_bit_identical():
    """30 lock-steps of a noisy dueling n = 3 engine on the device CartPole, the last ten updates replayed from the captured graph.  Two engines with one seed end
    with the same bits; every lane's epsilon is 0; across two consecutive replays the online counter advances by 2 each (the target's by 1) and the parameters
    change: the graph did not bake a draw id in.  The acting pass consumes one draw per lock-step."""
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    out = []
    for _ in range(2):
        eng = VectorQEngine(_noisy_cfg(), 0)
        assert eng.q_online.noisy and eng.q_target.noisy and bool((eng.eps == 0).all())
        assert eng.inf_online.noise_seed != eng.inf_target.noise_seed
        for _ in range(20):
            eng.step(learner_updates=1)
        eng.capture_graphs(warm_actor=False)
        for _ in range(8):
            eng.step(learner_updates=1)
        seen = []
        for _ in range(2):
            d0, t0 = eng.inf_online.next_draw(), eng.inf_target.next_draw()
            p0 = [p.detach().clone() for p in eng.q_online.kernel_parameters() + eng.q_online.kernel_sigmas()]
            eng.actor_step()
            assert eng.inf_online.next_draw() == d0 + 1
            assert eng._learner_graph is not None and eng.learner_step()
            assert (eng.inf_online.next_draw(), eng.inf_target.next_draw()) == (d0 + 3, t0 + 1)
            assert not any(torch.equal(a, c) for a, c in zip(p0, eng.q_online.kernel_parameters() + eng.q_online.kernel_sigmas()))
            seen.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert eng.train_count >= 20 and eng.nstep and not torch.equal(seen[0], seen[1])
        out.append(([p.detach().clone() for p in eng.q_online.kernel_parameters() + eng.q_online.kernel_sigmas()], eng.priorities.clone(), eng.loss.clone(),
                    eng.info()["loss"]))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2]) and np.isfinite(out[0][3])


def test_trained_noisy_engine_hands_its_networks_to_the_rainbow_plugin():
    """A rainbow.Config(enable_noisy_dense=True) engine trains on the device CartPole for a few dozen updates; `store_q_weights` puts its networks into the
    plugin's Parameter: every key present, mu and sigma finite, the sigmas moved from their initial value; `Runner.evaluate()` plays on the plugin path; the
    Parameter's tensors go back into a fresh engine unchanged."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import rainbow
    from simple_distributed_rl_amd.device import vector_runner as vr
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    rl = rainbow.Config(enable_noisy_dense=True)
    rl.memory.capacity, rl.memory.warmup_size = 64 * 30, 256
    runner = srl.Runner("CartPole-v1", rl)
    runner.set_device("cuda:0")
    runner.setup_rl_config()
    assert vr.why_not_flat_rainbow(runner.env, runner.rl_config, admit_noisy=True) == ""
    cfg = vr.mlp_config_from(runner.rl_config, runner.env, 64, 1)
    assert (cfg.dueling_units, cfg.multisteps, cfg.hidden_sizes, cfg.enable_noisy_dense) == (512, 3, (), True)
    eng = VectorQEngine(cfg, 0)
    initial = {k: v.clone() for k, v in eng.q_online.reference_state_dict().items()}
    assert list(initial) == list(runner.parameter.q_online.state_dict())
    for _ in range(40):
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    assert eng.train_count >= 30 and np.isfinite(eng.info()["loss"])
    vr.store_q_weights(eng, runner.parameter)
    for theirs, mine in ((runner.parameter.q_online, eng.q_online), (runner.parameter.q_target, eng.q_target)):
        sd = theirs.state_dict()
        assert list(sd) == list(initial)
        for k, v in mine.reference_state_dict().items():
            assert torch.equal(sd[k].cpu(), v.cpu()) and bool(torch.isfinite(v).all()), k
    moved = [k for k, v in runner.parameter.q_online.state_dict().items() if "sigma" in k and not torch.equal(v.cpu(), initial[k].cpu())]
    assert moved == [k for k in initial if "sigma" in k], moved
    rewards = runner.evaluate(max_episodes=3, enable_progress=False)
    assert len(rewards) == 3 and np.all(np.isfinite(rewards)) and min(rewards) >= 1
    fresh = VectorQEngine(cfg, 0)
    vr.load_q_weights(fresh, runner.parameter)
    for a, c in ((fresh.q_online, eng.q_online), (fresh.q_target, eng.q_target)):
        assert all(torch.equal(x, y) for x, y in zip(a.kernel_parameters() + a.kernel_sigmas(), c.kernel_parameters() + c.kernel_sigmas()))
