"""The MLP Q-network kernels (libsrlx srlx_mlpq_*, csrc/srlx_mlpq.hip) over the envelope srlx_mlpq_create admits -- observation length 1..256, 1..3 ReLU layers
of 32..512 units, 2..32 actions, learner batches 1..256 -- against the float64 yardstick of tests/mlpq_reference.py (pinned on the reference's recorded
Trainer.train() by tests/test_dqn_vector_cpu.py): the forward pass, the whole learner step (target, Q, loss, priorities, every gradient), Adam over several
steps, the online -> target copy and the argument checks.  Every test prints the error it measured ("MLPQ-ERR ...", shown with -s) before it asserts."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpq_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

DISCOUNT = 0.99
# (D, in_sizes, hidden_sizes, A): the input value block's layers, then the hidden block's
ENVELOPE = [
    (1, (), (32,), 2),  # every lower bound; weight row stride 2
    (3, (), (32, 64, 96), 3),  # three layers, all widths different, rising; odd D and A
    (255, (), (512, 512, 512), 31),  # largest LDS footprint (S = 513); 15-unit tiles with a 2-unit tail; three layers, so kMaxParams is full
    (256, (), (512, 32, 512), 32),  # every upper bound; In = 256: 31-unit tiles; In = 32: 248-unit tiles with a 16-unit tail; widths fall then rise
    (17, (), (480,), 5),  # a width that is a multiple of 32 but not of 64; one layer
    (4, (), (32, 512), 2),  # a second layer wider than the first
    (17, (), (96, 32), 5),  # a second layer narrower than the first
    (128, (), (256, 256), 18),  # mid-range; the image engine's action count
    (8, (64,), (96, 32), 4),  # a non-empty input block in EngineMLPQNet: three kernel layers from two config blocks
]
ALL_B = (1, 7, 8, 9, 100, 256)  # one item; one short of / exactly / one over a workgroup's 8 items; a partial last workgroup; the largest batch
FULL_B = (0, 1, 2, 3)  # ENVELOPE rows that run every batch size; the others run (9, 256)
LEARN_CASES = [(i, B) for i in range(len(ENVELOPE)) for B in (ALL_B if i in FULL_B else (9, 256))]


def _sid(i):
    D, ins, hid, A = ENVELOPE[i]
    return f"{D}-{'x'.join(str(w) for w in ins + hid)}-{A}"


@functools.lru_cache(maxsize=None)
def _params(i):
    """The float64 online and target parameters of ENVELOPE[i] (float32 values)."""
    D, ins, hid, A = ENVELOPE[i]
    return R.init_params(D, ins + hid, A, 1000 + i), R.init_params(D, ins + hid, A, 2000 + i)


@functools.lru_cache(maxsize=None)
def _items(i, double_dqn, rescale, extra=0):
    D, _, _, A = ENVELOPE[i]
    on, tg = _params(i)
    return R.pick_items(on, tg, D, A, DISCOUNT, double_dqn, rescale, 100 * extra + 10 * i + 2 * int(double_dqn) + int(rescale))


def _net(i, params):
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    D, ins, hid, A = ENVELOPE[i]
    net = EngineMLPQNet(D, ins, hid, A).cuda()
    with torch.no_grad():
        for p, v in zip(net.kernel_parameters(), params):
            p.copy_(v.float())
    return net


def _batch(it, D, B):
    """The first B items on the device.  Only the rows these items use are placed, on the even row slots of a NaN-filled buffer of 4 * 320 rows in a shuffled
    order: s_1 of an item is never the row after its s_0, items share rows where pick_items chained them, and a read of any other row poisons the result."""
    P = it.rows.shape[0]
    slot = torch.randperm(P, generator=torch.Generator().manual_seed(B)) * 2
    buf = torch.full((2 * P, D), float("nan"))
    used = torch.cat([it.i0[:B], it.i1[:B]]).unique()
    buf[slot[used]] = it.rows[used].float()
    off = torch.stack([slot[it.i0[:B]] * D, slot[it.i1[:B]] * D], 1).to(torch.int64)
    return types.SimpleNamespace(obs=buf.cuda(), off=off.cuda(), act=it.act[:B].int().view(B, 1).cuda(), rew=it.rew[:B].float().view(B, 1).cuda(),
                                 term=it.term[:B].float().view(B, 1).cuda(), w=it.w[:B].float().cuda())


def _outputs(B, A):
    """q0, target, loss, priorities with one guard row past the batch."""
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    return f(B + 1, A), f(B + 1), f(1), f(B + 1)


def _step(h, ht, B, b, double_dqn, rescale, steps, out):
    h.train_step(ht, B, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, double_dqn, rescale, steps, *out)
    torch.cuda.synchronize()


def _grads(net):
    return [p.grad.detach().clone() for p in net.kernel_parameters()]


@pytest.mark.parametrize("i", range(len(ENVELOPE)), ids=_sid)
def test_forward_matches_float64(i):
    """Q rows within 1e-5 * max |Q| of float64 at 1, 15, 16, 17 (a workgroup's 16 rows and its neighbours), 250 and 4096 rows; the same rows through a shuffled
    offset table are bit-equal."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A = ENVELOPE[i]
    on, _ = _params(i)
    h = MLPQHandle(_net(i, on), 4096)
    g = torch.Generator().manual_seed(i)
    worst = 0.0
    for rows in (1, 15, 16, 17, 250, 4096):
        x = torch.randn(rows, D, generator=g)
        xd = x.cuda()
        q = torch.zeros(rows, A, device="cuda")
        h.forward(rows, xd, q=q)
        perm = torch.randperm(rows, generator=g).cuda()
        q2 = torch.zeros(rows, A, device="cuda")
        h.forward(rows, xd.data_ptr(), offsets=(perm * D).to(torch.int64), q=q2)
        torch.cuda.synchronize()
        want = R.forward(on, x.double())
        err = float((q.double().cpu() - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (rows, err)
        assert torch.equal(q2, q[perm]), rows
    print(f"MLPQ-ERR forward {_sid(i)} worst_rel={worst:.3e}")


def test_fused_policy_takes_the_first_of_tied_maxima():
    """Epsilon 0 at A = 32 with two identical out_layer units: their Q values tie on every row, and where they are the row's maximum the action is the first
    of the two, as np.argmax gives it."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i, E = 3, 4096
    D, _, _, A = ENVELOPE[i]
    net = _net(i, _params(i)[0])
    with torch.no_grad():
        net.out_layer.weight[19].copy_(net.out_layer.weight[7])
        net.out_layer.bias[19] = net.out_layer.bias[7]
    h = MLPQHandle(net, E)
    x = torch.randn(E, D, generator=torch.Generator().manual_seed(5)).cuda()
    q = torch.zeros(E, A, device="cuda")
    acts = torch.full((E,), -1, dtype=torch.int32, device="cuda")
    h.forward(E, x, q=q, eps=torch.zeros(E, device="cuda"), seed=3, counter=torch.zeros(1, dtype=torch.int64, device="cuda"), actions=acts)
    torch.cuda.synchronize()
    qn = q.cpu().numpy()
    tied = (qn[:, 7] == qn[:, 19]) & (qn[:, 7] == qn.max(1))
    assert tied.sum() >= 16, tied.sum()
    np.testing.assert_array_equal(acts.cpu().numpy(), qn.argmax(1))
    assert (acts.cpu().numpy()[tied] == 7).all()


@pytest.mark.parametrize("rescale", [False, True], ids=["plain", "rescale"])
@pytest.mark.parametrize("double_dqn", [True, False], ids=["double", "single"])
@pytest.mark.parametrize("i, B", LEARN_CASES, ids=[f"{_sid(i)}-B{B}" for i, B in LEARN_CASES])
def test_learner_step_matches_float64_reference(i, B, double_dqn, rescale):
    """One srlx_mlpq_train_step (gradients only) on the first B items of pick_items against mlpq_reference.learner_step: Q of s_0, target and priorities at
    rtol 1e-5 / atol 1e-6, the loss at rel 1e-5, every gradient at rtol 1e-5 with an absolute slack of 1e-5 * max |g| of the tensor.  Nothing is written past
    row B of the outputs."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A = ENVELOPE[i]
    on, tg = _params(i)
    it = _items(i, double_dqn, rescale)
    net = _net(i, on)
    h, ht = MLPQHandle(net, 16, max_batch=B), MLPQHandle(_net(i, tg), 16)
    b = _batch(it, D, B)
    q0, target, loss, pri = out = _outputs(B, A)
    _step(h, ht, B, b, double_dqn, rescale, None, out)
    ref = R.learner_step(on, tg, it.rows[it.i0[:B]], it.rows[it.i1[:B]], it.act[:B], it.rew[:B], it.term[:B], it.w[:B], DISCOUNT, double_dqn, rescale)
    grads = _grads(net)
    gerr = max(float((gk.double().cpu() - gr).abs().max()) / float(gr.abs().max()) for gk, gr in zip(grads, ref.grads))
    print(f"MLPQ-ERR learner {_sid(i)} B={B} dd={int(double_dqn)} rs={int(rescale)} q0={float((q0[:B].double().cpu() - ref.q0).abs().max()):.3e} "
          f"target={float((target[:B].double().cpu() - ref.target).abs().max()):.3e} loss_rel={abs(float(loss) - ref.loss) / ref.loss:.3e} grad_rel={gerr:.3e}")
    assert float(q0[B].min()) == 7.0 and float(q0[B].max()) == 7.0 and float(target[B]) == 7.0 and float(pri[B]) == 7.0
    np.testing.assert_allclose(q0[:B].double().cpu(), ref.q0, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(target[:B].double().cpu(), ref.target, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pri[:B].double().cpu(), ref.priorities, rtol=1e-5, atol=1e-6)
    assert float(loss) == pytest.approx(ref.loss, rel=1e-5)
    for k, (gk, gr) in enumerate(zip(grads, ref.grads)):
        np.testing.assert_allclose(gk.double().cpu(), gr, rtol=1e-5, atol=1e-5 * float(gr.abs().max()) + 1e-12, err_msg=f"parameter {k}")


@pytest.mark.parametrize("i", [1, 6], ids=_sid)
def test_gradients_do_not_depend_on_max_batch_or_stale_scratch(i):
    """B = 9 on a fresh handle sized 9, and on a handle sized 256 that first ran B = 256 on other items (its scratch rows 9..255 then hold stale activations and
    d h rows): bit-equal outputs and gradients.  Both handles write gradients only, so the earlier step leaves the parameters as they were."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A = ENVELOPE[i]
    on, tg = _params(i)
    ht = MLPQHandle(_net(i, tg), 16)
    b9, b256 = _batch(_items(i, True, False), D, 9), _batch(_items(i, True, False, extra=1), D, 256)
    got = []
    for max_batch in (9, 256):
        net = _net(i, on)
        h = MLPQHandle(net, 16, max_batch=max_batch)
        if max_batch == 256:
            _step(h, ht, 256, b256, True, False, None, _outputs(256, A))
        out = _outputs(9, A)
        _step(h, ht, 9, b9, True, False, None, out)
        got.append(list(out) + _grads(net))
        assert all(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(net.kernel_parameters(), on))
    assert all(torch.equal(a, c) for a, c in zip(*got))


@pytest.mark.parametrize("i", [1, 4], ids=_sid)
def test_adam_over_six_steps(i):
    """Six consecutive updates (B = 100, steps_taken 0..5 in a device tensor) on fresh pick_items batches.  After every step the parameters equal
    torch.optim.Adam (float32) stepping on the kernel's own gradients (rtol 1e-6, atol 1e-7) and mlpq_reference.adam_steps in float64 (rtol 1e-5, atol 1e-7).
    The same inputs with write_grads=False (Adam only): parameters, exp_avg and exp_avg_sq bit-identical.  With lr=None (gradients only) from each step's
    starting parameters: the parameters stay untouched and the gradients are the same bits."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A = ENVELOPE[i]
    B, lr, n_steps = 100, 1e-3, 6
    on, tg = _params(i)
    ht = MLPQHandle(_net(i, tg), 16)
    net = _net(i, on)
    h = MLPQHandle(net, 16, max_batch=B, lr=lr)
    shadow = [v.float().cuda().requires_grad_(True) for v in on]
    opt = torch.optim.Adam(shadow, lr=lr)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    batches, starts, grads_per_step = [], [], []
    worst32 = worst64 = 0.0
    for k in range(n_steps):
        cur = [p.detach().double().cpu() for p in net.kernel_parameters()]
        starts.append(cur)
        batches.append(_batch(R.pick_items(cur, tg, D, A, DISCOUNT, True, False, 500 + 10 * i + k), D, B))
        assert int(steps) == k
        _step(h, ht, B, batches[k], True, False, steps, _outputs(B, A))
        steps += 1
        grads_per_step.append(_grads(net))
        for s, gk in zip(shadow, grads_per_step[k]):
            s.grad = gk.clone()
        opt.step()
        want64 = R.adam_steps(on, [[g.cpu() for g in gs] for gs in grads_per_step], lr)[0][k]
        for p, s, w64 in zip(net.kernel_parameters(), shadow, want64):
            worst32 = max(worst32, float((p.detach() - s.detach()).abs().max()))
            worst64 = max(worst64, float((p.detach().double().cpu() - w64).abs().max()))
            np.testing.assert_allclose(p.detach().cpu(), s.detach().cpu(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
            np.testing.assert_allclose(p.detach().double().cpu(), w64, rtol=1e-5, atol=1e-7, err_msg=f"step {k}")
    print(f"MLPQ-ERR adam {_sid(i)} steps={n_steps} max_abs_vs_torch_f32={worst32:.3e} max_abs_vs_f64={worst64:.3e}")
    # Adam only
    net2 = _net(i, on)
    h2 = MLPQHandle(net2, 16, max_batch=B, lr=lr, write_grads=False)
    steps.zero_()
    for k in range(n_steps):
        _step(h2, ht, B, batches[k], True, False, steps, _outputs(B, A))
        steps += 1
    assert all(torch.equal(a, c) for a, c in zip(net.kernel_parameters(), net2.kernel_parameters()))
    assert all(torch.equal(a, c) for a, c in zip(h.exp_avg, h2.exp_avg)) and all(torch.equal(a, c) for a, c in zip(h.exp_avg_sq, h2.exp_avg_sq))
    # gradients only
    net3 = _net(i, on)
    h3 = MLPQHandle(net3, 16, max_batch=B)
    for k in range(n_steps):
        with torch.no_grad():
            for p, v in zip(net3.kernel_parameters(), starts[k]):
                p.copy_(v.float())
        _step(h3, ht, B, batches[k], True, False, None, _outputs(B, A))
        assert all(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(net3.kernel_parameters(), starts[k]))
        assert all(torch.equal(a, c) for a, c in zip(_grads(net3), grads_per_step[k])), k


def test_publish_copies_every_tensor_of_a_three_layer_net():
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i = 2
    on, tg = _params(i)
    src, dst = _net(i, on), _net(i, tg)
    hs, hd = MLPQHandle(src, 16), MLPQHandle(dst, 16)
    assert len(dst.kernel_parameters()) == 8 and not any(torch.equal(a, c) for a, c in zip(src.kernel_parameters(), dst.kernel_parameters()))
    hs.publish_to(hd)
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(src.kernel_parameters(), dst.kernel_parameters()))
    assert all(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(src.kernel_parameters(), on))


def test_train_step_rejects_bad_arguments_without_a_launch():
    """Online and target handles whose widths differ in the third layer only, a batch above max_batch, an unbound target: an error, and the outputs and
    gradients keep what they held."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    i, B = 1, 8
    D, _, hid, A = ENVELOPE[i]
    on, tg = _params(i)
    net = _net(i, on)
    h = MLPQHandle(net, 16, max_batch=B)
    ht = MLPQHandle(_net(i, tg), 16)
    other = MLPQHandle(EngineMLPQNet(D, (), hid[:2] + (hid[2] + 32,), A).cuda(), 16)
    raw = N.c_p()
    widths = (ctypes.c_int * 3)(*hid)
    N.check(N.lib().srlx_mlpq_create(ctypes.byref(raw), D, 3, ctypes.cast(widths, N.c_p), A, 16, 0, 0))
    unbound = types.SimpleNamespace(h=raw)
    b = _batch(_items(i, True, False), D, B + 1)
    for p in net.kernel_parameters():
        p.grad.fill_(3.0)
    try:
        for target, batch, message in ((other, B, "layer widths differ"), (ht, B + 1, "batch 9"), (unbound, B, "unbound")):
            out = _outputs(B + 1, A)
            with pytest.raises(N.SrlxError, match=message):
                h.train_step(target, batch, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, True, False, None, *out)
            torch.cuda.synchronize()
            assert all(bool((t == 7.0).all()) for t in out) and all(bool((p.grad == 3.0).all()) for p in net.kernel_parameters())
        # (the handles work: the same call with a valid target and batch runs)
        out = _outputs(B, A)
        _step(h, ht, B, b, True, False, None, out)
        assert bool(torch.isfinite(out[0][:B]).all()) and not bool((out[0][:B] == 7.0).any())
    finally:
        N.lib().srlx_mlpq_destroy(raw)
