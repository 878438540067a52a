"""The categorical (C51) head of the MLP Q-network kernels (libsrlx srlx_mlpq_create_categorical / srlx_mlpq_train_categorical / srlx_c51_loss,
csrc/srlx_mlpq.hip + csrc/srlx_c51_math.h) over the envelope the create call admits, against the float64 yardstick of tests/c51_reference.py (checked by
tests/test_c51_cpu.py; parity with the TensorFlow reference is unpinned): the acting pass, the whole learner step, the clip's gradient mask, Adam, the
one-purpose loss kernel bit for bit against the fused one, and the refusals.  Every test prints the error it measured ("C51-ERR ...", shown with -s) before it
asserts."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import c51_reference as R  # noqa: E402
import hot_path_oracle as H  # noqa: E402  (rng_u64 / u53: the keyed draws select_action documents)

pytestmark = pytest.mark.gpu

DISCOUNT = 0.9
# (D, layers, A, N, v_min, v_max)
ENVELOPE = [
    (1, (32,), 2, 2, -1.0, 1.0),  # every lower bound
    (4, (512,), 2, 51, -10.0, 10.0),  # c51.Config()'s default blocks on CartPole
    (256, (512, 512, 512), 8, 64, -10.0, 10.0),  # every upper bound, A * N = 512, the largest LDS footprint
    (8, (32,), 7, 73, -3.0, 5.0),  # 511 columns: not a multiple of 32; an asymmetric support
    (4, (32,), 10, 51, -10.0, 10.0),  # the head wider than the trunk
]
ALL_B = (1, 7, 8, 9, 256)  # one item; one short of / exactly / one over a workgroup's 8 items; the largest batch
LEARN_CASES = [(i, B) for i in range(len(ENVELOPE)) for B in ALL_B]
NEED = 256


def _sid(i):
    D, layers, A, n, lo, hi = ENVELOPE[i]
    return f"{D}-{'x'.join(str(w) for w in layers)}-{A}x{n}"


def test_the_default_row_is_the_default_config():
    from simple_distributed_rl_amd.algorithms import c51

    c = c51.Config()
    assert ENVELOPE[1][1:] == (tuple(c.hidden_block.kwargs["layer_sizes"]), 2, c.categorical_num_atoms, c.categorical_v_min, c.categorical_v_max)


@functools.lru_cache(maxsize=None)
def _params(i, scale=1.0):
    D, layers, A, n, _, _ = ENVELOPE[i]
    ps = R.init_params(D, layers, A, n, 3000 + i)
    if scale != 1.0:  # the out_layer scaled: wide logits, probabilities below the clip
        ps = ps[:-2] + [(ps[-2] * scale).float().double(), (ps[-1] * scale).float().double()]
    return ps


@functools.lru_cache(maxsize=None)
def _items(i, scale=1.0):
    D, _, A, n, lo, hi = ENVELOPE[i]
    return R.pick_items(_params(i, scale), D, A, n, lo, hi, DISCOUNT, 10 * i + int(scale), NEED)


@functools.lru_cache(maxsize=None)
def _ref(i, B, scale=1.0):
    """The yardstick's update on the first B items (computed once per case, shared, never modified)."""
    _, _, A, n, lo, hi = ENVELOPE[i]
    it = _items(i, scale)
    return R.learner_step(_params(i, scale), it.rows[it.i0[:B]], it.rows[it.i1[:B]], it.act[:B], it.rew[:B], it.term[:B], DISCOUNT, A, n, lo, hi)


def _net(i, params):
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    D, layers, A, n, lo, hi = ENVELOPE[i]
    net = EngineMLPQNet(D, (), layers, A, n_atoms=n, v_min=lo, v_max=hi).cuda()
    with torch.no_grad():
        for p, v in zip(net.kernel_parameters(), params):
            p.copy_(v.float())
    return net


def _batch(it, D, B):
    """The first B items on the device.  Only the rows these items use are placed, on the even row slots of a NaN-filled buffer in a shuffled order: s_1 of an
    item is never the row after its s_0, items share rows where pick_items chained them, and a read of any other row poisons the result."""
    P = it.rows.shape[0]
    slot = torch.randperm(P, generator=torch.Generator().manual_seed(B)) * 2
    buf = torch.full((2 * P, D), float("nan"))
    used = torch.cat([it.i0[:B], it.i1[:B]]).unique()
    buf[slot[used]] = it.rows[used].float()
    off = torch.stack([slot[it.i0[:B]] * D, slot[it.i1[:B]] * D], 1).to(torch.int64)
    return types.SimpleNamespace(obs=buf.cuda(), off=off.cuda(), act=it.act[:B].int().cuda(), rew=it.rew[:B].float().cuda(), term=it.term[:B].float().cuda())


def _outputs(B, A, n):
    """q0, p0, m, loss, item_loss with one guard row past the batch."""
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    return f(B + 1, A), f(B + 1, n), f(B + 1, n), f(1), f(B + 1)


def _step(h, B, b, steps, out):
    h.train_categorical(B, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, DISCOUNT, steps, *out)
    torch.cuda.synchronize()


def _grads(net):
    return [p.grad.detach().clone() for p in net.kernel_parameters()]


def _guards_untouched(out, B):
    q0, p0, m, _, item = out
    return all(float(t[B].min()) == 7.0 and float(t[B].max()) == 7.0 for t in (q0, p0, m, item))


# ---- 1. the acting pass -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ENVELOPE)), ids=_sid)
def test_forward_expectations_and_actions(i):
    """1, 15, 16 and 17 rows (a workgroup takes 16): the expectations at rtol 1e-5 / atol 1e-6 of float64; with eps = 0 the yardstick's greedy action on every
    row whose two best means are further apart than pick_items' tie margin; with eps = 1 the keyed draw select_action documents; nothing past row `rows`."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, A, n, lo, hi = ENVELOPE[i]
    params = _params(i)
    h = MLPQHandle(_net(i, params), 32)
    g = torch.Generator().manual_seed(i)
    seed, worst = 0xC51 + i, 0.0
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for rows in (1, 15, 16, 17):
        x = torch.randn(rows, D, generator=g)
        q = torch.full((rows + 1, A), 7.0, device="cuda")
        greedy = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
        explore = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
        h.forward(rows, x.cuda(), q=q, eps=torch.zeros(rows, device="cuda"), seed=seed, counter=counter, actions=greedy)
        h.forward(rows, x.cuda(), eps=torch.ones(rows, device="cuda"), seed=seed, counter=counter, actions=explore)
        torch.cuda.synchronize()
        want = R.expectations(R.logits(params, x.double(), A, n), lo, hi)
        got = q[:rows].double().cpu()
        worst = max(worst, float((got - want).abs().max()))
        assert float(q[rows].min()) == 7.0 and float(q[rows].max()) == 7.0 and int(greedy[rows]) == -7 and int(explore[rows]) == -7
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
        top = want.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) >= 16 * n * 2.0 ** -24 * max(abs(lo), abs(hi))
        assert torch.equal(greedy[:rows].cpu().long()[clear], want.argmax(1)[clear])
        m = np.arange(rows, dtype=np.uint64)
        pick = np.minimum((H.u53(H.rng_u64(seed, np.uint64(5), 2 * m + np.uint64(1))) * A).astype(np.int64), A - 1)
        np.testing.assert_array_equal(explore[:rows].cpu().numpy(), pick)
    print(f"C51-ERR forward {_sid(i)} worst_abs={worst:.3e}")


# ---- 2. the learner step ------------------------------------------------------------------------------------------------------------------------------------
def _check_step(i, B, scale, out, grads, slack=None):
    """The bars of tests/test_rainbow_vector_gpu.py: q0 / p0 / m at rtol 1e-5 / atol 1e-6, the loss at rel 1e-5, every gradient at rtol 1e-5 with an absolute
    slack of 1e-5 * max |g| of its tensor; sum m = 1 within 1e-6.  `slack` (the clip test): per-output absolute slack, added to atol."""
    ref = _ref(i, B, scale)
    q0, p0, m, loss, item = out
    slack = slack or {}
    gerr = max(float((gk.double().cpu() - gr).abs().max()) / float(gr.abs().max()) for gk, gr in zip(grads, ref.grads))
    print(f"C51-ERR learner {_sid(i)} B={B} scale={scale} q0={float((q0[:B].double().cpu() - ref.q0).abs().max()):.3e} "
          f"p0={float((p0[:B].double().cpu() - ref.p0).abs().max()):.3e} m={float((m[:B].double().cpu() - ref.m).abs().max()):.3e} "
          f"loss_rel={abs(float(loss) - ref.loss) / ref.loss:.3e} grad_rel_to_max={gerr:.3e} mass={float((m[:B].double().sum(1) - 1).abs().max()):.3e}")
    assert _guards_untouched(out, B)
    np.testing.assert_allclose(q0[:B].double().cpu(), ref.q0, rtol=1e-5, atol=1e-6 + slack.get("q0", 0.0))
    np.testing.assert_allclose(p0[:B].double().cpu(), ref.p0, rtol=1e-5, atol=1e-6 + slack.get("p0", 0.0))
    np.testing.assert_allclose(m[:B].double().cpu(), ref.m, rtol=1e-5, atol=1e-6 + slack.get("m", 0.0))
    np.testing.assert_allclose(item[:B].double().cpu(), ref.item_loss, rtol=1e-5, atol=1e-6 + slack.get("item", 0.0))
    assert abs(float(loss) - ref.loss) <= 1e-5 * abs(ref.loss) + slack.get("loss", 0.0)
    assert float((m[:B].double().sum(1) - 1).abs().max()) <= 1e-6
    for k, (gk, gr) in enumerate(zip(grads, ref.grads)):
        np.testing.assert_allclose(gk.double().cpu(), gr, rtol=1e-5, atol=1e-5 * float(gr.abs().max()) + 1e-12 + slack.get(k, 0.0), err_msg=f"parameter {k}")


@pytest.mark.parametrize("i, B", LEARN_CASES, ids=[f"{_sid(i)}-B{B}" for i, B in LEARN_CASES])
def test_learner_step_matches_float64_yardstick(i, B):
    """One srlx_mlpq_train_categorical (gradients only) on the first B items of pick_items -- the forced cases first -- against c51_reference.learner_step.
    Nothing is written past row B of the outputs.  At B = 9 a second run on a fresh handle gives the same bits."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, A, n, _, _ = ENVELOPE[i]
    net = _net(i, _params(i))
    h = MLPQHandle(net, 16, max_batch=B)
    b = _batch(_items(i), D, B)
    out = _outputs(B, A, n)
    _step(h, B, b, None, out)
    grads = _grads(net)
    _check_step(i, B, 1.0, out, grads)
    if B >= R.FORCED:  # the forced cases: all mass on the last atom / the first atom / the reward's own atom
        m = out[2]
        assert float(m[0, n - 1]) == pytest.approx(1.0, abs=1e-6) and float(m[1, 0]) == pytest.approx(1.0, abs=1e-6)
        assert float(m[2, _items(i).atom]) == pytest.approx(1.0, abs=1e-6)
    if B == 9:
        net2 = _net(i, _params(i))
        out2 = _outputs(B, A, n)
        _step(MLPQHandle(net2, 16, max_batch=B), B, b, None, out2)
        assert all(torch.equal(a, c) for a, c in zip(list(out) + grads, list(out2) + _grads(net2)))


# ---- 3. the clip --------------------------------------------------------------------------------------------------------------------------------------------
CLIP_SCALE = 20.0


def test_clipped_probabilities_follow_the_closed_form():
    """ENVELOPE row 1 with the out_layer scaled by CLIP_SCALE: between 10 % and 60 % of the yardstick's (item, atom) probabilities of a_0 lie below 1e-6.  The
    checks of the learner-step test at its bars, except q0: the expectations miss atol 1e-6 on this set (2.2e-5 measured, the yardstick's own float32 run is
    1.1e-5 from its float64 run), so q0 alone gets an absolute slack of 2 x the yardstick's own |float32 - float64| on q0 (the rule of the README's parity
    statement; DESIGN.md 7j has the measured errors).  The seeds of clipped atoms carry no -u_k term: d loss / d logit_k = p_k sum_i u_i / B."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i, B = 1, 256
    D, _, A, n, lo, hi = ENVELOPE[i]
    params = _params(i, CLIP_SCALE)
    it = _items(i, CLIP_SCALE)
    ref = _ref(i, B, CLIP_SCALE)
    share = float((ref.p0 < R.CLIP_LO).double().mean())
    print(f"C51-ERR clip share_below_1e-6={share:.3f}")
    assert 0.10 <= share <= 0.60, share
    # the yardstick's own |float32 - float64| on every output: the same program evaluated with float32 tensors
    r32 = R.learner_step(params, it.rows[it.i0[:B]], it.rows[it.i1[:B]], it.act[:B], it.rew[:B], it.term[:B], DISCOUNT, A, n, lo, hi, dtype=torch.float32)
    slack = dict(q0=2.0 * float((r32.q0.double() - ref.q0).abs().max()))
    print(f"C51-ERR clip slack q0={slack['q0']:.3e}")
    net = _net(i, params)
    h = MLPQHandle(net, 16, max_batch=B)
    out = _outputs(B, A, n)
    _step(h, B, _batch(it, D, B), None, out)
    _check_step(i, B, CLIP_SCALE, out, _grads(net), slack)
    # the out_layer bias gradient is the batch sum of the seeds: on a_0's clipped atoms of item b the seed is p_k * sum_i u_i / B exactly in form
    p0, m = out[1][:B].double().cpu(), out[2][:B].double().cpu()
    u = torch.where((p0 >= R.CLIP_LO) & (p0 <= 1.0), m, torch.zeros_like(m))
    seeds = torch.zeros(B, A, n, dtype=torch.float64)
    seeds[torch.arange(B), it.act[:B]] = (p0 * u.sum(1, keepdim=True) - u) / B
    got_bias = net.out_layer.bias.grad.double().cpu().view(A, n)
    np.testing.assert_allclose(got_bias, seeds.sum(0), rtol=1e-5, atol=1e-5 * float(seeds.sum(0).abs().max()))
    # the per-item seeds, as srlx_c51_loss shows them on torch's logits of the same network: the yardstick's autograd gradient at the gradient bar, and on the
    # atoms the yardstick clips exactly p_k * sum_i u_i / B >= 0 -- with the -u_k term such a seed would be negative wherever m_k > p_k
    from simple_distributed_rl_amd.algorithms._device_ops import C51Ops

    b = _batch(it, D, B)
    with torch.no_grad():
        lg = net.logits(torch.cat([it.rows[it.i0[:B]], it.rows[it.i1[:B]]]).float().cuda()).reshape(2 * B, A * n)
    m2, p2, grad, _ = C51Ops(torch.device("cuda:0")).loss(lg[B:].contiguous(), lg[:B].contiguous(), b.act, b.rew, b.term, A, n, lo, hi, DISCOUNT)
    torch.cuda.synchronize()
    np.testing.assert_allclose(grad.double().cpu(), ref.grad_logits, rtol=1e-5, atol=1e-5 * float(ref.grad_logits.abs().max()))
    clipped = ref.p0 < R.CLIP_LO
    on_a0 = grad.double().cpu().view(B, A, n)[torch.arange(B), it.act[:B]]
    want = p2.double().cpu() * torch.where(p2.cpu() >= 1e-6, m2.cpu(), torch.zeros_like(m2.cpu())).double().sum(1, keepdim=True) / B
    assert bool(clipped.any()) and bool((on_a0[clipped] >= 0).all()) and bool((ref.m[clipped] > ref.p0[clipped]).any())
    np.testing.assert_allclose(on_a0[clipped], want[clipped], rtol=1e-5, atol=0)


# ---- 4. Adam ------------------------------------------------------------------------------------------------------------------------------------------------
def test_adam_steps_on_the_yardstick_gradients():
    """Two updates with Adam bound (B = 32, steps_taken 0 and 1 in a device tensor): after each, the parameters equal torch.optim.Adam stepping on the kernel's
    own gradients (rtol 1e-6, atol 1e-7: the bar of the MLP tests) and float64 Adam on the yardstick's gradients (rtol 1e-5, atol 1e-7), except entries whose
    gradient is below 1e-4 * max |g| (the first Adam steps are about lr * g / |g|: only the bound 2 lr holds there).  The second step starts from the updated
    weights: its yardstick is evaluated there."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i, B, lr = 1, 32, 1e-3
    D, _, A, n, lo, hi = ENVELOPE[i]
    it = _items(i)
    net = _net(i, _params(i))
    h = MLPQHandle(net, 16, max_batch=B, lr=lr)
    shadow = [v.float().cuda().requires_grad_(True) for v in _params(i)]
    opt = torch.optim.Adam(shadow, lr=lr)
    p64 = [v.clone().requires_grad_(True) for v in _params(i)]
    opt64 = torch.optim.Adam(p64, lr=lr)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    b = _batch(it, D, B)
    for k in range(2):
        cur = [p.detach().double().cpu() for p in net.kernel_parameters()]
        ref = R.learner_step(cur, it.rows[it.i0[:B]], it.rows[it.i1[:B]], it.act[:B], it.rew[:B], it.term[:B], DISCOUNT, A, n, lo, hi)
        out = _outputs(B, A, n)
        _step(h, B, b, steps, out)
        steps += 1
        assert abs(float(out[3]) - ref.loss) <= 1e-5 * ref.loss
        for s, gk in zip(shadow, _grads(net)):
            s.grad = gk.clone()
        opt.step()
        with torch.no_grad():
            for q, c in zip(p64, cur):
                q.copy_(c)
        for q, gr in zip(p64, ref.grads):
            q.grad = gr.clone()
        opt64.step()
        for p, s, q, gr in zip(net.kernel_parameters(), shadow, p64, ref.grads):
            np.testing.assert_allclose(p.detach().cpu(), s.detach().cpu(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
            big = gr.abs() >= 1e-4 * float(gr.abs().max())
            np.testing.assert_allclose(p.detach().double().cpu()[big], q.detach()[big], rtol=1e-5, atol=1e-7, err_msg=f"step {k}")
            assert float((p.detach().double().cpu() - q.detach()).abs().max()) <= 2 * lr
    assert not any(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(net.kernel_parameters(), _params(i)))


# ---- 5. the one-purpose loss kernel ---------------------------------------------------------------------------------------------------------------------------
def _dyadic_params(i, seed):
    """Parameters and observations on coarse dyadic grids, small enough that every float32 multiply-add of the forward pass is exact: the kernel's logits and
    torch's are then the same bits whatever the order of the sums."""
    D, layers, A, n, _, _ = ENVELOPE[i]
    assert len(layers) == 1
    g = torch.Generator().manual_seed(seed)
    grid = lambda shape, levels, step: (torch.randint(-levels, levels + 1, shape, generator=g).float() * step)  # noqa: E731
    W = layers[0]
    params = [grid((W, D), 8, 2.0 ** -4), grid((W,), 8, 2.0 ** -4), grid((A * n, W), 16, 2.0 ** -8), grid((A * n,), 16, 2.0 ** -4)]
    rows = grid((64, D), 8, 2.0 ** -3)
    return params, rows


@pytest.mark.parametrize("i", [1, 3], ids=_sid)
def test_loss_kernel_is_the_fused_kernel_bit_for_bit(i):
    """srlx_c51_loss on the logits of s' and s against srlx_mlpq_train_categorical, B = 9: m, p0 and the loss are bit-equal, and so is the gradient w.r.t. the
    logits where the fused step shows it -- its out_layer bias gradient is the sum of the [B][A * N] seed rows in item order.  The network and the observations
    lie on dyadic grids on which every float32 sum of the forward pass is exact, so torch's logits are the kernel's bits (asserted against float64)."""
    from simple_distributed_rl_amd.algorithms._device_ops import C51Ops
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    B = 9
    D, layers, A, n, lo, hi = ENVELOPE[i]
    params, rows = _dyadic_params(i, 77 + i)
    net = _net(i, [p.double() for p in params])
    g = torch.Generator().manual_seed(i)
    act = torch.randint(0, A, (B,), generator=g).int()
    rew = ((torch.rand(B, generator=g) * 2 - 1) * 0.25 * (hi - lo)).float()
    term = (torch.rand(B, generator=g) < 0.3).float()
    rew[0], term[0] = hi + 1, 1.0
    i0, i1 = torch.arange(B) * 2, torch.arange(B) * 2 + 1
    off = torch.stack([i0 * D, i1 * D], 1).to(torch.int64).cuda()
    obs = rows[: 2 * B].contiguous().cuda()
    h = MLPQHandle(net, 16, max_batch=B)
    out = _outputs(B, A, n)
    h.train_categorical(B, obs.data_ptr(), off, act.cuda(), rew.cuda(), term.cuda(), DISCOUNT, None, *out)
    torch.cuda.synchronize()
    with torch.no_grad():
        lg = net.logits(obs).reshape(2 * B, A * n)
        # (exactness: the float64 logits are float32 values)
        lg64 = R.logits([p.double() for p in params], rows[: 2 * B].double(), A, n).reshape(2 * B, A * n)
        assert torch.equal(lg.double().cpu(), lg64), "the dyadic grid is not exact for this shape"
    m, p0, grad, loss = C51Ops(torch.device("cuda:0")).loss(lg[1::2].contiguous(), lg[0::2].contiguous(), act.cuda(), rew.cuda(), term.cuda(), A, n, lo, hi, DISCOUNT)
    torch.cuda.synchronize()
    assert torch.equal(m, out[2][:B]) and torch.equal(p0, out[1][:B]) and torch.equal(loss, out[3])
    # grad_logits of the fused kernel: its out_layer bias gradient is their sum over the batch in item order (k_mlpq_grad_adam)
    want_bias = torch.zeros(A * n, device="cuda")
    for b in range(B):
        want_bias = want_bias + grad[b]
    assert torch.equal(net.out_layer.bias.grad, want_bias)
    assert float(grad.abs().max()) > 0 and bool((grad.view(B, A, n)[torch.arange(B), (act.long() + 1) % A] == 0).all())


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_handles_refuse_each_others_updates():
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    i, B = 1, 8
    D, layers, A, n, lo, hi = ENVELOPE[i]
    cat = MLPQHandle(_net(i, _params(i)), 16, max_batch=B)
    plain = MLPQHandle(EngineMLPQNet(D, (), layers, A).cuda(), 16, max_batch=B)
    duel = MLPQHandle(EngineMLPQNet(D, (), (64,), A, dueling_units=64).cuda(), 16, max_batch=B)
    b = _batch(_items(i), D, B)
    w = torch.ones(B, device="cuda")
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    q0, target, loss, pri = f(B, A), f(B), f(1), f(B)
    act2, rew2, term2 = b.act.view(B, 1), b.rew.view(B, 1), b.term.view(B, 1)
    with pytest.raises(N.SrlxError, match="srlx_mlpq_train_categorical"):
        cat.train_step(plain, B, b.obs.data_ptr(), b.off, act2, rew2, term2, w, DISCOUNT, True, False, None, q0, target, loss, pri)
    with pytest.raises(N.SrlxError, match="srlx_mlpq_train_categorical"):
        cat.train_nstep(plain, B, 1, b.obs.data_ptr(), b.off, act2, rew2, term2, w, DISCOUNT, 1.0, True, False, None, q0, target, loss, pri)
    sig = (N.c_p * 4)(*[p.data_ptr() for p in cat.params])
    import ctypes

    assert N.lib().srlx_mlpq_bind_noisy(cat.h, ctypes.cast(sig, N.c_p), ctypes.c_uint64(1)) != 0 and b"categorical handle" in N.lib().srlx_last_error()
    for other, word in ((plain, "a plain handle"), (duel, "a dueling handle")):
        out = _outputs(B, A, n)
        with pytest.raises(N.SrlxError, match=word):
            other.train_categorical(B, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, DISCOUNT, None, *out)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)
    assert all(bool((t == 7.0).all()) for t in (q0, target, loss, pri))
    out = _outputs(B, A, n)  # (the categorical handle works)
    _step(cat, B, b, None, out)
    assert bool(torch.isfinite(out[0][:B]).all()) and not bool((out[0][:B] == 7.0).any())
