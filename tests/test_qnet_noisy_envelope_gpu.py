"""The NoisyLinear form of the image Q-network (csrc/srlx_noisy.hip and the noisy branches of srlx_qnet_dense_rows, k_head, srlx_qnet_redraw_rows and backward_impl:
rainbow.Config.set_atari_config()'s own network) over the envelope the library admits for it, against the float64 yardstick of tests/qnet_noisy_reference.py
(tests/test_qnet_noisy_cpu.py shows its footing).

The noise is known EXACTLY without a library entry that hands it out: a TWIN handle of the same shape and `noise_seed` whose six mu tensors are 0 and whose sigmas
are 1 has effective tensors 0 + 1 * eps = eps bit for bit, contracted to an FMA or not; one draw is spent per forward_* / redraw_rows call, so as many calls on the
twin read the eps of any draw id before the handle under test uses it (`device_eps`).  That eps is held to the host mirror of csrc/srlx_noise_math.h
(`eps_mirror`), and every other comparison is float64 arithmetic on mu + sigma eps of the very draw the kernels used.

Bars, the project's own: Q-values within 1e-5 max |reference|, gradients rtol 1e-4 + atol 2e-5 max |reference| per tensor (tests/test_qnet_envelope_gpu.py).  Every
test prints what it measured as a fraction of its bar ("QNOISY-ERR ...", shown with -s) before it asserts; no element is left out of any comparison."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qnet_envelope_reference as R  # noqa: E402
import qnet_noisy_reference as NR  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
Q_BAR = 1e-5
EPS_BAR = 1e-5  # |device eps - float64 mirror|: see test_generator_equals_the_mirror
GRAD_NAMES = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc1.mu_w", "fc1.mu_b", "v2.mu_w", "v2.mu_b", "a2.mu_w", "a2.mu_b",
              "fc1.sigma_w", "fc1.sigma_b", "v2.sigma_w", "v2.sigma_b", "a2.sigma_w", "a2.sigma_b"]


# ---- networks and handles ----------------------------------------------------------------------------------------------------------------------------------------
def _noisy_net(case, twin=False):
    """The noisy EngineQNet of a case on the GPU: convolutions and mu of the case's randomised plain network, sigma of `make_sigma` (twin: mu = 0, sigma = 1)."""
    from simple_distributed_rl_amd.device.qnet import EngineQNet

    net_cpu, sigma, _ = NR.build(case)
    f = NR.as_forward(case)
    torch.manual_seed(0)
    net = EngineQNet(f.A, f.hw, f.window, f.hidden, f.filters, R._ENGINE_HEAD[f.head], noisy=True)
    with torch.no_grad():
        ps = net.kernel_parameters()
        for p, q in zip(ps[:6], net_cpu.kernel_parameters()[:6]):
            p.copy_(q)
        for p, q, s, sg in zip(ps[6:12], NR.dense_tensors(net_cpu), ps[12:], sigma):
            p.copy_(torch.zeros_like(q) if twin else q)
            s.copy_(torch.ones_like(sg) if twin else sg)
    return net.cuda()


def _handle(case, net, seed=None, max_batch=None):
    from simple_distributed_rl_amd.device.qnet import QNetInference

    return QNetInference(net, NR.as_forward(case).max_batch if max_batch is None else max_batch, noise_seed=NR.noise_seed(case) if seed is None else seed)


def _effective(qn):
    """([six effective tensors on the CPU, flat float32], the draw id they report)."""
    out = [qn.effective(k) for k in range(6)]
    torch.cuda.synchronize()
    ids = {d for _, d in out}
    assert len(ids) == 1, ids
    return [w.cpu() for w, _ in out], ids.pop()


def _read_twin(case, seed, n_draws):
    f = NR.as_forward(case)
    qn = _handle(case, _noisy_net(case, twin=True), seed, max_batch=1)
    ring = torch.zeros(f.hw[0] * f.hw[1], dtype=torch.uint8, device="cuda")
    off = torch.zeros((1, f.window), dtype=torch.int64, device="cuda")
    out = []
    for d in range(n_draws):
        qn.forward_u8(ring.data_ptr(), off)
        eff, draw = _effective(qn)
        assert draw == d
        out.append(eff)
    return out


@functools.lru_cache(maxsize=None)
def device_eps(case, seed, n_draws):
    """[draw][tensor] -> flat float32 CPU tensor: the kernels' own eps of draws 0 .. n_draws - 1 under `seed` at the case's shape, read through a twin handle."""
    return _read_twin(case, seed, n_draws)


def _is_effective(got, mu, sigma, eps):
    """Every element of `got` is float32(mu + sigma eps) evaluated as one FMA or with the product rounded first -- nothing else.  Returns the count of elements
    that match neither (0 = pass) and whether all took the FMA form / all the two-rounding form."""
    mu, sigma, eps, got = (t.detach().cpu().flatten() for t in (mu, sigma, eps, got))
    fma = (mu.double() + sigma.double() * eps.double()).float()  # (the product of two float32 values is exact in float64)
    two = mu + sigma * eps  # float32 on the CPU: the product rounded, then the sum
    return int(((got != fma) & (got != two)).sum()), bool((got == fma).all()), bool((got == two).all())


def _check_q(tag, got, want):
    got, want = got.detach().double().cpu(), want.double()
    scale, err = float(want.abs().max()), float((got - want).abs().max())
    print(f"QNOISY-ERR {tag} q_err/bar={err / (Q_BAR * scale):.3f} scale={scale:.3f}")
    assert torch.isfinite(got).all() and err <= Q_BAR * scale, (tag, err, scale)


@functools.lru_cache(maxsize=None)
def _forward_fixture(case):
    """(plain network on the CPU, noisy network on the GPU, ONE handle of the case's max_batch, ring, offsets, float stack, float64 convolution features of every
    row) -- shared by the forward tests of a case; they read the draw a call used back from the handle, so the order they run in does not matter."""
    net_cpu, _, inp = NR.build(case)
    net = _noisy_net(case)
    return net_cpu, net, _handle(case, net), inp.ring.cuda(), inp.off.cuda(), inp.x.cuda(), NR.features64(net_cpu, inp.x)


# ---- a. the generator --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [NR.FORWARD_CASES[k] for k in (0, 2, 3)], ids=NR.case_id)
def test_generator_equals_the_mirror(case):
    """The twin's eps of draws 0..2, all six tensors, within 1e-5 absolute of `eps_mirror`.  The bar: u1, u2 and the float32 products with 2^-24 are exact; float32
    rounding of 2 pi u2 and of the constant give at most 2 pi (2^-24 + 2.8e-8) in the angle, sin / cos are good to 2 float32 ulps of 1, logf / sqrtf to a few ulps
    of r <= 5.77 (u1 >= 2^-24): together at most 4.6e-6 (numpy's float32 evaluation against the float64 mirror: 2.0e-6 over 2e7 keys); 1e-5 is twice that, and a
    wrong key, bit field or pair order errs by O(1)."""
    seed = NR.noise_seed(case)
    eps = device_eps(case, seed, 3)
    sizes = [p.numel() for p in NR.dense_tensors(NR.build(case)[0])]
    worst = 0.0
    for d in range(3):
        for t, n in enumerate(sizes):
            got = eps[d][t]
            assert got.shape == (n,) and bool(torch.isfinite(got).all())
            err = float((got.double() - NR.eps_mirror(seed, d, t, n)).abs().max())
            worst = max(worst, err)
            print(f"QNOISY-ERR generator {NR.case_id(case)} draw {d} {NR.TENSORS[t]} n={n} eps_err/bar={err / EPS_BAR:.3f}")
            assert err <= EPS_BAR, (d, t, err)
    print(f"QNOISY-ERR generator {NR.case_id(case)} worst eps_err/bar={worst / EPS_BAR:.3f}")


def test_generator_of_the_mlp_q_network_equals_the_mirror():
    """srlx_mlpq_noisy_eps: the same header, with the index of `kernel_parameters()` as the tensor key -- every noisy tensor of a small shape (an odd-length bias
    among them) at draws 0, 1 and 2^40."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    torch.manual_seed(0)
    seed = 0xFEDCBA9876543210
    h = MLPQHandle(EngineMLPQNet(3, (), (64,), 3, 96, "average", noisy=True).cuda(), 16, noise_seed=seed)
    noisy = [k for k, s in enumerate(h.sigmas) if s is not None]
    assert len(noisy) >= 6 and any(h.params[k].numel() % 2 for k in noisy)
    worst = 0.0
    for d in (0, 1, 1 << 40):
        for k in noisy:
            got = h.eps(d, k)
            torch.cuda.synchronize()
            err = float((got.cpu().double().flatten() - NR.eps_mirror(seed, d, k, got.numel())).abs().max())
            worst = max(worst, err)
            assert err <= EPS_BAR, (d, k, err)
    print(f"QNOISY-ERR generator mlpq worst eps_err/bar={worst / EPS_BAR:.3f} over {len(noisy)} tensors x 3 draws")


def test_the_seed_is_the_stream():
    case = NR.FORWARD_CASES[3]
    seed = NR.noise_seed(case)
    a, b, c = _read_twin(case, seed, 2), _read_twin(case, seed, 2), _read_twin(case, seed + 1, 2)
    for d in range(2):
        for t in range(6):
            assert torch.equal(a[d][t], b[d][t])  # same seed on two fresh handles: the same bits
            assert not bool((a[d][t] == c[d][t]).any())  # another seed: another stream, in every element
        assert not bool((a[0][0] == a[1][0]).any())


# ---- b. the effective tensors ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NR.FORWARD_CASES, ids=NR.case_id)
def test_effective_tensors_are_mu_plus_sigma_eps(case):
    net_cpu, sigma, inp = NR.build(case)
    net = _noisy_net(case)
    before = [p.detach().clone() for p in net.kernel_parameters()]
    qn = _handle(case, net)
    eps = device_eps(case, NR.noise_seed(case), 3)
    ring, off = inp.ring.cuda(), inp.off.cuda()
    B = min(case.batches)
    forms = set()
    for d in range(3):
        qn.forward_u8(ring.data_ptr(), off[:B])
        eff, draw = _effective(qn)
        assert draw == d
        for t, (mu, sg) in enumerate(zip(NR.dense_tensors(net_cpu), sigma)):
            assert eff[t].shape == (mu.numel(),)
            bad, all_fma, all_two = _is_effective(eff[t], mu, sg, eps[d][t])
            forms.add("fma" if all_fma and not all_two else ("two" if all_two and not all_fma else "either"))
            print(f"QNOISY-ERR effective {NR.case_id(case)} draw {d} {NR.TENSORS[t]} n={mu.numel()} elements off both forms: {bad}")
            assert bad == 0, (d, t, bad)
    print(f"QNOISY-ERR effective {NR.case_id(case)} forms={sorted(forms)}")
    for name, p, b in zip(GRAD_NAMES, net.kernel_parameters(), before):
        assert torch.equal(p.detach(), b), name  # mu and sigma (and the convolutions) are read only


# ---- c. forward --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "u8"])
@pytest.mark.parametrize("case", NR.FORWARD_CASES, ids=NR.case_id)
def test_forward_matches_float64_on_the_draw_it_used(case, mode):
    """Every batch of the case, twice on the same rows: Q within the bar of float64 on the effective tensors read back after the call; rows past the batch -- one
    guard row past max_batch included -- keep their sentinel; the second call used another draw and gives other Q in every row."""
    net_cpu, net, qn, ring, off, x, feats = _forward_fixture(case)
    for B in case.batches:
        calls = []
        for rep in range(2):
            qbuf = torch.full((case.max_batch + 1, case.A), SENTINEL, device="cuda")
            if mode == "f32":
                qn.forward_f32(x[:B], out=qbuf[:B])
            else:
                qn.forward_u8(ring.data_ptr(), off[:B], out=qbuf[:B])
            eff, draw = _effective(qn)
            _check_q(f"forward_{mode} {NR.case_id(case)} B={B} call {rep} draw {draw}", qbuf[:B], NR.q_on_effective(net_cpu, eff, None, feats[:B]))
            assert bool((qbuf[B:] == SENTINEL).all()), "rows past the batch were written"
            calls.append((qbuf[:B].cpu(), draw))
        assert calls[1][1] == calls[0][1] + 1
        assert bool((calls[0][0] != calls[1][0]).any(dim=1).all())  # (the CPU suite: two draws move every row by more than 100 bars)


# ---- d. redraw + backward --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NR.BACKWARD_CASES, ids=NR.case_id)
def test_redraw_and_backward_match_float64_autograd(case):
    """forward_u8 over B * stride rows (draw 0), redraw_rows(B, stride) (draw 1), backward_u8: see the assertions.  The inputs are picked kink-free on
    eff(draw 1) computed from the twin's eps BEFORE the handle under test exists."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    net_cpu, sigma, _ = NR.build(case)
    B, stride, rows, seed = case.B, case.stride, case.B * case.stride, NR.noise_seed(case)
    eps = device_eps(case, seed, 2)
    mu = NR.dense_tensors(net_cpu)
    inp = NR.pick_inputs(case, net_cpu, NR.effective64(mu, sigma, [e.view(m.shape) for e, m in zip(eps[1], mu)]))
    feats = NR.features64(net_cpu, inp.x)
    net = _noisy_net(case)
    ring, off = inp.ring.cuda(), inp.off.cuda()
    grad_q = torch.randn((B, case.A), generator=torch.Generator().manual_seed(5 + B))
    dq = grad_q.cuda()
    train = torch.zeros(rows, dtype=torch.bool)
    train[::stride] = True

    def run(offsets):
        qn = QNetInference(net, rows, noise_seed=seed).enable_training(B)  # a fresh handle: draws 0 and 1 again
        q1 = qn.forward_u8(ring.data_ptr(), offsets).clone()
        eff0, d0 = _effective(qn)
        qbuf = torch.full((rows + 1, case.A), SENTINEL, device="cuda")
        qbuf[:rows] = q1
        qn.redraw_rows(B, stride, out=qbuf)
        eff1, d1 = _effective(qn)
        assert (d0, d1) == (0, 1)
        assert len(qn._params()) == 18
        for p in qn._params():
            p.grad.fill_(float("nan"))
        qn.backward_u8(ring.data_ptr(), offsets, dq, sample_stride=stride)
        torch.cuda.synchronize()
        for name, p in zip(GRAD_NAMES, qn._params()):
            assert p.grad.stride() == p.stride(), name  # the optimiser walks parameter and gradient with the same strides
        return q1.cpu(), qbuf.cpu(), eff0, eff1, [p.grad.detach().clone().cpu() for p in qn._params()]

    q1, q2, eff0, eff1, got = run(off)
    cid = NR.case_id(case)
    for d, eff in enumerate((eff0, eff1)):  # the draws are the twin's
        for t in range(6):
            assert _is_effective(eff[t], mu[t], sigma[t], eps[d][t])[0] == 0, (d, t)
    want0, want1 = NR.q_on_effective(net_cpu, eff0, None, feats), NR.q_on_effective(net_cpu, eff1, None, feats)
    _check_q(f"backward {cid} forward_u8 rows={rows} (draw 0)", q1, want0)
    _check_q(f"backward {cid} redraw_rows training rows (draw 1)", q2[:rows][train], want1[train])
    if stride > 1:
        assert torch.equal(q2[:rows][~train], q1[~train])  # the other rows keep the first call's bits ...
        _check_q(f"backward {cid} redraw_rows other rows (draw 0)", q2[:rows][~train], want0[~train])  # ... which are the first draw's
    assert bool((q2[:rows][train] != q1[train]).any(dim=1).all())
    assert bool((q2[rows:] == SENTINEL).all()), "the guard row was written"

    g12, gsig = NR.grads_on_effective(net_cpu, eff1, [e.view(m.shape) for e, m in zip(eps[1], mu)], inp.x[::stride], grad_q, range(B))
    worst = 0.0
    for name, g, w in zip(GRAD_NAMES, got, g12 + gsig):
        assert g.shape == w.shape, name
        bar = 1e-4 * w.abs() + 2e-5 * float(w.abs().max()) + 1e-12
        frac = float(((g.double() - w).abs() / bar).max())
        worst = max(worst, frac)
        print(f"QNOISY-ERR backward {cid} {name} grad_err/bar={frac:.3f} scale={float(w.abs().max()):.3e}")
    print(f"QNOISY-ERR backward {cid} worst grad_err/bar={worst:.3f} fc1_dgrad={'mfma' if B <= 32 else 'split'}")
    for name, g, w in zip(GRAD_NAMES, got, g12 + gsig):
        np.testing.assert_allclose(g.numpy(), w.numpy(), rtol=1e-4, atol=2e-5 * float(w.abs().max()) + 1e-12, err_msg=name)
    for t in range(6):  # d loss / d sigma = d loss / d effective * eps: ONE float32 product per element, with the twin's eps of draw 1
        assert torch.equal(got[12 + t].flatten(), got[6 + t].flatten() * eps[1][t]), GRAD_NAMES[12 + t]
    if stride > 1:  # rows that are not training rows contribute nothing: give them other frames
        off2 = off.clone()
        other = (~train).cuda()
        off2[other] = off[other].flip(0)
        assert not torch.equal(off2, off)
        q1b, q2b, _, _, got2 = run(off2)
        assert torch.equal(q2b[:rows][train], q2[:rows][train]) and not torch.equal(q1b, q1)
        for name, a, b in zip(GRAD_NAMES, got, got2):
            assert torch.equal(a, b), name


# ---- e. the policy pass ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NR.FORWARD_CASES[:2], ids=NR.case_id)
def test_policy_pass_spends_one_draw_and_is_greedy_on_its_own_q(case):
    net_cpu, net, _, ring, off, _, feats = _forward_fixture(case)
    qn = _handle(case, net)  # a fresh handle: draw ids from 0
    B = min(max(case.batches), 64)
    zeros = torch.zeros(B, device="cuda")
    counter = torch.tensor([7], dtype=torch.int64, device="cuda")
    for d in range(2):
        actions = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
        qbuf = torch.full((B + 1, case.A), SENTINEL, device="cuda")
        qn.forward_u8_policy(ring.data_ptr(), off[:B], zeros, 0x5EED, counter, actions, out=qbuf[:B])
        eff, draw = _effective(qn)
        assert draw == d  # exactly one draw per call
        _check_q(f"policy {NR.case_id(case)} B={B} draw {draw}", qbuf[:B], NR.q_on_effective(net_cpu, eff, None, feats[:B]))
        assert bool((qbuf[B:] == SENTINEL).all()) and int(actions[B]) == -1 and int(counter.item()) == 7
        assert np.array_equal(actions[:B].cpu().numpy(), np.argmax(qbuf[:B].cpu().numpy(), axis=1))  # (numpy: the FIRST maximum)


# ---- f. graph replay ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_forward_draws_anew_at_every_replay():
    """forward_u8 captured once (single stream, no side branches) and replayed three times: the draw counter lives on the device, so every replay spends a draw
    of its own and its Q belongs to the effective tensors it left."""
    case = NR.FORWARD_CASES[0]
    net_cpu, net, _, ring, off, _, feats = _forward_fixture(case)
    qn = _handle(case, net)
    B = max(case.batches)
    qbuf = torch.full((B + 1, case.A), SENTINEL, device="cuda")
    qn.forward_u8(ring.data_ptr(), off[:B], out=qbuf[:B])  # draw 0, eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        qn.forward_u8(ring.data_ptr(), off[:B], out=qbuf[:B])
    assert _effective(qn)[1] == 0  # capturing launched nothing
    seen = []
    for k in range(3):
        g.replay()
        eff, draw = _effective(qn)
        assert draw == k + 1
        _check_q(f"graph replay {k} {NR.case_id(case)} draw {draw}", qbuf[:B], NR.q_on_effective(net_cpu, eff, None, feats[:B]))
        assert bool((qbuf[B:] == SENTINEL).all())
        seen.append(qbuf[:B].cpu())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- g. re-bind --------------------------------------------------------------------------------------------------------------------------------------------------
def test_rebind_follows_the_new_mu_and_sigma_and_keeps_the_draw_counter():
    case = NR.FORWARD_CASES[3]
    net_cpu, sigma, inp = NR.build(case)
    net = _noisy_net(case)
    qn = _handle(case, net)
    eps = device_eps(case, NR.noise_seed(case), 3)
    ring, off, B = inp.ring.cuda(), inp.off.cuda(), max(case.batches)
    qn.forward_u8(ring.data_ptr(), off[:B])
    assert _effective(qn)[1] == 0
    # the 18 parameters move into fresh tensors: the convolutions keep their values, every mu is rolled by one element, every sigma reversed
    old = []
    with torch.no_grad():
        for k, p in enumerate(net.kernel_parameters()):
            old.append(p.data)
            new = p.data.clone(memory_format=torch.preserve_format)
            if 6 <= k < 12:
                new = new.flatten().roll(1).view(p.shape).contiguous()
            elif k >= 12:
                new = new.flatten().flip(0).view(p.shape).contiguous()
            p.data = new
            assert p.data_ptr() != old[-1].data_ptr()
    qn.bind()
    for t in old:
        t.fill_(float("nan"))  # whoever still reads the old homes shows
    net2 = copy.deepcopy(net_cpu)
    with torch.no_grad():
        for p, q in zip(NR.dense_tensors(net2), net.kernel_parameters()[6:12]):
            p.copy_(q.cpu())
    sigma2 = [p.detach().cpu() for p in net.kernel_parameters()[12:]]
    assert all(not torch.equal(a, b) for a, b in zip(sigma2[::2], sigma[::2]))
    qbuf = torch.full((case.max_batch + 1, case.A), SENTINEL, device="cuda")
    qn.forward_u8(ring.data_ptr(), off[:B], out=qbuf[:B])
    eff, draw = _effective(qn)
    assert draw == 1  # the counter runs on
    for t in range(6):
        assert _is_effective(eff[t], NR.dense_tensors(net2)[t], sigma2[t], eps[1][t])[0] == 0, t
    _check_q(f"re-bind {NR.case_id(case)} B={B} draw 1", qbuf[:B], NR.q_on_effective(net2, eff, inp.x[:B]))
    assert bool((qbuf[B:] == SENTINEL).all())


# ---- h. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def _small_noisy(max_batch=8, A=3):
    from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

    torch.manual_seed(0)
    net = EngineQNet(A, (20, 20), 4, 32, 32, "average", noisy=True).cuda()
    ring = torch.randint(0, 256, (9 * 400,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    off = (torch.arange(max_batch * 4, dtype=torch.int64, device="cuda").view(max_batch, 4) % 9) * 400
    return net, QNetInference(net, max_batch, noise_seed=3), ring, off


def test_setup_calls_a_noisy_handle_cannot_serve_are_refused_and_leave_it_as_it_was():
    from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

    lib = N.lib()
    net, qn, ring, off = _small_noisy()
    qn.enable_training(2)
    buf = torch.full((64,), SENTINEL, device="cuda")
    bump = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    m, v = torch.full_like(net.fc1.weight, SENTINEL), torch.full_like(net.fc1.weight, SENTINEL)
    tab = (N.c_p * 12)(*[buf.data_ptr()] * 12)
    refusals = [
        ("no persistent planes", lambda: lib.srlx_qnet_enable_fc1_planes(qn.h)),
        ("nothing to publish", lambda: lib.srlx_qnet_actor_sets_enable(qn.h)),
        ("qnet_publish: NoisyLinear source", lambda: lib.srlx_qnet_publish(qn.h, None, 0, 0, N.tptr(bump), N.torch_stream_ptr())),
        ("qnet_bind_uvfa: plain dueling handles only", lambda: lib.srlx_qnet_bind_uvfa(qn.h, N.tptr(buf), 4, 0, 1, -1, 0, -1, 0)),
        ("qnet_set_head_mode: .* plain layers", lambda: lib.srlx_qnet_set_head_mode(qn.h, 1, 16, None, None, 1e-5)),
        ("qnet_fuse_adam_fc1: NoisyLinear layers need the gradient of the effective weight", lambda: lib.srlx_qnet_fuse_adam_fc1(qn.h, N.tptr(m), N.tptr(v), 1e-3, 0.9, 0.999, 1e-8, N.tptr(steps))),
        # (the first dense layer's fused Adam, which this one takes its hyper-parameters from, was refused above: that is what it says)
        ("qnet_fuse_adam_rest: call srlx_qnet_fuse_adam_fc1 first", lambda: lib.srlx_qnet_fuse_adam_rest(qn.h, ctypes.cast(tab, N.c_p), ctypes.cast(tab, N.c_p), ctypes.cast(tab, N.c_p))),
    ]
    for message, call in refusals:
        with pytest.raises(N.SrlxError, match=message):
            N.check(call())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((m == SENTINEL).all()) and bool((v == SENTINEL).all()) and int(bump.item()) == 41 and int(steps.item()) == 0
    # srlx_qnet_bind_noisy on a plain-head handle
    plain = EngineQNet(3, (20, 20), 4, 32, 32, "plain").cuda()
    qp = QNetInference(plain, 8)
    sig = (N.c_p * 6)(*[p.data_ptr() for p in net.kernel_parameters()[12:]])
    with pytest.raises(N.SrlxError, match="qnet_bind_noisy: the plain Q head .* has no NoisyLinear form"):
        N.check(lib.srlx_qnet_bind_noisy(qp.h, ctypes.cast(sig, N.c_p), 3))
    with pytest.raises(N.SrlxError, match="not a noisy network"):  # ... and it did not become one
        qp.effective(0)
    x = torch.rand((8, 4, 20, 20), device="cuda")
    got = qp.forward_f32(x).clone()
    _check_q("refusal: the plain-head handle still serves its own network", got, R.reference_q(plain, x))
    # the noisy handle is what it was: no draw was spent, the next pass is draw 0 of its own network, training still works
    q = qn.forward_u8(ring.data_ptr(), off).clone()
    eff, draw = _effective(qn)
    assert draw == 0
    plain_twin = EngineQNet(3, (20, 20), 4, 32, 32, "average")
    with torch.no_grad():
        for p, s in zip(plain_twin.kernel_parameters()[:6], net.kernel_parameters()[:6]):
            p.copy_(s.cpu())
    frames = (ring.view(9, 20, 20)[off // 400].float() / 255).cpu()
    _check_q("refusal: the noisy handle still serves draw 0", q, NR.q_on_effective(plain_twin, eff, frames))
    qn.backward_u8(ring.data_ptr(), off, torch.ones((2, 3), device="cuda"), sample_stride=4)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in qn._params()) and float(net.fc1_sigma_w.grad.abs().max()) > 0


def test_redraw_rows_beyond_max_batch_is_refused_before_the_draw():
    net, qn, ring, off = _small_noisy()
    qbuf = torch.full((9, 3), SENTINEL, device="cuda")
    qn.forward_u8(ring.data_ptr(), off, out=qbuf[:8])
    eff, draw = _effective(qn)
    kept = qbuf.clone()
    for rows, stride in ((3, 3), (9, 1), (1, 9), (0, 1), (2, 0)):
        with pytest.raises(N.SrlxError, match="qnet_redraw_rows: rows -?\\d+ x stride -?\\d+ out of range"):
            qn.redraw_rows(rows, stride, out=qbuf)
    eff2, draw2 = _effective(qn)
    assert draw2 == draw == 0 and all(torch.equal(a, b) for a, b in zip(eff, eff2)) and torch.equal(qbuf, kept)  # no draw, no effective tensor, no Q row
    qn.redraw_rows(2, 4, out=qbuf)  # the largest it admits is served
    assert _effective(qn)[1] == 1 and bool((qbuf[8] == SENTINEL).all())


def test_backward_without_sigma_gradient_tensors_is_refused_before_any_launch():
    """A noisy training handle that never got srlx_qnet_bind_noisy_grads (a raw library call: `enable_training` always binds them): the refusal comes ahead of the
    backward pass's launches, so the twelve gradient tensors handed in keep their sentinel.  (It used to come from srlx_qnet_noisy_sigma_grads, the pass's LAST
    step, behind twelve written gradients.)"""
    lib = N.lib()
    net, qn, ring, off = _small_noisy()
    N.check(lib.srlx_qnet_enable_training(qn.h, 2))
    qn.forward_u8(ring.data_ptr(), off)
    grads = [torch.full_like(p, SENTINEL) for p in net.kernel_parameters()[:12]]
    tab = (N.c_p * 12)(*[g.data_ptr() for g in grads])
    dq = torch.ones((2, 3), device="cuda")
    with pytest.raises(N.SrlxError, match="the network is noisy but no sigma gradient tensors are bound \\(srlx_qnet_bind_noisy_grads\\)"):
        N.check(lib.srlx_qnet_backward_u8(qn.h, 2, 4, N.c_p(ring.data_ptr()), N.tptr(off), N.tptr(dq), ctypes.cast(tab, N.c_p), N.torch_stream_ptr()))
    torch.cuda.synchronize()
    for name, g in zip(GRAD_NAMES, grads):
        assert bool((g == SENTINEL).all()), f"{name}: written by a refused backward pass"
    # with the sigma gradients bound the same call is served
    sg = [torch.full_like(p, float("nan")) for p in net.kernel_parameters()[12:]]
    stab = (N.c_p * 6)(*[g.data_ptr() for g in sg])
    N.check(lib.srlx_qnet_bind_noisy_grads(qn.h, ctypes.cast(stab, N.c_p)))
    N.check(lib.srlx_qnet_backward_u8(qn.h, 2, 4, N.c_p(ring.data_ptr()), N.tptr(off), N.tptr(dq), ctypes.cast(tab, N.c_p), N.torch_stream_ptr()))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) for g in grads + sg) and not bool((grads[6] == SENTINEL).any())
