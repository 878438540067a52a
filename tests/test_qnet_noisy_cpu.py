"""The footing of the NoisyLinear envelope tests of the image Q-network, without a GPU (tests/qnet_noisy_reference.py has the mirror, the tables and the yardstick):
(1) the host mirror of the generator is a standard normal stream with the header's element pairing; (2) the noisy case tables reach the dispatch classes the GPU
file claims; (3) the noise matters at every case -- two draws move every row's Q by more than 100 Q bars, so a kernel that read the wrong draw could not pass;
(4) `pick_inputs` finds kink-free training rows; (5) sigma gradients as g_eff * eps ARE autograd's through mu + sigma eps; (6) the yardstick on effective tensors
is the reference-layout network holding them.  The noise is `eps_mirror` throughout; the per-case checks use the first rows of the case's inputs (at most ROWS)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qnet_envelope_reference as R  # noqa: E402
import qnet_noisy_reference as NR  # noqa: E402

ROWS = 4
Q_BAR = 1e-5  # the GPU suite's bar on Q, as a fraction of max |Q|


def _inputs(case):
    """(net, sigma, the first rows of the case's inputs) -- a backward case takes the draw-0 inputs `pick_inputs` starts from."""
    net, sigma, inp = NR.build(case)
    if inp is None:
        f = NR.as_forward(case)
        inp = R.make_inputs(f.hw, f.window, max(f.batches), NR.case_seed(case) + 7)
    return net, sigma, inp.x[:ROWS]


def _eff(case, net, sigma, draw):
    return NR.effective64(NR.dense_tensors(net), sigma, NR.eps_set(net, NR.noise_seed(case), draw))


# ---- 1. the mirror ---------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_is_a_standard_normal_stream():
    n, seed = 1 << 20, 5
    a, b = NR.eps_mirror(seed, 0, 0, n).numpy(), NR.eps_mirror(seed, 1, 0, n).numpy()
    se = 1.0 / np.sqrt(n)
    for e in (a, b):
        assert np.isfinite(e).all() and abs(e.mean()) <= 5 * se and abs(e.var() - 1.0) <= 5 * np.sqrt(2.0) * se
        assert abs(np.corrcoef(e[0::2], e[1::2])[0, 1]) <= 5 * np.sqrt(2.0) * se  # the two halves of a pair (n / 2 of them)
    assert abs(np.corrcoef(a, b)[0, 1]) <= 5 * se
    assert 4.5 < np.abs(a).max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-12  # tails exist and end where u1 = 2^-24 puts them (5.77)


def test_mirror_pairs_elements_and_keys_tensors():
    for n in (1, 7, 4097):
        odd, even = NR.eps_mirror(9, 3, 2, n), NR.eps_mirror(9, 3, 2, n + 1)
        assert odd.shape == (n,) and odd.dtype == torch.float64 and torch.equal(odd, even[:n])
    base = NR.eps_mirror(9, 3, 2, 64)
    for other in (NR.eps_mirror(9, 3, 3, 64), NR.eps_mirror(9, 4, 2, 64), NR.eps_mirror(10, 3, 2, 64)):
        assert not bool((other == base).any())  # another tensor, draw or seed: another stream
    # the key is seed + 0x9E37 (t + 1) in unsigned 64-bit arithmetic: it wraps, and tensor t of seed s is tensor 0 of seed s + 0x9E37 t
    assert torch.equal(NR.eps_mirror(2 ** 64 - 1, 0, 0, 8), NR.eps_mirror(0x9E37 - 1, 0, -1, 8))
    assert torch.equal(NR.eps_mirror(9, 3, 2, 64), NR.eps_mirror(9 + 2 * 0x9E37, 3, 0, 64))
    # one value by hand from the header's formula
    import hot_path_oracle as H

    x = int(H.rng_u64(np.uint64(9 + 3 * 0x9E37), np.uint64(3), np.uint64(5)))
    u1, u2 = ((x >> 40) + 1) / 2.0 ** 24, ((x >> 8) & 0xFFFFFF) / 2.0 ** 24
    r = np.sqrt(-2.0 * np.log(u1))
    assert abs(float(base[10]) - r * np.cos(2 * np.pi * u2)) <= 1e-15 * 6 and abs(float(base[11]) - r * np.sin(2 * np.pi * u2)) <= 1e-15 * 6


# ---- 2. the tables ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_noisy_tables_reach_the_classes_the_gpu_suite_claims():
    got = {}
    for c in NR.ALL_CASES:
        for k, v in R.dispatch_classes(c).items():
            got.setdefault(k, set()).update(v)
    assert got["head"] == {"average", "max", "naive"}
    assert {c.head for c in NR.BACKWARD_CASES} == {"average", "naive"}
    assert got["amax"] == {8, 16, 32}
    assert {b for b, _ in got["head_block"]} == {256, 512}
    assert got["fc1_dgrad"] == {"mfma", "split"}
    assert {R.dispatch_classes(c)["fc1_dgrad"].pop() for c in NR.BACKWARD_CASES if c.B in (32, 33)} == {"mfma", "split"}  # ... on both sides of the threshold
    assert {p.split("/")[0] for p in got["conv1"]} == {"fused", "AU8", "k_conv1_u8", "ANchw"}
    sizes = {NR.case_id(c): [p.numel() for p in NR.dense_tensors(NR.build(c)[0])] for c in NR.FORWARD_CASES[:1] + NR.FORWARD_CASES[2:3]}
    pairs = [sum((n + 1) // 2 for n in s) for s in sizes.values()]
    assert max(pairs) > 4096 * 1024  # k_noisy_eff's grid at its 4096-workgroup cap: a thread takes more than one pair
    assert min(pairs) < 4096 * 1024 // 256  # ... and a grid far below it (the smallest shape: 8219 pairs, 9 workgroups)
    assert any(1 in s for s in sizes.values())  # a one-element tensor: both halves of its pair partly unused
    shapes = {(c.hw, c.window, c.filters, c.hidden, c.A, c.head, c.batches) for c in NR.FORWARD_CASES}
    for row in [((8, 8), 1, 32, 32, 1, "average", (1, 3)), ((84, 84), 4, 32, 512, 6, "average", (1, 64, 257)), ((84, 84), 4, 64, 288, 17, "naive", (5,)),
                ((44, 20), 3, 32, 64, 9, "max", (5,)), ((20, 20), 4, 32, 960, 32, "average", (129, 257))]:
        assert row in shapes, row
    for row in [(8, 1, 32, 1, "average", 1, 1), (84, 4, 512, 6, "average", 32, 4), (84, 4, 512, 32, "naive", 64, 1), (44, 8, 64, 17, "naive", 33, 2),
                (12, 3, 96, 9, "average", 31, 3)]:
        assert R.BackwardCase(*row) in NR.BACKWARD_CASES, row
    assert len(NR.FORWARD_CASES) == 5 and len(NR.BACKWARD_CASES) == 5


def test_sigma_differs_in_every_element_and_is_sized_by_mu():
    net, sigma, _ = NR.build(NR.FORWARD_CASES[4])
    for p, s in zip(NR.dense_tensors(net), sigma):
        rms = float(p.detach().double().pow(2).mean().sqrt())
        assert s.shape == p.shape and s.dtype == torch.float32
        assert 0.25 * NR.SIGMA_FACTOR * rms * (1 - 1e-6) <= float(s.min()) and float(s.max()) <= NR.SIGMA_FACTOR * rms * (1 + 1e-6)
        assert s.numel() < 4 or s.flatten().unique().numel() > 0.9 * min(s.numel(), 1 << 20)


# ---- 3..6: per case --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NR.ALL_CASES, ids=NR.case_id)
def test_noise_matters_and_the_yardstick_is_the_reference_layout(case):
    net, sigma, x = _inputs(case)
    eff0, eff1 = _eff(case, net, sigma, 0), _eff(case, net, sigma, 1)
    q0, q1 = NR.q_on_effective(net, eff0, x), NR.q_on_effective(net, eff1, x)
    scale = float(torch.maximum(q0.abs().max(), q1.abs().max()))
    moved = (q0 - q1).abs().max(dim=1)[0]
    print(f"QNOISY-CPU {NR.case_id(case)} scale={scale:.3f} least moved row: {float(moved.min()) / (Q_BAR * scale):.0f} Q bars")
    assert 0.3 <= scale <= 100.0, scale
    assert float(moved.min()) > 100 * Q_BAR * scale  # EVERY row: a condition on the inputs (raise SIGMA_FACTOR for all cases if one fails it)
    # the cached-features path is the whole-network path ...
    feats = NR.features64(net, x)
    assert float((NR.q_on_effective(net, eff1, None, feats) - q1).abs().max()) <= 1e-13 * scale
    # ... and both are the reference-layout network (rl/torch_/networks.py:atari_qnetwork, noisy=False) loaded with eff through reference_state_dict's keys
    want = NR.reference_layout_q(net, eff1, x)
    assert float((q1 - want).abs().max()) <= 1e-13 * scale


@pytest.mark.parametrize("case", NR.BACKWARD_CASES, ids=NR.case_id)
def test_pick_inputs_ends_within_its_cap(case):
    net, sigma, _ = NR.build(case)
    eff1 = _eff(case, net, sigma, 1)
    inp = NR.pick_inputs(case, net, eff1)
    assert inp.x.shape[0] == case.B * case.stride
    assert R.kink_margin(NR.with_effective(net, eff1), inp.x[:: case.stride]) >= NR.KINK_MARGIN


@pytest.mark.parametrize("case", [NR.BACKWARD_CASES[0], NR.BACKWARD_CASES[4]], ids=NR.case_id)
def test_sigma_gradients_are_autograd_through_mu_plus_sigma_eps(case):
    net, sigma, x = _inputs(case)
    rows = list(range(0, x.shape[0], 2))
    grad_q = torch.randn((len(rows), case.A), generator=torch.Generator().manual_seed(3)).double()
    eps = NR.eps_set(net, NR.noise_seed(case), 1)
    g, g_sigma = NR.grads_on_effective(net, _eff(case, net, sigma, 1), eps, x, grad_q, rows)
    assert [t.shape for t in g] == [p.shape for p in net.kernel_parameters()] and [t.shape for t in g_sigma] == [s.shape for s in sigma]
    # autograd with mu and sigma as leaves
    n64 = R.engine_copy64(net)
    names = ["fc1.weight", "fc1.bias", "v2.weight", "v2.bias", "a2.weight", "a2.bias"]
    mu = [p.detach().clone().requires_grad_(True) for p in NR.dense_tensors(n64)]
    sg = [s.double().clone().requires_grad_(True) for s in sigma]
    q = torch.func.functional_call(n64, {k: m + s * e for k, m, s, e in zip(names, mu, sg, eps)}, (x.double(),))
    (q[rows] * grad_q).sum().backward()
    for name, a, b, c, d in zip(NR.TENSORS, g[6:], mu, g_sigma, sg):
        dead = case.A == 1 and case.head == "average" and name.startswith("a2")  # one action: adv - mean(adv) is 0 whatever a2 holds
        for got, want in ((a, b.grad), (c, d.grad)):
            scale = float(want.abs().max())
            assert (scale > 0) != dead and float((got - want).abs().max()) <= 1e-12 * scale, name
