"""Yardstick, noise mirror and case tables of the NoisyLinear envelope tests of the image Q-network (tests/test_qnet_noisy_cpu.py,
tests/test_qnet_noisy_envelope_gpu.py).  Nothing here needs a GPU.

`eps_mirror`: the generator of csrc/srlx_noise_math.h restated in float64 on the host -- the key `seed + 0x9E37 (t + 1)`, the two 24-bit fields of `normal_pair`,
Box-Muller with element 2 p taking r cos and element 2 p + 1 taking r sin.  It is written from the header's text, like the oracle's `rng_u64` it stands on; the GPU
suite holds the kernels' own eps (read through a twin handle with mu = 0, sigma = 1) to it.

`make_sigma`: every element of the six sigma tensors gets its own positive value (the initialisation's constant 0.5 / sqrt(fan_in) would not show a sigma read at the
wrong index), uniform in [0.25, 1] x SIGMA_FACTOR x rms(mu tensor).  SIGMA_FACTOR = 0.5 is the first value tried: tests/test_qnet_noisy_cpu.py asserts that at
every case two draws move every row's Q by more than 100 Q bars, and it holds there (no case needed more).

The float64 yardstick works on the EFFECTIVE tensors of a draw (`effective64` = mu + sigma eps): `q_on_effective` and `grads_on_effective` go through a float64 CPU
copy of a PLAIN `EngineQNet` whose six dense tensors are set to them (`with_effective`), with the autograd of `qnet_envelope_reference.reference_grads`.  The mu
gradients ARE the gradients with respect to the effective tensors, the sigma gradients those times eps (the chain rule: tests/test_qnet_noisy_cpu.py checks it
against autograd straight through mu + sigma eps)."""
import functools
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import hot_path_oracle as H  # noqa: E402
import qnet_envelope_reference as R  # noqa: E402

Case, BackwardCase, case_id, as_forward = R.Case, R.BackwardCase, R.case_id, R.as_forward
KINK_MARGIN = R.KINK_MARGIN
SIGMA_FACTOR = 0.5
MAX_DRAWS = 1000  # of the inputs of a backward case (qnet_envelope_reference.build's cap)
TENSORS = ["fc1.w", "fc1.b", "v2.w", "v2.b", "a2.w", "a2.b"]  # the order of the library's tensor index t (srlx_qnet_bind_noisy)

# Forward cases (noisy handles have no plain head): forward_f32 AND forward_u8 at every batch of `batches` on ONE handle of `max_batch` rows.
FORWARD_CASES = [
    Case((8, 8), 1, 32, 32, 1, "average", (1, 3), 3, "every lower bound; v2.b and a2.b are one-element tensors; 8219 pairs, the smallest k_noisy_eff grid"),
    Case((84, 84), 4, 32, 512, 6, "average", (1, 64, 257), 257, "set_atari_config(); fused convolutions; both head block sizes"),
    Case((84, 84), 4, 64, 288, 17, "naive", (5,), 5, "fc1 weight 576 x 15488 = 8.92 M elements > 2 * 4096 * 1024: k_noisy_eff's grid at its cap; odd A; k_head<32>"),
    Case((44, 20), 3, 32, 64, 9, "max", (5,), 7, "max head (forward only), odd A, non-square frame, odd window; B < max_batch"),
    Case((20, 20), 4, 32, 960, 32, "average", (129, 257), 257, "hidden beyond the training range; A at its maximum"),
]

# Backward cases (square frames, 32 filters; training admits average and naive): forward_u8 over B * stride rows, redraw_rows(B, stride), backward_u8.
BACKWARD_CASES = [
    BackwardCase(8, 1, 32, 1, "average", 1, 1),  # every lower bound
    BackwardCase(84, 4, 512, 6, "average", 32, 4),  # the Atari learner's own launch: batch 32, 3-step; last batch of the matrix-core FC1 data gradient
    BackwardCase(84, 4, 512, 32, "naive", 64, 1),  # every upper bound; split FC1 data gradient
    BackwardCase(44, 8, 64, 17, "naive", 33, 2),  # first batch of the split path; odd A
    BackwardCase(12, 3, 96, 9, "average", 31, 3),  # odd OH1 = 3; odd everything
]
ALL_CASES = FORWARD_CASES + BACKWARD_CASES


def case_seed(case):
    return 2000 + (FORWARD_CASES.index(case) if isinstance(case, Case) else 100 + BACKWARD_CASES.index(case))


def noise_seed(case):
    """The `noise_seed` the tests give the handles of a case (any value would do; large ones exercise the key's wrap-around at 2^64)."""
    return (0xFFFFFFFFFFFF0000 + 977 * case_seed(case)) & (2 ** 64 - 1)


# ---- the noise ---------------------------------------------------------------------------------------------------------------------------------------------------
def eps_mirror(seed, draw, t, n):
    """float64 [n]: eps(seed, draw, tensor t, elements 0..n-1) as csrc/srlx_noise_math.h defines it."""
    pairs = (n + 1) // 2
    key = (int(seed) + 0x9E37 * (int(t) + 1)) % 2 ** 64  # noisy_eps_pair: seed + 0x9E37ull * (u64)(t + 1), unsigned 64-bit arithmetic
    x = H.rng_u64(np.uint64(key), np.uint64(draw), np.arange(pairs, dtype=np.uint64))
    u1 = ((x >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0  # (0, 1]: the top 24 bits, plus one
    u2 = ((x >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0  # [0, 1): bits 8..31
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(2 * pairs, np.float64)
    out[0::2] = r * np.cos(2.0 * math.pi * u2)  # element 2 p
    out[1::2] = r * np.sin(2.0 * math.pi * u2)  # element 2 p + 1 (an odd n leaves the last pair's second half unused)
    return torch.from_numpy(out[:n].copy())


def dense_tensors(net):
    """The six dense tensors of a (plain or noisy) dueling EngineQNet in the library's order: for a noisy net these are the mu tensors."""
    return [net.fc1.weight, net.fc1.bias, net.v2.weight, net.v2.bias, net.a2.weight, net.a2.bias]


def eps_set(net, seed, draw):
    """The mirror's eps of one draw for all six tensors, each in its tensor's shape (the element index is the index into the contiguous tensor)."""
    return [eps_mirror(seed, draw, t, p.numel()).view(p.shape) for t, p in enumerate(dense_tensors(net))]


def make_sigma(net, seed):
    """Six float32 sigma tensors for `net`'s (randomised) mu: uniform in [0.25, 1] x SIGMA_FACTOR x rms(mu tensor), another value in every element."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in dense_tensors(net):
        rms = float(p.detach().double().pow(2).mean().sqrt())
        assert rms > 0
        out.append(((0.25 + 0.75 * torch.rand(p.shape, generator=g)) * (SIGMA_FACTOR * rms)).float())
    return out


def effective64(mu, sigma, eps):
    """mu + sigma eps per tensor, in float64 (the inputs' float32 values are exact in it)."""
    return [m.detach().double().cpu() + s.detach().double().cpu() * e.detach().double().cpu() for m, s, e in zip(mu, sigma, eps)]


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------------------------------
def with_effective(net, eff):
    """A float64 CPU copy of the plain EngineQNet `net` whose six dense tensors hold `eff` (any float type, flat or shaped)."""
    assert not net.noisy and not net.plain
    n64 = R.engine_copy64(net)
    with torch.no_grad():
        for p, e in zip(dense_tensors(n64), eff):
            p.copy_(e.detach().double().cpu().view(p.shape))
    return n64


def features64(net, x):
    """float64 [rows][flat]: what the convolutions (which carry no noise) hand the first dense layer, in its NHWC column order."""
    n64 = R.engine_copy64(net)
    with torch.no_grad():
        a = torch.relu(n64.conv3(torch.relu(n64.conv2(torch.relu(n64.conv1(x.detach().cpu().double()))))))
    return a.permute(0, 2, 3, 1).flatten(1)


def q_on_effective(net, eff, x, features=None):
    """float64 Q-values [rows][A] of `net`'s convolutions followed by the dense layers `eff`.  `features` = features64(net, x): the convolutions are the same under
    every draw, so a test that judges many draws on the same rows evaluates them once and only the copy's dense modules per draw (x is then not read;
    tests/test_qnet_noisy_cpu.py holds the two paths to each other)."""
    n64 = with_effective(net, eff)
    with torch.no_grad():
        if features is None:
            return n64(x.detach().cpu().double())
        h = torch.relu(n64.fc1(features))
        v, adv = n64.v2(h[:, : n64.hidden]), n64.a2(h[:, n64.hidden :])
        if n64.dueling_type == "average":
            return v + adv - adv.mean(dim=-1, keepdim=True)
        if n64.dueling_type == "max":
            return v + adv - adv.max(dim=-1, keepdim=True)[0]
        return v + adv


def reference_layout_q(net, eff, x):
    """float64 Q-values of the REFERENCE-LAYOUT network (rl/torch_/networks.py:atari_qnetwork, noisy=False) loaded with `eff` through `reference_state_dict`'s key
    mapping.  (Made float64 BEFORE the load: `qnet_envelope_reference.reference_network` loads into float32 modules, which would round a float64 `eff`.)"""
    from simple_distributed_rl_amd.rl.torch_.networks import atari_qnetwork

    n64 = with_effective(net, eff)
    ref = atari_qnetwork(net.n_actions, net.hw, net.window, net.hidden, False, net.filters, net.dueling_type).double()
    ref.load_state_dict(n64.reference_state_dict())
    with torch.no_grad():
        return ref(x.detach().cpu().double(), channels_first=True)


def grads_on_effective(net, eff, eps, x, grad_q, rows):
    """(the 12 gradients of sum(q[rows] * grad_q) in the order and layouts of `kernel_parameters()` -- entries 6..11 are the gradients with respect to the effective
    tensors, which are the mu gradients --, the 6 sigma gradients = those times eps), float64."""
    g = R.reference_grads(with_effective(net, eff), x, grad_q, rows)
    return g, [ge * e.detach().double().cpu().view(ge.shape) for ge, e in zip(g[6:], eps)]


@functools.lru_cache(maxsize=None)
def build(case):
    """(plain EngineQNet on the CPU with randomised mu, its six sigma tensors, inputs for a forward case's largest batch or None) -- cached and left unchanged."""
    from simple_distributed_rl_amd.device.qnet import EngineQNet

    f, seed = as_forward(case), case_seed(case)
    torch.manual_seed(seed)
    net = R.randomise(EngineQNet(f.A, f.hw, f.window, f.hidden, f.filters, R._ENGINE_HEAD[f.head]), seed)
    inp = R.make_inputs(f.hw, f.window, max(f.batches), seed + 7) if isinstance(case, Case) else None
    return net, make_sigma(net, seed + 3), inp


def pick_inputs(case, net, eff_s0):
    """Inputs of a backward case, drawn as `qnet_envelope_reference.build` draws them until no ReLU unit of a training row is within KINK_MARGIN of its kink -- the
    first dense layer's pre-activations taken on `eff_s0`, the effective tensors of the draw the gradient belongs to."""
    f, seed = as_forward(case), case_seed(case)
    net_s0 = with_effective(net, eff_s0)
    for draw in range(MAX_DRAWS):
        inp = R.make_inputs(f.hw, f.window, max(f.batches), seed + 7 + 1000 * draw)
        if R.kink_margin(net_s0, inp.x[:: case.stride]) >= KINK_MARGIN:
            return inp
    raise RuntimeError(f"{case_id(case)}: no draw of the inputs keeps every ReLU unit {KINK_MARGIN} away from its kink")
