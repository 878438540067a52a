"""The image Q-network kernels (libsrlx srlx_qnet_*: csrc/srlx_qnet.hip, srlx_qnet_bwd.hip, srlx_qnet_fused.hip) over the envelope srlx_qnet_create and
srlx_qnet_enable_training admit -- frames from 8 x 8 up, non-square, any window, 32 / 64 / 128 filters, hidden a multiple of 32, 1..32 actions, the four heads;
training on square frames of side 8..84 with 32 filters, batches 1..64 -- against the float64 yardstick of tests/qnet_envelope_reference.py (the reference-layout
network on the CPU; tests/test_qnet_envelope_cpu.py shows that float32 torch stays within 1e-6 of it and that the case tables reach every dispatch class).
Bars, the project's own: Q-values within 1e-5 max |reference| (north star; tests/test_qnet_gpu.py), gradients rtol 1e-4 + atol 2e-5 max |reference| per tensor
(test_backward_u8_matches_autograd).  Every test prints the error it measured ("QNET-ERR ...", shown with -s) before it asserts."""
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

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GRAD_NAMES = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc1.w", "fc1.b", "v2.w", "v2.b", "a2.w", "a2.b"]


@functools.lru_cache(maxsize=None)
def _device(case):
    """(network on the GPU, its inference handle of the case's max_batch, ring, offsets, float stack) -- shared by the two forward tests of a case."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    net_cpu, inp = R.build(case)
    net = copy.deepcopy(net_cpu).cuda()
    return net, QNetInference(net, R.as_forward(case).max_batch), inp.ring.cuda(), inp.off.cuda(), inp.x.cuda()


def _check_q(tag, got, want):
    got, want = got.detach().double().cpu(), want.double()
    scale, err = float(want.abs().max()), float((got - want).abs().max())
    print(f"QNET-ERR {tag} q_err/scale={err / scale:.3e} scale={scale:.3f}")
    assert torch.isfinite(got).all() and err <= 1e-5 * scale, (tag, err, scale)
    return err / scale


@pytest.mark.parametrize("mode", ["f32", "u8"])
@pytest.mark.parametrize("case", R.FORWARD_CASES, ids=R.case_id)
def test_forward_matches_the_float64_reference(case, mode):
    """forward_f32 on the float stack and forward_u8 on the bytes of the same frames (about 10 % zero-history slots, the ring's first and last frame among the
    sampled ones) at every batch of the case, into a q buffer whose rows past the batch -- one guard row past max_batch included -- must keep their sentinel."""
    net, qn, ring, off, x = _device(case)
    want = R.build_reference_q(case)
    for B in case.batches:
        qbuf = torch.full((case.max_batch + 1, case.A), SENTINEL, device="cuda")
        if mode == "f32":
            qn.forward_f32(x[:B], out=qbuf[:B])
        else:
            qn.forward_u8(ring.data_ptr(), off[:B], out=qbuf[:B])
        torch.cuda.synchronize()
        _check_q(f"forward_{mode} {R.case_id(case)} B={B} max_batch={case.max_batch} classes={_classes(case, mode, B)}", qbuf[:B], want[:B])
        assert bool((qbuf[B:] == SENTINEL).all()), "rows past the batch were written"


def _classes(case, mode, B):
    """The dispatch classes of this launch as the mirror sees them, for the log line."""
    conv1 = "ANchw" if mode == "f32" else R.conv1_path_u8(case.hw, case.window, case.filters, B)
    _, _, oh2, ow2, oh3, ow3, flat = R.geometry(case.hw, case.filters)
    splits, used = R.fc1_splits(flat, case.hidden, B, case.max_batch)
    tiles = "" if conv1 == "fused" else "/tiles%d,%d" % (R.gemm_tile(B * oh2 * ow2, 2 * case.filters), R.gemm_tile(B * oh3 * ow3, 2 * case.filters))
    return f"{conv1}{tiles}/used{used}of{splits}"


@pytest.mark.parametrize("case", R.BACKWARD_CASES, ids=R.case_id)
def test_backward_matches_float64_autograd(case):
    """forward_u8 over B * stride rows on a handle of exactly that many, training scratch for exactly B: Q-values, then every gradient of backward_u8 against float64
    autograd over the training rows 0, stride, 2 stride, ... -- written into NaN-filled gradient tensors of the parameters' own strides; and with other frames in
    the rows that are not training rows the gradients stay bit for bit the same."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    net_cpu, inp = R.build(case)
    B, stride, rows = case.B, case.stride, case.B * case.stride
    net = copy.deepcopy(net_cpu).cuda()
    qn = QNetInference(net, rows).enable_training(B)
    ring, off = inp.ring.cuda(), inp.off.cuda()
    grad_q = torch.randn((B, case.A), generator=torch.Generator().manual_seed(5 + B))
    train_rows = range(0, rows, stride)
    want = R.reference_grads(net_cpu, inp.x, grad_q, train_rows)
    dq = grad_q.cuda()

    def run(offsets):
        q = qn.forward_u8(ring.data_ptr(), offsets).clone()
        for k, p in enumerate(qn._params()):
            p.grad.fill_(0.0 if net.plain and k in (8, 9) else float("nan"))  # (the plain head's unused v2 entries receive no gradient)
        qn.backward_u8(ring.data_ptr(), offsets, dq, sample_stride=stride)
        torch.cuda.synchronize()
        return q, [p.grad.detach().clone() for p in qn._params()]

    q, got = run(off)
    _check_q(f"backward {R.case_id(case)} forward_u8 rows={rows}", q, R.build_reference_q(case))
    worst = 0.0
    for name, p, g, w in zip(GRAD_NAMES, qn._params(), got, want):
        assert p.grad.stride() == p.stride(), name  # the fused Adam walks parameter and gradient with the same strides
        scale = float(w.abs().max())
        err = float((g.double().cpu() - w).abs().max())
        print(f"QNET-ERR backward {R.case_id(case)} {name} grad_err/scale={err / (scale + 1e-300):.3e} scale={scale:.3e}")
        worst = max(worst, err / (scale + 1e-300))
    print(f"QNET-ERR backward {R.case_id(case)} worst grad_err/scale={worst:.3e} fc1_dgrad={'mfma' if B <= 32 else 'split'}")
    for name, g, w in zip(GRAD_NAMES, got, want):
        np.testing.assert_allclose(g.cpu().numpy(), w.numpy(), rtol=1e-4, atol=2e-5 * float(w.abs().max()) + 1e-12, err_msg=name)
    if stride > 1:  # rows that are not training rows contribute nothing: give them other frames
        off2 = off.clone()
        other = torch.ones(rows, dtype=torch.bool, device="cuda")
        other[::stride] = False
        off2[other] = off[other].flip(0)
        assert not torch.equal(off2, off)
        q2, got2 = run(off2)
        assert torch.equal(q2[::stride], q[::stride]) and not torch.equal(q2, q)
        for name, a, b in zip(GRAD_NAMES, got, got2):
            assert torch.equal(a, b), name


def _create(hw, window, filters, hidden, A, dueling, max_batch=4):
    h = N.c_p()
    N.check(N.lib().srlx_qnet_create(ctypes.byref(h), hw[0], hw[1], window, filters, hidden, A, dueling, max_batch, 0))
    return h


@pytest.mark.parametrize("args, limit", [
    (((20, 20), 4, 96, 32, 4, 0), "filters must be 32, 64 or 128"),
    (((20, 20), 4, 32, 48, 4, 0), "hidden multiples of 32"),
    (((20, 20), 4, 32, 32, 0, 0), "1 <= n_actions <= 32"),
    (((20, 20), 4, 32, 32, 33, 0), "1 <= n_actions <= 32"),
    (((7, 20), 4, 32, 32, 4, 0), "at least 8 x 8"),
    (((20, 7), 4, 32, 32, 4, 0), "at least 8 x 8"),
    (((20, 20), 4, 32, 32, 4, 4), r"dueling_type 0 \(average\), 1 \(max\), 2 \(naive\) or 3"),
])
def test_create_refuses_what_it_does_not_admit(args, limit):
    h = N.c_p()
    with pytest.raises(N.SrlxError, match=limit):
        N.check(N.lib().srlx_qnet_create(ctypes.byref(h), args[0][0], args[0][1], *args[1:], 4, 0))
    assert not h.value  # no handle: nothing to launch on
    good = _create((20, 20), 4, 32, 32, 4, 0)  # the same call inside the envelope is served
    assert good.value
    N.lib().srlx_qnet_destroy(good)


@pytest.mark.parametrize("hw, filters, hidden, head, max_train, limit", [
    ((20, 20), 64, 32, "average", 8, "32 filters"),
    ((20, 20), 32, 32, "max", 8, "dueling average / none or the plain head"),
    ((20, 24), 32, 32, "average", 8, "square frames"),
    ((22, 22), 32, 32, "average", 8, "multiple of 4"),
    ((88, 88), 32, 32, "average", 8, "at most 84"),
    ((20, 20), 32, 544, "average", 8, "hidden <= 512"),
    ((20, 20), 32, 32, "average", 65, "max_train_batch <= 64"),
])
def test_enable_training_refuses_what_the_backward_kernels_do_not_cover(hw, filters, hidden, head, max_train, limit):
    from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

    torch.manual_seed(0)
    net = EngineQNet(3, hw, 4, hidden, filters, R._ENGINE_HEAD[head]).cuda()
    qn = QNetInference(net, 80)
    with pytest.raises(N.SrlxError, match=limit):
        qn.enable_training(max_train)
    assert all(p.grad is None for p in net.parameters())  # nothing was allocated or launched ...
    g = (N.c_p * 12)(*[p.data_ptr() for p in net.kernel_parameters()])
    dq = torch.zeros((1, 3), device="cuda")
    off = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    ring = torch.zeros(hw[0] * hw[1], dtype=torch.uint8, device="cuda")
    with pytest.raises(N.SrlxError, match="srlx_qnet_enable_training first"):  # ... and the handle is not a training handle
        N.check(qn.lib.srlx_qnet_backward_u8(qn.h, 1, 1, N.c_p(ring.data_ptr()), N.tptr(off), N.tptr(dq), ctypes.cast(g, N.c_p), N.torch_stream_ptr()))
    x = torch.rand((2, 4) + hw, device="cuda")  # the forward pass of the same handle is served
    with torch.no_grad():
        _check_q(f"refusal {hw} f{filters} h{hidden} {head}: forward_f32 still served", qn.forward_f32(x), R.reference_q(net, x))


@pytest.mark.parametrize("mode", ["f32", "u8"])
def test_forward_refuses_a_batch_above_max_batch(mode):
    from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

    torch.manual_seed(0)
    net = EngineQNet(3, (20, 20), 4, 32).cuda()
    qn = QNetInference(net, 4)
    qbuf = torch.full((6, 3), SENTINEL, device="cuda")
    with pytest.raises(N.SrlxError, match="batch 5 exceeds max_batch 4"):
        if mode == "f32":
            qn.forward_f32(torch.rand((5, 4, 20, 20), device="cuda"), out=qbuf[:5])
        else:
            qn.forward_u8(torch.zeros(400, dtype=torch.uint8, device="cuda").data_ptr(), torch.zeros((5, 4), dtype=torch.int64, device="cuda"), out=qbuf[:5])
    torch.cuda.synchronize()
    assert bool((qbuf == SENTINEL).all())  # nothing was launched
