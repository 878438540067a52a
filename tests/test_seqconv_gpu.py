"""libsrlx's image block over float32 frame sequences (srlx_qnet_forward_convs_f32 / srlx_qnet_backward_convs_f32) against `DQNImageBlock` in
float64 on the CPU (tests/seqconv_reference.py).

Edges of the new kernels, each with a case on either side:
  * the weight-gradient partition (k_wgrad_seq): 256 parts; rows <= 256 -> one row per part, 257 -> two (129 parts), 512 | 513 -> three (171 parts);
    k_reduce_parts adds the parts in four slices: fewer parts than slices at rows = 1, 2
  * pixel pairs per MFMA: an odd pixel count per image (9, 25, 81, 121, 441) leaves half a step; an even one (4, 16, 36) does not
  * the eight-step fetch groups of the operand pipeline: 2 and 5 steps (< 8), exactly 8 (16 pixels: H = 16's conv1 and H = 24's conv2 output), 13 (> 8),
    18 (> 16: H = 24's conv1 output), 41, 61, 221
  * conv1's tiles of 32 taps: 2 C waves -- half a workgroup (C = 1), one (C = 2), one and a half (C = 3), two (C = 4)
  * the forward's 128-row GEMM tile over rows x pixels and the 64-row limit of srlx_qnet_enable_training: rows 63 | 64 | 65 and 130 at four pixels a row
  * ld_features / ld_grad: the feature count, and the feature count + 33 (odd: no row but the first is 16-byte aligned)
Every output and gradient buffer is followed by guard elements holding a pattern; the gradient rows' columns behind the features hold NaN."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

CASES = [(8, 1, r) for r in (1, 2, 63, 64, 65, 130, 256, 257, 512, 513)] + [(12, 1, 33), (16, 2, 3), (20, 3, 9), (24, 1, 2), (36, 1, 5), (84, 1, 3), (84, 4, 2)]
PATTERN = -7.25
NAMES = ("features", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")


def _trunk(H, C, scale, max_rows):
    import copy

    from seqconv_reference import block
    from simple_distributed_rl_amd.device.qnet import SeqImageTrunk

    blk = copy.deepcopy(block(H, C, scale)).cuda()
    return SeqImageTrunk(blk, (H, H), max_rows), blk


def _forward(trunk, frames, ld):
    """-> (features [rows][n], the whole buffer): rows + 2 rows of ld floats pre-filled with the pattern."""
    import torch

    from simple_distributed_rl_amd import _native as N

    rows = frames.shape[0]
    buf = torch.full((rows + 2, ld), PATTERN, dtype=torch.float32, device="cuda")
    N.check(trunk.lib.srlx_qnet_forward_convs_f32(trunk.h, rows, N.tptr(frames), N.tptr(buf), ld, N.torch_stream_ptr()))
    n = trunk.n_features
    assert bool((buf[:rows, n:] == PATTERN).all()) and bool((buf[rows:] == PATTERN).all()), "the forward wrote outside the features"
    return buf[:rows, :n].clone()


def _backward(trunk, frames, g, ld):
    """-> the six gradients as logical (torch-shaped) tensors; every raw buffer carries 64 guard floats."""
    import torch

    from simple_distributed_rl_amd import _native as N

    rows, n = g.shape
    gbuf = torch.full((rows + 2, ld), float("nan"), dtype=torch.float32, device="cuda")
    gbuf[:rows, :n] = g
    ps = trunk.params()
    raw = [torch.full((p.numel() + 64,), PATTERN, dtype=torch.float32, device="cuda") for p in ps]
    arr = (N.c_p * 6)(*[b.data_ptr() for b in raw])
    N.check(trunk.lib.srlx_qnet_backward_convs_f32(trunk.h, rows, N.tptr(frames), N.tptr(gbuf), ld, ctypes.cast(arr, N.c_p), N.torch_stream_ptr()))
    out = []
    for p, b in zip(ps, raw):
        assert bool((b[p.numel():] == PATTERN).all()), "a gradient kernel wrote behind its tensor"
        v = b[: p.numel()]
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():  # conv2 / conv3: [co][ky][kx][ci] memory
            co, ci, kh, kw = p.shape
            v = v.view(co, kh, kw, ci).permute(0, 3, 1, 2)
        out.append(v.reshape(p.shape).clone())
    return out


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("H,C,rows", CASES)
def test_seqconv_forward_backward_match_float64_reference(H, C, rows, scale):
    import torch

    from seqconv_reference import inputs, reference

    ref64, err32, zero_share = reference(H, C, rows, scale)
    assert all(0.2 <= z <= 0.8 for z in zero_share), zero_share  # every ReLU mask is exercised both ways
    frames, g = (t.cuda() for t in inputs(H, C, rows))
    trunk, _ = _trunk(H, C, scale, rows)
    plain, _ = _trunk(H, C, scale, rows)  # stays forward-only
    trunk.enable_training()
    n = trunk.n_features
    assert n == ref64[0].shape[1]
    results = []
    for ld in (n, n + 33):
        feats = _forward(trunk, frames, ld)
        grads = _backward(trunk, frames, g, ld)
        again = _backward(trunk, frames, g, ld)
        assert all(torch.equal(a, b) for a, b in zip(grads, again)), "two backward calls on the same data differ"
        assert torch.equal(feats, _forward(plain, frames, ld)), "a sequence-training handle and a forward-only handle differ"
        results.append([feats] + grads)
    assert all(torch.equal(a, b) for a, b in zip(*results)), "the row stride changed a result"
    other, _ = _trunk(H, C, scale, rows)
    other.enable_training()
    second = [_forward(other, frames, n)] + _backward(other, frames, g, n)
    assert all(torch.equal(a, b) for a, b in zip(results[0], second)), "a second handle differs"
    for name, got, ref, e32 in zip(NAMES, results[0], ref64, err32):
        err = float((got.double().cpu() - ref).abs().max())
        bound = max(1e-5 * float(ref.abs().max()), 2 * e32)
        print(f"H={H} C={C} rows={rows} x{scale} {name}: max|got - ref64| = {err:.3e}, bound = {bound:.3e} (max|ref| = {float(ref.abs().max()):.3e}, torch f32 = {e32:.3e})")
        assert err <= bound, (name, err, bound)


def test_seqconv_trunk_autograd_and_stale_backward():
    """SeqImageTrunk.features through autograd gives the entry points' gradients; a backward whose activations a later forward replaced raises."""
    import torch

    from seqconv_reference import inputs

    H, C, rows = 12, 1, 33
    frames, g = (t.cuda() for t in inputs(H, C, rows))
    trunk, blk = _trunk(H, C, 1, rows)
    y = trunk.features(frames)
    assert y.requires_grad and trunk.training_bytes > 0
    y.backward(g)
    want = _backward(trunk, frames, g, trunk.n_features)
    for p, w in zip(trunk.params(), want):
        assert torch.equal(p.grad, w)
    out = torch.full((rows, trunk.n_features + 5), PATTERN, device="cuda")
    y2 = trunk.features(frames, out=out)
    assert y2.data_ptr() == out.data_ptr() and torch.equal(y2[:, : trunk.n_features], y.detach()) and bool((y2[:, trunk.n_features:] == PATTERN).all())
    with torch.no_grad():
        trunk.features(frames)  # replaces the kept activations
    with pytest.raises(RuntimeError, match="another forward"):
        y2.backward(torch.zeros_like(y2))


def test_seqconv_byte_query_matches_allocation():
    import torch

    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.qnet import SeqImageTrunk

    lib = N.lib()
    for H, C, rows in ((8, 1, 130), (20, 3, 9), (84, 4, 64)):
        trunk, _ = _trunk(H, C, 1, rows)
        free0 = torch.cuda.mem_get_info()[0]
        trunk.enable_training()
        want = SeqImageTrunk.seq_training_bytes((H, H), C, 32, rows)
        print(f"H={H} C={C} rows={rows}: query {want} B, allocated {trunk.training_bytes} B, free memory fell by {free0 - torch.cuda.mem_get_info()[0]} B")
        assert want > 0 and trunk.training_bytes == want
    assert lib.srlx_qnet_seq_training_bytes(84, 84, 1, 32, 8192) > 0
    for bad in ((86, 86, 1, 32, 8), (84, 80, 1, 32, 8), (88, 88, 1, 32, 8), (4, 4, 1, 32, 8), (84, 84, 5, 32, 8), (84, 84, 0, 32, 8), (84, 84, 1, 64, 8), (84, 84, 1, 32, 0)):
        assert lib.srlx_qnet_seq_training_bytes(*bad) == -1, bad
    # a backward pass for other rows than the last forward's, and more rows than the scratch holds, are refused
    trunk, _ = _trunk(8, 1, 1, 4)
    trunk.enable_training()
    frames = torch.rand((4, 8, 8, 1), device="cuda")
    feats = torch.empty((4, trunk.n_features), device="cuda")
    N.check(lib.srlx_qnet_forward_convs_f32(trunk.h, 4, N.tptr(frames), N.tptr(feats), trunk.n_features, N.torch_stream_ptr()))
    arr = (N.c_p * 6)(*[torch.empty_like(p).data_ptr() for p in trunk.params()])
    assert lib.srlx_qnet_backward_convs_f32(trunk.h, 3, N.tptr(frames), N.tptr(feats), trunk.n_features, ctypes.cast(arr, N.c_p), N.torch_stream_ptr()) != 0
    assert lib.srlx_qnet_forward_convs_f32(trunk.h, 5, N.tptr(frames), N.tptr(feats), trunk.n_features, N.torch_stream_ptr()) != 0
    assert lib.srlx_qnet_forward_convs_f32(trunk.h, 4, N.tptr(frames), N.tptr(feats), trunk.n_features - 1, N.torch_stream_ptr()) != 0
