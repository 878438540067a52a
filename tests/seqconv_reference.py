"""The yardstick of tests/test_seqconv_gpu.py: `DQNImageBlock` (8x8/4, 4x4/2, 3x3/1 convolutions, replicate padding, ReLU) on the CPU with torch autograd, in
float64 (the reference) and in float32 (torch's own rounding error, which sets the slack term of the bound).  One result per case, computed once and shared."""
import copy
import functools

import torch

from simple_distributed_rl_amd.rl.torch_.networks import DQNImageBlock


@functools.lru_cache(maxsize=None)
def block(H: int, C: int, scale: int):
    """The block with torch's initialisation (seeded by the geometry), its convolution WEIGHTS times `scale`; float32, on the CPU."""
    torch.manual_seed(1000 * H + 10 * C)
    blk = DQNImageBlock((C, H, H), 32)
    with torch.no_grad():
        for conv in list(blk.image_layers)[0::2]:
            conv.weight.mul_(scale)
    return blk


@functools.lru_cache(maxsize=None)
def inputs(H: int, C: int, rows: int):
    """frames uniform in [0, 1) [rows][H][W][C]; g = randn at the features [rows][n_features]."""
    gen = torch.Generator().manual_seed(7 * H + 3 * C + rows)
    frames = torch.rand((rows, H, H, C), generator=gen, dtype=torch.float32)
    with torch.no_grad():
        n = block(H, C, 1)(torch.zeros((1, C, H, H))).flatten(1).shape[1]
    return frames, torch.randn((rows, n), generator=gen, dtype=torch.float32)


def _run(blk, frames, g, dtype):
    b = copy.deepcopy(blk).to(dtype)
    x = frames.permute(0, 3, 1, 2).to(dtype)
    zero_share = []
    for layer in b.image_layers:
        x = layer(x)
        if isinstance(layer, torch.nn.ReLU):
            zero_share.append(float((x == 0).double().mean()))
    y = x.flatten(1)
    y.backward(g.to(dtype))
    grads = [t.grad.detach() for conv in list(b.image_layers)[0::2] for t in (conv.weight, conv.bias)]
    return [y.detach()] + grads, zero_share


@functools.lru_cache(maxsize=None)
def reference(H: int, C: int, rows: int, scale: int):
    """(ref64, err32, zero_share): the seven tensors (features, conv1 w, b, conv2 w, b, conv3 w, b gradients) in float64, max |torch float32 on the CPU - ref64|
    of each, and each layer's share of zero activations in the float64 run."""
    frames, g = inputs(H, C, rows)
    ref64, zero_share = _run(block(H, C, scale), frames, g, torch.float64)
    got32, _ = _run(block(H, C, scale), frames, g, torch.float32)
    err32 = [float((a.double() - b).abs().max()) for a, b in zip(got32, ref64)]
    return ref64, err32, zero_share
