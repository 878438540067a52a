"""Yardstick and case tables of the image Q-network envelope tests (tests/test_qnet_envelope_cpu.py, tests/test_qnet_envelope_gpu.py).  Nothing here needs a GPU.

`reference_q` / `reference_grads`: float64 Q-values and gradients on the CPU.  The Q-values come from the REFERENCE-LAYOUT network
(rl/torch_/networks.py:atari_qnetwork, or algorithms/dqn.py:build_qnetwork for the plain head) loaded with `EngineQNet.reference_state_dict()`, so every case also
pins the kernel-friendly parameter layout to the reference's at its own shape.  The gradients come from autograd through a float64 CPU copy of the `EngineQNet`
(its parameters ARE the kernels' layouts); the CPU test asserts that this copy's forward equals `reference_q` to float64 round-off at every case.

`randomise`: parameters of both signs with non-zero biases, every hidden layer's pre-activations of unit variance, Q-values O(1) -- the default initialisation gives
max |Q| of about 0.07 and biases of zero, on which a wrong bias barely shows.

`dispatch_classes`: a pure-Python MIRROR of the kernels' dispatch rules (which conv1 kernel, which GEMM tile, how many K splits, which head template ...).  It is a
mirror, not the dispatch: whoever changes a rule in csrc/srlx_qnet.hip or csrc/srlx_qnet_bwd.hip updates it here, or the coverage test of
tests/test_qnet_envelope_cpu.py vouches for classes the kernels no longer take."""
import collections
import copy
import functools
import types

import torch
import torch.nn as nn

Case = collections.namedtuple("Case", "hw window filters hidden A head batches max_batch purpose")
BackwardCase = collections.namedtuple("BackwardCase", "side window hidden A head B stride")

_ENGINE_HEAD = {"average": "average", "max": "max", "naive": "", "plain": "plain"}  # EngineQNet's dueling_type strings (device/qnet.py:_DUELING)

# Forward cases: each runs forward_f32 AND forward_u8 (the float stack is the stack of the same bytes) at every batch of `batches` on ONE handle of
# `max_batch` rows.  The first nine rows are the table this suite was specified with; the rest reach the split regimes, head templates and conv1 kernels the nine leave out.
FORWARD_CASES = [
    Case((8, 8), 1, 32, 32, 1, "average", (1, 3), 3, "every lower bound; 8 splits"),
    Case((84, 84), 4, 128, 512, 32, "max", (8,), 8, "upper filters and actions; conv3 K = 2304; value stream in lane 32; 32 splits"),
    Case((84, 84), 4, 64, 256, 17, "naive", (37,), 37, "C = 64 and 128; 33 splits (the partial buffer's cap at a small max_batch)"),
    Case((84, 84), 4, 32, 512, 6, "average", (210, 211, 256, 257), 257, "the 200-workgroup tile boundary; both head block sizes; the fused kernel for uint8"),
    Case((44, 20), 3, 32, 64, 9, "average", (5,), 7, "taller than wide, odd window; 18 used of 33 splits; B < max_batch"),
    Case((21, 37), 2, 64, 96, 16, "plain", (6,), 6, "odd sides, W % 4 != 0, odd byte offsets"),
    Case((96, 88), 4, 32, 64, 8, "max", (3,), 3, "larger than the LDS staging admits"),
    Case((36, 36), 8, 32, 160, 8, "plain", (4,), 4, "K = 512"),
    Case((20, 20), 4, 32, 960, 8, "average", (129, 200, 256, 257), 257, "9 splits at 129..256 rows, 6 at 257; k_conv1_u8 with one and two workgroups per sample"),
    Case((24, 56), 1, 32, 32, 16, "average", (3,), 3968, "64 splits: needs max_batch >= 3968"),
    Case((44, 44), 2, 32, 32, 32, "plain", (5,), 4000, "36 splits: the 33..64 loop with a remainder; plain head with 32 actions"),
    Case((8, 8), 2, 32, 64, 1, "plain", (2,), 2, "plain head with one action"),
    Case((12, 16), 1, 32, 32, 9, "plain", (3,), 3, "plain head with 9 actions"),
    Case((8, 8), 1, 32, 160, 17, "plain", (256, 257), 257, "plain head with 17 actions; both plain-head block sizes"),
    Case((84, 20), 4, 32, 32, 3, "naive", (199, 200), 200, "k_conv1_u8 on a frame taller than wide, both grid heights"),
    Case((20, 84), 4, 32, 64, 5, "plain", (199, 200), 200, "k_conv1_u8 on a frame wider than tall, both grid heights"),
]

# Backward cases (square frames, 32 filters): forward_u8 over B * stride rows, then backward_u8 for rows 0, stride, 2 stride, ...
BACKWARD_CASES = [
    BackwardCase(8, 1, 32, 1, "average", 1, 1),  # every lower bound (OH1 = 2)
    BackwardCase(84, 4, 512, 32, "plain", 64, 1),  # every upper bound
    BackwardCase(44, 8, 64, 17, "naive", 33, 2),  # first batch of the split FC1 data gradient
    BackwardCase(12, 3, 96, 9, "average", 31, 3),  # odd OH1 = 3, odd window
    BackwardCase(36, 2, 480, 16, "naive", 32, 1),  # last batch of the matrix-core FC1 data gradient
    BackwardCase(20, 4, 32, 8, "plain", 7, 4),  # plain head away from 84
]


def case_id(c):
    if isinstance(c, BackwardCase):
        return f"{c.side}x{c.side}-w{c.window}-h{c.hidden}-A{c.A}-{c.head}-B{c.B}-s{c.stride}"
    return f"{c.hw[0]}x{c.hw[1]}-w{c.window}-f{c.filters}-h{c.hidden}-A{c.A}-{c.head}"


def as_forward(c):
    """A backward case as the forward launch it starts with: one batch of B * stride rows on a handle of exactly that many."""
    if isinstance(c, Case):
        return c
    return Case((c.side, c.side), c.window, 32, c.hidden, c.A, c.head, (c.B * c.stride,), c.B * c.stride, "backward")


# ---- the dispatch mirror ---------------------------------------------------------------------------------------------------------------------------------------
def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1  # srlx_qnet.hip:912


def geometry(hw, filters):
    """(OH1, OW1, OH2, OW2, OH3, OW3, flat) as srlx_qnet_create computes them (srlx_qnet.hip:1071-1074)."""
    oh1, ow1 = conv_out(hw[0], 8, 4, 3), conv_out(hw[1], 8, 4, 3)
    oh2, ow2 = conv_out(oh1, 4, 2, 2), conv_out(ow1, 4, 2, 2)
    oh3, ow3 = conv_out(oh2, 3, 1, 1), conv_out(ow2, 3, 1, 1)
    return oh1, ow1, oh2, ow2, oh3, ow3, oh3 * ow3 * 2 * filters


def fc1_splits(flat, hidden, B, max_batch):
    """(splits asked for, splits that own a K range) of srlx_qnet_dense_rows (srlx_qnet.hip:956-971) for a handle without operand planes."""
    n1 = 2 * hidden
    tiles = -(-B // 128) * -(-n1 // 64)
    splits = -(-512 // tiles)
    ksteps = flat // 32
    splits = min(splits, ksteps, 64)  # (max_splits = 64: srlx_qnet.hip:1076)
    partial_floats = (4096 + 128 + max_batch) * n1  # srlx_qnet.hip:1087
    splits = max(min(splits, partial_floats // (-(-B // 128) * 128 * n1)), 1)
    kps = -(-ksteps // splits)
    return splits, -(-ksteps // kps)


def gemm_tile(M, N):
    """Row tile of launch_gemm<.., BN = 64, ..> (srlx_qnet.hip:915-928): 64 rows while fewer than 200 workgroups of 128 rows would exist."""
    return 64 if -(-M // 128) * -(-N // 64) < 200 else 128


def conv1_path_u8(hw, window, filters, B):
    """forward_u8_impl (srlx_qnet.hip:1441-1461); the process-wide switch that turns the fused kernel off is not mirrored (the tests leave it alone)."""
    oh1, ow1 = geometry(hw, filters)[:2]
    if hw == (84, 84) and window == 4 and filters == 32:
        return "fused"
    if filters == 32 and window == 4 and 4 * (oh1 - 1) + 8 <= 88 and 4 * (ow1 - 1) + 8 <= 88 and hw[1] % 4 == 0:
        return "k_conv1_u8/y2" if B < 200 else "k_conv1_u8/y1"
    return "AU8"


def used_regime(used):
    """The reduction path k_head takes over `used` split slabs (srlx_qnet.hip:584-613): rounds of eight plus a remainder up to 8, the unrolled path for 9..32,
    rounds of eight plus a remainder again for 33..64 (k_head_plain always takes rounds of eight plus a remainder)."""
    if used < 8:
        return "<8"
    if used in (8, 9, 33, 64):
        return str(used)
    if used in (31, 32):
        return "31|32"
    if used < 31:
        return "10..30"
    return "34..63/multiple-of-8" if used % 8 == 0 else "34..63/remainder"


def dispatch_classes(case):
    """What the kernels' dispatch does with `case` (a Case: over forward_f32 and forward_u8 at every batch; a BackwardCase: its forward_u8 and backward_u8), as a
    dict of sets:
      conv1       "fused" | "k_conv1_u8/y1" | "k_conv1_u8/y2" | "AU8" | "ANchw"           forward_u8_impl, srlx_qnet_forward_f32 (srlx_qnet.hip:1441-1461, 1507-1517)
      conv_tile   ("conv2" | "conv3", 64 | 128, B) where run_tail runs                    launch_gemm (srlx_qnet.hip:915-928, 933-946)
      used        regime of the split count the head reduces (`used_regime`)             srlx_qnet_dense_rows (srlx_qnet.hip:956-971), k_head (:584-613)
      splits      (splits, used, B) as computed                                           the same
      head_block  (threads, B) where the first dense layer is wider than 256 units       srlx_qnet.hip:998 (dueling: hidden > 256), :1006 (plain: 2 hidden > 256)
      amax        8 | 16 | 32, the head template                                         srlx_qnet.hip:1005-1018
      actions     (A, "dueling" | "plain")
      head        "average" | "max" | "naive" | "plain"
      fc1_dgrad   "mfma" (B <= 32) | "split", backward cases only                        backward_impl (srlx_qnet_bwd.hip:1006, 1050-1056)
    THIS IS A MIRROR: it must be updated together with the dispatch it copies."""
    f = as_forward(case)
    oh1, ow1, oh2, ow2, oh3, ow3, flat = geometry(f.hw, f.filters)
    out = collections.defaultdict(set)
    for B in f.batches:
        modes = ("u8",) if isinstance(case, BackwardCase) else ("f32", "u8")
        for mode in modes:
            path = "ANchw" if mode == "f32" else conv1_path_u8(f.hw, f.window, f.filters, B)
            out["conv1"].add(path)
            if path != "fused":  # run_tail: conv2 and conv3 as implicit GEMMs
                out["conv_tile"].add(("conv2", gemm_tile(B * oh2 * ow2, 2 * f.filters), B))
                out["conv_tile"].add(("conv3", gemm_tile(B * oh3 * ow3, 2 * f.filters), B))
        splits, used = fc1_splits(flat, f.hidden, B, f.max_batch)
        out["used"].add(used_regime(used))
        out["splits"].add((splits, used, B))
        wide = (2 * f.hidden if f.head == "plain" else f.hidden) > 256
        if wide:
            out["head_block"].add((512 if B <= 256 else 256, B))
    out["amax"].add(8 if f.A <= 8 else (16 if f.A <= 16 else 32))
    out["actions"].add((f.A, "plain" if f.head == "plain" else "dueling"))
    out["head"].add(f.head)
    if isinstance(case, BackwardCase):
        out["fc1_dgrad"].add("mfma" if case.B <= 32 else "split")
    return dict(out)


# ---- networks, inputs, yardstick -------------------------------------------------------------------------------------------------------------------------------
def reference_network(net):
    """The reference-layout module tree of `net`'s shape in float64 on the CPU, holding `net`'s parameters (through `reference_state_dict`)."""
    if net.plain:  # DQN's tree: in_block -> hidden_block (one ReLU layer of 2 * hidden units) -> out_layer
        from simple_distributed_rl_amd.algorithms.dqn import build_qnetwork
        from simple_distributed_rl_amd.base.define import SpaceTypes
        from simple_distributed_rl_amd.base.spaces.box import BoxSpace
        from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
        from simple_distributed_rl_amd.rl.models.config import HiddenBlockConfig, InputBlockConfig

        cfg = types.SimpleNamespace(input_block=InputBlockConfig(), hidden_block=HiddenBlockConfig().set((2 * net.hidden,)),
                                    observation_space=BoxSpace((net.hw[0], net.hw[1], net.window), 0, 1, stype=SpaceTypes.IMAGE_MAP),
                                    action_space=DiscreteSpace(net.n_actions))
        cfg.input_block.image.set_dqn_block(filters=net.filters)
        ref = build_qnetwork(cfg)
    else:
        from simple_distributed_rl_amd.rl.torch_.networks import atari_qnetwork

        ref = atari_qnetwork(net.n_actions, net.hw, net.window, net.hidden, False, net.filters, net.dueling_type)
    ref.load_state_dict({k: v.detach().cpu() for k, v in net.reference_state_dict().items()})
    return ref.double()


def reference_q(net, x_nchw):
    """float64 Q-values [rows][A] of the reference-layout network with `net`'s parameters, on the CPU."""
    with torch.no_grad():
        return reference_network(net)(x_nchw.detach().cpu().double(), channels_first=True)


def relu_zero_fractions(net, x_nchw):
    """{ReLU module name: fraction of its outputs that are zero} of the reference-layout network on `x_nchw` (float64)."""
    ref, out, hooks = reference_network(net), {}, []
    for name, mod in ref.named_modules():
        if isinstance(mod, nn.ReLU):
            hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: out.__setitem__(name, float((o == 0).double().mean()))))
    with torch.no_grad():
        ref(x_nchw.detach().cpu().double(), channels_first=True)
    for h in hooks:
        h.remove()
    return out


def engine_copy64(net):
    """A float64 CPU copy of the EngineQNet (the kernels' parameter layouts; carries the autograd of `reference_grads`)."""
    return copy.deepcopy(net).cpu().double()


def reference_grads(net, x_nchw, grad_q, rows):
    """float64 gradients of sum(q[rows] * grad_q) in the order and layouts of `net.kernel_parameters()`; a tensor no Q-value depends on (the plain head's unused
    v2 entries) gets zeros."""
    n64 = engine_copy64(net)
    n64.zero_grad(set_to_none=True)
    q = n64(x_nchw.detach().cpu().double())
    (q[list(rows)] * grad_q.detach().cpu().double()).sum().backward()
    return [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in n64.kernel_parameters()]


def make_inputs(hw, window, rows, seed, n_frames=61):
    """A uint8 frame ring [n_frames][H][W], the byte offsets [rows][window] of the sampled frames (about 10 % are -1: zero history; the first slot samples the
    ring's first frame and the last slot its last) and the float32 stack [rows][window][H][W] = bytes / 255 a frame store would hand out."""
    g = torch.Generator().manual_seed(seed)
    ring = torch.randint(0, 256, (n_frames, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    sel = torch.randint(0, n_frames, (rows, window), generator=g)
    zero = torch.rand((rows, window), generator=g) < 0.1
    sel.view(-1)[0], zero.view(-1)[0] = 0, False
    sel.view(-1)[-1], zero.view(-1)[-1] = n_frames - 1, False
    off = sel * (hw[0] * hw[1])
    off[zero] = -1
    x = ring[sel].float() / 255
    x[zero] = 0.0
    return types.SimpleNamespace(ring=ring, off=off.to(torch.int64), x=x)


def randomise(net, seed):
    """In place: every convolution filter and first-dense-layer row is Gaussian with zero sum (a unit's pre-activation is then symmetric about its bias whatever the
    input's mean, so about half of every ReLU's outputs are zero), scaled to unit pre-activation variance on a probe batch of random frames, with biases
    N(0, 0.5^2).  The second layers: Gaussian weights that give the value and every advantage a spread of 0.5 over the hidden layer, biases of either sign with
    1 <= |b| <= 2 -- so Q-values are O(1) also where a case has a single one (one action, one row), and float32 rounding of the long sums below (about 4e-7 rms
    per unit-variance layer in torch on the CPU, measured) stays under 1e-6 of max |Q|.  The scale is chosen here on the CPU: tests/test_qnet_envelope_cpu.py
    asserts at every case that between 20 % and 80 % of each layer's reference activations are zero and that float32 torch is within 1e-6 max |Q| of float64
    (measured 1.5e-7 .. 8.9e-7; the largest at 128 filters, where conv3 sums 2304 and the first dense layer 30 976 products)."""
    g = torch.Generator().manual_seed(seed)
    x = make_inputs(net.hw, net.window, 4, seed + 1).x

    def fill(mod, inp):
        w = torch.randn(mod.weight.shape, generator=g)
        w = w - w.flatten(1).mean(1).view(-1, *([1] * (w.dim() - 1)))
        mod.weight.copy_(w)
        mod.bias.zero_()
        mod.weight.div_(mod(inp).std())
        mod.bias.copy_(0.5 * torch.randn(mod.bias.shape, generator=g))
        return torch.relu(mod(inp))

    with torch.no_grad():
        a = fill(net.conv3, fill(net.conv2, fill(net.conv1, x)))
        h = fill(net.fc1, a.permute(0, 2, 3, 1).flatten(1))
        heads = [(net.out_layer, h)] if net.plain else [(net.v2, h[:, : net.hidden]), (net.a2, h[:, net.hidden :])]
        for lin, inp in heads:
            lin.weight.copy_(0.5 * torch.randn(lin.weight.shape, generator=g) / float((inp * inp).sum(1).mean().sqrt()))
            sign = 2.0 * (torch.rand(lin.bias.shape, generator=g) < 0.5).float() - 1.0
            lin.bias.copy_(sign * (1.0 + torch.rand(lin.bias.shape, generator=g)))  # 1 <= |b| <= 2: a case with a single Q-value is O(1) too
    net._bump_version()
    return net


# A ReLU unit whose pre-activation is closer to zero than float32 evaluates it may be on in the kernels and off in the float64 reference (or the reverse); its whole
# gradient contribution -- one convolution unit reaches a bias entry and every tap of its filter -- then differs, which no tolerance on the gradients covers (it is the
# size of a gradient term, not of a rounding error).  Torch's float32 pre-activations of these unit-variance layers are within 4e-7 rms of float64 (measured, all
# layers); the training rows of a backward case are therefore drawn until no unit is within five times that of its kink.  A property of the test data, checked
# in float64 on the CPU (tests/test_qnet_envelope_cpu.py asserts it); the largest case has 2 M units and needs about thirty draws.
KINK_MARGIN = 2e-6


def kink_margin(net, x_nchw):
    """The smallest |pre-activation| over every ReLU unit of the float64 network on these rows."""
    n64 = engine_copy64(net)
    with torch.no_grad():
        z1 = n64.conv1(x_nchw.double())
        z2 = n64.conv2(torch.relu(z1))
        z3 = n64.conv3(torch.relu(z2))
        zf = n64.fc1(torch.relu(z3).permute(0, 2, 3, 1).flatten(1))
    return min(float(z.abs().min()) for z in (z1, z2, z3, zf))


@functools.lru_cache(maxsize=None)
def build(case):
    """(randomised EngineQNet on the CPU, inputs for the case's largest batch) -- cached: the tests of a case share them and leave them unchanged."""
    from simple_distributed_rl_amd.device.qnet import EngineQNet

    f = as_forward(case)
    seed = 1000 + (FORWARD_CASES.index(case) if isinstance(case, Case) else 100 + BACKWARD_CASES.index(case))
    torch.manual_seed(seed)
    net = randomise(EngineQNet(f.A, f.hw, f.window, f.hidden, f.filters, _ENGINE_HEAD[f.head]), seed)
    if isinstance(case, Case):
        return net, make_inputs(f.hw, f.window, max(f.batches), seed + 7)
    for draw in range(1000):
        inp = make_inputs(f.hw, f.window, max(f.batches), seed + 7 + 1000 * draw)
        if kink_margin(net, inp.x[:: case.stride]) >= KINK_MARGIN:
            return net, inp
    raise RuntimeError(f"{case_id(case)}: no draw of the inputs keeps every ReLU unit {KINK_MARGIN} away from its kink")


@functools.lru_cache(maxsize=None)
def build_reference_q(case):
    """reference_q at the case's largest batch (rows are independent: a smaller batch is its first rows)."""
    net, inp = build(case)
    return reference_q(net, inp.x)
