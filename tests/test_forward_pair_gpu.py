"""srlx_qnet_forward_pair_u8: the update's online pass and target pass as one chain of three launches (both convolution passes, both first dense layers, both heads
in one launch each).  Every workgroup runs the code of its own pass, so the bar is equality bit for bit with two srlx_qnet_forward_u8 calls: the Q rows, what a
backward pass behind the pair computes from the activations it kept, and the handles' next passes; outside its envelope the entry point launches nothing; and the
engine's lock-step with EngineSchedule.forward_pair computes what it computes without."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


class _DevView:
    """`n` elements of device memory at `ptr` as a tensor (torch.as_tensor reads __cuda_array_interface__)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


_ITEMS = {"act1": 0, "act2": 1, "act3": 2, "h1": 3, "planes": 4, "partial": 5, "wpack": 6, "w_t": 7, "w_t2": 8}


def _buf(h, name):
    """A handle's buffer as a tensor VIEW (srlx_qnet_inspect), or None where the handle owns none; the planes as int16 words."""
    from simple_distributed_rl_amd import _native as N

    ptr, n = N.c_p(), N.c_i64(0)
    N.check(h.lib.srlx_qnet_inspect(h.h, _ITEMS[name], ctypes.byref(ptr), ctypes.byref(n)))
    if not ptr.value:
        return None
    return torch.as_tensor(_DevView(ptr.value, n.value, "<i2" if name == "planes" else "<f4"), device="cuda")


def _flags(h):
    from simple_distributed_rl_amd import _native as N

    ptr, n, bits = N.c_p(), N.c_i64(0), ctypes.c_int(0)
    N.check(h.lib.srlx_qnet_inspect(h.h, 100, ctypes.byref(ptr), ctypes.byref(n)))
    N.check(h.lib.srlx_qnet_range_flags(h.h, ctypes.byref(bits)))
    return int(n.value), int(bits.value)


N1, FLAT, SLABS = 1024, 7744, 242  # first dense layer of the 84 x 84 x 4 network with 512 hidden units per stream: units, inputs (11 x 11 x 64), 32-deep K slabs
SPLITS = 32  # K splits a one-row-tile launch of this layer asks for (512 workgroups / 16 column tiles): 8 slabs each, so 31 of them own a K range


def _kept(h, rows):
    """Everything a `rows`-row forward pass leaves in a handle, cut to what the pass defines: activations and hidden layer of the rows, the operand planes' rows of
    every K slab (the launch pads to a 128-row tile; pad rows keep what they held), the partial sums' rows of every K split that owns a range, packed and transposed
    filters, host-side state and the range word."""
    out = {}
    for name in ("act1", "act2", "act3", "h1"):
        t = _buf(h, name)
        if t is not None:
            out[name] = t.view(128, -1)[:rows].clone()
    out["planes"] = _buf(h, "planes").view(SLABS, 128, 64)[:, :rows].clone()
    used = -(-SLABS // -(-SLABS // SPLITS))
    out["partial"] = _buf(h, "partial")[: used * 128 * N1].view(used, 128, N1)[:, :rows].clone()
    for name in ("wpack", "w_t", "w_t2"):
        t = _buf(h, name)
        if t is not None:
            out[name] = t.clone()
    out["state"] = torch.tensor(_flags(h))
    return out


def _poison(h):
    """Every buffer a forward pass writes, filled with a value no pass produces (NaN; the planes 0x7e7e = a float16 NaN)."""
    for name in ("act1", "act2", "act3", "h1", "partial"):
        t = _buf(h, name)
        if t is not None:
            t.fill_(float("nan"))
    _buf(h, "planes").fill_(0x7E7E)


@pytest.fixture(scope="module")
def pair():
    """Two networks, 128 frame stacks for each (one with an episode start), and TWO identically built pairs of handles on them -- an online training handle that reads a
    published set's operand planes and a target handle with planes of its own (what the fast lock-step builds): `ref` only ever runs forward_u8, `on` / `tg` run the
    pair from a poisoned state."""
    from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

    nets = []
    for seed in (21, 22):
        torch.manual_seed(seed)
        nets.append(EngineQNet(6, (84, 84), 4, 512, 32, "average").cuda())
    g = torch.Generator(device="cuda").manual_seed(3)
    F = 84 * 84
    ring = torch.randint(0, 256, (300 * F,), dtype=torch.uint8, device="cuda", generator=g)
    off_a = torch.randint(0, 300, (128, 4), device="cuda", generator=g) * F
    off_b = torch.randint(0, 300, (128, 4), device="cuda", generator=g) * F
    off_a[1, :3] = -1  # an episode start: zero history
    actor = QNetInference(nets[0], 512, 0)
    actor.enable_fc1_planes(private_weights=True)
    actor.enable_actor_sets()

    def handles():
        on = QNetInference(nets[0], 128, 0).enable_training(32)
        on.publish_to(actor, 1, with_fc1=True)
        on.enable_fc1_planes(private_weights=False)
        on.set_planes_small(True, actor.set_planes_ptr(1))
        tg = QNetInference(nets[1], 128, 0)
        tg.enable_fc1_planes(private_weights=True)
        tg.set_planes_small(True, None)
        tg.refresh_own_planes()
        tg.set_pack_sticky(True)
        return on, tg

    (on, tg), (on_ref, tg_ref) = handles(), handles()
    torch.cuda.synchronize()
    return dict(on=on, tg=tg, on_ref=on_ref, tg_ref=tg_ref, actor=actor, ring=ring, off_a=off_a, off_b=off_b)


def _backward(on, ring, off, rows):
    """Gradients of a backward pass over the first min(rows, 32) strided rows, read from the HANDLE's gradient tensors (two training handles share one network)."""
    B = min(rows, 32)
    stride = rows // B
    dq = torch.randn((B, 6), device="cuda", generator=torch.Generator(device="cuda").manual_seed(rows))
    for t in on._grads:
        t.fill_(float("nan"))
    on.backward_u8(ring.data_ptr(), off, dq, sample_stride=stride)
    torch.cuda.synchronize()
    return [t.detach().clone() for t in on._grads]


def _pair_against_reference(pair, ra, rb, with_backward):
    from simple_distributed_rl_amd.device.qnet import forward_pair_u8

    on, tg, on_ref, tg_ref, ring = pair["on"], pair["tg"], pair["on_ref"], pair["tg_ref"], pair["ring"]
    off_a, off_b = pair["off_a"][:ra].contiguous(), pair["off_b"][:rb].contiguous()
    # the reference: two forward_u8 calls on handles of their own, from a poisoned state too (what a pass does not define is cut away by _kept)
    for h in (on_ref, tg_ref, on, tg):
        _poison(h)
    want_a = on_ref.forward_u8(ring.data_ptr(), off_a).clone()
    want_b = tg_ref.forward_u8(ring.data_ptr(), off_b).clone()
    torch.cuda.synchronize()
    want_kept = _kept(on_ref, ra), _kept(tg_ref, rb)
    qa = torch.full((ra, 6), SENTINEL, device="cuda")
    qb = torch.full((rb, 6), SENTINEL, device="cuda")
    assert forward_pair_u8(on, off_a, tg, off_b, ring.data_ptr(), out_a=qa, out_b=qb) is not None, "the pair is inside the envelope"
    torch.cuda.synchronize()
    got_kept = _kept(on, ra), _kept(tg, rb)
    assert torch.equal(qa, want_a) and torch.equal(qb, want_b)
    assert torch.isfinite(want_a).all() and float(want_a.abs().max()) > 0 and not torch.equal(want_a[:1], want_b[:1])
    for which, (want, got) in enumerate(zip(want_kept, got_kept)):
        assert set(want) == set(got) and {"act3", "planes", "partial", "wpack", "state"} <= set(got), which
        for name in want:
            w, g = want[name], got[name]
            if w.is_floating_point():  # bit patterns: what a pass does not write (act1 / act2 of the target handle, which keeps none) is the poison in both
                w, g = w.view(torch.int32), g.view(torch.int32)
            assert torch.equal(w, g), (which, name)
        for name in ("act3", "partial") + (("act1", "act2", "h1") if which == 0 else ()):
            assert not bool(torch.isnan(got[name]).any()), (which, name)  # (every element the pass defines was written)
    assert {"act1", "act2", "h1", "w_t", "w_t2"} <= set(got_kept[0])  # the training handle keeps what its backward pass reads
    if with_backward:
        want_g, got_g = _backward(on_ref, ring, off_a, ra), _backward(on, ring, off_a, ra)
        for k, (x, y) in enumerate(zip(want_g, got_g)):
            assert torch.equal(x, y) and not bool(torch.isnan(y).any()), k
        assert torch.equal(on.forward_u8(ring.data_ptr(), off_a), want_a) and torch.equal(tg.forward_u8(ring.data_ptr(), off_b), want_b)


@pytest.mark.parametrize("rows", [(128, 96), (1, 1), (33, 128), (5, 3)], ids=lambda r: f"{r[0]}+{r[1]}")
def test_pair_equals_two_forward_passes(pair, rows):
    """The pair on poisoned handles against two forward_u8 calls on a second, identically built pair of handles: Q rows, act1 / act2 / act3 and the hidden layer of
    the training handle, both handles' activation planes, partial sums, packed and transposed filters, range word and host-side state (wt_from_forward, pack and
    plane validity) -- then the gradients of a backward pass behind each, and each handle's own next pass."""
    from simple_distributed_rl_amd.device.qnet import check_ranges

    _pair_against_reference(pair, rows[0], rows[1], True)
    check_ranges()


@pytest.mark.parametrize("ra", [31, 64, 65, 128])
def test_every_row_tile_combination_of_the_first_dense_layer(pair, ra):
    """k_fc1_planes_rows_pair<RTA, RTB> is instantiated for 1..4 row tiles of 32 on either side: all sixteen, at tile edges, with the same comparison."""
    for rb in (1, 33, 96, 97):
        _pair_against_reference(pair, ra, rb, False)


def test_outside_the_envelope_nothing_is_launched(pair):
    """A target handle whose small passes are not on operand planes: "not applicable", both output buffers untouched, both handles' next passes unchanged."""
    from simple_distributed_rl_amd.device.qnet import forward_pair_u8

    on, tg, ring = pair["on"], pair["tg"], pair["ring"]
    off_a, off_b = pair["off_a"], pair["off_b"][:96].contiguous()
    want_a, want_b = on.forward_u8(ring.data_ptr(), off_a).clone(), tg.forward_u8(ring.data_ptr(), off_b).clone()
    qa = torch.full((128, 6), SENTINEL, device="cuda")
    qb = torch.full((96, 6), SENTINEL, device="cuda")
    tg.set_planes_small(False, None)
    try:
        assert forward_pair_u8(on, off_a, tg, off_b, ring.data_ptr(), out_a=qa, out_b=qb) is None
        assert forward_pair_u8(on, off_a, on, off_a, ring.data_ptr(), out_a=qa, out_b=qa) is None  # (one handle twice)
        torch.cuda.synchronize()
        assert bool((qa == SENTINEL).all()) and bool((qb == SENTINEL).all())
        assert torch.equal(on.forward_u8(ring.data_ptr(), off_a), want_a) and torch.equal(tg.forward_u8(ring.data_ptr(), off_b), want_b)
    finally:
        tg.set_planes_small(True, None)
    assert forward_pair_u8(on, off_a, tg, off_b, ring.data_ptr(), out_a=qa, out_b=qb) is not None
    assert torch.equal(qa, want_a) and torch.equal(qb, want_b)


def _tree(eng):
    from simple_distributed_rl_amd import _native as N

    r = eng.replay
    tree = np.empty(2 * r.capacity - 1)
    N.check(r.lib.srlx_per_backup(r.h_per, ctypes.byref(N.c_f64(0)), ctypes.byref(N.c_i64(0)), ctypes.byref(N.c_i64(0)), N.np_ptr(tree)))
    return tree


def test_engine_lockstep_with_and_without_the_pair_forward():
    """RainbowEngine at 512 environments (the smallest the fast lock-step takes), six updating lock-steps, eager and then captured: EngineSchedule.forward_pair on
    against off -- online weights, loss, TD targets, priorities and the replay tree bit-equal throughout."""
    from simple_distributed_rl_amd.device.rainbow import EngineSchedule, RainbowDeviceConfig, RainbowEngine

    E = 512
    cfg = RainbowDeviceConfig(n_envs=E, batch_size=32, memory_capacity=E * 12, memory_warmup_size=E * 4, target_model_update_interval=5, lr=1e-4, seed=3)
    arms = [EngineSchedule(forward_pair=False), EngineSchedule(forward_pair=True)]
    engs = [RainbowEngine(dataclasses.replace(cfg, schedule=s), 0, episode_len=7, overlap=True, fast=True) for s in arms]
    ref = engs[0]
    assert not ref._forward_pair and engs[1]._forward_pair
    for k in range(11):
        if k == 8:
            for e in engs:
                e.capture_graphs()
        for e in engs:
            e.step(1)
        torch.cuda.synchronize()
        want_tree = _tree(ref)
        for j, e in enumerate(engs[1:]):
            assert e.train_count == ref.train_count
            assert torch.equal(e.loss, ref.loss) and torch.equal(e.target, ref.target) and torch.equal(e.priorities, ref.priorities), (k, j)
            for (name, p), q in zip(ref.q_online.named_parameters(), e.q_online.parameters()):
                assert torch.equal(p, q), (k, j, name)
            assert (_tree(e) == want_tree).all(), (k, j)
    assert ref.train_count >= 6
    # the pair forward was really what ran: every update issued behind a publishing update (all but the first eager one, and the captured variants) took it
    assert ref._pair_applied == 0 and engs[1]._pair_applied >= 4, engs[1]._pair_applied
    with pytest.raises(ValueError, match="forward_pair"):
        RainbowEngine(dataclasses.replace(cfg, schedule=EngineSchedule(forward_pair=True, learner_planes=False)), 0, episode_len=7, overlap=True, fast=True)
