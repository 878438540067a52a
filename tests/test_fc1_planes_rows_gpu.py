"""The learner's first dense layer on float16 operand planes (srlx_fc1_planes.hip: k_fc1_planes_rows, one row tile of <= 128 rows) against the staging-split GEMM
(k_gemm_s16<APlain, .., H16>): the same K split, k order and partial-product order, so every comparison here is bit for bit."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 32, 33, 96, 128]  # one lane of a tile, a whole tile, one row into the second, the target pass (a dead fourth tile), the online pass

# (frame side, filters, hidden) -> K-slabs of 32 and what the split count of srlx_qnet_dense_rows makes of them
GEOMETRIES = {
    "workload": (84, 32, 512),  # flat 7744 = 242 slabs, N1 = 1024: 32 splits asked, 8 slabs each -> 31 used, the last one 2 slabs short of the others' 8
    "small": (16, 32, 64),  # flat 576 = 18 slabs, N1 = 128 (ONE column tile): 256 splits asked, more than there are slabs -> 18 splits of one slab
    "long": (96, 32, 512),  # flat 10816 = 338 slabs, N1 = 1024: 11 slabs per split (more than the eight a wave holds: weight reloads, a second trip), last split 8
}


def _net(side, filters, hidden, seed=7):
    from simple_distributed_rl_amd.device.qnet import EngineQNet

    torch.manual_seed(seed)
    net = EngineQNet(6, (side, side), 4, hidden, filters, "average").cuda()
    with torch.no_grad():
        net.a2.bias.add_(torch.tensor([0.0, 0.3, 0.0, 0.3, -0.1, 0.2], device="cuda"))
    return net


def _frames(rows, side, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    px = side * side
    ring = torch.randint(0, 256, (rows * 4, px), dtype=torch.uint8, device="cuda", generator=g)
    off = (torch.arange(rows * 4, dtype=torch.int64, device="cuda") * px).view(rows, 4).clone()
    if rows > 1:
        off[1, :3] = -1  # an episode start: zero history
    return ring, off


@pytest.fixture(scope="module")
def nets():
    """One network per geometry, the staging-split Q rows of 128 frame stacks (computed once, never written again) and, for the workload geometry, an actor handle
    whose published set 1 holds the network's first dense layer as operand planes."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    out = {}
    for name, (side, filters, hidden) in GEOMETRIES.items():
        net = _net(side, filters, hidden)
        ring, off = _frames(128, side)
        ref = QNetInference(net, 128, 0)
        actor = None
        if name == "workload":
            actor = QNetInference(net, 512, 0)
            actor.enable_fc1_planes(private_weights=True)
            actor.enable_actor_sets()
            ref.publish_to(actor, 1, with_fc1=True)
        out[name] = dict(net=net, ring=ring, off=off, ref=ref, actor=actor)
    torch.cuda.synchronize()
    return out


def _want(g, rows):
    """The staging-split GEMM's Q rows of the first `rows` frame stacks: a launch of exactly `rows` rows (the split count depends on the launch, not on the handle)."""
    return g["ref"].forward_u8(g["ring"].data_ptr(), g["off"][:rows].contiguous()).clone()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_rows_kernel_equals_the_staging_split_gemm(nets, geometry, rows):
    """Q rows of a `rows`-row pass with srlx_qnet_set_planes_small -- the handle's own planes, and (workload geometry) an actor set's borrowed ones -- equal the
    staging-split GEMM's bit for bit; switched off again, the handle is back on that GEMM.  The three geometries cover a short last split, more splits asked than
    slabs exist, one and eight column tiles, and splits longer than the eight slabs of weight a wave holds in registers."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    g = nets[geometry]
    off = g["off"][:rows].contiguous()
    want = _want(g, rows)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    own = QNetInference(g["net"], rows, 0)
    own.enable_fc1_planes(private_weights=True)
    own.set_planes_small(True, None)
    own.refresh_own_planes()
    assert torch.equal(own.forward_u8(g["ring"].data_ptr(), off), want)
    if g["actor"] is not None:
        pl = QNetInference(g["net"], 128, 0)  # (a handle sized for the online pass running a shorter launch)
        pl.enable_fc1_planes(private_weights=False)
        pl.set_planes_small(True, g["actor"].set_planes_ptr(1))
        assert torch.equal(pl.forward_u8(g["ring"].data_ptr(), off), want)
        pl.set_planes_small(False, None)
        assert torch.equal(pl.forward_u8(g["ring"].data_ptr(), off), want)


def test_training_pass_on_planes_leaves_the_float32_activations(nets):
    """128 rows, sample_stride = 4: the backward pass behind a planes forward reads the float32 act3 / hidden layer that forward also wrote -- gradients bit-equal."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    g = nets["workload"]
    B = 32
    gen = torch.Generator(device="cuda").manual_seed(4)
    gq = torch.randn((B, 6), device="cuda", generator=gen)
    grads, qs = [], []
    for use_planes in (False, True):
        h = QNetInference(g["net"], 128, 0)
        h.enable_training(B)
        if use_planes:
            h.enable_fc1_planes(private_weights=False)
            h.set_planes_small(True, g["actor"].set_planes_ptr(1))
        qs.append(h.forward_u8(g["ring"].data_ptr(), g["off"]).clone())
        h.backward_u8(g["ring"].data_ptr(), g["off"], gq, sample_stride=4)
        torch.cuda.synchronize()
        grads.append([p.grad.clone() for p in g["net"].kernel_parameters()])
    assert torch.equal(qs[0], qs[1])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert any(float(a.abs().max()) > 0 for a in grads[0])


def _engine_pair():
    from simple_distributed_rl_amd.device.rainbow import EngineSchedule, RainbowDeviceConfig, RainbowEngine

    # 512 environments: the fewest the fast lock-step -- the only engine that owns published planes -- takes
    cfg = RainbowDeviceConfig(n_envs=512, batch_size=32, memory_capacity=512 * 10, memory_warmup_size=512 * 3, target_model_update_interval=3, lr=1e-4, seed=5)
    engs = [RainbowEngine(dataclasses.replace(cfg, schedule=EngineSchedule(learner_planes=on)), 0, episode_len=7, overlap=True, fast=True) for on in (True, False)]
    assert engs[0].fast and engs[0]._learner_planes and not engs[1]._learner_planes
    return engs


def _same_update(a, b, tag):
    torch.cuda.synchronize()
    assert a.train_count == b.train_count and a.sync_count == b.sync_count, tag
    for name in ("loss", "priorities", "target", "actions"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)
    for (name, p), q in zip(a.q_online.named_parameters(), b.q_online.parameters()):
        assert torch.equal(p, q), (tag, name)
    for p, q in zip(a.q_target.parameters(), b.q_target.parameters()):
        assert torch.equal(p, q), (tag, "target")


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_with_learner_planes_equals_the_engine_without(graphs):
    """Two fast lock-step engines on one seed, EngineSchedule(learner_planes=True / False): loss, priorities, TD targets, actions and every parameter bit-equal after
    every update -- across target syncs (the target handle's planes are re-split), and across a lock-step of two updates, whose first does not publish: the second
    finds no set holding the current weight and takes the staging-split GEMM, the next lock-step's is back on planes."""
    on, off = _engine_pair()
    try:
        for eng in (on, off):
            for _ in range(5):
                eng._random_rest()
        for eng in (on, off):
            eng.step(learner_updates=1)
        _same_update(on, off, "first")
        if graphs:
            for eng in (on, off):
                eng.enable_lazy_capture()
        seen = set()
        for k, u in enumerate((1, 1, 1, 2, 1, 1, 2, 1)):
            for eng in (on, off):
                eng.step(learner_updates=u)
            _same_update(on, off, (k, u))
            seen.add(on._fresh_set)
        assert on.train_count >= 10 and on.sync_count >= 3 and seen == {0, 1}
        # the variants that ran: the online pass on either set's planes and on none
        if graphs:
            assert {key[-1] for key in on._learner_graphs} == {None, 0, 1} and {key[-1] for key in off._learner_graphs} == {None}
        assert float(on.loss.item()) == float(on.loss.item()) and float(on.priorities.abs().max()) > 0
    finally:
        for eng in (on, off):
            eng.close()
