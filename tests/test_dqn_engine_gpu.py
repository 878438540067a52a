"""GPU tests: DQN on the device engine -- the plain Q head of libsrlx (dueling_type 3: q = W2 relu(h) + b2 over all units of the first dense layer,
srl/algorithms/dqn/model_torch.py:17-29) through every layer: forward on both first-dense-layer paths, the fused policy, one learner step against the reference's
Trainer.train() (tests/golden/train_step_dqn84.npz, oracle/gen_golden_dqn84.py), the fused TD / Adam paths, srl.Runner(...).train() and reproducibility."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

import dqn84_recipe as R  # noqa: E402


def _plain_net(A, seed=11, width=512):
    from simple_distributed_rl_amd.device.qnet import EngineQNet

    torch.manual_seed(seed)
    return EngineQNet(A, (84, 84), 4, width // 2, 32, "plain").cuda()


def _ring(B, seed=3):
    F = 84 * 84
    g = torch.Generator(device="cuda").manual_seed(seed)
    ring = torch.randint(0, 256, (600 * F,), dtype=torch.uint8, device="cuda", generator=g)
    idx = torch.randint(0, 600, (B, 4), device="cuda", generator=g)
    return ring, idx * F, idx.cpu()


@pytest.mark.parametrize("A", [6, 18])
@pytest.mark.parametrize("B, planes", [(1, False), (32, False), (1024, False), (1024, True)])
def test_plain_head_forward_against_float64(A, B, planes):
    """The device forward on uint8 frames (split-K first dense layer, or operand planes for a chip-filling launch) against the reference-layout module in float64.
    Bar (tests/test_qnet_pinned.py): at most twice the error of the module's own float32 evaluation + one ulp of max |Q|."""
    from simple_distributed_rl_amd.device.qnet import QNetInference

    net = _plain_net(A)
    qn = QNetInference(net, B)
    if planes:
        qn.enable_fc1_planes(private_weights=True)
    ring, off, idx = _ring(B)
    q = qn.forward_u8(ring.data_ptr(), off).double().cpu()
    ref = net.reference_module()
    ref.load_state_dict({k: v.cpu() for k, v in net.reference_state_dict().items()})
    x = ring.view(600, 84, 84).cpu()[idx].float() / 255.0
    with torch.no_grad():
        q32 = ref(x, channels_first=True).double()
        q64 = copy.deepcopy(ref).double()(x.double(), channels_first=True)
    scale = float(q64.abs().max())
    err, err_ref = float((q - q64).abs().max()), float((q32 - q64).abs().max())
    assert err <= 2 * err_ref + float(np.spacing(np.float32(scale))), (err, err_ref, scale)


def test_plain_head_policy_equals_rng_plus_epsilon_greedy():
    """srlx_qnet_forward_u8_policy on a plain-head handle: the Q rows of forward_u8 and the actions srlx_rng_uniform + srlx_policy_epsilon_greedy pick on them."""
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.qnet import QNetInference

    E, A = 512, 6
    net = _plain_net(A)
    with torch.no_grad():  # rows with tied maxima
        net.out_layer.bias.add_(torch.tensor([0.0, 0.3, 0.0, 0.3, -0.1, 0.2], device="cuda"))
    inf = QNetInference(net, E)
    ring, off, _ = _ring(E)
    lib = N.lib()
    eps = torch.full((E,), 0.1, device="cuda")
    eps[::3] = 1.0
    eps[1::7] = 0.0
    g = torch.Generator(device="cuda").manual_seed(1)
    invalid = (torch.rand((E, A), device="cuda", generator=g) < 0.3).to(torch.uint8)
    invalid[:, 2] = 0
    seed = 0xD01 ^ 5
    for inv in (None, invalid):
        for c0 in (0, 1, 12345):
            counter = torch.tensor([c0], dtype=torch.int64, device="cuda")
            act_f = torch.full((E,), -1, dtype=torch.int32, device="cuda")
            qc = torch.zeros((E, A), device="cuda")
            q_f = inf.forward_u8_policy(ring.data_ptr(), off, eps, seed, counter, act_f, invalid=inv, q_copy=qc).clone()
            q = inf.forward_u8(ring.data_ptr(), off).clone()
            u = torch.zeros(2 * E, dtype=torch.float64, device="cuda")
            N.check(lib.srlx_rng_uniform(seed, N.tptr(counter), 2 * E, N.tptr(u), N.torch_stream_ptr()))
            act = torch.full((E,), -1, dtype=torch.int32, device="cuda")
            N.check(lib.srlx_policy_epsilon_greedy(E, A, N.tptr(q), N.tptr(eps), N.tptr(u), N.tptr(inv), N.tptr(act), N.torch_stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(q_f, q) and torch.equal(qc, q)
            assert torch.equal(act_f, act), (inv is not None, c0)
            assert 0 < int((act != q.argmax(1).to(torch.int32)).sum())


def _golden_engine(schedule=None, fast=False):
    """A plain-head RainbowEngine (DQN's configuration: multisteps 1, double DQN) carrying the golden's recipe weights whose next `_learner_body` trains on the
    golden's 16 items (5 frames each, written into the ring by ordinary commits) with the golden's importance weights."""
    from simple_distributed_rl_amd.device.rainbow import RainbowDeviceConfig, RainbowEngine

    z = np.load(os.path.join(GOLDEN, "train_step_dqn84.npz"))
    frames, actions, reward, undone = z["frames"], z["actions"], z["reward"], z["undone"]
    B, n, E = R.B, 1, 512
    cfg = RainbowDeviceConfig(n_envs=E, batch_size=B, memory_capacity=E * 8, memory_warmup_size=E, lr=float(z["lr"]), discount=float(z["discount"]),
                              target_model_update_interval=1000, enable_reward_clip=False, enable_double_dqn=True, multisteps=1, hidden_units=R.W, plain_head=True,
                              n_actions=R.A)
    if schedule is not None:
        cfg.schedule = schedule
    eng = RainbowEngine(cfg, 0, episode_len=1000, overlap=fast, fast=fast)
    eng.q_online.load_reference_state_dict({k: torch.tensor(v) for k, v in R.recipe_state_dict(R.SEED_ONLINE).items()})
    eng.q_target.load_reference_state_dict({k: torch.tensor(v) for k, v in R.recipe_state_dict(R.SEED_TARGET).items()})
    rp, dev = eng.replay, eng.dev

    def lanes(x, dtype):
        t = torch.zeros((E,) + tuple(x.shape[1:]), dtype=dtype, device=dev)
        t[:B] = torch.tensor(x).to(dev).to(dtype)
        return t

    zero_i, zero_f = np.zeros(B, np.int32), np.zeros(B, np.float32)
    rp.reset_all(lanes(frames[:, 0].reshape(B, -1), torch.uint8))
    for i in range(1, 5):  # frame i arrives with the transition frame i - 1 -> i; the item's transition is commit number 3 (frames 3 -> 4)
        last = i == 4
        d = lanes(1.0 - undone if last else zero_f, torch.uint8)
        rp.commit(lanes(actions if last else zero_i, torch.int32), lanes(reward if last else zero_f, torch.float32), d, d,
                  lanes(frames[:, i].reshape(B, -1), torch.uint8))
    idx = (3 * E + torch.arange(B, device=dev, dtype=torch.int64)) + rp.capacity - 1
    w = torch.tensor(z["weights"]).to(dev)

    def fixed_batch(*a, **k):
        rp.batch.indices.copy_(idx)
        rp.batch.weights.copy_(w)
        return rp.gather_drawn(all_states=True)

    rp.sample_items = fixed_batch
    if eng.fast:
        eng._check_versions()
    else:
        eng.inf_online.weights_changed()
        eng.inf_target.weights_changed()
    return eng, z


def _check_outputs(eng, z):
    B = R.B
    q0 = eng.inf_online.q[: B * 2].view(B, 2, -1)[:, 0].cpu().numpy()
    np.testing.assert_allclose(q0, z["q0"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(eng.target.cpu().numpy(), z["target_q"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(float(eng.loss.item()), float(z["loss"]), rtol=1e-5)
    np.testing.assert_allclose(eng.priorities.cpu().numpy(), z["priorities"], rtol=1e-5, atol=1e-5 * float(np.abs(z["target_q"]).max()))


def _ref_grads(net):
    C, P, W = net.out_c, net.out_p, 2 * net.hidden
    conv = {"in_block.image_block.image_layers.0": net.conv1, "in_block.image_block.image_layers.2": net.conv2, "in_block.image_block.image_layers.4": net.conv3}
    got = {"hidden_block.hidden_layers.0.weight": net.fc1.weight.grad.reshape(W, P, C).permute(0, 2, 1).reshape(W, C * P),
           "hidden_block.hidden_layers.0.bias": net.fc1.bias.grad, "out_layer.weight": net.out_layer.weight.grad, "out_layer.bias": net.out_layer.bias.grad}
    for ref, c in conv.items():
        got[ref + ".weight"], got[ref + ".bias"] = c.weight.grad.contiguous(), c.bias.grad
    return got


def test_learner_step_against_the_reference_trainer():
    """One update with the optimiser as a launch of its own (fused_adam=False: the gradients are written out) against ONE Trainer.train() of the reference's DQN:
    target, Q, loss and priorities to rel 1e-5; every sampled `p.grad` entry at the bar of test_learner_gradients_against_the_reference_trainer."""
    from simple_distributed_rl_amd.device.rainbow import EngineSchedule

    eng, z = _golden_engine(EngineSchedule(fused_adam=False))
    assert eng.mfma_train and not eng.fast
    eng._learner_body()
    torch.cuda.synchronize()
    _check_outputs(eng, z)
    got = _ref_grads(eng.q_online)
    for k, _ in R.KEYS_SHAPES:
        pos = torch.tensor(z["pos." + k])
        g = got[k].detach().float().cpu().reshape(-1)[pos].numpy()
        np.testing.assert_allclose(g, z["grad." + k], rtol=1e-4, atol=1e-5 * float(z["gmax." + k]), err_msg=k)
        total = float(got[k].double().sum().item())
        assert abs(total - float(z["gsum." + k])) <= 1e-4 * float(np.abs(z["grad." + k]).sum() / len(pos) * got[k].numel()) + 1e-9, k
    assert float(eng.q_online.unused_w.grad.abs().sum()) == 0.0  # (the v2 entries of the handle: never written)


def test_fast_engine_learner_step_against_the_reference_trainer():
    """The shipped learner path (fast lock-step: fused TD head, Adam fused into the launches that finish each gradient, published sets) against the same golden:
    outputs to rel 1e-5, the Adam step's sign on 2048 entries per tensor and its sum (as the Rainbow test of tests/test_qnet_pinned.py)."""
    eng, z = _golden_engine(fast=True)
    assert eng.fast
    before = {k: v.clone() for k, v in eng.q_online.reference_state_dict().items()}
    eng._learner_body(publish=1)
    torch.cuda.synchronize()
    _check_outputs(eng, z)
    after = eng.q_online.reference_state_dict()
    lr = float(z["lr"])
    for k, _ in R.KEYS_SHAPES:
        pos = torch.tensor(z["pos." + k])
        got = (after[k].double().cpu().reshape(-1)[pos] - before[k].double().cpu().reshape(-1)[pos]).numpy()
        want = z["upd." + k].astype(np.float64)
        bad = np.abs(got - want) > 1e-2 * lr
        assert bad.mean() <= 0.02, (k, float(bad.mean()))
        assert np.abs(got - want).max() <= 2.0 * lr * (1 + 1e-3), (k, float(np.abs(got - want).max()))
        total = float((after[k].double() - before[k].double()).sum().item())
        assert abs(total - float(z["sum." + k])) <= 2e-2 * float(z["abs." + k]) + 1e-12, (k, total, float(z["sum." + k]))


def test_fused_td_and_fused_adam_equal_their_own_launches():
    """TD target / Huber / priorities inside the backward's head kernel equal the TD kernel as a launch of its own (bit for bit); Adam fused into the launches that
    finish the gradients equals the optimiser as one launch after them."""
    from simple_distributed_rl_amd.device.rainbow import EngineSchedule

    runs = {}
    for name, sch in (("fused", EngineSchedule()), ("td_apart", EngineSchedule(fused_td=False)), ("adam_apart", EngineSchedule(fused_adam=False))):
        eng, z = _golden_engine(sch)
        eng._learner_body()
        torch.cuda.synchronize()
        runs[name] = (eng.target.clone(), eng.loss.clone(), eng.priorities.clone(), {k: v.clone() for k, v in eng.q_online.reference_state_dict().items()})
        del eng
    f, t = runs["fused"], runs["td_apart"]
    for a, b in zip(f[:3], t[:3]):
        assert torch.equal(a, b)
    lr = float(z["lr"])
    for k, _ in R.KEYS_SHAPES:
        x, y = runs["fused"][3][k].double(), runs["adam_apart"][3][k].double()
        d = (x - y).abs()
        assert float((d > 1e-2 * lr).double().mean()) <= 0.02 and float(d.max()) <= 2.0 * lr, k


def _dqn_atari_like(capacity=20_000, warmup=2_048):
    from simple_distributed_rl_amd.algorithms import dqn

    cfg = dqn.Config()
    cfg.set_atari_config()  # dqn.py:88-101
    cfg.window_length = 4
    cfg.memory.capacity, cfg.memory.warmup_size = capacity, warmup
    cfg.epsilon_scheduler.set_linear(1.0, 0.1, 12)
    cfg.target_model_update_interval = 8
    return cfg


def test_runner_trains_dqn_on_the_engine():
    """srl.Runner("SyntheticAtari-v0", <DQN Atari config, small replay>).train(...): on the engine, epsilon follows epsilon_scheduler at the lock-step counts, every
    runner.parameter tensor (DQN's keys) changes, evaluate() works."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.base.run.callback import RunCallback

    cfg = _dqn_atari_like()
    runner = srl.Runner("SyntheticAtari-v0", cfg)
    runner.set_seed(2)
    runner.set_vector_envs(256)
    before = {k: v.detach().clone() for k, v in runner.parameter.q_online.state_dict().items()}
    assert set(before) == {k for k, _ in R.KEYS_SHAPES}
    seen = []

    class Eps(RunCallback):
        def on_step_end(self, context, state, **kw):
            act = runner._vector_actor
            seen.append((act._iteration - 1, float(act.engine.eps[0].item())))
            return False

    st = runner.train(max_steps=256 * 40, train_interval=64, callbacks=[Eps()])
    assert runner.vector_reason == ""
    assert st.train_count > 0
    sched = cfg.epsilon_scheduler.create(cfg.epsilon)
    for it, e in seen:
        assert e == pytest.approx(sched.update(it).to_float(), rel=1e-6), it
    assert seen[0][1] == pytest.approx(1.0) and seen[-1][1] == pytest.approx(0.1)
    after = runner.parameter.q_online.state_dict()
    changed = [k for k in before if not torch.equal(before[k].cpu(), after[k].cpu())]
    assert len(changed) == len(before), set(before) - set(changed)
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2


def test_two_engines_with_the_same_seed_are_bit_identical():
    """The fast lock-step (graph-replayed) of two plain-head engines with the same seed: identical parameters after N lock-steps."""
    from simple_distributed_rl_amd.device.rainbow import RainbowDeviceConfig, RainbowEngine

    out = []
    for _ in range(2):
        cfg = RainbowDeviceConfig(n_envs=512, batch_size=32, memory_capacity=512 * 16, memory_warmup_size=1024, target_model_update_interval=5, multisteps=1,
                                  enable_double_dqn=False, hidden_units=512, plain_head=True, seed=4, lr=1e-4)
        eng = RainbowEngine(cfg, 0, episode_len=37, overlap=True)
        assert eng.fast
        for _ in range(6):  # past the warm-up gate, eagerly
            eng.step(learner_updates=1)
        eng.capture_graphs()
        for _ in range(12):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        assert eng.train_count >= 12
        out.append({k: v.detach().clone() for k, v in eng.q_online.reference_state_dict().items()})
        eng.close()
        del eng
    assert all(torch.equal(out[0][k], out[1][k]) for k in out[0])
