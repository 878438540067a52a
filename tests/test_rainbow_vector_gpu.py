"""Rainbow on flat observations on the device (libsrlx srlx_mlpq_create_dueling / srlx_mlpq_train_nstep, csrc/srlx_mlpq.hip; device/mlpq.py:VectorQEngine
with `dueling_units` / `multisteps`) over the envelope the create call admits, against the float64 yardstick of tests/rainbow_vec_reference.py (pinned on the
reference's recorded Trainer.train() by tests/test_rainbow_vector_cpu.py): the dueling forward pass with the fused policy selection, the whole n-step learner
step, Adam over several steps, the recorded reference itself, the plain-handle n = 1 bit-equality with srlx_mlpq_train_step, the parameter copy, the n-step
float32 ring against the oracle's store model, and the engine end to end.  Every test prints the error it measured ("RAINBOW-VEC-ERR ...", shown with -s)
before it asserts."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rainbow_vec_recipe as RC  # noqa: E402
import rainbow_vec_reference as R  # noqa: E402

ENVELOPE, golden_inputs = R.ENVELOPE, R.golden_inputs

pytestmark = pytest.mark.gpu

DISCOUNT = 0.99
# ENVELOPE rows (D, trunk, H, A, dueling_type, n):
#   0 every lower bound, the head on the raw observation      1 rainbow.Config() on CartPole      2 every upper bound, largest LDS, 12 tensors
#   3 1/A not a power of two, n + 1 does not divide 16         4 head wider than the trunk          5 two items per workgroup with spare rows


def _sid(i):
    D, trunk, H, A, dtype, n = ENVELOPE[i]
    return f"{D}-{'x'.join(str(w) for w in trunk) or 'none'}-{H}-{A}-{dtype or 'naive'}-n{n}"


def _per_group(n):
    return 16 // (n + 1)  # items one workgroup of the learner kernel takes


@functools.lru_cache(maxsize=None)
def _params(i):
    D, trunk, H, A, _, _ = ENVELOPE[i]
    return R.init_params(D, trunk, H, A, 3000 + i), R.init_params(D, trunk, H, A, 4000 + i)


@functools.lru_cache(maxsize=None)
def _items(i, double_dqn, retrace_h, rescale):
    D, _, _, A, dtype, n = ENVELOPE[i]
    on, tg = _params(i)
    return R.pick_items(on, tg, D, A, n, dtype, DISCOUNT, retrace_h, double_dqn, rescale, 100 * i + 4 * int(double_dqn) + 2 * int(retrace_h == 1.0) + int(rescale))


def _net(i, params):
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet

    D, trunk, H, A, dtype, _ = ENVELOPE[i]
    net = EngineMLPQNet(D, (), trunk, A, H, dtype).cuda()
    with torch.no_grad():
        for p, v in zip(net.kernel_parameters(), params):
            p.copy_(v.float())
    return net


def _batch(it, D, B):
    """The first B items on the device.  Only the rows these items use are placed, on the even row slots of a NaN-filled buffer in a shuffled order: consecutive
    states of an item are never neighbours, items share rows where pick_items chained them, and a read of any other row poisons the result."""
    P = it.rows.shape[0]
    slot = torch.randperm(P, generator=torch.Generator().manual_seed(B)) * 2
    buf = torch.full((2 * P, D), float("nan"))
    used = it.idx[:B].reshape(-1).unique()
    buf[slot[used]] = it.rows[used].float()
    off = (slot[it.idx[:B]] * D).to(torch.int64).contiguous()
    return types.SimpleNamespace(obs=buf.cuda(), off=off.cuda(), act=it.act[:B].int().contiguous().cuda(), rew=it.rew[:B].float().contiguous().cuda(),
                                 term=it.term[:B].float().contiguous().cuda(), w=it.w[:B].float().cuda())


def _outputs(B, A):
    """q0, target, loss, priorities with one guard row past the batch."""
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    return f(B + 1, A), f(B + 1), f(1), f(B + 1)


def _step(h, ht, B, n, b, retrace_h, double_dqn, rescale, steps, out):
    h.train_nstep(ht, B, n, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, retrace_h, double_dqn, rescale, steps, *out)
    torch.cuda.synchronize()


def _grads(net):
    return [p.grad.detach().clone() for p in net.kernel_parameters()]


@pytest.mark.parametrize("i", range(len(ENVELOPE)), ids=_sid)
def test_forward_and_fused_policy(i):
    """Q rows within 1e-5 * max |Q| of float64 at 1, 15, 16, 17 (a workgroup's 16 rows and its neighbours) and 250 rows; the same rows through a shuffled offset
    table are bit-equal; the epsilon-greedy actions of the same launch equal srlx_policy_epsilon_greedy on the launch's own Q rows, bit for bit."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A, dtype, _ = ENVELOPE[i]
    on, _ = _params(i)
    h = MLPQHandle(_net(i, on), 256)
    g = torch.Generator().manual_seed(i)
    lib = N.lib()
    worst = 0.0
    for rows in (1, 15, 16, 17, 250):
        x = torch.randn(rows, D, generator=g)
        xd = x.cuda()
        q = torch.zeros(rows, A, device="cuda")
        acts = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        eps = torch.full((rows,), 0.3, device="cuda")
        counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        h.forward(rows, xd, q=q, eps=eps, seed=11, counter=counter, actions=acts)
        perm = torch.randperm(rows, generator=g).cuda()
        q2 = torch.zeros(rows, A, device="cuda")
        h.forward(rows, xd.data_ptr(), offsets=(perm * D).to(torch.int64), q=q2)
        u = torch.zeros(2 * rows, dtype=torch.float64, device="cuda")
        N.check(lib.srlx_rng_uniform(11, N.tptr(counter), 2 * rows, N.tptr(u), N.torch_stream_ptr()))
        want_a = torch.zeros(rows, dtype=torch.int32, device="cuda")
        N.check(lib.srlx_policy_epsilon_greedy(rows, A, N.tptr(q), N.tptr(eps), N.tptr(u), None, N.tptr(want_a), N.torch_stream_ptr()))
        torch.cuda.synchronize()
        want = R.forward(on, x.double(), dtype)
        err = float((q.double().cpu() - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (rows, err)
        assert torch.equal(q2, q[perm]), rows
        assert torch.equal(acts, want_a), rows
    print(f"RAINBOW-VEC-ERR forward {_sid(i)} worst_rel={worst:.3e}")


def _batch_sizes(n):
    P = _per_group(n)
    return sorted({1, max(P - 1, 1), P, P + 1, 256})


LEARN_CASES = [(i, dd, h, rs) for i in range(len(ENVELOPE)) for dd in (True, False) for h in (1.0, 0.5) for rs in (False, True)]


@pytest.mark.parametrize("i, double_dqn, retrace_h, rescale", LEARN_CASES,
                         ids=[f"{_sid(i)}-{'double' if dd else 'single'}-h{h}-{'rescale' if rs else 'plain'}" for i, dd, h, rs in LEARN_CASES])
def test_learner_step_matches_float64_reference(i, double_dqn, retrace_h, rescale):
    """One srlx_mlpq_train_nstep (gradients only) on the first B items of pick_items, B = 1, P - 1, P, P + 1 (P = the items of one workgroup at this n) and
    256, against rainbow_vec_reference.learner_step: Q of s_0, target and priorities at rtol 1e-5 / atol 1e-6, the loss at rel 1e-5, every gradient at rtol
    1e-5 with an absolute slack of 1e-5 * max |g| of the tensor.  Nothing is written past row B of the outputs.  At B = P + 1 a second run gives the same bits."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A, dtype, n = ENVELOPE[i]
    on, tg = _params(i)
    it = _items(i, double_dqn, retrace_h, rescale)
    ht = MLPQHandle(_net(i, tg), 16)
    for B in _batch_sizes(n):
        net = _net(i, on)
        h = MLPQHandle(net, 16, max_batch=B, max_nstep=n)
        b = _batch(it, D, B)
        q0, target, loss, pri = out = _outputs(B, A)
        _step(h, ht, B, n, b, retrace_h, double_dqn, rescale, None, out)
        ref = R.learner_step(on, tg, it.rows[it.idx[:B]], it.act[:B], it.rew[:B], it.term[:B], it.w[:B], DISCOUNT, retrace_h, double_dqn, rescale, dtype)
        grads = _grads(net)
        gerr = max(float((gk.double().cpu() - gr).abs().max()) / float(gr.abs().max()) for gk, gr in zip(grads, ref.grads))
        print(f"RAINBOW-VEC-ERR learner {_sid(i)} B={B} dd={int(double_dqn)} h={retrace_h} rs={int(rescale)} "
              f"q0={float((q0[:B].double().cpu() - ref.q0).abs().max()):.3e} target={float((target[:B].double().cpu() - ref.target).abs().max()):.3e} "
              f"loss_rel={abs(float(loss) - ref.loss) / ref.loss:.3e} grad_rel={gerr:.3e}")
        assert float(q0[B].min()) == 7.0 and float(q0[B].max()) == 7.0 and float(target[B]) == 7.0 and float(pri[B]) == 7.0
        np.testing.assert_allclose(q0[:B].double().cpu(), ref.q0, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(target[:B].double().cpu(), ref.target, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(pri[:B].double().cpu(), ref.priorities, rtol=1e-5, atol=1e-6)
        assert float(loss) == pytest.approx(ref.loss, rel=1e-5)
        for k, (gk, gr) in enumerate(zip(grads, ref.grads)):
            np.testing.assert_allclose(gk.double().cpu(), gr, rtol=1e-5, atol=1e-5 * float(gr.abs().max()) + 1e-12, err_msg=f"B={B} parameter {k}")
        if B == _per_group(n) + 1:
            net2 = _net(i, on)
            out2 = _outputs(B, A)
            _step(MLPQHandle(net2, 16, max_batch=256, max_nstep=7), ht, B, n, b, retrace_h, double_dqn, rescale, None, out2)
            assert all(torch.equal(a, c) for a, c in zip(list(out) + grads, list(out2) + _grads(net2)))


@pytest.mark.parametrize("i", [3, 4], ids=_sid)
def test_adam_over_six_steps(i):
    """Six consecutive updates (B = 100, steps_taken 0..5 in a device tensor) on fresh pick_items batches.  After every step the parameters equal
    torch.optim.Adam (float32) stepping on the kernel's own gradients (rtol 1e-6, atol 1e-7) and the float64 Adam (rtol 1e-5, atol 1e-7).  The same inputs with
    write_grads=False (Adam only): parameters, exp_avg and exp_avg_sq bit-identical."""
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    D, _, _, A, dtype, n = ENVELOPE[i]
    B, lr, n_steps = 100, 1e-3, 6
    on, tg = _params(i)
    ht = MLPQHandle(_net(i, tg), 16)
    net = _net(i, on)
    h = MLPQHandle(net, 16, max_batch=B, lr=lr, max_nstep=n)
    shadow = [v.float().cuda().requires_grad_(True) for v in on]
    opt = torch.optim.Adam(shadow, lr=lr)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    batches, grads_per_step = [], []
    worst32 = worst64 = 0.0
    for k in range(n_steps):
        cur = [p.detach().double().cpu() for p in net.kernel_parameters()]
        batches.append(_batch(R.pick_items(cur, tg, D, A, n, dtype, DISCOUNT, 1.0, True, False, 500 + 10 * i + k), D, B))
        assert int(steps) == k
        _step(h, ht, B, n, batches[k], 1.0, True, False, steps, _outputs(B, A))
        steps += 1
        grads_per_step.append(_grads(net))
        for s, gk in zip(shadow, grads_per_step[k]):
            s.grad = gk.clone()
        opt.step()
        want64 = R.adam_steps(on, [[g.cpu() for g in gs] for gs in grads_per_step], lr)[0][k]
        for p, s, w64 in zip(net.kernel_parameters(), shadow, want64):
            worst32 = max(worst32, float((p.detach() - s.detach()).abs().max()))
            worst64 = max(worst64, float((p.detach().double().cpu() - w64).abs().max()))
            np.testing.assert_allclose(p.detach().cpu(), s.detach().cpu(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
            np.testing.assert_allclose(p.detach().double().cpu(), w64, rtol=1e-5, atol=1e-7, err_msg=f"step {k}")
    print(f"RAINBOW-VEC-ERR adam {_sid(i)} steps={n_steps} max_abs_vs_torch_f32={worst32:.3e} max_abs_vs_f64={worst64:.3e}")
    net2 = _net(i, on)
    h2 = MLPQHandle(net2, 16, max_batch=B, lr=lr, write_grads=False, max_nstep=n)
    steps.zero_()
    for k in range(n_steps):
        _step(h2, ht, B, n, batches[k], 1.0, True, False, steps, _outputs(B, A))
        steps += 1
    assert all(torch.equal(a, c) for a, c in zip(net.kernel_parameters(), net2.kernel_parameters()))
    assert all(torch.equal(a, c) for a, c in zip(h.exp_avg, h2.exp_avg)) and all(torch.equal(a, c) for a, c in zip(h.exp_avg_sq, h2.exp_avg_sq))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_learner_step_against_the_reference_trainer(name):
    """One srlx_mlpq_train_nstep with Adam on the recipe's weights and items against the reference's recorded Trainer.train(): target, online Q of s_0, loss and
    priorities within rel 1e-5; every p.grad within rel 1e-5 with an absolute slack of 1e-5 * max |g|; every parameter after Adam within rel 1e-5 (+ 1e-7),
    except entries whose reference gradient is below 1e-4 * max |g| (the first Adam step is about lr * g / |g|: only the bound 2 lr holds there)."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    z = np.load(os.path.join(HERE, "golden", "train_step_rainbow_vec.npz"))
    g = lambda k: z[f"{name}.{k}"]  # noqa: E731
    case, keys, _, _, it = golden_inputs(name)
    ins, hid, H = RC.trunk_of(case)
    n, B, lr = case["n"], RC.B, float(g("lr"))
    nets = []
    for seed in (RC.SEED_ONLINE, RC.SEED_TARGET):
        sd = {k: torch.tensor(v) for k, v in RC.recipe_state_dict(case, seed).items()}
        nets.append(EngineMLPQNet(RC.D, ins, hid, RC.A, H, case["dueling_type"]).load_reference_state_dict(sd).cuda())
    assert list(nets[0].reference_state_dict()) == keys
    h, ht = MLPQHandle(nets[0], 16, max_batch=B, lr=lr, max_nstep=n), MLPQHandle(nets[1], 16)
    obs = it.states.reshape(-1, RC.D).contiguous().cuda()
    off = (torch.arange(B * (n + 1), dtype=torch.int64) * RC.D).view(B, n + 1).cuda()
    q0, target, loss, pri = out = _outputs(B, RC.A)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    h.train_nstep(ht, B, n, obs.data_ptr(), off, it.act.int().cuda(), it.rew.cuda(), it.term.cuda(), it.w.cuda(), float(g("discount")), case["retrace_h"],
                  case["double_dqn"], False, steps, *out)
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu().numpy() for k, p in zip(keys, nets[0].kernel_parameters())}
    after = {k: v.cpu().numpy() for k, v in nets[0].reference_state_dict().items()}
    gerr = max(float(np.abs(grads[k] - g("grad." + k)).max()) / float(np.abs(g("grad." + k)).max()) for k in keys)
    print(f"RAINBOW-VEC-ERR golden {name} target={float(np.abs(target[:B].cpu().numpy() - g('target_q')).max()):.3e} "
          f"loss_rel={abs(float(loss) - float(g('loss'))) / float(g('loss')):.3e} grad_rel={gerr:.3e}")
    np.testing.assert_allclose(q0[:B].cpu().numpy(), g("q0"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(target[:B].cpu().numpy(), g("target_q"), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss), float(g("loss")), rtol=1e-5)
    np.testing.assert_allclose(pri[:B].cpu().numpy(), g("priorities"), rtol=1e-5, atol=1e-5 * float(np.abs(g("target_q")).max()))
    for k in keys:
        gr, gmax = g("grad." + k), float(np.abs(g("grad." + k)).max())
        np.testing.assert_allclose(grads[k], gr, rtol=1e-5, atol=1e-5 * gmax, err_msg=k)
        want = g("after." + k)
        firm = np.abs(gr) >= 1e-4 * gmax
        np.testing.assert_allclose(after[k][firm], want[firm], rtol=1e-5, atol=1e-7, err_msg=k)
        assert np.abs(after[k][~firm] - want[~firm]).max(initial=0.0) <= 2 * lr * (1 + 1e-3), k


@pytest.mark.parametrize("rescale", [False, True], ids=["plain", "rescale"])
@pytest.mark.parametrize("B", [9, 256])
def test_plain_handle_at_one_step_is_bit_equal_to_train_step(B, rescale):
    """srlx_mlpq_train_nstep at n = 1, retrace_h = 1 on a plain (out_layer) handle against srlx_mlpq_train_step on the same inputs, over two consecutive Adam
    steps: Q of s_0, target, loss, priorities, every gradient, every parameter and both Adam moments are the same bits."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    D, A, widths = 17, 5, (96, 64)
    g = torch.Generator().manual_seed(B)
    rows = torch.randn(2 * B, D, generator=g).cuda()
    off = (torch.randperm(2 * B, generator=g) * D).view(B, 2).to(torch.int64).cuda()
    act = torch.randint(0, A, (B, 1), generator=g).int().cuda()
    rew = (torch.rand(B, 1, generator=g) * 4 - 2).cuda()
    term = (torch.rand(B, 1, generator=g) < 0.2).float().cuda()
    w = (torch.rand(B, generator=g) * 2 + 0.5).cuda()
    torch.manual_seed(3)
    base, tgt = EngineMLPQNet(D, (), widths, A).cuda(), EngineMLPQNet(D, (), widths, A).cuda()
    ht = MLPQHandle(tgt, 16)
    got = []
    for nstep in (False, True):
        net = EngineMLPQNet(D, (), widths, A).cuda()
        net.load_state_dict(base.state_dict())
        h = MLPQHandle(net, 16, max_batch=B, lr=1e-3)
        steps = torch.zeros(1, dtype=torch.int64, device="cuda")
        kept = []
        for _ in range(2):
            out = _outputs(B, A)
            if nstep:
                h.train_nstep(ht, B, 1, rows.data_ptr(), off, act, rew, term, w, DISCOUNT, 1.0, True, rescale, steps, *out)
            else:
                h.train_step(ht, B, rows.data_ptr(), off, act, rew, term, w, DISCOUNT, True, rescale, steps, *out)
            torch.cuda.synchronize()
            steps += 1
            kept += list(out) + _grads(net)
        got.append(kept + [p.detach().clone() for p in net.kernel_parameters()] + h.exp_avg + h.exp_avg_sq)
    assert not torch.equal(got[0][-1], torch.zeros_like(got[0][-1]))
    assert all(torch.equal(a, c) for a, c in zip(*got))


def test_publish_copies_every_tensor_of_a_dueling_net():
    from simple_distributed_rl_amd.device.mlpq import MLPQHandle

    i = 2
    on, tg = _params(i)
    src, dst = _net(i, on), _net(i, tg)
    hs, hd = MLPQHandle(src, 16), MLPQHandle(dst, 16)
    assert len(dst.kernel_parameters()) == 12 and not any(torch.equal(a, c) for a, c in zip(src.kernel_parameters(), dst.kernel_parameters()))
    hs.publish_to(hd)
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(src.kernel_parameters(), dst.kernel_parameters()))
    assert all(torch.equal(p.detach().cpu(), v.float()) for p, v in zip(src.kernel_parameters(), on))
    with pytest.raises(N.SrlxError, match="shapes differ"):  # another shape
        hs.publish_to(MLPQHandle(_net(1, _params(1)[0]), 16))


def test_train_nstep_rejects_bad_arguments_without_a_launch():
    """More steps than the handle was sized for, a target of the other head kind, a dueling handle handed to srlx_mlpq_train_step: an error, and the outputs and
    gradients keep what they held."""
    from simple_distributed_rl_amd.device.mlpq import EngineMLPQNet, MLPQHandle

    i, B = 3, 4
    D, trunk, H, A, dtype, n = ENVELOPE[i]
    on, tg = _params(i)
    net = _net(i, on)
    h, ht = MLPQHandle(net, 16, max_batch=B, max_nstep=n), MLPQHandle(_net(i, tg), 16)
    plain = MLPQHandle(EngineMLPQNet(D, (), trunk, A).cuda(), 16)
    b = _batch(_items(i, True, 1.0, False), D, B)
    for p in net.kernel_parameters():
        p.grad.fill_(3.0)
    out = _outputs(B, A)
    with pytest.raises(N.SrlxError, match="3 steps"):
        h.train_nstep(ht, B, n + 1, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, 1.0, True, False, None, *out)
    with pytest.raises(N.SrlxError, match="shapes differ"):
        h.train_nstep(plain, B, n, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, 1.0, True, False, None, *out)
    with pytest.raises(N.SrlxError, match="srlx_mlpq_train_nstep"):
        h.train_step(ht, B, b.obs.data_ptr(), b.off, b.act, b.rew, b.term, b.w, DISCOUNT, True, False, None, *out)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out) and all(bool((p.grad == 3.0).all()) for p in net.kernel_parameters())
    _step(h, ht, B, n, b, 1.0, True, False, None, out)
    assert bool(torch.isfinite(out[0][:B]).all()) and not bool((out[0][:B] == 7.0).any())


# ---- the engine -----------------------------------------------------------------------------------------------------------------------------------------------
class _DeviceFloats:
    """Zero-copy float32 view of device memory for torch.as_tensor (the ring lives in libsrlx, not in a torch tensor)."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f4", "data": (ptr, False), "version": 2}


class _ScriptedEnv:
    """E = 4 host-stepped lanes whose episodes last 1, 2, 4 and 7 steps; lanes 0 and 2 end terminated, lanes 1 and 3 truncated.  Every observation encodes
    (lane, episode, step), every reward the step.  A lane that ended delivers its next episode's first observation on the next step (the store's protocol)."""

    capturable = False
    LENS = (1, 2, 4, 7)

    def __init__(self, replay):
        self.E, self.dev = replay.E, replay.dev
        assert self.E == len(self.LENS) and replay.F == 4
        self.episode, self.t, self.pending = [0] * self.E, [0] * self.E, [False] * self.E
        self.next_obs = torch.zeros((self.E, 4), dtype=torch.float32, device=self.dev)
        self.rewards = torch.zeros(self.E, dtype=torch.float32, device=self.dev)
        self.terminated = torch.zeros(self.E, dtype=torch.uint8, device=self.dev)
        self.done = torch.zeros(self.E, dtype=torch.uint8, device=self.dev)
        self.log = []

    def _obs(self, e):
        return [float(e + 1), float(self.episode[e]), float(self.t[e]), 0.5 * self.t[e] - 0.25 * e]

    def reset(self):
        return torch.tensor([self._obs(e) for e in range(self.E)], dtype=torch.float32, device=self.dev)

    def step(self, actions):
        acts = actions.cpu().tolist()
        obs, rew, term, done = [], [], [], []
        for e in range(self.E):
            if self.pending[e]:
                self.pending[e] = False
                self.episode[e] += 1
                self.t[e] = 0
                obs.append(self._obs(e)), rew.append(0.0), term.append(0), done.append(0)
                continue
            self.t[e] += 1
            end = self.t[e] >= self.LENS[e]
            obs.append(self._obs(e)), rew.append(1.0 + 0.125 * self.t[e]), term.append(int(end and e % 2 == 0)), done.append(int(end))
            self.pending[e] = end
        self.log.append((acts, rew, term, done, obs))
        self.next_obs.copy_(torch.tensor(obs, dtype=torch.float32))
        self.rewards.copy_(torch.tensor(rew, dtype=torch.float32))
        self.terminated.copy_(torch.tensor(term, dtype=torch.uint8))
        self.done.copy_(torch.tensor(done, dtype=torch.uint8))
        return self.next_obs, self.rewards, self.terminated, self.done


def _rainbow_cfg(**kw):
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    base = dict(batch_size=32, lr=1e-3, target_model_update_interval=10, memory_capacity=64 * 20, memory_warmup_size=256, hidden_sizes=(), dueling_units=64,
                multisteps=3, n_envs=64, seed=4, epsilon=0.1, memory_alpha=0.6)
    base.update(kw)
    return VectorQConfig(**base)


def test_nstep_float_ring_matches_the_oracle_store():
    """E = 4 scripted lanes (episodes of 1, 2, 4 and 7 steps) at n = 3 on a ring of 9 item slots, 31 lock-steps (the ring wraps three times): for every live
    item the s_0..s_n rows the learner's offset table points at, and the gathered actions, rewards and terminated flags, equal hot_path_oracle's lock-step store
    model bit for bit -- the padding behind an episode's end included."""
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
    import hot_path_oracle as H
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    E, n, B = 4, 3, 4
    cfg = _rainbow_cfg(batch_size=B, n_envs=E, memory_capacity=E * 9, memory_warmup_size=10_000, dueling_units=32, epsilon=1.0, seed=9)
    eng = VectorQEngine(cfg, 0, env=_ScriptedEnv)
    r = eng.replay
    assert (r.n, r.W, r.item_len, r.capacity) == (n, 1, 9, E * 9) and not r.obs_uint8
    ora = H.StoreOracle(E, r.L, 4, 1, n, 2, False, cfg.seed, u8=False)
    ora.reset_all(eng.first_obs.cpu().numpy())
    live = {}
    checked = padded = 0
    for step in range(31):
        eng.actor_step()
        torch.cuda.synchronize()
        acts, rew, term, done, obs = eng.env.log[-1]
        mask = ora.commit_step(acts, rew, term, done, np.asarray(obs, np.float32))
        assert mask.tolist() == r.item_mask.cpu().tolist(), step
        for e in range(E):
            live[(step % r.item_len) * E + e] = bool(mask[e])
        if step < n + 1 or step % 5:
            continue
        ring = torch.as_tensor(_DeviceFloats(r.obs_base, E * r.L * 4), device="cuda").clone().cpu()
        leaves = [j for j, ok in sorted(live.items()) if ok]
        for k in range(0, len(leaves), B):
            chunk = (leaves[k:k + B] * B)[:B]
            r.batch.indices.copy_(torch.tensor(chunk, dtype=torch.int64) + (r.capacity - 1))
            b = r.gather_drawn(all_states=True)
            torch.cuda.synchronize()
            off = r.frame_off_all.view(B, n + 1).cpu()
            assert int(off.min()) >= 0 and int(off.max()) + 4 <= ring.numel() and bool((off % 4 == 0).all())
            for x, j in enumerate(chunk):
                want_obs, want_a, want_r, want_t, jd = ora.gather_item(*ora.locate(j + r.capacity - 1))
                got_obs = torch.stack([ring[int(o):int(o) + 4] for o in off[x]]).numpy()
                assert np.array_equal(got_obs, want_obs[:, 0]), (step, j)
                assert np.array_equal(b.actions[x].cpu().numpy(), want_a) and np.array_equal(b.rewards[x].cpu().numpy(), want_r), (step, j)
                assert np.array_equal(b.terminated[x].cpu().numpy(), want_t), (step, j)
                checked += 1
                padded += int(jd < n - 1)
    assert checked > 60 and padded > 10, (checked, padded)


def test_two_engines_with_one_seed_are_bit_identical():
    """20 lock-steps of a dueling n = 3 engine on the device CartPole (updates from the fifth lock-step on, the last five through the captured graph)."""
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    out = []
    for _ in range(2):
        eng = VectorQEngine(_rainbow_cfg(), 0)
        for _ in range(15):
            eng.step(learner_updates=1)
        eng.capture_graphs(warm_actor=False)
        for _ in range(5):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        assert eng.train_count >= 15 and eng.nstep
        out.append(([p.detach().clone() for p in eng.q_online.kernel_parameters()], eng.priorities.clone(), eng.loss.clone(), eng.info()["loss"]))
    assert all(torch.equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2]) and np.isfinite(out[0][3])


def test_default_config_issues_the_one_step_launches():
    """VectorQConfig's defaults are the DQN engine: a plain head, 1-step items, srlx_mlpq_train_step."""
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig, VectorQEngine

    eng = VectorQEngine(VectorQConfig(n_envs=16, memory_capacity=16 * 8, memory_warmup_size=32, hidden_sizes=(32,)), 0)
    assert not eng.nstep and eng.replay.n == 1 and eng.replay.L == 8 + 2 and len(eng.q_online.kernel_parameters()) == 4


def test_trained_engine_hands_its_networks_to_the_rainbow_plugin():
    """A rainbow.Config() engine (dueling (512,), n = 3) trains on the device CartPole for a few dozen updates; `store_q_weights` puts its networks into the
    Rainbow plugin's Parameter, whose `pred_q` on 64 observations equals the engine's forward pass within 1e-5, and `Runner.evaluate()` plays with it; the
    Parameter's weights go back into a fresh engine unchanged."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import rainbow
    from simple_distributed_rl_amd.device import vector_runner as vr
    from simple_distributed_rl_amd.device.mlpq import VectorQEngine

    rl = rainbow.Config()
    rl.memory.capacity, rl.memory.warmup_size = 64 * 30, 256
    runner = srl.Runner("CartPole-v1", rl)
    runner.set_device("cuda:0")
    runner.setup_rl_config()
    assert vr.why_not_flat_rainbow(runner.env, runner.rl_config) == ""
    cfg = vr.mlp_config_from(runner.rl_config, runner.env, 64, 1)
    assert (cfg.dueling_units, cfg.multisteps, cfg.hidden_sizes) == (512, 3, ())
    eng = VectorQEngine(cfg, 0)
    before = [p.detach().clone() for p in eng.q_online.kernel_parameters()]
    for _ in range(40):
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    assert eng.train_count >= 30 and np.isfinite(eng.info()["loss"])
    assert not any(torch.equal(a, p) for a, p in zip(before, eng.q_online.kernel_parameters()))
    vr.store_q_weights(eng, runner.parameter)
    x = torch.randn(64, 4, generator=torch.Generator().manual_seed(2))
    q = torch.zeros(64, 2, device="cuda")
    eng.inf_online.forward(64, x.cuda(), q=q)
    torch.cuda.synchronize()
    want = runner.parameter.pred_q(x.numpy())
    err = float(np.abs(q.cpu().numpy() - want).max()) / float(np.abs(want).max())
    print(f"RAINBOW-VEC-ERR plugin pred_q rel={err:.3e}")
    assert err <= 1e-5
    rewards = runner.evaluate(max_episodes=3, enable_progress=False)
    assert len(rewards) == 3 and np.all(np.isfinite(rewards)) and min(rewards) >= 1
    fresh = VectorQEngine(cfg, 0)
    vr.load_q_weights(fresh, runner.parameter)
    assert all(torch.equal(a, c) for a, c in zip(fresh.q_online.kernel_parameters(), eng.q_online.kernel_parameters()))
    assert all(torch.equal(a, c) for a, c in zip(fresh.q_target.kernel_parameters(), eng.q_target.kernel_parameters()))
