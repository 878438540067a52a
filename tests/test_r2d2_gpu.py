"""R2D2 on the GPU: libsrlx srlx_r2d2_seq_td (csrc/srlx_r2d2.hip) over its envelope and one whole `Trainer.train()` of algorithms/r2d2.py, both against
the float64 yardstick of tests/r2d2_reference.py (its footing: tests/test_r2d2_cpu.py; parity with the TensorFlow reference is unpinned), then the trainer's
and the runner's plumbing.  Every comparison prints the error it measured ("R2D2-ERR ...", shown with -s) before it asserts.

Measured on an MI355X, as fractions of the bars (rtol 1e-5 / atol 1e-6 on target and td_mean, 1e-5 relative on the loss, rtol 1e-5 + 1e-5 max|g| on grad_q): the
kernel's target <= 0.0056, td_mean <= 0.0054, loss <= 0.0060, grad_q <= 0.0027 over all eight shapes, which is float32's output rounding; one Trainer.train():
loss within 1.0e-7 relative, td_mean within 0.008 of its bar, gradients within 6.8e-7 of max|g| on "srlx" and 1.1e-6 on "torch" (DESIGN.md 7k)."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import r2d2_reference as R  # noqa: E402

import simple_distributed_rl_amd as srl  # noqa: E402
from simple_distributed_rl_amd import _native as N  # noqa: E402
from simple_distributed_rl_amd.algorithms import r2d2  # noqa: E402
from simple_distributed_rl_amd.algorithms._device_ops import TdOps  # noqa: E402

GAP, TRAINER_EPISODES, TRAINER_SEEDS = R.GAP, R.TRAINER_EPISODES, R.TRAINER_SEEDS

pytestmark = pytest.mark.gpu

SMALL = [(1, 1, 2), (3, 2, 3), (7, 5, 4), (32, 5, 2)]  # all eight flag combinations, retrace_h 1.0 and 0.95, with and without masks
LARGE = [(257, 3, 5), (2, 512, 3), (1024, 1, 64), (64, 80, 18)]  # more rows than one launch wave, the longest walk, the widest rows, set_atari_config's shape
DISCOUNT = 0.9


# ---- inputs on a lattice --------------------------------------------------------------------------------------------------------------------------------
def _lattice_q(g, B, S1, A):
    """Distinct multiples of 2^-6 per (row, step): every comparison of two entries comes out the same in float32 and float64."""
    out = np.empty((B, S1, A), np.float32)
    for b in range(B):
        for t in range(S1):
            out[b, t] = g.choice(257, A, replace=False).astype(np.float32) / 64 - 2
    return out


@functools.lru_cache(maxsize=None)
def _inputs(B, S, A, masked):
    g = np.random.default_rng(1000 * B + 10 * S + A + int(masked))
    q, qt = _lattice_q(g, B, S + 1, A), _lattice_q(g, B, S + 1, A)
    actions = g.integers(0, A, (B, S)).astype(np.int32)
    mu = (g.integers(1, 17, (B, S)) / 16).astype(np.float32)
    rewards = (g.integers(-64, 65, (B, S)) / 32).astype(np.float32)
    dones = (g.random((B, S)) < 0.15).astype(np.uint8)
    weights = (g.integers(8, 25, B) / 16).astype(np.float32)
    invalid = None
    if masked:
        invalid = (g.random((B, S + 1, A)) < 0.3).astype(np.uint8)
        invalid[np.arange(B)[:, None], np.arange(S + 1)[None, :], g.integers(0, A, (B, S + 1))] = 0  # at least one valid action everywhere
        for b in range(B):
            for t in range(S):
                if invalid[b, t, actions[b, t]]:  # a taken action was valid when it was taken
                    actions[b, t] = int(np.flatnonzero(invalid[b, t] == 0)[0])
    forced = _force(q, qt, actions, mu, rewards, dones, weights, invalid)
    for a in (q, qt, actions, mu, rewards, dones, weights) + ((invalid,) if masked else ()):
        a.setflags(write=False)
    return q, qt, actions, mu, rewards, dones, invalid, weights, forced


def _force(q, qt, actions, mu, rewards, dones, weights, invalid):
    """The forced rows, in front: row k gets case k as far as B, S and A have room for it.  Returns the names of the cases placed."""
    B, S1, A = q.shape
    S, mid, placed = S1 - 1, (S1 - 1) // 2, []

    def row(name, ok=True):
        b = len(placed)
        if b < B and ok:
            placed.append(name)
            dones[b] = 0
            if invalid is not None:
                invalid[b] = 0
            return b
        return None

    for name, ts in (("done at 0", [0]), ("done in the middle", [mid]), ("done at S-1", [S - 1]), ("done everywhere", list(range(S)))):
        if (b := row(name)) is not None:
            dones[b, ts] = 1
    if (b := row("tie at the taken action", A >= 2)) is not None:  # pi = 1/2
        a, other = int(actions[b, mid]), (int(actions[b, mid]) + 1) % A
        q[b, mid, a] = q[b, mid, other] = 3.0
        mu[b, mid] = 1.0
    if (b := row("tie in the selecting row", A >= 2)) is not None:  # the first index wins, in the online and in the target row alike
        for arr in (q, qt):
            arr[b, mid + 1, 0] = arr[b, mid + 1, A - 1] = 3.0
    if (b := row("unmasked maximum invalid", A >= 2 and invalid is not None)) is not None:
        invalid[b, mid + 1, int(np.argmax(q[b, mid + 1]))] = 1
        invalid[b, mid + 1, int(np.argmax(qt[b, mid + 1]))] = 1
        if invalid[b, mid + 1].all():
            invalid[b, mid + 1, int(np.argmin(q[b, mid + 1]))] = 0
    if (b := row("non-greedy action", A >= 2)) is not None:  # retrace falls to 0 behind it
        actions[b, S - 1] = int(np.argmin(q[b, S - 1]))
    if (b := row("mu 1/16 with pi 1")) is not None:  # the clip
        for t in range(S):
            actions[b, t] = int(np.argmax(q[b, t]))
        mu[b] = 1 / 16
    if (b := row("weighted TD above 1")) is not None:  # the linear Huber branch
        weights[b], rewards[b] = 8.0, 2.0
    if (b := row("weighted TD below 1")) is not None:  # the quadratic branch
        weights[b] = 1 / 64
    return placed


def _launch(ops, inp, h, retrace, dd, rescale):
    q, qt, actions, mu, rewards, dones, invalid, weights, _ = inp
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    out = ops.r2d2_seq_td(dev(q), dev(qt), dev(actions), dev(mu), dev(rewards), dev(dones), dev(invalid), dev(weights), DISCOUNT, h, retrace, dd, rescale)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]  # target, loss, grad_q, td_mean


def _compare(tag, got, want, worst):
    target, loss, grad, td = got
    gmax = float(np.abs(want.grad_q).max())
    errs = dict(target=float(np.max(np.abs(target - want.target) / (1e-6 + 1e-5 * np.abs(want.target)))),
                td_mean=float(np.max(np.abs(td - want.td_mean) / (1e-6 + 1e-5 * np.abs(want.td_mean)))),
                loss=abs(float(loss[0]) - want.loss) / (1e-5 * abs(want.loss)) if want.loss else float(loss[0] != 0),
                grad_q=float(np.max(np.abs(grad - want.grad_q) / (1e-5 * gmax + 1e-5 * np.abs(want.grad_q)))) if gmax else float(np.abs(grad).max() != 0))
    for k, v in errs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 1.0 for v in errs.values()), (tag, errs)  # each figure is the error as a fraction of its bar
    assert not grad[:, -1].any(), tag  # the last step's rows are zero (r2d2.py:149-150)


def _check(shape, combos):
    B, S, A = shape
    ops, worst, cases = TdOps(torch.device("cuda:0")), {}, set()
    for masked, h, (retrace, dd, rescale) in combos:
        inp = _inputs(B, S, A, masked)
        cases.update(inp[8])
        q, qt, actions, mu, rewards, dones, invalid, weights, _ = inp
        want = R.seq_td(q.astype(np.float64), qt.astype(np.float64), R.items_from_arrays(actions, mu, rewards, dones, invalid), weights.astype(np.float64),
                        DISCOUNT, h, retrace, dd, rescale)
        got = _launch(ops, inp, h, retrace, dd, rescale)
        _compare((shape, masked, h, retrace, dd, rescale), got, want, worst)
        again = _launch(ops, inp, h, retrace, dd, rescale)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again)), "two launches on the same inputs differ in bits"
    print(f"R2D2-ERR kernel {shape}: {len(combos)} cases, worst error as a fraction of its bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f"; forced rows: {sorted(cases)}")
    return cases


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_kernel_matches_the_yardstick_at_small_shapes(shape):
    flags = list(itertools.product((False, True), repeat=3))
    cases = _check(shape, [(masked, h, f) for masked in (False, True) for h in (1.0, 0.95) for f in flags])
    if shape == (32, 5, 2):  # the one small shape with room for every forced row
        assert len(cases) == 11, cases


@pytest.mark.parametrize("shape", LARGE, ids=str)
def test_kernel_matches_the_yardstick_at_large_shapes(shape):
    cases = _check(shape, [(True, 0.95, (True, True, True)), (False, 1.0, (True, False, False)), (True, 1.0, (False, True, True))])
    if shape[0] >= 11 and shape[1] > 1:
        assert len(cases) == 11, cases


def test_envelope_refusals_launch_nothing():
    lib = N.lib()
    B, S, A = 4, 3, 2
    f = lambda *s: torch.full(s, 7.0, device="cuda")  # noqa: E731
    q, qt, mu, rew, w = f(B, S + 1, A), f(B, S + 1, A), f(B, S), f(B, S), f(B)
    act, dones = torch.zeros((B, S), dtype=torch.int32, device="cuda"), torch.zeros((B, S), dtype=torch.uint8, device="cuda")
    outs = [f(B, S), f(1), f(B, S + 1, A), f(B)]
    ins = [q, qt, act, mu, rew, dones, None, w]

    def call(B=B, S=S, A=A, discount=0.9, h=1.0, null=None):
        p = [N.tptr(t) for t in ins + outs]
        if null is not None:
            p[null] = None
        return lib.srlx_r2d2_seq_td(B, S, A, *p[:8], discount, h, 1, 1, 0, *p[8:], N.torch_stream_ptr())

    bad = [dict(B=0), dict(B=1025), dict(S=0), dict(S=513), dict(A=0), dict(A=65), dict(discount=-1.0), dict(discount=float("nan")), dict(h=float("inf")),
           dict(h=-0.5)] + [dict(null=i) for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11)]
    for change in bad:
        assert call(**change) == N.ERR_INVALID and b"r2d2_seq_td" in lib.srlx_last_error(), change
    torch.cuda.synchronize()
    assert all(float(o.min()) == 7.0 == float(o.max()) for o in outs), "a refused call wrote an output"
    assert call() == N.OK
    torch.cuda.synchronize()
    assert all(float(o.max()) != 7.0 or float(o.min()) != 7.0 for o in outs)


# ---- one Trainer.train() against the yardstick ------------------------------------------------------------------------------------------------------------
def _runner(config, env="R2D2Walk-v0"):
    r = srl.Runner(env, config)
    r.set_device("cuda:0")
    return r


def _make_trainer(r):
    trainer = r.make_trainer()
    trainer.setup(r.context)  # (what the play loop does before the first train())
    return trainer


@functools.lru_cache(maxsize=None)
def _case(seed, retrace):
    """The CPU-acted episodes of tests/test_r2d2_cpu.py's gap test, their items in a proportional memory, and the first two batches that memory hands out."""
    R.register_walk()
    _, adds, cpu_parameter = R.worker_case(R.small_config(retrace), "R2D2Walk-v0", seed, TRAINER_EPISODES)
    c = R.small_config(retrace)
    c.memory.set_proportional()
    r = _runner(c)
    memory = r.make_memory()
    for item, _ in adds:  # the Worker's items, in the Worker's order
        memory.add(item, None)
    samples = [memory.sample() for _ in range(2)]
    return cpu_parameter.backup(serialized=True), samples


def _trainer(seed, retrace, backend, samples):
    """A fresh trainer on the case's initial parameters whose memory hands out `samples` in order and records what `update` receives."""
    state, _ = _case(seed, retrace)
    c = R.small_config(retrace)
    c.memory.set_proportional()
    r = _runner(c)
    parameter = r.make_parameter()
    parameter.restore(state, from_serialized=True)
    parameter.q_online.lstm_backend = parameter.q_target.lstm_backend = backend
    trainer = _make_trainer(r)
    queue, updates = list(samples), []
    trainer.memory.sample = lambda *a, **k: queue.pop(0)
    trainer.memory.update = lambda args, td, step: updates.append(np.array(td))
    return trainer, parameter, updates, c


@pytest.mark.parametrize("retrace", (True, False))
@pytest.mark.parametrize("seed", TRAINER_SEEDS)
def test_one_train_step_matches_the_yardstick(seed, retrace):
    _, samples = _case(seed, retrace)
    items, weights, _ = samples[0]
    err = {}
    for backend in ("torch", "srlx"):  # the torch arm first: its distance from float64 is the measuring stick of the srlx arm's gradients
        trainer, parameter, updates, c = _trainer(seed, retrace, backend, samples[:1])
        want = R.train_step(R.double_copy(parameter.q_online), R.double_copy(parameter.q_target), items, np.asarray(weights, np.float64), c)
        assert R.decision_gap(want, items, c.enable_double_dqn) >= GAP  # on the yardstick alone: no row is left out
        trainer.train()
        torch.cuda.synchronize()
        assert parameter.q_online.lstm_path == backend and trainer.train_count == 1
        loss_err = abs(trainer.info["loss"] - want.loss) / abs(want.loss)
        td_err = float(np.max(np.abs(updates[0] - want.td_mean) / (1e-6 + 1e-5 * np.abs(want.td_mean))))
        grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in parameter.q_online.named_parameters()}
        assert sorted(grads) == sorted(want.grads)
        err[backend] = {k: float(np.abs(grads[k] - want.grads[k]).max() / np.abs(want.grads[k]).max()) for k in grads}
        print(f"R2D2-ERR train seed {seed} retrace {retrace} {backend}: loss rel {loss_err:.3g}, td_mean {td_err:.3g} of its bar, "
              f"worst grad error / max|g| {max(err[backend].values()):.3g}")
        assert loss_err <= 1e-5 and td_err <= 1.0, (backend, loss_err, td_err)
    for k, e in err["srlx"].items():
        assert e <= max(1e-5, 2 * err["torch"][k]), (k, e, err["torch"][k])
    for k, e in err["torch"].items():
        assert e <= 1e-4, (k, e)  # (the measuring stick itself is float32's distance from float64, not something larger)


def test_two_fresh_trainers_give_equal_bits_after_two_steps():
    _, samples = _case(TRAINER_SEEDS[0], True)
    runs = []
    for _ in range(2):
        trainer, parameter, updates, _ = _trainer(TRAINER_SEEDS[0], True, "srlx", samples)
        trainer.train()
        trainer.train()
        torch.cuda.synchronize()
        assert parameter.q_online.lstm_path == "srlx" and trainer.train_count == 2
        runs.append(([v.cpu().numpy() for v in parameter.q_online.state_dict().values()], updates, trainer.info["loss"]))
    (sd_a, up_a, loss_a), (sd_b, up_b, loss_b) = runs
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(sd_a, sd_b)) and loss_a == loss_b
    assert all(np.array_equal(a, b) for a, b in zip(up_a, up_b))


# ---- other trainer and runner checks ----------------------------------------------------------------------------------------------------------------------
def _grid_runner(**kw):
    c = r2d2.Config(batch_size=4, burnin=2, sequence_length=3, lstm_units=16, **kw)
    c.hidden_block.set_dueling_network((32,))
    c.memory.set_proportional()
    c.memory.capacity, c.memory.warmup_size = 512, 8
    return _runner(c, "Grid")


def test_image_config_takes_a_step():
    c = r2d2.Config(batch_size=2, burnin=1, sequence_length=2, lstm_units=16, enable_rl_processors=False)
    c.hidden_block.set_dueling_network((32,))
    c.input_block.image.set_dqn_block()
    c.memory.warmup_size = 2
    r = _runner(c, srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(hw=(8, 8), n_actions=3, episode_len=5)))
    r.rollout(max_episodes=1, enable_progress=False)
    before = {k: v.clone() for k, v in r.parameter.q_online.state_dict().items()}
    trainer = _make_trainer(r)
    trainer.train()
    assert trainer.train_count == 1 and np.isfinite(trainer.info["loss"])
    after = r.parameter.q_online.state_dict()
    changed = {k.split(".")[0] for k in after if not torch.equal(before[k], after[k])}
    assert changed == {"in_block", "lstm_layer", "hidden_block"}, changed


def test_target_sync_at_zero_and_at_the_interval():
    r = _grid_runner(target_model_update_interval=2)
    r.rollout(max_episodes=2, enable_progress=False)
    trainer, p = _make_trainer(r), r.parameter
    same = lambda: all(torch.equal(a, b) for a, b in zip(p.q_online.state_dict().values(), p.q_target.state_dict().values()))  # noqa: E731
    syncs = []
    for _ in range(4):
        trainer.train()
        syncs.append((trainer.info["sync"], same()))
    assert syncs == [(1, True), (1, False), (2, True), (2, False)]  # train_count 0 and 2 sync (r2d2.py:101-103)


def test_backup_into_a_fresh_parameter_reproduces_the_acting_q_values():
    r = _grid_runner()
    r.rollout(max_episodes=1, enable_progress=False)
    _make_trainer(r).train()
    p = r.parameter
    fresh = _grid_runner().make_parameter()
    fresh.restore(p.backup(serialized=True), from_serialized=True)
    assert all(torch.equal(a, b) for a, b in zip(fresh.q_target.state_dict().values(), p.q_online.state_dict().values()))  # restore goes into both (:72-74)
    h_a, h_b = p.get_initial_hidden_state(), fresh.get_initial_hidden_state()
    for pos in ([1.0, 3.0], [2.0, 3.0], [3.0, 1.0]):
        state = np.array(pos, np.float32)[np.newaxis, np.newaxis, :]
        (q_a, h_a), (q_b, h_b) = p.predict_q(state, h_a), fresh.predict_q(state, h_b)
        assert np.array_equal(q_a.view(np.uint32), q_b.view(np.uint32))


def test_runner_trains_on_the_plugin_path_and_evaluates():
    r = _grid_runner()
    st = r.train(max_train_count=3, enable_progress=False)
    assert st.end_reason == "max_train_count over." and st.train_count == 3
    assert r.vector_reason == "no device engine for algorithm 'R2D2'"
    rewards = r.evaluate(max_episodes=2, enable_progress=False)
    assert len(rewards) == 2 and all(np.isfinite(x) for x in rewards)
    st = r.train_only(max_train_count=2, enable_progress=False)
    assert st.train_count >= 2


def test_train_mp_delivers_initial_priorities(monkeypatch):
    priorities = []
    inner = r2d2.Memory.add

    def add(self, batch, priority=None, serialized=False):  # (the learner finds the memory's worker functions by their names)
        priorities.append(priority)
        return inner(self, batch, priority, serialized)

    monkeypatch.setattr(r2d2.Memory, "add", add)
    r = _grid_runner()
    st = r.train_mp(actor_num=2, max_train_count=5, timeout=120, enable_mp_memory=False, enable_progress=False, trainer_parameter_send_interval=0.2,
                    actor_parameter_sync_interval=0.2)
    assert st.train_count >= 5 and st.end_reason == "max_train_count over."
    assert len(priorities) >= 8 and all(p is not None and np.isfinite(p) and p >= 0 for p in priorities)


@pytest.mark.slow
def test_r2d2_learns_the_grid():
    """Opt-in (SRLX_RUN_SLOW=1): 3000 updates on Grid reach a mean evaluation return above 0.3 (random play is about -1.4; the environment's own baseline is
    0.65)."""
    from simple_distributed_rl_amd.utils.common import set_seed

    set_seed(1, enable_gpu=True)
    c = r2d2.Config(batch_size=32, burnin=2, sequence_length=4, lstm_units=32, lr=0.001, target_model_update_interval=200, discount=0.95)
    c.hidden_block.set_dueling_network((64,))
    c.memory.set_proportional()
    c.memory.capacity, c.memory.warmup_size = 10_000, 200
    r = _runner(c, "Grid")
    r.train(max_train_count=3000, enable_progress=False)
    rewards = r.evaluate(max_episodes=20, enable_progress=False)
    print(f"R2D2-LEARN Grid: mean return {np.mean(rewards):.3f} over 20 episodes after 3000 updates")
    assert np.mean(rewards) > 0.3, rewards
