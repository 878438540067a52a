"""Discrete SAC without a GPU: the plugin resolves and its surface is the reference's (srl/algorithms/sac/config.py:30-87, sac_tf_discrete.py:105-272), the
yardstick of tests/sacd_reference.py stands on hand-worked numbers, and every argument check of libsrlx's srlx_sacd_* entry points runs before any device call.
Parity with the TensorFlow reference is unpinned."""
import ctypes
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import sac

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_cases as C  # noqa: E402
import sacd_reference as R  # noqa: E402


# ---- the plugin surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_runner_resolves_the_four_plugin_classes():
    runner = srl.Runner("CartPole-v1", sac.Config())
    assert type(runner.make_memory()) is sac.Memory
    assert type(runner.make_parameter()) is sac.Parameter
    assert type(runner.make_trainer()) is sac.Trainer
    assert type(runner.make_worker().worker) is sac.Worker
    assert runner.rl_config.get_name() == "SAC_Discrete" and runner.rl_config.get_framework() == "torch"


def test_config_fields_and_defaults_are_the_references():
    want = [
        ("input_block", None), ("policy_block", None), ("q_block", None), ("batch_size", 32), ("memory", None), ("discount", 0.99), ("lr_policy", 0.0001),
        ("lr_policy_scheduler", None), ("lr_q", 0.0001), ("lr_q_scheduler", None), ("lr_alpha", 0.0001), ("lr_alpha_scheduler", None),
        ("soft_target_update_tau", 0.02), ("hard_target_update_interval", 10000), ("squashed_gaussian_policy", True), ("start_steps", 10000),
        ("entropy_alpha_auto_scale", True), ("entropy_alpha", 0.2), ("enable_stable_gradients", True), ("stable_gradients_scale_range", (1e-10, 10)),
    ]
    base = {f.name for f in dataclasses.fields(sac.RLConfig)}
    own = [f.name for f in dataclasses.fields(sac.Config) if f.name not in base]
    assert own == [k for k, _ in want]
    c = sac.Config()
    for k, v in want:
        if v is not None:
            assert getattr(c, k) == v, k
    assert c.policy_block.kwargs["layer_sizes"] == (64, 64, 64) and c.q_block.kwargs["layer_sizes"] == (128, 128, 128)
    assert c.input_block.value.kwargs["layer_sizes"] == ()
    for sch in (c.lr_policy_scheduler, c.lr_q_scheduler, c.lr_alpha_scheduler):
        assert sch.schedule_type == ""
    with pytest.raises(TypeError):
        sac.Config(policy_block=None)  # init=False, as in the reference


def test_continuous_action_space_is_refused_in_words():
    runner = srl.Runner("Pendulum-v1", sac.Config())
    with pytest.raises(Exception) as e:
        runner.make_parameter()
    assert not isinstance(e.value, KeyError)
    assert "only SAC_Discrete is" in str(e.value) and "SAC_Continuous" in str(e.value)


def test_backup_restore_round_trip_on_cpu_parameters():
    cfg = C.make_config(4, 2, (64, 64, 64), (128, 128, 128))
    src, dst = C.make_parameter(cfg, 1), C.make_parameter(cfg, 2)
    dst.load_log_alpha = True
    with torch.no_grad():
        src.log_alpha.fill_(-0.75)
    assert not torch.equal(src.q1_target.q_out_layer.weight, src.q1_online.q_out_layer.weight)
    data = src.call_backup(serialized=True)
    assert len(data) == 4 and [type(d) for d in data[:3]] == [dict] * 3
    dst.call_restore(data, from_serialized=True)
    for name in ("policy", "q1_online", "q2_online"):
        for a, b in zip(getattr(src, name).parameters(), getattr(dst, name).parameters()):
            assert torch.equal(a, b)
    for tgt, net in ((dst.q1_target, dst.q1_online), (dst.q2_target, dst.q2_online)):
        for a, b in zip(tgt.parameters(), net.parameters()):
            assert torch.equal(a, b)
    assert float(dst.log_alpha) == -0.75 and dst.log_alpha.dtype == torch.float32 and dst.load_log_alpha is False


def test_fresh_policy_is_uniform_and_log_alpha_starts_at_log_entropy_alpha():
    runner = srl.Runner("CartPole-v1", sac.Config())
    p = runner.make_parameter()
    logits = p.logits(np.random.default_rng(0).standard_normal((5, 4)).astype(np.float32))
    assert logits.shape == (5, 2) and (logits == 0).all()
    assert float(p.log_alpha) == pytest.approx(math.log(0.2), rel=1e-7) and p.log_alpha.dtype == torch.float32 and p.log_alpha.dim() == 0
    assert [k.split(".")[0] for k in p.q1_online.state_dict()][-2:] == ["q_out_layer"] * 2
    assert p.q1_online.q_block.hidden_layers[0].in_features == 4 + 2


class _FakeRun:
    """What Worker.policy touches of a WorkerRun."""

    def __init__(self, n_actions, state):
        self.n, self.state, self.step_in_training, self.sampled = n_actions, state, 0, 0
        self._context = type("Ctx", (), dict(training=True, rl_render_mode=""))()

    def sample_action(self):
        self.sampled += 1
        return self.sampled % self.n

    def get_onehot_action(self, action):
        return np.identity(self.n, dtype=np.float32)[action]


def test_worker_plays_random_actions_for_start_steps_then_samples_the_policy():
    cfg = C.make_config(4, 2, (64,), (64,), start_steps=5)
    p = C.make_parameter(cfg, 3)
    with torch.no_grad():
        p.policy.out_layer.weight.zero_()
        p.policy.out_layer.bias.copy_(torch.tensor([-30.0, 30.0]))  # the policy takes action 1
    w = sac.Worker(cfg, p, None)
    run = _FakeRun(2, np.zeros(4, np.float32))
    w._set_worker_run(run)
    actions = []
    for step in range(12):
        run.step_in_training = step
        actions.append(w.policy(run))
        assert w.action.tolist() == [1.0 - actions[-1], float(actions[-1])]
    assert run.sampled == 5 and actions[:5] == [1, 0, 1, 0, 1] and actions[5:] == [1] * 7
    run._context.training = False  # evaluation samples the policy at every step
    run.step_in_training = 0
    assert w.policy(run) == 1 and run.sampled == 5


def test_gumbel_max_sampler_follows_the_softmax():
    logits = np.array([0.3, -1.2, 1.1, 0.0, -3.0])
    p = np.exp(logits) / np.exp(logits).sum()
    rng = np.random.RandomState(7)
    n = 20_000
    counts = np.bincount([sac.gumbel_max_sample(logits, rng) for _ in range(n)], minlength=5)
    sd = np.sqrt(p * (1 - p) / n)
    assert (np.abs(counts / n - p) <= 4 * sd).all(), (counts / n, p, sd)


# ---- the yardstick's footing ------------------------------------------------------------------------------------------------------------------------------------
def _hand_parameter():
    """B 1, A 2, D 1, every block one layer of one unit, weights set by hand (see test_yardstick_on_hand_worked_numbers)."""
    cfg = C.make_config(1, 2, (1,), (1,))
    p = sac.Parameter(cfg)
    set_ = lambda t, v: t.copy_(torch.tensor(v, dtype=torch.float32).reshape(t.shape))  # noqa: E731
    with torch.no_grad():
        set_(p.policy.hidden_block.hidden_layers[0].weight, [1.0]), set_(p.policy.hidden_block.hidden_layers[0].bias, [0.0])
        set_(p.policy.out_layer.weight, [0.5, -0.5]), set_(p.policy.out_layer.bias, [0.0, 0.0])
        for q in (p.q1_online, p.q1_target):
            set_(q.q_block.hidden_layers[0].weight, [1.0, 0.5, -0.5]), set_(q.q_block.hidden_layers[0].bias, [0.0])
            set_(q.q_out_layer.weight, [2.0]), set_(q.q_out_layer.bias, [0.1])
        for q in (p.q2_online, p.q2_target):
            set_(q.q_block.hidden_layers[0].weight, [0.5, 1.0, 0.0]), set_(q.q_block.hidden_layers[0].bias, [0.2])
            set_(q.q_out_layer.weight, [1.0]), set_(q.q_out_layer.bias, [0.0])
    return p


def test_yardstick_on_hand_worked_numbers():
    """s = 1, a = 1, s' = 2, r = 0.5, not done; discount 0.9, alpha 0.2, tau 0.1, lr_q 0.01.
    policy: h = relu(s), logits = (0.5 h, -0.5 h).  q1: h = relu(s + 0.5 e_0 - 0.5 e_1), q = 2 h + 0.1.  q2: h = relu(0.5 s + e_0 + 0.2), q = h.
    At s' = 2: p' = softmax(1, -1); q1' = (5.1, 3.1), q2' = (2.2, 1.2), so qmin' = (2.2, 1.2).
    At (s, a) = (1, e_1): q1 = 1.1, q2 = 0.7, both below y, so every gradient entry with a non-zero input is negative and the first Adam step adds lr to it
    (m / (sqrt(v) + eps) = g / (|g| + 1e-8)):  q1 -> h = relu(1.01 s + 0.5 e_0 - 0.49 e_1 + 0.01), q = 2.01 h + 0.11;
                                               q2 -> h = relu(0.51 s + 1.0 e_0 + 0.01 e_1 + 0.21), q = 1.01 h + 0.01."""
    alpha, disc, tau = 0.2, 0.9, 0.1
    y = R.Yardstick(_hand_parameter(), lr_policy=0.01, lr_q=0.01, lr_alpha=0.01, discount=disc, tau=tau, auto_scale=True, target_entropy=-2)
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    out = y.update(t([1.0]), t([0.0, 1.0]), t([2.0]), t(0.5), t(0.0), hard_sync=False)
    p0n = 1 / (1 + math.exp(-2.0))
    p1n = 1 - p0n
    want_y = 0.5 + disc * (p0n * (2.2 - alpha * math.log(p0n)) + p1n * (1.2 - alpha * math.log(p1n)))
    assert float(out["y"][0]) == pytest.approx(want_y, rel=1e-7)  # (alpha is exp(float32 log 0.2))
    assert float(out["q1"][0]) == pytest.approx(1.1, rel=1e-7) and float(out["q2"][0]) == pytest.approx(0.7, rel=1e-7)
    assert float(out["q1_loss"]) == pytest.approx((want_y - 1.1) ** 2, rel=1e-6) and float(out["q2_loss"]) == pytest.approx((want_y - 0.7) ** 2, rel=1e-6)
    qv = (min(2.01 * (1.01 + 0.5 + 0.01) + 0.11, 1.01 * (0.51 + 1.0 + 0.21) + 0.01), min(2.01 * (1.01 - 0.49 + 0.01) + 0.11, 1.01 * (0.51 + 0.01 + 0.21) + 0.01))
    p0 = 1 / (1 + math.exp(-1.0))
    p1 = 1 - p0
    entropy = -(p0 * math.log(p0) + p1 * math.log(p1))
    assert float(out["entropy"][0]) == pytest.approx(entropy, rel=1e-7)
    assert float(out["policy_loss"]) == pytest.approx(p0 * (alpha * math.log(p0) - qv[0]) + p1 * (alpha * math.log(p1) - qv[1]), rel=1e-6)
    assert float(out["grads"]["log_alpha"]) == pytest.approx(alpha * (2 + entropy), rel=1e-6)  # -alpha (target_entropy - entropy)
    assert float(out["alpha_loss"]) == pytest.approx(alpha * (2 + entropy), rel=1e-6)
    assert float(y.q1_target.q_out_layer.bias[0]) == pytest.approx((1 - tau) * 0.1 + tau * 0.11, rel=1e-6)  # one soft-sync element


def test_yardstick_done_row_has_y_equal_to_reward():
    B, D, A, pw, qw = C.SHAPES[2]
    p = C.make_parameter(C.make_config(D, A, pw, qw), 11)
    b = C.make_batch(B, D, A, 12)
    y = R.Yardstick(p, C.LR, C.LR, C.LR, C.DISCOUNT, C.TAU, True, -A)
    out = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=True)
    assert b["done"][0] == 1 and float(out["y"][0]) == float(b["reward"][0])
    assert b["done"][1] == 0 and float(out["y"][1]) != float(b["reward"][1])
    for tgt, net in ((y.q1_target, y.q1_online), (y.q2_target, y.q2_online)):  # a hard sync copies
        assert all(torch.equal(a, c) for a, c in zip(tgt.parameters(), net.parameters()))


def test_yardstick_clipped_probability_carries_no_alpha_term():
    """The forced-clip construction: d policy_loss / d out_layer.bias of one row equals p_j (c_j - sum_a p_a c_a) with c_a = alpha L_a - qv_a + alpha only where
    p_a is inside the clip -- and differs from the same form with the alpha term everywhere."""
    B, D, A, pw, qw = C.SHAPES[C.CLIP_SHAPE]
    p = C.make_parameter(C.make_config(D, A, pw, qw), 13, clip_case=True)
    b = C.make_batch(1, D, A, 14)
    y = R.Yardstick(p, 0.0, 0.0, 0.0, C.DISCOUNT, C.TAU, False, -A)
    out = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=False)
    probs = out["probs"][0]
    assert float(probs[1]) < 5e-8 and 2e-7 < float(probs[2]) < 1e-4
    alpha = float(out["alpha"])
    qv = R.all_q(b["state"], A, y.q1_online, y.q2_online).detach()[0]
    L = torch.log(torch.clip(probs, 1e-7, 1))
    inside = (probs >= 1e-7).double()
    got = out["grads"]["policy"][-1]

    def closed(mask):
        c = alpha * L - qv + alpha * mask
        return probs * (c - (probs * c).sum())

    np.testing.assert_allclose(got, closed(inside), rtol=1e-9, atol=1e-18)
    # with the term everywhere the clipped entry would move by alpha p_1 (1 - p_1): 6 % of it here, against the 1e-9 it is matched to above
    missing = float(closed(torch.ones(A, dtype=torch.float64))[1] - got[1])
    assert missing == pytest.approx(alpha * float(probs[1]), rel=1e-6) and abs(missing) > 0.05 * abs(float(got[1]))


# ---- libsrlx's argument checks (before any device call) ---------------------------------------------------------------------------------------------------------
def _widths(w):
    return (ctypes.c_int * 4)(*(list(w) + [0, 0, 0, 0])[:4])


OK_SHAPE = dict(D=4, A=2, pw=(64,), qw=(64,), max_batch=32)
BAD_SHAPES = [dict(D=0), dict(D=257), dict(A=1), dict(A=17), dict(pw=()), dict(pw=(64, 64, 64, 64)), dict(pw=(0,)), dict(pw=(31,)), dict(pw=(48,)), dict(pw=(544,)),
              dict(pw=(64, 48)), dict(qw=()), dict(qw=(64, 64, 64, 64)), dict(qw=(16,)), dict(qw=(33,)), dict(qw=(544,)), dict(qw=(64, 64, 40)), dict(max_batch=0),
              dict(max_batch=257)]
EDGE_SHAPES = [dict(D=1), dict(D=256), dict(A=16), dict(pw=(32,)), dict(pw=(512, 512, 512)), dict(qw=(32,)), dict(qw=(512, 512, 512)), dict(max_batch=1),
               dict(max_batch=256)]


def _scratch(c):
    return N.lib().srlx_sacd_scratch_floats(c["D"], c["A"], len(c["pw"]), _widths(c["pw"]), len(c["qw"]), _widths(c["qw"]), c["max_batch"])


def test_envelope_is_checked_from_both_sides_without_a_device():
    lib = N.lib()
    assert _scratch(OK_SHAPE) > 0
    for change in EDGE_SHAPES:  # each bound from the inside
        assert _scratch(dict(OK_SHAPE, **change)) > 0, change
    for change in BAD_SHAPES:  # and from the outside: the size query says -1, create refuses with a message and leaves the handle NULL
        c = dict(OK_SHAPE, **change)
        assert _scratch(c) == -1, change
        h = N.c_p()
        st = lib.srlx_sacd_create(ctypes.byref(h), c["D"], c["A"], len(c["pw"]), _widths(c["pw"]), len(c["qw"]), _widths(c["qw"]), c["max_batch"], 0)
        assert st == N.ERR_INVALID and not h, change
        assert b"sacd_create" in lib.srlx_last_error(), change
    assert lib.srlx_sacd_scratch_floats(4, 2, 1, None, 1, _widths((64,)), 32) == -1  # NULL widths


def test_null_arguments_are_refused_without_a_device():
    lib = N.lib()
    w = _widths((64,))
    assert lib.srlx_sacd_create(None, 4, 2, 1, w, 1, w, 32, 0) == N.ERR_INVALID and b"sacd_create" in lib.srlx_last_error()
    some = ctypes.cast((ctypes.c_float * 4)(), N.c_p)
    for name, args in (("sacd_bind", (None, some, some)), ("sacd_bind_grads", (None, some, some)), ("sacd_bind_adam", (None, some, some, some, 0.9, 0.999, 1e-8)),
                       ("sacd_steps", (None, some)), ("sacd_forward", (None, 1, some, 0, some, some, None)),
                       ("sacd_update", (None, 1, some, some, some, some, some, 1e-4, 1e-4, 1e-4, 0.99, 0.02, 0, 1, -2.0, some, some, some, some, some, None))):
        assert getattr(lib, "srlx_" + name)(*args) == N.ERR_INVALID, name
        assert name.encode() in lib.srlx_last_error(), name
    assert lib.srlx_sacd_destroy(None) == 0


def test_binding_says_why_it_does_not_serve():
    from simple_distributed_rl_amd.device.sacd import MAX_BATCH, SacdUpdate

    cfg = C.make_config(4, 2, (64,), (64,))
    assert SacdUpdate.why_not(C.make_parameter(cfg, 5)) == "the parameters are CPU tensors"
    assert SacdUpdate.envelope_reason(4, 2, (64,), (64,), 32) == ""
    assert SacdUpdate.envelope_reason(4, 2, (64,), (64,), MAX_BATCH + 1) == f"batch size {MAX_BATCH + 1} above max_batch {MAX_BATCH}"
    for bad in ((300, 2, (64,), (64,)), (4, 17, (64,), (64,)), (4, 2, (48,), (64,)), (4, 2, (64,), (64, 64, 64, 64))):
        assert "outside the envelope" in SacdUpdate.envelope_reason(*bad, 32), bad
    from simple_distributed_rl_amd.device import sacd

    with_in_block = C.make_parameter(C.make_config(4, 2, (64,), (64,), in_block_layers=(32,)), 6)
    assert "input_block has layers of its own" in sacd.shape_of(with_in_block)
    assert sacd.shape_of(C.make_parameter(cfg, 5)) == (4, 2, (64,), (64,))


def test_torch_backend_on_cpu_follows_the_yardstick():
    """Trainer.train_on_batch on CPU parameters (the torch backend serves them and says why libsrlx does not): two updates, a hard and a soft sync, against the
    float64 yardstick at the bars of the GPU tests."""
    B, D, A, pw, qw = C.SHAPES[2]
    cfg = C.make_config(D, A, pw, qw, lr_policy=C.LR, lr_q=C.LR, lr_alpha=C.LR, hard_target_update_interval=5)
    p = C.make_parameter(cfg, 21)
    y = R.Yardstick(p, C.LR, C.LR, C.LR, cfg.discount, cfg.soft_target_update_tau, True, -A)
    tr = sac.Trainer(cfg, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    for k in range(2):
        b = C.make_batch(B, D, A, 30 + k)
        ref = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=k == 0)
        out = tr.train_on_batch(b["state"].float(), b["onehot"].float(), b["n_state"].float(), b["reward"].float(), b["done"].to(torch.uint8))
        assert tr.update_path == "torch" and tr.why_not_srlx_update == "the parameters are CPU tensors"
        for key in ("y", "q1", "q2", "entropy"):
            np.testing.assert_allclose(out[key].double(), ref[key], rtol=1e-5, atol=1e-6, err_msg=key)
        want = [float(ref[key]) for key in ("q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha")]
        np.testing.assert_allclose(out["scalars"].double(), want, rtol=1e-5, atol=1e-6)
        assert set(tr.info) == {"q1_loss", "q2_loss", "policy_loss", "alpha_loss", "alpha"}
    assert tr.train_count == 2
    for name in R.NETWORKS:
        for a, c in zip(getattr(p, name).parameters(), getattr(y, name).parameters()):
            np.testing.assert_allclose(a.detach().double(), c.detach(), rtol=1e-5, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(float(p.log_alpha.detach()), float(y.log_alpha.detach()), rtol=1e-5)
