"""V-PPO without a GPU: the plugin's surface (Config, registrations, Worker, backup / restore), the "torch" backend against the float64 yardstick of
tests/vppo_reference.py on every case of tests/vppo_cases.py, the distance of every case from the kinks of the arithmetic, Runners on CPU parameters, and
libsrlx's host-side validation.  Bars: rtol 1e-5 / atol 1e-6; a gradient tensor at rtol 1e-5 with atol 1e-5 max |g|."""
import ctypes
import dataclasses
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo_v

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_cases as C  # noqa: E402
import vppo_reference as R  # noqa: E402


# ---- the plugin surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_config_fields_and_defaults_are_the_references():
    want = [
        ("epsilon", 0.1), ("test_epsilon", 0.0), ("policy_noise_normal_scale", 0.5), ("batch_size", 64), ("memory", None), ("input_block", None),
        ("hidden_block", None), ("value_block", None), ("policy_block", None), ("discount", 0.95), ("clip_range", 0.1), ("lr", 0.0002), ("lr_scheduler", None),
        ("entropy_weight", 0), ("loss_align_coeff", 0.1), ("max_grad_norm", 10), ("squashed_gaussian_policy", True), ("enable_stable_gradients", True),
        ("stable_gradients_scale_range", (1e-10, 10)),
    ]
    base = {f.name for f in dataclasses.fields(ppo_v.RLConfig)}
    own = [f.name for f in dataclasses.fields(ppo_v.Config) if f.name not in base]
    assert own == [k for k, _ in want]
    c = ppo_v.Config()
    for k, v in want:
        if v is not None:
            assert getattr(c, k) == v, k
    assert c.hidden_block.kwargs["layer_sizes"] == (64, 64) and c.value_block.kwargs["layer_sizes"] == (64,) and c.policy_block.kwargs["layer_sizes"] == ()
    assert c.input_block.value.kwargs["layer_sizes"] == () and c.lr_scheduler.schedule_type == ""
    for name in ("hidden_block", "value_block", "policy_block"):
        with pytest.raises(TypeError):
            ppo_v.Config(**{name: None})  # init=False, as in the reference
    c.set_model(32)
    assert c.hidden_block.kwargs["layer_sizes"] == (32, 32) and c.value_block.kwargs["layer_sizes"] == (32,) and c.policy_block.kwargs["layer_sizes"] == (32,)
    assert c.get_name() == "V-PPO" and c.get_framework() == "torch"


GRID_KEYS = ["hidden_block.hidden_layers.0", "hidden_block.hidden_layers.2", "value_block.hidden_layers.0", "value_out_layer", "policy_dist_block.h_layers.0"]
NORMAL_KEYS = GRID_KEYS[:4] + ["policy_dist_block.loc_layers.0", "policy_dist_block.log_scale_layers.0"]


@pytest.mark.parametrize("env, keys", [("Grid", GRID_KEYS), ("Pendulum-v1", NORMAL_KEYS)])
def test_both_registrations_resolve_and_make_the_references_module_tree(env, keys):
    runner = srl.Runner(env, ppo_v.Config())
    assert type(runner.make_memory()) is ppo_v.Memory and type(runner.make_trainer()) is ppo_v.Trainer and type(runner.make_worker().worker) is ppo_v.Worker
    p = runner.make_parameter()
    assert type(p) is ppo_v.Parameter
    assert list(p.net.state_dict()) == [f"{k}.{t}" for k in keys for t in ("weight", "bias")]
    from simple_distributed_rl_amd.device.vector_runner import engine_kind  # (there is no device engine for it)

    assert engine_kind(runner.rl_config) is None


def test_distributions_offer_what_the_references_do():
    cat = ppo_v.CategoricalDist(torch.tensor([[0.0, -30.0, 1.0]]))
    assert cat.probs().shape == (1, 3) and cat.logits().shape == (1, 3) and cat.sample().shape == (1, 3) and cat.sample(onehot=False).shape == (1, 1)
    lp = cat.log_prob(torch.tensor([[0.0, 1.0, 0.0]]))
    assert lp.shape == (1, 1) and float(lp) == pytest.approx(math.log(1e-7), rel=1e-6)  # log(clamp(p, 1e-7, 1)), p = 2.5e-14
    nd = ppo_v.NormalDist(torch.tensor([[0.5, -0.5]]), torch.tensor([[0.0, math.log(2.0)]]))
    assert nd.mean().tolist() == [[0.5, -0.5]] and nd.stddev()[0].tolist() == pytest.approx([1.0, 2.0]) and nd.sample().shape == (1, 2)
    x = torch.tensor([[1.5, 0.5]])
    want = [-0.5 * math.log(2 * math.pi) - 0.5, -0.5 * math.log(2 * math.pi) - math.log(2.0) - 0.125]
    assert nd.log_prob(x)[0].tolist() == pytest.approx(want, rel=1e-6)
    corr = sum(math.log(1.0 - math.tanh(v) ** 2) for v in (1.5, 0.5))
    assert nd.log_prob_sgp(x)[0].tolist() == pytest.approx([w - corr for w in want], rel=1e-6)  # the summed correction leaves every element
    block = ppo_v.NormalDistBlock(8, 2, enable_stable_gradients=True, stable_gradients_scale_range=(0.5, 2.0))
    with torch.no_grad():
        block.log_scale_layers[0].weight.zero_()
        block.log_scale_layers[0].bias.copy_(torch.tensor([-5.0, 5.0]))
    assert block(torch.zeros(1, 8)).stddev()[0].tolist() == pytest.approx([0.5, 2.0])


class _FakeRun:
    """What Worker.policy and Worker.on_step touch of a WorkerRun."""

    def __init__(self, n_actions):
        self.n, self.rows, self.sampled = n_actions, [], 0
        self._context = type("Ctx", (), dict(training=True, rl_render_mode=""))()
        self.state = self.next_state = None
        self.reward, self.terminated, self.done = 0.0, False, False

    def sample_action(self):
        self.sampled += 1
        return 2

    def get_onehot_action(self, action):
        return np.identity(self.n, dtype=np.float32)[action]

    def add_tracking(self, row):
        self.rows.append(row)

    def get_trackings(self):
        return [list(r.values()) for r in self.rows]


def test_worker_on_a_scripted_three_step_episode_gives_hand_worked_items(monkeypatch):
    """Step 0 takes the random branch (log(1/n)); steps 1 and 2 sample a policy that puts 1 - 4e-9 on action 1, so a sampled action 1 has log-probability -4e-9
    and the rigged action 0 of step 2 would have log(clamp(1e-9, 1e-7, 1)) = log(1e-7): the floor of log(1e-6) is checked on a log-probability set by hand.
    Items arrive in reversed order with total_reward = reward + discount * total_reward."""
    cfg = C.make_config(4, 0, 3, (32,), (), (), discount=0.5, epsilon=0.25)
    p = ppo_v.Parameter(cfg)
    with torch.no_grad():
        p.net.policy_dist_block.h_layers[0].weight.zero_()
        p.net.policy_dist_block.h_layers[0].bias.copy_(torch.tensor([-20.0, 0.0, -20.0]))
    mem = []
    w = ppo_v.Worker(cfg, p, type("Mem", (), dict(add=lambda self, item: mem.append(item)))())
    run = _FakeRun(3)
    w._set_worker_run(run)
    w.on_setup(run, None)
    draws = iter([0.1, 0.9, 0.9])  # epsilon 0.25: random, policy, policy
    monkeypatch.setattr(random, "random", lambda: next(draws))
    states = [np.full(4, float(k), np.float32) for k in range(4)]
    rewards, actions = [1.0, 2.0, 4.0], []
    for k in range(3):
        run.state, run.next_state, run.reward = states[k], states[k + 1], rewards[k]
        run.terminated = run.done = k == 2
        actions.append(w.policy(run))
        if k == 2:
            w.log_prob = np.array([-20.0], np.float32)  # under the floor
        w.on_step(run)
        assert len(mem) == (3 if k == 2 else 0)
    assert actions == [2, 1, 1] and run.sampled == 1
    assert [it[0][0] for it in mem] == [2.0, 1.0, 0.0] and [it[1][0] for it in mem] == [3.0, 2.0, 1.0]  # reversed
    assert [it[4] for it in mem] == [4.0, 2.0, 1.0] and [it[5] for it in mem] == [0, 1, 1]
    assert [it[6] for it in mem] == [4.0, 2.0 + 0.5 * 4.0, 1.0 + 0.5 * 4.0]
    assert mem[2][2].tolist() == [0.0, 0.0, 1.0] and mem[1][2].tolist() == [0.0, 1.0, 0.0]
    assert float(mem[2][3][0]) == pytest.approx(math.log(1.0 / 3.0), rel=1e-12)
    assert float(mem[1][3][0]) == pytest.approx(0.0, abs=1e-6)
    assert float(mem[0][3][0]) == pytest.approx(math.log(1e-6), rel=1e-6)
    run._context.training = False
    w.on_step(run)
    assert len(mem) == 3


def test_continuous_worker_squashes_and_evaluates_at_the_mean(monkeypatch):
    torch.manual_seed(5)
    cfg = C.make_config(3, 1, 2, (32,), (), (), epsilon=0.0)
    p = ppo_v.Parameter(cfg)
    w = ppo_v.Worker(cfg, p, None)
    run = _FakeRun(2)
    run.state = np.ones(3, np.float32)
    w._set_worker_run(run)
    w.on_setup(run, None)
    np.random.seed(0)
    env_action = w.policy(run)
    with torch.no_grad():
        dist = p.net(torch.ones(1, 3))[1]
    loc, scale = dist.mean().numpy()[0], dist.stddev().numpy()[0]
    assert env_action == pytest.approx(np.tanh(w.action), rel=1e-5, abs=1e-6)  # (the environment's action is float32) and w.log_prob.shape == (2,)
    lp = -0.5 * math.log(2 * math.pi) - np.log(scale) - 0.5 * ((w.action - loc) / scale) ** 2 - np.sum(np.log(1.0 - np.tanh(w.action) ** 2))
    assert w.log_prob == pytest.approx(lp, rel=1e-6)
    run._context.training = False
    assert w.policy(run) == pytest.approx(np.tanh(loc), rel=1e-5, abs=1e-6)
    cfg.squashed_gaussian_policy = False
    assert w.policy(run) == pytest.approx(np.clip(loc, -1, 1), rel=1e-5, abs=1e-6)


def test_backup_restore_round_trip():
    src, dst = C.make_parameter("default-b15", seed=1), C.make_parameter("default-b15", seed=2)
    ptrs = [t.data_ptr() for t in dst.net.parameters()]
    data = src.call_backup(serialized=True)
    assert type(data) is dict and list(data) == list(src.net.state_dict())
    dst.call_restore(data, from_serialized=True)
    assert all(torch.equal(a, b) for a, b in zip(src.net.parameters(), dst.net.parameters()))
    assert ptrs == [t.data_ptr() for t in dst.net.parameters()]  # in place: a libsrlx backend holds these tensors by address
    dst.restore(src.backup())
    assert all(torch.equal(a, b) for a, b in zip(src.net.parameters(), dst.net.parameters()))


# ---- the "torch" backend against the yardstick ---------------------------------------------------------------------------------------------------------------------
def _frac(got, want, gradient=False):
    got, want = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(want).detach().double().reshape(-1)
    atol = 1e-5 * float(want.abs().max()) if gradient else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


@pytest.mark.parametrize("name", C.NAMES)
def test_torch_backend_follows_the_yardstick(name):
    """Both updates of the case: v, n_v, new_logpi, the four losses, the norm and every gradient after the clip against the yardstick at the bars; the
    parameters after each step against the yardstick's Adam formulas stepping on the backend's own float32 gradients.  The parameters are split off in this way
     because float32 autograd cannot meet 1e-6 on them directly where a layer is wide: Adam's first steps are lr g / (|g| + eps), an entry of the
    256 x 512 layer of wide-b33 whose gradient cancels to about eps turns the float32 sums' relative error into a parameter error of 1.82 of the bar (every
    other case is under 0.11 of it); the float64-accumulating kernels are held to the direct comparison in tests/test_vppo_gpu.py, and the backend itself to it
    on the reference's own cases in tests/test_vppo_pinned_cpu.py."""
    refs, batches = C.reference(name), C.make_batches(name)
    p = C.make_parameter(name)
    cfg = p.config
    y = C._yardstick(name, p)
    tr = ppo_v.Trainer(cfg, p, None)
    tr.update_backend = "torch"
    tr.on_setup()
    worst = {}
    for k, (b, ref) in enumerate(zip(batches, refs)):
        B = b["state"].shape[0]
        col = lambda x: x.float().reshape(B, 1)  # noqa: E731
        out = tr.train_on_batch(b["state"].float(), b["n_state"].float(), C.onehot(name, b["action"]).float(), b["old_logpi"].float(), col(b["reward"]),
                                col(b["not_terminated"]), col(b["total_reward"]))
        assert tr.update_path == "torch" and tr.train_count == k + 1
        for key in ("v", "n_v", "new_logpi"):
            worst[key] = max(worst.get(key, 0.0), _frac(out[key], ref[key]))
        for j, key in enumerate(("loss_value", "loss_v_align", "loss_policy", "loss_e", "norm")):
            worst[key] = max(worst.get(key, 0.0), _frac(out["scalars"][j], ref[key]))
        grads = [t.grad.clone() for t in p.net.parameters()]
        worst["grads"] = max([worst.get("grads", 0.0)] + [_frac(g, w, gradient=True) for g, w in zip(grads, ref["grads"])])
        mine = y.update(**b, step_on=grads)
        worst["params"] = max([worst.get("params", 0.0)] + [_frac(t, w) for t, w in zip(p.net.parameters(), mine["params"])])
        info_keys = {"loss_value", "loss_v_align", "loss_policy"} | ({"loss_e"} if cfg.entropy_weight > 0 else set())
        assert set(tr.info) == info_keys
    print(f"VPPO-CPU-ERR {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", C.NAMES)
def test_no_case_is_near_a_kink(name):
    """The float64 restatement puts no element of either update within 1e-3 (relative) of a kink: 1 +- clip_range, Huber's |d| = 1, p = 1e-7, the log-scale
    clamp's ends, 1 - tanh^2 = 1e-10, norm = max_grad_norm, a tie of the surrogate's minimum outside the clip range (adv = 0).  This is what lets every
    comparison against float32 code keep every element of every case."""
    for ref in C.reference(name):
        assert ref["margin"] >= 1e-3, ref["margin"]


def test_the_cases_stand_on_both_sides_of_every_kink():
    total = {}
    for name in C.NAMES:
        for ref in C.reference(name):
            for k, v in ref["regions"].items():
                total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    assert {"norm_below", "norm_above", "p_below", "ls_below", "ls_above", "squash_clamped", "huber_linear", "ratio_above_adv-", "ratio_below_adv+"} <= set(total)
    forced = C.reference("normal-forced")[0]["regions"]
    assert forced["ls_below"] and forced["ls_inside"] and forced["ls_above"] and forced["squash_clamped"]
    assert C.reference("cat-forced")[0]["regions"]["p_below"] >= 3
    b = C.make_batches("default-b15")[0]
    assert float(b["not_terminated"][0]) == 0.0 and float(b["not_terminated"][1]) == 1.0


def test_yardstick_on_hand_worked_numbers():
    """One row, two actions, a network whose outputs are its biases: v = 0.5, logits (0, log 3) so p = (0.25, 0.75); action 1, old log-probability log 0.5:
    ratio 1.5, clipped to 1.1; r = 2, terminated: q = 2, adv = 1.5."""
    cfg = C.make_config(1, 0, 2, (32,), (), (), entropy_weight=0.1)
    p = ppo_v.Parameter(cfg)
    with torch.no_grad():
        for t in p.net.parameters():
            t.zero_()
        p.net.value_out_layer.bias.fill_(0.5)
        p.net.policy_dist_block.h_layers[0].bias.copy_(torch.tensor([0.0, math.log(3.0)]))
    y = R.Yardstick(p, 2e-4, 0.95, 0.1, 0.1, 0.1, 10.0, False)
    one = lambda v: torch.tensor([v], dtype=torch.float64)  # noqa: E731
    out = y.update(torch.zeros(1, 1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64), torch.tensor([1]), one(math.log(0.5)).reshape(1, 1), one(2.0),
                   one(0.0), one(1.0))
    assert float(out["new_logpi"]) == pytest.approx(math.log(0.75)) and float(out["v"]) == 0.5
    assert out["loss_value"] == pytest.approx(abs(1.5 * 2.0 - 0.5) - 0.5)  # Huber's linear region
    assert out["loss_v_align"] == pytest.approx((1.5 * 1.0 - 0.5) ** 2)
    assert out["loss_policy"] == pytest.approx(-min(1.5 * 1.5, 1.1 * 1.5))
    assert out["loss_e"] == pytest.approx(0.75 * math.log(0.75))
    g_lp = 0.1 * (0.75 * math.log(0.75) + 0.75)  # the surrogate is clipped with adv > 0: only the entropy term reaches the logits
    assert out["raw_grads"][-1].tolist() == pytest.approx([g_lp * -0.25, g_lp * 0.25])
    assert float(out["raw_grads"][3]) == pytest.approx(-1.0 + 0.1 * -2.0 * (1.5 - 0.5))  # d / d v: Huber's -sign(d) and the alignment term


# ---- Runner -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["Grid", "Pendulum-v1"])
def test_runner_trains_and_evaluates_on_cpu_parameters(env):
    cfg = ppo_v.Config(batch_size=16)
    cfg.memory.warmup_size = 32
    runner = srl.Runner(env, cfg)
    runner.set_device("cpu")
    start = [t.detach().clone() for t in runner.make_parameter().net.parameters()]
    runner.train(max_train_count=5)
    tr = runner.trainer
    assert tr.train_count == 5 and tr.update_path == "torch"
    assert tr.why_not_srlx_update == ("the parameters are CPU tensors" if ppo_v.Trainer.update_backend == "srlx" else "")
    assert set(tr.info) == {"loss_value", "loss_v_align", "loss_policy"} and all(np.isfinite(v) for v in tr.info.values())
    assert not any(torch.equal(a, c) for a, c in zip(start, runner.parameter.net.parameters()))
    assert runner.vector_reason == "the run is not on a GPU device"
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)


def test_rollout_then_train_only_on_the_plugin_path():
    cfg = ppo_v.Config(batch_size=16)
    cfg.memory.warmup_size = 32
    runner = srl.Runner("Grid", cfg)
    runner.set_device("cpu")
    runner.rollout(max_memory=64)
    assert runner.memory.length() >= 64 and len(runner.memory.sample()[0]) == 7  # [state, next_state, action, log_prob, reward, not_done, total_reward]
    runner.train_only(max_train_count=3)
    assert runner.trainer.train_count == 3 and runner.trainer.update_path == "torch"


def test_a_request_for_srlx_on_cpu_parameters_is_served_by_torch_and_says_why():
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    p = C.make_parameter("default-b15")
    assert VppoUpdate.why_not(p, 15, p.config) == "the parameters are CPU tensors" and not VppoUpdate.serves(p)
    tr = ppo_v.Trainer(p.config, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    b = C.make_batches("default-b15")[0]
    col = lambda x: x.float().reshape(15, 1)  # noqa: E731
    tr.train_on_batch(b["state"].float(), b["n_state"].float(), C.onehot("default-b15", b["action"]).float(), b["old_logpi"].float(), col(b["reward"]),
                      col(b["not_terminated"]), col(b["total_reward"]))
    assert tr.update_path == "torch" and tr.why_not_srlx_update == "the parameters are CPU tensors"
    with pytest.raises(ValueError, match="'srlx' or 'torch'"):
        t2 = ppo_v.Trainer(p.config, p, None)
        t2.update_backend = "eager"
        t2.on_setup()
        t2._choose_backend(1)


# ---- libsrlx's host validation ------------------------------------------------------------------------------------------------------------------------------------
def _widths(w):
    return ctypes.cast((ctypes.c_int * 4)(*(list(w) + [0, 0, 0, 0])[:4]), N.c_p)


def test_create_refuses_every_edge_of_the_envelope_without_a_device():
    """srlx_vppo_create validates before it touches a device; srlx_vppo_scratch_floats answers -1 for the same shapes and a positive count inside."""
    lib = N.lib()
    ok = dict(D=4, head=0, n_out=2, trunk=(64, 64), value=(64,), policy=(), max_batch=64)
    bad = [dict(D=0), dict(D=257), dict(head=2), dict(head=-1), dict(n_out=1), dict(n_out=17), dict(head=1, n_out=0), dict(head=1, n_out=9), dict(trunk=()),
           dict(trunk=(64, 64, 64, 64)), dict(trunk=(31,)), dict(trunk=(48,)), dict(trunk=(544,)), dict(trunk=(64, 0)), dict(value=(64, 64, 64)), dict(value=(48,)),
           dict(value=(544,)), dict(policy=(64, 64, 64)), dict(policy=(16,)), dict(policy=(64, 40)), dict(max_batch=0), dict(max_batch=257)]
    def call(c):
        args = (c["D"], c["head"], c["n_out"], len(c["trunk"]), _widths(c["trunk"]), len(c["value"]), _widths(c["value"]), len(c["policy"]), _widths(c["policy"]),
                c["max_batch"])
        h = N.c_p()
        return lib.srlx_vppo_create(ctypes.byref(h), *args, 0), h, lib.srlx_last_error(), lib.srlx_vppo_scratch_floats(*args)
    for change in bad:
        st, h, err, floats = call(dict(ok, **change))
        assert st == N.ERR_INVALID and not h and b"vppo_create" in err and floats == -1, change
    edges = [dict(D=1), dict(D=256), dict(n_out=16), dict(head=1, n_out=1), dict(head=1, n_out=8), dict(trunk=(32,)), dict(trunk=(512, 512, 512)), dict(value=()),
             dict(value=(512, 32)), dict(policy=(32, 512)), dict(max_batch=1), dict(max_batch=256)]
    for change in [{}] + edges:
        c = dict(ok, **change)
        assert lib.srlx_vppo_scratch_floats(c["D"], c["head"], c["n_out"], len(c["trunk"]), _widths(c["trunk"]), len(c["value"]), _widths(c["value"]),
                                            len(c["policy"]), _widths(c["policy"]), c["max_batch"]) > 0, change
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    assert VppoUpdate.envelope_reason(4, 0, 2, (64, 64), (64,), (), 64) == ""  # ppo_v.Config()'s defaults are inside
    assert "above max_batch" in VppoUpdate.envelope_reason(4, 0, 2, (64, 64), (64,), (), 257)
    assert "outside the envelope" in VppoUpdate.envelope_reason(4, 0, 2, (48,), (64,), (), 64)


def test_null_arguments_are_refused_without_a_device():
    lib = N.lib()
    assert lib.srlx_vppo_create(None, 4, 0, 2, 1, _widths((64,)), 0, _widths(()), 0, _widths(()), 8, 0) == N.ERR_INVALID
    assert lib.srlx_vppo_destroy(None) == 0
    assert lib.srlx_vppo_bind(None, None) == N.ERR_INVALID and b"vppo_bind" in lib.srlx_last_error()
    assert lib.srlx_vppo_bind_grads(None, None, None) == N.ERR_INVALID and lib.srlx_vppo_bind_adam(None, None, None, 0, 0.9, 0.999, 1e-8) == N.ERR_INVALID
    assert lib.srlx_vppo_steps(None) == -1 and b"vppo_steps" in lib.srlx_last_error()
    assert lib.srlx_vppo_forward(None, 1, None, 0.0, 1.0, None, None, None, None) == N.ERR_INVALID
    assert lib.srlx_vppo_update(None, 1, *([None] * 7), 1e-3, 0.9, 0.1, 0.0, 0.1, 10.0, 0, 0.0, 1.0, None, None, None, None, None) == N.ERR_INVALID


def test_why_not_names_what_keeps_a_block_on_torch():
    from simple_distributed_rl_amd.device.vppo import VppoUpdate, shape_of

    p = C.make_parameter("mixed-b17")
    assert shape_of(p) == (3, 0, 5, (32, 64, 96), (32, 64), (64, 32))
    assert shape_of(C.make_parameter("normal-k8")) == (1, 1, 8, (96,), (), (64, 64))
    cfg = C.make_config(4, 0, 2, (64,), (64,), ())
    cfg.value_block.set((64,), activation="tanh")
    assert "value_block is not a chain of Linear (with bias) + ReLU" in shape_of(ppo_v.Parameter(cfg))
    cfg = C.make_config(4, 0, 2, (64,), (64,), (), in_block_layers=(32,))
    assert shape_of(ppo_v.Parameter(cfg))[3] == (32, 64)  # an input value block's ReLU layers are the trunk's first
