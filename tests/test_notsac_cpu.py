"""NoT_SAC without a GPU: the plugin's surface (Config, registrations, Worker, backup / restore), the "torch" backend against the float64 yardstick of
tests/notsac_reference.py on every case of tests/notsac_cases.py, the distance of every case from the kinks of the arithmetic, the noise the trainer draws,
Runners on CPU parameters, and libsrlx's host-side validation.  Bars: rtol 1e-5 / atol 1e-6; a gradient tensor at rtol 1e-5 with atol 1e-5 max |g|."""
import ctypes
import dataclasses
import os
import random
import sys

import numpy as np
import pytest
import torch

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import sac_not

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import notsac_cases as C  # noqa: E402
import notsac_reference as R  # noqa: E402


# ---- the plugin surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_config_fields_and_defaults_are_the_references():
    want = [
        ("epsilon", 0.1), ("test_epsilon", 0), ("policy_training_scale", 0.5), ("batch_size", 64), ("memory", None), ("input_block", None),
        ("policy_block", None), ("q_block", None), ("act_emb_units", 64), ("lr", 0.0001), ("lr_scheduler", None), ("discount", 0.95),
        ("target_policy_temperature", 2.0), ("target_policy_noise_stddev", 0.2), ("target_policy_clip_range", 0.5), ("loss_align_coeff", 0.1),
        ("max_grad_norm", 10.0), ("squashed_gaussian_policy", True), ("enable_stable_gradients", True), ("stable_gradients_scale_range", (1e-10, 10)),
    ]
    base = {f.name for f in dataclasses.fields(sac_not.RLConfig)}
    own = [f.name for f in dataclasses.fields(sac_not.Config) if f.name not in base]
    assert own == [k for k, _ in want]
    c = sac_not.Config()
    for k, v in want:
        if v is not None:
            assert getattr(c, k) == v, k
    assert c.policy_block.kwargs["layer_sizes"] == (512,) and c.q_block.kwargs["layer_sizes"] == (512,)
    assert c.input_block.value.kwargs["layer_sizes"] == () and c.lr_scheduler.schedule_type == ""
    for name in ("policy_block", "q_block"):
        with pytest.raises(TypeError):
            sac_not.Config(**{name: None})  # init=False, as in the reference
    c.set_model(32)
    assert c.policy_block.kwargs["layer_sizes"] == (32, 32) and c.q_block.kwargs["layer_sizes"] == (32, 32) and c.act_emb_units == 32
    assert c.get_name() == "NoT_SAC" and c.get_framework() == "torch"


Q_KEYS = ["act_block.0", "q_block.hidden_layers.0", "q_out_layer"]
GRID_KEYS = ["policy_block.hidden_layers.0", "policy_dist_block.h_layers.0"]
NORMAL_KEYS = ["policy_block.hidden_layers.0", "policy_dist_block.loc_layers.0", "policy_dist_block.log_scale_layers.0"]


@pytest.mark.parametrize("env, keys, n_act", [("Grid", GRID_KEYS, 4), ("Pendulum-v1", NORMAL_KEYS, 1)])
def test_both_registrations_resolve_and_make_the_references_module_trees(env, keys, n_act):
    runner = srl.Runner(env, sac_not.Config())
    assert type(runner.make_memory()) is sac_not.Memory and type(runner.make_trainer()) is sac_not.Trainer and type(runner.make_worker().worker) is sac_not.Worker
    p = runner.make_parameter()
    assert type(p) is sac_not.Parameter
    assert list(p.policy.state_dict()) == [f"{k}.{t}" for k in keys for t in ("weight", "bias")]
    assert list(p.qnet.state_dict()) == [f"{k}.{t}" for k in Q_KEYS for t in ("weight", "bias")]
    assert tuple(p.qnet.act_block[0].weight.shape) == (64, n_act) and type(p.qnet.act_block[1]) is torch.nn.SiLU
    assert p.qnet.q_block.hidden_layers[0].in_features == p.policy.policy_block.hidden_layers[0].in_features + 64
    from simple_distributed_rl_amd.device.vector_runner import engine_kind, why_not_vector  # (there is no device engine for it)

    assert engine_kind(runner.rl_config) is None
    ctx = type("Ctx", (), dict(used_device_torch="cuda:0"))()
    assert why_not_vector(ctx, None, runner.rl_config) == "no device engine for algorithm 'NoT_SAC'"


def test_gumbel_head_offers_what_the_update_uses():
    u = torch.tensor([[0.5, 0.25, 0.75]])
    want = -torch.log(-torch.log(u + 1e-6) + 1e-6)
    assert torch.equal(sac_not.gumbel_inverse(u), want)
    dist = sac_not.CategoricalGumbelDist(torch.tensor([[0.0, 1.0, -1.0]]))
    assert dist.sample(onehot=True, noise=u).tolist() == [[0.0, 1.0, 0.0]] and dist.sample(noise=u).tolist() == [[1]]
    assert dist.sample(temperature=2.0, onehot=True, noise=u).tolist() == [[0.0, 1.0, 0.0]]  # a positive temperature never moves the argmax
    assert torch.allclose(dist.rsample(noise=u), torch.softmax(dist.logits + want, dim=-1), rtol=0, atol=0)
    assert dist.rsample().shape == (1, 3) and float(dist.rsample().sum()) == pytest.approx(1.0, rel=1e-6)
    assert dist.probs().tolist() == torch.softmax(dist.logits, dim=-1).tolist()


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


def _worker(cfg, p, n, mem=None):
    w = sac_not.Worker(cfg, p, type("Mem", (), dict(add=lambda self, item: mem.append(item)))() if mem is not None else None)
    run = _FakeRun(n)
    w._set_worker_run(run)
    w.on_setup(run, None)
    return w, run


def test_discrete_worker_on_a_scripted_three_step_episode_gives_hand_worked_items(monkeypatch):
    """Step 0 takes the epsilon branch (the one-hot of the sampled action 2); steps 1 and 2 take the Gumbel-max of logits (-20, 0, -20) + gumbel(u), which is
    action 1 for every u of a seeded draw (a Gumbel difference of 20 has probability 2e-9).  Items arrive in reversed order with the discounted return."""
    cfg = C.make_config(4, 0, 3, (32,), (32,), 32, discount=0.5, epsilon=0.25)
    p = sac_not.Parameter(cfg)
    with torch.no_grad():
        p.policy.policy_dist_block.h_layers[0].weight.zero_()
        p.policy.policy_dist_block.h_layers[0].bias.copy_(torch.tensor([-20.0, 0.0, -20.0]))
    mem = []
    w, run = _worker(cfg, p, 3, mem)
    draws = iter([0.1, 0.9, 0.9])  # epsilon 0.25: random, policy, policy
    monkeypatch.setattr(random, "random", lambda: next(draws))
    torch.manual_seed(0)
    states = [np.full(4, float(k), np.float32) for k in range(4)]
    rewards, actions = [1.0, 2.0, 4.0], []
    for k in range(3):
        run.state, run.next_state, run.reward = states[k], states[k + 1], rewards[k]
        run.terminated = run.done = k == 2
        actions.append(w.policy(run))
        w.on_step(run)
        assert len(mem) == (3 if k == 2 else 0)
    assert actions == [2, 1, 1] and run.sampled == 1
    assert all(len(it) == 6 for it in mem)  # [state, next_state, action, reward, not_done, total_reward]
    assert [it[0][0] for it in mem] == [2.0, 1.0, 0.0] and [it[1][0] for it in mem] == [3.0, 2.0, 1.0]  # reversed
    assert [it[3] for it in mem] == [4.0, 2.0, 1.0] and [it[4] for it in mem] == [0, 1, 1]
    assert [it[5] for it in mem] == [4.0, 2.0 + 0.5 * 4.0, 1.0 + 0.5 * 4.0]
    assert mem[2][2].tolist() == [0.0, 0.0, 1.0] and mem[1][2].tolist() == [0.0, 1.0, 0.0] and mem[0][2].tolist() == [0.0, 1.0, 0.0]  # the stored one-hot
    run._context.training = False
    w.on_step(run)
    assert len(mem) == 3


def test_discrete_worker_samples_the_gumbel_max_of_a_seeded_draw():
    cfg = C.make_config(4, 0, 5, (32,), (32,), 32, epsilon=0.0)
    torch.manual_seed(11)
    p = sac_not.Parameter(cfg)
    w, run = _worker(cfg, p, 5)
    run.state = np.ones(4, np.float32)
    with torch.no_grad():
        logits = p.policy(torch.ones(1, 4)).logits
    for seed in range(8):
        torch.manual_seed(seed)
        u = torch.rand(1, 5)
        torch.manual_seed(seed)
        a = w.policy(run)
        assert a == int(torch.argmax(logits + sac_not.gumbel_inverse(u))) and w.action.tolist() == np.identity(5)[a].tolist()


def test_continuous_worker_draws_at_the_training_scale_and_evaluates_at_the_mean():
    torch.manual_seed(5)
    cfg = C.make_config(3, 1, 2, (32,), (32,), 32, policy_training_scale=0.25)
    p = sac_not.Parameter(cfg)
    w, run = _worker(cfg, p, 2)
    run.state = np.ones(3, np.float32)
    with torch.no_grad():
        loc = p.policy(torch.ones(1, 3)).mean().numpy()[0]
    np.random.seed(0)
    want = np.random.normal(loc, 0.25, size=2)
    np.random.seed(0)
    env_action = w.policy(run)
    assert w.action.tolist() == np.tanh(want).tolist()  # what is stored is the squashed action
    assert env_action == pytest.approx(np.tanh(want), rel=1e-5, abs=1e-6)  # [-1, 1] onto the space's own [-1, 1]
    run._context.training = False
    assert w.policy(run) == pytest.approx(np.tanh(loc), rel=1e-5, abs=1e-6)
    cfg.squashed_gaussian_policy = False
    assert w.policy(run) == pytest.approx(np.clip(loc, -1, 1), rel=1e-5, abs=1e-6) and w.action.tolist() == loc.tolist()


def test_backup_restore_round_trip_in_place():
    src, dst = C.make_parameter("default-b16", seed=1), C.make_parameter("default-b16", seed=2)
    tensors = lambda p: list(p.policy.parameters()) + list(p.qnet.parameters())  # noqa: E731
    ptrs = [t.data_ptr() for t in tensors(dst)]
    data = src.call_backup(serialized=True)
    assert type(data) is list and len(data) == 2 and list(data[0]) == list(src.policy.state_dict()) and list(data[1]) == list(src.qnet.state_dict())
    dst.call_restore(data, from_serialized=True)
    assert all(torch.equal(a, b) for a, b in zip(tensors(src), tensors(dst)))
    assert ptrs == [t.data_ptr() for t in tensors(dst)]  # in place: a libsrlx backend holds these tensors by address
    dst.restore(src.backup())
    assert all(torch.equal(a, b) for a, b in zip(tensors(src), tensors(dst)))


# ---- the "torch" backend against the yardstick ---------------------------------------------------------------------------------------------------------------------
def _frac(got, want, gradient=False):
    got, want = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(want).detach().double().reshape(-1)
    atol = 1e-5 * float(want.abs().max()) if gradient else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _args(b):
    B = b["state"].shape[0]
    col = lambda x: x.float().reshape(B, 1)  # noqa: E731
    return (b["state"].float(), b["n_state"].float(), b["action"].float(), col(b["reward"]), col(b["not_terminated"]), col(b["total_reward"]))


SCALARS = ("loss_q", "loss_q_align", "loss_policy", "norm_q", "norm_policy")


@pytest.mark.parametrize("name", C.NAMES)
def test_torch_backend_follows_the_yardstick(name):
    """Both updates of the case: q, target_q, next_action, pi_action, the three losses, both norms and every gradient of both networks after its clip against
    the yardstick at the bars; the parameters after each step against the yardstick's Adam formulas stepping on the backend's own float32 gradients (the split
    of tests/test_vppo_cpu.py and DESIGN.md 7m: Adam's first steps are lr g / (|g| + eps), and a float32 sum that cancels to about eps cannot meet 1e-6 on a
    parameter directly; the float64-accumulating kernels are held to the direct comparison in tests/test_notsac_gpu.py)."""
    refs, batches = C.reference(name), C.make_batches(name)
    p = C.make_parameter(name)
    y = C.yardstick(name, p)
    tr = sac_not.Trainer(p.config, p, None)
    tr.update_backend = "torch"
    tr.on_setup()
    worst = {}
    for k, (b, ref) in enumerate(zip(batches, refs)):
        # the Q gradients are read between the two steps: the policy step's backward adds to them (nobody reads those)
        seen = {}
        tr._backend_for(b["state"].shape[0])
        step = tr.opt_q.step
        tr.opt_q.step = lambda *a, **kw: (seen.update(q=[t.grad.clone() for t in p.qnet.parameters()]), step(*a, **kw))[1]
        out = tr.train_on_batch(*_args(b), noise=b["noise"])
        tr.opt_q.step = step
        assert tr.update_path == "torch" and tr.train_count == k + 1
        for key in ("q", "target_q", "next_action", "pi_action"):
            worst[key] = max(worst.get(key, 0.0), _frac(out[key], ref[key]))
        for j, key in enumerate(SCALARS):
            worst[key] = max(worst.get(key, 0.0), _frac(out["scalars"][j], ref[key]))
        p_grads = [t.grad.clone() for t in p.policy.parameters()]
        worst["q_grads"] = max([worst.get("q_grads", 0.0)] + [_frac(g, w, gradient=True) for g, w in zip(seen["q"], ref["q_grads"])])
        worst["p_grads"] = max([worst.get("p_grads", 0.0)] + [_frac(g, w, gradient=True) for g, w in zip(p_grads, ref["p_grads"])])
        mine = y.update(**b, step_on=(seen["q"], p_grads))
        got = list(p.qnet.parameters()) + list(p.policy.parameters())
        worst["params"] = max([worst.get("params", 0.0)] + [_frac(t, w) for t, w in zip(got, mine["q_params"] + mine["p_params"])])
        assert set(tr.info) == {"loss_q", "loss_q_align", "loss_policy"}
        assert tr.info["loss_q"] == pytest.approx(ref["loss_q"], rel=1e-5, abs=1e-6)
    print(f"NOTSAC-CPU-ERR {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", C.NAMES + list(C.PIN_CASES))
def test_no_case_is_near_a_kink(name):
    """The float64 restatement puts neither update within 1e-3 of a kink: Huber's |target - q| = 1, the log-scale clamp's ends, a tie of the two largest noisy
    next-state logits, either norm = max_grad_norm.  This is what lets every comparison against float32 code keep every element of every case."""
    for ref in C.reference(name):
        assert ref["margin"] >= 1e-3, ref["margin"]


def test_the_cases_stand_on_both_sides_of_every_kink():
    huber = {"quadratic": 0, "linear": 0}
    for name in C.NAMES:
        for ref in C.reference(name):
            d = (ref["target_q"] - ref["q"]).abs()
            huber["quadratic"] += int((d < 1).sum())
            huber["linear"] += int((d > 1).sum())
    assert huber["quadratic"] > 50 and huber["linear"] > 50
    refs = C.reference("b17-mixed")
    assert all(r["norm_q"] > 0.01 and r["norm_policy"] > 0.01 for r in refs)  # both clips bite
    assert all(r["norm_q"] < 10.0 and r["norm_policy"] < 10.0 for r in C.reference("default-b16"))
    p = C.make_parameter("normal-forced")
    b = C.make_batches("normal-forced")[0]
    with torch.no_grad():
        ls = R.policy_forward(C.yardstick("normal-forced", p).policy, b["state"])[1]
    lo, hi = C.ls_range(p.config)
    assert bool((ls[:, 0] < lo).all()) and bool((ls[:, 2] > hi).all()) and bool(((ls[:, 1] > lo) & (ls[:, 1] < hi)).all())
    assert float(b["not_terminated"][0]) == 0.0 and float(b["not_terminated"][1]) == 1.0
    na = C.reference("cat-a5-deep")[0]["next_action"]
    assert bool((na.sum(1) == 1).all()) and len(set(na.argmax(1).tolist())) > 1  # one-hot rows, more than one action taken


def test_yardstick_on_hand_worked_numbers():
    """One row, one action element, networks whose outputs are their biases: loc 0.5, log-scale log 2; q = 0.25 whatever the action.  Noise (1, -1): the next
    action is tanh(0.5 + 2) and the policy's tanh(0.5 - 2).  r = 2, not terminated: target = 2 + 0.9 * 0.25, Huber's linear region."""
    import math

    cfg = C.make_config(1, 1, 1, (32,), (32,), 32)
    p = sac_not.Parameter(cfg)
    with torch.no_grad():
        for t in list(p.policy.parameters()) + list(p.qnet.parameters()):
            t.zero_()
        p.policy.policy_dist_block.loc_layers[0].bias.fill_(0.5)
        p.policy.policy_dist_block.log_scale_layers[0].bias.fill_(math.log(2.0))
        p.qnet.q_out_layer.bias.fill_(0.25)
    y = R.Yardstick(p, 1e-4, 0.9, 0.1, 10.0, True, C.ls_range(cfg))
    one = lambda v: torch.tensor([v], dtype=torch.float64)  # noqa: E731
    out = y.update(torch.zeros(1, 1), torch.zeros(1, 1), torch.zeros(1, 1), one(2.0), one(1.0), one(1.0), torch.tensor([[[1.0]], [[-1.0]]]))
    assert float(out["next_action"]) == pytest.approx(math.tanh(2.5)) and float(out["pi_action"]) == pytest.approx(math.tanh(-1.5))
    assert float(out["q"]) == 0.25 and float(out["target_q"]) == pytest.approx(2.0 + 0.9 * 0.25)
    assert out["loss_q"] == pytest.approx(abs(2.0 + 0.9 * 0.25 - 0.25) - 0.5) and out["loss_q_align"] == pytest.approx((1.0 - 0.25) ** 2)
    assert float(out["q_raw_grads"][-1]) == pytest.approx(-1.0 + 0.1 * -2.0 * (1.0 - 0.25))  # d / d q: Huber's -sign(d) and the alignment term
    assert out["norm_policy"] == 0.0  # the Q-network ignores the action: nothing reaches the policy
    assert out["loss_policy"] == pytest.approx(-float(out["q_params"][-1]))  # ... and the policy step sees the Q-network already stepped


# ---- the noise ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default-b16", "b17-mixed", "cat-a16-b17"])
def test_noise_none_draws_what_the_explicit_noise_of_the_same_seed_gives(name):
    b = C.make_batches(name)[0]
    B, n_out, head = C.spec(name)[0], C.spec(name)[3], C.spec(name)[2]
    outs = []
    for explicit in (False, True):
        p = C.make_parameter(name)
        tr = sac_not.Trainer(p.config, p, None)
        tr.update_backend = "torch"
        tr.on_setup()
        torch.manual_seed(123)
        noise = None
        if explicit:
            z, o = torch.zeros(B, n_out), torch.ones(B, n_out)
            noise = torch.stack([torch.normal(z, o), torch.normal(z, o)]) if head else torch.stack([torch.rand(B, n_out), torch.rand(B, n_out)])
        outs.append((tr.train_on_batch(*_args(b), noise=noise), list(p.policy.parameters()) + list(p.qnet.parameters())))
    assert all(torch.equal(outs[0][0][k], outs[1][0][k]) for k in outs[0][0])
    assert all(torch.equal(a, c) for a, c in zip(outs[0][1], outs[1][1]))


@pytest.mark.parametrize("shape", [(5, 1), (7, 2), (64, 1), (17, 8), (3, 3)])
def test_a_seeded_normal_sample_is_loc_plus_std_times_the_seeded_standard_draw(shape):
    """What lets a seeded CPU run of the "torch" backend reproduce the reference's draws: torch.normal(loc, std) then rsample's draw equal loc + std * e1 and e2."""
    g = torch.Generator().manual_seed(9)
    loc, std = torch.randn(shape, generator=g), torch.rand(shape, generator=g) + 0.1
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        sample = torch.normal(loc, std)
        e2 = torch.normal(torch.zeros(shape), torch.ones(shape))
        torch.manual_seed(seed)
        n1, n2 = torch.normal(torch.zeros(shape), torch.ones(shape)), torch.normal(torch.zeros(shape), torch.ones(shape))
        assert torch.equal(sample, loc + std * n1) and torch.equal(e2, n2)


# ---- Runner -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["Grid", "Pendulum-v1"])
def test_runner_trains_and_evaluates_on_cpu_parameters(env, monkeypatch):
    monkeypatch.setattr(sac_not.Trainer, "update_backend", "srlx")
    cfg = sac_not.Config(batch_size=16)
    cfg.memory.warmup_size = 32
    runner = srl.Runner(env, cfg)
    runner.set_device("cpu")
    tensors = lambda p: list(p.policy.parameters()) + list(p.qnet.parameters())  # noqa: E731
    start = [t.detach().clone() for t in tensors(runner.make_parameter())]
    runner.train(max_train_count=5)
    tr = runner.trainer
    assert tr.train_count == 5 and tr.update_path == "torch" and tr.why_not_srlx_update == "the parameters are CPU tensors"
    assert set(tr.info) == {"loss_q", "loss_q_align", "loss_policy"} and all(np.isfinite(v) for v in tr.info.values())
    assert not any(torch.equal(a, c) for a, c in zip(start, tensors(runner.parameter)))
    assert len(runner.memory.sample()[0]) == 6
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)


def test_rollout_then_train_only_on_the_plugin_path():
    cfg = sac_not.Config(batch_size=16)
    cfg.memory.warmup_size = 32
    runner = srl.Runner("Pendulum-v1", cfg)
    runner.set_device("cpu")
    runner.rollout(max_memory=64)
    assert runner.memory.length() >= 64 and len(runner.memory.sample()[0]) == 6  # [state, next_state, action, reward, not_done, total_reward]
    runner.train_only(max_train_count=3)
    assert runner.trainer.train_count == 3 and runner.trainer.update_path == "torch"


# ---- libsrlx's host validation ------------------------------------------------------------------------------------------------------------------------------------
def _widths(w):
    return ctypes.cast((ctypes.c_int * 4)(*(list(w) + [0, 0, 0, 0])[:4]), N.c_p)


OK = dict(D=3, head=1, n_out=1, policy=(512,), q=(512,), E=64, max_batch=64)
BAD = [dict(D=0), dict(D=257), dict(head=2), dict(head=-1), dict(n_out=0), dict(n_out=9), dict(head=0, n_out=1), dict(head=0, n_out=17), dict(policy=()),
       dict(policy=(64, 64, 64, 64)), dict(policy=(31,)), dict(policy=(48,)), dict(policy=(544,)), dict(q=()), dict(q=(64, 64, 64, 64)), dict(q=(48,)),
       dict(q=(544,)), dict(E=0), dict(E=16), dict(E=48), dict(E=544), dict(D=32, E=512), dict(D=256, E=288), dict(max_batch=0), dict(max_batch=257)]
EDGES = [dict(D=1), dict(D=256, E=256), dict(D=224, E=288), dict(head=0, n_out=2), dict(head=0, n_out=16), dict(n_out=8), dict(policy=(32,)),
         dict(policy=(512, 512, 512)), dict(q=(32,)), dict(q=(512, 32, 512)), dict(E=32), dict(D=1, E=480), dict(max_batch=1), dict(max_batch=256)]


def _shape_args(c):
    return (c["D"], c["head"], c["n_out"], len(c["policy"]), _widths(c["policy"]), len(c["q"]), _widths(c["q"]), c["E"], c["max_batch"])


def test_create_refuses_every_edge_of_the_envelope_without_a_device():
    """srlx_notsac_create validates before it touches a device; srlx_notsac_scratch_floats answers -1 for the same shapes and a positive count inside, and
    NotSacUpdate.envelope_reason gives a sentence exactly there -- D + E = 544 included."""
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    lib = N.lib()
    for change in BAD:
        c = dict(OK, **change)
        h = N.c_p()
        st = lib.srlx_notsac_create(ctypes.byref(h), *_shape_args(c), 0)
        assert st == N.ERR_INVALID and not h and b"notsac_create" in lib.srlx_last_error(), change
        assert lib.srlx_notsac_scratch_floats(*_shape_args(c)) == -1, change
        if c["max_batch"] < 1:  # (no batch has that size: `why_not` asks about a batch, `create` about a handle)
            continue
        reason = NotSacUpdate.envelope_reason(c["D"], c["head"], c["n_out"], c["policy"], c["q"], c["E"], c["max_batch"])
        assert ("above max_batch" in reason) if c["max_batch"] > 256 else ("outside the envelope" in reason), change
    assert 256 + 288 == 544 and dict(D=256, E=288) in BAD
    for change in [{}] + EDGES:
        c = dict(OK, **change)
        assert lib.srlx_notsac_scratch_floats(*_shape_args(c)) > 0, change
        assert NotSacUpdate.envelope_reason(c["D"], c["head"], c["n_out"], c["policy"], c["q"], c["E"], c["max_batch"]) == "", change


def test_null_arguments_are_refused_without_a_device():
    lib = N.lib()
    assert lib.srlx_notsac_create(None, *_shape_args(OK), 0) == N.ERR_INVALID
    assert lib.srlx_notsac_destroy(None) == 0
    assert lib.srlx_notsac_bind(None, 0, None) == N.ERR_INVALID and b"notsac_bind" in lib.srlx_last_error()
    assert lib.srlx_notsac_bind_grads(None, 0, None, None) == N.ERR_INVALID
    assert lib.srlx_notsac_bind_adam(None, 0, None, None, 0, 0.9, 0.999, 1e-8) == N.ERR_INVALID
    assert lib.srlx_notsac_set_rows_per_workgroup(None, 1) == N.ERR_INVALID and b"notsac_set_rows_per_workgroup" in lib.srlx_last_error()
    assert lib.srlx_notsac_steps(None) == -1 and b"notsac_steps" in lib.srlx_last_error()
    assert lib.srlx_notsac_forward(None, 1, None, 0.0, 1.0, None, None, None, None, None) == N.ERR_INVALID
    assert lib.srlx_notsac_update(None, 1, *([None] * 7), 1e-4, 0.9, 0.1, 10.0, 1, 0.0, 1.0, *([None] * 6)) == N.ERR_INVALID


def test_why_not_gives_a_sentence_for_every_refusal():
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate, shape_of

    p = C.make_parameter("b17-mixed")
    assert shape_of(p) == (4, 1, 2, (32, 64, 96), (96, 64, 32), 96)
    assert shape_of(C.make_parameter("cat-a16-b17")) == (3, 0, 16, (32, 64), (64,), 32)
    assert NotSacUpdate.why_not(p, 17, p.config) == "the parameters are CPU tensors" and not NotSacUpdate.serves(p)
    assert NotSacUpdate.config_reasons(p.config) == []
    cfg = C.make_config(4, 1, 2, (64,), (64,), 32, in_block_layers=(32,))
    assert any("input_block" in r for r in NotSacUpdate.config_reasons(cfg))
    assert "input_block" in shape_of(sac_not.Parameter(cfg))
    cfg = C.make_config(4, 1, 2, (64,), (64,), 32, target_policy_temperature=0.0)
    assert any("target_policy_temperature" in r for r in NotSacUpdate.config_reasons(cfg))
    cfg = C.make_config(4, 1, 2, (64,), (64,), 32)
    cfg.q_block.set((64,), activation="tanh")
    assert "q_block is not a chain of Linear (with bias) + ReLU" in shape_of(sac_not.Parameter(cfg))
    cfg = C.make_config(4, 1, 2, (64,), (64,), 32)
    cfg.policy_block.kwargs["foo"] = 1
    assert any("policy_block sets ['foo']" in r for r in NotSacUpdate.config_reasons(cfg))
    cfg = C.make_config(4, 1, 2, (64,), (64,), 32)
    cfg.lr_scheduler.schedule_type = "custom"
    assert any("lr schedule" in r for r in NotSacUpdate.config_reasons(cfg))


def test_a_request_for_srlx_on_cpu_parameters_is_served_by_torch_and_says_why():
    p = C.make_parameter("cat-default")
    tr = sac_not.Trainer(p.config, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    b = C.make_batches("cat-default")[0]
    tr.train_on_batch(*_args(b), noise=b["noise"])
    assert tr.update_path == "torch" and tr.why_not_srlx_update == "the parameters are CPU tensors"
