"""What a ppo.Config asks of the PPO device engine, the parts that need no GPU: the learning-rate schedules of libsrlx (`srlx_lr_factor`, host arithmetic of
csrc/srlx_lr_math.h -- the function k_ppo_adam evaluates on the device) against `LRSchedulerConfig.factor`, and the mapping of ppo.Config onto PPODeviceConfig
(`vector_runner.ppo_config_from`) with every reason `why_not_ppo_engine` gives.
Tolerance of the schedules: 1e-12 relative -- both sides are a handful of float64 operations, libm's pow / cos within an ulp or two; the staircase and the
piecewise schedule (one pow of an integer exponent, one division) must be EQUAL."""
import dataclasses

import pytest

import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo
from simple_distributed_rl_amd.device import vector_runner as vr
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig

LR = 2e-4
SCHEDULES = {
    "step-2-0.5": (lambda: LRSchedulerConfig().set_step(2, 0.5), range(13), True),
    "step-2000-0.01": (lambda: LRSchedulerConfig().set_step(2000, 0.01), (0, 1999, 2000, 3999, 4000), True),
    "exp-3-0.1": (lambda: LRSchedulerConfig().set_exp(3, 0.1), range(13), False),
    "cosine-4": (lambda: LRSchedulerConfig().set_cosine(4, 1e-5), range(13), False),
    "piecewise-2-4": (lambda: LRSchedulerConfig().set_piecewise([2, 4], [1e-3, 5e-4, 1e-4]), range(13), True),
    "constant": (lambda: LRSchedulerConfig(), range(13), True),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_lr_factor_against_the_scheduler_config(name):
    make, steps, exact = SCHEDULES[name]
    cfg = make()
    s = N.lr_schedule(cfg)
    for k in steps:
        got, want = N.lr_factor(s, k, LR), cfg.factor(k, LR)
        print("PPO-CFG lr_factor %s step %d: %.17g (python %.17g)" % (name, k, got, want))
        if exact:
            assert got == want, (name, k, got, want)
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (name, k, got, want)


def test_lr_factor_edges():
    """The staircase divides as integers (1999 // 2000 = 0); the cosine stays at its floor beyond decay_steps; at step == boundary the earlier piecewise value
    applies (step > b counts); bad schedules are refused before any arithmetic."""
    f = lambda cfg, k: N.lr_factor(N.lr_schedule(cfg), k, LR)  # noqa: E731
    stair = LRSchedulerConfig().set_step(2000, 0.01)
    assert (f(stair, 1999), f(stair, 2000), f(stair, 4000)) == (1.0, 0.01, 0.01 ** 2)
    cos = LRSchedulerConfig().set_cosine(4, 1e-5)
    assert f(cos, 4) == f(cos, 5) == f(cos, 12) and abs(f(cos, 4) - 1e-5 / LR) <= 1e-12 * (1e-5 / LR) and f(cos, 0) == 1.0
    pw = LRSchedulerConfig().set_piecewise([2, 4], [1e-3, 5e-4, 1e-4])
    assert (f(pw, 2), f(pw, 3), f(pw, 4), f(pw, 5)) == (1e-3 / LR, 5e-4 / LR, 5e-4 / LR, 1e-4 / LR)
    with pytest.raises(ValueError, match="at most 8"):
        N.lr_schedule(LRSchedulerConfig().set_piecewise(list(range(9)), [1.0] * 10))
    with pytest.raises(ValueError):
        N.lr_schedule(LRSchedulerConfig().set_piecewise([1, 2], [1.0, 0.5]))
    with pytest.raises(ValueError):
        N.lr_schedule(LRSchedulerConfig(schedule_type="linear"))
    bad = N.lr_schedule(LRSchedulerConfig().set_step(2, 0.5))
    bad.decay_steps = 0
    with pytest.raises(N.SrlxError):
        N.lr_factor(bad, 1, LR)
    bad.decay_steps, bad.kind = 2, 9
    with pytest.raises(N.SrlxError):
        N.lr_factor(bad, 1, LR)
    with pytest.raises(N.SrlxError):
        N.lr_factor(N.lr_schedule(stair), 1, 0.0)


def _pair(env_name, cfg=None):
    r = srl.Runner(env_name, cfg if cfg is not None else ppo.Config())
    r.setup_rl_config()
    return r.env, r.rl_config


def test_default_config_maps_onto_cartpole():
    env, c = _pair("CartPole-v1")
    assert vr.why_not_ppo_engine(env, c) == ""
    d = vr.ppo_config_from(c, env, 256, 7)
    assert (d.n_envs, d.seed, d.horizon, d.epochs, d.minibatches) == (256, 7, 32, 4, 4)
    assert (d.obs_dim, d.n_actions, d.episode_len) == (4, 2, 500)
    assert (d.hidden_sizes, d.value_sizes, d.policy_sizes) == ((64, 64), (64,), (64,))
    assert (d.discount, d.gae_discount, d.baseline_type, d.surrogate_type) == (0.9, 0.9, "advantage", "clip")
    assert (d.policy_clip_range, d.enable_value_clip, d.value_clip_range, d.value_loss_weight, d.entropy_weight) == (0.2, True, 0.2, 1.0, 0.01)
    assert (d.lr, d.global_gradient_clip_norm, d.stable_gradients_scale_range) == (0.0002, 0.5, (1e-10, 10.0))
    s = d.lr_scheduler
    assert (s.schedule_type, s.decay_steps, s.decay_rate) == ("step", 2000, 0.01) and s is not c.lr_scheduler
    assert d.reward_clip is None and d.state_clip is None and (d.action_scale, d.action_offset) == (1.0, 0.0)
    assert vr.ppo_config_from(c, env, 64, 1, horizon=8, epochs=1, minibatches=2).horizon == 8


def test_default_config_maps_onto_pendulum():
    cfg = ppo.Config(reward_clip=(-1, 0), state_clip=(-0.5, 0.5), baseline_type="normal", lr=1e-3)
    cfg.lr_scheduler.set_cosine(100, 1e-5)
    env, c = _pair("Pendulum-v1", cfg)
    assert vr.why_not_ppo_engine(*_pair("Pendulum-v1")) == "" and vr.why_not_ppo_engine(env, c) == ""
    d = vr.ppo_config_from(c, env, 128, 3)
    assert (d.obs_dim, d.n_actions, d.action_dim, d.episode_len) == (3, 0, 1, 200)
    assert (d.action_scale, d.action_offset) == (2.0, 0.0)
    assert (d.reward_clip, d.state_clip, d.baseline_type, d.lr) == ((-1.0, 0.0), (-0.5, 0.5), "normal", 1e-3)
    assert (d.lr_scheduler.schedule_type, d.lr_scheduler.decay_steps, d.lr_scheduler.min_lr) == ("cosine", 100, 1e-5)


def _with(**kw):
    return lambda: ppo.Config(**kw)


def _change(fn):
    def make():
        c = ppo.Config()
        fn(c)
        return c
    return make


def _image_processor_config():
    from simple_distributed_rl_amd.rl.processors.image_processor import ImageProcessor

    return ppo.Config(processors=[ImageProcessor()])


# (what the reason must say, the config that draws it); the environment's own reason is the Grid case
REASONS = {
    "environment": ("built-in environments", ppo.Config),
    "processors": ("observation processors", _image_processor_config),
    "window_length": ("window_length 1", _with(window_length=4)),
    "input_block": ("trainable input block", _change(lambda c: c.input_block.value.set((32,)))),
    "hidden_block-activation": ("MLPs of ReLU layers", _change(lambda c: c.hidden_block.set((64, 64), activation="tanh"))),
    "policy_block-bias": ("MLPs of ReLU layers", _change(lambda c: c.policy_block.set((64,), use_bias=False))),
    "value_block-name": ("MLPs of ReLU layers", _change(lambda c: setattr(c.value_block, "name", "DuelingNetwork"))),
    "mc": ('experience_collection_method "MC"', _with(experience_collection_method="MC")),
    "state_normalized": ("enable_state_normalized", _with(enable_state_normalized=True)),
    "stable_gradients": ("enable_stable_gradients=False", _with(enable_stable_gradients=False)),
    "baseline": ("unknown baseline_type 'median'", _with(baseline_type="median")),
    "surrogate": ("unknown surrogate_type 'kl'", _with(surrogate_type="kl")),
    "piecewise": ("at most 8", _change(lambda c: c.lr_scheduler.set_piecewise(list(range(1, 10)), [1e-3] * 10))),
    "frameskip": ("frameskip 0", _with(frameskip=2)),
    "sanitize": ("enable_sanitize", _with(enable_sanitize=False)),
    "reward_scale": ("reward_scale", _with(reward_scale=0.1)),
    "dtype": ("float32", _with(dtype="float64")),
}


@pytest.mark.parametrize("name", list(REASONS))
def test_every_reason_is_given(name):
    """On Grid (an environment the engine does not step: that reason is always there, and every other one beside it), and -- the environment's own aside -- on
    CartPole-v1, where the reason stands alone.  `ppo_config_from` refuses what `why_not_ppo_engine` refuses."""
    phrase, make = REASONS[name]
    try:
        env, c = _pair("Grid", make())
    except Exception as e:  # (a processor that does not take Grid's observation space: the plugin path refuses the pair itself)
        assert name == "processors", e
    else:
        why = vr.why_not_ppo_engine(env, c)
        print("PPO-CFG why_not (Grid) %s: %s" % (name, why))
        assert "built-in environments" in why and phrase in why
        with pytest.raises(ValueError, match="cannot run"):
            vr.ppo_config_from(c, env, 64, 0)
    if name == "environment":
        return
    if name == "processors":  # (CartPole's vector is no image either: the user's processor list alone draws the reason, before any set-up)
        c = make()
        assert phrase in vr.why_not_ppo_engine(_pair("CartPole-v1")[0], c)
        return
    env, c = _pair("CartPole-v1", make())
    why = vr.why_not_ppo_engine(env, c)
    assert phrase in why and "; " not in why, why  # (one reason: no separator)


def test_aliases_and_other_algorithms():
    env, c = _pair("CartPole-v1", ppo.Config(baseline_type="v", surrogate_type=""))
    assert vr.why_not_ppo_engine(env, c) == "" and vr.ppo_config_from(c, env, 64, 0).baseline_type == "v"
    from simple_distributed_rl_amd.algorithms import dqn

    r = srl.Runner("CartPole-v1", dqn.Config())
    r.setup_rl_config()
    assert "not a ppo.Config" in vr.why_not_ppo_engine(r.env, r.rl_config)
    assert vr.engine_kind(c) is None  # Runner.train() keeps PPO on the plugin path


def test_every_config_field_is_accounted_for():
    """Each field of ppo.Config (RLConfig's included) stands in exactly one of the three tuples of vector_runner: mapped, replaced by the engine's operating point,
    or refused with a reason -- a field added to the plugin later cannot be dropped silently.  Every mapped field changes the mapped configuration."""
    names = [f.name for f in dataclasses.fields(ppo.Config)]
    groups = (vr.PPO_MAPPED_FIELDS, vr.PPO_OPERATING_POINT_FIELDS, vr.PPO_REFUSED_FIELDS)
    for n in names:
        assert sum(n in g for g in groups) == 1, n
    assert sorted(n for g in groups for n in g) == sorted(names)
    assert len(set(vr.PPO_MAPPED_FIELDS)) == len(vr.PPO_MAPPED_FIELDS)
    other = dict(discount=0.95, gae_discount=0.8, baseline_type="ave", surrogate_type="", policy_clip_range=0.3, enable_value_clip=False, value_clip_range=0.1, lr=1e-3,
                 value_loss_weight=0.5, entropy_weight=0.0, global_gradient_clip_norm=0.0, state_clip=(-1.0, 1.0), reward_clip=(0.0, 0.5),
                 stable_gradients_scale_range=(1e-5, 5.0), lr_scheduler=LRSchedulerConfig().set_exp(10, 0.5))
    blocks = dict(hidden_block=(32,), value_block=(16, 16), policy_block=())
    assert sorted(list(other) + list(blocks)) == sorted(vr.PPO_MAPPED_FIELDS)
    env, base_c = _pair("CartPole-v1")
    base = vr.ppo_config_from(base_c, env, 64, 0)
    for n in vr.PPO_MAPPED_FIELDS:
        c = ppo.Config(**{n: other[n]}) if n in other else ppo.Config()
        if n in blocks:
            getattr(c, n).set(blocks[n])
        env, c = _pair("CartPole-v1", c)
        assert vr.ppo_config_from(c, env, 64, 0) != base, n
    for n, v in dict(batch_size=7, train_num=3, train_every_epoch=True).items():  # the plugin's schedule: no trace in the engine's configuration
        env, c = _pair("CartPole-v1", ppo.Config(**{n: v}))
        assert vr.ppo_config_from(c, env, 64, 0) == base, n


def test_engine_config_defaults_are_the_old_engine():
    from simple_distributed_rl_amd.device.ppo import BASELINES, PPODeviceConfig

    d = PPODeviceConfig()
    assert d.lr_scheduler.schedule_type == "" and d.reward_clip is None and d.state_clip is None and (d.action_scale, d.action_offset) == (1.0, 0.0)
    assert N.lr_schedule(d.lr_scheduler).kind == N.LR_CONSTANT
    assert BASELINES["v"] == "advantage" and BASELINES[""] == BASELINES["none"] == "none" and set(N.PPO_BASELINE_MODES) == {"ave", "std", "normal"}
