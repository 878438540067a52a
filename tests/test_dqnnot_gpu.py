"""NoTarget_DQN's update on libsrlx (srlx_dqnnot_update, csrc/srlx_dqnnot.hip) over the cases of tests/dqnnot_reference.py against its float64
yardstick at the standing bars (dqnnot_reference.over_the_bar): two consecutive updates on a fresh handle, no case and no element left out.  Every comparison
prints its worst fraction of each bar ("DQNNOT-ERR", shown with -s) before it asserts."""
import functools

import numpy as np
import pytest
import torch

import dqnnot_reference as R
import simple_distributed_rl_amd as srl
from simple_distributed_rl_amd.algorithms import dqn_not

pytestmark = pytest.mark.gpu


def _run(name):
    """Two updates on a fresh seeded GPU parameter of the case: (the update object, what each update left)."""
    from simple_distributed_rl_amd.device.dqnnot import DqnNotUpdate

    p = R.make_parameter(name, "cuda")
    u = DqnNotUpdate(p, max_batch=R.CASES[name][0])
    steps = []
    for b, _ in R.reference(name):
        out = u.update(*R.device_batch(b, "cuda"), R.DISCOUNT, R.ALIGN, R.LR)
        torch.cuda.synchronize()
        steps.append(dict(out=out, grads=[g.clone() for g in u.grads], params=[t.detach().clone() for t in u.params]))
    return u, steps


@functools.lru_cache(maxsize=None)
def _first(name):
    return _run(name)


@pytest.mark.parametrize("name", R.NAMES)
def test_update_matches_float64_yardstick(name):
    u, steps = _first(name)
    bad = {}
    for k, (st, (_, want)) in enumerate(zip(steps, R.reference(name))):
        bad.update({f"{k}:{key}": v for key, v in R.over_the_bar(f"srlx-{name}-{k}", st["out"], want, st["grads"], st["params"]).items()})
    assert u.steps() == 2
    assert not bad, f"{name}: over the bar (fraction of it): {bad}"


@pytest.mark.parametrize("name", R.NAMES)
def test_two_handles_on_equal_inputs_give_equal_bits(name):
    for sa, sb in zip(_first(name)[1], _run(name)[1]):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for key in ("grads", "params") for x, y in zip(sa[key], sb[key]))


@pytest.mark.parametrize("name", ["b33-u64", "b257"])
def test_trainer_runs_the_srlx_backend(name):
    b, want = R.reference(name)[0]
    p = R.make_parameter(name, "cuda")
    p.config.lr, p.config.discount, p.config.align_loss_coeff = R.LR, R.DISCOUNT, R.ALIGN
    tr = dqn_not.Trainer(p.config, p, None)
    tr.update_backend = "srlx"
    tr.on_setup()
    out = tr.train_on_batch(*R.device_batch(b, "cuda"))
    assert tr.update_path == "srlx" and tr.why_not_srlx_update == "" and tr.train_count == 1
    bad = R.over_the_bar(f"trainer-{name}", out, want, tr._srlx.grads, tr._srlx.params)
    assert tr.info["loss_q"] == pytest.approx(float(want["losses"][0]), rel=1e-5, abs=1e-6)
    assert tr.info["loss_align"] == pytest.approx(float(want["losses"][1]), rel=1e-5, abs=1e-6)
    assert not bad, bad


def test_runner_trains_cartpole_on_the_srlx_backend_and_evaluates(monkeypatch):
    monkeypatch.setattr(dqn_not.Trainer, "update_backend", "srlx")
    cfg = dqn_not.Config(batch_size=8, base_units=32)
    cfg.memory.warmup_size = 16
    runner = srl.Runner("CartPole-v1", cfg)
    runner.train(max_train_count=40)
    tr = runner.trainer
    assert tr.train_count == 40 and tr.update_path == "srlx" and all(np.isfinite(tr.info[k]) for k in ("loss_q", "loss_align"))
    assert all(bool(torch.isfinite(t).all()) for t in runner.parameter.q_online.parameters())
    rewards = runner.evaluate(max_episodes=2)
    assert len(rewards) == 2 and all(np.isfinite(r) for r in rewards)
