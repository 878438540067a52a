"""What device/lane_engine.py owns for the four plugin-trainer engines, on the GPU: the fresh state, the counters, the phase timer's names, `info()`'s key
set, a second `setup_trainer`, and the flat pair's refusal of an update that would run in torch.  Every engine is built by its own test file's builder at that
file's smallest shapes: SAC-Discrete and V-PPO on the device CartPole (E 16, B 8, blocks (32,), warm-up 32), R2D2 on the corridor and Agent57 on TinyImg (E 4).
The lanes' actions, rings and updates are pinned bit for bit in those four files."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _sacd():
    import test_sacd_engine_gpu as T

    return T._engine(seed=3)[1]


def _vppo():
    import test_vppo_engine_gpu as T

    return T._engine(seed=3)[1]


def _r2d2():
    import test_r2d2_engine_gpu as T

    return T._engine(seed=5)


def _agent57():
    import test_agent57_lane_engine_gpu as T

    return T._engine("TinyImg", True, seed=5)


BUILD = {"sacd": _sacd, "vppo": _vppo, "r2d2": _r2d2, "agent57": _agent57}
FLAT_PHASES, SEQUENCE_PHASES = {"actor", "learner"}, {"actor", "push", "adds", "train"}
PHASES = {"sacd": FLAT_PHASES, "vppo": FLAT_PHASES, "r2d2": SEQUENCE_PHASES, "agent57": SEQUENCE_PHASES}
# info()'s keys past the first update, as the engines gave them before the scaffold was shared (recorded from a run of that commit, not read off the code)
INFO_KEYS = {
    "sacd": {"alpha", "alpha_loss", "env_steps", "memory", "policy_loss", "q1_loss", "q2_loss", "train_count"},
    "vppo": {"env_steps", "loss_policy", "loss_v_align", "loss_value", "memory", "train_count"},
    "r2d2": {"loss", "memory", "sync", "train_count"},
    "agent57": {"emb_loss", "ext_loss", "int_loss", "lifelong_loss", "loss", "memory", "sync", "train_count"},
}


@pytest.mark.parametrize("name", list(BUILD))
def test_the_scaffolds_contract(name):
    from simple_distributed_rl_amd.base.context import RunContext

    eng = BUILD[name]()
    E = eng.E
    assert eng.overlap is False and eng.lock_steps == 0 and eng.total_env_steps == 0 and eng.replay.is_warmup_needed()
    assert eng.phase_times is None and eng.ledger is None and eng.record is None
    returned, inner = [], eng.learner_step

    def counted():
        returned.append(inner())
        return returned[-1]

    eng.learner_step = counted  # (`step` calls it through the instance)
    k, count0 = 0, eng.train_count
    while eng.replay.is_warmup_needed():
        eng.step()
        k += 1
    warm = len(returned)
    for _ in range(5):
        eng.step()
        k += 1
    assert eng.lock_steps == k and eng.total_env_steps == k * E
    assert all(r is True or r is False for r in returned) and all(returned[warm:]) and eng.train_count - count0 == sum(returned) >= 5
    assert eng.phase_times is None  # (nothing was timed)
    eng.phase_times = {}
    eng.step()
    assert set(eng.phase_times) == PHASES[name] and all(v > 0 for v in eng.phase_times.values())
    eng.phase_times = None
    eng.step()
    assert eng.phase_times is None and eng.lock_steps == k + 2
    assert set(eng.info()) == INFO_KEYS[name]
    eng.join_learner()
    eng.setup_trainer(RunContext())  # a run opens again: fresh optimisers, and the next lock-step trains
    count1, n = eng.train_count, len(returned)
    eng.step()
    assert returned[n:] == [True] and eng.train_count == count1 + 1


@pytest.mark.parametrize("name", ["sacd", "vppo"])
def test_the_flat_pair_refuses_an_update_that_would_run_in_torch_in_the_trainers_words(name):
    """float64 networks pass `why_not_*_engine` (it reads the config) and stay off libsrlx: the engine says so in `why_not_srlx_update`'s words."""
    from simple_distributed_rl_amd.base.context import RunContext

    if name == "sacd":
        import test_sacd_engine_gpu as T
        from simple_distributed_rl_amd.device.sacd import SacdUpdate as Update
        from simple_distributed_rl_amd.device.sacd_engine import SacdEngine as Engine
    else:
        import test_vppo_engine_gpu as T
        from simple_distributed_rl_amd.device.vppo import VppoUpdate as Update
        from simple_distributed_rl_amd.device.vppo_engine import VppoEngine as Engine
    runner = T._runner(0)
    p = runner.make_parameter()
    (p.policy if name == "sacd" else p.net).double()
    with pytest.raises(ValueError) as e:
        Engine(runner.rl_config, T.E, parameter=p)
    why = Update.why_not(p, T.B, runner.rl_config)
    assert why == "a parameter is not a dense float32 tensor"
    assert str(e.value) == f"{Engine.__name__}: the update does not run on libsrlx: {why}"
    trainer = runner.rl_config.make_trainer(p, None)
    trainer.setup(RunContext())
    with pytest.raises(ValueError):
        trainer.require_srlx_update(T.B, "a caller")
    assert trainer.why_not_srlx_update == why and str(e.value).endswith(trainer.why_not_srlx_update)
