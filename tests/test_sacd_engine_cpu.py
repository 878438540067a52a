"""The SAC-Discrete device engine without a GPU: the numpy mirror of srlx_sacd_act / srlx_sacd_ring_batch (tests/sacd_engine_reference.py) held to
hand-worked literals, every sentence of `why_not_sacd_engine` on a config that trips exactly that reason, and the two entry points' declaration and export."""
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_engine_reference as M  # noqa: E402

from simple_distributed_rl_amd.algorithms import sac  # noqa: E402
from simple_distributed_rl_amd.base.define import SpaceTypes  # noqa: E402
from simple_distributed_rl_amd.base.spaces.box import BoxSpace  # noqa: E402
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace  # noqa: E402
from simple_distributed_rl_amd.device.vector_runner import why_not_sacd_engine  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the mirror -----------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_random_phase_literals_two_actions():
    U = np.array([[0.49, 0.9], [0.5, 0.1], [0.0, 0.99], [0.999, 0.0]])
    assert M.random_actions(U, 2).tolist() == [0, 1, 0, 1]  # floor(0.98), floor(1.0), floor(0), floor(1.998): the row's first uniform alone


def test_mirror_random_phase_boundary_stays_below_the_action_count():
    top = 1.0 - 2.0 ** -53  # the largest keyed uniform
    assert top * 3 == 2.9999999999999996 and M.random_actions(np.array([[top, 0.0, 0.0]]), 3).tolist() == [2]
    assert top * 16 < 16 and M.random_actions(np.array([[top] + [0.0] * 15]), 16).tolist() == [15]
    assert M.random_actions(np.array([[1.0, 0.0]]), 2).tolist() == [1]  # (a value the generator never gives: the min still holds it inside)


def test_mirror_sampling_phase_literals_two_actions():
    U = np.array([[0.5, 0.25], [0.25, 0.9]])
    assert M.rescaled(U).tolist() == [[0.5000005, 0.25000075], [0.25000075, 0.9000001]]
    z = np.array([[0.0, 0.0], [0.5, -0.25]], np.float32)
    s = M.scores(z, U)
    # -log(-log(0.5000005)) = 0.36651436..., -log(-log(0.25000075)) = -0.32663209..., 0.5 + that, -0.25 - log(-log(0.9000001)) = -0.25 + 2.25036838...
    want = [[0.3665143632770244, -0.3266320959366241], [0.17336790406337588, 2.000368381893118]]
    np.testing.assert_allclose(s, want, rtol=0, atol=2e-15)
    assert s[0, 0] == -math.log(-math.log(0.5000005))
    assert M.first_argmax(s).tolist() == [0, 1]
    np.testing.assert_allclose(M.top_two_gap(s), [0.6931464592136485, 1.8270004778297421], rtol=0, atol=4e-15)


def test_mirror_tie_takes_the_first_action():
    U = np.full((2, 3), 0.3)
    z = np.array([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0]], np.float32)
    s = M.scores(z, U)
    assert s[0, 0] == s[0, 1] == s[0, 2] and s[1, 1] == s[1, 2] > s[1, 0]
    assert M.first_argmax(s).tolist() == [0, 1]
    assert M.top_two_gap(s).tolist() == [0.0, 0.0]


def test_mirror_uniforms_are_the_keyed_generator_and_the_phase_follows_the_counter():
    U = M.uniforms(7, 3, 2, 2)
    np.testing.assert_allclose(U.reshape(-1), [0.04136613, 0.7773777, 0.86880186, 0.2478679], rtol=0, atol=5e-9)  # oracle/hot_path_oracle.py at (7, 3)
    z = np.zeros((2, 2), np.float32)
    a_random, s = M.act(z, 7, 3, 4, 2)
    a_sample, s2 = M.act(z, 7, 3, 3, 2)
    assert a_random.tolist() == [0, 1]  # floor(0.0827), floor(1.7376)
    assert a_sample.tolist() == [1, 0] and np.array_equal(s, s2)  # equal logits: the larger uniform wins each row


def test_mirror_ring_batch_is_plain_indexing():
    ring = np.arange(40, dtype=np.float32)
    s, n, onehot, done = M.ring_batch(ring, [[8, 12], [37, 0]], [[2], [0]], [[0.0], [1.0]], 3, 3)
    assert s.tolist() == [[8, 9, 10], [37, 38, 39]] and n.tolist() == [[12, 13, 14], [0, 1, 2]]
    assert onehot.tolist() == [[0, 0, 1], [1, 0, 0]] and done.tolist() == [0, 1] and done.dtype == np.uint8 and onehot.dtype == np.float32


# ---- why_not_sacd_engine ----------------------------------------------------------------------------------------------------------------------------------------
def _env(A=2, shape=(4,), players=1, action_space=None):
    return SimpleNamespace(player_num=players, action_space=DiscreteSpace(A) if action_space is None else action_space,
                           observation_space=BoxSpace(shape, -np.inf, np.inf, np.float32, SpaceTypes.CONTINUOUS))


def _cfg(**kw):
    c = sac.Config(**kw)
    c._rl_act_space = DiscreteSpace(2)
    return c


def _one(reason):
    assert reason and "; " not in reason, reason
    return reason


def test_why_not_is_empty_for_the_default_config_on_cartpole():
    import simple_distributed_rl_amd as srl

    runner = srl.Runner("CartPole-v1", sac.Config())
    runner.set_device("cpu")
    runner.setup_rl_config()
    assert why_not_sacd_engine(runner.env, runner.rl_config) == ""
    assert why_not_sacd_engine(runner.env, runner.rl_config, n_envs=16) == ""
    assert why_not_sacd_engine(_env(), _cfg(), n_envs=4096) == ""


def test_why_not_names_each_reason_on_its_own():
    from simple_distributed_rl_amd.algorithms import dqn
    from simple_distributed_rl_amd.rl.memories.priority_replay_buffer import PriorityReplayBufferConfig

    assert why_not_sacd_engine(_env(), dqn.Config()) == "'DQN' is not a SAC_Discrete config"
    assert _one(why_not_sacd_engine(_env(players=2), _cfg())) == "multi-player environment"
    box = BoxSpace((1,), -1.0, 1.0, np.float32, SpaceTypes.CONTINUOUS)
    assert _one(why_not_sacd_engine(_env(action_space=box), _cfg())) == "the engine serves discrete action spaces"
    for A in (1, 17):
        assert re.fullmatch(rf"{A} actions: outside the envelope \(.*A 2\.\.16.*\)", _one(why_not_sacd_engine(_env(A=A), _cfg())))
    assert "flat BoxSpace((D,)) observations" in _one(why_not_sacd_engine(_env(shape=(4, 4)), _cfg()))
    assert re.fullmatch(r"257 observation elements: outside the envelope \(D 1\.\.256.*\)", _one(why_not_sacd_engine(_env(shape=(257,)), _cfg())))
    c = _cfg()
    c._obs_processors = [(object(), None, BoxSpace((4,), -np.inf, np.inf, np.float32, SpaceTypes.CONTINUOUS))]
    assert _one(why_not_sacd_engine(_env(), c)) == "observation processors are served by the plugin path"
    assert _one(why_not_sacd_engine(_env(), _cfg(window_length=2))) == "the networks read one observation (window_length 1)"
    c = _cfg()
    c.input_block.value.set((32,))
    assert _one(why_not_sacd_engine(_env(), c)).startswith("an input_block with layers of its own")
    for name in ("policy_block", "q_block"):
        for sizes in ((), (48,), (544,), (16,), (32, 32, 32, 32)):
            c = _cfg()
            getattr(c, name).set(sizes)
            assert re.fullmatch(rf"{name} \(.*\): outside the envelope \(.*1\.\.3 layers of 32\.\.512 units in multiples of 32\)", _one(why_not_sacd_engine(_env(), c)))
        c = _cfg()
        getattr(c, name).set((64,), activation="tanh")
        assert _one(why_not_sacd_engine(_env(), c)) == f"{name} is not an MLP of ReLU layers (Linear layers with biases)"
    assert _one(why_not_sacd_engine(_env(), _cfg(batch_size=257))) == "batch size 257 above max_batch 256"
    assert why_not_sacd_engine(_env(), _cfg(batch_size=256)) == ""
    c = _cfg()
    c.memory = PriorityReplayBufferConfig()
    assert "draws uniformly from the ReplayBuffer memory" in _one(why_not_sacd_engine(_env(), c))
    for n in (0, 4097, "AUTO"):
        assert _one(why_not_sacd_engine(_env(), _cfg(), n_envs=n)) == f"{n!r} lanes are outside the engine's 1..4096"


def test_why_not_joins_every_reason():
    c = _cfg(batch_size=300, window_length=2)
    c.policy_block.set((48,))
    reasons = why_not_sacd_engine(_env(A=17, players=2), c, n_envs=0).split("; ")
    assert len(reasons) == 6 and reasons[0] == "multi-player environment" and reasons[-1].startswith("0 lanes")


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_exported():
    from simple_distributed_rl_amd import _native as N

    header = open(os.path.join(ROOT, "include", "srlx.h")).read()
    lib = N.lib()
    for name in ("srlx_sacd_act", "srlx_sacd_ring_batch"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in N.SIGNATURES and hasattr(lib, name)


def test_entry_points_refuse_before_any_device_call():
    """The envelope is host arithmetic: without a device srlx_sacd_ring_batch still names what is outside, and srlx_sacd_act refuses a NULL handle."""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    one = N.c_p(16)  # (never dereferenced: every call below is refused first)
    assert lib.srlx_sacd_act(None, 1, one, None, 0, one, 0, one, None, None, None) == N.ERR_INVALID and b"sacd_act" in lib.srlx_last_error()
    for B, D, A in ((0, 4, 2), (257, 4, 2), (8, 0, 2), (8, 257, 2), (8, 4, 1), (8, 4, 17)):
        assert lib.srlx_sacd_ring_batch(B, D, A, *([one] * 9), None) == N.ERR_INVALID and b"sacd_ring_batch" in lib.srlx_last_error(), (B, D, A)
    for k in range(9):
        args = [one] * 9
        args[k] = None
        assert lib.srlx_sacd_ring_batch(8, 4, 2, *args, None) == N.ERR_INVALID and b"sacd_ring_batch: NULL" in lib.srlx_last_error(), k
