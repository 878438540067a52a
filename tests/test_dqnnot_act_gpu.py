"""NoTarget_DQN's acting kernel (srlx_dqnnot_act, csrc/srlx_dqnnot.hip: k_dqnnot_act) against the network's own forward in plain torch float64 at
the standing bars, rtol 1e-5 / atol 1e-6, no element left out; row independence bit for bit; and the plugin's surface (`dqn_not.Parameter.pred_q`).  The seeds
were picked on the CPU so that every row's float64 top-two gap exceeds 1e-4: the action test asserts that first and skips no row."""
import copy
import functools

import numpy as np
import pytest
import torch

import dqnnot_reference as R
from simple_distributed_rl_amd.algorithms import dqn_not

pytestmark = pytest.mark.gpu

# (n, D, U, A): the smallest of ...
CASES = [
    (1, 1, 32, 2),       # one row, everything minimal
    (16, 3, 32, 3),      # a full tile, unaligned D
    (17, 4, 64, 2),      # a second workgroup with one live row
    (33, 17, 96, 5),     # U no multiple of 64, odd D, three workgroups
    (5, 256, 512, 32),   # the LDS corner, 33 head rows
    (40, 4, 512, 2),     # dqn_not.Config() on CartPole
]
SEED = 7200


def _float64(parameter, x):
    """The network's forward in float64 on the CPU: (q [n][A], v [n][1])."""
    with torch.no_grad():
        return copy.deepcopy(parameter.q_online).cpu().double()(x.cpu().double())


@functools.lru_cache(maxsize=None)
def _case(n, D, U, A):
    """A seeded GPU Parameter, its states and the float64 answer.  Computed once; leave it unchanged."""
    torch.manual_seed(SEED + CASES.index((n, D, U, A)))
    p = dqn_not.Parameter(R.make_config(D, U, A, "cuda"))
    x = (0.5 * torch.randn(n, D)).cuda()
    return p, x, _float64(p, x)


def _assert_close(got, want):
    got = got.double().cpu()
    assert got.shape == want.shape and bool((got - want).abs().le(1e-6 + 1e-5 * want.abs()).all()), float(((got - want).abs() / (1e-6 + 1e-5 * want.abs())).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-d%d-u%d-a%d" % c)
def test_forward_and_action_match_float64(case):
    from simple_distributed_rl_amd.device.dqnnot import DqnNotAct

    p, x, (q64, v64) = _case(*case)
    top = q64.sort(dim=1, descending=True).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
    q, v, actions = DqnNotAct(p).act(x)
    _assert_close(q, q64)
    _assert_close(v, v64)
    assert actions.dtype == torch.int32 and np.array_equal(actions.cpu().numpy(), np.argmax(q.cpu().numpy(), axis=1))
    assert torch.equal(actions.cpu().long(), q64.argmax(dim=1))


def test_a_row_does_not_know_its_place_and_equal_inputs_give_equal_bits():
    from simple_distributed_rl_amd.device.dqnnot import DqnNotAct

    p, x, _ = _case(33, 17, 96, 5)
    act = DqnNotAct(p)
    whole = [t.clone() for t in act.act(x)]
    for r in (0, 15, 16, 32):
        assert all(torch.equal(one[0], w[r]) for one, w in zip(act.act(x[r:r + 1].clone()), whole)), r
    assert all(torch.equal(a, b) for a, b in zip(DqnNotAct(p).act(x.clone()), whole))


def test_pred_q_runs_the_kernel_and_sees_updates_by_address():
    from simple_distributed_rl_amd.device.dqnnot import DqnNotUpdate

    name = "b33-u64"
    batch = R.reference(name)[0][0]
    p = R.make_parameter(name, "cuda")
    p.act_backend = "srlx"
    states = batch["states"].float().numpy()
    q0, v0 = p.pred_q(states)
    assert p.act_path == "srlx" and p.why_not_srlx_act == ""
    assert isinstance(q0, np.ndarray) and q0.shape == (66, 2) and q0.dtype == np.float32 and isinstance(v0, np.ndarray) and v0.shape == (66, 1)
    DqnNotUpdate(p, max_batch=33).update(*R.device_batch(batch, "cuda"), R.DISCOUNT, R.ALIGN, 1e-2)
    q1, v1 = p.pred_q(states)
    q64, v64 = _float64(p, torch.from_numpy(states))  # (the NEW network's)
    _assert_close(torch.from_numpy(q1), q64)
    _assert_close(torch.from_numpy(v1), v64)
    assert float(np.abs(q1 - q0).max()) > 1e-2  # (the step moved the values far past the bars)
    p.to_device("cpu")
    p.pred_q(states)
    assert p.act_path == "torch" and p.why_not_srlx_act == "the parameters are CPU tensors"
    p.to_device("cuda")
    q2, _ = p.pred_q(states)
    assert p.act_path == "srlx" and np.array_equal(q2, q1)

    narrow = dqn_not.Parameter(R.make_config(4, 48, 2, "cuda"))
    narrow.act_backend = "srlx"
    q, v = narrow.pred_q(states)
    assert q.shape == (66, 2) and v.shape == (66, 1) and narrow.act_path == "torch"
    assert narrow.why_not_srlx_act == "base_units 48 outside 32..512 in multiples of 32"
