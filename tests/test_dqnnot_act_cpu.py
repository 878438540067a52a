"""NoTarget_DQN's acting path without a GPU: srlx_dqnnot_act's refusals that need no device, and `dqn_not.Parameter.pred_q` on CPU parameters."""
import os
import sys

import numpy as np
import pytest

from simple_distributed_rl_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqnnot_reference as R  # noqa: E402


@pytest.mark.parametrize("n, message", [(1, b"dqnnot_act: NULL handle"), (0, b"dqnnot_act: n_rows 0 (1..65536)"), (65537, b"dqnnot_act: n_rows 65537 (1..65536)")])
def test_act_refuses_before_any_device_call(n, message):
    lib = N.lib()
    assert lib.srlx_dqnnot_act(None, n, None, None, None, None, None) == N.ERR_INVALID and message in lib.srlx_last_error()


def test_pred_q_on_cpu_parameters_runs_torch_and_says_why():
    p = R.make_parameter("b5-unaligned")
    assert p.act_backend in ("srlx", "torch")
    states = np.ones((4, 3), np.float32)
    p.act_backend = "torch"
    want = p.pred_q(states)
    assert p.act_path == "torch" and p.why_not_srlx_act == ""
    p.act_backend = "srlx"
    q, v = p.pred_q(states)
    assert p.act_path == "torch" and p.why_not_srlx_act == "the parameters are CPU tensors"
    assert q.shape == (4, 3) and v.shape == (4, 1) and np.array_equal(q, want[0]) and np.array_equal(v, want[1])
    from simple_distributed_rl_amd.device.dqnnot import DqnNotAct

    assert DqnNotAct.rows_reason(65536) == "" and DqnNotAct.rows_reason(65537) == "65537 rows above 65536 in one call"
    p.act_backend = "hip"
    with pytest.raises(ValueError, match="act_backend 'hip'"):
        p.pred_q(states)
