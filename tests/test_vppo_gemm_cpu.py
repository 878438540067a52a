"""`update_backend = "srlx_gemm"` without a GPU: ppo_v.Trainer serves it as it serves "srlx", in torch with the reason; a trainer whose device update
has no gemm path refuses the name."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_cases as C  # noqa: E402
from simple_distributed_rl_amd.algorithms import ppo_v, sac  # noqa: E402


def test_gemm_request_on_cpu_parameters_runs_torch_and_says_why():
    name = "default-b15"
    p = C.make_parameter(name)
    b = C.make_batches(name)[0]
    reasons = {}
    for backend in ("srlx_gemm", "srlx"):
        tr = ppo_v.Trainer(p.config, C.make_parameter(name), None)
        tr.update_backend = backend
        tr.on_setup()
        tr.train_on_batch(b["state"].float(), b["n_state"].float(), C.onehot(name, b["action"]).float(), b["old_logpi"].float(), b["reward"].float()[:, None],
                          b["not_terminated"].float()[:, None], b["total_reward"].float()[:, None])
        assert tr.update_path == "torch" and tr.why_not_srlx_update
        reasons[backend] = tr.why_not_srlx_update
    assert reasons["srlx_gemm"] == reasons["srlx"]


def test_a_trainer_without_a_gemm_path_refuses_the_name():
    tr = sac.Trainer.__new__(sac.Trainer)
    tr.update_backend = "srlx_gemm"
    with pytest.raises(ValueError, match="'srlx' or 'torch'"):
        tr._choose_backend(8)
    tr = ppo_v.Trainer.__new__(ppo_v.Trainer)
    tr.update_backend = "gemm"
    with pytest.raises(ValueError, match="'srlx' or 'torch', 'srlx_gemm'"):
        tr._choose_backend(8)
