"""`update_backend = "srlx_gemm"` without a GPU: sac_not.Trainer serves it as it serves "srlx", in torch with the reason; an unknown name is
refused with the names it could have been."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import notsac_cases as C  # noqa: E402
from simple_distributed_rl_amd.algorithms import sac_not  # noqa: E402


def test_gemm_request_on_cpu_parameters_runs_torch_and_says_why():
    name = "default-b16"
    b = C.make_batches(name)[0]
    B = b["state"].shape[0]
    reasons = {}
    for backend in ("srlx_gemm", "srlx"):
        p = C.make_parameter(name)
        tr = sac_not.Trainer(p.config, p, None)
        tr.update_backend = backend
        tr.on_setup()
        tr.train_on_batch(b["state"].float(), b["n_state"].float(), b["action"].float(), b["reward"].float().reshape(B, 1),
                          b["not_terminated"].float().reshape(B, 1), b["total_reward"].float().reshape(B, 1), noise=b["noise"])
        assert tr.update_path == "torch" and tr.why_not_srlx_update
        reasons[backend] = tr.why_not_srlx_update
    assert reasons["srlx_gemm"] == reasons["srlx"]


def test_an_unknown_backend_name_is_refused_with_the_known_ones():
    tr = sac_not.Trainer.__new__(sac_not.Trainer)
    tr.update_backend = "gemm"
    with pytest.raises(ValueError, match="'srlx' or 'torch', 'srlx_gemm'"):
        tr._choose_backend(8)
