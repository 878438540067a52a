"""`update_backend = "srlx_gemm"` without a GPU: sac.Trainer serves it as it serves "srlx", in torch with the reason; an unknown name is refused
with the names it could have been."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sacd_cases as C  # noqa: E402
from simple_distributed_rl_amd.algorithms import sac  # noqa: E402


def test_gemm_request_on_cpu_parameters_runs_torch_and_says_why():
    B, D, A, pw, qw = C.SHAPES[2]
    b = C.make_batch(B, D, A, 30)
    reasons = {}
    for backend in ("srlx_gemm", "srlx"):
        cfg = C.make_config(D, A, pw, qw)
        tr = sac.Trainer(cfg, C.make_parameter(cfg, 21), None)
        tr.update_backend = backend
        tr.on_setup()
        tr.train_on_batch(b["state"].float(), b["onehot"].float(), b["n_state"].float(), b["reward"].float(), b["done"].to(torch.uint8))
        assert tr.update_path == "torch" and tr.train_count == 1
        reasons[backend] = tr.why_not_srlx_update
    assert reasons["srlx_gemm"] == reasons["srlx"] == "the parameters are CPU tensors"


def test_an_unknown_backend_name_is_refused_with_the_known_ones():
    B, D, A, pw, qw = C.SHAPES[2]
    cfg = C.make_config(D, A, pw, qw)
    tr = sac.Trainer(cfg, C.make_parameter(cfg, 21), None)
    tr.update_backend = "gemm"
    tr.on_setup()
    with pytest.raises(ValueError, match="'srlx' or 'torch', 'srlx_gemm'"):
        tr._choose_backend(8)
