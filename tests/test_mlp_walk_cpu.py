"""The MLP walk's acting path without a GPU: srlx_vppo_walk's and srlx_notsac_walk's refusals that need no device, `Parameter.dist` on CPU
parameters of both plugins, and the host's plane plan at the envelope's corner."""
import os
import sys

import numpy as np
import pytest
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo_v, sac_not
from simple_distributed_rl_amd.device import _row_update as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import notsac_cases as NC  # noqa: E402
import vppo_cases as VC  # noqa: E402


@pytest.mark.parametrize("n", [0, 65537])
@pytest.mark.parametrize("name, nargs", [("vppo_walk", 9), ("notsac_walk", 8)])
def test_walk_refuses_the_row_count_before_any_device_call(name, nargs, n):
    lib = N.lib()
    args = [None, n, None, -1.0, 1.0] + [None] * (nargs - 5)
    assert getattr(lib, "srlx_" + name)(*args) == N.ERR_INVALID
    assert f"{name}: n_rows {n} (1..65536)".encode() in lib.srlx_last_error()


@pytest.mark.parametrize("make", [lambda: ppo_v.Parameter(VC.make_config(3, 0, 2, (32,), (32,), ())), lambda: sac_not.Parameter(NC.make_config(3, 1, 2, (32,), (32,), 32))],
                         ids=["vppo", "notsac"])
def test_dist_on_cpu_parameters_runs_torch_and_says_why(make):
    p = make()
    assert type(p).act_backend == "torch"  # (the default of this change)
    states = np.ones((4, 3), np.float32)
    want = p.dist(states)
    assert p.act_path == "torch" and p.why_not_srlx_act == ""
    p.act_backend = "srlx"
    got = p.dist(states)
    assert p.act_path == "torch" and p.why_not_srlx_act == "the parameters are CPU tensors"
    value = lambda d: d.logits() if isinstance(d, ppo_v.CategoricalDist) else d.mean()  # noqa: E731
    assert type(got) is type(want) and torch.equal(value(got), value(want))
    p.act_backend = "hip"
    with pytest.raises(ValueError, match="act_backend 'hip'"):
        p.dist(states)


def test_the_plane_plan_of_the_corner_fits_the_lds():
    from simple_distributed_rl_amd.device.notsac import NotSacAct
    from simple_distributed_rl_amd.device.vppo import VppoAct

    w = (512, 512, 512)
    corner = R.walk_plan(256, *VppoAct.passes_of(256, 0, 16, w, w[:2], w[:2]))
    assert corner == (3, 4 * 16 * (260 + 3 * 516)) and corner[1] <= 163840  # 115 712 bytes
    assert R.walk_plan(256, *NotSacAct.passes_of(256, 1, 8, w, w, 32)) == (2, 4 * 16 * (260 + 2 * 516))
    assert R.walk_plan(1, *VppoAct.passes_of(1, 0, 2, (32,), (), ())) == (1, 4 * 16 * (36 + 36))
    # value () beside policy (64, 96): the trunk's output outlives both policy planes
    assert R.walk_plan(17, *VppoAct.passes_of(17, 1, 8, (96, 64, 32), (), (64, 96)))[0] == 3
    assert R.walk_plan(4, [(0, (32,)), (1, (32, 32)), (1, (32, 32))], (2, 3, 4, 5)) is None  # four values alive at once: refused
    assert VppoAct.rows_reason(65536) == "" and NotSacAct.rows_reason(65537) == "65537 rows above 65536 in one call"
