"""The gemm-only V-PPO handle without a GPU: the two envelopes side by side, the new cases' distance from the kinks by the yardstick alone, and
the trainers whose update class declares no GEMM_MAX_BATCH answering as they always did."""
import pytest

import notsac_cases
import sacd_cases
import vppo_wide_cases as W
from simple_distributed_rl_amd.algorithms import sac, sac_not
from simple_distributed_rl_amd.device import _row_update, sacd
from simple_distributed_rl_amd.device.vppo import VppoUpdate

SHAPE = (4, 0, 2, (64, 64), (64,), ())


def test_envelope_reason_at_both_bounds():
    assert VppoUpdate.GEMM_MAX_BATCH == 4096
    assert [VppoUpdate.envelope_reason(*SHAPE, b) for b in (256, 257, 4096, 4097)] == [
        "", "batch size 257 above max_batch 256", "batch size 4096 above max_batch 256", "batch size 4097 above max_batch 256"]
    assert [VppoUpdate.envelope_reason(*SHAPE, b, gemm=True) for b in (256, 257, 4096, 4097)] == ["", "", "", "batch size 4097 above max_batch 4096"]
    bad = (4, 0, 2, (48,), (64,), ())
    assert VppoUpdate.envelope_reason(*bad, 512, gemm=True) == VppoUpdate.envelope_reason(*bad, 64) != ""  # the same shape sentence


@pytest.mark.parametrize("name", list(W._ALL))
def test_every_case_stays_off_the_kinks(name):
    margins = [out["margin"] for out in W.reference(name)]
    print(f"VPPO-ERR wide-{name} margins={margins}")
    assert min(margins) >= 1e-3


def test_sac_trainers_keep_refusing_batches_above_256_on_the_gemm_name(monkeypatch):
    """(CPU parameters: the tensors' own reason is taken out of the way so that the batch is what `why_not` answers about.)"""
    monkeypatch.setattr(sacd, "tensor_reason", lambda tensors: "")
    monkeypatch.setattr(_row_update, "tensor_reason", lambda tensors: "")
    cfg = sacd_cases.make_config(4, 2, (64,), (64,))
    p = notsac_cases.make_parameter("default-b16")
    for tr in (sac.Trainer(cfg, sacd_cases.make_parameter(cfg, 21), None), sac_not.Trainer(p.config, p, None)):
        tr.update_backend = "srlx_gemm"
        tr.on_setup()
        tr._choose_backend(257)
        assert tr._backend == "torch" and tr.why_not_srlx_update == "batch size 257 above max_batch 256"
