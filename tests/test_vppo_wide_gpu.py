"""V-PPO's gemm-only handle (srlx_vppo_create_gemm, k_mlp_gemm_wgrad in csrc/srlx_mlp_gemm.h) over the cases of tests/vppo_wide_cases.py against the
float64 yardstick of tests/vppo_reference.py, at the standing bars of tests/test_vppo_gpu.py (whose helpers measure here too): rtol 1e-5 / atol 1e-6 on v, n_v,
new_logpi, the four losses, the norm and the parameters after two updates; 1e-5 |g| + 1e-5 max |g| per tensor on every gradient before and after the clip.  No
case and no element is left out.  Every test prints what it measured as a fraction of its bar ("VPPO-ERR wide-...", shown with -s) before it asserts."""
import ctypes

import pytest
import torch

import test_vppo_gpu as T
import vppo_wide_cases as W
from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import ppo_v

pytestmark = pytest.mark.gpu


def _dev(name, b):
    f = lambda x: x.float().cuda()  # noqa: E731
    return {k: (v.int().cuda() if k == "action" and not W._ALL[name][2] else f(v)) for k, v in b.items()}


def _run(name):
    """Two updates on a fresh seeded GPU parameter of the case, on a gemm-only handle."""
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    p = W.make_parameter(name, "cuda")
    cfg = p.config
    u = VppoUpdate(p, max_batch=W.CASES[name][0], gemm_only=True)
    steps = []
    for b in W.make_batches(name):
        d = _dev(name, b)
        out = u.update(d["state"], d["n_state"], d["action"], d["old_logpi"], d["reward"], d["not_terminated"], d["total_reward"], cfg.lr, cfg.discount,
                       cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy, gemm=True)
        torch.cuda.synchronize()
        steps.append(dict(out=out, raw=[g.clone() for g in u.raw_grads], grads=[g.clone() for g in u.grads], after=[t.detach().clone() for t in p.net.parameters()]))
    return u, d, steps


@pytest.mark.parametrize("name", W.NAMES)
def test_wide_update_matches_float64_yardstick(name):
    u, _, steps = _run(name)
    refs = W.reference(name)
    got, want = {}, {}
    for k in (0, 1):
        got.update(T._quantities(k, steps[k]["out"], steps[k]["raw"], steps[k]["grads"]))
        want.update(T._quantities(k, refs[k], refs[k]["raw_grads"], refs[k]["grads"]))
    got.update({f"p.{j}": T._f64(t) for j, t in enumerate(steps[-1]["after"])})
    want.update({f"p.{j}": T._f64(t) for j, t in enumerate(refs[-1]["params"])})
    bad = T._report(f"wide-{name}", got, want)
    assert u.steps() == 2
    assert not bad, f"{name}: over the bar (fraction of it): {bad}"


def test_two_handles_on_equal_inputs_give_equal_bits():
    for sa, sb in zip(_run("normal-b130")[2], _run("normal-b130")[2]):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for key in ("raw", "grads", "after") for x, y in zip(sa[key], sb[key]))


def test_gemm_only_handle_refuses_the_row_update_and_create_refuses_4097():
    u, d, _ = _run("one-row")
    with pytest.raises(ValueError, match="srlx_vppo_update_gemm only"):
        u.update(*d.values(), 1e-3, 0.9, 0.1, 0.0, 0.1, 10.0, False, gemm=False)
    out = torch.full((5,), 7.0, device="cuda")
    lib, ptrs = N.lib(), [N.tptr(t) for t in d.values()]
    st = lib.srlx_vppo_update(u._h, 1, *ptrs, 1e-3, 0.9, 0.1, 0.0, 0.1, 10.0, 0, u.ls_lo, u.ls_hi, N.tptr(out), N.tptr(out), N.tptr(out), N.tptr(out), None)
    torch.cuda.synchronize()
    assert st == N.ERR_INVALID and b"vppo_update: a handle of srlx_vppo_create_gemm" in lib.srlx_last_error()
    assert bool((out == 7.0).all()) and u.steps() == 2
    h, w = N.c_p(), N._int_array((32,))
    assert lib.srlx_vppo_create_gemm(ctypes.byref(h), 1, 0, 2, 1, w, 0, None, 0, None, 4097, 0) == N.ERR_INVALID and not h.value
    assert b"vppo_create_gemm: max_batch 4097 (1..4096)" in lib.srlx_last_error()


def _trainer(backend):
    name = "trainer-b512"
    p = W.make_parameter(name, "cuda")
    tr = ppo_v.Trainer(p.config, p, None)
    tr.update_backend = backend
    tr.on_setup()
    b = W.make_batches(name)[0]
    b = dict(b, action=torch.nn.functional.one_hot(b["action"], 2).double())
    col = lambda k: b[k].float().cuda().reshape(512, -1)  # noqa: E731
    out = tr.train_on_batch(*[col(k) for k in ("state", "n_state", "action", "old_logpi", "reward", "not_terminated", "total_reward")])
    torch.cuda.synchronize()
    return tr, out, W.reference(name)[0]


def test_trainer_runs_a_batch_of_512_on_the_gemm_backend():
    tr, out, ref = _trainer("srlx_gemm")
    assert tr.update_path == "srlx_gemm" and tr.why_not_srlx_update == "" and tr._srlx.gemm_only and tr._srlx.max_batch == 512
    bad = T._report("wide-trainer-b512", T._quantities(0, out, tr._srlx.raw_grads, tr._srlx.grads), T._quantities(0, ref, ref["raw_grads"], ref["grads"]))
    assert not bad, bad


def test_trainer_keeps_a_batch_of_512_on_torch_when_asked_for_srlx():
    tr, _, _ = _trainer("srlx")
    assert tr.update_path == "torch" and tr.why_not_srlx_update == "batch size 512 above max_batch 256"
