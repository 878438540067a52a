"""NoT_SAC's update on the float64 matrix cores (srlx_notsac_update_gemm, csrc/srlx_notsac.hip on csrc/srlx_mlp_gemm.h) over the cases of
tests/notsac_cases.py against the float64 yardstick of tests/notsac_reference.py, at the standing bars of tests/test_notsac_gpu.py (whose helpers measure here
too): rtol 1e-5 / atol 1e-6 on q, target_q, both actions, the three losses, both norms and every parameter after each step; 1e-5 |g| + 1e-5 max |g| per tensor on
every gradient of both networks before and after its clip.  No case and no element is left out.  Every test prints what it measured as a fraction of its bar
("NOTSAC-ERR gemm-...", shown with -s) before it asserts."""
import functools

import pytest
import torch

import notsac_cases as C
import test_notsac_gpu as T
from simple_distributed_rl_amd.algorithms import sac_not

pytestmark = pytest.mark.gpu
KEYS = ("raw", "grads", "after")


def _run(name, paths=(True, True)):
    """Two updates on a fresh seeded GPU parameter of the case, update k on the gemm path where paths[k]."""
    from simple_distributed_rl_amd.device.notsac import NotSacUpdate

    p = C.make_parameter(name, "cuda")
    cfg = p.config
    u = NotSacUpdate(p, max_batch=C.spec(name)[0])
    steps = []
    for b, gemm in zip(C.make_batches(name), paths):
        d = T._dev(name, b)
        out = u.update(d["state"], d["n_state"], d["action"], d["reward"], d["not_terminated"], d["total_reward"], d["noise"], cfg.lr, cfg.discount,
                       cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy, gemm=gemm)
        torch.cuda.synchronize()
        steps.append(dict(out=out, raw=[g.clone() for g in u.raw_grads], grads=[g.clone() for g in u.grads], after=[t.detach().clone() for t in u.params]))
    return u, steps


def _over_the_bar(tag, name, u, steps, ks=(0, 1)):
    """The quantities of updates `ks` that miss the yardstick's (printed as fractions of their bars first)."""
    refs = C.reference(name)
    got, want = {}, {}
    for k in ks:
        st, ref = steps[k], refs[k]
        got.update(T._quantities(k, st["out"], *u.split(st["raw"]), *u.split(st["grads"]), *u.split(st["after"])))
        want.update(T._quantities(k, ref, ref["p_raw_grads"], ref["q_raw_grads"], ref["p_grads"], ref["q_grads"], ref["p_params"], ref["q_params"]))
    return T._report(tag, got, want)


@functools.lru_cache(maxsize=None)
def _gemm(name):
    return _run(name)


@pytest.mark.parametrize("name", C.NAMES)
def test_gemm_update_matches_float64_yardstick(name):
    u, steps = _gemm(name)
    bad = _over_the_bar(f"gemm-{name}", name, u, steps)
    rows = _run(name, (False, False))[1]  # a record, not a bar: the matrix core's order inside 4 terms is not dense<double>'s
    pairs = [(x, y) for a, b in zip(steps, rows) for x, y in zip(list(a["out"].values()) + a["raw"] + a["grads"] + a["after"],
                                                                 list(b["out"].values()) + b["raw"] + b["grads"] + b["after"])]
    T._say(f"NOTSAC-ERR gemm-{name} values whose bits differ from the row path: {sum(int((x != y).sum()) for x, y in pairs)} of {sum(x.numel() for x, _ in pairs)}")
    assert u.steps() == 2
    assert not bad, f"{name}: over the bar (fraction of it): {bad}"


@pytest.mark.parametrize("name", C.NAMES)
def test_two_handles_on_equal_inputs_give_equal_bits(name):
    for sa, sb in zip(_gemm(name)[1], _run(name)[1]):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for key in KEYS for x, y in zip(sa[key], sb[key]))


@pytest.mark.parametrize("paths", [(False, True), (True, False)], ids=["rows-then-gemm", "gemm-then-rows"])
@pytest.mark.parametrize("name", ["b17-mixed", "cat-a16-b17"])
def test_one_handle_alternates_the_two_paths(name, paths):
    """Planes, segment tables, Adam moments and step count are shared: the second update, on the other path, meets the yardstick's second update."""
    u, steps = _run(name, paths)
    assert u.steps() == 2
    bad = _over_the_bar(f"gemm-{name}-{'gemm-first' if paths[0] else 'rows-first'}", name, u, steps, ks=(1,))
    assert not bad, bad


@pytest.mark.parametrize("name", ["default-b16", "cat-default"])
def test_trainer_runs_the_gemm_backend(name):
    ref = C.reference(name)[0]
    b = C.make_batches(name)[0]
    p = C.make_parameter(name, "cuda")
    tr = sac_not.Trainer(p.config, p, None)
    tr.update_backend = "srlx_gemm"
    tr.on_setup()
    B = b["state"].shape[0]
    col = lambda x: x.float().cuda().reshape(B, 1)  # noqa: E731
    out = tr.train_on_batch(b["state"].float().cuda(), b["n_state"].float().cuda(), b["action"].float().cuda(), col(b["reward"]), col(b["not_terminated"]),
                            col(b["total_reward"]), noise=b["noise"].cuda())
    assert tr.update_path == "srlx_gemm" and tr.why_not_srlx_update == "" and tr.train_count == 1
    u = tr._srlx
    got = T._quantities(0, out, *u.split(u.raw_grads), *u.split(u.grads), *u.split(u.params))
    want = T._quantities(0, ref, ref["p_raw_grads"], ref["q_raw_grads"], ref["p_grads"], ref["q_grads"], ref["p_params"], ref["q_params"])
    bad = T._report(f"gemm-trainer-{name}", got, want)
    for key in T.SCALARS[:3]:
        assert tr.info[key] == pytest.approx(ref[key], rel=1e-5, abs=1e-6)
    assert not bad, bad
