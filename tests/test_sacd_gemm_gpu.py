"""Discrete SAC's update on the float64 matrix cores (srlx_sacd_update_gemm, csrc/srlx_sacd.hip on csrc/srlx_mlp_gemm.h) over the shapes of
tests/sacd_cases.py against the float64 yardstick of tests/sacd_reference.py, at the standing bars of tests/test_sacd_gpu.py (whose helpers measure here too):
rtol 1e-5 / atol 1e-6 on y, q1, q2, entropy, the four losses, alpha and every parameter of the five networks and log_alpha after each update; 1e-5 |g| + 1e-5
max |g| per gradient tensor.  No case and no element is left out.  Every test prints what it measured as a fraction of its bar ("SACD-ERR gemm-...", shown
with -s) before it asserts."""
import functools

import pytest
import torch

import sacd_cases as C
import sacd_reference as R
import test_sacd_gpu as T
from simple_distributed_rl_amd.algorithms import sac

pytestmark = pytest.mark.gpu
CASES = T.CASES + [(C.CLIP_SHAPE, None)]
CASE_IDS = T.CASE_IDS + ["forced-clip"]


def _case(i, auto):
    return (i, True, True) if auto is None else (i, auto, False)


def _run(i, auto, clip=False, paths=(True, True)):
    """Two updates (a hard sync, then a soft one) on a fresh seeded GPU parameter of the case, update k on the gemm path where paths[k]."""
    from simple_distributed_rl_amd.device.sacd import SacdUpdate

    B, D, A, pw, qw = C.SHAPES[i]
    p = C.make_parameter(T._cfg(i, "cuda", auto), 1000 + i, clip_case=clip)
    u = SacdUpdate(p, max_batch=B)
    steps = []
    for k, (b, gemm) in enumerate(zip(T._batches(i), paths)):
        d = T._dev(b)
        out = u.update(d["state"], d["action"], d["n_state"], d["reward"], d["done"], C.LR, C.LR, C.LR, k == 0, C.DISCOUNT, C.TAU, auto, -A, gemm=gemm)
        torch.cuda.synchronize()
        steps.append(dict(out=out, grads={name: [g.clone() for g in u.grads[name]] for name in T.TRAINED}, gla=u.grad_log_alpha.clone(), after=T._snapshot(p),
                          log_alpha=float(p.log_alpha)))
    return u, steps


def _quantities(k, out, grads, gla, params, log_alpha):
    q = T._update_quantities(k, out, grads, gla)
    q.update({f"{name}@{k}": v for name, v in T._param_quantities(params, log_alpha).items()})
    return q


def _over_the_bar(tag, i, auto, clip, steps, ks=(0, 1)):
    """The quantities of updates `ks` that miss the yardstick's (printed as fractions of their bars first)."""
    refs = T._reference(i, auto, clip)
    got, want = {}, {}
    for k in ks:
        st, ref = steps[k], refs[k]
        got.update(_quantities(k, st["out"], st["grads"], st["gla"], st["after"], st["log_alpha"]))
        want.update(_quantities(k, ref, ref["grads"], ref["grads"]["log_alpha"], ref["params"], ref["log_alpha"]))
    return T._report(tag, got, want)


def _tensors(st):
    return list(st["out"].values()) + [g for name in T.TRAINED for g in st["grads"][name]] + [st["gla"]] + [t for name in R.NETWORKS for t in st["after"][name]]


@functools.lru_cache(maxsize=None)
def _gemm(i, auto, clip):
    return _run(i, auto, clip)


@pytest.mark.parametrize("i, auto", CASES, ids=CASE_IDS)
def test_gemm_update_matches_float64_yardstick(i, auto):
    i, auto, clip = _case(i, auto)
    tag = "gemm-" + ("clip-" if clip else "") + C.shape_id(i) + ("-auto" if auto else "-fixed")
    u, steps = _gemm(i, auto, clip)
    bad = _over_the_bar(tag, i, auto, clip, steps)
    rows = _run(i, auto, clip, (False, False))[1]  # a record, not a bar: the one-hot term joins the sum behind the matrix cores, whose order inside 4 terms is their own
    pairs = [(x, y) for a, b in zip(steps, rows) for x, y in zip(_tensors(a), _tensors(b))]
    print(f"SACD-ERR {tag} values whose bits differ from the row path: {sum(int((x != y).sum()) for x, y in pairs)} of {sum(x.numel() for x, _ in pairs)}")
    assert u.steps() == [2, 2, 2, 2 if auto else 0]
    assert not bad, f"{tag}: over the bar (fraction of it): {bad}"


@pytest.mark.parametrize("i, auto", T.CASES, ids=T.CASE_IDS)
def test_two_handles_on_equal_inputs_give_equal_bits(i, auto):
    for sa, sb in zip(_gemm(i, auto, False)[1], _run(i, auto)[1]):
        assert all(torch.equal(x, y) for x, y in zip(_tensors(sa), _tensors(sb))) and sa["log_alpha"] == sb["log_alpha"]


@pytest.mark.parametrize("paths", [(False, True), (True, False)], ids=["rows-then-gemm", "gemm-then-rows"])
@pytest.mark.parametrize("i", [3, 2], ids=C.shape_id)
def test_one_handle_alternates_the_two_paths(i, paths):
    """Planes, segment tables, Adam moments and step counts are shared: the second update, on the other path, meets the yardstick's second update."""
    u, steps = _run(i, True, paths=paths)
    assert u.steps() == [2, 2, 2, 2]
    bad = _over_the_bar(f"gemm-{C.shape_id(i)}-{'gemm-first' if paths[0] else 'rows-first'}", i, True, False, steps, ks=(1,))
    assert not bad, bad


def test_trainer_runs_the_gemm_backend():
    B, A = 8, 2
    b = T._cartpole_batch(B)
    cfg = C.make_config(4, A, (64, 64, 64), (128, 128, 128), device="cuda", batch_size=B)
    p = C.make_parameter(cfg, 77)
    y = R.Yardstick(p, cfg.lr_policy, cfg.lr_q, cfg.lr_alpha, cfg.discount, cfg.soft_target_update_tau, True, -A)
    ref = y.update(b["state"], b["onehot"], b["n_state"], b["reward"], b["done"], hard_sync=True)
    tr = sac.Trainer(cfg, p, None)
    tr.update_backend = "srlx_gemm"
    tr.on_setup()
    out = tr.train_on_batch(b["state"].float().cuda(), b["onehot"].float().cuda(), b["n_state"].float().cuda(), b["reward"].float().cuda(),
                            b["done"].to(torch.uint8).cuda())
    torch.cuda.synchronize()
    assert tr.update_path == "srlx_gemm" and tr.why_not_srlx_update == "" and tr.train_count == 1
    bad = T._report("gemm-trainer", T._update_quantities(0, out, tr._srlx.grads, tr._srlx.grad_log_alpha),
                    T._update_quantities(0, ref, ref["grads"], ref["grads"]["log_alpha"]))
    for key in T.SCALARS[:4]:
        assert tr.info[key] == pytest.approx(float(ref[key]), rel=1e-5, abs=1e-6)
    assert not bad, bad
