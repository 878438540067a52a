"""V-PPO's update on the float64 matrix cores (srlx_vppo_update_gemm, csrc/srlx_mlp_gemm.h) over the cases of tests/vppo_cases.py against the float64
yardstick of tests/vppo_reference.py, at the standing bars of tests/test_vppo_gpu.py (whose helpers measure here too): rtol 1e-5 / atol 1e-6 on v, n_v, new_logpi,
the four losses, the norm and the parameters after two updates; 1e-5 |g| + 1e-5 max |g| per tensor on every gradient before and after the clip.  No case and no
element is left out.  Every test prints what it measured as a fraction of its bar ("VPPO-ERR gemm-...", shown with -s) before it asserts."""
import functools

import pytest
import torch

import test_vppo_gpu as T
from simple_distributed_rl_amd.algorithms import ppo_v

C, R = T.C, T.R
pytestmark = pytest.mark.gpu
KEYS = ("raw", "grads", "after")


def _run(name, paths=(True, True)):
    """Two updates on a fresh seeded GPU parameter of the case, update k on the gemm path where paths[k]."""
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    p = C.make_parameter(name, "cuda")
    cfg = p.config
    u = VppoUpdate(p, max_batch=C.CASES[name][0])
    steps = []
    for b, gemm in zip(C.make_batches(name), paths):
        d = T._dev(name, b)
        out = u.update(d["state"], d["n_state"], d["action"], d["old_logpi"], d["reward"], d["not_terminated"], d["total_reward"], cfg.lr, cfg.discount,
                       cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy, gemm=gemm)
        torch.cuda.synchronize()
        steps.append(dict(out=out, raw=[g.clone() for g in u.raw_grads], grads=[g.clone() for g in u.grads], after=[t.detach().clone() for t in p.net.parameters()]))
    return u, steps


def _over_the_bar(tag, name, steps, ks=(0, 1)):
    """The quantities of updates `ks`, and the parameters after the second, that miss the yardstick's (printed as fractions of their bars first)."""
    refs = C.reference(name)
    got, want = {}, {}
    for k in ks:
        got.update(T._quantities(k, steps[k]["out"], steps[k]["raw"], steps[k]["grads"]))
        want.update(T._quantities(k, refs[k], refs[k]["raw_grads"], refs[k]["grads"]))
    got.update({f"p.{j}": T._f64(t) for j, t in enumerate(steps[-1]["after"])})
    want.update({f"p.{j}": T._f64(t) for j, t in enumerate(refs[-1]["params"])})
    return T._report(tag, got, want)


@functools.lru_cache(maxsize=None)
def _gemm(name):
    return _run(name)


@pytest.mark.parametrize("name", C.NAMES)
def test_gemm_update_matches_float64_yardstick(name):
    u, steps = _gemm(name)
    bad = _over_the_bar(f"gemm-{name}", name, steps)
    rows = _run(name, (False, False))[1]  # a record, not a bar: the matrix core's order inside 4 terms is not dense<double>'s
    pairs = [(x, y) for a, b in zip(steps, rows) for x, y in zip(list(a["out"].values()) + a["raw"] + a["grads"] + a["after"],
                                                                 list(b["out"].values()) + b["raw"] + b["grads"] + b["after"])]
    print(f"VPPO-ERR gemm-{name} values whose bits differ from the row path: {sum(int((x != y).sum()) for x, y in pairs)} of {sum(x.numel() for x, _ in pairs)}")
    assert u.steps() == 2
    assert not bad, f"{name}: over the bar (fraction of it): {bad}"


@pytest.mark.parametrize("name", C.NAMES)
def test_two_handles_on_equal_inputs_give_equal_bits(name):
    for sa, sb in zip(_gemm(name)[1], _run(name)[1]):
        assert all(torch.equal(sa["out"][k], sb["out"][k]) for k in sa["out"])
        assert all(torch.equal(x, y) for key in KEYS for x, y in zip(sa[key], sb[key]))


@pytest.mark.parametrize("paths", [(False, True), (True, False)], ids=["rows-then-gemm", "gemm-then-rows"])
@pytest.mark.parametrize("name", ["mixed-b17", "normal-k8"])
def test_one_handle_alternates_the_two_paths(name, paths):
    """Planes, segment table, Adam moments and step count are shared: the second update, on the other path, meets the yardstick's second update."""
    u, steps = _run(name, paths)
    assert u.steps() == 2
    bad = _over_the_bar(f"gemm-{name}-{'gemm-first' if paths[0] else 'rows-first'}", name, steps, ks=(1,))
    assert not bad, bad


def test_trainer_runs_the_gemm_backend():
    B, env = 8, "CartPole-v1"
    D, head, n_out = T.ENVS[env]
    b = T._env_batch(env, B)
    cfg = C.make_config(D, head, n_out, (64, 64), (64,), (), device="cuda", batch_size=B, entropy_weight=0.1)
    torch.manual_seed(77)
    p = ppo_v.Parameter(cfg)
    y = R.Yardstick(p, cfg.lr, cfg.discount, cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy, C.ls_range(cfg))
    ref = y.update(b["state"], b["n_state"], b["action"].argmax(1), b["old_logpi"], b["reward"][:, 0], b["not_terminated"][:, 0], b["total_reward"][:, 0])
    tr = ppo_v.Trainer(cfg, p, None)
    tr.update_backend = "srlx_gemm"
    tr.on_setup()
    out = tr.train_on_batch(*[b[k].float().cuda() for k in ("state", "n_state", "action", "old_logpi", "reward", "not_terminated", "total_reward")])
    torch.cuda.synchronize()
    assert tr.update_path == "srlx_gemm" and tr.why_not_srlx_update == "" and tr.train_count == 1
    bad = T._report("gemm-trainer", T._quantities(0, out, None, tr._srlx.grads), T._quantities(0, ref, None, ref["grads"]))
    for key in ("loss_value", "loss_v_align", "loss_policy", "loss_e"):
        assert tr.info[key] == pytest.approx(float(ref[key]), rel=1e-5, abs=1e-6)
    assert not bad, bad
