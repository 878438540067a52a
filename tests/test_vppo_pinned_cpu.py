"""V-PPO pinned on the reference's own code.  A child interpreter (tests/vppo_recorder.py, the reference on its path) loads the weights of
tests/vppo_cases.py's pin cases into the reference's `srl.algorithms.ppo_v` network, hand-feeds their items into its memory -- the batch is the whole memory --
and runs two `Trainer.train()` calls on the reference's Grid (discrete) and on a toy continuous environment (k = 2, squashed and plain).  The plugin's "torch"
backend on the CPU and the float64 yardstick of tests/vppo_reference.py then have to give the reference's four losses, its gradients as optimizer.step() found
them, and its parameters after one and after two steps, at the project's standing bars (rtol 1e-5 / atol 1e-6; a gradient tensor at rtol 1e-5 with atol
1e-5 max |g|).  Nothing the child writes is committed.  CPU only; the whole module is skipped where the reference cannot be imported
(oracle/_golden_record.reference_root: $SRL_REFERENCE)."""
import importlib.machinery
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ORACLE = os.path.join(ROOT, "oracle")
if ORACLE not in sys.path:
    sys.path.insert(0, ORACLE)

import _golden_record  # noqa: E402

try:
    REFERENCE = _golden_record.reference_root()
except SystemExit as e:
    pytest.skip(f"the reference cannot be imported: {e}", allow_module_level=True)
if importlib.machinery.PathFinder.find_spec("srl", [REFERENCE]) is None or importlib.machinery.PathFinder.find_spec("torch") is None:
    pytest.skip(f"the reference cannot be imported: no srl package under {REFERENCE}, or no torch", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vppo_cases as C  # noqa: E402
import vppo_recorder  # noqa: E402
from simple_distributed_rl_amd.algorithms import ppo_v  # noqa: E402

PINS = list(C.PIN_CASES)
LOSSES = ("loss_value", "loss_v_align", "loss_policy", "loss_e")


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """The reference's two steps of every pin case: computed once in one child interpreter, shared, never modified."""
    folder = str(tmp_path_factory.mktemp("vppo_pin"))
    cases = []
    for name in PINS:
        B, D, head, n_out, trunk, value, policy, squashed, ew, max_norm, forced = C.spec(name)
        p = C.make_parameter(name)
        save = {"w_" + k: v.numpy() for k, v in p.net.state_dict().items()}
        for k, b in enumerate(C.make_batches(name)):
            cols = dict(state=b["state"], n_state=b["n_state"], action=C.onehot(name, b["action"]), old_logpi=b["old_logpi"], reward=b["reward"],
                        not_done=b["not_terminated"], total_reward=b["total_reward"])
            save.update({f"s{k}_{c}": v.numpy().astype(np.float32) for c, v in cols.items()})
        np.savez(os.path.join(folder, f"in_{name}.npz"), **save)
        cases.append(dict(name=name, env="toy" if head else "Grid", batch_size=B,
                          config=dict(lr=C.LR, discount=C.DISCOUNT, clip_range=C.CLIP, entropy_weight=ew, loss_align_coeff=C.ALIGN, max_grad_norm=max_norm,
                                      squashed_gaussian_policy=squashed)))
    json.dump(cases, open(os.path.join(folder, "cases.json"), "w"))
    env = dict(os.environ, SRL_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vppo_recorder.py"), folder], env=env, cwd=folder, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return {name: dict(np.load(os.path.join(folder, f"out_{name}.npz"))) for name in PINS}


def _frac(got, want, gradient=False):
    got, want = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(want).detach().double().reshape(-1)
    atol = 1e-5 * float(want.abs().max()) if gradient else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _batch_of(rec, k):
    """Step k's batch as the reference's trainer held it (its sample's order), float32 tensors in the Trainer's layout."""
    return [torch.from_numpy(rec[f"k{k}_{n}"].copy()) for n in vppo_recorder.NP_ARRAYS]


@pytest.mark.parametrize("name", PINS)
def test_state_dicts_move_between_the_reference_and_the_plugin_by_key(name, recorded):
    rec = recorded[name]
    p = C.make_parameter(name)
    sd = p.net.state_dict()
    assert list(rec["keys"]) == list(sd)
    for key, t in sd.items():
        assert rec[f"k0_before_{key}"].shape == tuple(t.shape) and rec[f"k0_before_{key}"].dtype == np.float32, key
        assert np.array_equal(rec[f"k0_before_{key}"], t.numpy()), key  # (the child loaded this project's state dict into the reference's network, by key)
    p.call_restore({key: torch.from_numpy(rec[f"k1_after_{key}"]) for key in sd}, from_serialized=True)
    for key, t in p.net.state_dict().items():
        assert np.array_equal(rec[f"k1_after_{key}"], t.numpy()), key


@pytest.mark.parametrize("name", PINS)
def test_the_batch_is_the_whole_memory(name, recorded):
    """Every hand-fed item is in each step's batch, once (the reference's sample is a permutation of the memory)."""
    rec = recorded[name]
    for k, b in enumerate(C.make_batches(name)):
        fed = np.concatenate([b["state"].numpy(), b["old_logpi"].numpy(), b["reward"].numpy()[:, None]], axis=1).astype(np.float32)
        got = np.concatenate([rec[f"k{k}_state_np"], rec[f"k{k}_old_logpi_np"], rec[f"k{k}_reward_np"]], axis=1)
        assert sorted(map(tuple, fed.tolist())) == sorted(map(tuple, got.tolist()))


@pytest.mark.parametrize("name", PINS)
def test_torch_backend_gives_the_references_losses_gradients_and_parameters(name, recorded):
    rec = recorded[name]
    p = C.make_parameter(name)
    tr = ppo_v.Trainer(p.config, p, None)
    tr.update_backend = "torch"
    tr.on_setup()
    worst = {}
    for k in range(2):
        tr.train_on_batch(*_batch_of(rec, k))
        want_info = {key: float(rec[f"k{k}_info_{key}"]) for key in LOSSES if f"k{k}_info_{key}" in rec}
        assert set(tr.info) == set(want_info) == ({"loss_value", "loss_v_align", "loss_policy"} | ({"loss_e"} if p.config.entropy_weight > 0 else set()))
        for key, v in want_info.items():
            worst[key] = max(worst.get(key, 0.0), _frac(tr.info[key], v))
        for i, t in enumerate(p.net.parameters()):
            worst["grads"] = max(worst.get("grads", 0.0), _frac(t.grad, rec[f"k{k}_grad_{i}"], gradient=True))
        for key, t in p.net.state_dict().items():
            worst[f"params@{k}"] = max(worst.get(f"params@{k}", 0.0), _frac(t, rec[f"k{k}_after_{key}"]))
    print(f"VPPO-PIN torch {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", PINS)
def test_yardstick_gives_the_references_losses_gradients_and_parameters(name, recorded):
    rec = recorded[name]
    head = C.spec(name)[2]
    y = C._yardstick(name, C.make_parameter(name))
    worst = {}
    for k in range(2):
        state, n_state, action, old_logpi, reward, not_term, total_reward = [t.double() for t in _batch_of(rec, k)]
        out = y.update(state, n_state, action if head else action.argmax(1), old_logpi, reward[:, 0], not_term[:, 0], total_reward[:, 0])
        assert out["margin"] >= 1e-3
        for key in LOSSES:
            if f"k{k}_info_{key}" in rec:
                worst[key] = max(worst.get(key, 0.0), _frac(out[key], rec[f"k{k}_info_{key}"]))
        for i, g in enumerate(out["grads"]):
            worst["grads"] = max(worst.get("grads", 0.0), _frac(g, rec[f"k{k}_grad_{i}"], gradient=True))
        for key, t in zip(rec["keys"], out["params"]):
            worst[f"params@{k}"] = max(worst.get(f"params@{k}", 0.0), _frac(t, rec[f"k{k}_after_{key}"]))
    print(f"VPPO-PIN yardstick {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
