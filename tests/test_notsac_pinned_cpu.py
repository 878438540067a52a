"""NoT_SAC pinned on the reference's own code.  A child interpreter (tests/notsac_recorder.py, the reference on its path) loads the weights of
tests/notsac_cases.py's pin cases into the reference's two `srl.algorithms.sac_not` networks by key, hand-feeds their items into its memory -- the batch is the
whole memory -- and runs two `Trainer.train()` calls, each behind a `torch.manual_seed`, on the reference's Grid (discrete) and on a toy continuous
environment (K = 2, squashed and plain).  The plugin seeds the same way and has to draw the noise that reproduces the actions the reference's Q-network was
called with; the plugin's "torch" backend on the CPU and the float64 yardstick of tests/notsac_reference.py then have to give the reference's three losses, both
gradient sets as the two optimizer.step() calls found them, and both networks' parameters after one and after two steps, at the project's standing bars (rtol
1e-5 / atol 1e-6; a gradient tensor at rtol 1e-5 with atol 1e-5 max |g|).  Nothing the child writes is committed.  CPU only; the whole module is skipped where
the reference cannot be imported (oracle/_golden_record.reference_root: $SRL_REFERENCE)."""
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
import notsac_cases as C  # noqa: E402
import notsac_recorder  # noqa: E402
from simple_distributed_rl_amd.algorithms import sac_not  # noqa: E402

PINS = list(C.PIN_CASES)
LOSSES = ("loss_q", "loss_q_align", "loss_policy")
SEEDS = (4321, 8765)


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """The reference's two steps of every pin case: computed once in one child interpreter, shared, never modified."""
    folder = str(tmp_path_factory.mktemp("notsac_pin"))
    cases = []
    for name in PINS:
        B, D, head, n_out, policy, q, act_emb, squashed, max_norm, forced = C.spec(name)
        p = C.make_parameter(name)
        save = {"wp_" + k: v.numpy() for k, v in p.policy.state_dict().items()}
        save.update({"wq_" + k: v.numpy() for k, v in p.qnet.state_dict().items()})
        for k, b in enumerate(C.make_batches(name)):
            cols = dict(state=b["state"], n_state=b["n_state"], action=b["action"], reward=b["reward"], not_done=b["not_terminated"], total_reward=b["total_reward"])
            save.update({f"s{k}_{c}": v.numpy().astype(np.float32) for c, v in cols.items()})
        np.savez(os.path.join(folder, f"in_{name}.npz"), **save)
        cases.append(dict(name=name, env="toy" if head else "Grid", batch_size=B, seeds=list(SEEDS),
                          config=dict(lr=C.LR, discount=C.DISCOUNT, loss_align_coeff=C.ALIGN, max_grad_norm=max_norm, squashed_gaussian_policy=squashed)))
    json.dump(cases, open(os.path.join(folder, "cases.json"), "w"))
    env = dict(os.environ, SRL_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "notsac_recorder.py"), folder], env=env, cwd=folder, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return {name: dict(np.load(os.path.join(folder, f"out_{name}.npz"))) for name in PINS}


def _frac(got, want, gradient=False):
    got, want = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(want).detach().double().reshape(-1)
    atol = 1e-5 * float(want.abs().max()) if gradient else 1e-6
    return float(((got - want).abs() / (atol + 1e-5 * want.abs() + 1e-300)).max())


def _batch_of(rec, k):
    """Step k's batch as the reference's trainer held it (its sample's order), float32 tensors in the Trainer's layout."""
    return [torch.from_numpy(rec[f"k{k}_{n}"].copy()) for n in notsac_recorder.NP_ARRAYS]


def _trainer(name):
    p = C.make_parameter(name)
    tr = sac_not.Trainer(p.config, p, None)
    tr.update_backend = "torch"
    tr.on_setup()
    return p, tr


@pytest.mark.parametrize("name", PINS)
def test_state_dicts_move_between_the_reference_and_the_plugin_by_key(name, recorded):
    rec = recorded[name]
    p = C.make_parameter(name)
    for tag, net in (("p", p.policy), ("q", p.qnet)):
        sd = net.state_dict()
        assert list(rec[f"keys_{tag}"]) == list(sd)
        for key, t in sd.items():
            assert rec[f"k0_before_{tag}_{key}"].dtype == np.float32 and np.array_equal(rec[f"k0_before_{tag}_{key}"], t.numpy()), key
    p.call_restore([{key: torch.from_numpy(rec[f"k1_after_{tag}_{key}"]) for key in net.state_dict()} for tag, net in (("p", p.policy), ("q", p.qnet))],
                   from_serialized=True)
    for tag, net in (("p", p.policy), ("q", p.qnet)):
        for key, t in net.state_dict().items():
            assert np.array_equal(rec[f"k1_after_{tag}_{key}"], t.numpy()), key


@pytest.mark.parametrize("name", PINS)
def test_the_batch_is_the_whole_memory(name, recorded):
    """Every hand-fed item is in each step's batch, once (the reference's sample is a permutation of the memory)."""
    rec = recorded[name]
    for k, b in enumerate(C.make_batches(name)):
        fed = np.concatenate([b["state"].numpy(), b["action"].numpy(), b["reward"].numpy()[:, None]], axis=1).astype(np.float32)
        got = np.concatenate([rec[f"k{k}_state_np"], rec[f"k{k}_action_np"], rec[f"k{k}_reward_np"]], axis=1)
        assert sorted(map(tuple, fed.tolist())) == sorted(map(tuple, got.tolist()))
        assert np.array_equal(rec[f"k{k}_qcall_1"], rec[f"k{k}_action_np"])  # the Q-network's second call is on the stored actions


@pytest.mark.parametrize("name", PINS)
def test_the_plugins_seeded_noise_reproduces_the_references_actions(name, recorded):
    """After the same torch.manual_seed the trainer's two noise planes give, through the plugin's own heads, the next action and the policy action the
    reference's Q-network was called with -- at every step (the weights of step 1 are the reference's own after step 0)."""
    rec = recorded[name]
    p, tr = _trainer(name)
    cfg = p.config
    for k in range(2):
        p.call_restore([{key: torch.from_numpy(rec[f"k{k}_before_{tag}_{key}"]) for key in net.state_dict()} for tag, net in (("p", p.policy), ("q", p.qnet))],
                       from_serialized=True)
        state, n_state = _batch_of(rec, k)[:2]
        torch.manual_seed(SEEDS[k])
        noise = tr.draw_noise(state.shape[0])
        with torch.no_grad():
            n_dist = p.policy(n_state)
            if tr.discrete:
                n_action = n_dist.sample(temperature=cfg.target_policy_temperature, onehot=True, noise=noise[0])
            else:
                n_action = n_dist.mean() + n_dist.stddev() * noise[0]
                n_action = torch.tanh(n_action) if cfg.squashed_gaussian_policy else n_action
        assert torch.equal(n_action, torch.from_numpy(rec[f"k{k}_qcall_0"])), k  # the same float32 operations on the same draws: bit for bit
        # the policy action is taken after the Q step: checked through a whole train_on_batch
        p2, tr2 = _trainer(name)
        p2.call_restore([{key: torch.from_numpy(rec[f"k{k}_before_{tag}_{key}"]) for key in net.state_dict()} for tag, net in (("p", p2.policy), ("q", p2.qnet))],
                        from_serialized=True)
        out = tr2.train_on_batch(*_batch_of(rec, k), noise=noise)
        assert _frac(out["next_action"], rec[f"k{k}_qcall_0"]) <= 1.0 and _frac(out["pi_action"], rec[f"k{k}_qcall_2"]) <= 1.0


@pytest.mark.parametrize("name", PINS)
def test_torch_backend_gives_the_references_losses_gradients_and_parameters(name, recorded):
    """noise=None: the trainer draws its own planes behind the reference's seeds."""
    rec = recorded[name]
    p, tr = _trainer(name)
    worst = {}
    for k in range(2):
        seen = {}
        tr._backend_for(C.spec(name)[0])
        step = tr.opt_q.step
        tr.opt_q.step = lambda *a, **kw: (seen.update(q=[t.grad.clone() for t in p.qnet.parameters()]), step(*a, **kw))[1]
        torch.manual_seed(SEEDS[k])
        tr.train_on_batch(*_batch_of(rec, k))
        tr.opt_q.step = step
        want_info = {key: float(rec[f"k{k}_info_{key}"]) for key in LOSSES}
        assert set(tr.info) == set(LOSSES)
        exact = []  # what is not equal to the reference's to the bit
        for key, v in want_info.items():
            worst[key] = max(worst.get(key, 0.0), _frac(tr.info[key], v))
            exact += [key] if tr.info[key] != v else []
        for i, g in enumerate(seen["q"]):
            worst["q_grads"] = max(worst.get("q_grads", 0.0), _frac(g, rec[f"k{k}_qgrad_{i}"], gradient=True))
            exact += [f"qgrad{i}"] if not np.array_equal(g.numpy(), rec[f"k{k}_qgrad_{i}"]) else []
        for i, t in enumerate(p.policy.parameters()):
            worst["p_grads"] = max(worst.get("p_grads", 0.0), _frac(t.grad, rec[f"k{k}_pgrad_{i}"], gradient=True))
            exact += [f"pgrad{i}"] if not np.array_equal(t.grad.numpy(), rec[f"k{k}_pgrad_{i}"]) else []
        for tag, net in (("p", p.policy), ("q", p.qnet)):
            for key, t in net.state_dict().items():
                worst[f"params@{k}"] = max(worst.get(f"params@{k}", 0.0), _frac(t, rec[f"k{k}_after_{tag}_{key}"]))
                exact += [f"{tag}.{key}"] if not np.array_equal(t.numpy(), rec[f"k{k}_after_{tag}_{key}"]) else []
        # The same float32 torch operations on the same draws in the same order.  Whether that is equal to the BIT is printed, not required: the bars are the
        # requirement, since a matrix product's summation order may change with the thread count of the two interpreters.
        worst[f"not_bit_equal@{k}"] = float(len(exact))
    print(f"NOTSAC-PIN torch {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for k, v in worst.items() if not k.startswith("not_bit_equal")), worst


@pytest.mark.parametrize("name", PINS)
def test_yardstick_gives_the_references_losses_gradients_and_parameters(name, recorded):
    rec = recorded[name]
    p, tr = _trainer(name)
    y = C.yardstick(name, p)
    worst = {}
    for k in range(2):
        state, n_state, action, reward, not_term, total_reward = [t.double() for t in _batch_of(rec, k)]
        torch.manual_seed(SEEDS[k])
        noise = tr.draw_noise(state.shape[0])
        out = y.update(state, n_state, action, reward[:, 0], not_term[:, 0], total_reward[:, 0], noise)
        assert out["margin"] >= 1e-3
        worst["actions"] = max(worst.get("actions", 0.0), _frac(out["next_action"], rec[f"k{k}_qcall_0"]), _frac(out["pi_action"], rec[f"k{k}_qcall_2"]))
        for key in LOSSES:
            worst[key] = max(worst.get(key, 0.0), _frac(out[key], rec[f"k{k}_info_{key}"]))
        for tag in ("q", "p"):
            for i, g in enumerate(out[f"{tag}_grads"]):
                worst[f"{tag}_grads"] = max(worst.get(f"{tag}_grads", 0.0), _frac(g, rec[f"k{k}_{tag}grad_{i}"], gradient=True))
            for key, t in zip(rec[f"keys_{tag}"], out[f"{tag}_params"]):
                worst[f"params@{k}"] = max(worst.get(f"params@{k}", 0.0), _frac(t, rec[f"k{k}_after_{tag}_{key}"]))
    print(f"NOTSAC-PIN yardstick {name} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
