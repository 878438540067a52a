"""Agent57's plugin with its image block on libsrlx (`QNetwork.in_block_backend = "srlx"`) and its LSTM there too: the reference's recorded trainer
step at the tolerances of tests/test_agent57_gpu.py / test_agent57_lstm_gpu.py (whose helpers build the trainer), the same step from the device sequence store,
run-to-run reproducibility, a Runner run whose worker acts through the trunk (one row), and the default, which stays torch."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


@pytest.fixture
def srlx_in_block():
    """Every QNetwork built inside the test takes "srlx" for both switches (the class attributes are the defaults); the embedding / lifelong networks' image
    blocks stay MIOpen's, which is asked for its deterministic solvers (test_agent57_lstm_gpu.py)."""
    import torch

    from simple_distributed_rl_amd.algorithms import agent57

    was = agent57.QNetwork.in_block_backend, agent57.QNetwork.lstm_backend, agent57.Memory.sequence_store, torch.backends.cudnn.deterministic
    agent57.QNetwork.in_block_backend, agent57.QNetwork.lstm_backend, torch.backends.cudnn.deterministic = "srlx", "srlx", True
    yield agent57
    agent57.QNetwork.in_block_backend, agent57.QNetwork.lstm_backend, agent57.Memory.sequence_store, torch.backends.cudnn.deterministic = was


def _record_in_block(param):
    """Every Q-network call appends (network, steps, had gradient, in_block_path, why_not_srlx_in_block)."""
    import torch

    from test_agent57_lstm_gpu import _q_nets

    calls = []
    for name, net in _q_nets(param).items():
        def hook(mod, args, out, name=name):
            calls.append((name, int(args[0][0].shape[1]), torch.is_grad_enabled(), mod.in_block_path, mod.why_not_srlx_in_block))
        net.register_forward_hook(hook)
    return calls


def _assert_golden(z, td_ext, td_int, pri, info, sds):
    """The comparisons of test_agent57_trainer_step_on_srlx_lstm_matches_reference_golden, at its tolerances."""
    np.testing.assert_allclose(td_ext.cpu().numpy(), z["td_ext"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(td_int.cpu().numpy(), z["td_int"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(pri, z["priorities"], rtol=1e-4, atol=2e-6)
    for key in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        np.testing.assert_allclose(info[key], float(z[key]), rtol=1e-5, err_msg=key)
    for name in ("q_ext", "q_int", "emb", "lifelong_train"):
        pre = f"after.{name}."
        lr = dict(q_ext=float(z["lr_ext"]), q_int=float(z["lr_int"]), emb=float(z["episodic_lr"]), lifelong_train=float(z["lifelong_lr"]))[name]
        for k in z.files:
            if k.startswith(pre):
                got = sds[name][k[len(pre):]].cpu().numpy()
                np.testing.assert_allclose(got, z[k], rtol=1e-5, atol=lr / 4, err_msg=k)
                assert np.mean(np.abs(got - z[k]) > 5e-6) < 2e-2, k


def test_trainer_step_on_srlx_in_block_matches_reference_golden(srlx_in_block):
    from test_agent57_lstm_gpu import _record_paths, _trainer_at_golden

    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    runner, rl, param, trainer, nets, rec = _trainer_at_golden(z)
    calls, lstm_calls = _record_in_block(param), _record_paths(param)
    trainer.train()
    bi, S1 = rl.burnin, rl.sequence_length + 1
    for pair in ("q_ext", "q_int"):
        want = {(pair, bi, False), (pair + "_target", bi, False), (pair + "_target", S1, False), (pair, S1, True)}  # burn-in x 2, target pass, online pass
        assert {c[:3] for c in calls if c[0].startswith(pair)} == want, calls
    assert len(calls) == 8 and all(c[3] == "srlx" and c[4] is None for c in calls), calls
    assert all(c[3] == "srlx" for c in lstm_calls), lstm_calls
    assert param.q_ext_online._trunk.training_bytes > 0 and param.q_ext_target._trunk.training_bytes == 0  # a target network's handle stays forward-only
    assert param.q_ext_online._trunk.max_rows == rl.batch_size * max(S1, bi)
    _assert_golden(z, trainer.td_ext, trainer.td_int, rec["pri"], trainer.info, {name: net.state_dict() for name, net in nets.items()})


def test_trainer_step_from_the_device_store_equals_the_host_memory(srlx_in_block):
    import torch

    from test_agent57_seqstore_gpu import _golden_step

    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    dev_out, trainer, nets = _golden_step(z, "device", srlx_in_block.Memory)
    assert all(nets[n].in_block_path == "srlx" for n in ("q_ext", "q_int", "q_ext_target", "q_int_target"))
    _assert_golden(z, dev_out["td_ext"], dev_out["td_int"], dev_out["pri"], dev_out["info"], dev_out["nets"])
    host_out, _, nets = _golden_step(z, "host", srlx_in_block.Memory)
    assert all(nets[n].in_block_path == "srlx" for n in ("q_ext", "q_int", "q_ext_target", "q_int_target"))
    assert host_out["info"] == dev_out["info"]
    np.testing.assert_array_equal(host_out["pri"], dev_out["pri"])
    assert torch.equal(host_out["td_ext"], dev_out["td_ext"]) and torch.equal(host_out["td_int"], dev_out["td_int"])
    differ = [(name, k) for name, sd in host_out["nets"].items() for k, v in sd.items() if not torch.equal(v, dev_out["nets"][name][k])]
    assert not differ, differ


def test_two_trainer_steps_are_reproducible(srlx_in_block):
    """Two fresh runners, two steps each from the golden's state: every parameter of q_ext and q_int equal bit for bit, and moved."""
    import torch

    from test_agent57_lstm_gpu import _trainer_at_golden

    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    after = []
    for _ in range(2):
        runner, rl, param, trainer, nets, rec = _trainer_at_golden(z)
        trainer.train()
        trainer.train()
        assert param.q_ext_online.in_block_path == "srlx" and param.q_int_online.in_block_path == "srlx"
        after.append({name: {k: v.clone() for k, v in nets[name].state_dict().items()} for name in ("q_ext", "q_int")})
    differ = [(name, k) for name in ("q_ext", "q_int") for k, v in after[0][name].items() if not torch.equal(v, after[1][name][k])]
    assert not differ, differ
    key = "in_block.image_block.image_layers.0.weight"
    for name in ("q_ext", "q_int"):
        assert not torch.equal(after[0][name][key].cpu(), torch.tensor(z[f"before.{name}.{key}"]))


def test_runner_end_to_end_acts_through_the_trunk(srlx_in_block):
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=True, device="cuda:0", ep_len=6, seed=1)
    rl.episodic_memory_capacity = 64
    runner.set_seed(3)
    param = runner.make_parameter()
    calls = _record_in_block(param)
    st = runner.train(max_train_count=15)
    assert st.train_count == 15 and runner.parameter is param
    for key in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        assert np.isfinite(runner.trainer.info[key]), key
    assert len(runner.evaluate(max_episodes=2)) == 2
    assert calls and all(c[3] == "srlx" for c in calls), [c for c in calls if c[3] != "srlx"][:5]
    assert any(c[1] == 1 for c in calls), "no acting pass was recorded"


def test_default_stays_torch_and_keeps_contiguous_weights():
    import torch

    from simple_distributed_rl_amd.algorithms import agent57
    from test_agent57_lstm_gpu import _trainer_at_golden

    assert agent57.QNetwork.in_block_backend == "torch"
    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    runner, rl, param, trainer, nets, rec = _trainer_at_golden(z)
    trainer.train()
    for name in ("q_ext", "q_int", "q_ext_target", "q_int_target"):
        net = nets[name]
        assert net.in_block_path == "torch" and net.why_not_srlx_in_block is None and net._trunk is None
        for conv in list(net.in_block.image_block.image_layers)[0::2]:
            assert conv.weight.is_contiguous()
