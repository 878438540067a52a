"""Agent57's plugin with its recurrent layer on libsrlx's LSTM kernels (`lstm_backend = "srlx"` forced on all four Q-networks, whatever the default is): the
reference's recorded trainer step at tests/test_agent57_gpu.py's tolerances, a short Runner run whose worker acts through the kernels (B = 1, T = 1), and
run-to-run reproducibility of a trainer step."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-5

pytestmark = pytest.mark.gpu


def _q_nets(param):
    return dict(q_ext=param.q_ext_online, q_int=param.q_int_online, q_ext_target=param.q_ext_target, q_int_target=param.q_int_target)


def _force_srlx(param):
    for net in _q_nets(param).values():
        net.lstm_backend = "srlx"


def _record_paths(param):
    """Every Q-network call appends (network, steps, had gradient, lstm_path)."""
    import torch

    calls = []
    for name, net in _q_nets(param).items():
        def hook(mod, args, out, name=name):
            calls.append((name, int(args[0][0].shape[1]), torch.is_grad_enabled(), mod.lstm_path))
        net.register_forward_hook(hook)
    return calls


def _trainer_at_golden(z):
    import torch

    from simple_distributed_rl_amd.base.context import RunContext
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(z, intrinsic=True, device="cuda:0")
    param, trainer = runner.parameter, runner.trainer
    ctx = RunContext(runner.env_config, rl)
    ctx.setup_device()
    trainer.setup(ctx)
    _force_srlx(param)
    nets = dict(_q_nets(param), emb=param.emb_network, lifelong_target=param.lifelong_target, lifelong_train=param.lifelong_train)
    for name, net in nets.items():
        pre = f"before.{name}."
        net.load_state_dict({k[len(pre):]: torch.tensor(z[k]) for k in z.files if k.startswith(pre)})
    A, B = int(z["n_actions"]), len(z["actor_idx"])
    eye = np.identity(A, dtype=int)
    batches = [[list(z["states"][b]), [eye[a] for a in z["actions"][b]], list(z["rewards_ext"][b]), list(z["rewards_int"][b]), list(z["dones"][b]),
                int(z["actor_idx"][b]), [[] for _ in range(int(z["sequence_length"]))], [z["h_ext"][b], z["c_ext"][b]], [z["h_int"][b], z["c_int"][b]]]
               for b in range(B)]
    rec = {}
    trainer.memory.sample = lambda *a, **k: (batches, z["weights"], list(range(B)))
    trainer.memory.update = lambda args, pri, step: rec.update(pri=np.asarray(pri).copy())
    trainer.train_count = 1
    return runner, rl, param, trainer, nets, rec


def test_agent57_trainer_step_on_srlx_lstm_matches_reference_golden():
    """test_agent57_trainer_step_matches_reference_golden's body and tolerances with the LSTM on libsrlx; the burn-in, target and online passes of both
    Q-network pairs all took the kernels."""
    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    runner, rl, param, trainer, nets, rec = _trainer_at_golden(z)
    calls = _record_paths(param)
    trainer.train()
    bi, S1 = rl.burnin, rl.sequence_length + 1
    for pair in ("q_ext", "q_int"):
        want = {(pair, bi, False), (pair + "_target", bi, False), (pair + "_target", S1, False), (pair, S1, True)}  # burn-in x 2, target pass, online pass
        assert {c[:3] for c in calls if c[0].startswith(pair)} == want, calls
    assert len(calls) == 8 and all(c[3] == "srlx" for c in calls), calls
    np.testing.assert_allclose(trainer.td_ext.cpu().numpy(), z["td_ext"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(trainer.td_int.cpu().numpy(), z["td_int"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(rec["pri"], z["priorities"], rtol=1e-4, atol=2e-6)
    for key in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        np.testing.assert_allclose(trainer.info[key], float(z[key]), rtol=RTOL, err_msg=key)
    for name in ("q_ext", "q_int", "emb", "lifelong_train"):
        pre = f"after.{name}."
        sd = nets[name].state_dict()
        for k in z.files:
            if k.startswith(pre):
                got = sd[k[len(pre):]].cpu().numpy()
                # Adam's first step moves a weight by lr * g / (|g| + 1e-8): at this batch size (8) some gradients are ~1e-8 and a
                # last-ulp difference becomes a fraction of lr -- bound those by lr / 4 and require them to be rare
                lr = dict(q_ext=float(z["lr_ext"]), q_int=float(z["lr_int"]), emb=float(z["episodic_lr"]), lifelong_train=float(z["lifelong_lr"]))[name]
                np.testing.assert_allclose(got, z[k], rtol=1e-5, atol=lr / 4, err_msg=k)
                assert np.mean(np.abs(got - z[k]) > 5e-6) < 2e-2, k


def test_agent57_trainer_step_on_srlx_lstm_is_reproducible():
    """Two trainer steps from the same state in two fresh runners: every parameter of q_ext and q_int is equal bit for bit.  The input block's convolutions are
    still MIOpen's, whose default weight-gradient solvers add with atomics; the test asks the library for its deterministic ones, so that what is compared is
    the whole update and what could differ is the recurrent layer."""
    import torch

    z = np.load(os.path.join(GOLDEN, "train_step_agent57.npz"))
    after = []
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for _ in range(2):
            runner, rl, param, trainer, nets, rec = _trainer_at_golden(z)
            trainer.train()
            trainer.train()
            assert param.q_ext_online.lstm_path == "srlx" and param.q_int_online.lstm_path == "srlx"
            after.append({name: {k: v.clone() for k, v in nets[name].state_dict().items()} for name in ("q_ext", "q_int")})
    finally:
        torch.backends.cudnn.deterministic = was
    differ = [(name, k) for name in ("q_ext", "q_int") for k, v in after[0][name].items() if not torch.equal(v, after[1][name][k])]
    assert not differ, differ
    for name in ("q_ext", "q_int"):
        assert not torch.equal(after[0][name]["lstm_layer.weight_hh_l0"].cpu(), torch.tensor(z[f"before.{name}.lstm_layer.weight_hh_l0"]))


def test_agent57_runner_end_to_end_on_srlx_lstm():
    """Runner.train + evaluate: the worker's B = 1, T = 1 acting pass and the trainer both go through the kernels."""
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=True, device="cuda:0", ep_len=6, seed=1)
    rl.episodic_memory_capacity = 64
    runner.set_seed(3)
    param = runner.make_parameter()
    _force_srlx(param)
    calls = _record_paths(param)
    st = runner.train(max_train_count=15)
    assert st.train_count == 15
    assert runner.parameter is param
    info = runner.trainer.info
    for key in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        assert np.isfinite(info[key]), key
    assert len(runner.evaluate(max_episodes=2)) == 2
    assert calls and all(c[3] == "srlx" for c in calls), [c for c in calls if c[3] != "srlx"][:5]
    assert any(c[1] == 1 for c in calls), "no acting pass was recorded"
