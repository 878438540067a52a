"""The host side of Agent57's image block in libsrlx that needs no GPU: the byte query's envelope (host arithmetic), and `QNetwork.in_block_backend`'s refusals."""
import numpy as np
import pytest


def _bytes(H, C, rows):
    """What srlx_qnet_enable_seq_training allocates (srlx.h): three activation gradients, the padded data gradient, two transposed filters, 256 weight parts."""
    oh1 = (H - 2) // 4 + 1
    oh2 = oh1 // 2 + 1
    q = (oh1 + 5) // 2
    floats = rows * oh2 * oh2 * 64 * 2 + rows * oh1 * oh1 * 32 + rows * max(4 * q * q * 32, (oh2 + 2) ** 2 * 64) + 128 * 64
    floats += 64 * 9 * 64 + 64 * 16 * 32 + 256 * (max(64 * 9 * 64, 32 * C * 64) + 64)
    return 4 * floats


def test_seq_training_bytes_envelope():
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    for H in range(8, 88, 4):
        for C in (1, 2, 3, 4):
            for rows in (1, 64, 5184, 8192, 65536):
                assert lib.srlx_qnet_seq_training_bytes(H, H, C, 32, rows) == _bytes(H, C, rows), (H, C, rows)
    assert lib.srlx_qnet_seq_training_bytes(84, 84, 1, 32, 5184) < 2 * 1024 ** 3  # the Atari step pass: under 2 GiB a network
    ok = dict(h=84, w=84, c=1, f=32, rows=8192)
    for change in (dict(h=4, w=4), dict(h=88, w=88), dict(h=82, w=82), dict(w=80), dict(c=0), dict(c=5), dict(f=64), dict(f=16), dict(rows=0), dict(rows=65537)):
        a = dict(ok, **change)
        assert lib.srlx_qnet_seq_training_bytes(a["h"], a["w"], a["c"], a["f"], a["rows"]) == -1, change


def _network():
    from simple_distributed_rl_amd.algorithms import agent57
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=False)
    runner.make_parameter()
    return agent57, runner.parameter.q_ext_online, rl


def _inputs(rl, B=2, S=3, A=4):
    import torch

    return [torch.rand((B, S, 8, 8, 1)), torch.zeros((B, S, 1)), torch.zeros((B, S, 1)), torch.zeros((B, S, A)), torch.eye(rl.actor_num)[:1].expand(B, S, rl.actor_num)]


def test_in_block_backend_on_cpu_runs_torch_and_says_why():
    import torch

    agent57, net, rl = _network()
    assert agent57.QNetwork.in_block_backend == "torch" and net.in_block_path is None
    x = _inputs(rl)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    strides = {k: v.stride() for k, v in net.state_dict().items()}
    with torch.no_grad():
        q0, _ = net(x, net.get_initial_state(2, "cpu"))
    assert net.in_block_path == "torch" and net.why_not_srlx_in_block is None
    net.in_block_backend = "srlx"
    with torch.no_grad():
        q1, _ = net(x, net.get_initial_state(2, "cpu"))
    assert net.in_block_path == "torch" and "GPU" in net.why_not_srlx_in_block
    assert torch.equal(q0, q1)
    after = net.state_dict()
    assert list(after) == list(before)
    for k, v in after.items():  # a refused request changes neither a value nor a memory layout
        assert torch.equal(v, before[k]) and v.stride() == strides[k], k


def test_bad_in_block_backend_raises():
    agent57, net, rl = _network()
    net.in_block_backend = "miopen"
    with pytest.raises(ValueError, match="in_block_backend"):
        net(_inputs(rl), net.get_initial_state(2, "cpu"))
