"""libsrlx's LSTM entry points without a GPU: the size functions and the envelope are host arithmetic, a call outside the envelope is refused before any
device call, and Agent57's QNetwork on CPU parameters is torch.nn.LSTM itself."""
import numpy as np
import torch

OK_SHAPE = dict(B=8, T=5, I=37, H=48)
BAD = [dict(H=h) for h in (0, 8, 24, 528)] + [dict(I=i) for i in (0, 16385)] + [dict(B=b) for b in (0, 257)] + [dict(T=t) for t in (0, 257)]


def _args(d):
    return d["B"], d["T"], d["I"], d["H"]


def test_lstm_size_functions_are_host_arithmetic():
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    for shape in (OK_SHAPE, dict(B=1, T=1, I=1, H=16), dict(B=256, T=256, I=16384, H=512), dict(B=64, T=121, I=7777, H=512)):
        B, T, I, H = _args(shape)
        assert lib.srlx_lstm_workspace_floats(B, T, I, H, 1) >= 5 * B * T * H
        assert lib.srlx_lstm_workspace_floats(B, T, I, H, 0) >= 0  # a pass without gradient keeps nothing
        for training in (0, 1):
            assert lib.srlx_lstm_scratch_floats(B, T, I, H, training) > 0
    for change in BAD:
        B, T, I, H = _args(dict(OK_SHAPE, **change))
        for training in (0, 1):
            assert lib.srlx_lstm_workspace_floats(B, T, I, H, training) == -1, change
            assert lib.srlx_lstm_scratch_floats(B, T, I, H, training) == -1, change


def test_lstm_forward_refuses_shapes_outside_the_envelope_before_any_device_call():
    """The pointers are host memory of the right sizes: had the call gone on to a launch, it would not have returned a status for the shape."""
    from simple_distributed_rl_amd import _native as N

    lib = N.lib()
    for change in BAD:
        B, T, I, H = _args(dict(OK_SHAPE, **change))
        bufs = [np.zeros(max(1, n), np.float32) for n in (B * T * I, B * H, B * H, 4 * H * I, 4 * H * H, 4 * H, 4 * H, B * T * H, B * H, B * H, 1, 1)]
        st = lib.srlx_lstm_forward(B, T, I, H, *[N.np_ptr(b) for b in bufs[:10]], None, N.np_ptr(bufs[11]), None)
        assert st != 0, change
        assert b"lstm" in lib.srlx_last_error(), change
        st = lib.srlx_lstm_backward(B, T, I, H, *([N.np_ptr(bufs[0])] * 18), None)
        assert st != 0 and b"lstm" in lib.srlx_last_error(), change


def test_agent57_qnetwork_on_cpu_is_nn_lstm(monkeypatch):
    from simple_distributed_rl_amd import _native as N
    from simple_distributed_rl_amd.device.lstm import SrlxLstm
    from test_agent57_cpu import _agent57_runner

    runner, rl = _agent57_runner(None, intrinsic=True)
    net = runner.make_parameter().q_ext_online
    assert net.lstm_backend in ("srlx", "torch")
    assert sorted(k for k in net.state_dict() if k.startswith("lstm_layer.")) == ["lstm_layer.bias_hh_l0", "lstm_layer.bias_ih_l0", "lstm_layer.weight_hh_l0",
                                                                                  "lstm_layer.weight_ih_l0"]
    g = torch.Generator().manual_seed(0)
    B, S = 3, 4
    obs = tuple(rl.observation_space.shape)
    inputs = [torch.rand((B, S) + obs, generator=g), torch.randn(B, S, 1, generator=g), torch.randn(B, S, 1, generator=g),
              torch.eye(rl.action_space.n)[torch.randint(0, rl.action_space.n, (B, S), generator=g)], torch.eye(rl.actor_num)[torch.zeros(B, S, dtype=torch.long)]]
    hid = (torch.randn(1, B, net.hidden_size, generator=g), torch.randn(1, B, net.hidden_size, generator=g))
    def no_lib():
        raise AssertionError("a CPU call reached libsrlx")

    x_cpu = torch.randn(B, S, net.lstm_layer.input_size, generator=g)
    with monkeypatch.context() as mp:  # SrlxLstm answers for CPU tensors before any call into libsrlx, let alone a device call
        mp.setattr(N, "lib", no_lib)
        assert SrlxLstm().serves(net.lstm_layer, x_cpu) is False
        assert SrlxLstm.serves(net.lstm_layer, x_cpu.double()) is False
    for backend in ("srlx", "torch"):
        net.lstm_backend = backend
        with torch.no_grad():
            q, (h_n, c_n) = net(inputs, hid)
            assert net.lstm_path == "torch"
            x = torch.cat([net.in_block(inputs[0].reshape((B * S,) + obs)).view(B, S, -1)] + [p for p, on in ((inputs[1], net.input_ext_reward),
                          (inputs[2], net.input_int_reward), (inputs[3], net.input_action)) if on] + [inputs[4]], dim=2)
            y, (h_w, c_w) = net.lstm_layer(x, hid)
            want = net.hidden_block(y.reshape(B * S, -1)).view(B, S, -1)
        assert torch.equal(q, want) and torch.equal(h_n, h_w) and torch.equal(c_n, c_w)
