"""libsrlx's LSTM (srlx_lstm_forward / srlx_lstm_backward, csrc/srlx_lstm.hip) against torch.nn.LSTM in float64 on the CPU with float64 autograd.

Shapes are the smallest that can still go wrong.  From the issue: H in {16, 48, 128} (one unit tile, a count that is no power of two, several tiles), B in
{1, 3, 17} (partial and crossed row tiles), T in {1, 2, 7}, I in {1, 5, 37, 260} (K no multiple of the MFMA's K, K across a staging tile).  The tile edges
the kernels as built have, each with a value on either side:
  * step kernels, 16 rows x 16 units per workgroup: B = 15 / 16 / 17 (H is a multiple of 16 by the envelope: H = 16 and 32 are one and two unit tiles);
  * step kernels, K walked in chunks of 16 dealt to four waves (a round is 64): H = 48 (a wave idles), 64 (one full round), 80 (a second round begins); the
    backward step's K is 4 H: H = 16 (64: one round) and 32 (128: two);
  * the GEMM's 128 x 128 x 16 block: M = B T = 128 (16 x 8) / 129 (43 x 3); N = 4 H = 128 (H = 32) / 192 (H = 48); N = I = 128 / 129; N = H = 128 / 144 (dW_hh);
    K = I = 16 / 17; K = B T = 16 (2 x 8) / 17 (1 x 17);
  * the bias gradient's 32 row slices: B T = 32 (4 x 8) / 33 (11 x 3).
The Atari shape (B = 64, T = 121, I = 7777, H = 512: B T I is beyond 2^31) runs once, behind the `slow` marker."""
import pytest
import torch

import lstm_reference as R

pytestmark = pytest.mark.gpu

ISSUE_SHAPES = [  # (B, T, I, H): every value of the issue's four sets, each of H x B, H x I and B x T at least once
    (1, 1, 1, 16), (3, 2, 5, 16), (17, 7, 37, 16), (3, 7, 260, 16),
    (1, 2, 260, 48), (3, 1, 37, 48), (17, 2, 1, 48), (17, 1, 5, 48),
    (1, 7, 5, 128), (3, 7, 1, 128), (17, 7, 260, 128), (3, 2, 37, 128), (17, 1, 260, 16),
]
EDGE_SHAPES = [
    (15, 2, 5, 16), (16, 8, 16, 32), (43, 3, 17, 64), (2, 8, 128, 80), (1, 17, 129, 144), (4, 8, 15, 32), (11, 3, 33, 32),
]
SHAPES = ISSUE_SHAPES + EDGE_SHAPES


def _env():
    from simple_distributed_rl_amd import _native as N

    return N, torch.device("cuda:0")


_cache = {}


def _case(shape, saturate):
    """Inputs and the CPU references of a case, computed once and shared (read-only) by the tests."""
    key = (shape, saturate)
    if key not in _cache:
        B, T, I, H = shape
        c = R.make_case(B, T, I, H, saturate, seed=1000 * H + 100 * B + 10 * T + I + int(saturate))
        _cache[key] = dict(c=c, f64={s: R.reference(c, torch.float64, s) for s in (True, False)}, f32={s: R.reference(c, torch.float32, s) for s in (True, False)})
    return _cache[key]


def _ids(s):
    return "B%d-T%d-I%d-H%d" % s


def _guard_ok(name, t, rows):
    assert bool((t[rows:] == R.SENTINEL).all()), (name, "the row past the end was written")


def _run(shape, saturate):
    N, dev = _env()
    k = _case(shape, saturate)
    c = R.to_device(k["c"], dev)
    B, T, I, H = shape
    where = "%s %s" % (_ids(shape), "x4" if saturate else "init")
    ws, sc, n_ws, n_sc = R.buffers(N, c, dev)
    plain = R.forward(N, c, dev, None, sc)
    train = R.forward(N, c, dev, ws, sc)
    rows = dict(y=B * T, h_n=B, c_n=B)
    for name in R.OUT_FWD:
        assert torch.equal(plain[name], train[name]), (where, name, "with and without a workspace differ")
        _guard_ok(name, train[name], rows[name])
        R.check_tensor(name, train[name][:rows[name]], k["f64"][True][name], k["f32"][True][name], where)
    assert bool((ws[n_ws:] == R.SENTINEL).all()) and bool((sc[n_sc:] == R.SENTINEL).all()), (where, "wrote past the workspace or scratch size it asked for")
    rows = dict(dx=B * T, dw_ih=4 * H, dw_hh=4 * H, db_ih=4 * H, db_hh=4 * H, dh0=B, dc0=B)
    for state_grads in (True, False):
        got = R.backward(N, c, dev, train["y"], ws, sc, state_grads)
        again = R.backward(N, c, dev, train["y"], ws, sc, state_grads)
        for name in R.OUT_BWD:
            assert torch.equal(got[name], again[name]), (where, name, "two backward calls on the same inputs differ")
            _guard_ok(name, got[name], rows[name])
            R.check_tensor(name, got[name][:rows[name]], k["f64"][state_grads][name], k["f32"][state_grads][name], "%s state_grads=%d" % (where, state_grads))
        assert torch.equal(got["db_ih"], got["db_hh"])
        assert bool((ws[n_ws:] == R.SENTINEL).all()) and bool((sc[n_sc:] == R.SENTINEL).all()), (where, "wrote past the workspace or scratch size it asked for")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lstm_matches_float64_torch_init(shape):
    _run(shape, False)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lstm_matches_float64_saturating_weights(shape):
    """The same weights times 4: a part of the gates saturates (more than 1 % and fewer than 50 % of the sigmoid gate activations outside [0.01, 0.99] in the
    float64 helper), where the pointwise derivatives are small differences."""
    k = _case(shape, True)
    frac = R.saturated_fraction(k["c"], k["f64"][True]["y"])
    assert 0.01 < frac < 0.5, frac
    _run(shape, True)


def test_lstm_module_keeps_no_stale_workspace():
    """QNetwork's cached buffers: a pass with gradient at (B = 17, T = 7) followed by one at (B = 3, T = 2) on the same module gives what a fresh module gives,
    bit for bit; and a backward whose workspace a later pass of the same shape has taken refuses instead of using it."""
    import copy

    from test_agent57_cpu import _agent57_runner

    N, dev = _env()
    runner, rl = _agent57_runner(None, intrinsic=True, device="cuda:0")
    rl.lstm_units = 48
    net = runner.make_parameter().q_ext_online.to(dev)
    assert net.lstm_backend in ("srlx", "torch")
    net.lstm_backend = "srlx"
    fresh = copy.deepcopy(net)
    I, H = net.lstm_layer.input_size, 48
    g = torch.Generator().manual_seed(5)

    def one(m, B, T, seed):
        g.manual_seed(seed)
        x = torch.randn(B, T, I, generator=g).to(dev).requires_grad_(True)
        hid = (torch.randn(1, B, H, generator=g).to(dev), torch.randn(1, B, H, generator=g).to(dev))
        dy = torch.randn(B, T, H, generator=g).to(dev)
        m.zero_grad()
        y, (h_n, c_n) = m._lstm(x, hid)
        assert m.lstm_path == "srlx"
        (y * dy).sum().backward()
        return [y.detach(), h_n.detach(), c_n.detach(), x.grad] + [p.grad.clone() for p in m.lstm_layer.parameters()]

    one(net, 17, 7, 1)
    got = one(net, 3, 2, 2)
    want = one(fresh, 3, 2, 2)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    x = torch.randn(3, 2, I, generator=g).to(dev).requires_grad_(True)
    hid = net.get_initial_state(3, dev)
    y1, _ = net._lstm(x, hid)
    y2, _ = net._lstm(x, hid)
    with pytest.raises(RuntimeError, match="workspace"):
        y1.sum().backward()
    y2.sum().backward()


@pytest.mark.slow
def test_lstm_atari_shape():
    """set_atari_config's shape: B = 64, T = 40 + 80 + 1, I = 7744 + 1 + 32, H = 512 (element indices of x and dx pass 2^31)."""
    _run((64, 121, 7777, 512), False)
