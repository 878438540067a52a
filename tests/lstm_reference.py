"""Yardstick and plumbing of tests/test_lstm_gpu.py: torch.nn.LSTM in float64 on the CPU with float64 autograd (never the kernels), the same in float32 as the
measure of what float32 arithmetic costs on the same inputs, and thin wrappers that call srlx_lstm_forward / srlx_lstm_backward into sentinel-guarded buffers."""
import math

import torch

SENTINEL = -12345.0
OUT_FWD = ("y", "h_n", "c_n")
OUT_BWD = ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh", "dh0", "dc0")


def make_case(B, T, I, H, saturate, seed):
    """CPU float32 inputs.  Weights: torch's own initialisation of nn.LSTM(I, H) (uniform in +-1/sqrt(H)); `saturate`: the same weights times 4, and inputs
    scaled so that the input projection's pre-activations have a standard deviation of about 3 whatever I and H are (std(x) = 0.75 sqrt(3 H / I): 4 / sqrt(H)
    * sqrt(I / 3) * std(x) = 3), which drives a part of the gates into saturation at every shape (asserted by the test through `saturated_fraction`)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, H, batch_first=True)
    p = {k: getattr(m, k + "_l0").detach().clone() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    xs = 1.0
    if saturate:
        p = {k: v * 4 for k, v in p.items()}
        xs = 0.75 * math.sqrt(3.0 * H / I)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(B=B, T=T, I=I, H=H, x=r(B, T, I) * xs, h0=torch.tanh(r(B, H)), c0=r(B, H), w_ih=p["weight_ih"], w_hh=p["weight_hh"], b_ih=p["bias_ih"],
                b_hh=p["bias_hh"], dy=r(B, T, H), dh_n=r(B, H), dc_n=r(B, H))


def _module(c, dtype):
    m = torch.nn.LSTM(c["I"], c["H"], batch_first=True).to(dtype)
    with torch.no_grad():
        for k, n in (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0")):
            getattr(m, n).copy_(c[k].to(dtype))
    return m


def reference(c, dtype=torch.float64, state_grads=True):
    """nn.LSTM on the CPU in `dtype`: forward outputs and the gradients of sum(y dy) [+ sum(h_n dh_n) + sum(c_n dc_n)]."""
    m = _module(c, dtype)
    x, h0, c0 = (c[k].to(dtype).clone().requires_grad_(True) for k in ("x", "h0", "c0"))
    y, (h_n, c_n) = m(x, (h0.unsqueeze(0), c0.unsqueeze(0)))
    loss = (y * c["dy"].to(dtype)).sum()
    if state_grads:
        loss = loss + (h_n[0] * c["dh_n"].to(dtype)).sum() + (c_n[0] * c["dc_n"].to(dtype)).sum()
    loss.backward()
    return dict(y=y.detach(), h_n=h_n[0].detach(), c_n=c_n[0].detach(), dx=x.grad, dw_ih=m.weight_ih_l0.grad, dw_hh=m.weight_hh_l0.grad, db_ih=m.bias_ih_l0.grad,
                db_hh=m.bias_hh_l0.grad, dh0=h0.grad, dc0=c0.grad)


def saturated_fraction(c, y64):
    """Share of the sigmoid gate activations (i, f, o of every step, row and unit; float64) outside [0.01, 0.99].  Recomputed by hand from the float64
    reference's hidden states, which also checks the gate row order i, f, g, o against nn.LSTM."""
    d = torch.float64
    x, w_ih, w_hh, b = c["x"].to(d), c["w_ih"].to(d), c["w_hh"].to(d), (c["b_ih"] + 0).to(d) + c["b_hh"].to(d)
    H = c["H"]
    h, cell = c["h0"].to(d), c["c0"].to(d)
    acts = []
    for t in range(c["T"]):
        pre = x[:, t] @ w_ih.T + h @ w_hh.T + b
        i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        cell = f * cell + i * g
        h = o * torch.tanh(cell)
        acts += [i, f, o]
    torch.testing.assert_close(h, y64[:, -1], rtol=1e-10, atol=1e-12)
    a = torch.stack(acts)
    return float(((a < 0.01) | (a > 0.99)).double().mean())


# ---- the C ABI into guarded buffers ----------------------------------------------------------------------------------------------------------------------------
def _guarded(dev, rows, cols):
    """[rows + 1][cols] filled with the sentinel: the kernels own the first `rows` rows; the last one must stay as it is."""
    return torch.full((rows + 1, cols), SENTINEL, dtype=torch.float32, device=dev)


def to_device(c, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}


def buffers(N, c, dev):
    B, T, I, H = c["B"], c["T"], c["I"], c["H"]
    lib = N.lib()
    ws, sc = lib.srlx_lstm_workspace_floats(B, T, I, H, 1), lib.srlx_lstm_scratch_floats(B, T, I, H, 1)
    assert ws >= 5 * B * T * H and sc > 0
    return torch.full((ws + 64,), SENTINEL, device=dev), torch.full((sc + 64,), SENTINEL, device=dev), ws, sc


def forward(N, c, dev, workspace, scratch):
    """c: device tensors.  Returns guarded y [B T + 1][H], h_n, c_n [B + 1][H]."""
    B, T, I, H = c["B"], c["T"], c["I"], c["H"]
    out = dict(y=_guarded(dev, B * T, H), h_n=_guarded(dev, B, H), c_n=_guarded(dev, B, H))
    N.check(N.lib().srlx_lstm_forward(B, T, I, H, N.tptr(c["x"]), N.tptr(c["h0"]), N.tptr(c["c0"]), N.tptr(c["w_ih"]), N.tptr(c["w_hh"]), N.tptr(c["b_ih"]),
                                      N.tptr(c["b_hh"]), N.tptr(out["y"]), N.tptr(out["h_n"]), N.tptr(out["c_n"]), N.tptr(workspace), N.tptr(scratch), None))
    torch.cuda.synchronize()
    return out


def backward(N, c, dev, y, workspace, scratch, state_grads=True):
    B, T, I, H = c["B"], c["T"], c["I"], c["H"]
    out = dict(dx=_guarded(dev, B * T, I), dw_ih=_guarded(dev, 4 * H, I), dw_hh=_guarded(dev, 4 * H, H), db_ih=_guarded(dev, 4 * H, 1), db_hh=_guarded(dev, 4 * H, 1),
               dh0=_guarded(dev, B, H), dc0=_guarded(dev, B, H))
    N.check(N.lib().srlx_lstm_backward(B, T, I, H, N.tptr(c["x"]), N.tptr(c["h0"]), N.tptr(c["c0"]), N.tptr(c["w_ih"]), N.tptr(c["w_hh"]), N.tptr(y),
                                       N.tptr(workspace), N.tptr(c["dy"]), N.tptr(c["dh_n"]) if state_grads else None, N.tptr(c["dc_n"]) if state_grads else None,
                                       N.tptr(out["dx"]), N.tptr(out["dw_ih"]), N.tptr(out["dw_hh"]), N.tptr(out["db_ih"]), N.tptr(out["db_hh"]), N.tptr(out["dh0"]),
                                       N.tptr(out["dc0"]), N.tptr(scratch), None))
    torch.cuda.synchronize()
    return out


def check_tensor(name, got, want64, ref32, where):
    """The project's standing tolerance (tests/test_ppo_envelope_gpu.py: rtol 1e-5, atol 1e-5 of the tensor's largest entry) against float64; failing that, a
    tensor may be as far from float64 as twice float32 nn.LSTM on the CPU is on the same inputs -- measured from torch, never from the kernel, and printed."""
    got = got.detach().double().cpu().reshape(want64.shape)
    atol = 1e-5 * float(want64.abs().max())
    try:
        torch.testing.assert_close(got, want64, rtol=1e-5, atol=atol)
        return
    except AssertionError as e:
        err = float((got - want64).abs().max())
        cpu32 = float((ref32.double() - want64).abs().max())
        print("LSTM-ESCAPE %s %s: |kernel - f64| %.3g beyond rtol 1e-5 / atol %.3g; float32 nn.LSTM on the CPU is %.3g from f64; allowed %.3g" % (
            where, name, err, atol, cpu32, 2 * cpu32))
        assert err <= 2 * cpu32, f"{where} {name}: {e}"
