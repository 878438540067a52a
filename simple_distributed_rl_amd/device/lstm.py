"""A torch.nn.LSTM's forward and backward through time on libsrlx: `SrlxLstm` reads the module's four parameters per call and owns only the
cached workspace / scratch buffers, so the module stays what holds the parameters (state-dict keys, optimisers, `load_state_dict`)."""
import torch

from simple_distributed_rl_amd import _native as N


class _LstmFunction(torch.autograd.Function):
    """y, h_n, c_n = LSTM(x, (h0, c0)) with the forward AND the backward through time in libsrlx (srlx_lstm_forward / srlx_lstm_backward: float32 matrix-core
    kernels with fixed summation orders, so an update is reproducible run to run).  The four LSTM parameters are inputs only so that autograd routes their
    gradients through `backward`; the kernels read them by address.  `bufs` is the caller's cached workspace / scratch pair of this (B, T)."""

    @staticmethod
    def forward(ctx, bufs, training, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
        B, T, I = x.shape
        H = w_hh.shape[1]
        x, h0, c0 = _dense16(x), _dense16(h0), _dense16(c0)
        y = torch.empty((B, T, H), dtype=torch.float32, device=x.device)
        h_n, c_n = torch.empty_like(h0), torch.empty_like(c0)
        ws = bufs["workspace"] if training else None
        N.check(N.lib().srlx_lstm_forward(B, T, I, H, N.tptr(x), N.tptr(h0), N.tptr(c0), N.tptr(w_ih), N.tptr(w_hh), N.tptr(b_ih), N.tptr(b_hh), N.tptr(y),
                                          N.tptr(h_n), N.tptr(c_n), N.tptr(ws), N.tptr(bufs["scratch"]), N.torch_stream_ptr()))
        if training:
            bufs["serial"] += 1
            ctx.bufs, ctx.serial, ctx.keep = bufs, bufs["serial"], (x, h0, c0, w_ih, w_hh, y)
            ctx.set_materialize_grads(False)
        return y, h_n, c_n

    @staticmethod
    def backward(ctx, dy, dh_n, dc_n):
        bufs = ctx.bufs
        if bufs["serial"] != ctx.serial:
            raise RuntimeError("Agent57 LSTM: another pass with gradient of the same (batch, steps) ran on this module before this one's backward; its workspace is gone")
        x, h0, c0, w_ih, w_hh, y = ctx.keep
        B, T, I = x.shape
        H = w_hh.shape[1]
        dy = torch.zeros_like(y) if dy is None else dy.contiguous()
        dh_n, dc_n = (None if g is None else g.contiguous() for g in (dh_n, dc_n))
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[2] else None
        dh0 = torch.empty_like(h0) if need[3] else None
        dc0 = torch.empty_like(c0) if need[4] else None
        dw_ih, dw_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
        db_ih, db_hh = (torch.empty(4 * H, dtype=torch.float32, device=x.device) for _ in range(2))
        N.check(N.lib().srlx_lstm_backward(B, T, I, H, N.tptr(x), N.tptr(h0), N.tptr(c0), N.tptr(w_ih), N.tptr(w_hh), N.tptr(y), N.tptr(bufs["workspace"]), N.tptr(dy),
                                           N.tptr(dh_n), N.tptr(dc_n), N.tptr(dx), N.tptr(dw_ih), N.tptr(dw_hh), N.tptr(db_ih), N.tptr(db_hh), N.tptr(dh0),
                                           N.tptr(dc0), N.tptr(bufs["scratch"]), N.torch_stream_ptr()))
        ctx._keep_grads = (dy, dh_n, dc_n)  # alive until the stream has run the launches
        return None, None, dx, dh0, dc0, dw_ih, dw_hh, db_ih, db_hh


def _dense16(t):
    """float32, dense and 16-byte aligned (the kernels' vector loads): a view at an odd storage offset is copied."""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class SrlxLstm:
    """The one-layer, batch-first `nn.LSTM` it is called with, run by libsrlx: `lstm(module, x, (h0, c0))` returns what `module(x, (h0, c0))` returns, and is
    differentiable with respect to x, h0, c0 and the module's four parameters.  Inside libsrlx's envelope only (srlx.h: B, T <= 256, I <= 16384, H a multiple
    of 16 up to 512): ask `serves` first."""

    def __init__(self):
        self._bufs = {}  # (device, B, T) -> workspace / scratch of that shape, allocated once

    @staticmethod
    def serves(module, x) -> bool:
        w = module.weight_ih_l0
        if not (x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32):
            return False  # (answered before libsrlx is loaded)
        B, T, I = x.shape
        return N.lib().srlx_lstm_scratch_floats(B, T, I, module.hidden_size, 1) >= 0

    def __call__(self, module, x, hidden_states):
        B, T, I = x.shape
        H = module.hidden_size
        key = (x.device, B, T)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = dict(workspace=None, serial=0,
                                          scratch=torch.empty(N.lib().srlx_lstm_scratch_floats(B, T, I, H, 1), dtype=torch.float32, device=x.device))
        h0, c0 = hidden_states[0][0], hidden_states[1][0]
        params = (module.weight_ih_l0, module.weight_hh_l0, module.bias_ih_l0, module.bias_hh_l0)
        training = torch.is_grad_enabled() and any(t.requires_grad for t in (x, h0, c0) + params)
        if training and bufs["workspace"] is None:  # a layer that is only called under no_grad never allocates one
            bufs["workspace"] = torch.empty(N.lib().srlx_lstm_workspace_floats(B, T, I, H, 1), dtype=torch.float32, device=x.device)
        y, h_n, c_n = _LstmFunction.apply(bufs, training, x, h0, c0, *params)
        return y, (h_n.unsqueeze(0), c_n.unsqueeze(0))
