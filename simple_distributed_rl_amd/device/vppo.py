"""V-PPO's update on libsrlx (csrc/srlx_vppo.hip): `VppoUpdate` binds an `algorithms.ppo_v.Parameter`'s own tensors by address -- the network
stays what the plugin, checkpoints and `load_state_dict` see -- and owns the handle, the gradient tensors the kernels write (before and after the norm clip)
and the Adam state (moments here, the step count in the handle).  One `update` is the whole of torch_model.py:132-176 for one batch, in three launches."""
import ctypes

import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd._native import _int_array, _linear_widths, _ptrs
from simple_distributed_rl_amd.device import _row_update as R
from simple_distributed_rl_amd.device._row_update import MAX_BATCH


def shape_of(parameter):
    """(D, head, n_out, trunk widths, value widths, policy widths) of a ppo_v.Parameter, or a sentence saying why its network is not one the kernels run."""
    net = parameter.net
    if not hasattr(net.in_block, "hidden_layers"):
        return "the input_block is an image block (the kernels start at a flat observation)"
    widths = []
    for name in ("in_block", "hidden_block", "value_block", "policy_block"):
        w = _linear_widths(getattr(net, name))
        if w is None:
            return f"the {name} is not a chain of Linear (with bias) + ReLU layers"
        widths.append(w)
    first = [m for m in list(net.in_block.hidden_layers) + list(net.hidden_block.hidden_layers) if isinstance(m, torch.nn.Linear)]
    if not first:
        return "the trunk (input_block + hidden_block) has no layer"
    D = first[0].in_features
    head = R.head_of(net.policy_dist_block, "categorical")
    if isinstance(head, str):
        return head
    return D, head[0], head[1], widths[0] + widths[1], widths[2], widths[3]


def log_scale_range(parameter):
    """The Normal head's clamp as the kernels take it: (lo, hi), infinite when there is none."""
    return R.log_scale_range(parameter.net.policy_dist_block)


class VppoUpdate(R.RowUpdate):
    ABI = "vppo"
    shape_of = staticmethod(shape_of)

    @staticmethod
    def tensors_of(parameter) -> list:
        return list(parameter.net.parameters())

    def __init__(self, parameter, max_batch: int = MAX_BATCH, betas=(0.9, 0.999), eps: float = 1e-8):
        self.D, self.head, self.n_out, self.trunk_widths, self.value_widths, self.policy_widths = self._open(parameter, max_batch, betas, eps)
        self.K = self.n_out if self.head else 1
        self.ls_lo, self.ls_hi = log_scale_range(parameter)
        N.check(self._lib.srlx_vppo_create(ctypes.byref(self._h), self.D, self.head, self.n_out, len(self.trunk_widths), _int_array(self.trunk_widths),
                                           len(self.value_widths), _int_array(self.value_widths), len(self.policy_widths), _int_array(self.policy_widths),
                                           max_batch, self.device.index or 0))
        self._alloc()
        N.check(self._lib.srlx_vppo_bind(self._h, _ptrs(self.params)))
        N.check(self._lib.srlx_vppo_bind_grads(self._h, _ptrs(self.grads), _ptrs(self.raw_grads)))
        N.check(self._lib.srlx_vppo_bind_adam(self._h, _ptrs(self.exp_avg), _ptrs(self.exp_avg_sq), 0, betas[0], betas[1], eps))

    # ---- what it serves (`why_not` and `serves`: RowUpdate) ------------------------------------------------------------------------------------------------
    @staticmethod
    def config_reasons(config) -> list:
        """What `why_not` refuses on the config alone, every sentence (no Parameter, no device)."""
        blocks = R.block_kwarg_reasons(config, ("hidden_block", "value_block", "policy_block"), "the kernels' layers are Linear with bias + ReLU")
        return blocks + R.lr_schedule_reason(config)

    @staticmethod
    def envelope_reason(D, head, n_out, tw, vw, pw, batch: int = 1) -> str:
        """The envelope of srlx_vppo_create as a sentence ('' inside it).  Host arithmetic: no device needed."""
        if batch > MAX_BATCH:
            return f"batch size {batch} above max_batch {MAX_BATCH}"
        if N.lib().srlx_vppo_scratch_floats(D, head, n_out, len(tw), _int_array(tw), len(vw), _int_array(vw), len(pw), _int_array(pw), max(1, batch)) < 0:
            return ("outside the envelope (D 1..256, trunk 1..3 layers, value and policy block 0..2 layers of 32..512 units in multiples of 32, 2..16 actions or "
                    f"1..8 action elements): D {D}, {'Normal' if head else 'categorical'} {n_out}, trunk {tuple(tw)}, value {tuple(vw)}, policy {tuple(pw)}")
        return ""

    # ---- the calls (`steps`: RowUpdate) --------------------------------------------------------------------------------------------------------------------
    def update(self, state, next_state, action, old_logpi, reward, not_terminated, total_reward, lr, discount, clip_range, entropy_weight, loss_align_coeff,
               max_grad_norm, squashed: bool) -> dict:
        """state / next_state f32 [B][D]; action i32 [B] (categorical) or f32 [B][K] (Normal); old_logpi f32 [B][K]; reward, not_terminated, total_reward f32 [B];
        all on the device.  Returns v, n_v [B], new_logpi [B][K] and `scalars` [5] (loss_value, loss_v_align, loss_policy, loss_e, the gradient norm before the
        clip), device tensors; nothing synchronises."""
        B = state.shape[0]
        if B > self.max_batch:
            raise ValueError(f"VppoUpdate: batch size {B} above max_batch {self.max_batch}")
        keep = [t.contiguous() for t in (state, next_state, action, old_logpi, reward, not_terminated, total_reward)]
        assert keep[2].dtype == (torch.float32 if self.head else torch.int32) and all(t.dtype == torch.float32 for t in keep[:2] + keep[3:])
        assert keep[0].numel() == B * self.D and keep[1].numel() == B * self.D and keep[2].numel() == B * self.K and keep[3].numel() == B * self.K
        assert all(t.numel() == B for t in keep[4:])
        out = {"v": torch.empty(B, dtype=torch.float32, device=self.device), "n_v": torch.empty(B, dtype=torch.float32, device=self.device),
               "new_logpi": torch.empty((B, self.K), dtype=torch.float32, device=self.device), "scalars": torch.empty(5, dtype=torch.float32, device=self.device)}
        N.check(self._lib.srlx_vppo_update(self._h, B, *[N.tptr(t) for t in keep], float(lr), float(discount), float(clip_range), float(entropy_weight),
                                           float(loss_align_coeff), float(max_grad_norm), int(bool(squashed)), self.ls_lo, self.ls_hi, N.tptr(out["v"]),
                                           N.tptr(out["n_v"]), N.tptr(out["new_logpi"]), N.tptr(out["scalars"]), N.torch_stream_ptr()))
        self._keep = keep
        return out

    def forward(self, state, want_v: bool = True, want_head: bool = True):
        """v [n] and the head's outputs of n rows: logits [n][A], or (locs, clamped log-scales) [n][k] each; None for what is not wanted."""
        x = state.contiguous()
        n = x.shape[0]
        v = torch.empty(n, dtype=torch.float32, device=self.device) if want_v else None
        h0 = torch.empty((n, self.n_out), dtype=torch.float32, device=self.device) if want_head else None
        h1 = torch.empty((n, self.n_out), dtype=torch.float32, device=self.device) if want_head and self.head else None
        N.check(self._lib.srlx_vppo_forward(self._h, n, N.tptr(x), self.ls_lo, self.ls_hi, N.tptr(v), N.tptr(h0), N.tptr(h1), N.torch_stream_ptr()))
        self._keep_fwd = x
        return v, (h0 if not self.head else (h0, h1))

    def act(self, n_rows: int, obs, seed: int, counter, epsilon: float, actions, logp, logits=None, cdf=None) -> None:
        """srlx_vppo_act: the Worker's policy() for `n_rows` dense rows [n_rows][D] (a tensor or a device address) in one launch, on the
        categorical head.  `counter` is a device int64 the call reads; `actions` int32 [n_rows] and `logp` float32 [n_rows] receive the result, `logits`
        float32 [n_rows][A] and `cdf` float64 [n_rows][A] when given.  Nothing synchronises."""
        rows = obs if isinstance(obs, ctypes.c_void_p) else N.tptr(obs)
        N.check(self._lib.srlx_vppo_act(self._h, n_rows, rows, ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), N.tptr(counter), float(epsilon), N.tptr(actions),
                                        N.tptr(logp), N.tptr(logits), N.tptr(cdf), N.torch_stream_ptr()))

    def act_normal(self, n_rows: int, obs, seed: int, counter, epsilon: float, noise_scale: float, squashed: bool, low, high, actions, logp, env_actions, loc=None,
                   log_scale=None, z=None) -> None:
        """srlx_vppo_act_normal: the Worker's policy() for `n_rows` dense rows [n_rows][D] (a tensor or a device address) in one launch, on the
        Normal head.  `counter` is a device int64 the call reads; `low` / `high` float32 [K] are the action space's bounds on the device; `actions` (before tanh),
        `logp` and `env_actions` float32 [n_rows][K] receive the result, `loc` / `log_scale` float32 and `z` float64 [n_rows][K] when given.  The log-scale clamp
        is the Parameter's own.  Nothing synchronises."""
        rows = obs if isinstance(obs, ctypes.c_void_p) else N.tptr(obs)
        N.check(self._lib.srlx_vppo_act_normal(self._h, n_rows, rows, ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), N.tptr(counter), float(epsilon), float(noise_scale),
                                               int(bool(squashed)), self.ls_lo, self.ls_hi, N.tptr(low), N.tptr(high), N.tptr(actions), N.tptr(logp),
                                               N.tptr(env_actions), N.tptr(loc), N.tptr(log_scale), N.tptr(z), N.torch_stream_ptr()))
