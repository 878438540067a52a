"""NoT_SAC's update on libsrlx (csrc/srlx_notsac.hip): `NotSacUpdate` binds an `algorithms.sac_not.Parameter`'s own tensors by address -- the two
networks stay what the plugin, checkpoints and `load_state_dict` see -- and owns the handle, the gradient tensors the kernels write (before and after each
network's norm clip) and the Adam state (moments here, the step count in the handle).  One `update` is the whole of torch_model.py:150-189 for one batch and one
noise tensor, in six launches."""
import ctypes
import math

import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd._native import _int_array, _linear_widths, _ptrs

MAX_BATCH = 256
# block options the kernels' layers cover; anything else set on a block keeps the update on torch
_MLP_FREE_KWARGS = {"layer_sizes", "activation", "kernel_initializer", "bias_initializer"}


def shape_of(parameter):
    """(D, head, n_out, policy widths, q widths, act_emb_units) of a sac_not.Parameter, or a sentence saying why its networks are not ones the kernels run."""
    policy, qnet = parameter.policy, parameter.qnet
    for net in (policy, qnet):
        if not hasattr(net.in_block, "hidden_layers"):
            return "the input_block is an image block (the kernels start at a flat observation)"
        if _linear_widths(net.in_block) != ():
            return "the input_block has layers of its own (the Q-network concatenates behind it: the kernels concatenate behind the observation)"
    pw, qw = _linear_widths(policy.policy_block), _linear_widths(qnet.q_block)
    if pw is None:
        return "the policy_block is not a chain of Linear (with bias) + ReLU layers"
    if qw is None:
        return "the q_block is not a chain of Linear (with bias) + ReLU layers"
    if not pw or not qw:
        return "the policy_block or the q_block has no layer"
    act = qnet.act_block[0]
    D = [m for m in policy.policy_block.hidden_layers if isinstance(m, torch.nn.Linear)][0].in_features
    dist = policy.policy_dist_block
    if hasattr(dist, "loc_layers"):
        if len(dist.h_layers) or len(dist.loc_layers) != 1 or len(dist.log_scale_layers) != 1:
            return "the Normal head has hidden layers of its own"
        head, n_out = 1, dist.loc_layers[0].out_features
    else:
        if len(dist.h_layers) != 1:
            return "the Gumbel head has hidden layers of its own"
        head, n_out = 0, dist.h_layers[0].out_features
    return D, head, n_out, pw, qw, act.out_features


def log_scale_range(parameter):
    """The Normal head's clamp as the kernels take it: (lo, hi), infinite when there is none."""
    dist = parameter.policy.policy_dist_block
    if getattr(dist, "enable_stable_gradients", False):
        return float(dist.stable_gradients_scale_range[0]), float(dist.stable_gradients_scale_range[1])
    return -math.inf, math.inf


class NotSacUpdate:
    def __init__(self, parameter, max_batch: int = MAX_BATCH, betas=(0.9, 0.999), eps: float = 1e-8):
        reason = self.why_not(parameter, max_batch)
        if reason:
            raise ValueError(f"NotSacUpdate: {reason}")
        self.parameter = parameter
        self.D, self.head, self.n_out, self.policy_widths, self.q_widths, self.act_emb = shape_of(parameter)
        self.max_batch = max_batch
        self.policy_params, self.q_params = list(parameter.policy.parameters()), list(parameter.qnet.parameters())
        self.params = self.policy_params + self.q_params  # the order of srlx_notsac_bind
        self.device = self.params[0].device
        self.betas, self.eps = betas, eps
        self.ls_lo, self.ls_hi = log_scale_range(parameter)
        self._lib = N.lib()
        self._h = N.c_p()
        N.check(self._lib.srlx_notsac_create(ctypes.byref(self._h), self.D, self.head, self.n_out, len(self.policy_widths), _int_array(self.policy_widths),
                                             len(self.q_widths), _int_array(self.q_widths), self.act_emb, max_batch, self.device.index or 0))
        self.grads = [torch.zeros_like(p) for p in self.params]      # after the norm clips: what Adam reads
        self.raw_grads = [torch.zeros_like(p) for p in self.params]  # before them
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        n = len(self.params)
        N.check(self._lib.srlx_notsac_bind(self._h, n, _ptrs(self.params)))
        N.check(self._lib.srlx_notsac_bind_grads(self._h, n, _ptrs(self.grads), _ptrs(self.raw_grads)))
        N.check(self._lib.srlx_notsac_bind_adam(self._h, n, _ptrs(self.exp_avg), _ptrs(self.exp_avg_sq), 0, betas[0], betas[1], eps))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.srlx_notsac_destroy(self._h)
            self._h = None

    def split(self, tensors):
        """(the policy's, the Q-network's) of a list in bind order."""
        return tensors[:len(self.policy_params)], tensors[len(self.policy_params):]

    # ---- what it serves ---------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def why_not(parameter, batch: int = 1, config=None) -> str:
        """'' when libsrlx runs this Parameter's update at this batch size, otherwise the reason it does not."""
        tensors = list(parameter.policy.parameters()) + list(parameter.qnet.parameters())
        if not all(t.is_cuda for t in tensors):
            return "the parameters are CPU tensors"  # (answered before libsrlx is loaded)
        if not all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
            return "a parameter is not a dense float32 tensor"
        if config is not None:
            reasons = NotSacUpdate.config_reasons(config)
            if reasons:
                return reasons[0]
        shape = shape_of(parameter)
        if isinstance(shape, str):
            return shape
        return NotSacUpdate.envelope_reason(*shape, batch)

    @staticmethod
    def config_reasons(config) -> list:
        """What `why_not` refuses on the config alone, every sentence (no Parameter, no device)."""
        why = []
        for name in ("policy_block", "q_block"):
            extra = set(getattr(config, name).kwargs) - _MLP_FREE_KWARGS
            if extra:
                why.append(f"the {name} sets {sorted(extra)} (the kernels' layers are Linear with bias + ReLU)")
        extra = set(config.input_block.value.kwargs) - _MLP_FREE_KWARGS
        if extra:
            why.append(f"the input_block sets {sorted(extra)} (the kernels start at the observation)")
        if tuple(config.input_block.value.kwargs.get("layer_sizes", ())) != ():
            why.append("the input_block has layers of its own (the Q-network concatenates behind it: the kernels concatenate behind the observation)")
        if not config.target_policy_temperature > 0:
            why.append(f"target_policy_temperature {config.target_policy_temperature} is not positive (the kernel's argmax assumes a temperature that keeps the order)")
        sch = config.lr_scheduler
        if sch.schedule_type not in ("", "step", "exp", "cosine", "piecewise"):
            why.append(f"the lr schedule {sch.schedule_type!r} is not one the host evaluates per step")
        return why

    @staticmethod
    def envelope_reason(D, head, n_out, pw, qw, act_emb, batch: int = 1) -> str:
        """The envelope of srlx_notsac_create as a sentence ('' inside it).  Host arithmetic: no device needed."""
        if batch > MAX_BATCH:
            return f"batch size {batch} above max_batch {MAX_BATCH}"
        if N.lib().srlx_notsac_scratch_floats(D, head, n_out, len(pw), _int_array(pw), len(qw), _int_array(qw), act_emb, max(1, batch)) < 0:
            return ("outside the envelope (D 1..256, policy and q block 1..3 layers of 32..512 units in multiples of 32, act_emb_units 32..512 in multiples of 32 "
                    f"with D + act_emb_units <= 512, 2..16 actions or 1..8 action elements): D {D}, {'Normal' if head else 'Gumbel'} {n_out}, policy {tuple(pw)}, "
                    f"q {tuple(qw)}, act_emb_units {act_emb}")
        return ""

    @classmethod
    def serves(cls, parameter, batch: int = 1, config=None) -> bool:
        return cls.why_not(parameter, batch, config) == ""

    # ---- the calls --------------------------------------------------------------------------------------------------------------------------------------
    def steps(self) -> int:
        """Optimiser steps taken (by each of the two optimisers)."""
        return int(self._lib.srlx_notsac_steps(self._h))

    def set_rows_per_workgroup(self, rows: int = 0) -> None:
        """The row kernels' launch shape: 1, 2, 4, 8 or 16 rows per workgroup, 0 for the default (one row per workgroup for every update).  Never changes a bit."""
        N.check(self._lib.srlx_notsac_set_rows_per_workgroup(self._h, int(rows)))

    def update(self, state, next_state, action, reward, not_terminated, total_reward, noise, lr, discount, loss_align_coeff, max_grad_norm, squashed: bool) -> dict:
        """state / next_state f32 [B][D]; action i32 [B] (Gumbel: the index of the stored one-hot's maximum) or f32 [B][K] (Normal); reward, not_terminated,
        total_reward f32 [B]; noise f32 [2][B][n_out]; all on the device.  Returns q, target_q [B], next_action, pi_action [B][n_out] and `scalars` [5] (loss_q,
        loss_q_align, loss_policy, the Q-network's and the policy's gradient norm before their clips), device tensors; nothing synchronises."""
        B = state.shape[0]
        if B > self.max_batch:
            raise ValueError(f"NotSacUpdate: batch size {B} above max_batch {self.max_batch}")
        keep = [t.contiguous() for t in (state, next_state, action, reward, not_terminated, total_reward, noise)]
        assert keep[2].dtype == (torch.float32 if self.head else torch.int32) and all(t.dtype == torch.float32 for t in keep[:2] + keep[3:])
        assert keep[0].numel() == B * self.D and keep[1].numel() == B * self.D and keep[2].numel() == (B * self.n_out if self.head else B)
        assert all(t.numel() == B for t in keep[3:6]) and tuple(keep[6].shape) == (2, B, self.n_out)
        f = dict(dtype=torch.float32, device=self.device)
        out = {"q": torch.empty(B, **f), "target_q": torch.empty(B, **f), "next_action": torch.empty((B, self.n_out), **f),
               "pi_action": torch.empty((B, self.n_out), **f), "scalars": torch.empty(5, **f)}
        N.check(self._lib.srlx_notsac_update(self._h, B, *[N.tptr(t) for t in keep], float(lr), float(discount), float(loss_align_coeff), float(max_grad_norm),
                                             int(bool(squashed)), self.ls_lo, self.ls_hi, N.tptr(out["q"]), N.tptr(out["target_q"]), N.tptr(out["next_action"]),
                                             N.tptr(out["pi_action"]), N.tptr(out["scalars"]), N.torch_stream_ptr()))
        self._keep = keep
        return out

    def forward(self, state, action=None, want_head: bool = True):
        """The head's outputs of n rows -- logits [n][A], or (locs, clamped log-scales) [n][K] each -- and q(s, action) [n] for `action` f32 [n][n_out]; None
        for what is not wanted."""
        x = state.contiguous()
        n = x.shape[0]
        f = dict(dtype=torch.float32, device=self.device)
        h0 = torch.empty((n, self.n_out), **f) if want_head else None
        h1 = torch.empty((n, self.n_out), **f) if want_head and self.head else None
        a = action.contiguous() if action is not None else None
        q = torch.empty(n, **f) if a is not None else None
        N.check(self._lib.srlx_notsac_forward(self._h, n, N.tptr(x), self.ls_lo, self.ls_hi, N.tptr(h0), N.tptr(h1), N.tptr(a), N.tptr(q), N.torch_stream_ptr()))
        self._keep_fwd = (x, a)
        return (h0 if not self.head else (h0, h1)) if want_head else None, q
