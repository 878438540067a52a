"""NoT_SAC's update on libsrlx (csrc/srlx_notsac.hip): `NotSacUpdate` binds an `algorithms.sac_not.Parameter`'s own tensors by address -- the two
networks stay what the plugin, checkpoints and `load_state_dict` see -- and owns the handle, the gradient tensors the kernels write (before and after each
network's norm clip) and the Adam state (moments here, the step count in the handle).  One `update` is the whole of torch_model.py:150-189 for one batch and one
noise tensor, in six launches."""
import ctypes

import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd._native import _int_array, _linear_widths, _ptrs
from simple_distributed_rl_amd.device import _row_update as R
from simple_distributed_rl_amd.device._row_update import MAX_BATCH


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
    head = R.head_of(policy.policy_dist_block, "Gumbel")
    if isinstance(head, str):
        return head
    return D, head[0], head[1], pw, qw, act.out_features


def log_scale_range(parameter):
    """The Normal head's clamp as the kernels take it: (lo, hi), infinite when there is none."""
    return R.log_scale_range(parameter.policy.policy_dist_block)


class NotSacUpdate(R.RowUpdate):
    ABI = "notsac"
    shape_of = staticmethod(shape_of)

    @staticmethod
    def tensors_of(parameter) -> list:
        """The policy's tensors, then the Q-network's: the order of srlx_notsac_bind."""
        return list(parameter.policy.parameters()) + list(parameter.qnet.parameters())

    def __init__(self, parameter, max_batch: int = MAX_BATCH, betas=(0.9, 0.999), eps: float = 1e-8):
        self.D, self.head, self.n_out, self.policy_widths, self.q_widths, self.act_emb = self._open(parameter, max_batch, betas, eps)
        n_policy = len(list(parameter.policy.parameters()))
        self.policy_params, self.q_params = self.params[:n_policy], self.params[n_policy:]
        self.ls_lo, self.ls_hi = log_scale_range(parameter)
        N.check(self._lib.srlx_notsac_create(ctypes.byref(self._h), self.D, self.head, self.n_out, len(self.policy_widths), _int_array(self.policy_widths),
                                             len(self.q_widths), _int_array(self.q_widths), self.act_emb, max_batch, self.device.index or 0))
        self._alloc()
        n = len(self.params)
        N.check(self._lib.srlx_notsac_bind(self._h, n, _ptrs(self.params)))
        N.check(self._lib.srlx_notsac_bind_grads(self._h, n, _ptrs(self.grads), _ptrs(self.raw_grads)))
        N.check(self._lib.srlx_notsac_bind_adam(self._h, n, _ptrs(self.exp_avg), _ptrs(self.exp_avg_sq), 0, betas[0], betas[1], eps))

    def split(self, tensors):
        """(the policy's, the Q-network's) of a list in bind order."""
        return tensors[:len(self.policy_params)], tensors[len(self.policy_params):]

    # ---- what it serves (`why_not` and `serves`: RowUpdate) ------------------------------------------------------------------------------------------------
    @staticmethod
    def config_reasons(config) -> list:
        """What `why_not` refuses on the config alone, every sentence (no Parameter, no device)."""
        why = R.block_kwarg_reasons(config, ("policy_block", "q_block"), "the kernels start at the observation")
        if tuple(config.input_block.value.kwargs.get("layer_sizes", ())) != ():
            why.append("the input_block has layers of its own (the Q-network concatenates behind it: the kernels concatenate behind the observation)")
        if not config.target_policy_temperature > 0:
            why.append(f"target_policy_temperature {config.target_policy_temperature} is not positive (the kernel's argmax assumes a temperature that keeps the order)")
        return why + R.lr_schedule_reason(config)

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

    # ---- the calls (`steps`: RowUpdate) --------------------------------------------------------------------------------------------------------------------
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
