"""Discrete SAC's update on libsrlx (csrc/srlx_sacd.hip): `SacdUpdate` binds an `algorithms.sac.Parameter`'s own tensors by address -- the
five networks and `log_alpha` stay what the plugin, checkpoints and `load_state_dict` see -- and owns the handle, the gradient tensors the kernels write and
the Adam state (moments here, step counts in the handle).  One `update` is the whole of sac_tf_discrete.py:158-243 for one batch, in five launches."""
import ctypes

import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd._native import _int_array, _linear_widths, _ptrs
from simple_distributed_rl_amd.device._row_update import MAX_BATCH, LibUpdate, tensor_reason

TRAINED = ("policy", "q1_online", "q2_online")
NETWORKS = ("policy", "q1_online", "q1_target", "q2_online", "q2_target")


def shape_of(parameter):
    """(D, A, policy widths, q widths) of a sac.Parameter, or a sentence saying why its networks are not ones the kernels run."""
    pol, q = parameter.policy, parameter.q1_online
    for name, net in (("policy", pol), ("q", q)):
        w = _linear_widths(net.in_block)
        if w is None or len(w):
            return f"the {name} network's input_block has layers of its own (the kernels start at the observation)"
    pw, qw = _linear_widths(pol.hidden_block), _linear_widths(q.q_block)
    if pw is None or qw is None:
        return "a block is not a chain of Linear (with bias) + ReLU layers"
    D = pol.in_block.out_size
    A = pol.out_layer.out_features
    return D, A, pw, qw


class SacdUpdate(LibUpdate):
    ABI = "sacd"

    def __init__(self, parameter, max_batch: int = MAX_BATCH, betas=(0.9, 0.999), eps: float = 1e-8):
        reason = self.why_not(parameter, max_batch)
        if reason:
            raise ValueError(f"SacdUpdate: {reason}")
        self.parameter = parameter
        self.D, self.A, self.policy_widths, self.q_widths = shape_of(parameter)
        self.max_batch = max_batch
        self.device = parameter.log_alpha.device
        self.betas, self.eps = betas, eps
        self._lib = N.lib()
        self._h = N.c_p()
        N.check(self._lib.srlx_sacd_create(ctypes.byref(self._h), self.D, self.A, len(self.policy_widths), _int_array(self.policy_widths), len(self.q_widths),
                                           _int_array(self.q_widths), max_batch, self.device.index or 0))
        self.params = {name: list(getattr(parameter, name).parameters()) for name in NETWORKS}
        self.grads = {name: [torch.zeros_like(p) for p in self.params[name]] for name in TRAINED}
        self.grad_log_alpha = torch.zeros_like(parameter.log_alpha)
        self.exp_avg = {name: [torch.zeros_like(p) for p in self.params[name]] for name in TRAINED}
        self.exp_avg_sq = {name: [torch.zeros_like(p) for p in self.params[name]] for name in TRAINED}
        self.alpha_exp_avg, self.alpha_exp_avg_sq = torch.zeros_like(parameter.log_alpha), torch.zeros_like(parameter.log_alpha)
        flat = [p for name in NETWORKS for p in self.params[name]]
        N.check(self._lib.srlx_sacd_bind(self._h, _ptrs(flat), N.tptr(parameter.log_alpha)))
        N.check(self._lib.srlx_sacd_bind_grads(self._h, _ptrs([g for name in TRAINED for g in self.grads[name]]), N.tptr(self.grad_log_alpha)))
        self._bind_adam([0, 0, 0, 0])

    def _bind_adam(self, steps):
        m = [t for name in TRAINED for t in self.exp_avg[name]] + [self.alpha_exp_avg]
        v = [t for name in TRAINED for t in self.exp_avg_sq[name]] + [self.alpha_exp_avg_sq]
        N.check(self._lib.srlx_sacd_bind_adam(self._h, _ptrs(m), _ptrs(v), (N.c_i64 * 4)(*steps), self.betas[0], self.betas[1], self.eps))

    # ---- what it serves ---------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def why_not(parameter, batch: int = 1, config=None) -> str:
        """'' when libsrlx runs this Parameter's update at this batch size, otherwise the reason it does not.  (`config`: as `VppoUpdate.why_not` takes it; nothing
        a sac.Config sets keeps the update off libsrlx.)"""
        tensors = [parameter.log_alpha] + [p for name in NETWORKS for p in getattr(parameter, name).parameters()]
        reason = tensor_reason(tensors)
        if reason:
            return reason
        shape = shape_of(parameter)
        if isinstance(shape, str):
            return shape
        return SacdUpdate.envelope_reason(*shape, batch)

    @staticmethod
    def envelope_reason(D, A, pw, qw, batch: int = 1) -> str:
        """The envelope of srlx_sacd_create as a sentence ('' inside it).  Host arithmetic: no device needed."""
        if batch > MAX_BATCH:
            return f"batch size {batch} above max_batch {MAX_BATCH}"
        if N.lib().srlx_sacd_scratch_floats(D, A, len(pw), _int_array(pw), len(qw), _int_array(qw), max(1, batch)) < 0:
            return f"outside the envelope (D 1..256, A 2..16, 1..3 layers of 32..512 units in multiples of 32): D {D}, A {A}, policy {tuple(pw)}, q {tuple(qw)}"
        return ""

    # ---- the calls --------------------------------------------------------------------------------------------------------------------------------------
    def steps(self):
        """Optimiser steps taken: [policy, q1, q2, alpha]."""
        out = (N.c_i64 * 4)()
        N.check(self._lib.srlx_sacd_steps(self._h, out))
        return list(out)

    def reset_alpha_optimizer(self):
        """A fresh Adam for log_alpha (sac_tf_discrete.py:170-173: rebuilt after a restore); the networks' optimisers go on."""
        self.alpha_exp_avg.zero_()
        self.alpha_exp_avg_sq.zero_()
        self._bind_adam(self.steps()[:3] + [0])

    def update(self, state, action, next_state, reward, done, lr_policy, lr_q, lr_alpha, hard_sync: bool, discount: float, tau: float, auto_scale: bool,
               target_entropy: float) -> dict:
        """state / next_state f32 [B][D], action i32 [B], reward f32 [B], done u8 [B], all on the device.  Returns y, q1, q2, entropy [B] and `scalars` [5]
        (q1_loss, q2_loss, policy_loss, alpha_loss, alpha), device tensors; nothing synchronises."""
        B = state.shape[0]
        if B > self.max_batch:
            raise ValueError(f"SacdUpdate: batch size {B} above max_batch {self.max_batch}")
        keep = [state.contiguous(), action.contiguous(), next_state.contiguous(), reward.contiguous(), done.contiguous()]
        assert keep[0].dtype == torch.float32 and keep[1].dtype == torch.int32 and keep[3].dtype == torch.float32 and keep[4].dtype == torch.uint8
        out = {k: torch.empty(B, dtype=torch.float32, device=self.device) for k in ("y", "q1", "q2", "entropy")}
        out["scalars"] = torch.empty(5, dtype=torch.float32, device=self.device)
        N.check(self._lib.srlx_sacd_update(self._h, B, N.tptr(keep[0]), N.tptr(keep[1]), N.tptr(keep[2]), N.tptr(keep[3]), N.tptr(keep[4]), float(lr_policy), float(lr_q),
                                           float(lr_alpha), float(discount), float(tau), int(bool(hard_sync)), int(bool(auto_scale)), float(target_entropy),
                                           N.tptr(out["y"]), N.tptr(out["q1"]), N.tptr(out["q2"]), N.tptr(out["entropy"]), N.tptr(out["scalars"]),
                                           N.torch_stream_ptr()))
        self._keep = keep
        return out

    def forward(self, state, target: bool = False, want_logits: bool = True, want_q: bool = True):
        """logits [n][A] and min(q1, q2) over every action [n][A] (None when not wanted) of the online or the target Q-networks."""
        x = state.contiguous()
        n = x.shape[0]
        logits = torch.empty((n, self.A), dtype=torch.float32, device=self.device) if want_logits else None
        qmin = torch.empty((n, self.A), dtype=torch.float32, device=self.device) if want_q else None
        N.check(self._lib.srlx_sacd_forward(self._h, n, N.tptr(x), int(bool(target)), N.tptr(logits), N.tptr(qmin), N.torch_stream_ptr()))
        self._keep_fwd = x
        return logits, qmin

    def act(self, n_rows: int, obs_base, row_offsets, seed: int, counter, random_until: int, actions, logits=None, scores=None):
        """srlx_sacd_act: the Worker's action of `n_rows` rows in one launch.  `obs_base`: a float32 device tensor or the address of a ring
        (DeviceReplay.obs_base); `row_offsets`: i64 [n_rows] offsets in floats (None: dense rows); `counter`: i64 [1] device tensor, read and not advanced;
        `actions` i32 [n_rows]; optional `logits` f32 [n_rows][A] and `scores` f64 [n_rows][A].  Nothing synchronises; returns `actions`."""
        base = N.tptr(obs_base) if isinstance(obs_base, torch.Tensor) else (None if obs_base is None else N.c_p(obs_base))
        N.check(self._lib.srlx_sacd_act(self._h, int(n_rows), base, N.tptr(row_offsets), N.c_u64(int(seed) & 0xFFFFFFFFFFFFFFFF), N.tptr(counter), int(random_until),
                                        N.tptr(actions), N.tptr(logits), N.tptr(scores), N.torch_stream_ptr()))
        return actions


def ring_batch(B: int, D: int, A: int, obs_base, offsets, actions, rewards, terminated, states, next_states, onehot, done):
    """srlx_sacd_ring_batch: what a DeviceReplay draw wrote (`frame_off_all` i64 [B][2], `batch.actions` i32, `batch.rewards` and
    `batch.terminated` f32, all [B] or [B][1]) as the arguments of `sac.Trainer.train_on_batch`: states / next states f32 [B][D], one-hot f32 [B][A], done u8 [B]."""
    base = N.tptr(obs_base) if isinstance(obs_base, torch.Tensor) else (None if obs_base is None else N.c_p(obs_base))
    N.check(N.lib().srlx_sacd_ring_batch(int(B), int(D), int(A), base, N.tptr(offsets), N.tptr(actions), N.tptr(rewards), N.tptr(terminated), N.tptr(states),
                                         N.tptr(next_states), N.tptr(onehot), N.tptr(done), N.torch_stream_ptr()))
