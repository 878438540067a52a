"""NoTarget_DQN's update on libsrlx (csrc/srlx_dqnnot.hip): `DqnNotUpdate` binds an `algorithms.dqn_not.Parameter`'s own tensors by address -- the
network stays what the plugin, checkpoints and `load_state_dict` see -- and owns the handle, the gradient tensors the kernels write and the Adam state (moments
here, the step count in the handle).  One `update` is the whole of trainer.py:54-80 for one batch, in six launches on the float64 matrix cores.  `DqnNotAct`
is the acting side: a handle that binds the same tensors and nothing else, and runs the network's forward in one launch."""
import ctypes

import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd._native import _linear_widths, _ptrs
from simple_distributed_rl_amd.device import _row_update as R

MAX_BATCH = 4096  # srlx_dqnnot_create's largest max_batch
MAX_ACT_ROWS = 65536  # srlx_dqnnot_act's largest n_rows


def shape_of(parameter):
    """(D, U, A) of a dqn_not.Parameter, or a sentence saying why its network is not one the kernels run."""
    net = parameter.q_online
    if not hasattr(net.in_block, "hidden_layers"):
        return "the input_block is an image block (the kernels start at a flat observation)"
    if _linear_widths(net.in_block) != ():
        return "the input_block has layers of its own (the kernels' first layer is the hidden_block's)"
    return net.hidden_block[0].in_features, net.hidden_block[0].out_features, net.adv_block[2].out_features


def tensors_of(parameter) -> list:
    """hidden_block.0, v_block.0, v_block.2, adv_block.0, adv_block.2, weight then bias each: the order of srlx_dqnnot_bind_params."""
    net = parameter.q_online
    return [t for lin in (net.hidden_block[0], net.v_block[0], net.v_block[2], net.adv_block[0], net.adv_block[2]) for t in (lin.weight, lin.bias)]


class DqnNotUpdate(R.RowUpdate):
    ABI = "dqnnot"
    MAX_BATCH = MAX_BATCH  # declaring it is what lets SrlxUpdateBackend size an ordinary update past 256
    shape_of = staticmethod(shape_of)
    tensors_of = staticmethod(tensors_of)

    def __init__(self, parameter, max_batch: int = 256, betas=(0.9, 0.999), eps: float = 1e-8):
        self.D, self.U, self.A = self._open(parameter, max_batch, betas, eps)
        N.check(self._lib.srlx_dqnnot_create(ctypes.byref(self._h), self.D, self.U, self.A, max_batch, self.device.index or 0))
        self._alloc()
        self.raw_grads = self.grads  # (the reference does not clip: one set of tensors serves both of the handle's lists)
        N.check(self._lib.srlx_dqnnot_bind_params(self._h, _ptrs(self.params)))
        N.check(self._lib.srlx_dqnnot_bind_grads(self._h, _ptrs(self.grads), _ptrs(self.raw_grads)))
        N.check(self._lib.srlx_dqnnot_bind_adam(self._h, _ptrs(self.exp_avg), _ptrs(self.exp_avg_sq), 0, betas[0], betas[1], eps))

    # ---- what it serves (`why_not` and `serves`: RowUpdate) ------------------------------------------------------------------------------------------------
    @staticmethod
    def config_reasons(config) -> list:
        """What `why_not` refuses on the config alone, every sentence (no Parameter, no device)."""
        why = R.block_kwarg_reasons(config, (), "the kernels start at the observation")
        if tuple(config.input_block.value.kwargs.get("layer_sizes", ())) != ():
            why.append("the input_block has layers of its own (the kernels' first layer is the hidden_block's)")
        return why

    @staticmethod
    def envelope_reason(D, U, A, batch: int = 1) -> str:
        """The envelope of srlx_dqnnot_create as a sentence ('' inside it).  Host arithmetic: no device needed."""
        if batch > MAX_BATCH:
            return f"batch size {batch} above max_batch {MAX_BATCH}"
        if not 1 <= D <= 256:
            return f"observation length {D} outside 1..256"
        if not (32 <= U <= 512 and U % 32 == 0):
            return f"base_units {U} outside 32..512 in multiples of 32"
        if not 2 <= A <= 32:
            return f"{A} actions outside 2..32"
        return ""

    # ---- the call (`steps`: RowUpdate) -----------------------------------------------------------------------------------------------------------------------
    def update(self, states, actions, reward, not_terminated, total_reward, weights, discount, align_coeff, lr) -> dict:
        """states f32 [2B][D] (rows B.. are the next states); actions i32 [B]; reward, not_terminated, total_reward f32 [B]; weights f32 [B] or None (every
        weight 1); all on the device.  Returns q, target_q [B] and `losses` [2] (loss_q, loss_align), device tensors; nothing synchronises."""
        B = actions.shape[0]
        if B > self.max_batch:
            raise ValueError(f"DqnNotUpdate: batch size {B} above max_batch {self.max_batch}")
        keep = [t.contiguous() if t is not None else None for t in (states, actions, reward, not_terminated, total_reward, weights)]
        assert keep[1].dtype == torch.int32 and all(t.dtype == torch.float32 for t in keep[:1] + keep[2:] if t is not None)
        assert keep[0].numel() == 2 * B * self.D and all(t.numel() == B for t in keep[2:] if t is not None)
        f = dict(dtype=torch.float32, device=self.device)
        out = {"q": torch.empty(B, **f), "target_q": torch.empty(B, **f), "losses": torch.empty(2, **f)}
        N.check(self._lib.srlx_dqnnot_update(self._h, *[N.tptr(t) for t in keep], B, float(discount), float(align_coeff), float(lr), N.tptr(out["q"]),
                                             N.tptr(out["target_q"]), N.tptr(out["losses"]), N.torch_stream_ptr()))
        self._keep = keep
        return out


class DqnNotAct(R.LibUpdate):
    """The network's forward on libsrlx for acting (srlx_dqnnot_act): a handle of its own with max_batch 1 -- nothing of the acting launch is
    sized by it -- that binds the Parameter's own tensors by address and nothing else: no gradient tensors, no Adam state.  It reads the weights where they
    are, so it sees `load_state_dict` and every update of a DqnNotUpdate on the same tensors."""
    ABI = "dqnnot"
    MAX_ROWS = MAX_ACT_ROWS

    @staticmethod
    def rows_reason(n: int) -> str:
        return f"{n} rows above {MAX_ACT_ROWS} in one call" if n > MAX_ACT_ROWS else ""

    @classmethod
    def why_not(cls, parameter, n: int = 1, config=None) -> str:
        """'' when libsrlx runs this Parameter's forward for n rows, otherwise the reason it does not: DqnNotUpdate's sentences, then the rows'."""
        reason = R.tensor_reason(tensors_of(parameter))
        if reason:
            return reason
        shape = shape_of(parameter)
        if isinstance(shape, str):
            return shape
        return DqnNotUpdate.envelope_reason(*shape) or cls.rows_reason(n)

    def __init__(self, parameter):
        reason = self.why_not(parameter)
        if reason:
            raise ValueError(f"DqnNotAct: {reason}")
        self.params = tensors_of(parameter)
        self.device = self.params[0].device
        self.D, self.U, self.A = shape_of(parameter)
        self._lib = N.lib()
        self._h = N.c_p()
        N.check(self._lib.srlx_dqnnot_create(ctypes.byref(self._h), self.D, self.U, self.A, 1, self.device.index or 0))
        N.check(self._lib.srlx_dqnnot_bind_params(self._h, _ptrs(self.params)))

    def act(self, states):
        """states f32 [n][D] on the device, n 1..65536.  Returns q f32 [n][A], v f32 [n][1] and the greedy actions i32 [n] -- the first maximum of the returned
        q row -- as device tensors; nothing synchronises."""
        states = states.contiguous()
        n = states.shape[0]
        assert states.dtype == torch.float32 and states.device == self.device and states.numel() == n * self.D
        q = torch.empty(n, self.A, dtype=torch.float32, device=self.device)
        v = torch.empty(n, 1, dtype=torch.float32, device=self.device)
        actions = torch.empty(n, dtype=torch.int32, device=self.device)
        N.check(self._lib.srlx_dqnnot_act(self._h, n, N.tptr(states), N.tptr(q), N.tptr(v), N.tptr(actions), N.torch_stream_ptr()))
        self._keep = states
        return q, v, actions
