"""What the plugin-side wrappers of libsrlx's row-blocked updates share (csrc/srlx_param_tail.h is the same cut on the library's side).  `LibUpdate` is a handle
and the question whether libsrlx serves a Parameter; `RowUpdate` adds what V-PPO's and NoT_SAC's wrappers have in common: the refusal sentences of a
flat-observation actor-critic, the four tensor lists beside the Parameter's own and the order in which `why_not` asks.  A subclass keeps its `shape_of`, its
envelope sentence, its `create` / `bind` argument lists (the two ABIs differ there) and its calls."""
import math

import torch

from simple_distributed_rl_amd import _native as N

MAX_BATCH = 256
# block options the kernels' layers cover; anything else set on a block keeps the update on torch
_MLP_FREE_KWARGS = {"layer_sizes", "activation", "kernel_initializer", "bias_initializer"}


def tensor_reason(tensors) -> str:
    """Why libsrlx cannot bind these tensors by address ('' when it can)."""
    if not all(t.is_cuda for t in tensors):
        return "the parameters are CPU tensors"  # (answered before libsrlx is loaded)
    if not all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
        return "a parameter is not a dense float32 tensor"
    return ""


def block_kwarg_reasons(config, names, input_sentence: str) -> list:
    """A sentence for every block of `names`, then for the input block's value part, that sets an option the kernels' layers do not cover."""
    why = []
    for name in names:
        extra = set(getattr(config, name).kwargs) - _MLP_FREE_KWARGS
        if extra:
            why.append(f"the {name} sets {sorted(extra)} (the kernels' layers are Linear with bias + ReLU)")
    extra = set(config.input_block.value.kwargs) - _MLP_FREE_KWARGS
    if extra:
        why.append(f"the input_block sets {sorted(extra)} ({input_sentence})")
    return why


def lr_schedule_reason(config) -> list:
    sch = config.lr_scheduler
    if sch.schedule_type not in ("", "step", "exp", "cosine", "piecewise"):
        return [f"the lr schedule {sch.schedule_type!r} is not one the host evaluates per step"]
    return []


def head_of(dist_block, discrete_name: str):
    """(head, n_out) of a policy's distribution block -- 1: Normal with n_out elements, 0: `discrete_name` with n_out actions -- or the sentence that refuses it."""
    if hasattr(dist_block, "loc_layers"):
        if len(dist_block.h_layers) or len(dist_block.loc_layers) != 1 or len(dist_block.log_scale_layers) != 1:
            return "the Normal head has hidden layers of its own"
        return 1, dist_block.loc_layers[0].out_features
    if len(dist_block.h_layers) != 1:
        return f"the {discrete_name} head has hidden layers of its own"
    return 0, dist_block.h_layers[0].out_features


def log_scale_range(dist_block):
    """The Normal head's clamp as the kernels take it: (lo, hi), infinite when there is none."""
    if getattr(dist_block, "enable_stable_gradients", False):
        return float(dist_block.stable_gradients_scale_range[0]), float(dist_block.stable_gradients_scale_range[1])
    return -math.inf, math.inf


class LibUpdate:
    """A libsrlx handle `_h` of the entry points srlx_<ABI>_*, and `serves` over the subclass's `why_not`."""
    ABI = ""

    def __del__(self):
        if getattr(self, "_h", None):
            getattr(self._lib, f"srlx_{self.ABI}_destroy")(self._h)
            self._h = None

    @classmethod
    def serves(cls, parameter, batch: int = 1, config=None) -> bool:
        return cls.why_not(parameter, batch, config) == ""


class RowUpdate(LibUpdate):
    """A subclass gives ABI, `tensors_of(parameter)` (bind order), `shape_of(parameter)` (a tuple or a sentence), `config_reasons(config)` and
    `envelope_reason(*shape, batch)`."""

    def _open(self, parameter, max_batch, betas, eps):
        """Everything of a constructor that comes before srlx_<ABI>_create; returns the shape."""
        reason = self.why_not(parameter, max_batch)
        if reason:
            raise ValueError(f"{type(self).__name__}: {reason}")
        self.parameter = parameter
        self.max_batch = max_batch
        self.params = self.tensors_of(parameter)
        self.device = self.params[0].device
        self.betas, self.eps = betas, eps
        self._lib = N.lib()
        self._h = N.c_p()
        return self.shape_of(parameter)

    def _alloc(self):
        """The tensors the kernels write beside the Parameter's own, in bind order."""
        self.grads = [torch.zeros_like(p) for p in self.params]      # after the norm clip: what Adam reads
        self.raw_grads = [torch.zeros_like(p) for p in self.params]  # before it
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]

    @classmethod
    def why_not(cls, parameter, batch: int = 1, config=None) -> str:
        """'' when libsrlx runs this Parameter's update at this batch size, otherwise the reason it does not."""
        reason = tensor_reason(cls.tensors_of(parameter))
        if reason:
            return reason
        if config is not None:
            reasons = cls.config_reasons(config)
            if reasons:
                return reasons[0]
        shape = cls.shape_of(parameter)
        if isinstance(shape, str):
            return shape
        return cls.envelope_reason(*shape, batch)

    def steps(self) -> int:
        """Optimiser steps taken (by every optimiser of the handle)."""
        return int(getattr(self._lib, f"srlx_{self.ABI}_steps")(self._h))
