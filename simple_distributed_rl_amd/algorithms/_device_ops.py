"""Device-side arithmetic shared by the DQN / Rainbow / C51 plugin trainers: thin wrappers that hand torch
tensors to libsrlx.  A trainer on a non-GPU device fails loudly -- there is no CPU fallback."""
import numpy as np
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.device.sequence_store import fill_invalid_mask


def require_gpu(device_str: str) -> torch.device:
    if not str(device_str).startswith("cuda") or not torch.cuda.is_available():
        raise RuntimeError(
            f"simple_distributed_rl_amd: this trainer runs its TD-target / loss / priority arithmetic in libsrlx HIP kernels and "
            f"needs an MI355X (device was '{device_str}'). There is no CPU fallback; use the reference for CPU-only runs."
        )
    N.lib()
    return torch.device(device_str)


def invalid_mask(invalid_lists, shape, device) -> torch.Tensor:
    """nested lists of invalid action ids -> uint8 mask of `shape` (..., A), or None when all empty."""
    m = np.empty(shape, np.uint8)
    return torch.from_numpy(m).to(device) if fill_invalid_mask(m.reshape(-1, shape[-1]), invalid_lists) else None


class SrlxUpdateBackend:
    """The backend choice of a trainer whose update runs on libsrlx or in torch (sac.Trainer, ppo_v.Trainer).  `update_backend` asks for "srlx" or "torch"; the
    first `train_on_batch` (or `require_srlx_update`) fixes the answer until the next `setup`: "srlx" when the device layer's update serves the Parameter at that
    batch size, otherwise "torch", with the reason in `why_not_srlx_update`.  `update_path` names the backend the last update ran on.  The trainer supplies
    `_srlx_update_class()`, the device layer's update (`why_not(parameter, batch, config)` and a constructor over the Parameter), and `_make_torch_update()`, its
    torch optimisers and schedulers."""

    def _reset_backend(self) -> None:
        """(from `on_setup`)"""
        self.update_path = ""
        self.why_not_srlx_update = ""
        self._backend = None

    def _choose_backend(self, batch: int) -> None:
        if self.update_backend not in ("srlx", "torch"):
            raise ValueError(f"update_backend {self.update_backend!r}: 'srlx' or 'torch'")
        self._backend = "torch"
        if self.update_backend == "srlx":
            update = self._srlx_update_class()
            self.why_not_srlx_update = update.why_not(self.parameter, batch, self.config)
            if not self.why_not_srlx_update:
                self._backend = "srlx"
                self._srlx = update(self.parameter, max_batch=max(batch, min(256, self.config.batch_size)))
        if self._backend == "torch":
            self._make_torch_update()

    def _backend_for(self, batch: int) -> str:
        """The backend a batch of this size runs on: chosen at the first call, and a libsrlx update is sized then."""
        if self._backend is None:
            self._choose_backend(batch)
        if self._backend == "srlx" and batch > self._srlx.max_batch:
            raise ValueError(f"a batch of {batch} on a libsrlx update sized for {self._srlx.max_batch} (the backend is fixed at the first train())")
        return self._backend

    def require_srlx_update(self, batch: int, caller: str):
        """For a device engine, whose acting pass runs on the update's own handle: asks for "srlx", fixes the backend now and not at the first update, and returns
        the bound update.  An update that would run in torch is an error there, not a slower engine: ValueError in `caller`'s name with the reason."""
        self.update_backend = "srlx"
        self._choose_backend(batch)
        if self._backend != "srlx":
            raise ValueError(f"{caller}: the update does not run on libsrlx: {self.why_not_srlx_update}")
        return self._srlx


class TdOps:
    def __init__(self, device: torch.device):
        self.dev = device
        self.lib = N.lib()

    def nstep(self, q_on_next, q_tg_next, q0, actions, rewards, terminated, invalid, weights, discount, retrace_h, double_dqn, rescale):
        B, n, A = q_tg_next.shape
        d = self.dev
        target = torch.empty(B, dtype=torch.float32, device=d)
        loss = torch.empty(1, dtype=torch.float32, device=d)
        grad = torch.empty((B, A), dtype=torch.float32, device=d)
        pri = torch.empty(B, dtype=torch.float32, device=d)
        keep = [t.contiguous() for t in (q_on_next, q_tg_next, q0.detach(), actions, rewards, terminated, weights)]
        inv = invalid.contiguous() if invalid is not None else None
        N.check(
            self.lib.srlx_nstep_td_huber_priority(
                B, n, A, N.tptr(keep[0]), N.tptr(keep[1]), N.tptr(keep[2]), N.tptr(keep[3]), N.tptr(keep[4]), N.tptr(keep[5]), N.tptr(inv),
                N.tptr(keep[6]), float(discount), float(retrace_h), int(double_dqn), int(rescale), N.tptr(target), N.tptr(loss), N.tptr(grad),
                N.tptr(pri), N.torch_stream_ptr(),
            )
        )
        self._keep = keep + [inv]
        return target, loss, grad, pri

    def huber(self, target, q_all, actions, weights):
        """loss / grad / priorities for a given target: the n=1 degenerate case of the fused kernel
        (reward = target, terminated = 1 passes the target through bit-exactly)."""
        B, A = q_all.shape
        z = torch.zeros((B, 1, A), dtype=torch.float32, device=self.dev)
        ones = torch.ones((B, 1), dtype=torch.float32, device=self.dev)
        return self.nstep(z, z, q_all, actions.view(B, 1), target.view(B, 1), ones, None, weights, 0.0, 1.0, True, False)

    def dqn_target(self, q_on_next, q_tg_next, rewards, undone, invalid, discount, double_dqn, rescale, f64_accum, discount_per_sample=None):
        B, A = q_tg_next.shape
        out = torch.empty(B, dtype=torch.float32, device=self.dev)
        keep = [t.contiguous() if t is not None else None for t in (q_on_next, q_tg_next, rewards, undone, invalid, discount_per_sample)]
        N.check(
            self.lib.srlx_dqn_target(B, A, N.tptr(keep[0]), N.tptr(keep[1]), N.tptr(keep[2]), N.tptr(keep[3]), N.tptr(keep[4]), float(discount),
                                     N.tptr(keep[5]), int(double_dqn), int(rescale), int(f64_accum), N.tptr(out), N.torch_stream_ptr())
        )
        self._keep2 = keep
        return out

    def agent57_priority(self, target_ext, q_ext, target_int, q_int, actions, actor_idx, beta_list, n_actions=None):
        """|td_ext + beta[actor] * td_int| with td = target - q[action] (agent57_light/model_torch.py:442,367-373);
        q_ext=None: target_ext / target_int already are TD errors (Agent57's sequence means).
        Returns (td_ext, td_int or None, priorities)."""
        B, A = (q_ext.shape if q_ext is not None else (target_ext.shape[0], n_actions))
        d = self.dev
        pri = torch.empty(B, dtype=torch.float32, device=d)
        td_e = torch.empty(B, dtype=torch.float32, device=d)
        td_i = torch.empty(B, dtype=torch.float32, device=d) if target_int is not None else None
        keep = [t.detach().contiguous() if t is not None else None for t in (target_ext, q_ext, target_int, q_int, actions, actor_idx, beta_list)]
        N.check(
            self.lib.srlx_agent57_priority(B, A, *[N.tptr(t) for t in keep], N.tptr(td_e), N.tptr(td_i), N.tptr(pri), N.torch_stream_ptr())
        )
        self._keep3 = keep
        return td_e, td_i, pri

    def agent57_seq_td(self, q, q_target, actions, rewards, dones, invalid, discounts, weights, retrace_h, double_dqn, rescale):
        """srlx_agent57_seq_td (agent57.py:301-379 + model_torch.py:469-492) over q [B][S + 1][A]: returns (target [S][B], loss [1], grad_q, td_mean [B])."""
        d = self.dev
        B, S1, A = q.shape
        S = S1 - 1
        target = torch.empty((S, B), dtype=torch.float32, device=d)
        loss = torch.empty(1, dtype=torch.float32, device=d)
        grad = torch.empty((B, S1, A), dtype=torch.float32, device=d)
        td = torch.empty(B, dtype=torch.float32, device=d)
        scratch = torch.empty(2 * B * S, dtype=torch.float32, device=d)
        keep = [t.detach().contiguous() if t is not None else None for t in (q, q_target, actions, rewards, dones, invalid, discounts, weights)]
        N.check(self.lib.srlx_agent57_seq_td(B, S, A, *[N.tptr(t) for t in keep], float(retrace_h), int(double_dqn), int(rescale), N.tptr(target), N.tptr(loss),
                                             N.tptr(grad), N.tptr(td), N.tptr(scratch), N.torch_stream_ptr()))
        self._keep4 = keep + [scratch]
        return target, loss, grad, td

    def r2d2_seq_td(self, q, q_target, actions, mu, rewards, dones, invalid, weights, discount, retrace_h, retrace, double_dqn, rescale):
        """srlx_r2d2_seq_td (r2d2.py:152-209) over q [B][S + 1][A]: returns (target [B][S], loss [1], grad_q, td_mean [B] = mean_t(gain - q[a]), signed).
        actions i32, dones u8 and invalid u8 [B][S + 1][A] or None."""
        d = self.dev
        B, S1, A = q.shape
        S = S1 - 1
        target = torch.empty((B, S), dtype=torch.float32, device=d)
        loss = torch.empty(1, dtype=torch.float32, device=d)
        grad = torch.empty((B, S1, A), dtype=torch.float32, device=d)
        td = torch.empty(B, dtype=torch.float32, device=d)
        keep = [t.detach().contiguous() if t is not None else None for t in (q, q_target, actions, mu, rewards, dones, invalid, weights)]
        assert keep[2].dtype == torch.int32 and keep[5].dtype == torch.uint8 and (keep[6] is None or keep[6].dtype == torch.uint8)
        N.check(self.lib.srlx_r2d2_seq_td(B, S, A, *[N.tptr(t) for t in keep], float(discount), float(retrace_h), int(retrace), int(double_dqn), int(rescale),
                                          N.tptr(target), N.tptr(loss), N.tptr(grad), N.tptr(td), N.torch_stream_ptr()))
        self._keep5 = keep
        return target, loss, grad, td


class C51Ops:
    """C51's update arithmetic on logits torch produced (csrc/srlx_c51_math.h through srlx_c51_loss), as `TdOps.huber` serves DQN's."""

    def __init__(self, device: torch.device):
        self.dev = device
        self.lib = N.lib()

    def loss(self, logits_next, logits, actions, rewards, terminated, n_actions, n_atoms, v_min, v_max, discount):
        """logits_next / logits: f32 [B][A * N] (or [B][A][N]) of s' and s.  Returns (m [B][N], p0 [B][N], grad of the mean loss w.r.t. `logits` in its
        shape, loss [1])."""
        B, d = logits.shape[0], self.dev
        m = torch.empty((B, n_atoms), dtype=torch.float32, device=d)
        p0 = torch.empty((B, n_atoms), dtype=torch.float32, device=d)
        grad = torch.empty(tuple(logits.shape), dtype=torch.float32, device=d)
        loss = torch.empty(1, dtype=torch.float32, device=d)
        keep = [t.detach().contiguous() for t in (logits_next, logits, actions, rewards, terminated)]
        assert keep[0].numel() == keep[1].numel() == B * n_actions * n_atoms and keep[2].dtype == torch.int32
        N.check(self.lib.srlx_c51_loss(B, int(n_actions), int(n_atoms), float(v_min), float(v_max), float(discount), N.tptr(keep[0]), N.tptr(keep[1]),
                                       N.tptr(keep[2]), N.tptr(keep[3]), N.tptr(keep[4]), N.tptr(m), N.tptr(p0), N.tptr(grad), N.tptr(loss),
                                       N.torch_stream_ptr()))
        self._keep = keep
        return m, p0, grad, loss


class NguOps:
    """Device-resident episodic memories + novelty rewards (csrc/srlx_ngu.hip)."""

    def __init__(self, device: torch.device, n_envs: int, emb_dim: int, capacity: int, k: int, epsilon: float, cluster_distance: float, pseudo_counts: float):
        import ctypes

        self.dev, self.lib, self.n_envs, self.emb_dim = device, N.lib(), n_envs, emb_dim
        h = ctypes.c_void_p()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        N.check(self.lib.srlx_ngu_create(ctypes.byref(h), n_envs, emb_dim, capacity, k, float(epsilon), float(cluster_distance), float(pseudo_counts), idx))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.srlx_ngu_destroy(self.h)
            self.h = None

    def reset(self):
        N.check(self.lib.srlx_ngu_reset(self.h, N.torch_stream_ptr()))

    def episodic(self, emb: torch.Tensor, reset: torch.Tensor = None, active: torch.Tensor = None) -> torch.Tensor:
        emb = emb.detach().to(torch.float32).contiguous().view(self.n_envs, self.emb_dim)
        out = torch.empty(self.n_envs, dtype=torch.float32, device=self.dev)
        self._keep = (emb, reset, active)
        N.check(self.lib.srlx_ngu_episodic_reward(self.h, N.tptr(emb), N.tptr(reset), N.tptr(active), N.tptr(out), N.torch_stream_ptr()))
        return out

    def lifelong(self, target: torch.Tensor, train: torch.Tensor, lifelong_max: float) -> torch.Tensor:
        target, train = target.detach().contiguous(), train.detach().contiguous()
        n, dim = target.shape
        out = torch.empty(n, dtype=torch.float32, device=self.dev)
        self._keep_l = (target, train)
        N.check(self.lib.srlx_ngu_lifelong_reward(n, dim, N.tptr(target), N.tptr(train), float(lifelong_max), N.tptr(out), N.torch_stream_ptr()))
        return out
