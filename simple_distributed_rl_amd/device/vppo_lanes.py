"""V-PPO's episode store in HBM (csrc/srlx_vppo_lanes.hip): the Worker's trackings and the ReplayBuffer of algorithms/ppo_v.py for E lock-stepped
lanes.  A V-PPO item carries the discounted return to its episode's end, so a lane's steps wait in a tracking ring until the episode closes; the closing push
walks them backwards and appends the items to the item ring in that order, as `Worker.on_step` does.  `sample` draws B distinct items (Floyd's algorithm on keyed
uniforms) as the update's dense tensors.  The store offers what `CartPoleVecEnv` asks of a replay (`E`, `dev`, `seed`, `F`, `obs_uint8`, `needs_reset_ptr`).
`action_dim` = K > 0 makes it the Normal head's store: K float32 action elements and K log-probabilities per step, the same kernels."""
import ctypes

import torch

from simple_distributed_rl_amd import _native as N

MAX_EPISODE_STEPS = 4094  # srlx_vppo_lanes_create: the close keeps one lane's rewards and returns in LDS
_VIEWS = ("obs", "action", "logp", "reward", "not_terminated", "done", "length", "needs_reset", "item_s", "item_s2", "item_action", "item_logp", "item_reward",
          "item_not_terminated", "item_total", "count")


class VppoLanes:
    obs_uint8 = False

    def __init__(self, n_envs: int, obs_dim: int, max_episode_steps: int, capacity: int, batch_size: int, warmup_size: int, discount: float, seed: int = 0,
                 device: int = 0, action_dim: int = 0):
        self.E, self.F, self.D = int(n_envs), int(obs_dim), int(obs_dim)
        self.R, self.capacity, self.B, self.warmup_size = int(max_episode_steps) + 2, int(capacity), int(batch_size), int(warmup_size)
        self.seed, self.discount = int(seed), float(discount)
        self.dev = torch.device(f"cuda:{device}")
        self._lib = N.lib()
        self._h = N.c_p()
        self.action_dim = int(action_dim)  # 0: one int32 action per step (the categorical head)
        self.K = max(1, self.action_dim)
        if self.action_dim:
            N.check(self._lib.srlx_vppo_lanes_create_normal(ctypes.byref(self._h), self.E, self.D, int(max_episode_steps), self.capacity, self.discount, self.action_dim,
                                                            device))
        else:
            N.check(self._lib.srlx_vppo_lanes_create(ctypes.byref(self._h), self.E, self.D, int(max_episode_steps), self.capacity, self.discount, device))
        self._push, self._sample = ((self._lib.srlx_vppo_lanes_push_normal, self._lib.srlx_vppo_lanes_sample_normal) if self.action_dim else
                                    (self._lib.srlx_vppo_lanes_push, self._lib.srlx_vppo_lanes_sample))
        self._action_dtype = torch.float32 if self.action_dim else torch.int32
        views, row = (N.c_p * len(_VIEWS))(), N.c_i64(0)
        N.check(self._lib.srlx_vppo_lanes_views(self._h, views, ctypes.byref(row)))
        self._ptr = {k: int(views[i] or 0) for i, k in enumerate(_VIEWS)}
        self.needs_reset_ptr = N.c_p(self._ptr["needs_reset"])
        self.lock_steps = 0
        self._open = False  # the warm-up gate: the count is monotone, so once open it is never read again
        B, D, d = self.B, self.D, self.dev
        self.states = torch.zeros((B, D), dtype=torch.float32, device=d)
        self.next_states = torch.zeros((B, D), dtype=torch.float32, device=d)
        self.actions = torch.zeros((B, self.K) if self.action_dim else B, dtype=self._action_dtype, device=d)
        self.old_logpi = torch.zeros((B, self.K), dtype=torch.float32, device=d)
        self.rewards = torch.zeros((B, 1), dtype=torch.float32, device=d)
        self.not_terminated = torch.zeros((B, 1), dtype=torch.float32, device=d)
        self.total_rewards = torch.zeros((B, 1), dtype=torch.float32, device=d)
        self.slots = torch.zeros(B, dtype=torch.int64, device=d)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.srlx_vppo_lanes_destroy(self._h)
            self._h = None

    # ---- the lock-step ------------------------------------------------------------------------------------------------------------------------------------
    def reset_all(self, first_obs: torch.Tensor) -> None:
        x = first_obs.contiguous()
        assert x.dtype == torch.float32 and x.numel() == self.E * self.D
        N.check(self._lib.srlx_vppo_lanes_reset(self._h, N.tptr(x), N.torch_stream_ptr()))
        self._keep = x
        self.lock_steps, self._open = 0, False

    def current_row_ptr(self):
        """The dense [E][D] row the lanes act on at this lock-step: srlx_vppo_act's input as it stands."""
        return N.c_p(self._ptr["obs"] + 4 * (self.lock_steps % self.R) * self.E * self.D)

    def push(self, actions, logp, rewards, terminated, done, next_obs, bump=None) -> None:
        """One lock-step (two launches): the fields of every lane's step, `next_obs` into the next row, and the close of every lane whose step was done."""
        assert actions.dtype == self._action_dtype and logp.dtype == torch.float32 and rewards.dtype == torch.float32
        assert actions.is_contiguous() and logp.is_contiguous()  # (K elements per lane, dense)
        assert terminated.dtype == torch.uint8 and done.dtype == torch.uint8 and next_obs.dtype == torch.float32 and next_obs.is_contiguous()
        assert actions.numel() == self.E * self.K and logp.numel() == self.E * self.K
        assert rewards.numel() == self.E and terminated.numel() == self.E and done.numel() == self.E
        assert next_obs.numel() == self.E * self.D
        N.check(self._push(self._h, N.tptr(actions), N.tptr(logp), N.tptr(rewards), N.tptr(terminated), N.tptr(done), N.tptr(next_obs), N.tptr(bump), N.torch_stream_ptr()))
        self.lock_steps += 1

    def sample(self, batch: int = None):
        """B distinct items as `train_on_batch`'s tensors (views of buffers the next draw overwrites): state, next state, int32 actions [B] (float32 [B][K] on a
        Normal store), old log-probabilities [B][K], rewards, not-terminated, total rewards, and the drawn slots."""
        B = self.B if batch is None else int(batch)
        assert 1 <= B <= self.B
        N.check(self._sample(self._h, B, ctypes.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), N.tptr(self.states), N.tptr(self.next_states), N.tptr(self.actions),
                             N.tptr(self.old_logpi), N.tptr(self.rewards), N.tptr(self.not_terminated), N.tptr(self.total_rewards), N.tptr(self.slots),
                             N.torch_stream_ptr()))
        return (self.states[:B], self.next_states[:B], self.actions[:B], self.old_logpi[:B], self.rewards[:B], self.not_terminated[:B], self.total_rewards[:B],
                self.slots[:B])

    # ---- read-backs -----------------------------------------------------------------------------------------------------------------------------------------
    def count(self):
        """(items ever added, the sticky error word); synchronises."""
        added, err = N.c_i64(0), ctypes.c_int32(0)
        N.check(self._lib.srlx_vppo_lanes_count(self._h, ctypes.byref(added), ctypes.byref(err), N.torch_stream_ptr()))
        return int(added.value), int(err.value)

    def check(self) -> None:
        err = self.count()[1]
        if err == 1:
            raise RuntimeError("VppoLanes: an episode stored more steps than max_episode_steps; the whole episode was dropped")
        if err:
            raise RuntimeError("VppoLanes: a draw asked for more items than the ring holds")

    def length(self) -> int:
        return min(self.capacity, self.count()[0])

    def is_warmup_needed(self) -> bool:
        """One synchronising read per call while the gate is closed, none once it is open.  The gate also waits for a whole batch: a draw of more items than
        the ring holds is an error (a config whose warmup_size is under its batch_size would otherwise reach it)."""
        if not self._open:
            self._open = self.length() >= max(self.warmup_size, self.B)
        return not self._open

    def hbm_bytes(self) -> int:
        RE, C, D, K = self.R * self.E, self.capacity, self.D, self.K
        return RE * (4 * D + 8 * K + 9) + 5 * self.E + C * (8 * D + 8 * K + 12) + 20

    def view(self, name: str) -> torch.Tensor:
        """A host copy of one of the store's arrays (the tests): the tracking ring's in [R][E] order, the item ring's in slot order, `count` the two words."""
        C, D, E = self.capacity, self.D, self.E
        k = (self.K,) if self.action_dim else ()  # (a Normal store's action and log-probability views carry the K elements)
        shape, dt = {"obs": ((self.R, E, D), torch.float32), "action": ((self.R, E) + k, self._action_dtype), "logp": ((self.R, E) + k, torch.float32),
                     "reward": ((self.R, E), torch.float32), "not_terminated": ((self.R, E), torch.float32), "done": ((self.R, E), torch.uint8),
                     "length": ((E,), torch.int32), "needs_reset": ((E,), torch.uint8), "item_s": ((C, D), torch.float32), "item_s2": ((C, D), torch.float32),
                     "item_action": ((C,) + k, self._action_dtype), "item_logp": ((C,) + k, torch.float32), "item_reward": ((C,), torch.float32),
                     "item_not_terminated": ((C,), torch.float32), "item_total": ((C,), torch.float32), "count": ((2,), torch.int64)}[name]
        out = torch.empty(shape, dtype=dt)
        N.check(self._lib.srlx_vppo_lanes_read(self._h, _VIEWS.index(name), out.numel() * out.element_size(), N.c_p(out.data_ptr()), N.torch_stream_ptr()))
        return out
