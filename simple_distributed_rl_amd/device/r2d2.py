"""Device engine of R2D2: E lock-stepped lanes on one GPU around the plugin's own Q-network and trainer (algorithms/r2d2.py).

The reference runs ONE environment per actor (srl/algorithms/r2d2/r2d2.py:221-367): one batch-1 LSTM pass per step, a window of L = burnin + sequence_length + 1
states shifted through Python lists and stored whole on every step.  Here every per-actor quantity is a per-lane device array:

    the acting pass (:283-285)                                        ONE forward of q_online over [E][1] inputs with the lanes' (h, c) (SrlxLstm for E <= 256)
    epsilon-greedy probabilities and the roulette draw (:286-289)     srlx_rng_uniform + srlx_r2d2_policy: the action and the probability it was drawn with
    the shifted window lists and their padding (:264-281, :293-320)   the lane ring: srlx_r2d2_lane_push stores each step once, a window is a view
    the sequence replay and the update                                r2d2.Memory's priority memory over the ring (`LaneMemory`) + r2d2.Trainer, unchanged

The engine trains the Parameter it is given in place (torch networks), so nothing has to be exported.  Invalid-action masks come from the batch environment's
optional `invalid_mask()`; an environment without it runs unmasked."""
from typing import Optional, Sequence

import numpy as np
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms import r2d2 as plugin
from simple_distributed_rl_amd.device.lane_engine import SequenceLaneEngine
from simple_distributed_rl_amd.device.sequence_store import R2D2LaneStore
from simple_distributed_rl_amd.device.vector_runner import HostVecEnv

_LANE_RING = "this memory reads an engine's lane ring"


class LaneMemory(plugin.Memory):
    """`r2d2.Memory` with an engine's lane ring behind it: the inner priority memory (its tree, its random stream, its eviction order) keeps each emitted
    window's serial as its opaque item, and `sample` returns the `SequenceBatch` the ring gathers for the sampled serials.  Items cannot be added, backed up
    or restored here; the plugin path's `r2d2.Memory` is untouched."""

    def __init__(self, *args):
        super().__init__(*args)
        self._store = None

    def attach_lane_store(self, store) -> None:
        if self._store is not None or self.memory.length() > 0:
            raise RuntimeError("attach_lane_store: the memory already holds sequences (or a ring); hand it the lane ring before anything is added")
        if self.cfg.enable_demo_memory:
            raise ValueError("attach_lane_store: enable_demo_memory keeps demonstration items in a host ring of its own; use the plugin path")
        if store.ledger.seq_capacity != self.cfg.capacity:
            raise ValueError(f"attach_lane_store: the lane ring keeps {store.ledger.seq_capacity} live windows, the memory's capacity is {self.cfg.capacity}")
        self._store = store

    def add_serial(self, serial: int, priority=None) -> None:
        """A window the attached lane ring emitted: its serial is the inner priority memory's item."""
        if self._store is None:
            raise RuntimeError("add_serial: no lane ring is attached (attach_lane_store)")
        self.memory.add(int(serial), priority)

    def add(self, batch, priority=None, serialized: bool = False) -> None:
        raise RuntimeError(f"r2d2 lane memory: {_LANE_RING}; items are pushed there, not added here")

    def sample(self, step: int = -1, batch_size: int = -1):
        if self._store is None:
            raise RuntimeError("r2d2 lane memory: no lane ring is attached (attach_lane_store)")
        if self.memory.length() < self.cfg.warmup_size:
            return None
        serials, weights, update_args = self.memory.sample(batch_size if batch_size > -1 else self.batch_size, step if step > -1 else self.step)
        return self._store.gather_serials(serials), np.asarray(weights, dtype=self.dtype), update_args

    def call_backup(self, **kwargs):
        raise RuntimeError(f"r2d2 lane memory: {_LANE_RING}, which has no backup format yet (its windows are views of rings the running lanes still write); "
                           "back up a plugin-path memory instead")

    def call_restore(self, data, **kwargs) -> None:
        raise RuntimeError(f"r2d2 lane memory: {_LANE_RING}, which has no restore yet (its windows are views of rings the running lanes still write); "
                           "restore into a plugin-path memory instead")


class MaskedHostVecEnv(HostVecEnv):
    """`HostVecEnv` with `invalid_mask()`: uint8 [E][A] on the device, from each copy's `get_invalid_actions()`, for the observations `reset` / `step` last
    returned.  Everything else is the base class's."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.A = int(self.envs[0].action_space.n)
        self._host_mask = torch.zeros((self.E, self.A), dtype=torch.uint8).pin_memory()
        self._mask = torch.zeros((self.E, self.A), dtype=torch.uint8, device=self.dev)

    def invalid_mask(self) -> torch.Tensor:
        from simple_distributed_rl_amd.device.sequence_store import fill_invalid_mask

        torch.cuda.current_stream(self.dev).synchronize()  # (the previous upload has read the pinned rows)
        fill_invalid_mask(self._host_mask.numpy(), [env.get_invalid_actions() for env in self.envs])
        self._mask.copy_(self._host_mask, non_blocking=True)
        return self._mask


class R2D2Engine(SequenceLaneEngine):
    """E environments + the plugin trainer on one GPU, training only (evaluation plays the trained Parameter on the plugin path).  `rl_config`: a set-up
    algorithms.r2d2.Config (window_length 1); `parameter`: its Parameter, created here when not given; `env`: a batch environment of `HostVecEnv`'s contract
    with float32 observations and, optionally, `invalid_mask()`, or a callable that makes one from an object with `.dev` and `.obs_uint8 == False`;
    `lane_epsilon`: E floats that override `rl_config.epsilon` per lane."""

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, ring_len: Optional[int] = None, context=None,
                 lane_epsilon: Optional[Sequence[float]] = None):
        self._open_sequence(rl_config, n_envs, device, seed, parameter, env)
        c, E, d = self.cfg, self.E, self.dev
        self.lib = N.lib()
        self._attach_ring(LaneMemory(c), R2D2LaneStore(d, E, c.memory.capacity, self.L, self.S, self.A, self.H, self.obs_shape, seed=self.seed ^ 0x2D2, ring_len=ring_len),
                           context)
        if lane_epsilon is None:
            lane_epsilon = [c.epsilon] * E
        if len(lane_epsilon) != E:
            raise ValueError(f"R2D2Engine: lane_epsilon has {len(lane_epsilon)} entries, the engine has {E} lanes")
        self.eps = torch.tensor(np.asarray(lane_epsilon, np.float32), device=d)
        self.mu = torch.zeros(E, dtype=torch.float32, device=d)
        self.hidden = tuple(torch.zeros((1, E, self.H), dtype=torch.float32, device=d) for _ in range(2))
        self.u_policy = torch.zeros(E, dtype=torch.float64, device=d)
        self._reset_lanes(env)
        self.masked = hasattr(self.env, "invalid_mask")
        self.mask = self.env.invalid_mask() if self.masked else None  # of `obs`
        zf = torch.zeros(E, dtype=torch.float32, device=d)
        self._push_first_frames(self.obs.contiguous(), self.actions, zf, zf, torch.zeros(E, dtype=torch.uint8, device=d), invalid=self.mask)

    def _hidden_rows(self):
        return tuple(t[0].contiguous() for t in self.hidden)

    # ---- actor ----------------------------------------------------------------------------------
    def policy_q(self) -> torch.Tensor:
        """One forward of the online network over [E][1] inputs from the lanes' recurrent state (:283-285); the state moves on.  Returns q float32 [E][A]."""
        net = self.parameter.q_online
        with torch.no_grad():
            net.eval()
            q, self.hidden = net(self.obs.view(self.E, 1, *self.obs_shape), self.hidden)
        return q[:, 0].contiguous()

    def actor_step(self):
        """One lock-step of all lanes: action values, the roulette draw, environments, ring push, priority adds."""
        E, st = self.E, N.torch_stream_ptr()
        t0 = self._clock()
        q = self.policy_q()
        N.check(self.lib.srlx_rng_uniform(self.seed ^ 0xAC7, N.tptr(self.policy_counter), E, N.tptr(self.u_policy), st))
        N.check(self.lib.srlx_r2d2_policy(E, self.A, N.tptr(q), N.tptr(self.eps), N.tptr(self.u_policy), N.tptr(self.mask), N.tptr(self.actions), N.tptr(self.mu), st))
        if self.record is not None:
            self.record.append(dict(q=q.cpu().numpy(), mask=None if self.mask is None else self.mask.cpu().numpy(), u=self.u_policy.cpu().numpy(),
                                    eps=self.eps.cpu().numpy(), actions=self.actions.cpu().numpy(), mu=self.mu.cpu().numpy(), first=self._first_host.copy(),
                                    obs=self.obs.cpu().numpy()))
        next_obs, rewards, terminated, done = self.env.step(self.actions)
        next_obs = next_obs.view(E, -1)
        mask = self.env.invalid_mask() if self.masked else None  # of `next_obs`
        if self.ledger is not None:
            self.ledger.account(rewards, done, N.tptr(self.reset_lane))
        first = self.reset_lane.bool()  # lanes whose lock-step only delivered a new episode's first frame: they took no action
        # a lane that begins an episode consumes its first frame from the zero state (on_reset :273)
        self.hidden = self._zero_first(self.hidden, first)
        if self.record is not None:
            h, c = self._hidden_rows()
            self.record[-1].update(next_obs=next_obs.cpu().numpy(), reward=rewards.cpu().numpy(), terminated=terminated.cpu().numpy(), done=done.cpu().numpy(),
                                   next_mask=None if mask is None else mask.cpu().numpy(), hidden=torch.stack([h, c], dim=1).cpu().numpy())
        t0 = self._tick("actor", t0)
        self._push(next_obs.contiguous(), self.actions, self.mu, rewards.contiguous(), terminated.contiguous(), invalid=mask)
        t0 = self._tick("push", t0)
        self.obs, self.mask = next_obs, mask
        self._emit_windows(done, t0)
