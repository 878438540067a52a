"""Device engine of discrete SAC: E lock-stepped lanes on one GPU around the plugin's own Parameter and Trainer (algorithms/sac.py).

The plugin path plays ONE host environment: per step a policy forward through torch, a numpy Gumbel draw and a Python list memory, per `train()` a `zip` and
five host-to-device copies.  Here every per-actor quantity is a per-lane device array:

    the Worker's policy() (sac.py:334-338)          ONE launch, srlx_sacd_act: logits of the ring's current rows, keyed uniforms, random or Gumbel-max action
    the environments                                the device CartPole (1 launch) or a `HostVecEnv`
    Memory.add (sac.py:342-345)                     `DeviceReplay.commit`: float32 frames, window 1, 1-step items, uniform draws without replacement (C51's mapping)
    Memory.sample + the five uploads                the store's draw + srlx_sacd_ring_batch: the drawn items as the update's dense tensors, nothing leaves HBM
    the update                                      `sac.Trainer.train_on_batch` on its "srlx" backend, unchanged: five launches, its lr schedules, syncs and `info`

The engine trains the Parameter it is given in place, so nothing has to be exported: `runner.evaluate()` plays it on the plugin path.  Training only."""
import math

import torch

from simple_distributed_rl_amd.device import sacd
from simple_distributed_rl_amd.device.lane_engine import FlatLaneEngine
from simple_distributed_rl_amd.device.replay import DeviceReplay
from simple_distributed_rl_amd.device.vector_runner import why_not_sacd_engine


class SacdEngine(FlatLaneEngine):
    """E environments + the plugin trainer on one GPU.  `rl_config`: a set-up algorithms.sac.Config; `parameter`: its Parameter, created here when not given and
    moved to the device; `env`: None for the device CartPole, otherwise a batch environment of `HostVecEnv`'s contract with float32 observations or a callable
    that makes one from the replay."""

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, context=None):
        self._open_flat(rl_config, n_envs, device, seed, parameter, context, why_not_sacd_engine)
        c, E, d, B = self.cfg, self.E, self.dev, self.B
        mem = c.memory
        # VectorQEngine's replay for C51: the uniform ReplayBuffer is the alpha = 0 corner of the sum-tree, drawn without replacement
        self.replay = DeviceReplay(E, -(-int(mem.capacity) // E) + 2, self.D, 1, 1, self.A, B, False, False, 0.0, 0.4, 1_000_000, 0.0001, int(mem.warmup_size),
                                   self.seed, device, has_duplicate=False, sample_slack=8 if B <= 64 else 4 * B)
        self._start_envs(env)
        self.random_until = math.ceil(c.start_steps / E)  # lock-steps of random actions: the Worker's start_steps, in whole lock-steps
        self.train_count_dev = torch.zeros(1, dtype=torch.int64, device=d)  # (feeds the draw's beta schedule, which alpha = 0 ignores)
        self.states = torch.zeros((B, self.D), dtype=torch.float32, device=d)
        self.next_states = torch.zeros((B, self.D), dtype=torch.float32, device=d)
        self.onehot = torch.zeros((B, self.A), dtype=torch.float32, device=d)
        self.done = torch.zeros(B, dtype=torch.uint8, device=d)

    # ---- actor ----------------------------------------------------------------------------------
    def actor_step(self):
        """One lock-step of all lanes, 3 launches on the device CartPole: srlx_sacd_act on the ring's current rows, the environments' step, the ring commit
        (which also writes the next pass's row table and advances the policy counter) -- and the replay's add."""
        r, E = self.replay, self.E
        t0 = self._clock()
        off = r.frame_table_current()  # (no launch: the last commit wrote it)
        rec = None if self.record is None else self._record_buffers("scores")
        self.actor.act(E, r.obs_base, off.view(-1), self.seed ^ 0xAC7, self.policy_counter, self.random_until, self.actions,
                       logits=None if rec is None else rec["logits"], scores=None if rec is None else rec["scores"])
        if rec is not None:
            rec = self._record_policy(rec)
        next_obs, rewards, terminated, done = self._env_step(rec)
        r.commit(self.actions, rewards, terminated, done, next_obs, next_table=True, bump=self.policy_counter)
        self._end_lock_step("actor", t0)

    # ---- learner --------------------------------------------------------------------------------
    def draw_batch(self):
        """The store's draw and srlx_sacd_ring_batch: the five tensors of `train_on_batch` (and the int32 actions), device tensors the next draw overwrites."""
        r = self.replay
        b = r.sample_items(self.train_count_dev, all_states=True)
        sacd.ring_batch(self.B, self.D, self.A, r.obs_base, r.frame_off_all, b.actions, b.rewards, b.terminated, self.states, self.next_states, self.onehot, self.done)
        return self.states, self.onehot, self.next_states, b.rewards.view(-1), self.done, b.actions.view(-1)

    def learner_step(self) -> bool:
        """One update of the plugin's trainer on a batch drawn from the ring; False while the replay is warming up."""
        if self.replay.is_warmup_needed():
            return False
        t0 = self._clock()
        state, onehot, n_state, reward, done, actions = self.draw_batch()
        self.trainer.train_on_batch(state, onehot, n_state, reward, done, actions=actions)
        self.train_count_dev += 1
        self._tick("learner", t0)
        return True

    def info(self) -> dict:
        self.replay.check_draws()
        return super().info()
