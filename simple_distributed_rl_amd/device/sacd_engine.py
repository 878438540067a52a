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
import time

import numpy as np
import torch

from simple_distributed_rl_amd.device import sacd
from simple_distributed_rl_amd.device.replay import DeviceReplay
from simple_distributed_rl_amd.device.vector_runner import why_not_sacd_engine

MAX_LANES = 4096


class _ConfigSpaces:
    """What `why_not_sacd_engine` asks of an environment, from a set-up config (the engine is handed a batch environment, not an EnvRun)."""

    player_num = 1

    def __init__(self, rl_config):
        self.action_space, self.observation_space = rl_config.action_space, rl_config.observation_space


class SacdEngine:
    """E environments + the plugin trainer on one GPU.  `rl_config`: a set-up algorithms.sac.Config; `parameter`: its Parameter, created here when not given and
    moved to the device; `env`: None for the device CartPole, otherwise a batch environment of `HostVecEnv`'s contract with float32 observations or a callable
    that makes one from the replay."""

    overlap = False

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, context=None):
        c = self.cfg = rl_config
        assert c.is_setup(), "rl_config.setup(env) first: the networks are built from the negotiated spaces"
        why = why_not_sacd_engine(_ConfigSpaces(c), c, n_envs=n_envs)
        if why:
            raise ValueError(f"SacdEngine cannot run this configuration: {why}")
        self.dev = torch.device(f"cuda:{device}")
        self.E, self.seed = int(n_envs), int(seed)
        E, d = self.E, self.dev
        self.D, self.A, self.B = int(c.observation_space.shape[0]), int(c.action_space.n), int(c.batch_size)
        c._set_device(str(d))
        if parameter is None:
            parameter = c.make_parameter()
        parameter.to_device(d)
        self.parameter = parameter
        self.trainer = c.make_trainer(parameter, None)  # (train_on_batch is handed its batch: the plugin memory is not needed)
        self.trainer.update_backend = "srlx"
        self.setup_trainer(context)
        mem = c.memory
        # VectorQEngine's replay for C51: the uniform ReplayBuffer is the alpha = 0 corner of the sum-tree, drawn without replacement
        self.replay = DeviceReplay(E, -(-int(mem.capacity) // E) + 2, self.D, 1, 1, self.A, self.B, False, False, 0.0, 0.4, 1_000_000, 0.0001, int(mem.warmup_size),
                                   self.seed, device, has_duplicate=False, sample_slack=8 if self.B <= 64 else 4 * self.B)
        if env is None:
            from simple_distributed_rl_amd.device.mlpq import CartPoleVecEnv

            assert self.D == 4 and self.A == 2, "SacdEngine: the device CartPole has 4 observation elements and 2 actions; pass a batch environment"
            self.env = CartPoleVecEnv(self.replay)
        else:
            self.env = env(self.replay) if callable(env) else env
        # the backend is chosen now, not at the first update: the acting pass runs on the trainer's own handle (it needs the bound parameters only), and an
        # engine whose update would run in torch is an error, not a slower engine
        self.trainer._choose_backend(self.B)
        if self.trainer._backend != "srlx":
            raise ValueError(f"SacdEngine: the update does not run on libsrlx: {self.trainer.why_not_srlx_update}")
        self.actor = self.trainer._srlx
        self.random_until = math.ceil(c.start_steps / E)  # lock-steps of random actions: the Worker's start_steps, in whole lock-steps
        self.actions = torch.zeros(E, dtype=torch.int32, device=d)
        self.policy_counter = torch.zeros(1, dtype=torch.int64, device=d)
        self.train_count_dev = torch.zeros(1, dtype=torch.int64, device=d)  # (feeds the draw's beta schedule, which alpha = 0 ignores)
        B = self.B
        self.states = torch.zeros((B, self.D), dtype=torch.float32, device=d)
        self.next_states = torch.zeros((B, self.D), dtype=torch.float32, device=d)
        self.onehot = torch.zeros((B, self.A), dtype=torch.float32, device=d)
        self.done = torch.zeros(B, dtype=torch.uint8, device=d)
        self.total_env_steps = 0
        self.lock_steps = 0
        self.ledger = None  # an EpisodeLedger, when a driver wants episode results
        self.phase_times = None  # a dict: the engine then synchronises around its phases and adds up their host seconds (tools/sacd_engine_probe.py)
        # a list: every lock-step then appends what the policy drew and what the ring was handed, as host arrays (the tests).  `first`: the lanes whose lock-step
        # only delivers a new episode's first observation (their previous step ended an episode: the store's needs_reset protocol); they store no item
        self.record = None
        self._first_host = None  # (kept while recording; set `record` before the first lock-step)
        self.first_obs = self.env.reset()
        self.replay.reset_all(self.first_obs)

    # ---- helpers --------------------------------------------------------------------------------
    @property
    def train_count(self) -> int:
        return self.trainer.train_count

    def setup_trainer(self, context=None):
        """`RLTrainer.setup` with the run's context, as the plugin learner does when a run opens."""
        if context is None:
            from simple_distributed_rl_amd.base.context import RunContext

            context = RunContext()
        self.trainer.setup(context)

    def _tick(self, name: str, t0: float) -> float:
        if self.phase_times is None:
            return 0.0
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.phase_times[name] = self.phase_times.get(name, 0.0) + (now - t0)
        return now

    # ---- actor ----------------------------------------------------------------------------------
    def actor_step(self):
        """One lock-step of all lanes, 3 launches on the device CartPole: srlx_sacd_act on the ring's current rows, the environments' step, the ring commit
        (which also writes the next pass's row table and advances the policy counter) -- and the replay's add."""
        r, E = self.replay, self.E
        t0 = time.perf_counter() if self.phase_times is not None else 0.0
        off = r.frame_table_current()  # (no launch: the last commit wrote it)
        rec = None
        if self.record is not None:
            rec = dict(logits=torch.zeros((E, self.A), dtype=torch.float32, device=self.dev), scores=torch.zeros((E, self.A), dtype=torch.float64, device=self.dev))
        self.actor.act(E, r.obs_base, off.view(-1), self.seed ^ 0xAC7, self.policy_counter, self.random_until, self.actions,
                       logits=None if rec is None else rec["logits"], scores=None if rec is None else rec["scores"])
        if rec is not None:
            if self._first_host is None:
                self._first_host = np.zeros(E, bool)
            rec = {k: v.cpu().numpy() for k, v in rec.items()}
            rec.update(counter=int(self.policy_counter.item()), actions=self.actions.cpu().numpy(), first=self._first_host)
        e = self.env
        next_obs, rewards, terminated, done = e.step(self.actions)
        if rec is not None:
            rec.update(next_obs=next_obs.view(E, -1).cpu().numpy(), reward=rewards.cpu().numpy(), terminated=terminated.cpu().numpy(), done=done.cpu().numpy())
            self._first_host = rec["done"].astype(bool)
            self.record.append(rec)
        if self.ledger is not None:  # before the commit: the store's needs_reset view still marks the lanes that only received a first observation
            self.ledger.account(rewards, done, r.needs_reset_ptr)
        r.commit(self.actions, rewards, terminated, done, next_obs, next_table=True, bump=self.policy_counter)
        self.total_env_steps += E
        self.lock_steps += 1
        self._tick("actor", t0)

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
        t0 = time.perf_counter() if self.phase_times is not None else 0.0
        state, onehot, n_state, reward, done, actions = self.draw_batch()
        self.trainer.train_on_batch(state, onehot, n_state, reward, done, actions=actions)
        self.train_count_dev += 1
        self._tick("learner", t0)
        return True

    def step(self, learner_updates: int = 1):
        self.actor_step()
        for _ in range(learner_updates):
            self.learner_step()

    def join_learner(self):
        """(updates run on the caller's stream: nothing to join)"""

    def info(self) -> dict:
        self.replay.check_draws()
        d = dict(self.trainer.info)
        d.update(train_count=self.train_count, memory=self.replay.length(), env_steps=self.total_env_steps)
        return d
