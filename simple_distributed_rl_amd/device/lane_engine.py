"""The host-side scaffold of the engines that wrap a plugin's own Parameter and Trainer in E lock-stepped lanes, updates on the caller's stream:
`SequenceLaneEngine` for the pair that trains on windows of a lane ring (device/agent57.py, device/r2d2.py), `FlatLaneEngine` for the pair that trains on flat
transitions through the trainer's libsrlx update (device/sacd_engine.py, device/vppo_engine.py).  Nothing here knows a policy, a store's fields or a draw: an
engine's `__init__` calls its half's opening steps in order between its own lines (`_open_sequence`, `_attach_ring`, `_reset_lanes`; `_open_flat`, `_start_envs`), and its `actor_step` / `learner_step` call the helpers.  (The overlapped engines
have device/lockstep.py.)"""
import time

import numpy as np
import torch

MAX_LANES = 4096  # (the flat pair's lane count; device/vector_runner.py's why_not_* refuse more)


class _ObsRingStub:
    """What a batch-environment factory asks of the engine's replay: float32 observations on this device."""

    obs_uint8 = False

    def __init__(self, dev):
        self.dev = dev


class _MemoryView:
    """What the loop and the learner driver ask of `engine.replay`: the priority memory's length and warm-up."""

    def __init__(self, memory):
        self._memory = memory

    def length(self) -> int:
        return self._memory.length()

    def is_warmup_needed(self) -> bool:
        return self._memory.is_warmup_needed()


class _ConfigSpaces:
    """What a `why_not_*_engine` asks of an environment, from a set-up config (the engine is handed a batch environment, not an EnvRun)."""

    player_num = 1

    def __init__(self, rl_config, max_episode_steps=None):
        self.action_space, self.observation_space = rl_config.action_space, rl_config.observation_space
        self.max_episode_steps = max_episode_steps


def _batch_env(env, ring):
    """`env`: a batch environment, or a callable that makes one from the engine's ring."""
    return env(ring) if callable(env) else env


class LaneEngine:
    """E environments + the plugin trainer on one GPU: the opening, the counters, the phase timer and the lock-step loop of all four engines."""

    overlap = False

    def _open(self, rl_config, n_envs: int, device: int, seed: int, parameter, why_not=None):
        """The device, the lane count, the seed, and the Parameter (created here when not given) on the device.  `why_not`: a callable that says why the engine
        cannot run the set-up config ('' when it can); its words are the refusal's."""
        c = self.cfg = rl_config
        assert c.is_setup(), "rl_config.setup(env) first: the networks are built from the negotiated spaces"
        why = why_not() if why_not is not None else ""
        if why:
            raise ValueError(f"{type(self).__name__} cannot run this configuration: {why}")
        self.dev = torch.device(f"cuda:{device}")
        self.E, self.seed = int(n_envs), int(seed)
        c._set_device(str(self.dev))
        if parameter is None:
            parameter = c.make_parameter()
        parameter.to_device(self.dev)
        self.parameter = parameter

    def _open_trainer(self, memory, context):
        """The plugin's trainer over `memory`, set up for the run, and the state every engine keeps."""
        self.trainer = self.cfg.make_trainer(self.parameter, memory)
        self.setup_trainer(context)
        self.actions = torch.zeros(self.E, dtype=torch.int32, device=self.dev)
        self.policy_counter = torch.zeros(1, dtype=torch.int64, device=self.dev)  # the policy stream is keyed by (seed ^ 0xAC7, this counter)
        self.total_env_steps = 0
        self.lock_steps = 0
        self.ledger = None  # an EpisodeLedger, when a driver wants episode results
        self.phase_times = None  # a dict: the engine then synchronises around its phases and adds up their host seconds (the engine's probe under tools/)
        self.record = None  # a list: every lock-step then appends what the policy saw and drew, as host arrays (the engines' tests)

    @property
    def train_count(self) -> int:
        return self.trainer.train_count

    def setup_trainer(self, context=None):
        """`RLTrainer.setup` with the run's context, as the plugin learner does when a run opens (fresh optimisers; the memory and the networks stay)."""
        if context is None:
            from simple_distributed_rl_amd.base.context import RunContext

            context = RunContext()
        self.trainer.setup(context)

    # ---- the phase timer ------------------------------------------------------------------------
    def _clock(self) -> float:
        """Where a timed phase begins: the clock is read only while `phase_times` collects."""
        return time.perf_counter() if self.phase_times is not None else 0.0

    def _tick(self, name: str, t0: float) -> float:
        if self.phase_times is None:
            return 0.0
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.phase_times[name] = self.phase_times.get(name, 0.0) + (now - t0)
        return now

    def _end_lock_step(self, name: str, t0: float):
        self.total_env_steps += self.E
        self.lock_steps += 1
        if self.phase_times is not None:
            self._tick(name, t0)

    # ---- the loop -------------------------------------------------------------------------------
    def step(self, learner_updates: int = 1):
        self.actor_step()
        for _ in range(learner_updates):
            self.learner_step()

    def join_learner(self):
        """(updates run on the caller's stream: nothing to join)"""


class SequenceLaneEngine(LaneEngine):
    """The recurrent pair: a lane ring that stores each step once (`self.store`), the plugin's priority memory over its windows' serials (`self.memory`), a host
    environment stepped in a batch.  `reset_lane` (device) / `_first_host` mark the lanes whose lock-step only delivers a new episode's first frame.  The engine
    supplies `_hidden_rows()`: the lanes' recurrent state as the store's trailing push arguments."""

    def _open_sequence(self, rl_config, n_envs, device, seed, parameter, env):
        assert env is not None, f"{type(self).__name__}: a batch environment (HostVecEnv's contract, float32 observations) is required"
        self._open(rl_config, n_envs, device, seed, parameter)
        c = self.cfg
        self.obs_shape = tuple(int(x) for x in c.observation_space.shape)
        self.A, self.H = int(c.action_space.n), int(c.lstm_units)
        self.L, self.S = c.burnin + c.sequence_length + 1, c.sequence_length

    def _attach_ring(self, memory, store, context):
        """The engine's lane ring behind the plugin's memory, and the trainer over that memory."""
        self.memory, self.store = memory, store
        memory.attach_lane_store(store)
        self.replay = _MemoryView(memory)
        self._open_trainer(memory, context)

    def _reset_lanes(self, env):
        """The environments and their first observations; every lane is at position 0, about to deliver its episode's first frame."""
        self.env = _batch_env(env, _ObsRingStub(self.dev))
        self.obs = self.env.reset().view(self.E, -1).to(torch.float32)
        self.reset_lane = torch.ones(self.E, dtype=torch.uint8, device=self.dev)
        self._first_host = np.ones(self.E, bool)

    def _push(self, *fields, **kw):
        self.store.push(*fields, *self._hidden_rows(), first=self._first_host, first_dev=self.reset_lane, **kw)

    def _push_first_frames(self, *fields, **kw):
        """The position-0 push: no lane has taken an action yet, no window is emitted."""
        self._push(*fields, **kw)
        self.store.emit(np.zeros(self.E, bool))
        self.reset_lane = torch.zeros(self.E, dtype=torch.uint8, device=self.dev)
        self._first_host = np.zeros(self.E, bool)

    def _zero_first(self, hidden, first):
        """A lane that begins an episode consumes its first frame from the zero state (the reference's on_reset)."""
        return tuple(torch.where(first.view(1, self.E, 1), torch.zeros_like(t), t) for t in hidden)

    def _emit_windows(self, done, t0: float):
        """After the push: this lock-step's done lanes deliver a first frame next, and every window the ring emitted joins the priority memory."""
        self.reset_lane = done.clone()
        done_host = done.cpu().numpy().astype(bool)  # the host needs the window count
        serials = self.store.emit(done_host)
        self._first_host = done_host
        for s in serials:  # (every emitted window: the memory's oldest item must stay among the ledger's live serials)
            self.memory.add_serial(int(s), None)
        self.last_serials = serials
        self._end_lock_step("adds", t0)

    def learner_step(self) -> bool:
        """One `Trainer.train()` of the plugin: it samples serials from the priority memory, and the memory gathers them from the lane ring."""
        t0 = self._clock()
        before = self.trainer.train_count
        self.trainer.train()
        self._tick("train", t0)
        return self.trainer.train_count > before

    def info(self) -> dict:
        d = dict(train_count=self.train_count, memory=self.memory.length())
        d.update(self.trainer.info)
        return d


class FlatLaneEngine(LaneEngine):
    """The flat pair: observations [D], A discrete actions (or a continuous action of K elements: `self.K` > 0 and `self.A` = K), batches of B drawn from a device
    store (`self.replay`, which the engine makes between `_open_flat` and `_start_envs`) and handed to the trainer's `train_on_batch`, whose libsrlx update
    handle also runs the acting kernel (`self.actor`)."""

    def _open_flat(self, rl_config, n_envs, device, seed, parameter, context, why_not, max_episode_steps=None):
        self._open(rl_config, n_envs, device, seed, parameter, lambda: why_not(_ConfigSpaces(rl_config, max_episode_steps), rl_config, n_envs=n_envs))
        c = self.cfg
        space = c.action_space
        self.K = 0 if hasattr(space, "n") else int(space.size)  # 0: A discrete actions; K > 0: a continuous action of K elements (the head's outputs: A = K)
        self.D, self.A, self.B = int(c.observation_space.shape[0]), int(space.n) if not self.K else self.K, int(c.batch_size)
        self._open_trainer(None, context)  # (train_on_batch is handed its batch: the plugin memory is not needed)

    def _start_envs(self, env, **cartpole_kw):
        """The environments (None: the device CartPole on the store), the acting handle, the first observations."""
        if env is None:
            from simple_distributed_rl_amd.device.mlpq import CartPoleVecEnv

            assert self.D == 4 and self.A == 2, f"{type(self).__name__}: the device CartPole has 4 observation elements and 2 actions; pass a batch environment"
            self.env = CartPoleVecEnv(self.replay, **cartpole_kw)
        else:
            self.env = _batch_env(env, self.replay)
        # the backend is chosen now, not at the first update: the acting pass runs on the trainer's own handle (it needs the bound parameters only), and an
        # engine whose update would run in torch is an error, not a slower engine
        self.actor = self.trainer.require_srlx_update(self.B, type(self).__name__)
        # `record`: `first` marks the lanes whose lock-step only delivers a new episode's first observation (their previous step ended an episode: the store's
        # needs_reset protocol); they store nothing
        self._first_host = None  # (kept while recording; set `record` before the first lock-step)
        self.first_obs = self.env.reset()
        self.replay.reset_all(self.first_obs)

    def _record_buffers(self, name: str):
        """While recording: the device arrays the acting kernel fills beside the actions, `logits` f32 and `name` f64, [E][A] each."""
        return {"logits": torch.zeros((self.E, self.A), dtype=torch.float32, device=self.dev), name: torch.zeros((self.E, self.A), dtype=torch.float64, device=self.dev)}

    def _record_policy(self, rec, **drawn):
        """What the policy drew, as host arrays."""
        if self._first_host is None:
            self._first_host = np.zeros(self.E, bool)
        rec = {k: v.cpu().numpy() for k, v in rec.items()}
        rec.update(counter=int(self.policy_counter.item()), actions=self.actions.cpu().numpy(), **{k: v.cpu().numpy() for k, v in drawn.items()}, first=self._first_host)
        return rec

    def _env_step(self, rec, env_actions=None):
        """The environments' step on `self.actions` (or on `env_actions`, where what the environments take is not what the store keeps); the record gets what they
        returned, the ledger its episodes."""
        next_obs, rewards, terminated, done = self.env.step(self.actions if env_actions is None else env_actions)
        if rec is not None:
            rec.update(next_obs=next_obs.view(self.E, -1).cpu().numpy(), reward=rewards.cpu().numpy(), terminated=terminated.cpu().numpy(), done=done.cpu().numpy())
            self._first_host = rec["done"].astype(bool)
            self.record.append(rec)
        if self.ledger is not None:  # before the store takes the step: its needs_reset view still marks the lanes that only received a first observation
            self.ledger.account(rewards, done, self.replay.needs_reset_ptr)
        return next_obs, rewards, terminated, done

    def info(self) -> dict:
        d = dict(self.trainer.info)
        d.update(train_count=self.train_count, memory=self.replay.length(), env_steps=self.total_env_steps)
        return d
