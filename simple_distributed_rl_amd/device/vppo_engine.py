"""Device engine of V-PPO: E lock-stepped lanes on one GPU around the plugin's own Parameter and Trainer (algorithms/ppo_v.py) on flat
observations: `VppoEngine` for the categorical head, `VppoNormalEngine` for the Normal head (a continuous action of 1..8 elements).

The plugin path plays ONE host environment: per step a torch forward of the whole actor-critic for one row and a torch `Categorical.sample`, a Python tracking
list and a reversed Python walk at episode end, per `train()` a `zip` and seven host-to-device copies.  Here every per-actor quantity is a per-lane device array:

    the Worker's policy() (ppo_v.py: Worker.policy)     ONE launch, srlx_vppo_act on the tracking ring's current row: trunk + policy branch, keyed uniforms,
                                                        the epsilon branch or the inverse CDF, the action's log-probability in the update's own form
    the environments                                    the device CartPole (1 launch) or a `HostVecEnv`
    add_tracking + the walk at episode end (on_step)    `VppoLanes.push`, two launches: the step's fields, then the close of every lane whose step was done
    Memory.sample + the seven uploads                   `VppoLanes.sample`, two launches: Floyd's draw and the items as the update's dense tensors
    the update                                          `ppo_v.Trainer.train_on_batch` on its "srlx" backend with the int32 actions: three launches

The engine trains the Parameter it is given in place, so nothing has to be exported: `runner.evaluate()` plays it on the plugin path.  Training only."""
import functools

import torch

from simple_distributed_rl_amd.device.lane_engine import FlatLaneEngine
from simple_distributed_rl_amd.device.vector_runner import normal_action_bounds, why_not_vppo_engine
from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes


class VppoEngine(FlatLaneEngine):
    """E environments + the plugin trainer on one GPU.  `rl_config`: a set-up algorithms.ppo_v.Config; `parameter`: its Parameter, created here when not given and
    moved to the device; `env`: None for the device CartPole (max_episode_steps 500), otherwise a batch environment of `HostVecEnv`'s contract with float32
    observations or a callable that makes one from the store; `max_episode_steps`: the longest episode the environments play (the tracking ring's depth)."""

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, context=None, max_episode_steps=None):
        if env is None and max_episode_steps is None:
            max_episode_steps = 500
        self._open_flat(rl_config, n_envs, device, seed, parameter, context, why_not_vppo_engine, max_episode_steps)
        c, E, mem = self.cfg, self.E, self.cfg.memory
        # (+ 1: an EnvRun ends an episode when its step count EXCEEDS max_episode_steps (base/env/env_run.py), so a host-stepped lane can store one step more)
        self.replay = VppoLanes(E, self.D, int(max_episode_steps) + 1, int(mem.capacity), self.B, int(mem.warmup_size), float(c.discount), self.seed, device)
        self._start_envs(env, max_steps=int(max_episode_steps))
        self.epsilon = float(c.epsilon)
        self.logp = torch.zeros(E, dtype=torch.float32, device=self.dev)

    # ---- actor ----------------------------------------------------------------------------------
    def actor_step(self):
        """One lock-step of all lanes, 4 launches on the device CartPole: srlx_vppo_act on the tracking ring's current row, the environments' step, the push's two
        (which also advance the policy counter)."""
        r, E = self.replay, self.E
        t0 = self._clock()
        rec = None if self.record is None else self._record_buffers("cdf")
        self.actor.act(E, r.current_row_ptr(), self.seed ^ 0xAC7, self.policy_counter, self.epsilon, self.actions, self.logp,
                       logits=None if rec is None else rec["logits"], cdf=None if rec is None else rec["cdf"])
        if rec is not None:
            rec = self._record_policy(rec, logp=self.logp)
        next_obs, rewards, terminated, done = self._env_step(rec)
        r.push(self.actions, self.logp, rewards, terminated, done, next_obs.view(E, -1), bump=self.policy_counter)
        self._end_lock_step("actor", t0)

    # ---- learner --------------------------------------------------------------------------------
    def draw_batch(self):
        """The store's draw: the seven tensors of `train_on_batch` (the action as int32 [B]) and the drawn slots, device tensors the next draw overwrites."""
        return self.replay.sample()

    def learner_step(self) -> bool:
        """One update of the plugin's trainer on a batch drawn from the item ring; False while the store is warming up."""
        if self.replay.is_warmup_needed():
            return False
        t0 = self._clock()
        state, n_state, actions, old_logpi, reward, not_terminated, total_reward, _ = self.draw_batch()
        self.trainer.train_on_batch(state, n_state, None, old_logpi, reward, not_terminated, total_reward, actions=actions)
        self._tick("learner", t0)
        return True

    def info(self) -> dict:
        self.replay.check()
        return super().info()


class VppoNormalEngine(VppoEngine):
    """`VppoEngine` on the Normal head: the action space is a flat continuous vector of K = 1..8 elements with finite bounds.  The lanes' policy is
    ONE launch of srlx_vppo_act_normal (Box-Muller on keyed uniforms, the epsilon branch, the action before tanh, every element's log-probability in the update's
    own form, the environment's action), the store keeps K float32 action elements and K log-probabilities per step, and the update reads them as they are.
    `env`: None for the device Pendulum (max_episode_steps 200, 3 observation elements, one torque), otherwise a batch environment whose `step` takes float32
    actions [E][K] (`FloatActionHostVecEnv`) or a callable that makes one from the store.  The draw, `learner_step` and `info` are `VppoEngine`'s."""

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, context=None, max_episode_steps=None):
        if env is None and max_episode_steps is None:
            max_episode_steps = 200
        self._open_flat(rl_config, n_envs, device, seed, parameter, context, functools.partial(why_not_vppo_engine, admit_normal=True), max_episode_steps)
        c, E, K, mem = self.cfg, self.E, self.K, self.cfg.memory
        if not K:
            raise ValueError("VppoNormalEngine cannot run this configuration: a discrete action space is VppoEngine's")
        low, high = normal_action_bounds(c.action_space)
        self.low, self.high = torch.from_numpy(low).to(self.dev), torch.from_numpy(high).to(self.dev)
        self.replay = VppoLanes(E, self.D, int(max_episode_steps) + 1, int(mem.capacity), self.B, int(mem.warmup_size), float(c.discount), self.seed, device,
                                action_dim=K)
        self.actions = torch.zeros((E, K), dtype=torch.float32, device=self.dev)  # what the store keeps: the draw before tanh
        self.env_actions = torch.zeros((E, K), dtype=torch.float32, device=self.dev)  # what the environments take
        self.logp = torch.zeros((E, K), dtype=torch.float32, device=self.dev)
        if env is None:
            from simple_distributed_rl_amd.device.mlpq import PendulumLaneVecEnv

            assert self.D == 3 and K == 1, "VppoNormalEngine: the device Pendulum has 3 observation elements and one torque; pass a batch environment"
            env = lambda replay: PendulumLaneVecEnv(replay, max_steps=int(max_episode_steps))  # noqa: E731
        self._start_envs(env)
        self.epsilon, self.noise_scale, self.squashed = float(c.epsilon), float(c.policy_noise_normal_scale), bool(c.squashed_gaussian_policy)

    def actor_step(self):
        """One lock-step of all lanes, 4 launches on the device Pendulum: srlx_vppo_act_normal on the tracking ring's current row, the environments' step on the
        rescaled actions, the push's two (which also advance the policy counter)."""
        r, E, K = self.replay, self.E, self.K
        t0 = self._clock()
        rec = None
        if self.record is not None:
            rec = {"loc": torch.zeros((E, K), dtype=torch.float32, device=self.dev), "log_scale": torch.zeros((E, K), dtype=torch.float32, device=self.dev),
                   "z": torch.zeros((E, K), dtype=torch.float64, device=self.dev)}
        self.actor.act_normal(E, r.current_row_ptr(), self.seed ^ 0xAC7, self.policy_counter, self.epsilon, self.noise_scale, self.squashed, self.low, self.high,
                              self.actions, self.logp, self.env_actions, loc=None if rec is None else rec["loc"], log_scale=None if rec is None else rec["log_scale"],
                              z=None if rec is None else rec["z"])
        if rec is not None:
            rec = self._record_policy(rec, logp=self.logp, env_actions=self.env_actions)
        next_obs, rewards, terminated, done = self._env_step(rec, self.env_actions)
        r.push(self.actions, self.logp, rewards, terminated, done, next_obs.view(E, -1), bump=self.policy_counter)
        self._end_lock_step("actor", t0)

    def learner_step(self) -> bool:
        """One update of the plugin's trainer on a batch drawn from the item ring (the action as float32 [B][K]); False while the store is warming up."""
        if self.replay.is_warmup_needed():
            return False
        t0 = self._clock()
        state, n_state, actions, old_logpi, reward, not_terminated, total_reward, _ = self.draw_batch()
        self.trainer.train_on_batch(state, n_state, actions, old_logpi, reward, not_terminated, total_reward)
        self._tick("learner", t0)
        return True
