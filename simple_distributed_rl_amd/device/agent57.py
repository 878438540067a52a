"""Device engine of Agent57 (the LSTM one): E lock-stepped lanes on one GPU around the plugin's own networks and trainer.

The reference runs ONE environment per actor (srl/algorithms/agent57/agent57.py:404-663): two batch-1 LSTM passes per step, a window of
L = burnin + sequence_length + 1 steps shifted through Python lists and stored whole on every step.  Here every per-actor quantity is a per-lane device array:

    the two Q-networks' acting pass (:516-541)                       ONE forward each over [E][1] inputs with the lanes' recurrent state (SrlxLstm for E <= 256)
    sliding-window UCB over the actor family (:499-514)              UcbBank (srlx_agent57_ucb_step), one controller per lane
    epsilon-greedy on q_ext + beta[arm] q_int (:536-541)             srlx_rng_uniform + srlx_policy_epsilon_greedy
    NGU intrinsic reward on the next observation (:559-563)          NguOps with its reset / active masks (E episodic memories)
    the shifted window lists and their padding (:423-497, :583-610)  the lane ring: srlx_seq_lane_push stores each step once, a window is a view
    the sequence replay and the update                               agent57.Memory (sequence_store "device") over the ring + agent57.Trainer, unchanged

The engine trains the Parameter it is given in place (torch networks), so nothing has to be exported.  The lanes carry no invalid-action lists."""
from typing import Optional

import numpy as np
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.algorithms._device_ops import NguOps
from simple_distributed_rl_amd.device.agent57_light import UcbBank
from simple_distributed_rl_amd.device.lane_engine import SequenceLaneEngine
from simple_distributed_rl_amd.device.sequence_store import LaneSequenceStore
from simple_distributed_rl_amd.rl import functions as funcs


class Agent57Engine(SequenceLaneEngine):
    """E environments + the plugin trainer on one GPU, training only (evaluation plays the trained Parameter on the plugin path).  `rl_config`: a set-up algorithms.agent57.Config (window_length 1); `parameter`: its Parameter, created
    here when not given; `env`: a batch environment of `HostVecEnv`'s contract with float32 observations, or a callable that makes one from an object with
    `.dev` and `.obs_uint8 == False`."""

    def __init__(self, rl_config, n_envs: int, device: int = 0, seed: int = 0, env=None, parameter=None, ring_len: Optional[int] = None, context=None):
        from simple_distributed_rl_amd.algorithms import agent57 as plugin

        self._open_sequence(rl_config, n_envs, device, seed, parameter, env)
        c, E, d, p = self.cfg, self.E, self.dev, self.parameter
        self.lib = N.lib()
        self._attach_ring(plugin.Memory(c, sequence_store="device"),
                           LaneSequenceStore(d, E, c.memory.capacity, self.L, self.S, self.A, self.H, self.obs_shape, seed=self.seed ^ 0x57A, ring_len=ring_len), context)
        Na = c.actor_num
        self.beta_list = torch.tensor(np.array(funcs.create_beta_list(Na), np.float32), device=d)
        self.eps_list = torch.tensor(np.array(funcs.create_epsilon_list(Na), np.float32), device=d)
        self.actor_eye = torch.eye(Na, dtype=torch.float32, device=d)
        self.action_eye = torch.eye(self.A, dtype=torch.float32, device=d)
        self.ucb = UcbBank(E, Na, c.ucb_window_size, c.ucb_epsilon, c.ucb_beta, d, self.seed)
        self.ngu = None
        if c.enable_intrinsic_reward:
            self.ngu = NguOps(d, E, p.emb_network.emb_block.out_size, c.episodic_memory_capacity, c.episodic_count_max, c.episodic_epsilon,
                              c.episodic_cluster_distance, c.episodic_pseudo_counts)
        # per-lane actor state (the reference keeps these on the worker object, :423-452)
        z = lambda dt: torch.zeros(E, dtype=dt, device=d)  # noqa: E731
        self.episode_reward, self.prev_r_ext, self.prev_r_int = z(torch.float32), z(torch.float32), z(torch.float32)
        self.prev_action = z(torch.int64)
        self.hidden_ext = tuple(torch.zeros((1, E, self.H), dtype=torch.float32, device=d) for _ in range(2))
        self.hidden_int = tuple(torch.zeros((1, E, self.H), dtype=torch.float32, device=d) for _ in range(2))
        self.u_policy = torch.zeros(2 * E, dtype=torch.float64, device=d)
        self.gen = torch.Generator(device=d)
        self.gen.manual_seed(self.seed + 17)
        self._reset_lanes(env)
        self._begin_episodes(None)
        zf = z(torch.float32)
        self._push_first_frames(self.obs.contiguous(), self.actions, zf, zf, zf, self.ucb.arm.to(torch.int32))

    # ---- helpers --------------------------------------------------------------------------------
    def _hidden_rows(self):
        return tuple(t[0].contiguous() for t in self.hidden_ext + self.hidden_int)

    def _begin_episodes(self, done: Optional[torch.Tensor]):
        """on_reset (:438-450) for the lanes in `done` (None = all): the episode is booked with the lane's UCB controller and the next arm drawn; random previous
        action, zero previous rewards.  The recurrent state and the episodic memory restart on the lock-step that delivers the new first frame."""
        self.ucb.step(done, self.episode_reward)
        rnd_a = torch.randint(0, self.A, (self.E,), device=self.dev, generator=self.gen)
        if done is None:
            self.prev_action.copy_(rnd_a)
            self.prev_r_ext.zero_()
            self.prev_r_int.zero_()
            self.episode_reward.zero_()
        else:
            m = done.bool()
            zero = torch.zeros_like(self.prev_r_ext)
            self.prev_action = torch.where(m, rnd_a, self.prev_action)
            self.prev_r_ext = torch.where(m, zero, self.prev_r_ext)
            self.prev_r_int = torch.where(m, zero, self.prev_r_int)
            self.episode_reward = torch.where(m, zero, self.episode_reward)

    def arm(self) -> torch.Tensor:
        return self.ucb.arm.long()

    # ---- actor ----------------------------------------------------------------------------------
    def policy_q(self):
        """One forward of both online Q-networks over [E][1] inputs from the lanes' recurrent state (:516-534); the state moves on.  Returns q_ext, q_int, q."""
        p, E, arm = self.parameter, self.E, self.arm()
        in_ = [self.obs.view(E, 1, *self.obs_shape), self.prev_r_ext.view(E, 1, 1), self.prev_r_int.view(E, 1, 1), self.action_eye[self.prev_action].view(E, 1, self.A),
               self.actor_eye[arm].view(E, 1, -1)]
        with torch.no_grad():
            p.q_ext_online.eval()
            p.q_int_online.eval()
            q_ext, self.hidden_ext = p.q_ext_online(in_, self.hidden_ext)
            q_int, self.hidden_int = p.q_int_online(in_, self.hidden_int)
        q_ext, q_int = q_ext[:, 0], q_int[:, 0]
        return q_ext, q_int, (q_ext + self.beta_list[arm].view(-1, 1) * q_int).contiguous()

    def actor_step(self):
        """One lock-step of all lanes: arms and action values, actions, environments, intrinsic reward, ring push, priority adds."""
        c, E, st = self.cfg, self.E, N.torch_stream_ptr()
        t0 = self._clock()
        arm = self.arm()
        _, _, q = self.policy_q()
        eps = self.eps_list[arm].contiguous()
        N.check(self.lib.srlx_rng_uniform(self.seed ^ 0xAC7, N.tptr(self.policy_counter), self.u_policy.numel(), N.tptr(self.u_policy), st))
        N.check(self.lib.srlx_policy_epsilon_greedy(E, self.A, N.tptr(q), N.tptr(eps), N.tptr(self.u_policy), None, N.tptr(self.actions), st))
        next_obs, rewards, terminated, done = self.env.step(self.actions)
        next_obs = next_obs.view(E, -1)
        if self.ledger is not None:
            self.ledger.account(rewards, done, N.tptr(self.reset_lane))
        first = self.reset_lane.bool()  # lanes whose lock-step only delivered a new episode's first frame: they took no action
        live = ~first
        r_int = torch.zeros(E, dtype=torch.float32, device=self.dev)
        if c.enable_intrinsic_reward:
            p = self.parameter
            with torch.no_grad():
                p.emb_network.eval()
                p.lifelong_train.eval()
                s = next_obs.view(E, *self.obs_shape)
                episodic = self.ngu.episodic(p.emb_network.predict(s), reset=self.reset_lane, active=live.to(torch.uint8))
                lifelong = self.ngu.lifelong(p.lifelong_target(s), p.lifelong_train(s), c.lifelong_max)
            r_int = torch.where(live, episodic * lifelong, r_int)  # :559-563
        # a lane that begins an episode consumes its first frame from the zero state (on_reset :432-433)
        self.hidden_ext, self.hidden_int = self._zero_first(self.hidden_ext, first), self._zero_first(self.hidden_int, first)
        t0 = self._tick("actor", t0)
        undone = 1.0 - terminated.to(torch.float32)
        self._push(next_obs.contiguous(), self.actions, rewards.contiguous(), r_int, undone, arm.to(torch.int32))
        t0 = self._tick("push", t0)
        # the worker's bookkeeping (:546-566): lanes in a reset lock-step took no action
        self.obs = next_obs
        self.prev_action = torch.where(live, self.actions.long(), self.prev_action)
        self.prev_r_ext = torch.where(live, rewards, self.prev_r_ext)
        self.prev_r_int = torch.where(live, r_int, self.prev_r_int)
        self.episode_reward = self.episode_reward + torch.where(live, rewards, torch.zeros_like(rewards))
        self._begin_episodes(done)  # lanes whose episode just ended: book it with their UCB controller, draw the next arm
        self._emit_windows(done, t0)

    def info(self) -> dict:
        d = super().info()
        if "ext_loss" in d:
            d["loss"] = d["ext_loss"]
        return d
