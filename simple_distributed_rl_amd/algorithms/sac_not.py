"""NoT_SAC, the reference's torch SAC without target networks and without a temperature (srl/algorithms/sac_not/config.py:13-67,
srl/algorithms/sac_not/torch_model.py:23-278), registered as "NoT_SAC:torch".  A Normal head (squashed or plain) acts on continuous spaces, a Gumbel head on
discrete ones: the one off-policy learner of this project that takes a continuous action.

The reference's own code is torch, so this plugin is held to it directly: tests/test_notsac_pinned_cpu.py runs the reference's `Trainer.train()` in a child
interpreter on hand-fed items and requires the losses, both gradient sets and both networks' parameters after one and two steps of this module's "torch"
backend and of the float64 yardstick tests/notsac_reference.py (parity PINNED wherever the reference can be imported).  The libsrlx backend is held to that
yardstick on the GPU.

Networks.  PolicyNetwork (:27-56): in_block -> policy_block -> policy_dist_block.  QNetwork (:59-84): in_block beside act_block = Linear(A or K, act_emb_units)
+ SiLU, the two concatenated, then q_block -> q_out_layer Linear(1).  The module trees and the state-dict keys are the reference's
(`policy_block.hidden_layers.*`, `policy_dist_block.h_layers.0.*` for the Gumbel head, `policy_dist_block.loc_layers.0.*` / `.log_scale_layers.0.*` for the
Normal head, `act_block.0.*`, `q_block.hidden_layers.*`, `q_out_layer.*`), so a state dict moves between the two by key.  The Normal head is ppo_v's block: the
reference builds the same one.

Trainer.train() (:131-191) is DESIGN.md 7r's contract, on one of two backends that implement it alike:
  "srlx"   one libsrlx call, six launches (device/notsac.py, csrc/srlx_notsac.hip), for GPU parameters inside the kernels' envelope;
  "torch"  the reference's step in plain torch float32 with two torch.optim.Adam, for everything else.
`update_backend`, `update_path` and `why_not_srlx_update` work as in ppo_v.Trainer.  `engine_kind(sac_not.Config())` is None: there is no device engine.

The noise is an input.  `train_on_batch(..., noise)` takes a float32 tensor [2][B][K] of standard normals (Normal head) or [2][B][A] of uniforms in [0, 1)
(Gumbel head): plane 0 serves the target's next action, plane 1 the policy step.  With None the trainer draws the planes with torch on the parameter's
device in the reference's order and shapes (torch.normal(zeros, ones) twice, or torch.rand twice).  The Normal sample is loc + exp(log_scale) * e, a multiply
and then an add; on the CPU torch.normal(loc, std) after a manual_seed gives exactly loc + std * e for the e that torch.normal(0, 1) gives after the same seed,
so a seeded CPU run of the "torch" backend reproduces the reference's seeded draws.

What is kept from the reference although it reads oddly:
  * The target is the FIRST argument of HuberLoss and MSELoss (:164-165); q is their second and takes the gradient.
  * The policy step (:177-189) runs through the Q-network that was already stepped in the same train().
  * The policy step's backward also leaves gradients on the Q-network, which nobody reads (the next train() zeroes them).
  * `target_policy_temperature` divides the noisy logits before an argmax (:153) and so changes nothing for T > 0.
  * `rsample` is called with temperature 1 (:178).
  * `target_policy_noise_stddev` and `target_policy_clip_range` are configured and never read.
  * There is no log-probability and no entropy term anywhere.
Stated departures:
  * The "srlx" backend takes the action of a discrete item as the index of its one-hot's maximum: exact for everything the Worker stores.
  * The "srlx" backend evaluates exp, tanh, SiLU, softmax and the Gumbel transform in float64 and every sum in float64 (rounded to float32 once)."""
import random
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch
import torch.nn as nn

from simple_distributed_rl_amd.algorithms._device_ops import SrlxUpdateBackend
from simple_distributed_rl_amd.algorithms.ppo_v import NormalDistBlock
from simple_distributed_rl_amd.base.exception import UndefinedError
from simple_distributed_rl_amd.base.rl.algorithms.base_ppo import RLConfig, RLWorker
from simple_distributed_rl_amd.base.rl.parameter import RLParameter
from simple_distributed_rl_amd.base.rl.registration import register
from simple_distributed_rl_amd.base.rl.trainer import RLTrainer
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
from simple_distributed_rl_amd.base.spaces.np_array import NpArraySpace
from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig, RLReplayBuffer
from simple_distributed_rl_amd.rl.models.config import HiddenBlockConfig, InputBlockConfig
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig


@dataclass
class Config(RLConfig):
    """config.py:13-67, field for field."""

    epsilon: float = 0.1
    test_epsilon: float = 0
    policy_training_scale: float = 0.5
    batch_size: int = 64
    memory: ReplayBufferConfig = field(default_factory=lambda: ReplayBufferConfig())
    input_block: InputBlockConfig = field(default_factory=lambda: InputBlockConfig())
    policy_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig())
    q_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig())
    act_emb_units: int = 64
    lr: float = 0.0001
    lr_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    discount: float = 0.95
    target_policy_temperature: float = 2.0
    target_policy_noise_stddev: float = 0.2
    target_policy_clip_range: float = 0.5
    loss_align_coeff: float = 0.1
    max_grad_norm: float = 10.0
    squashed_gaussian_policy: bool = True
    enable_stable_gradients: bool = True
    stable_gradients_scale_range: tuple = (1e-10, 10)

    def set_model(self, units: int = 64):
        self.policy_block.set((units, units))
        self.q_block.set((units, units))
        self.act_emb_units = units

    def get_name(self) -> str:
        return "NoT_SAC"

    def get_framework(self) -> str:
        return "torch"


register(Config(), *[__name__ + ":" + c for c in ("Memory", "Parameter", "Trainer", "Worker")], check_duplicate=False)


class Memory(RLReplayBuffer):
    """Items: [state, next_state, action, reward, not_done, total_reward] (:238-251)."""


# ---- the Gumbel head (srl/rl/torch_/distributions/categorical_gumbel_dist_block.py) -----------------------------------------------------------------------------
def gumbel_inverse(u, eps: float = 1e-6):
    """categorical_gumbel_dist_block.py:10-12."""
    return -torch.log(-torch.log(u + eps) + eps)


class CategoricalGumbelDist:
    """categorical_gumbel_dist_block.py:15-60 (what NoT_SAC uses of it).  `noise`: the uniforms to use instead of a fresh torch.rand_like draw."""

    def __init__(self, logits):
        self.classes = logits.shape[-1]
        self.logits = logits

    def probs(self, temperature: float = 1.0):
        return torch.softmax(self.logits / temperature, dim=-1)

    def _noisy(self, noise):
        u = torch.rand_like(self.logits) if noise is None else noise
        return self.logits + gumbel_inverse(u)

    def sample(self, temperature: float = 1.0, onehot: bool = False, noise=None):
        act = torch.argmax(self._noisy(noise) / temperature, dim=-1)
        return torch.nn.functional.one_hot(act, num_classes=self.classes).float() if onehot else act.unsqueeze(-1)

    def rsample(self, temperature: float = 1.0, noise=None):
        return torch.softmax(self._noisy(noise) / temperature, dim=-1)


class CategoricalGumbelDistBlock(nn.Module):
    """categorical_gumbel_dist_block.py:93-116 with no hidden layers of its own: what NoT_SAC builds (:37-40)."""

    def __init__(self, in_size: int, classes: int):
        super().__init__()
        self.classes = classes
        self.h_layers = nn.ModuleList([nn.Linear(in_size, classes)])

    def forward(self, x):
        return CategoricalGumbelDist(self.h_layers[0](x))


class PolicyNetwork(nn.Module):
    """:27-56."""

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        self.policy_block = config.policy_block.create_torch_block(self.in_block.out_size)
        space = config.action_space
        if isinstance(space, DiscreteSpace):
            self.is_discrete = True
            self.policy_dist_block = CategoricalGumbelDistBlock(self.policy_block.out_size, space.n)
        elif isinstance(space, NpArraySpace):
            self.is_discrete = False
            self.policy_dist_block = NormalDistBlock(self.policy_block.out_size, space.size, enable_stable_gradients=config.enable_stable_gradients,
                                                     stable_gradients_scale_range=config.stable_gradients_scale_range)
        else:
            raise UndefinedError(space)

    def forward(self, x):
        return self.policy_dist_block(self.policy_block(self.in_block(x)))


class QNetwork(nn.Module):
    """:59-84."""

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        space = config.action_space
        self.act_block = nn.Sequential(nn.Linear(space.n if isinstance(space, DiscreteSpace) else space.size, config.act_emb_units), nn.SiLU())
        self.q_block = config.q_block.create_torch_block(self.in_block.out_size + config.act_emb_units)
        self.q_out_layer = nn.Linear(self.q_block.out_size, 1)

    def forward(self, x, action):
        x = torch.cat([self.in_block(x), self.act_block(action)], dim=-1)
        return self.q_out_layer(self.q_block(x))


class Parameter(RLParameter):
    """:87-105."""

    def setup(self):
        self.np_dtype = self.config.get_dtype("np")
        self.device = torch.device(self.config.used_device_torch)
        self.policy = PolicyNetwork(self.config).to(self.device)
        self.qnet = QNetwork(self.config).to(self.device)

    def call_restore(self, data: Any, from_serialized: bool = False, **kwargs) -> None:
        # (in place: the libsrlx backend holds these tensors by address)
        self.policy.load_state_dict(data[0])
        self.qnet.load_state_dict(data[1])

    def call_backup(self, serialized: bool = False, **kwargs) -> Any:
        out = []
        for net in (self.policy, self.qnet):
            sd = net.state_dict()
            out.append({k: v.detach().to("cpu").clone() for k, v in sd.items()} if serialized else sd)
        return out

    def to_device(self, device):
        """Moves every tensor; the tensors are new ones afterwards (call before a Trainer binds them)."""
        self.device = torch.device(device)
        self.policy.to(self.device)
        self.qnet.to(self.device)

    def summary(self, **kwargs):
        print(self.policy)
        print(self.qnet)


class Trainer(SrlxUpdateBackend, RLTrainer):
    # "srlx" | "torch".  The default follows the project's 1.10 rule: 1.45 ms per train() on "srlx" against 3.41 ms on "torch" at sac_not.Config()
    # on Pendulum (profiles/notsac_probe.json).  At the envelope's largest corner "torch" is the faster one (54.8 against 3 to 6 ms): set it there.
    update_backend = "srlx"

    def on_setup(self) -> None:
        cfg = self.config
        self.device = torch.device(cfg.used_device_torch)
        if self.parameter.device != self.device:
            self.parameter.to_device(self.device)
        self.np_dtype = cfg.get_dtype("np")
        self.discrete = isinstance(cfg.action_space, DiscreteSpace)
        self._reset_backend()

    # ---- the backends -----------------------------------------------------------------------------------------------------------------------------------
    def _srlx_update_class(self):
        from simple_distributed_rl_amd.device.notsac import NotSacUpdate

        return NotSacUpdate

    def _make_torch_update(self) -> None:
        cfg, p = self.config, self.parameter
        self.opt_q = torch.optim.Adam(p.qnet.parameters(), lr=cfg.lr)  # :110-114
        self._sched_q = cfg.lr_scheduler.apply_torch_scheduler(self.opt_q)
        self.opt_policy = torch.optim.Adam(p.policy.parameters(), lr=cfg.lr)
        self._sched_policy = cfg.lr_scheduler.apply_torch_scheduler(self.opt_policy)
        self.huber_loss, self.mse_loss = nn.HuberLoss(), nn.MSELoss()

    def draw_noise(self, batch: int) -> torch.Tensor:
        """float32 [2][B][K or A] on the parameter's device, in the reference's order: the target's draw, then the policy step's."""
        space = self.config.action_space
        d = self.parameter.device
        if self.discrete:
            return torch.stack([torch.rand((batch, space.n), device=d), torch.rand((batch, space.n), device=d)])
        z, o = torch.zeros((batch, space.size), device=d), torch.ones((batch, space.size), device=d)
        return torch.stack([torch.normal(z, o), torch.normal(z, o)])

    def train(self) -> None:
        batches = self.memory.sample()
        if batches is None:
            return
        state, n_state, action, reward, not_terminated, total_reward = zip(*batches)  # :136-148
        B, d, f = len(batches), self.device, self.np_dtype
        col = lambda x: torch.as_tensor(np.asarray(x, dtype=f).reshape(B, -1), device=d)  # noqa: E731
        self.train_on_batch(torch.as_tensor(np.asarray(state, dtype=f), device=d), torch.as_tensor(np.asarray(n_state, dtype=f), device=d), col(action),
                            col(reward), col(not_terminated), col(total_reward))

    def train_on_batch(self, state, n_state, action, reward, not_terminated, total_reward, noise=None) -> dict:
        """One update (:150-191) from device tensors: state / n_state f32 [B][...]; action f32 [B][A] one-hot or [B][K]; reward, not_terminated and
        total_reward f32 [B][1]; noise f32 [2][B][K or A] or None (module docstring)."""
        B = state.shape[0]
        backend = self._backend_for(B)
        if noise is None:
            noise = self.draw_noise(B)
        if backend == "srlx":
            out = self._update_srlx(state, n_state, action, reward, not_terminated, total_reward, noise)
        else:
            out = self._update_torch(state, n_state, action, reward, not_terminated, total_reward, noise)
        self.update_path = backend
        self.train_count += 1
        scalars = out["scalars"].tolist()  # (the one synchronisation of the call)
        self.info["loss_q"], self.info["loss_q_align"], self.info["loss_policy"] = scalars[0], scalars[1], scalars[2]
        return out

    def _update_srlx(self, state, n_state, action, reward, not_terminated, total_reward, noise) -> dict:
        cfg, u = self.config, self._srlx
        B = state.shape[0]
        lr = cfg.lr * cfg.lr_scheduler.factor(u.steps(), cfg.lr)
        act = action.argmax(dim=1).to(torch.int32) if self.discrete else action
        return u.update(state.reshape(B, -1), n_state.reshape(B, -1), act, reward.reshape(B), not_terminated.reshape(B), total_reward.reshape(B), noise, lr,
                        cfg.discount, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy)

    def _update_torch(self, state, n_state, action, reward, not_terminated, total_reward, noise) -> dict:
        cfg, policy, qnet = self.config, self.parameter.policy, self.parameter.qnet
        with torch.no_grad():  # :150-160
            n_p_dist = policy(n_state)
            if self.discrete:
                n_action = n_p_dist.sample(temperature=cfg.target_policy_temperature, onehot=True, noise=noise[0]).to(state.dtype)
            else:
                n_action = n_p_dist.mean() + n_p_dist.stddev() * noise[0]
                if cfg.squashed_gaussian_policy:
                    n_action = torch.tanh(n_action)
            n_q = qnet(n_state, n_action)
            target_q = reward + not_terminated * cfg.discount * n_q
        q = qnet(state, action)  # :163-174
        loss_q = self.huber_loss(target_q, q)
        loss_q_align = self.mse_loss(total_reward, q)
        loss = loss_q + cfg.loss_align_coeff * loss_q_align
        self.opt_q.zero_grad()
        loss.backward()
        norm_q = torch.nn.utils.clip_grad_norm_(qnet.parameters(), max_norm=cfg.max_grad_norm)
        self.opt_q.step()
        if self._sched_q is not None:
            self._sched_q.step()
        p_dist = policy(state)  # :177-189
        if self.discrete:
            pi_action = p_dist.rsample(noise=noise[1])
        else:
            pi_action = p_dist.mean() + p_dist.stddev() * noise[1]
            if cfg.squashed_gaussian_policy:
                pi_action = torch.tanh(pi_action)
        loss_policy = -qnet(state, pi_action).mean()
        self.opt_policy.zero_grad()
        loss_policy.backward()
        norm_p = torch.nn.utils.clip_grad_norm_(policy.parameters(), max_norm=cfg.max_grad_norm)
        self.opt_policy.step()
        if self._sched_policy is not None:
            self._sched_policy.step()
        return {"q": q.detach()[:, 0], "target_q": target_q[:, 0], "next_action": n_action, "pi_action": pi_action.detach(),
                "scalars": torch.stack([loss_q.detach(), loss_q_align.detach(), loss_policy.detach(), norm_q.detach(), norm_p.detach()])}


class Worker(RLWorker):
    """:194-251, on the host."""

    def on_setup(self, worker, context):
        self.np_dtype = self.config.get_dtype("np")

    def _dist(self, worker):
        p = self.parameter
        with torch.no_grad():
            return p.policy(torch.as_tensor(worker.state[np.newaxis, ...].astype(self.np_dtype), device=p.device))

    def policy(self, worker):
        cfg = self.config
        p_dist = self._dist(worker)
        epsilon = cfg.epsilon if self.training else cfg.test_epsilon
        space = cfg.action_space
        if isinstance(space, DiscreteSpace):
            if random.random() < epsilon:  # :209-211
                env_action = self.sample_action()
                self.action = worker.get_onehot_action(env_action)
            else:  # :213-215
                self.action = p_dist.sample(onehot=True).cpu().numpy()[0]
                env_action = int(np.argmax(self.action))
            return env_action
        if isinstance(space, NpArraySpace):
            loc = p_dist.mean().cpu().numpy()[0]
            if self.training:  # :218-221
                self.action = np.random.normal(loc, cfg.policy_training_scale, size=space.size)
            else:
                self.action = loc
            if cfg.squashed_gaussian_policy:  # :226-228
                self.action = np.tanh(self.action)
                return space.rescale_from(self.action, src_low=-1, src_high=1)
            return space.sanitize(space.rescale_from(self.action))  # :230-231
        raise UndefinedError(space)

    def on_step(self, worker):
        if not self.training:
            return
        worker.add_tracking({
            "state": worker.state,
            "next_state": worker.next_state,
            "action": self.action,
            "reward": worker.reward,
            "not_done": int(not worker.terminated),
        })
        if worker.done:  # :247-251
            total_reward = 0
            for b in reversed(worker.get_trackings()):
                total_reward = b[3] + self.config.discount * total_reward
                self.memory.add(b + [total_reward])

    def render_terminal(self, worker, **kwargs) -> None:
        p = self.parameter
        state = torch.as_tensor(worker.state[np.newaxis, ...].astype(self.np_dtype), device=p.device)
        with torch.no_grad():
            p_dist = p.policy(state)
            if isinstance(self.config.action_space, DiscreteSpace):
                probs, logits = p_dist.probs().cpu().numpy()[0], p_dist.logits.cpu().numpy()[0]
                for a in range(len(probs)):
                    q = p.qnet(state, torch.as_tensor(np.array([worker.get_onehot_action(a)]).astype(self.np_dtype), device=p.device))
                    print(f"  {a}: {probs[a] * 100:5.1f}%, logits {logits[a]:7.3f}, q {float(q[0][0]):.5f}")
            else:
                action = p_dist.mean()
                q = p.qnet(state, action)
                for a in range(self.config.action_space.size):
                    print(f"[{a}] mean: {float(action[0][a]):.7f}, stddev: {float(p_dist.stddev()[0][a]):.7f}")
                print(f"q: {float(q[0][0]):.7f}")
