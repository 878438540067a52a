"""Soft actor-critic for discrete actions (SAC, https://arxiv.org/abs/1812.05905; srl/algorithms/sac/config.py:30-87, srl/algorithms/sac/sac_tf_discrete.py:20-272),
registered as "SAC_Discrete:torch".

The reference's SAC is a TensorFlow/Keras model (`get_framework() == "tensorflow"`, config.py:82-83) and TensorFlow is not installed, so this module is a
restatement of the cited lines on the torch/ROCm stack, NOT pinned against recorded reference outputs (parity UNPINNED).  The yardstick of the update's
arithmetic is tests/sacd_reference.py, a float64 restatement of sac_tf_discrete.py:158-243 written as a different program.

Only the discrete variant is built.  A continuous action space resolves to "SAC_Continuous:torch", whose Parameter refuses with a sentence: the continuous
family needs float actions in the rings and a continuous base class the project does not have (out of scope).

Networks.  PolicyNetwork: in_block -> policy_block -> `out_layer` (:20-38); the out layer starts at zero as CategoricalGumbelDistBlock's
kernel_initializer="zeros" does, so a fresh policy is uniform.  QNetwork: concat(in_block(state), one-hot action) -> q_block -> Linear(1) (:69-95).

Trainer.train() (:158-243) is DESIGN.md 7m's contract, on one of two backends that implement it alike:
  "srlx"   one libsrlx call, five launches (device/sacd.py, csrc/srlx_sacd.hip), for GPU parameters inside the kernels' envelope;
  "torch"  plain torch float32 with torch.optim.Adam, for everything else.
`update_backend` is an attribute of the class (the default) or of a Trainer; the backend is fixed for a Trainer's life at its first train(), and each backend
owns its Adam state.  `update_path` names the path of the last call, `why_not_srlx_update` the reason a request for "srlx" was served by torch.
`device/sacd_engine.py: SacdEngine` runs E lock-stepped lanes on one GPU around this Parameter and Trainer (`train_on_batch`); `Runner.train()` does
not route there yet.

What is kept from the reference although it reads oddly:
  * target_entropy = -A (:151-156, "-1 * n"), the continuous-control heuristic.  A discrete policy's entropy lies in [0, log A], so target_entropy - entropy is
    always negative, d alpha_loss / d log_alpha = -mean(alpha (target_entropy - entropy)) is always positive, and the automatic temperature only ever falls.
  * The clip is 1e-7 (the reference writes 10e-8), and the next state's log-probabilities are not clipped.
  * The Worker samples when evaluating too (:254-256).
Stated departures:
  * Adam is torch's (betas 0.9 / 0.999, eps 1e-8, eps added outside the bias-corrected root), as in the rest of the project -- not Keras' eps of 1e-7.
  * The next state's log-probabilities are z - logsumexp(z), finite for any logits; the reference's log(softmax(z)) is -inf once a probability underflows and
    its 0 * -inf is NaN.  For logit gaps up to 30 the two agree to rounding.  Both backends do this.
  * The host random stream cannot equal TensorFlow's: the Worker's Gumbel-max sample (noise uniform on [1e-6, 1), categorical_gumbel_dist_block.py:43-50) equals
    the reference's in distribution only."""
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch

from simple_distributed_rl_amd.algorithms._device_ops import SrlxUpdateBackend
from simple_distributed_rl_amd.base.exception import NotSupportedError
from simple_distributed_rl_amd.base.rl.algorithms.base_ppo import RLConfig, RLWorker
from simple_distributed_rl_amd.base.rl.parameter import RLParameter
from simple_distributed_rl_amd.base.rl.registration import register
from simple_distributed_rl_amd.base.rl.trainer import RLTrainer
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig, RLReplayBuffer
from simple_distributed_rl_amd.rl.models.config import HiddenBlockConfig, InputBlockConfig
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig

CONTINUOUS_SENTENCE = ("SAC on a continuous action space (SAC_Continuous) is not built: only SAC_Discrete is, "
                       "the continuous family needs float actions in the replay rings and a continuous base class")


@dataclass
class Config(RLConfig):
    """config.py:30-87, field for field."""

    input_block: InputBlockConfig = field(default_factory=lambda: InputBlockConfig())
    policy_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig().set((64, 64, 64)))
    q_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig().set((128, 128, 128)))
    batch_size: int = 32
    memory: ReplayBufferConfig = field(default_factory=lambda: ReplayBufferConfig())
    discount: float = 0.99
    lr_policy: float = 0.0001
    lr_policy_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    lr_q: float = 0.0001
    lr_q_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    lr_alpha: float = 0.0001
    lr_alpha_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    soft_target_update_tau: float = 0.02
    hard_target_update_interval: int = 10000
    squashed_gaussian_policy: bool = True  # (continuous variant only)
    start_steps: int = 10000
    entropy_alpha_auto_scale: bool = True
    entropy_alpha: float = 0.2
    enable_stable_gradients: bool = True  # (continuous variant only)
    stable_gradients_scale_range: tuple = (1e-10, 10)  # (continuous variant only)

    def get_name(self) -> str:
        space = self.action_space
        return "SAC_Discrete" if space is None or isinstance(space, DiscreteSpace) else "SAC_Continuous"

    def get_framework(self) -> str:
        return "torch"


def _register():
    """sac/__init__.py:7-13: one name per action space.  The continuous name resolves to the same classes, whose Parameter refuses it in words."""
    from simple_distributed_rl_amd.base.spaces.np_array import NpArraySpace

    entries = [__name__ + ":" + c for c in ("Memory", "Parameter", "Trainer", "Worker")]
    register(Config(), *entries, check_duplicate=False)
    continuous = Config()
    continuous._rl_act_space = NpArraySpace(1)
    register(continuous, *entries, check_duplicate=False)


_register()


class Memory(RLReplayBuffer):
    """Items: [state, one-hot action, next_state, reward, terminated] (:264-272)."""


class PolicyNetwork(torch.nn.Module):
    """:20-38."""

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        self.hidden_block = config.policy_block.create_torch_block(self.in_block.out_size)
        self.out_layer = torch.nn.Linear(self.hidden_block.out_size, config.action_space.n)
        torch.nn.init.zeros_(self.out_layer.weight)
        torch.nn.init.zeros_(self.out_layer.bias)

    def forward(self, state):
        """The logits."""
        return self.out_layer(self.hidden_block(self.in_block(state)))


class QNetwork(torch.nn.Module):
    """:69-95."""

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        self.q_block = config.q_block.create_torch_block(self.in_block.out_size + config.action_space.n)
        self.q_out_layer = torch.nn.Linear(self.q_block.out_size, 1)

    def forward(self, state, onehot_action):
        return self.q_out_layer(self.q_block(torch.cat([self.in_block(state), onehot_action], dim=1)))


def all_action_min_q(state, n_actions: int, q1, q2):
    """compute_discrete_all_q (:54-66): min(q1, q2)(s, e_a) for every action, [B][A]."""
    B = state.shape[0]
    rows = state.repeat_interleave(n_actions, dim=0)
    onehot = torch.eye(n_actions, dtype=state.dtype, device=state.device).repeat(B, 1)
    return torch.minimum(q1(rows, onehot), q2(rows, onehot)).view(B, n_actions)


def gumbel_max_sample(logits: np.ndarray, rng=np.random) -> int:
    """categorical_gumbel_dist_block.py:43-50: argmax(logits - log(-log(u))), u uniform on [1e-6, 1)."""
    u = rng.uniform(1e-6, 1.0, size=logits.shape)
    return int(np.argmax(logits - np.log(-np.log(u))))


class Parameter(RLParameter):
    def setup(self):
        if not isinstance(self.config.action_space, DiscreteSpace):
            raise NotSupportedError(CONTINUOUS_SENTENCE)
        self.np_dtype = self.config.get_dtype("np")
        self.device = torch.device(self.config.used_device_torch)
        self.policy = PolicyNetwork(self.config).to(self.device)
        self.q1_online = QNetwork(self.config).to(self.device)
        self.q1_target = QNetwork(self.config).to(self.device)
        self.q2_online = QNetwork(self.config).to(self.device)
        self.q2_target = QNetwork(self.config).to(self.device)
        self.q1_target.load_state_dict(self.q1_online.state_dict())
        self.q2_target.load_state_dict(self.q2_online.state_dict())
        for net in (self.q1_target, self.q2_target):
            net.requires_grad_(False)
        self.log_alpha = torch.tensor(math.log(self.config.entropy_alpha), dtype=torch.float32, device=self.device)
        self.load_log_alpha = False

    def call_restore(self, data: Any, from_serialized: bool = False, **kwargs) -> None:  # :119-126
        # (in place: the libsrlx backend holds these tensors by address)
        self.policy.load_state_dict(data[0])
        self.q1_online.load_state_dict(data[1])
        self.q1_target.load_state_dict(data[1])
        self.q2_online.load_state_dict(data[2])
        self.q2_target.load_state_dict(data[2])
        with torch.no_grad():
            self.log_alpha.copy_(torch.as_tensor(data[3], dtype=torch.float32))
        self.load_log_alpha = False

    def call_backup(self, serialized: bool = False, **kwargs) -> Any:  # :128-134
        nets = [self.policy.state_dict(), self.q1_online.state_dict(), self.q2_online.state_dict()]
        if serialized:
            return [{k: v.detach().to("cpu").clone() for k, v in sd.items()} for sd in nets] + [self.log_alpha.detach().to("cpu").clone()]
        return nets + [self.log_alpha]

    def to_device(self, device):
        """Moves every tensor; the tensors are new ones afterwards (call before a Trainer binds them)."""
        self.device = torch.device(device)
        for net in (self.policy, self.q1_online, self.q1_target, self.q2_online, self.q2_target):
            net.to(self.device)
        self.log_alpha = self.log_alpha.detach().to(self.device)

    def logits(self, state: np.ndarray) -> np.ndarray:
        with torch.no_grad():
            return self.policy(torch.as_tensor(np.asarray(state, dtype=self.np_dtype), device=self.device)).cpu().numpy()


class Trainer(SrlxUpdateBackend, RLTrainer):
    # "srlx" | "torch".  The default follows the project's 1.10 rule: 1.65 ms per train() on "srlx" against 3.58 ms on "torch" at sac.Config() on
    # CartPole (profiles/sacd_probe.json)
    update_backend = "srlx"

    def on_setup(self) -> None:
        cfg = self.config
        self.device = torch.device(cfg.used_device_torch)
        if self.parameter.device != self.device:
            self.parameter.to_device(self.device)
        self.np_dtype = cfg.get_dtype("np")
        self.target_entropy = -1 * cfg.action_space.n  # :151-156
        self._reset_backend()
        self.parameter.load_log_alpha = False

    # ---- the backends -----------------------------------------------------------------------------------------------------------------------------------
    def _srlx_update_class(self):
        from simple_distributed_rl_amd.device.sacd import SacdUpdate

        return SacdUpdate

    def _make_torch_update(self) -> None:
        p, cfg = self.parameter, self.config
        self.q1_optimizer = torch.optim.Adam(p.q1_online.parameters(), lr=cfg.lr_q)
        self.q2_optimizer = torch.optim.Adam(p.q2_online.parameters(), lr=cfg.lr_q)
        self.policy_optimizer = torch.optim.Adam(p.policy.parameters(), lr=cfg.lr_policy)
        self._schedulers = [cfg.lr_q_scheduler.apply_torch_scheduler(self.q1_optimizer), cfg.lr_q_scheduler.apply_torch_scheduler(self.q2_optimizer),
                            cfg.lr_policy_scheduler.apply_torch_scheduler(self.policy_optimizer)]
        self.alpha_optimizer = None

    def train(self) -> None:
        batches = self.memory.sample()
        if batches is None:
            return
        state, action, n_state, reward, done = zip(*batches)
        d = self.device
        state = torch.as_tensor(np.asarray(state, dtype=self.np_dtype), device=d)
        n_state = torch.as_tensor(np.asarray(n_state, dtype=self.np_dtype), device=d)
        action = torch.as_tensor(np.asarray(action, dtype=np.float32), device=d)
        reward = torch.as_tensor(np.asarray(reward, dtype=np.float32), device=d)
        done = torch.as_tensor(np.asarray(done, dtype=np.uint8), device=d)
        self.train_on_batch(state, action, n_state, reward, done)

    def train_on_batch(self, state, onehot_action, n_state, reward, done, actions=None) -> dict:
        """One update (:170-243) from device tensors: state / n_state f32 [B][...], one-hot actions f32 [B][A], reward f32 [B], done u8 [B].  `actions`: the
        same actions as int32 [B], when the caller has them (the device engine's ring does): the libsrlx backend then skips its argmax over the one-hot rows."""
        backend = self._backend_for(state.shape[0])
        cfg = self.config
        hard_sync = self.train_count % cfg.hard_target_update_interval == 0
        if backend == "srlx":
            out = self._update_srlx(state, onehot_action, n_state, reward, done, hard_sync, actions)
        else:
            out = self._update_torch(state, onehot_action, n_state, reward, done, hard_sync)
        self.update_path = backend
        self.train_count += 1
        scalars = out["scalars"].tolist()  # (the one synchronisation of the call)
        self.info["q1_loss"], self.info["q2_loss"], self.info["policy_loss"] = scalars[0], scalars[1], scalars[2]
        if cfg.entropy_alpha_auto_scale:
            self.info["alpha_loss"], self.info["alpha"] = scalars[3], scalars[4]
        return out

    def _update_srlx(self, state, onehot_action, n_state, reward, done, hard_sync: bool, actions=None) -> dict:
        cfg, u = self.config, self._srlx
        if not self.parameter.load_log_alpha:  # :170-173
            u.reset_alpha_optimizer()
            self.parameter.load_log_alpha = True
        steps = u.steps()
        lr_policy = cfg.lr_policy * cfg.lr_policy_scheduler.factor(steps[0], cfg.lr_policy)
        lr_q = cfg.lr_q * cfg.lr_q_scheduler.factor(steps[1], cfg.lr_q)
        lr_alpha = cfg.lr_alpha * cfg.lr_alpha_scheduler.factor(steps[3], cfg.lr_alpha)
        B = state.shape[0]
        if actions is None:
            actions = onehot_action.argmax(dim=1).to(torch.int32)
        return u.update(state.reshape(B, -1), actions, n_state.reshape(B, -1), reward, done, lr_policy, lr_q, lr_alpha,
                        hard_sync, cfg.discount, cfg.soft_target_update_tau, cfg.entropy_alpha_auto_scale, self.target_entropy)

    def _update_torch(self, state, onehot_action, n_state, reward, done, hard_sync: bool) -> dict:
        cfg, p = self.config, self.parameter
        A = cfg.action_space.n
        if not p.load_log_alpha:  # :170-173
            p.log_alpha.requires_grad_(True)
            self.alpha_optimizer = torch.optim.Adam([p.log_alpha], lr=cfg.lr_alpha)
            self._alpha_scheduler = cfg.lr_alpha_scheduler.apply_torch_scheduler(self.alpha_optimizer)
            p.load_log_alpha = True
        alpha = torch.exp(p.log_alpha.detach())  # step 0: one float32 value for the whole call
        with torch.no_grad():  # :179-191
            n_logp = torch.log_softmax(p.policy(n_state), dim=1)
            n_q = all_action_min_q(n_state, A, p.q1_target, p.q2_target)
            v = (torch.exp(n_logp) * (n_q - alpha * n_logp)).sum(dim=1)
            y = reward + ((1.0 - done.to(torch.float32)) * cfg.discount) * v
        out = {"y": y}
        losses = []
        for key, net, opt in (("q1", p.q1_online, self.q1_optimizer), ("q2", p.q2_online, self.q2_optimizer)):  # :194-206
            q = net(state, onehot_action)[:, 0]
            loss = torch.mean(torch.square(y - q))
            opt.zero_grad()
            loss.backward()
            opt.step()
            out[key] = q.detach()
            losses.append(loss.detach())
        with torch.no_grad():  # :209-214
            qv = all_action_min_q(state, A, p.q1_online, p.q2_online)
        probs = torch.softmax(p.policy(state), dim=1)  # :41-51
        logp = torch.log(torch.clamp(probs, 1e-7, 1.0))
        entropy = -(probs * logp).sum(dim=1)
        policy_loss = torch.mean((probs * (alpha * logp - qv)).sum(dim=1))
        self.policy_optimizer.zero_grad()
        policy_loss.backward()
        self.policy_optimizer.step()
        out["entropy"] = entropy.detach()
        alpha_loss = torch.zeros((), dtype=torch.float32, device=state.device)
        if cfg.entropy_alpha_auto_scale:  # :226-233
            alpha_loss = -torch.mean(torch.exp(p.log_alpha) * (self.target_entropy - entropy.detach()))
            self.alpha_optimizer.zero_grad()
            alpha_loss.backward()
            self.alpha_optimizer.step()
            if self._alpha_scheduler is not None:
                self._alpha_scheduler.step()
        for sch in self._schedulers:
            if sch is not None:
                sch.step()
        with torch.no_grad():  # :236-241
            tau = cfg.soft_target_update_tau
            for tgt, net in ((p.q1_target, p.q1_online), (p.q2_target, p.q2_online)):
                for t, w in zip(tgt.parameters(), net.parameters()):
                    if hard_sync:
                        t.copy_(w)
                    else:
                        t.copy_(float(np.float32(1.0 - tau)) * t + float(np.float32(tau)) * w)
        out["scalars"] = torch.stack(losses + [policy_loss.detach(), alpha_loss.detach(), alpha])
        return out


class Worker(RLWorker):
    """:246-272."""

    def policy(self, worker) -> int:
        if self.training and self.step_in_training < self.config.start_steps:
            env_action = self.sample_action()
        else:
            env_action = gumbel_max_sample(self.parameter.logits(worker.state[np.newaxis, ...])[0])
        self.action = worker.get_onehot_action(env_action)
        return env_action

    def on_step(self, worker):
        if not self.training:
            return
        self.memory.add([worker.state, self.action, worker.next_state, worker.reward, worker.terminated])
