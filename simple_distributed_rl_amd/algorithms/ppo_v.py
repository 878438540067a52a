"""V-PPO, the reference's torch PPO (srl/algorithms/ppo_v/config.py:13-70, srl/algorithms/ppo_v/torch_model.py:25-249), registered as "V-PPO:torch".

The reference's own code is torch, so this plugin is held to it directly: tests/test_vppo_pinned_cpu.py runs the reference's `Trainer.train()` in a child
interpreter on hand-fed items and requires the losses, the gradients and the parameters after one and two steps of this module's "torch" backend and of the
float64 yardstick tests/vppo_reference.py (parity PINNED wherever the reference can be imported).  The libsrlx backend is held to that yardstick on the GPU.

Networks.  ActorCriticNetwork (:29-72): in_block -> hidden_block -> (value_block -> value_out_layer Linear(1)) and (policy_block -> policy_dist_block); the
module tree and the state-dict keys are the reference's (`hidden_block.hidden_layers.*`, `value_block.hidden_layers.*`, `value_out_layer.*`,
`policy_dist_block.h_layers.0.*` for the categorical head, `policy_dist_block.loc_layers.0.*` / `.log_scale_layers.0.*` for the Normal head:
srl/rl/torch_/distributions/categorical_dist_block.py:74-97, normal_dist_block.py:66-145), so a state dict moves between the two by key.  The blocks'
layers start as the reference's do (he_normal / zeros in the MLP blocks, torch's default nn.Linear in the out layer and the heads).

Trainer.train() (:111-178) is DESIGN.md 7o's contract, on one of two backends that implement it alike:
  "srlx"   one libsrlx call, three launches (device/vppo.py, csrc/srlx_vppo.hip), for GPU parameters inside the kernels' envelope;
  "torch"  the reference's step in plain torch float32 with torch.optim.Adam, for everything else.
`update_backend` is an attribute of the class (the default) or of a Trainer; the backend is fixed for a Trainer's life at its first train(), and each backend
owns its Adam state.  `update_path` names the path of the last call, `why_not_srlx_update` the reason a request for "srlx" was served by torch.
`engine_kind(ppo_v.Config())` is None and `Runner.train()` runs the plugin path; `device/vppo_engine.py: VppoEngine` trains a Parameter of this
module in place on E lock-stepped lanes for the categorical head on flat observations, `VppoNormalEngine` (7q) for the Normal head.

What is kept from the reference although it reads oddly:
  * The broadcasting (:144-163).  With an action of k > 1 elements new_logpi and ratio are [B][k] while v, q and adv are [B][1]: the Huber, the MSE and the
    surrogate means run over B k elements, every element against its row's v.
  * The value is the TARGET argument of HuberLoss / MSELoss (:154-155); both pass their gradient to it.
  * The squashing correction is summed over the action's elements and subtracted from EVERY element's log-probability (normal_dist_block.py:20-29).
  * The categorical clamp is 1e-7 (the reference writes 10e-8, categorical_dist_block.py:53-54).
  * The entropy term is -exp(logpi) logpi of the taken action only (:168), and is skipped, `loss_e` with it, unless entropy_weight > 0.
  * The Worker floors a stored log-probability at log(1e-6) (:240) and adds an episode's items in reversed order (:245-249).
Stated departures:
  * The "srlx" backend takes the action of a discrete item as the index of its one-hot's maximum: exact for everything the Worker stores.
  * The "srlx" backend evaluates the squashing correction log(clamp(1 - tanh(a)^2, 1e-10, 1)) in float64 and every sum in float64 (rounded to float32 once).
    The "torch" backend evaluates it in float32 as the reference does, where tanh(a) is 1 from |a| = 9.1 on and the correction is log(1e-10) although
    1 - tanh(a)^2 only falls under 1e-10 at |a| = 12.2; between the two the backends differ by up to 4.6 per element, and the float64 value is the exact one."""
import math
import random
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch
import torch.nn as nn

from simple_distributed_rl_amd.algorithms._device_ops import SrlxUpdateBackend
from simple_distributed_rl_amd.base.exception import UndefinedError
from simple_distributed_rl_amd.base.rl.algorithms.base_ppo import RLConfig, RLWorker
from simple_distributed_rl_amd.base.rl.parameter import RLParameter
from simple_distributed_rl_amd.base.rl.registration import register
from simple_distributed_rl_amd.base.rl.trainer import RLTrainer
from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
from simple_distributed_rl_amd.base.spaces.np_array import NpArraySpace
from simple_distributed_rl_amd.rl.functions import compute_normal_logprob, compute_normal_logprob_sgp
from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig, RLReplayBuffer
from simple_distributed_rl_amd.rl.models.config import HiddenBlockConfig, InputBlockConfig
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig
from simple_distributed_rl_amd.rl.torch_.networks import convert_activation


@dataclass
class Config(RLConfig):
    """config.py:13-70, field for field."""

    epsilon: float = 0.1
    test_epsilon: float = 0.0
    policy_noise_normal_scale: float = 0.5
    batch_size: int = 64
    memory: ReplayBufferConfig = field(default_factory=lambda: ReplayBufferConfig())
    input_block: InputBlockConfig = field(default_factory=lambda: InputBlockConfig())
    hidden_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig().set((64, 64)))
    value_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig().set((64,)))
    policy_block: HiddenBlockConfig = field(init=False, default_factory=lambda: HiddenBlockConfig().set(()))
    discount: float = 0.95
    clip_range: float = 0.1
    lr: float = 0.0002
    lr_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    entropy_weight: float = 0
    loss_align_coeff: float = 0.1
    max_grad_norm: float = 10
    squashed_gaussian_policy: bool = True
    enable_stable_gradients: bool = True
    stable_gradients_scale_range: tuple = (1e-10, 10)

    def set_model(self, units: int = 64):
        self.hidden_block.set((units, units))
        self.value_block.set((units,))
        self.policy_block.set((units,))

    def get_name(self) -> str:
        return "V-PPO"

    def get_framework(self) -> str:
        return "torch"


register(Config(), *[__name__ + ":" + c for c in ("Memory", "Parameter", "Trainer", "Worker")], check_duplicate=False)


class Memory(RLReplayBuffer):
    """Items: [state, next_state, action, log_prob, reward, not_done, total_reward] (:235-249)."""


# ---- the two distribution blocks (srl/rl/torch_/distributions) ------------------------------------------------------------------------------------------------
def normal_logprob(x, loc, log_scale):
    """normal_dist_block.py:11-17."""
    return -0.5 * math.log(2 * math.pi) - log_scale - 0.5 * (((x - loc) / torch.exp(log_scale)) ** 2)


def normal_logprob_sgp(x, loc, log_scale, epsilon: float = 1e-10):
    """normal_dist_block.py:20-29; x is the value before tanh."""
    logmu = normal_logprob(x, loc, log_scale)
    x = torch.clamp(1.0 - torch.tanh(x) ** 2, epsilon, 1.0)
    return logmu - torch.sum(torch.log(x), dim=-1, keepdim=True)


class CategoricalDist:
    """categorical_dist_block.py:10-71 (what V-PPO uses of it)."""

    def __init__(self, logits):
        self.classes = logits.shape[-1]
        self._dist = torch.distributions.Categorical(logits=logits)

    def logits(self):
        return self._dist.logits

    def probs(self):
        return self._dist.probs

    def mean(self):
        return self._dist.mean

    def stddev(self):
        return self._dist.stddev

    def sample(self, onehot: bool = True):
        a = self._dist.sample()
        return torch.nn.functional.one_hot(a, num_classes=self.classes).float() if onehot else torch.unsqueeze(a, -1)

    def log_probs(self):
        return torch.log(torch.clamp(self._dist.probs, 1e-7, 1))

    def log_prob(self, a, onehot: bool = False, keepdims: bool = True, **kwargs):
        if onehot:
            a = torch.nn.functional.one_hot(a.squeeze(1) if a.ndim == 2 else a, num_classes=self.classes).to(self._dist.logits.dtype)
        lp = torch.sum(self.log_probs() * a, dim=-1)
        return lp.unsqueeze(-1) if keepdims else lp


class CategoricalDistBlock(nn.Module):
    """categorical_dist_block.py:74-97."""

    def __init__(self, in_size: int, classes: int, hidden_layer_sizes=(), activation="ReLU"):
        super().__init__()
        self.classes = classes
        act = convert_activation(activation)
        self.h_layers = nn.ModuleList()
        for size in hidden_layer_sizes:
            self.h_layers.append(nn.Linear(in_size, size))
            self.h_layers.append(act())
            in_size = size
        self.h_layers.append(nn.Linear(in_size, classes))

    def forward(self, x):
        for layer in self.h_layers:
            x = layer(x)
        return CategoricalDist(x)


class NormalDist:
    """normal_dist_block.py:32-63."""

    def __init__(self, loc, log_scale):
        self._loc, self._log_scale = loc, log_scale

    def mean(self):
        return self._loc

    def stddev(self):
        return torch.exp(self._log_scale)

    def sample(self):
        return torch.normal(self._loc, torch.exp(self._log_scale))

    def log_prob(self, x):
        return normal_logprob(x, self._loc, self._log_scale)

    def log_prob_sgp(self, x):
        return normal_logprob_sgp(x, self._loc, self._log_scale)


class NormalDistBlock(nn.Module):
    """normal_dist_block.py:66-145 with no hidden, loc or scale layers of its own and no fixed scale: what V-PPO builds (:52-57)."""

    def __init__(self, in_size: int, out_size: int, enable_stable_gradients: bool = True, stable_gradients_scale_range: tuple = (1e-10, 10)):
        super().__init__()
        self.out_size = out_size
        self.enable_stable_gradients = enable_stable_gradients
        if enable_stable_gradients:
            self.stable_gradients_scale_range = (np.log(stable_gradients_scale_range[0]), np.log(stable_gradients_scale_range[1]))
        self.h_layers = nn.ModuleList()
        self.loc_layers = nn.ModuleList([nn.Linear(in_size, out_size)])
        self.log_scale_layers = nn.ModuleList([nn.Linear(in_size, out_size)])

    def forward(self, x):
        loc, log_scale = self.loc_layers[0](x), self.log_scale_layers[0](x)
        if self.enable_stable_gradients:
            log_scale = torch.clamp(log_scale, self.stable_gradients_scale_range[0], self.stable_gradients_scale_range[1])
        return NormalDist(loc, log_scale)


class ActorCriticNetwork(nn.Module):
    """:29-72."""

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        self.hidden_block = config.hidden_block.create_torch_block(self.in_block.out_size)
        self.value_block = config.value_block.create_torch_block(self.hidden_block.out_size)
        self.value_out_layer = nn.Linear(self.value_block.out_size, 1)
        self.policy_block = config.policy_block.create_torch_block(self.hidden_block.out_size)
        space = config.action_space
        if isinstance(space, DiscreteSpace):
            self.policy_dist_block = CategoricalDistBlock(self.policy_block.out_size, space.n)
        elif isinstance(space, NpArraySpace):
            self.policy_dist_block = NormalDistBlock(self.policy_block.out_size, space.size, enable_stable_gradients=config.enable_stable_gradients,
                                                     stable_gradients_scale_range=config.stable_gradients_scale_range)
        else:
            raise UndefinedError(space)

    def forward(self, x):
        x = self.hidden_block(self.in_block(x))
        return self.value_out_layer(self.value_block(x)), self.policy_dist_block(self.policy_block(x))


class Parameter(RLParameter):
    """:75-87."""

    def setup(self):
        self.np_dtype = self.config.get_dtype("np")
        self.device = torch.device(self.config.used_device_torch)
        self.net = ActorCriticNetwork(self.config).to(self.device)

    def call_restore(self, data: Any, from_serialized: bool = False, **kwargs) -> None:
        # (in place: the libsrlx backend holds these tensors by address)
        self.net.load_state_dict(data)

    def call_backup(self, serialized: bool = False, **kwargs) -> Any:
        sd = self.net.state_dict()
        if serialized:
            return {k: v.detach().to("cpu").clone() for k, v in sd.items()}
        return sd

    def to_device(self, device):
        """Moves every tensor; the tensors are new ones afterwards (call before a Trainer binds them)."""
        self.device = torch.device(device)
        self.net.to(self.device)

    def summary(self, **kwargs):
        print(self.net)


class Trainer(SrlxUpdateBackend, RLTrainer):
    # "srlx" | "torch".  The default follows the project's 1.10 rule: 0.36 ms per train() on "srlx" against 2.02 ms on "torch" at ppo_v.Config() on
    # CartPole (profiles/vppo_probe.json).  At the envelope's largest corner "torch" is the faster one (46.9 against 2.6 ms): set it there.
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
        from simple_distributed_rl_amd.device.vppo import VppoUpdate

        return VppoUpdate

    def _make_torch_update(self) -> None:
        self.opt = torch.optim.Adam(self.parameter.net.parameters(), lr=self.config.lr)  # :95-96
        self._scheduler = self.config.lr_scheduler.apply_torch_scheduler(self.opt)
        self.huber_loss, self.mse_loss = nn.HuberLoss(), nn.MSELoss()

    def train(self) -> None:
        batches = self.memory.sample()
        if batches is None:
            return
        state, n_state, action, old_logpi, reward, not_terminated, total_reward = zip(*batches)  # :116-130
        B, d, f = len(batches), self.device, self.np_dtype
        col = lambda x: torch.as_tensor(np.asarray(x, dtype=f).reshape(B, -1), device=d)  # noqa: E731
        self.train_on_batch(torch.as_tensor(np.asarray(state, dtype=f), device=d), torch.as_tensor(np.asarray(n_state, dtype=f), device=d), col(action),
                            col(old_logpi), col(reward), col(not_terminated), col(total_reward))

    def train_on_batch(self, state, n_state, action, old_logpi, reward, not_terminated, total_reward, actions=None) -> dict:
        """One update (:132-178) from device tensors: state / n_state f32 [B][...]; action f32 [B][A] one-hot or [B][k]; old_logpi f32 [B][1 or k]; reward,
        not_terminated and total_reward f32 [B][1].  `actions`: the discrete actions as int32 [B], for a caller that has them (the device engine): the "srlx"
        backend then reads them instead of the one-hot's argmax, and `action` may be None there."""
        backend = self._backend_for(state.shape[0])
        if backend == "srlx":
            out = self._update_srlx(state, n_state, action, old_logpi, reward, not_terminated, total_reward, actions)
        else:
            out = self._update_torch(state, n_state, action, old_logpi, reward, not_terminated, total_reward)
        self.update_path = backend
        self.train_count += 1
        scalars = out["scalars"].tolist()  # (the one synchronisation of the call)
        self.info["loss_value"], self.info["loss_v_align"], self.info["loss_policy"] = scalars[0], scalars[1], scalars[2]
        if self.config.entropy_weight > 0:
            self.info["loss_e"] = scalars[3]
        return out

    def _update_srlx(self, state, n_state, action, old_logpi, reward, not_terminated, total_reward, actions=None) -> dict:
        cfg, u = self.config, self._srlx
        B = state.shape[0]
        lr = cfg.lr * cfg.lr_scheduler.factor(u.steps(), cfg.lr)
        if self.discrete:
            act = actions if actions is not None else action.argmax(dim=1).to(torch.int32)
        else:
            act = action
        return u.update(state.reshape(B, -1), n_state.reshape(B, -1), act, old_logpi, reward.reshape(B), not_terminated.reshape(B), total_reward.reshape(B), lr,
                        cfg.discount, cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff, cfg.max_grad_norm, cfg.squashed_gaussian_policy)

    def _update_torch(self, state, n_state, action, old_logpi, reward, not_terminated, total_reward) -> dict:
        cfg, net = self.config, self.parameter.net
        v, p_dist = net(state)
        with torch.no_grad():
            n_v, _ = net(n_state)
        if self.discrete:
            new_logpi = p_dist.log_prob(action, keepdims=True)
        elif cfg.squashed_gaussian_policy:
            new_logpi = p_dist.log_prob_sgp(action)
        else:
            new_logpi = p_dist.log_prob(action)
        ratio = torch.exp(new_logpi - old_logpi)
        q = reward + not_terminated * cfg.discount * n_v  # :149-150
        adv = (q - v).detach()
        ratio_detach = ratio.detach()
        loss_value = self.huber_loss(ratio_detach * q, v)  # :153-156
        loss_v_align = self.mse_loss(ratio_detach * total_reward, v)
        loss = loss_value + cfg.loss_align_coeff * loss_v_align
        ratio_clipped = torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range)  # :161-164
        loss_policy = -torch.mean(torch.minimum(ratio * adv, ratio_clipped * adv))
        loss = loss + loss_policy
        loss_e = torch.zeros((), dtype=torch.float32, device=state.device)
        if cfg.entropy_weight > 0:  # :167-171
            loss_e = -torch.sum(-torch.exp(new_logpi) * new_logpi, dim=-1).mean()
            loss = loss + cfg.entropy_weight * loss_e
        self.opt.zero_grad()
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=cfg.max_grad_norm)
        self.opt.step()
        if self._scheduler is not None:
            self._scheduler.step()
        return {"v": v.detach()[:, 0], "n_v": n_v[:, 0], "new_logpi": new_logpi.detach(),
                "scalars": torch.stack([loss_value.detach(), loss_v_align.detach(), loss_policy.detach(), loss_e.detach(), norm.detach()])}


class Worker(RLWorker):
    """:181-249, on the host."""

    def on_setup(self, worker, context):
        self.np_dtype = self.config.get_dtype("np")

    def _dist(self, worker):
        p = self.parameter
        with torch.no_grad():
            return p.net(torch.as_tensor(worker.state[np.newaxis, ...].astype(self.np_dtype), device=p.device))[1]

    def policy(self, worker):
        cfg = self.config
        p_dist = self._dist(worker)
        epsilon = cfg.epsilon if self.training else cfg.test_epsilon
        space = cfg.action_space
        if isinstance(space, DiscreteSpace):
            if random.random() < epsilon:  # :196-199
                env_action = self.sample_action()
                self.action = worker.get_onehot_action(env_action)
                self.log_prob = [math.log(1.0 / space.n)]
            else:  # :201-205
                action = p_dist.sample(onehot=True)
                self.log_prob = p_dist.log_prob(action).cpu().numpy()[0]
                self.action = action.cpu().numpy()[0]
                env_action = int(np.argmax(self.action))
            return env_action
        if isinstance(space, NpArraySpace):
            loc = p_dist.mean().cpu().numpy()[0]
            scale = p_dist.stddev().cpu().numpy()[0]
            if self.training:  # :210-214
                if random.random() < epsilon:
                    loc = 0
                    scale = cfg.policy_noise_normal_scale
                self.action = np.random.normal(loc, scale, size=space.size)
            else:
                self.action = p_dist.mean().cpu().numpy()[0]
            if cfg.squashed_gaussian_policy:  # :219-222
                self.log_prob = compute_normal_logprob_sgp(self.action, loc, scale)
                return space.rescale_from(np.tanh(self.action), src_low=-1, src_high=1)
            self.log_prob = compute_normal_logprob(self.action, loc, scale)  # :224-226
            return space.sanitize(space.rescale_from(self.action))
        raise UndefinedError(space)

    def on_step(self, worker):
        if not self.training:
            return
        worker.add_tracking({
            "state": worker.state,
            "next_state": worker.next_state,
            "action": self.action,
            "log_prob": np.maximum(self.log_prob, math.log(1e-6)),  # :240
            "reward": worker.reward,
            "not_done": int(not worker.terminated),
        })
        if worker.done:  # :245-249
            total_reward = 0
            for b in reversed(worker.get_trackings()):
                total_reward = b[4] + self.config.discount * total_reward
                self.memory.add(b + [total_reward])

    def render_terminal(self, worker, **kwargs) -> None:
        p = self.parameter
        with torch.no_grad():
            v, p_dist = p.net(torch.as_tensor(worker.state[np.newaxis, ...].astype(self.np_dtype), device=p.device))
        print(f"V: {float(v[0][0]):.7f}")
        if isinstance(self.config.action_space, DiscreteSpace):
            probs, logits = p_dist.probs().cpu().numpy()[0], p_dist.logits().cpu().numpy()[0]
            for a in range(len(probs)):
                print(f"  {a}: {probs[a] * 100:5.1f}%, logits {logits[a]:.7f}")
        else:
            for a in range(self.config.action_space.size):
                print(f"[{a}] mean: {float(p_dist.mean()[0][a]):.7f}, stddev: {float(p_dist.stddev()[0][a]):.7f}")
