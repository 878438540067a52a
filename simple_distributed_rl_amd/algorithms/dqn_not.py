"""NoTarget_DQN, the reference's torch DQN without a target network (srl/algorithms/dqn_not/config.py:16-61, parameter.py:17-71, trainer.py:16-87,
worker.py:15-60), registered as "NoTarget_DQN:torch": the value-based member of the target-free family beside V-PPO (ppo_v) and NoT_SAC (sac_not).

Network (parameter.py:17-46).  in_block -> hidden_block = Linear(units) + ReLU -> v_block = Linear(units) + ReLU + Linear(1) beside adv_block = Linear(units) +
ReLU + Linear(A); forward returns (q, v) with q = v + adv - mean(adv).  The module tree and the state-dict keys are the reference's (`hidden_block.0.*`,
`v_block.0.*`, `v_block.2.*`, `adv_block.0.*`, `adv_block.2.*`), so a state dict moves between the two by key.

Trainer.train() (trainer.py:33-87): ONE forward of the online network over [s; s'] (2B rows); rows B.. are detached and give the target
r + nd * discount * (max_a q(s') + v(s')) / 2; the loss is mean(w huber(target, q[a])) + align_coeff * mean(w (total_reward - q[a])^2) with the replay's
importance weights (1 for a memory without priorities); Adam at torch's defaults, no gradient clip; priorities |target - q[a]|.  Two backends implement it alike:
  "srlx"   one libsrlx call, six launches on the float64 matrix cores (device/dqnnot.py, csrc/srlx_dqnnot.hip), for GPU parameters inside the
           kernels' envelope (flat observations of 1..256 floats, base_units 32..512 in multiples of 32, 2..32 actions, batches up to 4096);
  "torch"  the reference's step in plain torch float32 with torch.optim.Adam, for CPU parameters and everything else.
`update_backend`, `update_path` and `why_not_srlx_update` work as in ppo_v.Trainer.  `engine_kind(dqn_not.Config())` is None: there is no device engine; the
Worker acts through `Parameter.pred_q`, whose forward is one srlx_dqnnot_act launch for GPU parameters inside the same envelope (`Parameter.act_backend`,
DESIGN.md 7z) and the module's torch forward otherwise; the epsilon branch and the argmax stay on the host.

Kept from the reference although it reads oddly:
  * The target is the FIRST argument of HuberLoss and MSELoss (trainer.py:66,70); q is their second and takes the gradient.
  * The Worker's full window of an unfinished episode adds ONE item (worker.py:39-44, see `Worker.on_step`).
Stated departure: the "srlx" backend keeps v and adv in float64 up to q (the reference rounds each Linear's output to float32 first)."""
import random
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch
import torch.nn as nn

from simple_distributed_rl_amd.algorithms._device_ops import SrlxUpdateBackend
from simple_distributed_rl_amd.base.rl.algorithms.base_dqn import RLConfig, RLWorker
from simple_distributed_rl_amd.base.rl.parameter import RLParameter
from simple_distributed_rl_amd.base.rl.registration import register
from simple_distributed_rl_amd.base.rl.trainer import RLTrainer
from simple_distributed_rl_amd.rl.memories.priority_replay_buffer import PriorityReplayBufferConfig, RLPriorityReplayBuffer
from simple_distributed_rl_amd.rl.models.config import InputBlockConfig
from simple_distributed_rl_amd.rl.schedulers.scheduler import SchedulerConfig


@dataclass
class Config(RLConfig):
    """config.py:16-47, field for field."""

    test_epsilon: float = 0
    epsilon: float = 0.1
    epsilon_scheduler: SchedulerConfig = field(default_factory=lambda: SchedulerConfig())
    discount: float = 0.995
    max_discount_steps: int = 500
    align_loss_coeff: float = 0.1
    align_loss_coeff_scheduler: SchedulerConfig = field(default_factory=lambda: SchedulerConfig())
    memory: PriorityReplayBufferConfig = field(default_factory=lambda: PriorityReplayBufferConfig())
    batch_size: int = 32
    lr: float = 0.0002
    input_block: InputBlockConfig = field(default_factory=lambda: InputBlockConfig())
    base_units: int = 512

    def get_name(self) -> str:
        return "NoTarget_DQN"

    def get_framework(self) -> str:
        return "torch"

    def setup_from_env(self, env) -> None:
        if env.player_num != 1:
            raise ValueError(f"assert {env.player_num} == 1")


register(Config(), *[__name__ + ":" + c for c in ("Memory", "Parameter", "Trainer", "Worker")], check_duplicate=False)


class Memory(RLPriorityReplayBuffer):
    """Items: [state, next_state, action, reward, not_done, total_reward] (worker.py:29-47)."""


class QNetwork(nn.Module):
    """parameter.py:17-46."""

    def __init__(self, config: Config):
        super().__init__()
        units = config.base_units
        self.in_block = config.input_block.create_torch_block(config)
        self.hidden_block = nn.Sequential(nn.Linear(self.in_block.out_size, units), nn.ReLU())
        self.v_block = nn.Sequential(nn.Linear(units, units), nn.ReLU(), nn.Linear(units, 1))
        self.adv_block = nn.Sequential(nn.Linear(units, units), nn.ReLU(), nn.Linear(units, config.action_space.n))

    def forward(self, x):
        x = self.hidden_block(self.in_block(x))
        v = self.v_block(x)
        adv = self.adv_block(x)
        return v + adv - torch.mean(adv, dim=-1, keepdim=True), v


class Parameter(RLParameter):
    """parameter.py:49-71.  `pred_q` runs on one of two backends, as the Trainer's update does: `act_backend` asks for "srlx" (one srlx_dqnnot_act launch,
    device/dqnnot.py: DqnNotAct) or "torch" (the module's forward); `act_path` names what the last call ran, and `why_not_srlx_act` holds the
    reason when "srlx" was asked for and torch ran: CPU parameters, an image or layered input block, a shape outside the kernels' envelope, more than 65536
    rows.  The handle is made at the first GPU call and binds the tensors by address, so it sees `call_restore` and a Trainer's updates; `to_device` drops it."""

    # "srlx" | "torch".  The default follows the project's 1.10 rule: 0.133 to 0.134 ms per pred_q of one row on "srlx" against 0.236 to 0.237 ms
    # on "torch" at dqn_not.Config() on CartPole, a ratio of 0.57 in every round (profiles/dqnnot_act_probe.json).
    act_backend = "srlx"

    def setup(self):
        self.np_dtype = self.config.get_dtype("np")
        self.device = torch.device(self.config.used_device_torch)
        self.q_online = QNetwork(self.config).to(self.device)
        self.q_online.train()
        self.act_path = self.why_not_srlx_act = ""
        self._act, self._act_why = None, None  # the acting handle, and why there is none (None: not asked yet for these tensors)

    def call_restore(self, data: Any, from_serialized: bool = False, **kwargs) -> None:
        self.q_online.load_state_dict(data)  # (in place: the libsrlx backend holds these tensors by address)

    def call_backup(self, serialized: bool = False, **kwargs) -> Any:
        sd = self.q_online.state_dict()
        return {k: v.detach().to("cpu").clone() for k, v in sd.items()} if serialized else sd

    def to_device(self, device):
        """Moves every tensor; the tensors are new ones afterwards (call before a Trainer binds them)."""
        self.device = torch.device(device)
        self.q_online.to(self.device)
        self._act, self._act_why = None, None  # (the handle held the old tensors' addresses)

    def summary(self, **kwargs):
        print(self.q_online)

    def _srlx_act(self, n: int):
        """The acting handle when libsrlx serves a call of n rows; otherwise None, with the reason in `why_not_srlx_act` ('' where "torch" was asked for)."""
        if self.act_backend not in ("srlx", "torch"):
            raise ValueError(f"act_backend {self.act_backend!r}: 'srlx' or 'torch'")
        self.why_not_srlx_act = ""
        if self.act_backend == "torch":
            return None
        from simple_distributed_rl_amd.device.dqnnot import DqnNotAct

        if self._act_why is None:
            self._act_why = DqnNotAct.why_not(self)
            if not self._act_why:
                self._act = DqnNotAct(self)
        self.why_not_srlx_act = self._act_why or DqnNotAct.rows_reason(n)
        return None if self.why_not_srlx_act else self._act

    def pred_q(self, state: np.ndarray):
        """(q [n][A], v [n][1]) as numpy arrays (parameter.py:65-71)."""
        x = torch.as_tensor(np.asarray(state, dtype=self.np_dtype), device=self.device)
        act = self._srlx_act(x.shape[0])
        if act is not None:
            q, v, _ = act.act(x.reshape(x.shape[0], -1).float())
        else:
            with torch.no_grad():
                q, v = self.q_online(x)
        self.act_path = "srlx" if act is not None else "torch"
        return q.cpu().numpy(), v.cpu().numpy()


class Trainer(SrlxUpdateBackend, RLTrainer):
    # "srlx" | "torch".  The default follows the project's 1.10 rule: 0.19 ms per train() on "srlx" against 1.24 ms on "torch" at dqn_not.Config()
    # on CartPole, a ratio of 0.15 in every round (profiles/dqnnot_probe.json).
    update_backend = "srlx"

    def on_setup(self) -> None:
        cfg = self.config
        self.device = torch.device(cfg.used_device_torch)
        if self.parameter.device != self.device:
            self.parameter.to_device(self.device)
        self.np_dtype = cfg.get_dtype("np")
        self.align_loss_coeff_sch = cfg.align_loss_coeff_scheduler.create(cfg.align_loss_coeff)  # trainer.py:25
        self._reset_backend()

    # ---- the backends -----------------------------------------------------------------------------------------------------------------------------------
    def _srlx_update_class(self):
        from simple_distributed_rl_amd.device.dqnnot import DqnNotUpdate

        return DqnNotUpdate

    def _make_torch_update(self) -> None:
        self.opt = torch.optim.Adam(self.parameter.q_online.parameters(), lr=self.config.lr)  # trainer.py:21-23
        self.criterion1, self.criterion2 = nn.HuberLoss(reduction="none"), nn.MSELoss(reduction="none")

    def train(self) -> None:
        sampled = self.memory.sample()
        if sampled is None:
            return
        batches, weights, update_args = sampled
        state, n_state, action, reward, not_terminated, total_reward = zip(*batches)  # trainer.py:43-54
        d, f = self.device, self.np_dtype
        vec = lambda x: torch.as_tensor(np.asarray(x, dtype=f), device=d)  # noqa: E731
        priority = self.config.memory.requires_priority()
        out = self.train_on_batch(vec(state + n_state), torch.as_tensor(np.asarray(action, dtype=np.int32), device=d), vec(reward), vec(not_terminated),
                                  vec(total_reward), vec(weights) if priority else None)
        if priority:  # trainer.py:83-85
            self.memory.update(update_args, np.abs((out["target_q"] - out["q"]).cpu().numpy()), self.train_count - 1)

    def train_on_batch(self, states, actions, reward, not_terminated, total_reward, weights=None) -> dict:
        """One update (trainer.py:54-87) from device tensors: states f32 [2B][...] (rows B.. are the next states); actions integer [B]; reward, not_terminated
        and total_reward f32 [B]; weights f32 [B] or None (every weight 1).  Returns q, target_q [B] and `losses` [2] (loss_q, loss_align)."""
        B = actions.shape[0]
        backend = self._backend_for(B)
        align_coeff = self.align_loss_coeff_sch.update(self.train_count).to_float()  # (evaluated on the host, as the reference does)
        if backend != "torch":
            out = self._srlx.update(states.reshape(2 * B, -1), actions.to(torch.int32), reward, not_terminated, total_reward, weights, self.config.discount,
                                    align_coeff, self.config.lr)
        else:
            out = self._update_torch(states, actions, reward, not_terminated, total_reward, weights, align_coeff)
        self.update_path = backend
        self.train_count += 1
        self.info["loss_q"], self.info["loss_align"] = out["losses"].tolist()  # (the one synchronisation of the call)
        if self.config.align_loss_coeff_scheduler.is_update_step():
            self.info["loss_align_coeff"] = align_coeff
        return out

    def _update_torch(self, states, actions, reward, not_terminated, total_reward, weights, align_coeff) -> dict:
        B = actions.shape[0]
        w = 1 if weights is None else weights
        q_all, v_all = self.parameter.q_online(states)  # trainer.py:58-80
        n_q = q_all[B:].detach()
        n_v = v_all[B:].detach().squeeze(-1)
        n_maxq = n_q.max(dim=1).values
        target_q = reward + not_terminated * self.config.discount * (n_maxq + n_v) / 2
        q = q_all[:B].gather(1, actions.to(torch.int64).reshape(B, 1)).squeeze(1)
        loss_q = (self.criterion1(target_q, q) * w).mean()
        loss_align = (self.criterion2(total_reward, q) * w).mean()
        loss = loss_q + align_coeff * loss_align
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return {"q": q.detach(), "target_q": target_q, "losses": torch.stack([loss_q.detach(), loss_align.detach()])}


class Worker(RLWorker):
    """worker.py:15-60, on the host."""

    def on_setup(self, worker, context) -> None:
        self.epsilon_sch = self.config.epsilon_scheduler.create(self.config.epsilon)
        worker.set_tracking_max_size(self.config.max_discount_steps)

    def policy(self, worker) -> int:
        epsilon = self.epsilon_sch.update(self.step_in_training).to_float() if self.training else self.config.test_epsilon
        if random.random() < epsilon:
            return self.sample_action()
        q, _ = self.parameter.pred_q(worker.state[np.newaxis, ...])
        return int(np.argmax(q[0]))

    def on_step(self, worker):
        if not self.training:
            return
        worker.add_tracking({
            "state": worker.state,
            "n_state": worker.next_state,
            "action": worker.action,
            "reward": worker.reward,
            "not_done": int(not worker.terminated),
        })
        discount = self.config.discount
        if worker.done:  # worker.py:45-49: every tracked step with its return to the episode's end
            total_reward = 0
            for b in reversed(worker.get_trackings()):
                total_reward = b[3] + discount * total_reward
                self.memory.add(b + [total_reward])
        elif worker.get_tracking_length() == self.config.max_discount_steps:
            # worker.py:39-44, kept as the reference has it: on a full window of an unfinished episode the walk runs over the whole window and ONE item is
            # added behind it, the last one the walk reached: the window's OLDEST step with the window's return.  (The window then slides by one step per step,
            # so each step leaves it once this way; the steps still tracked when the episode ends are added again by the branch above.)
            total_reward, b = 0, None
            for b in reversed(worker.get_trackings()):
                total_reward = b[3] + discount * total_reward
            self.memory.add(b + [total_reward])

    def render_terminal(self, worker, **kwargs) -> None:
        q, v = self.parameter.pred_q(worker.state[np.newaxis, ...])
        q, v = q[0], v[0][0]
        print(f"V={v:.7f}")
        worker.print_discrete_action_info(int(np.argmax(q)), lambda a: f"{q[a]:8.5f} (adv: {q[a] - v:8.5f})")
