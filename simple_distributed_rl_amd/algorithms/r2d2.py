"""R2D2 plugin (Recurrent Replay Distributed DQN, https://openreview.net/forum?id=r1lyTjAqYX; srl/algorithms/r2d2/config.py:44-128,
srl/algorithms/r2d2/r2d2.py:23-367), registered as "R2D2:torch".

The reference's R2D2 is a TensorFlow/Keras model (`get_framework() == "tensorflow"`, config.py:120-121) and cannot be imported in the build container, so
this module is a restatement of the cited lines on the torch/ROCm stack, NOT pinned against recorded reference outputs (parity UNPINNED; the update's
arithmetic and the worker's windows are checked against tests/r2d2_reference.py, a float64 restatement of r2d2.py:109-215 and :227-367 written as a
different program).

Network: in_block per step -> LSTM -> dueling head per step (r2d2.py:27-57).  "Keras LSTM on torch" follows the reference's own torch recurrent model
(srl/algorithms/agent57/model_torch.py:39-46,74-87): an `nn.LSTM` with its two biases and its initialisation holds the parameters; with
`lstm_backend == "srlx"` the layer runs on libsrlx's float32 matrix-core kernels (device/lstm.py), as Agent57's does.
Trainer: the batch goes to the GPU once, burn-in of both networks and the target pass without grad, one online pass with grad, then ONE libsrlx entry point
for everything after the forwards (`srlx_r2d2_seq_td`: masked double-DQN gains, value rescaling, retrace with the stored acting probability, the backward
target recursion, the Huber loss, its gradient seeds and the per-sequence mean TD error); torch back-propagates the seeds and takes the Adam step.
Worker: the reference's host logic, one environment.  The E-lane device engine is device/r2d2.py, taken by `Runner.train()` only under
set_vector_envs(n); device/vector_runner.py:engine_kind stays None for R2D2."""
import random
from dataclasses import dataclass, field
from typing import Any, List, Optional

import numpy as np
import torch
import torch.nn as nn

from simple_distributed_rl_amd.base.define import SpaceTypes
from simple_distributed_rl_amd.base.rl.algorithms.base_dqn import RLConfig, RLWorker
from simple_distributed_rl_amd.base.rl.parameter import RLParameter
from simple_distributed_rl_amd.base.rl.registration import register
from simple_distributed_rl_amd.base.rl.trainer import RLTrainer
from simple_distributed_rl_amd.device.lstm import SrlxLstm
from simple_distributed_rl_amd.rl import functions as funcs
from simple_distributed_rl_amd.rl.memories.priority_replay_buffer import PriorityReplayBufferConfig, RLPriorityReplayBuffer
from simple_distributed_rl_amd.rl.models.config import DuelingNetworkConfig, InputBlockConfig
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig

from ._device_ops import TdOps, invalid_mask, require_gpu


@dataclass
class Config(RLConfig):
    """config.py:44-128, field for field."""

    test_epsilon: float = 0
    epsilon: float = 0.1
    actor_epsilon: float = 0.4
    actor_alpha: float = 7.0
    batch_size: int = 32
    memory: PriorityReplayBufferConfig = field(default_factory=lambda: PriorityReplayBufferConfig())
    input_block: InputBlockConfig = field(default_factory=lambda: InputBlockConfig())
    lstm_units: int = 512
    hidden_block: DuelingNetworkConfig = field(init=False, default_factory=lambda: DuelingNetworkConfig().set_dueling_network((512,)))
    burnin: int = 5
    sequence_length: int = 5
    discount: float = 0.997
    lr: float = 0.001
    lr_scheduler: LRSchedulerConfig = field(default_factory=lambda: LRSchedulerConfig())
    target_model_update_interval: int = 1000
    enable_double_dqn: bool = True
    enable_rescale: bool = False
    enable_retrace: bool = True
    retrace_h: float = 1.0

    def setup_from_actor(self, actor_num: int, actor_id: int) -> None:
        self.epsilon = funcs.create_epsilon_list(actor_num, epsilon=self.actor_epsilon, alpha=self.actor_alpha)[actor_id]

    def set_atari_config(self):
        """config.py:88-112"""
        self.lstm_units = 512
        self.input_block.image.set_dqn_block()
        self.hidden_block.set_dueling_network((512,))
        self.burnin = 40
        self.sequence_length = 80
        self.discount = 0.997
        self.lr = 0.0001
        self.batch_size = 64
        self.target_model_update_interval = 2500
        self.enable_double_dqn = True
        self.enable_rescale = True
        self.enable_retrace = False
        self.memory.capacity = 1_000_000
        self.memory.set_proportional(alpha=0.9, beta_initial=0.6, beta_steps=1_000_000)

    def get_name(self) -> str:
        return "R2D2"

    def get_processors(self, prev_observation_space) -> list:
        """config.py:117-118 through input_block.py:195-200,274-279: the DQN image block asks for 84 x 84 grey frames in 0..1; a value block for nothing."""
        if prev_observation_space.is_image_like() and self.input_block.image.name == "DQN":
            from simple_distributed_rl_amd.rl.processors.image_processor import ImageProcessor

            return [ImageProcessor(SpaceTypes.GRAY_HW1, (84, 84), normalize_type="0to1")]
        return []

    def get_framework(self) -> str:
        return "torch"

    def validate_params(self) -> None:
        super().validate_params()
        if not (self.burnin >= 0):
            raise ValueError(f"assert {self.burnin} >= 0")
        if not (self.sequence_length >= 1):
            raise ValueError(f"assert {self.sequence_length} >= 1")


register(Config(), __name__ + ":Memory", __name__ + ":Parameter", __name__ + ":Trainer", __name__ + ":Worker", check_duplicate=False)


class Memory(RLPriorityReplayBuffer):
    pass


class QNetwork(nn.Module):
    """in_block per step -> LSTM -> hidden_block (dueling head) per step (r2d2.py:27-57).

    The reference's layer is Keras' LSTM; here, as in the reference's own torch recurrent model (srl/algorithms/agent57/model_torch.py:39-46,74-87),
    `lstm_layer` is an `nn.LSTM(in_block.out_size, lstm_units, batch_first=True)` with torch's two biases and torch's initialisation, holding the parameters
    under torch's keys.  With `lstm_backend == "srlx"`, tensors on a GPU and a shape inside libsrlx's envelope (srlx.h: B, T <= 256, I <= 16384, H a multiple
    of 16 up to 512) the layer runs on libsrlx's kernels; otherwise (CPU parameters, `lstm_backend = "torch"`, other shapes) it is `nn.LSTM` itself.
    `lstm_path` names the path of the last call.  The in-block is the torch module."""

    lstm_backend = "srlx"  # "srlx" | "torch": an attribute of the network (of the class: the default), not of the process environment

    def __init__(self, config: Config):
        super().__init__()
        self.in_block = config.input_block.create_torch_block(config)
        self.hidden_size = config.lstm_units
        self.lstm_layer = nn.LSTM(self.in_block.out_size, config.lstm_units, batch_first=True)
        self.hidden_block = config.hidden_block.create_torch_block(config.lstm_units, config.action_space.n)
        self.lstm_path = None
        self._srlx_lstm = SrlxLstm()  # the libsrlx path of `lstm_layer` (device/lstm.py): owns its cached buffers, no parameters

    def _lstm(self, x, hidden_states):
        if self.lstm_backend not in ("srlx", "torch"):
            raise ValueError(f"lstm_backend {self.lstm_backend!r}: 'srlx' or 'torch'")
        srlx = self.lstm_backend == "srlx" and self._srlx_lstm.serves(self.lstm_layer, x)
        self.lstm_path = "srlx" if srlx else "torch"
        return self._srlx_lstm(self.lstm_layer, x, hidden_states) if srlx else self.lstm_layer(x, hidden_states)

    def forward(self, state, hidden_states):
        """state [B][T][...], hidden_states (h, c) of [1][B][H] each -> q [B][T][A], (h_n, c_n)."""
        B, T = state.shape[:2]
        x = self.in_block(state.reshape((B * T,) + tuple(state.shape[2:]))).view(B, T, -1)
        x, hidden_states = self._lstm(x, hidden_states)
        return self.hidden_block(x.reshape(B * T, -1)).view(B, T, -1), hidden_states

    def get_initial_state(self, batch_size, device):
        return (torch.zeros(1, batch_size, self.hidden_size, device=device), torch.zeros(1, batch_size, self.hidden_size, device=device))


class Parameter(RLParameter):
    def setup(self):
        self.np_dtype = self.config.get_dtype("np")
        self.device = torch.device(self.config.used_device_torch)
        self.q_online = QNetwork(self.config).to(self.device)
        self.q_target = QNetwork(self.config).to(self.device)
        self.q_target.eval()
        self.q_target.load_state_dict(self.q_online.state_dict())

    def to_device(self, device):
        self.device = torch.device(device)
        self.q_online.to(self.device)
        self.q_target.to(self.device)

    def call_restore(self, data: Any, from_serialized: bool = False, **kwargs) -> None:  # r2d2.py:72-74
        self.q_online.load_state_dict(data)
        self.q_target.load_state_dict(data)

    def call_backup(self, serialized: bool = False, **kwargs) -> Any:  # :76-77
        sd = self.q_online.state_dict()
        return {k: v.detach().to("cpu").clone() for k, v in sd.items()} if serialized else sd

    def get_initial_hidden_state(self):
        return self.q_online.get_initial_state(1, self.device)

    def predict_q(self, state: np.ndarray, hidden_state):
        """One acting step: state [1][1][...] -> (q [A] numpy, the next recurrent state)."""
        self.q_online.eval()
        with torch.no_grad():
            q, h = self.q_online(torch.as_tensor(np.asarray(state, dtype=np.float32), device=self.device), hidden_state)
        return q[0][0].cpu().numpy(), h

    def convert_numpy_from_hidden_state(self, h) -> list:
        """(h, c) of [1][1][H] -> [h [H], c [H]] numpy (r2d2.py:244: `hidden_state[0][0]`, `hidden_state[1][0]`)."""
        return [h[0][0][0].cpu().numpy(), h[1][0][0].cpu().numpy()]


@dataclass
class SequenceBatch:
    """One training batch on the device, its fields named after the reference's item keys (r2d2.py:352-360); L = burnin + sequence_length + 1 and
    S = sequence_length.  Built in one place (`from_items`) so that a device-resident sequence store can hand the trainer the same object."""

    states: torch.Tensor  # f32 [B][L][...]
    actions: torch.Tensor  # i32 [B][S]
    probs: torch.Tensor  # f32 [B][S]
    rewards: torch.Tensor  # f32 [B][S]
    dones: torch.Tensor  # u8 [B][S]
    invalid_actions: Optional[torch.Tensor]  # u8 [B][S + 1][A], None when no item has an invalid action
    hidden_states: tuple  # (h, c) f32 [1][B][H] each: the recurrent state at the window head

    @classmethod
    def from_items(cls, batches: List[dict], n_actions: int, device) -> "SequenceBatch":
        B, S = len(batches), len(batches[0]["actions"])
        t = lambda key, dtype: torch.from_numpy(np.asarray([b[key] for b in batches], dtype=dtype)).to(device)  # noqa: E731
        h = torch.from_numpy(np.asarray([b["hidden_states"][0] for b in batches], dtype=np.float32)).to(device).unsqueeze(0)
        c = torch.from_numpy(np.asarray([b["hidden_states"][1] for b in batches], dtype=np.float32)).to(device).unsqueeze(0)
        return cls(states=t("states", np.float32), actions=t("actions", np.int32), probs=t("probs", np.float32), rewards=t("rewards", np.float32),
                   dones=t("dones", np.uint8), invalid_actions=invalid_mask([lst for b in batches for lst in b["invalid_actions"]], (B, S + 1, n_actions), device),
                   hidden_states=(h, c))


class Trainer(RLTrainer):
    def on_setup(self) -> None:
        self.device = require_gpu(self.config.used_device_torch)
        self.parameter.to_device(self.device)
        self.ops = TdOps(self.device)
        self.optimizer = torch.optim.Adam(self.parameter.q_online.parameters(), lr=self.config.lr)
        self.lr_sch = self.config.lr_scheduler.apply_torch_scheduler(self.optimizer)
        self.sync_count = 0

    def train(self) -> None:  # r2d2.py:91-107
        sampled = self.memory.sample()
        if sampled is None:
            return
        batches, weights, update_args = sampled
        c = self.config
        sb = batches if isinstance(batches, SequenceBatch) else SequenceBatch.from_items(batches, c.action_space.n, self.device)
        w = torch.as_tensor(np.asarray(weights, dtype=np.float32), device=self.device)
        td_mean, loss = self._train_on_batch(sb, w)
        self.memory.update(update_args, td_mean.cpu().numpy(), self.train_count)
        if self.train_count % c.target_model_update_interval == 0:
            self.parameter.q_target.load_state_dict(self.parameter.q_online.state_dict())
            self.sync_count += 1
        self.train_count += 1
        self.info["loss"] = float(loss.item())
        self.info["sync"] = self.sync_count

    def _train_on_batch(self, sb: SequenceBatch, weights: torch.Tensor):  # :109-215
        c, online, target_net = self.config, self.parameter.q_online, self.parameter.q_target
        burnin_states, step_states = sb.states[:, : c.burnin], sb.states[:, c.burnin :]
        hidden = hidden_t = sb.hidden_states
        with torch.no_grad():
            if c.burnin > 0:  # :134-136
                _, hidden = online(burnin_states, hidden)
                _, hidden_t = target_net(burnin_states, hidden_t)
            q_target, _ = target_net(step_states, hidden_t)  # :139
        online.train()
        q, _ = online(step_states, hidden)  # :145
        _, loss, grad, td_mean = self.ops.r2d2_seq_td(q, q_target, sb.actions, sb.probs, sb.rewards, sb.dones, sb.invalid_actions, weights, c.discount,
                                                      c.retrace_h, c.enable_retrace, c.enable_double_dqn, c.enable_rescale)
        self.optimizer.zero_grad()
        q.backward(grad)
        self.optimizer.step()
        if self.lr_sch is not None:
            self.lr_sch.step()
        return td_mean, loss


class Worker(RLWorker):
    """r2d2.py:221-367: windows of burnin + sequence_length + 1 states and sequence_length actions / probs / rewards / dones shifted every step, padded with
    dummy states, random actions and 1 / A probabilities before the episode and after its end, the recurrent state captured at the window head."""

    def on_setup(self, worker, context) -> None:
        self.dummy_state = np.zeros(self.config.observation_space.shape, dtype=np.float32)

    def on_reset(self, worker):
        c, n = self.config, self.config.action_space.n
        L = c.burnin + c.sequence_length + 1
        self._recent_states = [self.dummy_state for _ in range(L)]
        self.recent_actions = [random.randint(0, n - 1) for _ in range(c.sequence_length)]
        self.recent_probs = [1.0 / n for _ in range(c.sequence_length)]
        self.recent_rewards = [0.0 for _ in range(c.sequence_length)]
        self.recent_done = [False for _ in range(c.sequence_length)]
        self.recent_invalid_actions = [[] for _ in range(c.sequence_length + 1)]
        self.hidden_state = self.parameter.get_initial_hidden_state()
        h0 = self.parameter.convert_numpy_from_hidden_state(self.hidden_state)
        self.recent_hidden_states = [[h0[0], h0[1]] for _ in range(L)]
        self._recent_states.pop(0)
        self._recent_states.append(worker.state.astype(np.float32))
        self.recent_invalid_actions.pop(0)
        self.recent_invalid_actions.append(worker.invalid_actions)
        self._calc_td_error = bool(self.distributed and c.memory.requires_priority())  # :251-258
        self._history_batch = []

    def policy(self, worker) -> int:
        c = self.config
        q, self.hidden_state = self.parameter.predict_q(worker.state[np.newaxis, np.newaxis, ...], self.hidden_state)
        epsilon = c.epsilon if self.training else c.test_epsilon
        probs = funcs.calc_epsilon_greedy_probs(q, worker.invalid_actions, epsilon, c.action_space.n)
        self.action = funcs.random_choice_by_probs(probs)
        self.prob = probs[self.action]
        self.q = q
        return self.action

    def _shift(self, state, action, prob, reward, done, invalid, hidden):
        for lst, v in ((self._recent_states, state), (self.recent_actions, action), (self.recent_probs, prob), (self.recent_rewards, reward),
                       (self.recent_done, done), (self.recent_invalid_actions, invalid)):
            lst.pop(0)
            lst.append(v)
        self.recent_hidden_states.pop(0)
        if hidden is not None:
            self.recent_hidden_states.append(hidden)

    def on_step(self, worker):
        if not self.training:
            return
        c, n = self.config, self.config.action_space.n
        self._shift(worker.next_state.astype(np.float32), self.action, self.prob, worker.reward, worker.terminated, worker.next_invalid_actions,
                    self.parameter.convert_numpy_from_hidden_state(self.hidden_state))
        self._add_memory({"q": self.q[self.action], "reward": worker.reward} if self._calc_td_error else None)
        if worker.done:  # the remaining steps of the window (:311-349); the list of recurrent states only shrinks (:326)
            for _ in range(len(self.recent_rewards) - 1):
                self._shift(self.dummy_state, random.randint(0, n - 1), 1.0 / n, 0.0, True, [], None)
                self._add_memory({"q": self.q[self.action], "reward": 0.0})
                if self._calc_td_error:  # Monte-Carlo initial priorities over the episode so far, newest first, once per flushed item as the reference has it (:335-349)
                    reward = 0
                    for batch, info in reversed(self._history_batch):
                        _r = funcs.inverse_rescaling(reward) if c.enable_rescale else reward
                        reward = info["reward"] + c.discount * _r
                        if c.enable_rescale:
                            reward = funcs.rescaling(reward)
                        self.memory.add(batch, abs(reward - info["q"]))

    def _add_memory(self, calc_info):
        batch = {
            "states": self._recent_states[:],
            "actions": self.recent_actions[:],
            "probs": self.recent_probs[:],
            "rewards": self.recent_rewards[:],
            "dones": self.recent_done[:],
            "invalid_actions": self.recent_invalid_actions[:],
            "hidden_states": self.recent_hidden_states[0],
        }
        if self._calc_td_error:
            self._history_batch.append([batch, calc_info])
        else:
            self.memory.add(batch, None)

    def render_terminal(self, worker, **kwargs) -> None:
        q = self.q
        maxa = int(np.argmax(q))
        if self.config.enable_rescale:
            q = funcs.inverse_rescaling(q)
        worker.print_discrete_action_info(maxa, lambda a: f"{q[a]:7.5f}")
