"""DQN on flat observations on the device engine: the MLP Q-network of libsrlx (`srlx_mlpq_*`, srlx_mlpq.hip), a device-resident batch CartPole, and
`VectorQEngine`, which speaks the driver surface `VectorActor` / `VectorLearner` call on `RainbowEngine` (device/vector_runner.py).

Reference semantics kept (file:line under the reference root):
  srl/algorithms/dqn/model_torch.py:17-29   in_block -> hidden_block (MLP) -> out_layer             -> EngineMLPQNet
  srl/algorithms/dqn/dqn.py:144-176         the 1-step (double) DQN target                           -> srlx_mlpq_train_step
  srl/algorithms/dqn/model_torch.py:89-131  IS-weighted Huber loss, Adam, priorities, target sync   -> srlx_mlpq_train_step, srlx_mlpq_publish
  srl/algorithms/rainbow/model_torch.py:15-29  in_block -> hidden_block (MLP over layer_sizes[:-1] + DuelingNetworkBlock) -> EngineMLPQNet(dueling_units=H)
  srl/algorithms/rainbow/rainbow.py:185-287    the n-step retrace target                              -> srlx_mlpq_train_nstep
  srl/rl/torch_/modules/noisy_linear.py:8-52   NoisyLinear (enable_noisy_dense: the hidden block's MLP layers and the head) -> EngineMLPQNet(noisy=True),
                                               srlx_mlpq_bind_noisy; rainbow.py:305-309: a noisy net acts greedily          -> VectorQEngine.eps = 0
  srl/algorithms/c51/c51.py:23-42              in_block -> hidden_block (MLP) -> Dense(A * N) reshaped to [A][N]           -> EngineMLPQNet(n_atoms=N)
  srl/algorithms/c51/c51.py:70-142             the categorical update on the online network alone (no target network)      -> srlx_mlpq_train_categorical
The replay is the engine's `DeviceReplay` with float32 observations, window 1 and `multisteps`-step items.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.device.replay import DeviceReplay
from simple_distributed_rl_amd.rl.torch_.networks import NoisyLinear


DUELING_TYPES = {"average": 0, "": 1}  # srlx_mlpq_create_dueling's dueling_type


class EngineMLPQNet(nn.Module):
    """DQN's module tree for a flat input (algorithms/dqn.py:build_qnetwork): `in_sizes` = the input value block's layers, `hidden_sizes` = the MLP hidden
    block's, every one Linear + ReLU, then `out_layer`.  Parameters stay in torch's Linear layout, which is the one libsrlx reads.

    `dueling_units` = H > 0 is Rainbow's tree instead (rl/torch_/networks.py:create_dueling_hidden_block): `hidden_sizes` = the hidden block's layer_sizes[:-1],
    then a DuelingNetworkBlock with H = layer_sizes[-1] units in its value and advantage branches (`dueling_type` "average" or "") in place of `out_layer`.

    `noisy` (Rainbow's enable_noisy_dense; dueling nets only): the `hidden_sizes` layers and the four head layers are NoisyLinear (`w_mu / w_sigma / b_mu /
    b_sigma`, the reference's initialisation and keys, fresh torch.randn noise on every forward); the `in_sizes` layers stay nn.Linear
    (rainbow/model_torch.py:19-24: the input value block takes no noisy flag).

    `n_atoms` = N > 0 is C51's tree (algorithms/c51.py:build_network): `out_layer` is Linear(., A * N), row a * N + j = atom j of action a on the support
    linspace(v_min, v_max, N).  `forward` returns the expectations [rows][A], `dist` the probabilities [rows][A][N]."""

    def __init__(self, obs_dim: int, in_sizes: Sequence[int], hidden_sizes: Sequence[int], n_actions: int, dueling_units: int = 0,
                 dueling_type: str = "average", noisy: bool = False, n_atoms: int = 0, v_min: float = -10.0, v_max: float = 10.0):
        super().__init__()
        self.n_atoms, self.v_min, self.v_max = int(n_atoms), float(v_min), float(v_max)
        assert not self.n_atoms or not (dueling_units or noisy), "the categorical head is a plain out_layer (c51.py:29-32)"
        self.noisy = bool(noisy)
        assert not self.noisy or dueling_units, "noisy layers belong to the dueling (Rainbow) network"
        lin = NoisyLinear if self.noisy else nn.Linear
        self.obs_dim, self.n_actions = int(obs_dim), int(n_actions)
        self.in_sizes, self.hidden_sizes = tuple(int(x) for x in in_sizes), tuple(int(x) for x in hidden_sizes)
        self.dueling_units, self.dueling_type = int(dueling_units), str(dueling_type)
        sizes = self.in_sizes + self.hidden_sizes
        self.layers = nn.ModuleList()
        prev = self.obs_dim
        for k, s in enumerate(sizes):
            self.layers.append((nn.Linear if k < len(self.in_sizes) else lin)(prev, s))
            prev = s
        # the reference's keys: in_block.hidden_layers = [Flatten, Linear, ReLU, ...], hidden_block.hidden_layers = [Linear, ReLU, ...]
        self._keys = [f"in_block.hidden_layers.{1 + 2 * k}" for k in range(len(self.in_sizes))]
        self._keys += [f"hidden_block.hidden_layers.{2 * k}" for k in range(len(self.hidden_sizes))]
        if self.dueling_units:
            assert self.dueling_type in DUELING_TYPES, self.dueling_type
            H = self.dueling_units
            self.v_hidden, self.v_out = lin(prev, H), lin(H, 1)
            self.adv_hidden, self.adv_out = lin(prev, H), lin(H, self.n_actions)
            head = f"hidden_block.hidden_layers.{2 * len(self.hidden_sizes)}"  # the DuelingNetworkBlock: v_layers / adv_layers = [Linear, ReLU, Linear]
            self._keys += [head + ".v_layers.0", head + ".v_layers.2", head + ".adv_layers.0", head + ".adv_layers.2"]
        else:
            self.out_layer = nn.Linear(prev, self.n_actions * max(self.n_atoms, 1))
            if self.n_atoms:  # (float32(linspace in float64): what the expectation multiplies by, c51.py:93)
                self.register_buffer("support", torch.linspace(self.v_min, self.v_max, self.n_atoms, dtype=torch.float64).to(torch.float32), persistent=False)
            self._keys.append("out_layer")
        self.weights_version = 0

    @property
    def widths(self):
        return self.in_sizes + self.hidden_sizes

    def forward(self, x):
        if self.n_atoms:  # the expectations over the support (c51.py:93)
            return (self.dist(x) * self.support).sum(-1)
        x = x.reshape(x.shape[0], -1)
        for layer in self.layers:
            x = F.relu(layer(x))
        if not self.dueling_units:
            return self.out_layer(x)
        v, adv = self.v_out(F.relu(self.v_hidden(x))), self.adv_out(F.relu(self.adv_hidden(x)))
        if self.dueling_type == "average":
            return v + adv - torch.mean(adv, dim=-1, keepdim=True)
        return v + adv

    def logits(self, x):
        """[rows][A][N] logits of the categorical head."""
        x = x.reshape(x.shape[0], -1)
        for layer in self.layers:
            x = F.relu(layer(x))
        return self.out_layer(x).view(-1, self.n_actions, self.n_atoms)

    def dist(self, x):
        """[rows][A][N] probabilities over the atoms (c51.py:92)."""
        return torch.softmax(self.logits(x), dim=2)

    def _linears(self):
        if self.dueling_units:
            return list(self.layers) + [self.v_hidden, self.v_out, self.adv_hidden, self.adv_out]
        return list(self.layers) + [self.out_layer]

    def kernel_parameters(self):
        """The tensors libsrlx binds, in the reference's key order: weight then bias of every layer, out_layer (or the head's v_layers.0, v_layers.2,
        adv_layers.0, adv_layers.2) last."""
        ps = []
        for lin in self._linears():
            ps += [lin.w_mu, lin.b_mu] if isinstance(lin, NoisyLinear) else [lin.weight, lin.bias]
        return ps

    def kernel_sigmas(self):
        """One entry per `kernel_parameters()` tensor: the sigma tensor of a noisy layer's weight / bias, None for a plain layer's."""
        ss = []
        for lin in self._linears():
            ss += [lin.w_sigma, lin.b_sigma] if isinstance(lin, NoisyLinear) else [None, None]
        return ss

    @staticmethod
    def _named(key, lin):
        """(reference key, tensor) pairs of one layer in the reference's parameter order."""
        if isinstance(lin, NoisyLinear):
            return [(key + ".w_mu", lin.w_mu), (key + ".w_sigma", lin.w_sigma), (key + ".b_mu", lin.b_mu), (key + ".b_sigma", lin.b_sigma)]
        return [(key + ".weight", lin.weight), (key + ".bias", lin.bias)]

    def load_reference_state_dict(self, sd):
        self.weights_version += 1
        with torch.no_grad():
            for key, lin in zip(self._keys, self._linears()):
                for k, t in self._named(key, lin):
                    t.copy_(sd[k])
        return self

    def reference_state_dict(self):
        sd = {}
        for key, lin in zip(self._keys, self._linears()):
            for k, t in self._named(key, lin):
                sd[k] = t.detach().clone()
        return sd


class MLPQHandle:
    """One libsrlx handle over an EngineMLPQNet's parameters (zero copy).  `max_batch` > 0: the handle trains -- gradient tensors (`p.grad`) and, with `lr`,
    torch's Adam state are bound, and `train_step` / `train_nstep` run the whole update in two launches.  A dueling net gets a srlx_mlpq_create_dueling handle
    (`max_nstep`: the longest item its `train_nstep` takes).  A noisy net's sigma tensors, their gradients and Adam state are bound beside the mu tensors'
    (srlx_mlpq_bind_noisy, `noise_seed`: the key of the handle's noise stream; srlx.h: the draw-id contract).  A net with `n_atoms` gets a
    srlx_mlpq_create_categorical handle: `forward` writes expectations and `train_categorical` is its update."""

    def __init__(self, net: EngineMLPQNet, max_rows: int, device: int = 0, max_batch: int = 0, lr: Optional[float] = None, betas=(0.9, 0.999),
                 eps: float = 1e-8, write_grads: bool = True, max_nstep: int = 7, noise_seed: int = 0):
        self.lib = N.lib()
        self.net = net
        widths = (ctypes.c_int * 3)(*(list(net.widths) + [0, 0, 0])[:3])
        h = N.c_p()
        if getattr(net, "n_atoms", 0):
            N.check(self.lib.srlx_mlpq_create_categorical(ctypes.byref(h), net.obs_dim, len(net.widths), ctypes.cast(widths, N.c_p), net.n_actions, net.n_atoms,
                                                          float(net.v_min), float(net.v_max), int(max_rows), int(max_batch), int(device)))
        elif net.dueling_units:
            N.check(self.lib.srlx_mlpq_create_dueling(ctypes.byref(h), net.obs_dim, len(net.widths), ctypes.cast(widths, N.c_p), net.dueling_units,
                                                      DUELING_TYPES[net.dueling_type], net.n_actions, int(max_rows), int(max_batch), int(max_nstep), int(device)))
        else:
            N.check(self.lib.srlx_mlpq_create(ctypes.byref(h), net.obs_dim, len(net.widths), ctypes.cast(widths, N.c_p), net.n_actions, int(max_rows),
                                              int(max_batch), int(device)))
        self.h = h
        self.params = net.kernel_parameters()
        assert all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in self.params)
        self._ptab = (N.c_p * len(self.params))(*[p.data_ptr() for p in self.params])
        N.check(self.lib.srlx_mlpq_bind(h, ctypes.cast(self._ptab, N.c_p)))
        self.exp_avg = self.exp_avg_sq = None
        self.noise_seed = int(noise_seed) & (2**64 - 1)
        self.sigmas = net.kernel_sigmas() if getattr(net, "noisy", False) else []
        self.exp_avg_sigma = self.exp_avg_sq_sigma = None
        table = lambda ts: (N.c_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
        if self.sigmas:
            assert all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in self.sigmas)
            self._stab = table(self.sigmas)
            N.check(self.lib.srlx_mlpq_bind_noisy(h, ctypes.cast(self._stab, N.c_p), ctypes.c_uint64(self.noise_seed)))
        if max_batch > 0:
            for p in self.params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            if write_grads:
                self._gtab = (N.c_p * len(self.params))(*[p.grad.data_ptr() for p in self.params])
                N.check(self.lib.srlx_mlpq_bind_grads(h, ctypes.cast(self._gtab, N.c_p)))
            if lr is not None:
                self.exp_avg = [torch.zeros_like(p) for p in self.params]
                self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
                self._mtab = (N.c_p * len(self.params))(*[t.data_ptr() for t in self.exp_avg])
                self._vtab = (N.c_p * len(self.params))(*[t.data_ptr() for t in self.exp_avg_sq])
                N.check(self.lib.srlx_mlpq_bind_adam(h, ctypes.cast(self._mtab, N.c_p), ctypes.cast(self._vtab, N.c_p), float(lr), float(betas[0]), float(betas[1]),
                                                     float(eps)))
            if self.sigmas:
                for t in self.sigmas:
                    if t is not None and t.grad is None:
                        t.grad = torch.zeros_like(t)
                if write_grads:
                    self._sgtab = table([None if t is None else t.grad for t in self.sigmas])
                    N.check(self.lib.srlx_mlpq_bind_noisy_grads(h, ctypes.cast(self._sgtab, N.c_p)))
                if lr is not None:
                    self.exp_avg_sigma = [None if t is None else torch.zeros_like(t) for t in self.sigmas]
                    self.exp_avg_sq_sigma = [None if t is None else torch.zeros_like(t) for t in self.sigmas]
                    self._smtab, self._svtab = table(self.exp_avg_sigma), table(self.exp_avg_sq_sigma)
                    N.check(self.lib.srlx_mlpq_bind_noisy_adam(h, ctypes.cast(self._smtab, N.c_p), ctypes.cast(self._svtab, N.c_p)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize()
                self.lib.srlx_mlpq_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- NoisyLinear: the handle's draw counter and its noise (srlx.h: the draw-id contract) ----
    def next_draw(self) -> int:
        """The id the handle's next pass will use (synchronises the device)."""
        out = N.c_i64(0)
        N.check(self.lib.srlx_mlpq_noisy_draw(self.h, None, ctypes.byref(out)))
        return int(out.value)

    def set_next_draw(self, draw: int):
        N.check(self.lib.srlx_mlpq_noisy_draw(self.h, ctypes.byref(N.c_i64(int(draw))), None))

    def eps(self, draw: int, k: int) -> torch.Tensor:
        """The noise of tensor `k` (kernel_parameters() index) under draw id `draw`, in the tensor's shape."""
        out = torch.empty_like(self.params[k])
        N.check(self.lib.srlx_mlpq_noisy_eps(self.h, int(draw), int(k), N.tptr(out), N.torch_stream_ptr()))
        return out

    def forward(self, rows: int, obs, offsets=None, q=None, eps=None, seed: int = 0, counter=None, actions=None):
        """Q of `rows` observations (obs: a float32 tensor, or a device address with `offsets` int64 [rows] element offsets) and, with `actions`, the
        epsilon-greedy action of every row in the same launch."""
        base = obs if isinstance(obs, int) else obs.data_ptr()
        N.check(self.lib.srlx_mlpq_forward(self.h, int(rows), N.c_p(base), N.tptr(offsets), N.tptr(q), N.tptr(eps), ctypes.c_uint64(seed & (2**64 - 1)),
                                           N.tptr(counter), N.tptr(actions), N.torch_stream_ptr()))
        return q

    def train_step(self, target: "MLPQHandle", batch: int, obs_base: int, offsets, actions, rewards, terminated, weights, discount: float, double_dqn: bool,
                   rescale: bool, steps_taken, q0, target_out, loss, priorities):
        N.check(self.lib.srlx_mlpq_train_step(self.h, target.h, int(batch), N.c_p(obs_base), N.tptr(offsets), N.tptr(actions), N.tptr(rewards), N.tptr(terminated),
                                              N.tptr(weights), float(discount), int(bool(double_dqn)), int(bool(rescale)), N.tptr(steps_taken), N.tptr(q0),
                                              N.tptr(target_out), N.tptr(loss), N.tptr(priorities), N.torch_stream_ptr()))

    def train_nstep(self, target: "MLPQHandle", batch: int, n: int, obs_base: int, offsets, actions, rewards, terminated, weights, discount: float,
                    retrace_h: float, double_dqn: bool, rescale: bool, steps_taken, q0, target_out, loss, priorities):
        """One n-step retrace update (rainbow.py:185-287, model_torch.py:85-122): offsets int64 [B][n + 1], actions / rewards / terminated [B][n]."""
        N.check(self.lib.srlx_mlpq_train_nstep(self.h, target.h, int(batch), int(n), N.c_p(obs_base), N.tptr(offsets), N.tptr(actions), N.tptr(rewards),
                                               N.tptr(terminated), N.tptr(weights), float(discount), float(retrace_h), int(bool(double_dqn)), int(bool(rescale)),
                                               N.tptr(steps_taken), N.tptr(q0), N.tptr(target_out), N.tptr(loss), N.tptr(priorities), N.torch_stream_ptr()))

    def train_categorical(self, batch: int, obs_base: int, offsets, actions, rewards, terminated, discount: float, steps_taken, q0, p0, m, loss, item_loss):
        """One C51 update (c51.py:70-142): offsets int64 [B][2], actions / rewards / terminated [B]; q0 [B][A] expectations, p0 / m [B][N], item_loss [B]."""
        N.check(self.lib.srlx_mlpq_train_categorical(self.h, int(batch), N.c_p(obs_base), N.tptr(offsets), N.tptr(actions), N.tptr(rewards), N.tptr(terminated),
                                                     float(discount), N.tptr(steps_taken), N.tptr(q0), N.tptr(p0), N.tptr(m), N.tptr(loss), N.tptr(item_loss),
                                                     N.torch_stream_ptr()))

    def publish_to(self, dst: "MLPQHandle"):
        """Every parameter of this handle's network into `dst`'s (one launch, on the current stream)."""
        N.check(self.lib.srlx_mlpq_publish(self.h, dst.h, N.torch_stream_ptr()))


class CartPoleVecEnv:
    """E device-resident CartPole-v1 environments (envs/cartpole.py, libsrlx srlx_cartpole_step): float64 state, float32 observations.  A lane that ended gets
    its next episode on the NEXT lock-step, which only delivers that episode's first observation (the store's needs_reset protocol)."""

    capturable = True

    def __init__(self, replay: DeviceReplay, max_steps: int = 500, seed: Optional[int] = None):
        assert not replay.obs_uint8 and replay.F == 4
        self.replay, self.E, self.max_steps = replay, replay.E, int(max_steps)
        self.seed = replay.seed if seed is None else int(seed)
        d = replay.dev
        self.lib = N.lib()
        self.state = torch.zeros((self.E, 4), dtype=torch.float64, device=d)
        self.steps = torch.zeros(self.E, dtype=torch.int32, device=d)
        self.episodes = torch.zeros(self.E, dtype=torch.int32, device=d)
        self.next_obs = torch.zeros((self.E, 4), dtype=torch.float32, device=d)
        self.rewards = torch.zeros(self.E, dtype=torch.float32, device=d)
        self.terminated = torch.zeros(self.E, dtype=torch.uint8, device=d)
        self.done = torch.zeros(self.E, dtype=torch.uint8, device=d)

    def reset(self) -> torch.Tensor:
        N.check(self.lib.srlx_cartpole_step(self.E, N.tptr(self.state), N.tptr(self.steps), N.tptr(self.episodes), None, None, self.max_steps, ctypes.c_uint64(self.seed),
                                            N.tptr(self.next_obs), None, None, None, N.torch_stream_ptr()))
        return self.next_obs.clone()

    def step(self, actions: torch.Tensor):
        N.check(self.lib.srlx_cartpole_step(self.E, N.tptr(self.state), N.tptr(self.steps), N.tptr(self.episodes), self.replay.needs_reset_ptr, N.tptr(actions),
                                            self.max_steps, ctypes.c_uint64(self.seed), N.tptr(self.next_obs), N.tptr(self.rewards), N.tptr(self.terminated),
                                            N.tptr(self.done), N.torch_stream_ptr()))
        return self.next_obs, self.rewards, self.terminated, self.done


class PendulumLaneVecEnv:
    """E device-resident Pendulum-v1 environments for a lane engine (envs/pendulum.py, libsrlx srlx_pendulum_lane_step): float64 state (th, thdot), float32
    observations (cos th, sin th, thdot), one float32 torque per lane.  `CartPoleVecEnv`'s contract, the store's needs_reset protocol included.  (The fused PPO
    engine's `device/ppo.py: PendulumVecEnv` resets itself inside its step and keeps float32 state: another environment.)"""

    capturable = True

    def __init__(self, replay, max_steps: int = 200, seed: Optional[int] = None):
        assert not replay.obs_uint8 and replay.F == 3
        self.replay, self.E, self.max_steps = replay, replay.E, int(max_steps)
        self.seed = replay.seed if seed is None else int(seed)
        d = replay.dev
        self.lib = N.lib()
        self.state = torch.zeros((self.E, 2), dtype=torch.float64, device=d)
        self.steps = torch.zeros(self.E, dtype=torch.int32, device=d)
        self.episodes = torch.zeros(self.E, dtype=torch.int32, device=d)
        self.next_obs = torch.zeros((self.E, 3), dtype=torch.float32, device=d)
        self.rewards = torch.zeros(self.E, dtype=torch.float32, device=d)
        self.terminated = torch.zeros(self.E, dtype=torch.uint8, device=d)
        self.done = torch.zeros(self.E, dtype=torch.uint8, device=d)

    def reset(self) -> torch.Tensor:
        N.check(self.lib.srlx_pendulum_lane_step(self.E, N.tptr(self.state), N.tptr(self.steps), N.tptr(self.episodes), None, None, self.max_steps,
                                                 ctypes.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), N.tptr(self.next_obs), None, None, None, N.torch_stream_ptr()))
        return self.next_obs.clone()

    def step(self, torques: torch.Tensor):
        """`torques`: float32, E elements ([E] or [E][1])."""
        assert torques.dtype == torch.float32 and torques.numel() == self.E and torques.is_contiguous()
        N.check(self.lib.srlx_pendulum_lane_step(self.E, N.tptr(self.state), N.tptr(self.steps), N.tptr(self.episodes), self.replay.needs_reset_ptr, N.tptr(torques),
                                                 self.max_steps, ctypes.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), N.tptr(self.next_obs), N.tptr(self.rewards),
                                                 N.tptr(self.terminated), N.tptr(self.done), N.torch_stream_ptr()))
        return self.next_obs, self.rewards, self.terminated, self.done


@dataclass
class VectorQConfig:
    # --- dqn.Config fields (srl/algorithms/dqn/dqn.py:50-101)
    batch_size: int = 32
    epsilon: float = 0.1
    test_epsilon: float = 0.0
    lr: float = 0.001
    discount: float = 0.99
    target_model_update_interval: int = 1000
    enable_reward_clip: bool = False
    enable_double_dqn: bool = True
    enable_rescale: bool = False
    # --- memory
    memory_capacity: int = 100_000
    memory_warmup_size: int = 1000
    memory_alpha: float = 0.0
    memory_beta_initial: float = 0.4
    memory_beta_steps: int = 1_000_000
    memory_epsilon: float = 0.0001
    memory_has_duplicate: bool = False
    # --- model: input value block layers, then the hidden block's
    obs_dim: int = 4
    in_sizes: tuple = ()
    hidden_sizes: tuple = (512,)
    n_actions: int = 2
    # --- rainbow.Config (srl/algorithms/rainbow/rainbow.py:57-107): dueling_units = the hidden block's layer_sizes[-1] (0: the plain out_layer; `hidden_sizes`
    # is then layer_sizes[:-1]), its dueling_type ("average" or ""), multisteps, retrace_h
    dueling_units: int = 0
    dueling_type: str = "average"
    multisteps: int = 1
    retrace_h: float = 1.0
    # rainbow.Config.enable_noisy_dense (rainbow.py:46): NoisyLinear in the hidden block's MLP layers and the dueling head, greedy acting (needs dueling_units)
    enable_noisy_dense: bool = False
    # --- c51.Config (srl/algorithms/c51/config.py:50-52): categorical_atoms = N > 0 turns out_layer into the [A][N] categorical head on the support
    # linspace(v_min, v_max, N); the update is c51.py:70-142 on the online network alone (no target network, no dueling head, 1-step items, plain layers)
    categorical_atoms: int = 0
    categorical_v_min: float = -10.0
    categorical_v_max: float = 10.0
    # --- engine
    n_envs: int = 1024
    seed: int = 0


class VectorQEngine:
    """E lock-stepped environments and DQN (or, with `dueling_units` / `multisteps`, Rainbow) updates on one GPU for flat observations, every network pass in
    libsrlx:
      actor_front   1 launch (Q rows + epsilon-greedy from the store's float ring) + the environments' step
      actor_commit  ring commit (also writes the next pass's row table and advances the policy counter) + the replay's add
      learner_step  the replay's draw + gather, srlx_mlpq_train_step (or srlx_mlpq_train_nstep; 2 launches), the priority write-back (train_count += 1 on the device)
    Actors and learner share one stream and one parameter set (no copy to refresh).  With `enable_noisy_dense` both networks hold NoisyLinear layers: every pass
    costs one more launch (the draw's effective tensors; the learner's three draws share one), the draw ids live on the device, so the captured update replays
    with fresh noise, and every lane acts greedily on its noisy Q row (`eps` = 0).  With `categorical_atoms` the engine is C51's: the actors' launch turns
    the logit rows into expectations before the same selection, the update is srlx_mlpq_train_categorical (2 launches), and there is no target network --
    `q_target` / `inf_target` are None and `sync` stays 0."""

    overlap = False

    def __init__(self, cfg: VectorQConfig, device: int = 0, env=None):
        self.cfg = cfg
        self.dev = torch.device(f"cuda:{device}")
        self.lib = N.lib()
        torch.manual_seed(cfg.seed)
        E, B, A, D = cfg.n_envs, cfg.batch_size, cfg.n_actions, cfg.obs_dim
        n = int(cfg.multisteps)
        self.categorical = int(cfg.categorical_atoms) > 0
        assert not self.categorical or not cfg.dueling_units, "categorical_atoms: C51's head is a plain out_layer (c51.py:29-32); dueling_units must be 0"
        assert not self.categorical or n == 1, "categorical_atoms: C51's target is the 1-step distributional Bellman update (c51.py:102-121); multisteps must be 1"
        assert not self.categorical or not cfg.enable_noisy_dense, "categorical_atoms: C51 builds plain Dense layers; enable_noisy_dense must be False"
        self.nstep = n > 1 or cfg.dueling_units > 0  # srlx_mlpq_train_nstep; the defaults keep srlx_mlpq_train_step
        ring_len = -(-cfg.memory_capacity // E) + n + 1  # item_len * E >= capacity (n_step n + window 1)
        self.replay = DeviceReplay(E, ring_len, D, 1, n, A, B, False, cfg.enable_reward_clip, cfg.memory_alpha, cfg.memory_beta_initial, cfg.memory_beta_steps,
                                   cfg.memory_epsilon, cfg.memory_warmup_size, cfg.seed, device, has_duplicate=cfg.memory_has_duplicate,
                                   # (a draw without replacement rejects repeats: 8 spare uniforms serve B <= 64 as in RainbowEngine; B = 128 from 512 items needs ~16)
                                   sample_slack=8 if B <= 64 else 4 * B)
        if env is None:
            self.env = CartPoleVecEnv(self.replay)
        else:
            self.env = env(self.replay) if callable(env) else env
        noisy = bool(cfg.enable_noisy_dense)
        assert not noisy or cfg.dueling_units > 0, "enable_noisy_dense needs the dueling head (dueling_units > 0)"
        cat = dict(n_atoms=int(cfg.categorical_atoms), v_min=cfg.categorical_v_min, v_max=cfg.categorical_v_max) if self.categorical else {}
        self.q_online = EngineMLPQNet(D, cfg.in_sizes, cfg.hidden_sizes, A, cfg.dueling_units, cfg.dueling_type, noisy, **cat).to(self.dev)
        self.q_actor = self.q_online
        # (the two networks' noise streams are independent: the target pass has its own layers, model_torch.py:103)
        self.inf_online = MLPQHandle(self.q_online, max(E, B), device, max_batch=B, lr=cfg.lr, max_nstep=n, noise_seed=cfg.seed ^ 0x6E6F6973)
        if self.categorical:  # c51.py:91 evaluates s' with the online network: there is no target network to keep or to sync
            self.q_target = self.inf_target = None
        else:
            self.q_target = EngineMLPQNet(D, cfg.in_sizes, cfg.hidden_sizes, A, cfg.dueling_units, cfg.dueling_type, noisy).to(self.dev)
            self.q_target.load_state_dict(self.q_online.state_dict())
            self.inf_target = MLPQHandle(self.q_target, max(E, B), device, max_nstep=n, noise_seed=cfg.seed ^ 0x74677473)
        d = self.dev
        self.eps = torch.full((E,), 0.0 if noisy else float(cfg.epsilon), dtype=torch.float32, device=d)  # rainbow.py:305-309: no epsilon for a noisy net
        self.actions = torch.zeros(E, dtype=torch.int32, device=d)
        self.policy_counter = torch.zeros(1, dtype=torch.int64, device=d)
        self.train_count_dev = torch.zeros(1, dtype=torch.int64, device=d)
        self.replay.count_updates_in(self.train_count_dev)  # train_count += 1 rides on the priority write-back (= the Adam steps taken)
        self.q0 = torch.zeros((B, A), dtype=torch.float32, device=d)
        self.target = torch.zeros(B, dtype=torch.float32, device=d)
        self.loss = torch.zeros(1, dtype=torch.float32, device=d)
        self.priorities = torch.zeros(B, dtype=torch.float32, device=d)  # (categorical: the items' cross-entropies stand here; alpha = 0 ignores the values)
        if self.categorical:
            self.p0 = torch.zeros((B, cat["n_atoms"]), dtype=torch.float32, device=d)
            self.m = torch.zeros((B, cat["n_atoms"]), dtype=torch.float32, device=d)
        self.train_count = self.sync_count = self.total_env_steps = 0
        self.ledger = None
        self._learner_graph = None
        self.first_obs = self.env.reset()
        self.replay.reset_all(self.first_obs)

    # ---- actors -----------------------------------------------------------------------------------
    def actor_front(self, events=None):
        r = self.replay
        off = r.frame_table_current()  # (no launch: the last commit wrote it)
        self.inf_online.forward(self.cfg.n_envs, r.obs_base, off.view(-1), eps=self.eps, seed=self.cfg.seed ^ 0xAC7, counter=self.policy_counter, actions=self.actions)
        self.env.step(self.actions)

    def actor_commit(self):
        e = self.env
        if self.ledger is not None:  # before the commit: the store's needs_reset view still marks the lanes that only received a first observation
            self.ledger.account(e.rewards, e.done, self.replay.needs_reset_ptr)
        self.replay.commit(self.actions, e.rewards, e.terminated, e.done, e.next_obs, next_table=True, bump=self.policy_counter)
        self.total_env_steps += self.cfg.n_envs

    def actor_step(self):
        self.actor_front()
        self.actor_commit()

    def join_learner(self):
        """(actors and learner share one stream)"""

    def refresh_actor_copy(self):
        """(the actors read the online parameters themselves)"""

    # ---- learner ----------------------------------------------------------------------------------
    def _learner_body(self):
        cfg, r = self.cfg, self.replay
        b = r.sample_items(self.train_count_dev, all_states=True)
        if self.categorical:
            self.inf_online.train_categorical(cfg.batch_size, r.obs_base, r.frame_off_all, b.actions, b.rewards, b.terminated, cfg.discount, self.train_count_dev,
                                              self.q0, self.p0, self.m, self.loss, self.priorities)
        elif self.nstep:
            self.inf_online.train_nstep(self.inf_target, cfg.batch_size, cfg.multisteps, r.obs_base, r.frame_off_all, b.actions, b.rewards, b.terminated, b.weights,
                                        cfg.discount, cfg.retrace_h, cfg.enable_double_dqn, cfg.enable_rescale, self.train_count_dev, self.q0, self.target,
                                        self.loss, self.priorities)
        else:
            self.inf_online.train_step(self.inf_target, cfg.batch_size, r.obs_base, r.frame_off_all, b.actions, b.rewards, b.terminated, b.weights, cfg.discount,
                                       cfg.enable_double_dqn, cfg.enable_rescale, self.train_count_dev, self.q0, self.target, self.loss, self.priorities)
        r.update(b.indices, self.priorities)  # model_torch.py:121-122; train_count_dev += 1 in the same launch

    def learner_step(self) -> bool:
        if self.replay.is_warmup_needed():
            return False
        if self._learner_graph is not None:
            self._learner_graph.replay()
        else:
            self._learner_body()
        if not self.categorical and self.train_count % self.cfg.target_model_update_interval == 0:  # model_torch.py:125-127 (fires at 0 too)
            self.sync_target()
        self.train_count += 1
        return True

    def sync_target(self):
        self.inf_online.publish_to(self.inf_target)
        self.sync_count += 1

    def capture_graphs(self, actor: bool = True, learner: bool = True, warm_actor: bool = True, warm_learner: bool = True):
        """The update (draw + gather, the two network launches, the write-back) as one HIP graph once the replay is warm; the actors stay eager."""
        torch.cuda.synchronize(self.dev)
        if actor and warm_actor:
            self.actor_step()
        if learner and warm_learner:
            self.learner_step()  # a real update, eager
        if learner and not self.replay.is_warmup_needed():
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    self._learner_body()
            torch.cuda.current_stream(self.dev).wait_stream(side)
            self._learner_graph = g
        torch.cuda.synchronize(self.dev)

    def step(self, learner_updates: int = 1):
        self.actor_step()
        for _ in range(learner_updates):
            self.learner_step()

    def info(self):
        self.replay.check_draws()
        return dict(loss=float(self.loss.item()), train_count=self.train_count, sync=self.sync_count, memory=self.replay.length())
