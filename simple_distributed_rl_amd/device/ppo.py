"""PPO on the vectorised path (BASELINE.json config 5: "PPO continuous (Pendulum-shaped obs), 4096
vectorized envs, fused GAE kernel, data-parallel").

E lock-stepped environments live on the GPU.  A rollout of T steps costs 3 launches per step around the network
(`srlx_ppo_normal_act` = sample + log-prob, `srlx_pendulum_step` = environment + auto-reset, buffer writes are slices
of preallocated [T][E] tensors); the advantages of all E x T transitions come from ONE `srlx_gae_scan`; every
minibatch update is forward -> ONE `srlx_ppo_loss_normal` (losses + gradient seeds for loc / log_scale / v) ->
backward -> global-norm clip -> Adam.  Nothing crosses to the host inside an iteration.

Reference semantics kept (srl/algorithms/ppo/ppo.py): the Normal head with the stable-gradient log-scale clip,
log-prob floor log(1e-6) (:322), GAE with no bootstrap at an episode end, truncation included (:389-404), the SAME
GAE value used as v_target and as advantage with `baseline_type="advantage"` subtracting V again (:214-215,121-122)
-- `v_target="return"` selects the textbook target (advantage + V) instead --, clipped surrogate, value clipping,
entropy bonus on the taken action's log-prob (:166), global gradient clipping (:240-241).

Round 6: with the reference's default blocks (hidden (64, 64), value (64,), policy (64,)) the network itself is libsrlx code too (`fused`, the default then;
csrc/srlx_ppo_net.hip): the WHOLE rollout of an iteration -- T network passes, policy samples, environment steps, the buffers, V(s_T), the GAE scan -- is one
launch, a minibatch update is three (forward + loss + backward; gradient reduction; clip + Adam), and an iteration is ~55 launches instead of ~1700 framework
kernels.  The parameters are one flat float32 vector; the `ActorCritic` module's tensors are views of it.  `fused=False` keeps the torch-autograd path as the
yardstick the fused one is tested against.

Discrete actions (`PPODeviceConfig.n_actions > 0`): a categorical head (ppo.py:316-324, CategoricalDist) on E self-resetting CartPole environments (envs/cartpole.py
on the device, float64 state; `episode_len` is its step limit).  The same three-launch update and one-launch rollout with the head swapped (`srlx_ppo_cat_*`); the
torch-autograd yardstick is log_softmax -> `srlx_ppo_categorical_act` / `srlx_ppo_loss_logpi`.  `export_to` / `load_from` exchange the weights with the PPO plugin's
`Parameter` (algorithms/ppo.py), so a policy trained here is evaluated through `Runner.evaluate()`.

What a `ppo.Config` asks beyond the network (`vector_runner.ppo_config_from` maps one): `lr_scheduler` -- evaluated INSIDE the clip + Adam launch from the step count in
device memory (`srlx_ppo_*_adam_sched`), so the captured update graph follows it; `baseline_type` "ave" / "std" / "normal" -- one `srlx_ppo_adv_baseline` launch per
minibatch in front of the minibatch launch (mean / population deviation of THAT minibatch, as the plugin's trainer normalises the batch it drew); `reward_clip`,
`state_clip`, `action_scale` / `action_offset` -- inside the one-launch rollout (`srlx_ppo_*_rollout_ex`), with torch ops around the step-wise kernels.  With none of
them set the engine launches exactly what it launched before they existed.

`surrogate_type="kl"` (ppo.py:138-146, :279-287): the policy term is ratio * adv - beta * KL(old || new), no ratio clip.  The rollout records the acting distribution
(`old_dist`: probs [T][E][n], or loc and clamped log-scale [T][E][A]; `srlx_ppo_*_rollout_kl`, the step-wise samplers `srlx_ppo_*_act_dist`), the minibatch launch
gathers it and adds the KL seeds (`srlx_ppo_*_minibatch_kl`; torch path: `srlx_ppo_loss_*_kl`), and beta is ONE float32 in device memory (`kl_beta`) which the launch
that forms the losses adapts after every minibatch -- so `capture_graphs()` works on both paths, and `export_to` / `load_from` carry beta in
`parameter.adaptive_kl_beta`.  Not data-parallel: each rank would adapt its own beta from its local kl_mean.

Data parallel (config 5): `DistributedPPO` gives every rank its own E environments and averages the gradients of
every minibatch with one all-reduce of the flat ~52 KB gradient vector (latency-bound; RCCL over xGMI) -- the only exchange; with the fused network and RCCL
it sits INSIDE the captured update graph, between the gradient reduction and the clip + Adam launch.
"""
import ctypes
import math
import struct
from dataclasses import dataclass, field
from typing import Callable, Optional, Tuple

import torch
import torch.nn as nn

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.rl.schedulers.lr_scheduler import LRSchedulerConfig


@dataclass
class PPODeviceConfig:
    n_envs: int = 4096
    horizon: int = 32
    epochs: int = 4
    minibatches: int = 4
    episode_len: int = 200
    obs_dim: int = 3
    action_dim: int = 1
    hidden_sizes: Tuple[int, ...] = (64, 64)   # hidden_block (config.py:47)
    value_sizes: Tuple[int, ...] = (64,)       # value_block
    policy_sizes: Tuple[int, ...] = (64,)      # policy_block
    discount: float = 0.9
    gae_discount: float = 0.9
    baseline_type: str = "advantage"
    v_target: str = "gae"                      # "gae" = the reference's target (ppo.py:214), "return" = gae + V
    surrogate_type: str = "clip"
    policy_clip_range: float = 0.2
    enable_value_clip: bool = True
    value_clip_range: float = 0.2
    lr: float = 0.0002
    value_loss_weight: float = 1.0
    entropy_weight: float = 0.01
    global_gradient_clip_norm: float = 0.5
    stable_gradients_scale_range: Tuple[float, float] = (1e-10, 10)
    seed: int = 0
    n_actions: int = 0                         # 0: the Normal head on Pendulum; > 0: a categorical head on CartPole (obs_dim 4; action_dim unused; episode_len = max_steps).
    #                                            CartPole has two moves: action 1 pushes right, every other action pushes left -- n_actions 3..8 is accepted, but adds duplicates of "left"
    lr_scheduler: LRSchedulerConfig = field(default_factory=LRSchedulerConfig)  # constant by default; optimiser step k (0-based) runs at lr * factor(k) (ppo.Config: set_step(2000, 0.01))
    reward_clip: Optional[Tuple[float, float]] = None  # (lo, hi): what the buffers and GAE see; episode returns keep the raw reward (ppo.py:374-379)
    state_clip: Optional[Tuple[float, float]] = None   # (lo, hi): every observation the network reads or the buffers keep; never the environment's state
    action_scale: float = 1.0                  # the Normal head's action reaches the environment as action * action_scale + action_offset (ppo.py:336: [-1, 1] onto
    action_offset: float = 0.0                 # the action space's bounds; Pendulum: 2 and 0); b_act / b_logp keep the policy's own action
    adaptive_kl_target: float = 0.01           # surrogate_type "kl": beta halves below target / 1.5 and doubles above target * 1.5 while beta < 10 (ppo.py:279-287)
    adaptive_kl_beta: float = 0.5              # ... and starts here (ppo.py:177)


class ActorCritic(nn.Module):
    """in -> hidden_block -> {value_block -> V, policy_block -> (loc, log_scale)} (ppo.py:55-99); with `n_actions` the policy head is `logits_layer` and forward
    returns (v, logits)."""

    def __init__(self, cfg: PPODeviceConfig):
        super().__init__()

        def mlp(n_in, sizes):
            layers, n = [], n_in
            for s in sizes:
                layers += [nn.Linear(n, s), nn.ReLU()]
                n = s
            return nn.Sequential(*layers), n

        self.hidden_block, n = mlp(cfg.obs_dim, cfg.hidden_sizes)
        self.value_block, nv = mlp(n, cfg.value_sizes)
        self.value_out_layer = nn.Linear(nv, 1)
        self.policy_block, n_pol = mlp(n, cfg.policy_sizes)
        self.categorical = head_of(cfg).cat
        if self.categorical:
            self.logits_layer = nn.Linear(n_pol, cfg.n_actions)  # categorical_dist_block.py:134-153
        else:
            self.loc_layer = nn.Linear(n_pol, cfg.action_dim)
            self.log_scale_layer = nn.Linear(n_pol, cfg.action_dim)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight)  # ppo.py:60-61
                nn.init.zeros_(m.bias)
        if self.categorical:
            nn.init.zeros_(self.logits_layer.weight)  # categorical_dist_block.py:147: the policy starts uniform
        else:
            nn.init.trunc_normal_(self.loc_layer.bias, std=0.05)  # normal_dist_block.py:101-106

    def forward(self, x):
        h = self.hidden_block(x)
        p = self.policy_block(h)
        v = self.value_out_layer(self.value_block(h)).squeeze(-1)
        if self.categorical:
            return v, self.logits_layer(p)
        return v, self.loc_layer(p), self.log_scale_layer(p)

    def linears(self):
        """The Linear layers in the plugin network's order (algorithms/ppo.py:ActorCriticNetwork): hidden, value, value_out, policy, policy_out [, log_scale_out]."""
        lin = lambda seq: [m for m in seq if isinstance(m, nn.Linear)]  # noqa: E731
        heads = [self.logits_layer] if self.categorical else [self.loc_layer, self.log_scale_layer]
        return lin(self.hidden_block) + lin(self.value_block) + [self.value_out_layer] + lin(self.policy_block) + heads


class PendulumVecEnv:
    """E Pendulum-shaped environments stepped by `srlx_pendulum_step` (state stays on the device)."""

    def __init__(self, n_envs: int, episode_len: int, seed: int, device: torch.device):
        self.E, self.episode_len, self.seed, self.dev, self.lib = n_envs, episode_len, seed, device, N.lib()
        g = torch.Generator(device="cpu").manual_seed(seed)
        th = (torch.rand(n_envs, generator=g) * 2 - 1) * math.pi
        thd = torch.rand(n_envs, generator=g) * 2 - 1
        self.state = torch.stack([th, thd], dim=1).to(device).contiguous()
        self.t = torch.zeros(n_envs, dtype=torch.int32, device=device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.obs = torch.stack([torch.cos(self.state[:, 0]), torch.sin(self.state[:, 0]), self.state[:, 1]], dim=1).contiguous()

    def step(self, action: torch.Tensor, obs_out: torch.Tensor, reward_out: torch.Tensor, done_out: torch.Tensor):
        N.check(self.lib.srlx_pendulum_step(self.E, N.tptr(self.state), N.tptr(self.t), N.tptr(action), self.episode_len, self.seed, N.tptr(self.counter),
                                            N.tptr(obs_out), N.tptr(reward_out), N.tptr(done_out), N.torch_stream_ptr()))


class CartPoleAutoVecEnv:
    """E CartPole environments (envs/cartpole.py) stepped by `srlx_cartpole_autoreset_step`: float64 state on the device, a lane starts its next episode in the step
    that ends one.  `episode_len` is the step limit (max_steps)."""

    def __init__(self, n_envs: int, episode_len: int, seed: int, device: torch.device):
        self.E, self.episode_len, self.seed, self.dev, self.lib = n_envs, episode_len, seed, device, N.lib()
        self.state = torch.zeros((n_envs, 4), dtype=torch.float64, device=device)
        self.t = torch.zeros(n_envs, dtype=torch.int32, device=device)
        self.episodes = torch.zeros(n_envs, dtype=torch.int32, device=device)
        self.obs = torch.zeros((n_envs, 4), dtype=torch.float32, device=device)
        # every lane's first episode: the reset of srlx_cartpole_step (the same key the self-resetting step uses)
        N.check(self.lib.srlx_cartpole_step(n_envs, N.tptr(self.state), N.tptr(self.t), N.tptr(self.episodes), None, None, episode_len, seed, N.tptr(self.obs), None, None, None,
                                            N.torch_stream_ptr()))

    def step(self, action: torch.Tensor, obs_out: torch.Tensor, reward_out: torch.Tensor, done_out: torch.Tensor):
        N.check(self.lib.srlx_cartpole_autoreset_step(self.E, N.tptr(self.state), N.tptr(self.t), N.tptr(self.episodes), N.tptr(action), self.episode_len, self.seed,
                                                      N.tptr(obs_out), N.tptr(reward_out), N.tptr(done_out), N.torch_stream_ptr()))


def make_env(cfg: PPODeviceConfig, seed: int, device: torch.device):
    """The built-in environment of a configuration: CartPole under a categorical head, the Pendulum-shaped one otherwise."""
    return head_of(cfg).env_cls(cfg.n_envs, cfg.episode_len, seed, device)


BASELINES = {"advantage": "advantage", "v": "advantage", "": "none", "none": "none", "ave": "ave", "std": "std", "normal": "normal"}  # ppo.py:222-233 (+ the aliases)


def _f32(x: float) -> float:
    """x rounded to float32 (what a float field of a libsrlx struct holds): the torch ops of the step-wise path clip at the same bounds as the kernels."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _loss_args(cfg):
    return (int(BASELINES.get(cfg.baseline_type) == "advantage"), int(cfg.surrogate_type == "clip"), cfg.policy_clip_range, int(cfg.enable_value_clip), cfg.value_clip_range,
            cfg.value_loss_weight, cfg.entropy_weight)


def _kl_loss_args(cfg):  # the "kl" entry points: no surrogate switch, no clip range; the target in their place
    return (int(BASELINES.get(cfg.baseline_type) == "advantage"), int(cfg.enable_value_clip), cfg.value_clip_range, cfg.value_loss_weight, cfg.entropy_weight,
            cfg.adaptive_kl_target)


class NormalPendulumHead:
    """The Normal head (loc, log_scale per action dimension; ppo.py:316-339) on the Pendulum-shaped environment: `srlx_ppo_net_*`.  Every method takes the engine `e`
    and reads its environment, buffers and counters at call time (`e.env` may be swapped after construction)."""
    cat, env_cls, env_obs_dim, act_dtype, fused_sizes, envelope = False, PendulumVecEnv, 3, torch.float32, range(1, 5), "action_dim <= 4"

    def __init__(self, cfg, lib):
        self.size, self.act_shape = cfg.action_dim, (cfg.action_dim,)  # the head's size for libsrlx; b_act / b_logp are [T][E] + act_shape
        self.param_count, self.partials_floats = lib.srlx_ppo_net_param_count, lib.srlx_ppo_net_partials_floats
        self.adam, self.adam_sched, self.rollout_max_horizon = lib.srlx_ppo_net_adam, lib.srlx_ppo_net_adam_sched, lib.srlx_ppo_net_rollout_max_horizon
        self.kl_partials_floats = lib.srlx_ppo_net_kl_partials_floats
        self.dist_shapes = ((cfg.action_dim,), (cfg.action_dim,))  # "kl": the old distribution's buffers are [T][E] + these: loc, clamped log_scale

    def sample(self, e, loc, ls, action_out, logp_out, deterministic, dist_out=None):  # the step-wise path's policy sample + log-probability [+ the acting distribution]
        if dist_out is not None:
            N.check(e.lib.srlx_ppo_normal_act_dist(loc.numel(), N.tptr(loc), N.tptr(ls), e.ls_range[0], e.ls_range[1], e.cfg.seed ^ 0x61637400, N.tptr(e.act_counter),
                                                   int(deterministic), N.tptr(action_out), N.tptr(logp_out), N.tptr(dist_out[0]), N.tptr(dist_out[1]), N.torch_stream_ptr()))
            return
        N.check(e.lib.srlx_ppo_normal_act(loc.numel(), N.tptr(loc), N.tptr(ls), e.ls_range[0], e.ls_range[1], e.cfg.seed ^ 0x61637400, N.tptr(e.act_counter),
                                          int(deterministic), N.tptr(action_out), N.tptr(logp_out), N.torch_stream_ptr()))

    def forward(self, e, obs):  # the libsrlx network: (v [n], loc [n][A], log_scale [n][A])
        n, A = obs.shape[0], self.size
        v, loc, ls = (torch.empty(shape, dtype=torch.float32, device=e.dev) for shape in (n, (n, A), (n, A)))
        N.check(e.lib.srlx_ppo_net_forward(n, e.cfg.obs_dim, A, N.tptr(e.flat), N.tptr(obs.contiguous()), N.tptr(v), N.tptr(loc), N.tptr(ls), N.torch_stream_ptr()))
        return v, loc, ls

    def rollout(self, e):  # T steps of everything in ONE launch (csrc/srlx_ppo_net.hip: k_ppo_rollout<PendulumNormal>)
        cfg, env = e.cfg, e.env
        args = (cfg.n_envs, cfg.horizon, cfg.action_dim, N.tptr(e.flat), N.tptr(env.state), N.tptr(env.t), N.tptr(env.obs), env.episode_len, env.seed, N.tptr(env.counter),
                cfg.seed ^ 0x61637400, N.tptr(e.act_counter), e.ls_range[0], e.ls_range[1], cfg.discount, cfg.gae_discount, N.tptr(e.b_obs), N.tptr(e.b_act), N.tptr(e.b_logp),
                N.tptr(e.b_val), N.tptr(e.b_rew), N.tptr(e.b_done), N.tptr(e.b_adv), N.tptr(e._last_v), N.tptr(e.episode_return), N.tptr(e.finished_returns))
        if e.kl:
            N.check(e.lib.srlx_ppo_net_rollout_kl(*args, N.tptr(e.old_dist[0]), N.tptr(e.old_dist[1]), None if e.env_opts is None else ctypes.byref(e.env_opts),
                                                  N.torch_stream_ptr()))
        elif e.env_opts is None:
            N.check(e.lib.srlx_ppo_net_rollout(*args, N.torch_stream_ptr()))
        else:
            N.check(e.lib.srlx_ppo_net_rollout_ex(*args, ctypes.byref(e.env_opts), N.torch_stream_ptr()))

    def loss_and_seeds(self, e, obs, action, old_logp, adv, v_target, old_v, old_dist=None):
        v, loc, ls = e.net(obs)
        B, A = loc.shape
        g_loc, g_ls, g_v = torch.empty_like(loc), torch.empty_like(ls), torch.empty_like(v)
        if e.kl:
            e._keep_loss = (loc.detach().contiguous(), ls.detach().contiguous(), v.detach().contiguous()) + tuple(old_dist)
            N.check(e.lib.srlx_ppo_loss_normal_kl(
                B, A, N.tptr(e._keep_loss[0]), N.tptr(e._keep_loss[1]), e.ls_range[0], e.ls_range[1], N.tptr(action), N.tptr(old_logp), N.tptr(old_dist[0]), N.tptr(old_dist[1]),
                N.tptr(adv), N.tptr(e._keep_loss[2]), N.tptr(v_target), N.tptr(old_v), *_kl_loss_args(e.cfg), N.tptr(e.kl_beta), N.tptr(e.losses), N.tptr(g_loc), N.tptr(g_ls),
                N.tptr(g_v), N.torch_stream_ptr()))
            return (v, loc, ls), (g_v, g_loc, g_ls)
        N.check(e.lib.srlx_ppo_loss_normal(
            B, A, N.tptr(loc.detach()), N.tptr(ls.detach()), e.ls_range[0], e.ls_range[1], N.tptr(action), N.tptr(old_logp), N.tptr(adv), N.tptr(v.detach()),
            N.tptr(v_target), N.tptr(old_v), *_loss_args(e.cfg), N.tptr(e.losses), N.tptr(g_loc), N.tptr(g_ls), N.tptr(g_v), N.torch_stream_ptr()))
        return (v, loc, ls), (g_v, g_loc, g_ls)

    def minibatch(self, e, mb, rows, buffers, outputs):
        if e.kl:
            partials, grad, losses, st = outputs
            N.check(e.lib.srlx_ppo_net_minibatch_kl(mb, N.tptr(rows), e.cfg.obs_dim, self.size, *buffers, N.tptr(e.old_dist[0]), N.tptr(e.old_dist[1]), e.ls_range[0], e.ls_range[1],
                                                    *_kl_loss_args(e.cfg), N.tptr(e.kl_beta), partials, grad, losses, st))
            return
        N.check(e.lib.srlx_ppo_net_minibatch(mb, N.tptr(rows), e.cfg.obs_dim, self.size, *buffers, e.ls_range[0], e.ls_range[1], *_loss_args(e.cfg), *outputs))


class CategoricalCartPoleHead:
    """The categorical head (n_actions logits; ppo.py:316-324, CategoricalDist) on self-resetting CartPole: `srlx_ppo_cat_*`; one action index and one
    log-probability per step.  Same methods as the Normal head."""
    cat, env_cls, env_obs_dim, act_dtype, fused_sizes, envelope = True, CartPoleAutoVecEnv, 4, torch.int32, range(2, 9), "2 <= n_actions <= 8"

    def __init__(self, cfg, lib):
        if cfg.obs_dim != 4:
            raise ValueError("PPODeviceConfig(n_actions > 0) runs CartPole: obs_dim must be 4")
        if cfg.n_actions < 2:
            raise ValueError("a categorical policy needs at least 2 actions")
        self.size, self.act_shape = cfg.n_actions, ()
        self.param_count, self.partials_floats = lib.srlx_ppo_cat_param_count, lib.srlx_ppo_cat_partials_floats
        self.adam, self.adam_sched, self.rollout_max_horizon = lib.srlx_ppo_cat_adam, lib.srlx_ppo_cat_adam_sched, lib.srlx_ppo_cat_rollout_max_horizon
        self.kl_partials_floats = lib.srlx_ppo_cat_kl_partials_floats
        self.dist_shapes = ((cfg.n_actions,),)  # "kl": probs [T][E][n]

    def sample(self, e, logits, action_out, logp_out, deterministic, dist_out=None):
        if dist_out is not None:
            N.check(e.lib.srlx_ppo_categorical_act_dist(logits.shape[0], self.size, N.tptr(logits), e.cfg.seed ^ 0x61637400, N.tptr(e.act_counter), int(deterministic),
                                                        N.tptr(action_out), N.tptr(logp_out), N.tptr(dist_out[0]), N.torch_stream_ptr()))
            return
        N.check(e.lib.srlx_ppo_categorical_act(logits.shape[0], self.size, N.tptr(logits), e.cfg.seed ^ 0x61637400, N.tptr(e.act_counter), int(deterministic),
                                               N.tptr(action_out), N.tptr(logp_out), N.torch_stream_ptr()))

    def forward(self, e, obs):  # the libsrlx network: (v [n], logits [n][n_actions])
        n = obs.shape[0]
        v, logits = torch.empty(n, dtype=torch.float32, device=e.dev), torch.empty((n, self.size), dtype=torch.float32, device=e.dev)
        N.check(e.lib.srlx_ppo_cat_forward(n, e.cfg.obs_dim, self.size, N.tptr(e.flat), N.tptr(obs.contiguous()), N.tptr(v), N.tptr(logits), N.torch_stream_ptr()))
        return v, logits

    def rollout(self, e):  # (csrc/srlx_ppo_net.hip: k_ppo_rollout<CartPoleCategorical>)
        cfg, env = e.cfg, e.env
        args = (cfg.n_envs, cfg.horizon, cfg.n_actions, N.tptr(e.flat), N.tptr(env.state), N.tptr(env.t), N.tptr(env.episodes), N.tptr(env.obs), env.episode_len, env.seed,
                cfg.seed ^ 0x61637400, N.tptr(e.act_counter), cfg.discount, cfg.gae_discount, N.tptr(e.b_obs), N.tptr(e.b_act), N.tptr(e.b_logp), N.tptr(e.b_val), N.tptr(e.b_rew),
                N.tptr(e.b_done), N.tptr(e.b_adv), N.tptr(e._last_v), N.tptr(e.episode_return), N.tptr(e.finished_returns))
        if e.kl:
            N.check(e.lib.srlx_ppo_cat_rollout_kl(*args, N.tptr(e.old_dist[0]), None if e.env_opts is None else ctypes.byref(e.env_opts), N.torch_stream_ptr()))
        elif e.env_opts is None:
            N.check(e.lib.srlx_ppo_cat_rollout(*args, N.torch_stream_ptr()))
        else:
            N.check(e.lib.srlx_ppo_cat_rollout_ex(*args, ctypes.byref(e.env_opts), N.torch_stream_ptr()))

    def loss_and_seeds(self, e, obs, action, old_logp, adv, v_target, old_v, old_dist=None):
        v, logits = e.net(obs)
        if e.kl:  # the KL term needs every logit: the kernel takes the logits and returns their seeds
            if self.size not in self.fused_sizes:
                raise ValueError('surrogate_type "kl": srlx_ppo_loss_categorical_kl covers ' + self.envelope)
            g_logits, g_v = torch.empty_like(logits), torch.empty_like(v)
            e._keep_loss = (logits.detach().contiguous(), v.detach().contiguous(), action.reshape(-1).contiguous(), old_dist[0])
            N.check(e.lib.srlx_ppo_loss_categorical_kl(logits.shape[0], self.size, N.tptr(e._keep_loss[0]), N.tptr(e._keep_loss[2]), N.tptr(old_logp), N.tptr(old_dist[0]), N.tptr(adv),
                                                       N.tptr(e._keep_loss[1]), N.tptr(v_target), N.tptr(old_v), *_kl_loss_args(e.cfg), N.tptr(e.kl_beta), N.tptr(e.losses),
                                                       N.tptr(g_logits), N.tptr(g_v), N.torch_stream_ptr()))
            return (v, logits), (g_v, g_logits)
        lp = torch.log_softmax(logits, dim=-1).gather(1, action.long().view(-1, 1))  # CategoricalDist.log_prob of the taken action, [B][1]
        g_lp, g_v = torch.empty_like(lp), torch.empty_like(v)
        e._keep_loss = (lp.detach().contiguous(), v.detach().contiguous())
        N.check(e.lib.srlx_ppo_loss_logpi(lp.shape[0], 1, N.tptr(e._keep_loss[0]), N.tptr(old_logp), N.tptr(adv), N.tptr(e._keep_loss[1]), N.tptr(v_target), N.tptr(old_v),
                                          *_loss_args(e.cfg), N.tptr(e.losses), N.tptr(g_lp), N.tptr(g_v), N.torch_stream_ptr()))
        return (v, lp), (g_v, g_lp)

    def minibatch(self, e, mb, rows, buffers, outputs):
        if e.kl:
            partials, grad, losses, st = outputs
            N.check(e.lib.srlx_ppo_cat_minibatch_kl(mb, N.tptr(rows), e.cfg.obs_dim, self.size, *buffers, N.tptr(e.old_dist[0]), *_kl_loss_args(e.cfg), N.tptr(e.kl_beta), partials, grad,
                                                    losses, st))
            return
        N.check(e.lib.srlx_ppo_cat_minibatch(mb, N.tptr(rows), e.cfg.obs_dim, self.size, *buffers, *_loss_args(e.cfg), *outputs))


def head_of(cfg: PPODeviceConfig):  # the head (and with it the built-in environment) a configuration selects
    return CategoricalCartPoleHead if cfg.n_actions > 0 else NormalPendulumHead


def _plugin_linears(model):
    lin = lambda block: [m for m in block.modules() if isinstance(m, nn.Linear)]  # noqa: E731
    if any(True for _ in model.in_block.parameters()):
        raise ValueError("the plugin network has a trainable input block: the engine's network has none")
    heads = [model.policy_out] + ([model.log_scale_out] if model.continuous else [])
    return lin(model.hidden_block) + lin(model.value_block) + [model.value_out] + lin(model.policy_block) + heads


def _paired_linears(net: ActorCritic, parameter):
    mine, theirs = net.linears(), _plugin_linears(parameter.model)
    if len(mine) != len(theirs) or any(a.weight.shape != b.weight.shape for a, b in zip(mine, theirs)):
        raise ValueError("the plugin's network and the engine's differ in shape: %s vs %s" % ([tuple(m.weight.shape) for m in theirs], [tuple(m.weight.shape) for m in mine]))
    return list(zip(mine, theirs))


class PPOEngine:
    def __init__(self, cfg: PPODeviceConfig, device: int = 0, grad_sync: Optional[Callable[[nn.Module], None]] = None, fused: Optional[bool] = None,
                 flat_grad_sync: Optional[Callable[[torch.Tensor], float]] = None):
        """fused: the network in libsrlx (None: whenever the geometry is the reference's default blocks; True: required; False: torch modules + autograd, the test
        yardstick).  grad_sync(module): the torch path's gradient exchange; flat_grad_sync(flat_grad) -> scale: the fused path's (all-reduces the flat gradient in
        place, returns the factor the optimiser launch applies: 1 / world size)."""
        if not torch.cuda.is_available():
            raise RuntimeError("simple_distributed_rl_amd.device.ppo needs an MI355X: its rollout / GAE / loss arithmetic is libsrlx HIP code (no CPU fallback)")
        if cfg.surrogate_type not in ("clip", "", "kl"):
            raise ValueError('surrogate_type must be "clip", "" or "kl"')
        self.kl = cfg.surrogate_type == "kl"
        if self.kl and not cfg.adaptive_kl_target > 0:
            raise ValueError("adaptive_kl_target must be positive")
        if self.kl and (grad_sync is not None or flat_grad_sync is not None):
            raise ValueError('surrogate_type "kl" is not data-parallel: each rank would adapt its own beta from its local kl_mean (exchanging kl_mean is not built)')
        if cfg.baseline_type not in BASELINES:
            raise ValueError(f"baseline_type {cfg.baseline_type!r}: the engine serves {sorted(BASELINES)}")
        self.baseline = BASELINES[cfg.baseline_type]  # "advantage" (inside the loss), "none", or a batch statistic: "ave" / "std" / "normal"
        for name in ("reward_clip", "state_clip"):
            c = getattr(cfg, name)
            if c is not None and not (len(c) == 2 and float(c[0]) <= float(c[1])):
                raise ValueError(f"{name} is None or (lo, hi) with lo <= hi")
        self.rescale = (float(cfg.action_scale), float(cfg.action_offset)) != (1.0, 0.0)
        if self.rescale and head_of(cfg).cat:
            raise ValueError("action_scale / action_offset belong to the Normal head: a categorical action is an index")
        self.lr_sched = N.lr_schedule(cfg.lr_scheduler)  # (raises for an unknown type or a piecewise schedule beyond 8 boundaries)
        self.scheduled = self.lr_sched.kind != N.LR_CONSTANT
        if self.scheduled and not cfg.lr > 0:
            raise ValueError("a learning-rate schedule needs lr > 0")
        # srlx_ppo_env_opts_t for the one-launch rollout (None: the plain entry point); the step-wise path clips at the same float32 bounds
        self.reward_clip = None if cfg.reward_clip is None else (_f32(cfg.reward_clip[0]), _f32(cfg.reward_clip[1]))
        self.state_clip = None if cfg.state_clip is None else (_f32(cfg.state_clip[0]), _f32(cfg.state_clip[1]))
        self.action_map = (_f32(cfg.action_scale), _f32(cfg.action_offset))
        self.env_opts = None
        if self.reward_clip or self.state_clip or self.rescale:
            rc, sc = self.reward_clip or (0.0, 0.0), self.state_clip or (0.0, 0.0)
            self.env_opts = N.PPOEnvOpts(int(self.reward_clip is not None), rc[0], rc[1], int(self.state_clip is not None), sc[0], sc[1], *self.action_map)
        self.cfg, self.lib = cfg, N.lib()
        self.dev = torch.device(f"cuda:{device}")
        torch.manual_seed(cfg.seed)
        self.head = head = head_of(cfg)(cfg, self.lib)  # everything below that depends on the policy head goes through it
        self.cat = head.cat
        self.net = ActorCritic(cfg).to(self.dev)
        can_fuse = tuple(cfg.hidden_sizes) == (64, 64) and tuple(cfg.value_sizes) == (64,) and tuple(cfg.policy_sizes) == (64,) and 1 <= cfg.obs_dim <= 8 and head.size in head.fused_sizes
        if fused and not can_fuse:
            raise ValueError("PPOEngine(fused=True): the libsrlx network covers hidden (64, 64), value (64,), policy (64,), obs_dim <= 8, " + head.envelope)
        self.fused = can_fuse if fused is None else bool(fused)
        self.grad_sync, self.flat_grad_sync = grad_sync, flat_grad_sync
        if self.fused:
            # one flat parameter vector in `parameters()` order; the module's tensors become views of it (state_dict / export keep working, always current)
            P = head.param_count(cfg.obs_dim, head.size)
            ps = list(self.net.parameters())
            assert sum(p.numel() for p in ps) == P
            self.flat = torch.cat([p.detach().reshape(-1) for p in ps]).contiguous()
            off = 0
            for p in ps:
                p.data = self.flat[off : off + p.numel()].view_as(p)
                off += p.numel()
            self.flat_grad = torch.zeros(P, dtype=torch.float32, device=self.dev)
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
            self.opt_step = torch.zeros(2, dtype=torch.int64, device=self.dev)  # [steps taken, the optimiser launch's arrival counter]
            self.partials = torch.zeros((head.kl_partials_floats if self.kl else head.partials_floats)(cfg.obs_dim, head.size), dtype=torch.float32, device=self.dev)
            self.opt = None
        else:
            self.opt = torch.optim.Adam(self.net.parameters(), lr=cfg.lr, capturable=True)
            self.lr_sch = cfg.lr_scheduler.apply_torch_scheduler(self.opt)  # a LambdaLR over `factor`, as the plugin's trainer (None: constant)
        self.env = make_env(cfg, cfg.seed, self.dev)
        self.ls_range = (math.log(cfg.stable_gradients_scale_range[0]), math.log(cfg.stable_gradients_scale_range[1]))
        E, T, d = cfg.n_envs, cfg.horizon, self.dev
        f32 = dict(dtype=torch.float32, device=d)
        self.b_obs = torch.zeros((T + 1, E, cfg.obs_dim), **f32)
        self.b_act = torch.zeros((T, E) + head.act_shape, dtype=head.act_dtype, device=d)
        self.b_logp = torch.zeros((T, E) + head.act_shape, **f32)
        self.b_val = torch.zeros((T, E), **f32)
        self.b_rew = torch.zeros((T, E), **f32)
        self.b_done = torch.zeros((T, E), dtype=torch.uint8, device=d)
        self.b_adv = torch.zeros((T, E), **f32)
        self.b_adv_base = torch.zeros((T, E), **f32) if self.baseline in N.PPO_BASELINE_MODES else None  # what srlx_ppo_adv_baseline writes, minibatch by minibatch
        self.act_counter = torch.zeros(1, dtype=torch.int64, device=d)
        self.losses = torch.zeros(5 if self.kl else 3, **f32)  # policy, value, entropy [, kl_mean, beta as adapted]
        # "kl": the acting distribution of every step, and beta -- device state, adapted by the launch that forms the losses
        self.old_dist = tuple(torch.zeros((T, E) + shape, **f32) for shape in head.dist_shapes) if self.kl else None
        self.kl_beta = torch.full((1,), float(cfg.adaptive_kl_beta), **f32) if self.kl else None
        self.b_obs[0].copy_(self.env.obs)
        self.iterations = 0
        self._rollout_graph = None
        self._update_graph = None
        self._last_v = torch.zeros(E, **f32)
        self.episode_return = torch.zeros(E, **f32)
        self.finished_returns = torch.zeros(2, **f32)  # sum, count of finished episodes since the last read
        # One minibatch permutation per epoch from libsrlx's keyed permutation kernel (srlx_rng_permutation: device state only), INSIDE the captured
        # update.  What round 2 hid behind a hipStreamSynchronize per iteration (a bisect on ROCm 7.2 / torch 2.10, E = 4096; tools/README.md): with NO
        # eager launch between replays of the two large graphs (~700 / ~1000 nodes) -- fixed permutations, or this kernel -- 40 unsynchronised iterations
        # equal the synchronised run to 1e-7; with torch.randperm as a graph node (torch refreshes the generator's offset tensors with eager launches before
        # every replay) they turn non-finite, and with torch.randperm drawn eagerly between the replays they stay finite but train differently: eager
        # kernels enqueued behind a large graph launch do not reliably wait for the graph's tail (an event recorded there does not either:
        # event.synchronize() per iteration does not help, hipStreamSynchronize does).  A graph whose only node is randperm replays fine.
        # (The initial values below are overwritten before their first use; the draws keep torch's CUDA generator where every later draw expects it.)
        self._perms = torch.stack([torch.randperm(T * E, device=d) for _ in range(cfg.epochs)])
        self.perm_counter = torch.zeros(1, dtype=torch.int64, device=d)

    # --- rollout ---------------------------------------------------------------------------------------------------
    def act(self, obs: torch.Tensor, action_out: torch.Tensor, logp_out: torch.Tensor, deterministic: bool = False, dist_out=None):
        """dist_out ("kl"): tensors that receive the acting distribution -- (probs [n][n_actions],), or (loc, clamped log_scale) [n][A]"""
        v, *self._keep = self.forward(obs)  # (the head's outputs stay alive behind the launch)
        if dist_out is None:
            self.head.sample(self, *self._keep, action_out, logp_out, deterministic)
        else:
            self.head.sample(self, *self._keep, action_out, logp_out, deterministic, dist_out)
        return v

    def forward(self, obs: torch.Tensor):
        """(v [n], loc [n][A], log_scale [n][A]) of obs [n][obs_dim] -- categorical: (v [n], logits [n][n_actions]): the libsrlx network when fused, the torch modules
        otherwise."""
        if not self.fused:
            with torch.no_grad():
                return self.net(obs)
        return self.head.forward(self, obs)

    def _fused_rollout_ok(self) -> bool:
        cfg, head = self.cfg, self.head  # the head's built-in environment, 16 environments per workgroup, a horizon that fits its LDS (longer: the step-wise kernels)
        return (self.fused and isinstance(self.env, head.env_cls) and cfg.obs_dim == head.env_obs_dim and cfg.n_envs % 16 == 0
                and cfg.horizon <= head.rollout_max_horizon(head.size))

    def rollout(self):
        cfg = self.cfg
        if self._fused_rollout_ok():
            return self.head.rollout(self)
        # reward_clip / state_clip / the action rescale with torch ops around the step-wise kernels: the arithmetic of k_ppo_rollout's options (clamp = min(max(x, lo), hi)
        # in float32; the rescale a multiply, then an add)
        if self.state_clip:
            self.b_obs[0].clamp_(*self.state_clip)
        for t in range(cfg.horizon):
            self.b_val[t].copy_(self.act(self.b_obs[t], self.b_act[t], self.b_logp[t], dist_out=tuple(b[t] for b in self.old_dist) if self.kl else None))
            # the environment takes the first action dimension (a categorical head's only one; a copy only where action_dim > 1)
            env_action = self.b_act[t].reshape(cfg.n_envs, -1)[:, 0].contiguous()
            if self.rescale:
                env_action = (env_action * self.action_map[0] + self.action_map[1]).contiguous()
            self.env.step(env_action, self.b_obs[t + 1], self.b_rew[t], self.b_done[t])
            self.episode_return += self.b_rew[t]  # (the raw reward)
            d = self.b_done[t].bool()
            self.finished_returns[0] += (self.episode_return * d).sum()
            self.finished_returns[1] += d.sum()
            self.episode_return.masked_fill_(d, 0.0)
            if self.reward_clip:
                self.b_rew[t].clamp_(*self.reward_clip)
            if self.state_clip:
                self.b_obs[t + 1].clamp_(*self.state_clip)
        last_v = self.forward(self.b_obs[cfg.horizon])[0]
        # episode ends are never bootstrapped (ppo.py:396-397); a horizon cut inside an episode bootstraps from V(s_T)
        N.check(self.lib.srlx_gae_scan(cfg.n_envs, cfg.horizon, N.tptr(self.b_rew), N.tptr(self.b_val), N.tptr(self.b_done), N.tptr(last_v.contiguous()),
                                       cfg.discount, cfg.gae_discount, N.tptr(self.b_adv), N.torch_stream_ptr()))
        self._last_v = last_v

    # --- update ----------------------------------------------------------------------------------------------------
    def loss_and_seeds(self, obs, action, old_logp, adv, v_target, old_v, old_dist=None):
        """forward + the fused loss kernel; returns (v, loc, log_scale) with their gradient seeds -- categorical: (v, log-probability of the taken action); under "kl"
        (old_dist: the sampled rows of the acting distribution) the categorical pair is (v, logits), and the launch adapts `kl_beta`."""
        if self.kl:
            return self.head.loss_and_seeds(self, obs, action, old_logp, adv, v_target, old_v, old_dist)
        return self.head.loss_and_seeds(self, obs, action, old_logp, adv, v_target, old_v)

    def update(self):
        cfg = self.cfg
        T, E = cfg.horizon, cfg.n_envs
        n = T * E
        obs = self.b_obs[:T].reshape(n, cfg.obs_dim)
        act = self.b_act.reshape(n, -1)  # [n][action_dim]; categorical: [n][1]
        logp = self.b_logp.reshape(n, -1)
        adv = self.b_adv.reshape(n)
        val = self.b_val.reshape(n)
        v_target = adv if cfg.v_target == "gae" else adv + val
        mb = n // cfg.minibatches
        if self.fused:
            return self._update_fused(n, mb, obs, act, logp, adv, val, v_target)
        for ep in range(cfg.epochs):
            N.check(self.lib.srlx_rng_permutation(cfg.seed ^ 0x7065726D, N.tptr(self.perm_counter), n, N.tptr(self._perms[ep]), N.torch_stream_ptr()))
            perm = self._perms[ep]
            for k in range(cfg.minibatches):
                idx = perm[k * mb : (k + 1) * mb]
                old = tuple(b.reshape(n, -1)[idx].contiguous() for b in self.old_dist) if self.kl else None
                outs, seeds = self.loss_and_seeds(obs[idx], act[idx].contiguous(), logp[idx].contiguous(), self._batch_baseline(adv[idx]).contiguous(),
                                                  v_target[idx].contiguous(), val[idx].contiguous(), old)
                self.opt.zero_grad(set_to_none=False)
                torch.autograd.backward(outs, seeds)
                if self.grad_sync is not None:
                    self.grad_sync(self.net)
                if cfg.global_gradient_clip_norm != 0:
                    torch.nn.utils.clip_grad_norm_(self.net.parameters(), cfg.global_gradient_clip_norm)
                self.opt.step()
                if self.lr_sch is not None:
                    self.lr_sch.step()

    def _batch_baseline(self, a: torch.Tensor) -> torch.Tensor:
        """baseline_type "ave" / "std" / "normal" over one minibatch's advantages with torch ops (ppo.py:222-233: population deviation, + 1e-8) -- the yardstick of
        `srlx_ppo_adv_baseline`: float64 statistics, one rounding to float32.  Under `DistributedPPO` the statistics are per rank, over the LOCAL minibatch (only
        gradients are exchanged), on this path and on the fused one."""
        if self.baseline not in N.PPO_BASELINE_MODES:
            return a
        x = a.double()
        mean, sd = x.mean(), x.std(unbiased=False) + 1e-8
        return {"ave": x - mean, "std": x / sd, "normal": (x - mean) / sd}[self.baseline].float()

    def _update_fused(self, n, mb, obs, act, logp, adv, val, v_target):
        """epochs x minibatches of [k_ppo_adv_baseline ->] (k_ppo_minibatch + k_ppo_reduce) -> [all-reduce of the flat gradient] -> k_ppo_adam; the buffers are read in
        place through the permutation's rows.  baseline_type "ave" / "std" / "normal": one more launch per minibatch writes that minibatch's transformed advantages
        into `b_adv_base` at the same rows, and the minibatch launch reads them there (`v_target` keeps the untouched ones).  Under `DistributedPPO` the mean and
        deviation are per rank, over the local minibatch.  A schedule goes to the launch as data: it is evaluated there, from `opt_step[0]`."""
        cfg = self.cfg
        st = N.torch_stream_ptr()
        mode = N.PPO_BASELINE_MODES.get(self.baseline, 0)
        # the epochs' shuffles in one launch (the values `epochs` successive srlx_rng_permutation calls would write)
        N.check(self.lib.srlx_rng_permutations(cfg.seed ^ 0x7065726D, N.tptr(self.perm_counter), n, cfg.epochs, N.tptr(self._perms), st))
        for ep in range(cfg.epochs):
            for k in range(cfg.minibatches):
                rows = self._perms[ep][k * mb : (k + 1) * mb]
                if mode:
                    N.check(self.lib.srlx_ppo_adv_baseline(mb, N.tptr(rows), N.tptr(adv), mode, N.tptr(self.b_adv_base), st))
                self.head.minibatch(self, mb, rows, (N.tptr(self.flat), N.tptr(obs), N.tptr(act), N.tptr(logp), N.tptr(self.b_adv_base if mode else adv), N.tptr(v_target),
                                                     N.tptr(val)), (N.tptr(self.partials), N.tptr(self.flat_grad), N.tptr(self.losses), st))
                scale = self.flat_grad_sync(self.flat_grad) if self.flat_grad_sync is not None else 1.0
                state = (cfg.obs_dim, self.head.size, N.tptr(self.flat), N.tptr(self.flat_grad), N.tptr(self.exp_avg), N.tptr(self.exp_avg_sq), N.tptr(self.opt_step), cfg.lr)
                rest = (0.9, 0.999, 1e-8, cfg.global_gradient_clip_norm, scale, st)
                N.check(self.head.adam_sched(*state, ctypes.byref(self.lr_sched), *rest) if self.scheduled else self.head.adam(*state, *rest))

    def capture_graphs(self):
        """Captures the T-step rollout (+ GAE) and the whole update phase into two HIP graphs: an iteration becomes two
        graph launches instead of ~T*20 + epochs*minibatches*60 eager ones.  Call after a few eager iterations (Adam
        state and every scratch buffer must exist).  The fused update's graph follows `lr_scheduler` (the rate is computed in the launch); the torch path's Adam
        takes its rate from the host, so a schedule there cannot be captured."""
        if not self.fused and self.scheduled:
            raise ValueError("capture_graphs(): the torch path's learning-rate schedule is stepped on the host; the fused engine's is evaluated on the device")
        torch.cuda.synchronize(self.dev)
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):  # warm-up on a capture-style stream
            self.rollout()
            self.update()
            self.b_obs[0].copy_(self.b_obs[self.cfg.horizon])
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, capture_error_mode="thread_local"):
            self.rollout()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, capture_error_mode="thread_local"):
            self.update()
            self.b_obs[0].copy_(self.b_obs[self.cfg.horizon])
        self._rollout_graph, self._update_graph = g1, g2
        torch.cuda.synchronize(self.dev)

    def step(self):
        """one PPO iteration: T x E environment steps + epochs x minibatches updates"""
        if self._rollout_graph is not None:
            # two graph launches per iteration, nothing waits on the host and nothing is launched eagerly between them (see __init__)
            self._rollout_graph.replay()
            self._update_graph.replay()
        else:
            self.rollout()
            self.update()
            self.b_obs[0].copy_(self.b_obs[self.cfg.horizon])
        self.iterations += 1

    def pop_mean_episode_return(self) -> float:
        s, c = self.finished_returns.tolist()
        self.finished_returns.zero_()
        return s / c if c else float("nan")

    def info(self) -> dict:
        pl, vl, el, *kl = self.losses.tolist()
        out = dict(policy_loss=pl, value_loss=vl, entropy_loss=el)
        if self.kl:
            out["kl_mean"], out["kl_beta"] = kl[0], float(self.kl_beta.item())  # (the last minibatch's mean KL; beta as it stands)
        return out

    # --- weight exchange with the PPO plugin (algorithms/ppo.py:Parameter; its network's keys: hidden_block, value_block, value_out, policy_block, policy_out) ---
    def export_to(self, parameter) -> None:
        """Copies this engine's network into a plugin `ppo.Parameter` (same blocks, same head), e.g. to evaluate it with `Runner.evaluate()`."""
        with torch.no_grad():
            for a, b in _paired_linears(self.net, parameter):
                b.weight.copy_(a.weight)
                b.bias.copy_(a.bias)
        if getattr(self, "kl", False):
            parameter.adaptive_kl_beta = float(self.kl_beta.item())

    def load_from(self, parameter) -> None:
        """Copies a plugin `ppo.Parameter`'s network into this engine (the fused path's flat vector included: the module's tensors are views of it)."""
        with torch.no_grad():
            for a, b in _paired_linears(self.net, parameter):
                a.weight.copy_(b.weight)
                a.bias.copy_(b.bias)
        if getattr(self, "kl", False):
            self.kl_beta.fill_(float(parameter.adaptive_kl_beta))


def flat_grad_all_reduce(net: nn.Module, group=None):
    """Average the gradients of every rank: ONE all-reduce of a flat buffer (about 40 KB for the config-5 network)."""
    import torch.distributed as dist

    grads = [p.grad for p in net.parameters() if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    staged = dist.get_backend(group) == "gloo" and flat.is_cuda  # test rigs: ranks sharing one GPU
    buf = flat.cpu() if staged else flat
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    buf = buf.to(flat.device) / dist.get_world_size(group)
    off = 0
    for g in grads:
        g.copy_(buf[off : off + g.numel()].view_as(g))
        off += g.numel()


def flat_vector_all_reduce(flat: torch.Tensor, group=None) -> float:
    """The fused network's exchange: ONE in-place all-reduce (sum) of the flat gradient vector; returns 1 / world size, which the clip + Adam launch applies.  With
    RCCL the collective is captured into the update graph like any other node; gloo (test rigs: ranks sharing one GPU) stages through the host and runs eagerly."""
    import torch.distributed as dist

    if dist.get_backend(group) == "gloo" and flat.is_cuda:
        h = flat.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        flat.copy_(h)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    return 1.0 / dist.get_world_size(group)


class DistributedPPO:
    """Data-parallel PPO (BASELINE config 5): identical networks, disjoint environments, averaged gradients.  Only gradients are exchanged: the batch baselines
    ("ave" / "std" / "normal") take their mean and deviation per rank, over the local minibatch; the learning-rate schedule follows each rank's own step count,
    which is the same on every rank."""

    def __init__(self, cfg: PPODeviceConfig, device: int, fused: Optional[bool] = None):
        import dataclasses

        import torch.distributed as dist

        if cfg.surrogate_type == "kl":
            raise ValueError('DistributedPPO: surrogate_type "kl" is not data-parallel -- each rank would adapt its own beta from its local kl_mean (exchanging kl_mean is not built)')
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        local = dataclasses.replace(cfg, seed=cfg.seed)  # same seed -> same initial network on every rank
        self.engine = PPOEngine(local, device, grad_sync=flat_grad_all_reduce, flat_grad_sync=flat_vector_all_reduce, fused=fused)
        # decorrelate environments and sampling noise across ranks
        self.engine.env = make_env(cfg, cfg.seed + 7919 * (self.rank + 1), self.engine.dev)
        self.engine.b_obs[0].copy_(self.engine.env.obs)
        self.engine.act_counter.fill_(self.rank << 40)
        tensors = [self.engine.flat] if self.engine.fused else [p.data for p in self.engine.net.parameters()]
        for t in tensors:  # belt and braces: one broadcast of the initial parameters
            if dist.get_backend() == "gloo" and t.is_cuda:
                h = t.cpu()
                dist.broadcast(h, src=0)
                t.copy_(h)
            else:
                dist.broadcast(t, src=0)

    def capture_graphs(self):
        """The rollout and the update as HIP graphs; with the fused network over RCCL the update's graph holds its 16 all-reduces of the flat gradient (every rank
        replays the same graph, so the collectives stay matched).  Other set-ups keep the update eager (a host-staged gloo all-reduce cannot be captured)."""
        import torch.distributed as dist

        if self.engine.fused and dist.get_backend() == "nccl":
            self.engine.capture_graphs()

    def step(self):
        self.engine.step()
