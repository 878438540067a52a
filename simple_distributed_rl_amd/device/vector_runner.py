"""The device drivers of the sequence loop: `Runner.train()` on the hand-written engine.

`srl.Runner(env, rainbow.Config(...)).train(...)` in the reference plays ONE environment through a Python loop
(srl/runner/runner.py:95-183 -> srl/base/run/core_play.py:115-214).  When the algorithm is the Rainbow family on a
GPU device and the environment produces image frames, the same call here hands the loop
(`base/run/sequence.py`) two drivers that own a `RainbowEngine`:

    VectorActor    `lanes` = E environments per iteration: uint8 frame ring -> matrix-core Q-network ->
                   epsilon-greedy -> environments -> ring commit + PER add, all enqueued, nothing read back
    VectorLearner  the updates the loop owes (`train_interval` / `train_repeat`), enqueued on the engine's learner
                   stream so that they run beside the NEXT lock-step's network pass

so `RunCallback` hooks, stop rules (`max_steps`, `max_train_count`, `max_memory`, `max_episodes`, `timeout`) and
the `RunState` counters behave as in the reference's loop, with `state.total_step` advancing by E per iteration.
Episode results stay on the device (`EpisodeLedger`, libsrlx `srlx_episode_account`): the host learns about them
through a pinned mailbox without synchronising the stream, and reads individual episodes only when somebody asks
(an `on_episode_end` hook, `max_episodes`, the end of the run).

Environments: a class registered under an environment id may offer `device_vector(replay, **kwargs)` returning a
device-resident batch environment (the built-in "SyntheticAtari-v0" does); every other image environment is
stepped on the host in E copies and its frames uploaded each lock-step (`HostVecEnv`).
"""
import ctypes
from typing import List, Optional, Tuple

import numpy as np
import torch

from simple_distributed_rl_amd import _native as N
from simple_distributed_rl_amd.base.define import SpaceTypes
from simple_distributed_rl_amd.base.run.sequence import ActorDriver, LearnerDriver
from simple_distributed_rl_amd.device.lane_engine import MAX_LANES


# ---------------------------------------------------------------------------------------------
# episode results without leaving HBM
# ---------------------------------------------------------------------------------------------
class EpisodeLedger:
    """Running return/length per environment + a ring of finished episodes + running totals, all in HBM
    (env_run.py:334-352 and core_play.py:200-214 for E environments)."""

    SLOTS = 4

    def __init__(self, n_envs: int, device: torch.device, ring_cap: int = 1 << 16):
        self.E, self.dev, self.cap = int(n_envs), device, int(ring_cap)
        self.lib = N.lib()
        self.ep_return = torch.zeros(self.E, dtype=torch.float32, device=device)
        self.ep_len = torch.zeros(self.E, dtype=torch.int32, device=device)
        self.ring = torch.zeros((self.cap, 2), dtype=torch.float32, device=device)
        self.totals = torch.zeros(4, dtype=torch.int64, device=device)  # episodes, steps, float64 bits of return sum, length sum
        self._mail = torch.zeros((self.SLOTS, 4), dtype=torch.int64).pin_memory()
        self._posted = [torch.cuda.Event() for _ in range(self.SLOTS)]
        self._n_posts = 0
        self._last = (0, 0, 0.0, 0)
        self.read_upto = 0  # episodes already handed to the host

    def clear(self):
        """A new run: counters and the finished-episode ring start over (the lanes' running episodes continue)."""
        torch.cuda.current_stream(self.dev).synchronize()
        self.totals.zero_()
        self._n_posts, self._last, self.read_upto = 0, (0, 0, 0.0, 0), 0

    def account(self, rewards: torch.Tensor, done: torch.Tensor, skip_ptr=None):
        N.check(self.lib.srlx_episode_account(self.E, N.tptr(rewards), N.tptr(done), skip_ptr, N.tptr(self.ep_return), N.tptr(self.ep_len),
                                              N.tptr(self.ring), self.cap, N.tptr(self.totals), N.torch_stream_ptr()))

    def post(self):
        """Enqueue a copy of the totals into the next mailbox slot (no synchronisation)."""
        k = self._n_posts % self.SLOTS
        self._mail[k].copy_(self.totals, non_blocking=True)
        self._posted[k].record()
        self._n_posts += 1

    @staticmethod
    def _decode(row) -> Tuple[int, int, float, int]:
        return int(row[0]), int(row[1]), float(row[2:3].view(torch.float64)[0]), int(row[3])

    def peek(self, wait: bool = False) -> Tuple[int, int, float, int]:
        """(episodes, env steps, return sum, length sum) of the newest mailbox slot whose copy has landed; `wait`
        blocks for the newest post.  A slot whose event has completed has no later write in flight (a later post into the
        same slot re-records its event), so its four values are consistent."""
        for back in range(min(self.SLOTS, self._n_posts)):
            k = (self._n_posts - 1 - back) % self.SLOTS
            if wait and back == 0:
                self._posted[k].synchronize()
            if self._posted[k].query():
                self._last = self._decode(self._mail[k])
                break
        return self._last

    def drain(self) -> List[Tuple[float, int]]:
        """Synchronises and returns the (return, length) records of the episodes that finished since the last drain
        (at most the ring's capacity: older ones were overwritten)."""
        self.post()
        episodes = self.peek(wait=True)[0]
        first = max(self.read_upto, episodes - self.cap)
        out: List[Tuple[float, int]] = []
        if episodes > first:
            idx = torch.arange(first, episodes, device=self.dev) % self.cap
            rows = self.ring[idx].cpu().numpy()
            out = [(float(r), int(l)) for r, l in rows]
        self.read_upto = episodes
        return out


# ---------------------------------------------------------------------------------------------
# environments
# ---------------------------------------------------------------------------------------------
class HostVecEnv:
    """E host copies of an image environment behind the engine's batch-environment contract (`reset()` ->
    uint8 [E, F] first frames; `step(actions)` -> next_obs / rewards / terminated / done device tensors).  A lane whose
    episode ended gets its environment reset on the NEXT lock-step, which then only delivers the new episode's first frame
    (the store's `needs_reset` protocol, srlx_store_commit_step)."""

    capturable = False  # step() synchronises with the host

    def __init__(self, env_config, n_envs: int, device: torch.device, seed: Optional[int] = None, processor=None, float_obs: bool = False):
        """processor: an ImageProcessor whose space has been remapped from this environment's (raw uint8 frames, e.g. ALE's 210 x 160 x 3):
        the raw frames are uploaded as they are and ONE srlx_image_preprocess launch per lock-step turns them into the ring's gray frames
        -- the reference runs OpenCV per frame on the host and hands the network float32 (image_processor.py:104-151).
        float_obs: the observations go to a float32 ring as they are (a flat BoxSpace((D,)) environment: no /255 scaling, no processor)."""
        from simple_distributed_rl_amd.base.env.registration import make as make_env_run

        self.envs = [make_env_run(env_config) for _ in range(n_envs)]
        self.E, self.dev = n_envs, device
        self.seed = seed
        self.processor = processor
        self.float_obs = bool(float_obs)
        assert not (self.float_obs and processor is not None)
        sp = self.envs[0].observation_space
        if processor is not None:
            self._raw_shape = tuple(sp.shape)
            self._host_raw = torch.zeros((n_envs,) + self._raw_shape, dtype=torch.uint8).pin_memory()
            self.F = int(processor._out_hw[0] * processor._out_hw[1])
        else:
            self.F = int(np.prod(sp.shape)) if hasattr(sp, "shape") else int(sp.size)  # (an ArrayDiscreteSpace, Grid's, has a size and no shape)
        self._scale = 255.0 if float(np.max(sp.high)) <= 1.0 else 1.0  # "0to1" frames (image_processor.py:140-142) back to bytes
        obs_dtype = torch.float32 if self.float_obs else torch.uint8
        self._host_obs = torch.zeros((n_envs, self.F), dtype=obs_dtype).pin_memory()
        self._host_scal = torch.zeros((n_envs, 3), dtype=torch.float32).pin_memory()
        self.next_obs = torch.zeros((n_envs, self.F), dtype=obs_dtype, device=device)
        self.rewards = torch.zeros(n_envs, dtype=torch.float32, device=device)
        self.terminated = torch.zeros(n_envs, dtype=torch.uint8, device=device)
        self.done = torch.zeros(n_envs, dtype=torch.uint8, device=device)
        self._needs_reset = [False] * n_envs
        self._episodes = 0

    def _bytes(self, frame) -> np.ndarray:
        if self.float_obs:
            return np.asarray(frame, np.float32).reshape(-1)
        return np.rint(np.asarray(frame, np.float32).reshape(-1) * self._scale).astype(np.uint8)

    def _take(self, i: int):
        """Lane i's current frame into the staging row: raw bytes when a device processor follows, ring bytes otherwise."""
        if self.processor is not None:
            self._host_raw[i] = torch.from_numpy(np.ascontiguousarray(self.envs[i].state, dtype=np.uint8).reshape(self._raw_shape))
        else:
            self._host_obs.numpy()[i] = self._bytes(self.envs[i].state)

    def _upload(self, dst: torch.Tensor) -> torch.Tensor:
        if self.processor is not None:
            raw = self._host_raw.to(self.dev, non_blocking=True)
            self.processor.preprocess_batch(raw, out_u8=dst.view((self.E,) + tuple(self.processor._out_hw)))
            self._raw_keep = raw  # alive until the kernel has read it
        else:
            dst.copy_(self._host_obs, non_blocking=True)
        return dst

    def _reset_lane(self, i: int):
        seed = None if self.seed is None else self.seed + self._episodes
        self._episodes += 1
        self.envs[i].reset(seed=seed)
        self._take(i)

    def setup(self, context):
        for e in self.envs:
            e.setup(context)

    def teardown(self):
        for e in self.envs:
            e.teardown()

    def reset(self) -> torch.Tensor:
        for i in range(self.E):
            self._reset_lane(i)
        first = self._upload(torch.zeros((self.E, self.F), dtype=self.next_obs.dtype, device=self.dev))
        torch.cuda.current_stream(self.dev).synchronize()
        return first

    def _lane_action(self, acts: np.ndarray, i: int):
        """Lane i's action as its environment takes it (a subclass with float actions hands over the row)."""
        return int(acts[i])

    def step(self, actions: torch.Tensor):
        from simple_distributed_rl_amd.base.define import DoneTypes

        acts = actions.cpu().numpy()  # also orders this call after the previous lock-step's uploads
        scal = self._host_scal.numpy()
        for i, env in enumerate(self.envs):
            if self._needs_reset[i]:
                self._reset_lane(i)
                scal[i] = 0.0
                self._needs_reset[i] = False
                continue
            env.step(self._lane_action(acts, i))
            self._take(i)
            scal[i, 0] = env.reward
            scal[i, 1] = 1.0 if env.done_type == DoneTypes.TERMINATED else 0.0
            scal[i, 2] = 1.0 if env.done else 0.0
            self._needs_reset[i] = env.done
        self._upload(self.next_obs)
        dev_scal = self._host_scal.to(self.dev, non_blocking=True)
        self.rewards.copy_(dev_scal[:, 0])
        self.terminated.copy_(dev_scal[:, 1].to(torch.uint8))
        self.done.copy_(dev_scal[:, 2].to(torch.uint8))
        return self.next_obs, self.rewards, self.terminated, self.done


class FloatActionHostVecEnv(HostVecEnv):
    """`HostVecEnv` for environments with a continuous action: `step` takes float32 actions [E][K] and hands lane i its row (the V-PPO engine's Normal head,
    DESIGN.md 7q)."""

    def _lane_action(self, acts: np.ndarray, i: int):
        return np.asarray(acts[i], np.float32).reshape(-1)


# ---------------------------------------------------------------------------------------------
# eligibility + configuration
# ---------------------------------------------------------------------------------------------
def _image_hw(space) -> Optional[Tuple[int, int]]:
    stype = getattr(space, "stype", None)
    shape = tuple(getattr(space, "shape", ()))
    if stype == SpaceTypes.GRAY_HW and len(shape) == 2:
        return shape
    if stype == SpaceTypes.GRAY_HW1 and len(shape) == 3 and shape[2] == 1:
        return shape[:2]
    return None


def why_not_vector(context, env, rl_config) -> str:
    """Empty string when `Runner.train()` can run on the device engine; otherwise the reason it stays on the plugin path."""
    if not str(context.used_device_torch).startswith("cuda"):
        return "the run is not on a GPU device"
    kind = engine_kind(rl_config)
    if kind is None:
        return f"no device engine for algorithm '{rl_config.get_name()}'"
    if kind == "agent57":  # the LSTM engine has its own envelope (device/agent57.py)
        return why_not_agent57_engine(env, rl_config)
    if kind == "c51":  # the categorical head of the MLP Q-network (device/mlpq.py)
        return why_not_c51_engine(env, rl_config)
    if env.player_num != 1:
        return "multi-player environment"
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    if not isinstance(env.action_space, DiscreteSpace) or env.action_space.n > 32:
        return "the engine serves discrete action spaces of at most 32 actions"
    if getattr(rl_config, "_obs_processors", None) and frame_processor(rl_config) is None:
        return "observation processors other than one ImageProcessor over uint8 frames are served by the plugin path"
    hw = _image_hw(frame_space(env, rl_config))
    if kind == "dqn" and hw is None:  # flat observations: the MLP Q-network (device/mlpq.py, srlx_mlpq.hip)
        return _why_not_flat_dqn(env, rl_config)
    if hw is None or hw[0] < 8 or hw[1] < 8:
        return "observations are not single-channel image frames (after the config's ImageProcessor, if any)"
    why = _why_not_memory(rl_config)
    if why:
        return why
    if kind == "agent57_light":  # torch networks: any DQN-image / dueling shape the plugin builds
        if getattr(rl_config.input_block, "image", None) is None or rl_config.input_block.image.name != "DQN":
            return "input block is not the DQN image block"
        return ""
    if rl_config.window_length != 4:
        return "the matrix-core network reads a window of 4 frames"
    ib = getattr(rl_config.input_block, "image", None)
    if ib is None or ib.name != "DQN" or ib.kwargs.get("filters", 32) != 32 or str(ib.kwargs.get("activation", "relu")).lower() != "relu":
        return "input block is not the DQN image block (32 filters, ReLU)"
    hb = rl_config.hidden_block
    sizes = tuple(hb.kwargs.get("layer_sizes", ()))
    if kind == "dqn":  # dqn/model_torch.py:17-29: MLP hidden block + out_layer -- the plain Q head (srlx.h: dueling_type 3)
        if hb.name != "MLP" or len(sizes) != 1:
            return "hidden block is not one MLP layer (the plain Q head covers in_block -> one dense layer -> out_layer)"
        if str(hb.kwargs.get("activation", "relu")).lower() != "relu":
            return "the plain Q head's dense layer is ReLU"
        if sizes[0] % 64 != 0 or sizes[0] > 1024:
            return "the plain Q head covers a dense layer of a multiple of 64 (<= 1024) units"
        if rl_config.batch_size > 64:
            return "the hand-written gradient step covers batches of at most 64"
        return ""
    if hb.name != "DuelingNetwork" or len(sizes) != 1 or sizes[0] % 32 != 0 or sizes[0] > 512:
        return "hidden block is not one dueling layer of a multiple of 32 (<= 512) units"
    if hb.kwargs.get("dueling_kwargs", {}).get("dueling_type", "average") not in ("average", ""):
        return "the hand-written gradient step covers the dueling types 'average' and ''"
    if rl_config.batch_size > 64:
        return "the hand-written gradient step covers batches of at most 64"
    return ""


def _why_not_memory(rl_config) -> str:
    mem = rl_config.memory
    if mem.name not in ("Proportional", "Proportional_cpp", "ReplayBuffer"):
        return f"no device replay for memory '{mem.name}'"
    if mem.enable_demo_memory:
        return "demo memory is served by the plugin memory"
    return ""


def flat_dim(space) -> Optional[int]:
    """D for a flat BoxSpace((D,)) observation, None otherwise."""
    from simple_distributed_rl_amd.base.spaces.box import BoxSpace

    if type(space) is not BoxSpace or len(tuple(space.shape)) != 1 or _image_hw(space) is not None:
        return None
    return int(space.shape[0])


def mlp_layer_sizes(rl_config):
    """(input value block layers, hidden block layers) of a DQN config, or None when either block is not an MLP of ReLU layers."""
    iv, hb = rl_config.input_block.value, rl_config.hidden_block
    if iv.name != "MLP" or hb.name != "MLP":
        return None
    if any(str(b.kwargs.get("activation", "relu")).lower() != "relu" for b in (iv, hb)):
        return None
    return tuple(int(x) for x in iv.kwargs.get("layer_sizes", ())), tuple(int(x) for x in hb.kwargs.get("layer_sizes", ()))


# the block kwargs the MLP Q-network's module tree does not depend on (rl/torch_/networks.py: InputValueBlock, MLPBlock); use_bias / input_flatten only at
# their defaults -- without biases, or without the Flatten module, the reference's keys differ from EngineMLPQNet's
_MLP_FREE_KWARGS = ("layer_sizes", "activation", "kernel_initializer", "bias_initializer")
_MLP_DEFAULT_KWARGS = dict(use_bias=True, input_flatten=True)


def _mlp_kwargs_reason(rl_config) -> str:
    for b in (rl_config.input_block.value, rl_config.hidden_block):
        for k, v in b.kwargs.items():
            if k in _MLP_FREE_KWARGS or (k in _MLP_DEFAULT_KWARGS and v == _MLP_DEFAULT_KWARGS[k]):
                continue
            return f"the MLP Q-network covers Linear layers with biases after a Flatten; block option {k}={v!r} stays on the plugin path"
    return ""


def is_flat_dqn(env, rl_config) -> bool:
    """Does this (environment, config) pair belong to the MLP Q-network engine (VectorQEngine) rather than the image engine?"""
    return engine_kind(rl_config) == "dqn" and _image_hw(frame_space(env, rl_config)) is None


def _why_not_flat_dqn(env, rl_config) -> str:
    """dqn.Config on flat observations: the shapes srlx_mlpq covers (srlx.h)."""
    space = frame_space(env, rl_config)
    D = flat_dim(space)
    if D is None:  # (neither image frames nor a flat vector: the reason every engine gave before flat observations were served)
        return "observations are not single-channel image frames (after the config's ImageProcessor, if any)"
    if getattr(rl_config, "_obs_processors", None):
        return "observation processors on flat observations are served by the plugin path"
    if D > 256:
        return "the MLP Q-network reads at most 256 observation elements"
    if rl_config.window_length != 1:
        return "the MLP Q-network reads one observation (window_length 1)"
    if env.action_space.n < 2:
        return "the MLP Q-network serves at least 2 actions"
    sizes = mlp_layer_sizes(rl_config)
    if sizes is None:
        return "the MLP Q-network's input value block and hidden block are MLPs of ReLU layers"
    why = _mlp_kwargs_reason(rl_config)
    if why:
        return why
    layers = sizes[0] + sizes[1]
    if not 1 <= len(layers) <= 3:
        return "the MLP Q-network covers 1 to 3 dense layers (input value block plus hidden block)"
    if any(w % 32 != 0 or not 32 <= w <= 512 for w in layers):
        return "the MLP Q-network covers dense layers of 32..512 units in multiples of 32"
    if rl_config.batch_size > 256:
        return "the MLP Q-network's gradient step covers batches of at most 256"
    return _why_not_memory(rl_config)


def dueling_layer_sizes(rl_config):
    """(input value block layers, the hidden block's layer_sizes[:-1], dueling units, dueling_type) of a rainbow.Config whose hidden block is a DuelingNetwork
    of ReLU layers behind an MLP input value block, or None."""
    iv, hb = rl_config.input_block.value, rl_config.hidden_block
    if iv.name != "MLP" or hb.name != "DuelingNetwork":
        return None
    acts = [iv.kwargs.get("activation", "relu"), hb.kwargs.get("mlp_kwargs", {}).get("activation", "relu"),
            hb.kwargs.get("dueling_kwargs", {}).get("activation", "relu")]
    sizes = tuple(int(x) for x in hb.kwargs.get("layer_sizes", ()))
    if any(str(a).lower() != "relu" for a in acts) or not sizes:
        return None
    return (tuple(int(x) for x in iv.kwargs.get("layer_sizes", ())), sizes[:-1], sizes[-1],
            str(hb.kwargs.get("dueling_kwargs", {}).get("dueling_type", "average")))


def why_not_flat_rainbow(env, rl_config, admit_noisy: bool = False) -> str:
    """rainbow.Config on flat observations: the shapes srlx_mlpq_create_dueling / srlx_mlpq_train_nstep cover (srlx.h).  Empty string: VectorQEngine can run it
    (`mlp_config_from`).  `Runner.train()` does not ask yet: `why_not_vector` keeps Rainbow on flat observations on the plugin path.

    `admit_noisy=True` puts `enable_noisy_dense` inside the envelope (srlx_mlpq_bind_noisy serves it); the default keeps the answer callers have had so far.
    The change that routes `Runner.train()` here drops the keyword and admits noisy configs always."""
    space = frame_space(env, rl_config)
    D = flat_dim(space)
    if D is None:
        return "observations are not single-channel image frames (after the config's ImageProcessor, if any)"
    if getattr(rl_config, "_obs_processors", None):
        return "observation processors on flat observations are served by the plugin path"
    if D > 256:
        return "the MLP Q-network reads at most 256 observation elements"
    if rl_config.window_length != 1:
        return "the MLP Q-network reads one observation (window_length 1)"
    if not 2 <= env.action_space.n <= 32:
        return "the MLP Q-network serves 2 to 32 actions"
    if rl_config.enable_noisy_dense and not admit_noisy:
        return "the MLP Q-network has no noisy dense layers"
    if rl_config.hidden_block.name == "MLP":
        return "the MLP Q-network's Rainbow form ends in a dueling head; an MLP hidden block stays on the plugin path"
    sizes = dueling_layer_sizes(rl_config)
    if sizes is None:
        return "the MLP Q-network's input value block is an MLP and its hidden block a DuelingNetwork, all of ReLU layers"
    ins, hid, units, dtype = sizes
    if dtype not in ("average", ""):
        return "the dueling head covers the dueling types 'average' and ''"
    hb = rl_config.hidden_block
    for k, v in list(rl_config.input_block.value.kwargs.items()) + list(hb.kwargs.get("mlp_kwargs", {}).items()):
        if k in _MLP_FREE_KWARGS or (k in _MLP_DEFAULT_KWARGS and v == _MLP_DEFAULT_KWARGS[k]):
            continue
        return f"the MLP Q-network covers Linear layers with biases after a Flatten; block option {k}={v!r} stays on the plugin path"
    if len(ins + hid) > 2:
        return "the dueling MLP Q-network covers at most 2 dense layers in front of the head (input value block plus the hidden block's layer_sizes[:-1])"
    if any(w % 32 != 0 or not 32 <= w <= 512 for w in ins + hid + (units,)):
        return "the MLP Q-network covers dense layers of 32..512 units in multiples of 32"
    if rl_config.multisteps > 7:
        return "the MLP Q-network's gradient step covers multisteps of at most 7"
    if rl_config.batch_size > 256:
        return "the MLP Q-network's gradient step covers batches of at most 256"
    return _why_not_memory(rl_config)


def auto_lanes_reason(env, rl_config, n_envs) -> str:
    """Flat-observation DQN, C51 and Agent57 engage the device engine only for an explicit set_vector_envs(n): "AUTO" keeps today's plugin path."""
    if engine_kind(rl_config) == "agent57" and isinstance(n_envs, str):
        return "Agent57 stays on the plugin path under set_vector_envs(\"AUTO\"); set_vector_envs(n) with n > 0 engages the device engine"
    if engine_kind(rl_config) == "c51" and isinstance(n_envs, str):
        return "C51 stays on the plugin path under set_vector_envs(\"AUTO\"); set_vector_envs(n) with n > 0 engages the device engine"
    if is_flat_dqn(env, rl_config) and isinstance(n_envs, str):
        return "flat-observation DQN stays on the plugin path under set_vector_envs(\"AUTO\"); set_vector_envs(n) with n > 0 engages the device engine"
    return ""


def mlp_config_from(rl_config, env, n_envs: int, seed: int):
    """dqn.Config (srl/algorithms/dqn/dqn.py:50-101) or rainbow.Config (srl/algorithms/rainbow/rainbow.py:57-107) on a flat observation -> VectorQConfig
    (device/mlpq.py)."""
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    mem = rl_config.memory
    prop = mem.name != "ReplayBuffer"
    kw = mem.kwargs if prop else {}
    head = {}
    if engine_kind(rl_config) == "rainbow":
        ins, hid, units, dtype = dueling_layer_sizes(rl_config)
        head = dict(dueling_units=units, dueling_type=dtype, multisteps=int(rl_config.multisteps), retrace_h=float(rl_config.retrace_h),
                    enable_noisy_dense=bool(rl_config.enable_noisy_dense))
    else:
        ins, hid = mlp_layer_sizes(rl_config)
    return VectorQConfig(
        batch_size=rl_config.batch_size, epsilon=rl_config.epsilon, test_epsilon=rl_config.test_epsilon, lr=rl_config.lr, discount=rl_config.discount,
        target_model_update_interval=rl_config.target_model_update_interval, enable_reward_clip=rl_config.enable_reward_clip,
        enable_double_dqn=rl_config.enable_double_dqn, enable_rescale=rl_config.enable_rescale,
        memory_capacity=mem.capacity, memory_warmup_size=mem.warmup_size,
        memory_has_duplicate=bool(kw.get("has_duplicate", True)) if prop else False,
        memory_alpha=float(kw.get("alpha", 0.0)), memory_beta_initial=float(kw.get("beta_initial", 0.4)),
        memory_beta_steps=int(kw.get("beta_steps", 1_000_000)), memory_epsilon=float(kw.get("epsilon", 1e-4)),
        obs_dim=flat_dim(frame_space(env, rl_config)), in_sizes=ins, hidden_sizes=hid, n_actions=env.action_space.n, n_envs=n_envs, seed=seed, **head,
    )


# ---- ppo.Config -> PPOEngine (device/ppo.py) -----------------------------------------------------------------------------------------------------------------------
# Every field of ppo.Config (the RLConfig base included) stands in exactly one of three tuples (tests/test_ppo_config_cpu.py walks dataclasses.fields):
# what `ppo_config_from` carries over;
PPO_MAPPED_FIELDS = ("hidden_block", "value_block", "policy_block", "discount", "gae_discount", "baseline_type", "surrogate_type", "policy_clip_range", "enable_value_clip",
                     "value_clip_range", "lr", "lr_scheduler", "value_loss_weight", "entropy_weight", "global_gradient_clip_norm", "state_clip", "reward_clip",
                     "stable_gradients_scale_range")
# the plugin's collect-then-train schedule -- fill a buffer of memory.warmup_size steps from ONE environment, then `train_num` calls that take one step (or
# `train_num` with train_every_epoch) on `batch_size` samples of it.  The engine's schedule is another one: `horizon` steps of `n_envs` environments, then
# `epochs` passes over `minibatches` shuffled minibatches -- its operating point, explicit arguments of `ppo_config_from` (as Rainbow's `train_interval` is the
# loop's argument and the engines' operating point is one update per lock-step: INTEGRATION.md);
PPO_OPERATING_POINT_FIELDS = ("batch_size", "memory", "train_num", "train_every_epoch")
# and what `why_not_ppo_engine` refuses off the one value the engine serves (adaptive_kl_target is read only by the "kl" surrogate, which surrogate_type refuses;
# enable_rl_processors / enable_state_encode act through the processors they switch).
PPO_REFUSED_FIELDS = ("observation_mode", "frameskip", "processors", "enable_rl_processors", "enable_state_encode", "enable_action_decode", "window_length", "reward_scale",
                      "reward_shift", "enable_sanitize", "enable_assertion", "dtype", "input_block", "experience_collection_method", "adaptive_kl_target",
                      "enable_state_normalized", "enable_stable_gradients")


def _ppo_block_sizes(block) -> Optional[Tuple[int, ...]]:
    """layer_sizes of a block the engine's `ActorCritic` builds (Linear + ReLU per layer), None for anything else."""
    if getattr(block, "name", None) != "MLP" or str(block.kwargs.get("activation", "relu")).lower() != "relu":
        return None
    if any(not (k in _MLP_FREE_KWARGS or (k in _MLP_DEFAULT_KWARGS and v == _MLP_DEFAULT_KWARGS[k])) for k, v in block.kwargs.items()):
        return None
    return tuple(int(x) for x in block.kwargs.get("layer_sizes", ()))


def _ppo_action_map(env) -> Optional[Tuple[float, float]]:
    """(scale, offset) of `action_space.rescale_from`: [-1, 1] onto the bounds, when every action dimension has the same finite bounds."""
    sp = env.action_space
    lo, hi = np.asarray(sp.low, np.float64).reshape(-1), np.asarray(sp.high, np.float64).reshape(-1)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo == lo[0]) and np.all(hi == hi[0])):
        return None
    return float((hi[0] - lo[0]) / 2.0), float((hi[0] + lo[0]) / 2.0)


def why_not_ppo_engine(env, rl_config, admit_kl: bool = False) -> str:
    """Empty string when `PPOEngine` (device/ppo.py) can run this ppo.Config on this environment as it is configured -- `ppo_config_from` maps it; otherwise EVERY
    reason it cannot, joined with "; ".  `Runner.train()` does not ask: PPO stays on the plugin path (`engine_kind`, `why_not_vector` are as they were).
    `admit_kl=True` puts `surrogate_type="kl"` (with `adaptive_kl_target`) inside the envelope -- the engine serves it (srlx_ppo_*_minibatch_kl); the default keeps the
    answer, and the three field tuples the reading, callers have had so far.  The keyword disappears when the route flips."""
    from simple_distributed_rl_amd.device.ppo import BASELINES
    from simple_distributed_rl_amd.envs.cartpole import CartPole
    from simple_distributed_rl_amd.envs.pendulum import Pendulum

    c, why = rl_config, []
    if c.get_name() != "PPO":
        return f"'{c.get_name()}' is not a ppo.Config"
    inner = type(getattr(env, "unwrapped", env))
    if inner not in (CartPole, Pendulum):
        why.append("the engine steps its built-in environments on the device: CartPole (envs/cartpole.py) under a categorical head, Pendulum (envs/pendulum.py) under a Normal head")
    elif inner is Pendulum and _ppo_action_map(env) is None:
        why.append("the action rescale is one scale and offset for every action dimension")
    if getattr(c, "_obs_processors", None) or c.processors or not c.enable_state_encode or c.observation_mode != "":
        why.append("observation processors and observation modes are served by the plugin path: the engine's network reads the environment's observation vector")
    if c.window_length != 1:
        why.append("the engine's network reads one observation (window_length 1)")
    if c.frameskip != 0:
        why.append("the device environments do not skip frames (frameskip 0)")
    if not c.enable_action_decode or not c.enable_sanitize or c.enable_assertion:
        why.append("the device environments take the policy's action bounded to the action space, without per-step assertions (enable_action_decode and enable_sanitize on, enable_assertion off)")
    if (c.reward_scale, c.reward_shift) != (1.0, 0):
        why.append("reward_scale / reward_shift are not applied on the device (reward_clip is)")
    if str(c.dtype).lower() != "float32":
        why.append("the engine computes in float32")
    iv = c.input_block.value
    if iv.name != "MLP" or tuple(iv.kwargs.get("layer_sizes", ())) != ():
        why.append("a trainable input block: the engine's network starts at the hidden block")
    if any(_ppo_block_sizes(b) is None for b in (c.hidden_block, c.value_block, c.policy_block)):
        why.append("the hidden, value and policy blocks are MLPs of ReLU layers (Linear layers with biases)")
    if c.experience_collection_method != "GAE":
        why.append('experience_collection_method "MC": the rollout ends in a GAE scan')
    if c.enable_state_normalized:
        why.append("enable_state_normalized normalises each training batch's states: the engine has no such pass")
    if not c.enable_stable_gradients:
        why.append("enable_stable_gradients=False: the Normal head's log-scale clip is part of the kernels")
    if c.baseline_type not in BASELINES:
        why.append(f"unknown baseline_type {c.baseline_type!r}")
    if admit_kl and c.surrogate_type == "kl":
        if not c.adaptive_kl_target > 0:
            why.append("adaptive_kl_target must be positive")
    elif c.surrogate_type not in ("clip", ""):
        why.append(f'unknown surrogate_type {c.surrogate_type!r} (the engine serves "clip" and "", and "kl", with adaptive_kl_target, is not offered)')
    try:
        N.lr_schedule(c.lr_scheduler)
    except ValueError as e:  # an unknown type, or a piecewise schedule with more than 8 boundaries
        why.append(f"lr_scheduler: {e}")
    return "; ".join(why)


def ppo_config_from(rl_config, env, n_envs: int, seed: int, horizon: int = 32, epochs: int = 4, minibatches: int = 4, admit_kl: bool = False):
    """ppo.Config (srl/algorithms/ppo/config.py:31-128) -> PPODeviceConfig, for a pair `why_not_ppo_engine` admits.  Carried over: the three blocks, both discounts,
    every loss field, lr and its schedule, the gradient clip norm, the log-scale range, reward_clip / state_clip, episode_len = the environment's step limit, the head
    (n_actions of a discrete action space; action_dim, and action_scale / action_offset from the bounds, of a continuous one -- Pendulum: 2 and 0).
    `batch_size`, `memory.*`, `train_num` and `train_every_epoch` describe the plugin's collect-then-train schedule and have no counterpart: the engine's schedule is
    `horizon` x `n_envs` steps per iteration, then `epochs` x `minibatches` updates -- its operating point, chosen here by the caller (PPO_OPERATING_POINT_FIELDS).
    `admit_kl=True` (as `why_not_ppo_engine`'s) also maps `surrogate_type="kl"` and carries `adaptive_kl_target`; beta starts at the reference's 0.5."""
    import copy

    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
    from simple_distributed_rl_amd.device.ppo import PPODeviceConfig

    why = why_not_ppo_engine(env, rl_config, admit_kl=admit_kl)
    if why:
        raise ValueError("PPOEngine cannot run this configuration: " + why)
    c = rl_config
    kl = dict(adaptive_kl_target=float(c.adaptive_kl_target)) if c.surrogate_type == "kl" else {}
    if isinstance(env.action_space, DiscreteSpace):
        head = dict(n_actions=int(env.action_space.n))
    else:
        scale, offset = _ppo_action_map(env)
        head = dict(action_dim=int(np.prod(env.action_space.shape)), action_scale=scale, action_offset=offset)
    return PPODeviceConfig(
        n_envs=n_envs, horizon=horizon, epochs=epochs, minibatches=minibatches, seed=seed, episode_len=int(env.max_episode_steps),
        obs_dim=int(np.prod(env.observation_space.shape)), hidden_sizes=_ppo_block_sizes(c.hidden_block), value_sizes=_ppo_block_sizes(c.value_block),
        policy_sizes=_ppo_block_sizes(c.policy_block), discount=float(c.discount), gae_discount=float(c.gae_discount), baseline_type=c.baseline_type,
        surrogate_type=c.surrogate_type, policy_clip_range=float(c.policy_clip_range), enable_value_clip=bool(c.enable_value_clip),
        value_clip_range=float(c.value_clip_range), lr=float(c.lr), lr_scheduler=copy.deepcopy(c.lr_scheduler), value_loss_weight=float(c.value_loss_weight),
        entropy_weight=float(c.entropy_weight), global_gradient_clip_norm=float(c.global_gradient_clip_norm),
        stable_gradients_scale_range=tuple(float(x) for x in c.stable_gradients_scale_range),
        reward_clip=None if c.reward_clip is None else tuple(float(x) for x in c.reward_clip),
        state_clip=None if c.state_clip is None else tuple(float(x) for x in c.state_clip), **head, **kl,
    )


def engine_kind(rl_config) -> Optional[str]:
    """Which device engine serves this algorithm config (None = the plugin classes only)."""
    return {"Rainbow": "rainbow", "Rainbow_no_multisteps": "rainbow", "Agent57_light": "agent57_light", "DQN": "dqn", "Agent57": "agent57",
            "C51": "c51"}.get(rl_config.get_name())


C51_MP_REASON = "C51 runs on the device engine in train() under set_vector_envs(n); train_mp() keeps it on the plugin path"


def why_not_c51_engine(env, rl_config) -> str:
    """Empty string when `VectorQEngine` (device/mlpq.py) can run this c51.Config on this environment -- `c51_config_from` maps it; otherwise EVERY reason it
    cannot, joined with "; " (as `why_not_ppo_engine`).  The envelope figures are srlx_mlpq_create_categorical's (srlx.h)."""
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    c, why = rl_config, []
    if c.get_name() != "C51":
        return f"'{c.get_name()}' is not a c51.Config"
    if env.player_num != 1:
        why.append("multi-player environment")
    discrete = isinstance(env.action_space, DiscreteSpace)
    A = int(env.action_space.n) if discrete else 0
    if not discrete or not 2 <= A <= 32:
        why.append("the categorical MLP Q-network serves discrete action spaces of 2 to 32 actions")
    N_ = int(c.categorical_num_atoms)
    if not 2 <= N_ <= 256:
        why.append(f"{N_} atoms are outside the categorical head's 2..256")
    elif discrete and A * N_ > 512:
        why.append(f"{A} actions x {N_} atoms = {A * N_} out_layer rows; the categorical head covers at most 512")
    v_min, v_max = float(c.categorical_v_min), float(c.categorical_v_max)
    if not (np.isfinite(v_min) and np.isfinite(v_max) and v_min < v_max):
        why.append(f"the support needs finite categorical_v_min < categorical_v_max (got {v_min}..{v_max})")
    D = flat_dim(frame_space(env, c))
    if D is None:
        why.append("the categorical MLP Q-network reads flat BoxSpace((D,)) observations; image observations stay on the plugin path")
    elif D > 256:
        why.append("the MLP Q-network reads at most 256 observation elements")
    if getattr(c, "_obs_processors", None):
        why.append("observation processors are served by the plugin path")
    if c.window_length != 1:
        why.append("the MLP Q-network reads one observation (window_length 1)")
    sizes = mlp_layer_sizes(c)
    if sizes is None:
        why.append("the MLP Q-network's input value block and hidden block are MLPs of ReLU layers")
    else:
        kw = _mlp_kwargs_reason(c)
        if kw:
            why.append(kw)
        layers = sizes[0] + sizes[1]
        if not 1 <= len(layers) <= 3:
            why.append("the MLP Q-network covers 1 to 3 dense layers (input value block plus hidden block)")
        if any(w % 32 != 0 or not 32 <= w <= 512 for w in layers):
            why.append("the MLP Q-network covers dense layers of 32..512 units in multiples of 32")
    if c.batch_size > 256:
        why.append("the MLP Q-network's gradient step covers batches of at most 256")
    from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig

    if not isinstance(c.memory, ReplayBufferConfig):
        name = getattr(c.memory, "name", type(c.memory).__name__)
        why.append(f"C51 draws uniformly from the ReplayBuffer memory (c51.py:19-20); memory '{name}' stays on the plugin path")
    if c.lr_scheduler.schedule_type != "":
        why.append(f"the MLP Q-network's Adam step takes a constant learning rate; lr_scheduler '{c.lr_scheduler.schedule_type}' stays on the plugin path")
    return "; ".join(why)


def c51_config_from(rl_config, env, n_envs: int, seed: int):
    """c51.Config (srl/algorithms/c51/config.py:23-58) on a flat observation -> VectorQConfig (device/mlpq.py), for a pair `why_not_c51_engine` admits: the
    categorical head's three fields, the uniform memory (alpha = 0, draws without replacement), no target network (target_model_update_interval is unused)."""
    from simple_distributed_rl_amd.device.mlpq import VectorQConfig

    why = why_not_c51_engine(env, rl_config)
    if why:
        raise ValueError("VectorQEngine cannot run this C51 configuration: " + why)
    c, mem = rl_config, rl_config.memory
    ins, hid = mlp_layer_sizes(c)
    return VectorQConfig(
        batch_size=c.batch_size, epsilon=c.epsilon, test_epsilon=c.test_epsilon, lr=c.lr, discount=c.discount, enable_reward_clip=False, enable_double_dqn=False,
        enable_rescale=False, memory_capacity=mem.capacity, memory_warmup_size=mem.warmup_size, memory_has_duplicate=False, memory_alpha=0.0,
        obs_dim=flat_dim(frame_space(env, c)), in_sizes=ins, hidden_sizes=hid, n_actions=int(env.action_space.n),
        categorical_atoms=int(c.categorical_num_atoms), categorical_v_min=float(c.categorical_v_min), categorical_v_max=float(c.categorical_v_max),
        n_envs=n_envs, seed=seed,
    )


def why_not_sacd_engine(env, rl_config, n_envs=None) -> str:
    """Empty string when `SacdEngine` (device/sacd_engine.py) can run this sac.Config on this environment; otherwise EVERY reason it cannot, joined
    with "; " (as `why_not_c51_engine`).  The envelope figures are `SacdUpdate.envelope_reason`'s (srlx_sacd_create's, srlx.h): each dimension is asked about on
    its own beside the smallest shape the kernels take, and the sentence ends in that answer.  `n_envs`: the lane count, when the caller has one.
    `Runner.train()` does not ask: `engine_kind` and `why_not_vector` keep SAC_Discrete on the plugin path; the engine is built around `runner.make_parameter()`."""
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
    from simple_distributed_rl_amd.device.sacd import SacdUpdate
    from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig

    c, why = rl_config, []
    if c.get_name() != "SAC_Discrete":
        return f"'{c.get_name()}' is not a SAC_Discrete config"
    small = dict(D=1, A=2, pw=(32,), qw=(32,), batch=1)  # the smallest shape of the envelope: what stands beside the one dimension that is asked about

    def outside(**one) -> str:
        head, sep, _ = SacdUpdate.envelope_reason(**dict(small, **one)).partition("): ")  # (the tail restates the whole shape, the stand-in values included)
        return head + ")" if sep else head

    if env.player_num != 1:
        why.append("multi-player environment")
    if not isinstance(env.action_space, DiscreteSpace):
        why.append("the engine serves discrete action spaces")
    elif outside(A=int(env.action_space.n)):
        why.append(f"{int(env.action_space.n)} actions: " + outside(A=int(env.action_space.n)))
    D = flat_dim(frame_space(env, c))
    if D is None:
        why.append("the policy and Q-networks read flat BoxSpace((D,)) observations, anything else stays on the plugin path")
    elif outside(D=D):
        why.append(f"{D} observation elements: " + outside(D=D))
    if getattr(c, "_obs_processors", None):
        why.append("observation processors are served by the plugin path")
    if c.window_length != 1:
        why.append("the networks read one observation (window_length 1)")
    iv = c.input_block.value
    if iv.name != "MLP" or tuple(iv.kwargs.get("layer_sizes", ())) != ():
        why.append("an input_block with layers of its own: the kernels start at the observation")
    for name, block in (("policy_block", c.policy_block), ("q_block", c.q_block)):
        sizes = _ppo_block_sizes(block)
        if sizes is None:
            why.append(f"{name} is not an MLP of ReLU layers (Linear layers with biases)")
        elif outside(**{"pw" if name == "policy_block" else "qw": sizes}):
            why.append(f"{name} {sizes}: " + outside(**{"pw" if name == "policy_block" else "qw": sizes}))
    if outside(batch=int(c.batch_size)):
        why.append(outside(batch=int(c.batch_size)))
    if not isinstance(c.memory, ReplayBufferConfig):
        name = getattr(c.memory, "name", type(c.memory).__name__)
        why.append(f"SAC draws uniformly from the ReplayBuffer memory, memory '{name}' stays on the plugin path")
    if n_envs is not None and not (isinstance(n_envs, int) and 1 <= n_envs <= MAX_LANES):
        why.append(f"{n_envs!r} lanes are outside the engine's 1..{MAX_LANES}")
    return "; ".join(why)


def normal_action_bounds(space):
    """(low, high) as float32 [K] arrays of a continuous action space the Normal head's acting kernel serves -- an NpArraySpace, or a flat continuous
    BoxSpace((K,)), with finite bounds -- or a sentence saying why it is not one.  K itself is judged by the update's envelope."""
    from simple_distributed_rl_amd.base.spaces.box import BoxSpace
    from simple_distributed_rl_amd.base.spaces.np_array import NpArraySpace

    flat = isinstance(space, NpArraySpace) or (type(space) is BoxSpace and len(tuple(space.shape)) == 1 and space.stype == SpaceTypes.CONTINUOUS)
    if not flat:
        return "a continuous action space that is not a flat vector of floats (an NpArraySpace or a BoxSpace((K,))): it stays on the plugin path"
    low, high = np.asarray(space.low, np.float32).reshape(-1), np.asarray(space.high, np.float32).reshape(-1)
    if not (np.isfinite(low).all() and np.isfinite(high).all()):
        return "a continuous action space with an infinite bound: the acting kernel rescales its draw onto [low, high]"
    if not (low <= high).all():
        return "a continuous action space whose low is above its high"
    return low, high


def why_not_vppo_engine(env, rl_config, n_envs=None, admit_normal=False) -> str:
    """Empty string when `VppoEngine` (device/vppo_engine.py) can run this ppo_v.Config on this environment; otherwise EVERY reason it cannot, joined
    with "; " (as `why_not_sacd_engine`).  The envelope figures are `VppoUpdate.envelope_reason`'s (srlx_vppo_create's, srlx.h): each dimension is asked about on
    its own beside the smallest shape the kernels take.  `env.max_episode_steps` sizes the tracking ring.  `n_envs`: the lane count, when the caller has one.
    `Runner.train()` does not ask: `engine_kind` and `why_not_vector` keep V-PPO on the plugin path; the engine is built around `runner.make_parameter()`.
    `admit_normal`: the caller runs the Normal head too (`VppoNormalEngine`): a flat continuous action space of 1..8 elements with finite bounds is
    then admitted; the default keeps the categorical engine's answers."""
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace
    from simple_distributed_rl_amd.device.vppo import VppoUpdate
    from simple_distributed_rl_amd.device.vppo_lanes import MAX_EPISODE_STEPS
    from simple_distributed_rl_amd.rl.memories.replay_buffer import ReplayBufferConfig

    c, why = rl_config, []
    if c.get_name() != "V-PPO":
        return f"'{c.get_name()}' is not a V-PPO config"
    small = dict(D=1, head=0, n_out=2, tw=(32,), vw=(), pw=(), batch=1)  # the smallest shape of the envelope: what stands beside the one dimension asked about

    def outside(**one) -> str:
        head, sep, _ = VppoUpdate.envelope_reason(**dict(small, **one)).partition("): ")  # (the tail restates the whole shape, the stand-in values included)
        return head + ")" if sep else head

    if env.player_num != 1:
        why.append("multi-player environment")
    if not isinstance(env.action_space, DiscreteSpace):
        if not admit_normal:
            why.append("a continuous action space: the Normal head's acting kernel is not built, it stays on the plugin path")
        else:
            bounds = normal_action_bounds(env.action_space)
            K = None if isinstance(bounds, str) else len(bounds[0])
            if K is None:
                why.append(bounds)
            elif outside(head=1, n_out=K):
                why.append(f"{K} action elements: " + outside(head=1, n_out=K))
    elif outside(n_out=int(env.action_space.n)):
        why.append(f"{int(env.action_space.n)} actions: " + outside(n_out=int(env.action_space.n)))
    D = flat_dim(frame_space(env, c))
    if D is None:
        why.append("the actor-critic reads flat BoxSpace((D,)) observations, anything else stays on the plugin path")
    elif outside(D=D):
        why.append(f"{D} observation elements: " + outside(D=D))
    if getattr(c, "_obs_processors", None):
        why.append("observation processors are served by the plugin path")
    if getattr(c, "window_length", 1) != 1:
        why.append("the network reads one observation (window_length 1)")
    iv = c.input_block.value
    trunk = []
    refused = VppoUpdate.config_reasons(c)  # block options and lr schedules `VppoUpdate.why_not` refuses
    for name, block in (("input_block", iv), ("hidden_block", c.hidden_block), ("value_block", c.value_block), ("policy_block", c.policy_block)):
        sizes = _ppo_block_sizes(block)
        if sizes is None:
            if not any(f"the {name} sets" in r for r in refused):
                why.append(f"{name} is not an MLP of ReLU layers (Linear layers with biases)")
            if name in ("input_block", "hidden_block"):
                trunk = None
        elif name in ("input_block", "hidden_block"):
            if trunk is not None:
                trunk += list(sizes)
        elif outside(**{"vw" if name == "value_block" else "pw": sizes}):
            why.append(f"{name} {sizes}: " + outside(**{"vw" if name == "value_block" else "pw": sizes}))
    if trunk is not None and outside(tw=tuple(trunk)):
        why.append(f"input_block + hidden_block {tuple(trunk)}: " + outside(tw=tuple(trunk)))
    why += refused
    if outside(batch=int(c.batch_size)):
        why.append(outside(batch=int(c.batch_size)))
    if not isinstance(c.memory, ReplayBufferConfig):
        name = getattr(c.memory, "name", type(c.memory).__name__)
        why.append(f"V-PPO draws uniformly from the ReplayBuffer memory, memory '{name}' stays on the plugin path")
    steps = getattr(env, "max_episode_steps", None)
    if not isinstance(steps, (int, np.integer)) or steps < 1:
        why.append("no known max_episode_steps: the tracking ring holds a whole episode per lane")
    elif steps > MAX_EPISODE_STEPS - 1:  # (the engine sizes the ring for one step more: an EnvRun truncates when its step count exceeds the limit)
        why.append(f"max_episode_steps {int(steps)} above the tracking ring's {MAX_EPISODE_STEPS - 1}")
    elif isinstance(c.memory, ReplayBufferConfig) and steps > int(c.memory.capacity):
        why.append(f"max_episode_steps {int(steps)} above the memory's capacity {int(c.memory.capacity)}: one episode would not fit the item ring")
    if n_envs is not None and not (isinstance(n_envs, int) and 1 <= n_envs <= MAX_LANES):
        why.append(f"{n_envs!r} lanes are outside the engine's 1..{MAX_LANES}")
    return "; ".join(why)


AGENT57_MP_REASON = "Agent57 runs on the device engine in train() under set_vector_envs(n); train_mp() keeps it on the plugin path"


def why_not_agent57_engine(env, rl_config, n_envs=None) -> str:
    """Empty string when `Agent57Engine` (device/agent57.py) can run this agent57.Config on this environment; otherwise EVERY reason it cannot, joined with "; "
    (as `why_not_ppo_engine`).  The envelope figures are srlx_seq_lane_gather's (srlx.h: SRLX_SEQ_MAX_*) and SrlxLstm's.  `n_envs`: the lane count of
    set_vector_envs(n), when the caller has one: the reasons that depend on it are then part of the answer."""
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    c, why = rl_config, []
    if c.get_name() != "Agent57":
        return f"'{c.get_name()}' is not an agent57.Config"
    if not str(c.used_device_torch).startswith("cuda"):
        why.append("the run is not on a GPU device")
    if not isinstance(env.action_space, DiscreteSpace):
        why.append("the engine serves discrete action spaces")
    if env.player_num != 1:
        why.append("multi-player environment")
    mem = _why_not_memory(c)
    if mem:
        why.append(mem)
    if c.window_length != 1:
        why.append("the engine's networks read one observation per step (window_length 1)")
    if getattr(c, "_obs_processors", None):
        why.append("observation processors are served by the plugin path: the lanes hand the networks the environment's float32 observation")
    L = c.burnin + c.sequence_length + 1
    if not 2 <= L <= 513:
        why.append(f"the window burnin + sequence_length + 1 = {L} is outside the lane gather's 2..513")
    n = getattr(env.action_space, "n", 0)
    if isinstance(env.action_space, DiscreteSpace) and not 1 <= n <= 64:
        why.append(f"{n} actions are outside the lane gather's 1..64")
    if not 1 <= c.lstm_units <= 1024:
        why.append(f"{c.lstm_units} recurrent units are outside the lane gather's 1..1024")
    if c.batch_size > 1024:
        why.append(f"a batch of {c.batch_size} is outside the lane gather's 1..1024")
    if isinstance(n_envs, int) and n_envs > 0:
        if n_envs > 256:
            why.append(f"{n_envs} lanes: the acting pass's LSTM kernels serve at most 256 rows (srlx.h), and the engine does not fall back to nn.LSTM")
        if n_envs * L > c.memory.capacity:
            why.append(f"{n_envs} lanes of window {L} emit up to {n_envs * L} windows in one lock-step, more than memory.capacity {c.memory.capacity} keeps")
    return "; ".join(why)


R2D2_MP_REASON = "R2D2 runs on the device engine in train() under set_vector_envs(n); train_mp() keeps it on the plugin path"


def why_not_r2d2_engine(env, rl_config, n_envs=None) -> str:
    """Empty string when `R2D2Engine` (device/r2d2.py) can run this r2d2.Config on this environment; otherwise EVERY reason it cannot, joined
    with "; " (as `why_not_agent57_engine`).  The envelope figures are srlx_r2d2_lane_gather's (srlx.h: SRLX_SEQ_MAX_*) and SrlxLstm's.  `n_envs`: the lane
    count of set_vector_envs(n), when the caller has one: the reasons that depend on it are then part of the answer.  `engine_kind` stays None for R2D2: the
    Runner asks this question on its own, ahead of `why_not_vector`, and only under an explicit lane count."""
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    c, why = rl_config, []
    if c.get_name() != "R2D2":
        return f"'{c.get_name()}' is not an r2d2.Config"
    if not str(c.used_device_torch).startswith("cuda"):
        why.append("the run is not on a GPU device")
    if not isinstance(env.action_space, DiscreteSpace):
        why.append("the engine serves discrete action spaces")
    if env.player_num != 1:
        why.append("multi-player environment")
    mem = _why_not_memory(c)
    if mem:
        why.append(mem)
    if c.window_length != 1:
        why.append("the engine's network reads one observation per step (window_length 1)")
    if getattr(c, "_obs_processors", None):
        why.append("observation processors are served by the plugin path: the lanes hand the network the environment's float32 observation")
    L = c.burnin + c.sequence_length + 1
    if not 2 <= L <= 513:
        why.append(f"the window burnin + sequence_length + 1 = {L} is outside the lane gather's 2..513")
    n = getattr(env.action_space, "n", 0)
    if isinstance(env.action_space, DiscreteSpace) and not 1 <= n <= 64:
        why.append(f"{n} actions are outside the lane gather's 1..64")
    if not 1 <= c.lstm_units <= 1024:
        why.append(f"{c.lstm_units} recurrent units are outside the lane gather's 1..1024")
    if c.batch_size > 1024:
        why.append(f"a batch of {c.batch_size} is outside the lane gather's 1..1024")
    if isinstance(n_envs, int) and n_envs > 0:
        if n_envs > 256:
            why.append(f"{n_envs} lanes: the acting pass's LSTM kernels serve at most 256 rows (srlx.h), and the engine does not fall back to nn.LSTM")
        S = c.sequence_length
        if n_envs * S > c.memory.capacity:
            why.append(f"{n_envs} lanes of sequence length {S} emit up to {n_envs * S} windows in one lock-step, more than memory.capacity {c.memory.capacity} keeps")
    return "; ".join(why)


def frame_space(env, rl_config):
    """The observation space the algorithm sees per step: the environment's, remapped by the config's observation processors."""
    procs = getattr(rl_config, "_obs_processors", None)
    return procs[-1][2] if procs else env.observation_space


def frame_processor(rl_config):
    """The (single) ImageProcessor of the config that a host-stepped batch environment can run on the device, or None."""
    from simple_distributed_rl_amd.rl.processors.image_processor import ImageProcessor

    procs = getattr(rl_config, "_obs_processors", None) or []
    if len(procs) == 1 and isinstance(procs[0][0], ImageProcessor) and "int" in str(np.dtype(procs[0][1].dtype)):
        return procs[0][0]
    return None


def device_config_from(rl_config, env, n_envs: int, seed: int):
    """rainbow.Config (srl/algorithms/rainbow/rainbow.py:57-114) -> the engine's configuration; dqn.Config (srl/algorithms/dqn/dqn.py:50-101) -> the same engine
    with the plain Q head and 1-step targets (dqn.py:144-176 is rainbow_nomultisteps.py:10-43's formula: multisteps=1, retrace_h unused)."""
    from simple_distributed_rl_amd.device.rainbow import RainbowDeviceConfig

    mem = rl_config.memory
    prop = mem.name != "ReplayBuffer"
    kw = mem.kwargs if prop else {}
    hw = _image_hw(frame_space(env, rl_config))
    hb = rl_config.hidden_block
    if engine_kind(rl_config) == "dqn":
        head = dict(enable_noisy_dense=False, multisteps=1, retrace_h=1.0, hidden_units=int(hb.kwargs["layer_sizes"][0]), plain_head=True)
    else:
        head = dict(enable_noisy_dense=rl_config.enable_noisy_dense, multisteps=rl_config.multisteps, retrace_h=rl_config.retrace_h,
                    hidden_units=int(hb.kwargs["layer_sizes"][0]), dueling_type=hb.kwargs.get("dueling_kwargs", {}).get("dueling_type", "average"))
    return RainbowDeviceConfig(
        batch_size=rl_config.batch_size, epsilon=rl_config.epsilon, test_epsilon=rl_config.test_epsilon, lr=rl_config.lr, discount=rl_config.discount,
        target_model_update_interval=rl_config.target_model_update_interval, enable_reward_clip=rl_config.enable_reward_clip,
        enable_double_dqn=rl_config.enable_double_dqn, enable_rescale=rl_config.enable_rescale, window_length=rl_config.window_length,
        memory_capacity=mem.capacity, memory_warmup_size=mem.warmup_size,
        # the uniform ReplayBuffer (priority_memories/replay_buffer.py:10-55) is the alpha = 0 corner of the sum-tree: every leaf
        # weighs 1, so every importance weight is 1 whatever beta is; like random.sample its draws are WITHOUT replacement (a second hit
        # of an item is rejected in draw order, proportional_memory.py:153-157 -- the has_duplicate=False rule of the proportional memory)
        memory_has_duplicate=bool(kw.get("has_duplicate", True)) if prop else False,
        memory_alpha=float(kw.get("alpha", 0.0)), memory_beta_initial=float(kw.get("beta_initial", 0.4)),
        memory_beta_steps=int(kw.get("beta_steps", 1_000_000)), memory_epsilon=float(kw.get("epsilon", 1e-4)),
        filters=32, obs_hw=tuple(hw), n_actions=env.action_space.n, n_envs=n_envs, seed=seed, **head,
    )


class _ReplayFacade:
    """What the loop and callbacks ask of `state.memory` (length for the max_memory rule and progress lines)."""

    def __init__(self, replay):
        self._replay = replay

    def length(self) -> int:
        return self._replay.length()

    def __getattr__(self, item):
        return getattr(self._replay, item)


def load_q_weights(eng, parameter):
    """The Runner's Parameter (reference layout) -> a Q-network engine's online and target networks, and its actors' private copy where it keeps one.  A
    Parameter without `q_target` (C51: c51.py:45-47 holds one network) exchanges the online network alone."""
    online = parameter.q_online.state_dict()
    nets = [(eng.q_online, online)]
    if getattr(parameter, "q_target", None) is not None:
        nets.append((eng.q_target, parameter.q_target.state_dict()))
    if eng.q_actor is not eng.q_online:
        nets.append((eng.q_actor, online))
    for net, sd in nets:
        (net.load_reference_state_dict if hasattr(net, "load_reference_state_dict") else net.load_state_dict)(sd)


def store_q_weights(eng, parameter):
    """The engine's trained online and target networks -> the Runner's Parameter."""
    torch.cuda.synchronize(eng.dev)
    pairs = [(eng.q_online, parameter.q_online)]
    if getattr(parameter, "q_target", None) is not None:
        pairs.append((eng.q_target, parameter.q_target))
    for mine, theirs in pairs:
        sd = mine.reference_state_dict() if hasattr(mine, "reference_state_dict") else mine.state_dict()
        theirs.load_state_dict({k: v.to(next(theirs.parameters()).device) for k, v in sd.items()})


# ---------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------
class VectorActor(ActorDriver):
    def __init__(self, env_run, rl_config, parameter, n_envs: int, overlap: bool = True, use_graphs: bool = True):
        self.env_run, self.rl_config, self.parameter = env_run, rl_config, parameter
        self.lanes = int(n_envs)
        self.overlap, self.use_graphs = overlap, use_graphs
        self.engine = None
        self._eps_sched = None
        self._iteration = 0
        self._graphs_ready = False

    # -- set-up ---------------------------------------------------------------------------------
    def _make_batch_env(self, replay, context):
        base = self.env_run.unwrapped
        maker = getattr(type(base), "device_vector", None)
        if maker is not None:
            return maker(replay, **self.env_run.config.kwargs)
        if not replay.obs_uint8:  # flat observations (VectorQEngine)
            env = HostVecEnv(self.env_run.config, self.lanes, replay.dev, context.seed, float_obs=True)
        else:
            env = HostVecEnv(self.env_run.config, self.lanes, replay.dev, context.seed, processor=frame_processor(self.rl_config))
        env.setup(context)
        return env

    def open(self, context, state):
        """(everything happens in `attach`: the engine draws from its own seeded generators, not from the process-wide ones on_start may precede)"""

    def attach(self, context, state):
        dev = torch.device(context.used_device_torch)
        if self.engine is None:  # the engine (replay included) lives as long as the Runner: a second train() continues on the same memory
            self.engine = self._make_engine(context, dev.index or 0, 0 if context.seed is None else int(context.seed))
        eng = self.engine
        self._load_weights()
        if eng.ledger is None:
            eng.ledger = EpisodeLedger(self.lanes, dev)  # same tensors for the engine's lifetime: the captured commit graph points at them
        eng.ledger.clear()
        self._iteration = 0  # every lane is a worker whose step_in_training restarts with the run (worker_run.py setup)
        self._set_mode(context)
        state.env, state.worker, state.workers = self.env_run, None, []
        state.parameter, state.memory = self.parameter, _ReplayFacade(eng.replay)
        state.worker_indices = [0]
        state.episode_count = 0
        self._episodes_announced = 0

    def _make_engine(self, context, device: int, seed: int):
        def env(replay):
            return self._make_batch_env(replay, context)

        if engine_kind(self.rl_config) == "c51":  # the MLP Q-network engine with the categorical head
            from simple_distributed_rl_amd.device.mlpq import VectorQEngine

            self.cfg = c51_config_from(self.rl_config, self.env_run, self.lanes, seed)
            return VectorQEngine(self.cfg, device, env=env)
        if is_flat_dqn(self.env_run, self.rl_config):  # flat observations: the MLP Q-network engine
            from simple_distributed_rl_amd.device.mlpq import VectorQEngine

            self.cfg = mlp_config_from(self.rl_config, self.env_run, self.lanes, seed)
            return VectorQEngine(self.cfg, device, env=env)
        from simple_distributed_rl_amd.device.rainbow import RainbowEngine

        self.cfg = device_config_from(self.rl_config, self.env_run, self.lanes, seed)
        return RainbowEngine(self.cfg, device, env=env, overlap=self.overlap)

    def _load_weights(self):
        if self.parameter is not None:
            load_q_weights(self.engine, self.parameter)

    def _store_weights(self):
        if self.parameter is not None:
            store_q_weights(self.engine, self.parameter)

    def _set_mode(self, context):
        """This run's exploration: the config's epsilon schedule while training (none for noisy nets), `test_epsilon` otherwise."""
        self._eps_sched = None if getattr(self.rl_config, "enable_noisy_dense", False) else self.rl_config.epsilon_scheduler.create(self.rl_config.epsilon)
        self._eps_now = None
        self._training = bool(context.training)
        if not self._training:
            self.engine.eps.fill_(float(self.rl_config.test_epsilon))

    # -- the loop's calls -------------------------------------------------------------------------
    def _book(self, state, records, hooks, fire: bool):
        for ret, length in records:
            state.episode_count += 1
            state.episode_rewards_list.append([ret])
            state.last_episode_rewards = [ret]
            state.last_episode_step = length
            if fire:
                hooks.fire("on_episode_end")

    def roll_episodes(self, context, state, hooks) -> bool:
        if self._iteration == 0:
            hooks.fire("on_episode_begin")  # the E first episodes begin together
        elif hooks.wants("on_episode_begin"):
            while self._episodes_announced < state.episode_count:  # one per episode that ended: its lane started the next one
                self._episodes_announced += 1
                hooks.fire("on_episode_begin")
        if context.max_episodes > 0 and state.episode_count >= context.max_episodes:
            return False
        return True

    def act(self, context, state, hooks):
        eng = self.engine
        if self._eps_sched is not None and self._training:
            eps = self._eps_sched.update(self._iteration).to_float()  # every lane is a worker at its `_iteration`-th step (rainbow.py:311)
            if eps != getattr(self, "_eps_now", None):
                eng.eps.fill_(float(eps))
                self._eps_now = eps
        eng.actor_front()
        state.action = eng.actions
        hooks.fire("on_step_action_after")
        if eng.overlap:
            eng.join_learner()  # the updates forked after the previous lock-step: they must finish before the replay changes
            eng.refresh_actor_copy()
        eng.actor_commit()
        eng.ledger.post()
        state.total_step += self.lanes
        self._iteration += 1

    def settle(self, context, state, hooks):
        led = self.engine.ledger
        exact = context.max_episodes > 0 or hooks.wants("on_episode_end", "on_episode_begin")
        if exact:
            self._book(state, led.drain(), hooks, fire=True)
        else:
            state.episode_count = led.peek()[0]  # lags the device by at most the mailbox depth; exact at close

    def close(self, context, state):
        if self.engine is not None:
            self.engine.join_learner()
            self._finish(state)

    def _finish(self, state):
        """End-of-run bookkeeping (the ledger's last episodes, the exact step count), then the weights go back to the Runner's Parameter."""
        eng = self.engine
        torch.cuda.synchronize(eng.dev)
        already = len(state.episode_rewards_list)
        records = eng.ledger.drain()
        total = eng.ledger.peek(wait=True)
        state.episode_count = already  # _book counts up from what was booked one by one
        self._book(state, records, None, fire=False)
        state.episode_count = total[0]
        state.shared_vars["env_steps_exact"] = total[1]  # lanes that only received a reset frame are not environment steps
        self._store_weights()

    # -- graphs -----------------------------------------------------------------------------------
    def ensure_graphs(self):
        """Capture the lock-step's launch-bound parts and the whole update into HIP graphs, once the replay is warm (the
        learner's arenas are sized by one eager update first; that update is a real one and is counted by the caller)."""
        if self._graphs_ready or not self.use_graphs:
            return 0
        eng = self.engine
        before = eng.train_count
        eng.join_learner()
        # a host-stepped batch environment reads the actions back every lock-step: its step cannot live in a graph
        eng.capture_graphs(actor=getattr(eng.env, "capturable", True), learner=True, warm_actor=False, warm_learner=True)
        self._graphs_ready = True
        return eng.train_count - before


class VectorLearner(LearnerDriver):
    """`trainer`-shaped view of the engine's learner: `train_count`, `info`, `train()`."""

    def __init__(self, actor: VectorActor):
        self.actor = actor
        self.info: dict = {}

    @property
    def engine(self):
        return self.actor.engine

    @property
    def train_count(self) -> int:
        return self.engine.train_count if self.engine is not None else 0

    def attach(self, context, state):
        state.trainer = self

    def open(self, context, state):
        pass

    def train(self):
        self.update(1, None)

    def update(self, count: int, state) -> int:
        eng = self.engine
        if eng.replay.is_warmup_needed():
            return 0
        ran = self.actor.ensure_graphs()  # first warm call: one eager update + graph capture
        count -= ran
        if count > 0:
            if eng.overlap:
                ran += eng.fork_learner(count)
            else:
                for _ in range(count):
                    ran += int(eng.learner_step())
        return ran

    def close(self, context, state):
        eng = self.engine
        if eng is not None:
            eng.join_learner()
            torch.cuda.synchronize(eng.dev)
            self.info = eng.info()


class VectorAgent57Actor(VectorActor):
    """`Runner.train()` with Agent57_light on a GPU: E lanes of an Agent57_light engine.  84 x 84 x 4 configs get `Agent57LightFastEngine` (device/agent57_fast.py),
    which trains master copies of its own: the Runner's Parameter holds the trained networks only once `close` has exported them.  Other geometries get
    `Agent57LightEngine` (device/agent57_light.py), which trains the Parameter's five torch networks in place."""

    def _make_engine(self, context, device: int, seed: int):
        from simple_distributed_rl_amd.device.agent57_fast import Agent57LightFastEngine, why_not_fast
        from simple_distributed_rl_amd.device.agent57_light import Agent57LightEngine

        # 84 x 84 x 4 configs: every network pass and optimiser step in libsrlx (round 6); other geometries: the round-5 engine (image trunks in libsrlx, dense
        # tails in torch)
        cls = Agent57LightFastEngine if not why_not_fast(self.rl_config) else Agent57LightEngine
        return cls(self.rl_config, self.lanes, device, seed=seed, env=lambda replay: self._make_batch_env(replay, context), parameter=self.parameter)

    def _load_weights(self):
        """(the engine took the Runner's Parameter when it was built)"""

    def _store_weights(self):
        if hasattr(self.engine, "export_parameter"):  # the all-libsrlx engine trains masters of its own: the Runner's Parameter gets the result
            self.engine.export_parameter(self.parameter)

    def _set_mode(self, context):
        self.engine.training = bool(context.training)

    def act(self, context, state, hooks):
        eng = self.engine
        eng.actor_step()
        state.action = eng.actions
        hooks.fire("on_step_action_after")
        eng.ledger.post()
        state.total_step += self.lanes
        self._iteration += 1

    def close(self, context, state):
        if self.engine is not None:  # (no join here: `actor_step` joins the forked updates before its tree add, and joining again would be one more stream wait)
            self._finish(state)

    def ensure_graphs(self):
        """The whole update as one HIP graph once the replay is warm (its warm-up updates are real ones and are counted by the caller)."""
        eng = self.engine
        if self._graphs_ready or not self.use_graphs:
            return 0
        before = eng.train_count
        eng.capture_graphs()
        self._graphs_ready = True
        return eng.train_count - before


class VectorAgent57LstmActor(VectorAgent57Actor):
    """`Runner.train()` with Agent57 (the LSTM one) on a GPU under set_vector_envs(n): n lanes of `Agent57Engine` (device/agent57.py), which steps host
    environments with float32 observations and trains the Runner's Parameter in place with the plugin's own trainer."""

    def _make_batch_env(self, ring, context):
        env = HostVecEnv(self.env_run.config, self.lanes, ring.dev, context.seed, float_obs=True)
        env.setup(context)
        return env

    def _make_engine(self, context, device: int, seed: int):
        from simple_distributed_rl_amd.device.agent57 import Agent57Engine

        return Agent57Engine(self.rl_config, self.lanes, device, seed=seed, env=lambda ring: self._make_batch_env(ring, context), parameter=self.parameter,
                             context=context)

    def attach(self, context, state):
        fresh = self.engine is None
        super().attach(context, state)
        if not fresh:  # a further train() on the same engine: the trainer is set up with this run's context, as the plugin learner's is when a run opens
            self.engine.setup_trainer(context)

    def _set_mode(self, context):
        assert context.training, "Agent57Engine only trains: evaluate / rollout stay on the plugin path"

    def ensure_graphs(self):
        """(the lock-step reads `done` back and the trainer is torch's eager autograd: nothing is captured)"""
        return 0


class VectorR2D2Actor(VectorAgent57LstmActor):
    """`Runner.train()` with R2D2 on a GPU under set_vector_envs(n): n lanes of `R2D2Engine` (device/r2d2.py), which steps host environments with float32
    observations and their invalid-action masks and trains the Runner's Parameter in place with the plugin's own trainer."""

    def _make_batch_env(self, ring, context):
        from simple_distributed_rl_amd.device.r2d2 import MaskedHostVecEnv

        env = MaskedHostVecEnv(self.env_run.config, self.lanes, ring.dev, context.seed, float_obs=True)
        env.setup(context)
        return env

    def _make_engine(self, context, device: int, seed: int):
        from simple_distributed_rl_amd.device.r2d2 import R2D2Engine

        return R2D2Engine(self.rl_config, self.lanes, device, seed=seed, env=lambda ring: self._make_batch_env(ring, context), parameter=self.parameter,
                          context=context)

    def _set_mode(self, context):
        assert context.training, "R2D2Engine only trains: evaluate / rollout stay on the plugin path"


class VectorR2D2Learner(VectorLearner):
    """`VectorLearner` that stops at the run's `max_train_count`: a lock-step of n lanes owes n updates, and the plugin path's run ends on the update that
    reaches the budget, not on the lock-step that crosses it."""

    def open(self, context, state):
        self._budget = int(context.max_train_count) if context.max_train_count > 0 else None

    def update(self, count: int, state) -> int:
        if self._budget is not None and state is not None:
            count = min(count, self._budget - state.train_count)
        return super().update(count, state) if count > 0 else 0
