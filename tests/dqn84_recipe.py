"""The inputs of tests/golden/train_step_dqn84.npz (oracle/gen_golden_dqn84.py): DQN's network at the Atari shape (dqn/model_torch.py:17-29 --
DQN image block, one dense layer of 512, out_layer over 6 actions), its weights regenerated from seeds instead of stored, and the sampled batch.
Imported by the generator and by tests/test_dqn_engine_gpu.py; pure numpy, identical on every platform."""
import numpy as np

SEED_ONLINE, SEED_TARGET = 20261016, 20261017
B, A, W = 16, 6, 512
TERMINAL = 3  # the item whose transition ends its episode (undone = 0)

# the reference module tree's state_dict keys and shapes, in its order (in_block -> hidden_block -> out_layer)
KEYS_SHAPES = [
    ("in_block.image_block.image_layers.0.weight", (32, 4, 8, 8)), ("in_block.image_block.image_layers.0.bias", (32,)),
    ("in_block.image_block.image_layers.2.weight", (64, 32, 4, 4)), ("in_block.image_block.image_layers.2.bias", (64,)),
    ("in_block.image_block.image_layers.4.weight", (64, 64, 3, 3)), ("in_block.image_block.image_layers.4.bias", (64,)),
    ("hidden_block.hidden_layers.0.weight", (W, 7744)), ("hidden_block.hidden_layers.0.bias", (W,)),
    ("out_layer.weight", (A, W)), ("out_layer.bias", (A,)),
]


def recipe_state_dict(seed: int):
    """Every tensor uniform in +-1 / sqrt(fan_in) (biases: fan_in = their length), drawn in key order from one PCG64 stream."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for key, shape in KEYS_SHAPES:
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
        out[key] = rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), size=shape).astype(np.float32)
    return out


def make_items(seed: int = 23):
    """frames uint8 [B][5][84][84] (s_0 = frames[b, 0:4], s_1 = frames[b, 1:5], oldest first), actions int32 [B], rewards float32 [B] in {-1, 0, 1},
    undone float32 [B] (item TERMINAL ends its episode), importance weights float32 [B]."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, 5, 84, 84), dtype=np.uint8)
    actions = rng.integers(0, A, B).astype(np.int32)
    reward = rng.integers(-1, 2, B).astype(np.float32)
    undone = np.ones(B, np.float32)
    undone[TERMINAL] = 0.0
    weights = (0.3 + 0.7 * rng.random(B)).astype(np.float32)
    return frames, actions, reward, undone, weights
