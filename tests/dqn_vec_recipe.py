"""The inputs of tests/golden/train_step_dqn_vec.npz (oracle/gen_golden_dqn_vec.py): DQN's network on a flat Box(4) observation with 2 actions
(dqn/model_torch.py:17-29 -- in_block (flatten) -> hidden_block (MLP) -> out_layer), its weights regenerated from seeds instead of stored, and the sampled
batch.  Imported by the generator and by tests/test_dqn_vector_gpu.py; pure numpy, identical on every platform."""
import numpy as np

SEED_ONLINE, SEED_TARGET = 20261101, 20261102
B, D, A = 32, 4, 2
TERMINAL = 5  # the item whose transition ends its episode (undone = 0)
SHAPES = {"h64x64": (64, 64), "h512": (512,)}  # the hidden block's layer sizes
DOUBLE = (True, False)


def case_name(shape_key: str, double_dqn: bool) -> str:
    return f"{shape_key}_dd{int(bool(double_dqn))}"


def keys_shapes(hidden):
    """The reference module tree's state_dict keys and shapes, in its order (the input value block has no layers: Flatten only)."""
    out, prev = [], D
    for k, w in enumerate(hidden):
        out += [(f"hidden_block.hidden_layers.{2 * k}.weight", (w, prev)), (f"hidden_block.hidden_layers.{2 * k}.bias", (w,))]
        prev = w
    out += [("out_layer.weight", (A, prev)), ("out_layer.bias", (A,))]
    return out


def recipe_state_dict(hidden, seed: int):
    """Every tensor uniform in +-1 / sqrt(fan_in) (biases: fan_in = their length), drawn in key order from one PCG64 stream."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for key, shape in keys_shapes(hidden):
        fan_in = int(shape[1]) if len(shape) > 1 else int(shape[0])
        out[key] = rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), size=shape).astype(np.float32)
    return out


def make_items(seed: int = 29):
    """s0, s1 float32 [B][D] (CartPole-like scales), actions int32 [B], rewards float32 [B], undone float32 [B] (item TERMINAL ends its episode),
    importance weights float32 [B]."""
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 1.5, 0.1, 1.5], np.float32)
    s0 = (rng.standard_normal((B, D)) * scale).astype(np.float32)
    s1 = (s0 + 0.05 * rng.standard_normal((B, D)) * scale).astype(np.float32)
    actions = rng.integers(0, A, B).astype(np.int32)
    reward = np.ones(B, np.float32)
    reward[::7] = 0.0
    undone = np.ones(B, np.float32)
    undone[TERMINAL] = 0.0
    weights = (0.3 + 0.7 * rng.random(B)).astype(np.float32)
    return s0, s1, actions, reward, undone, weights
