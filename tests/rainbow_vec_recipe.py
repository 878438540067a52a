"""The inputs of tests/golden/train_step_rainbow_vec.npz (oracle/gen_golden_rainbow_vec.py): Rainbow's network on a flat Box(4) observation with 2 actions
(rainbow/model_torch.py:15-29 -- in_block (flatten + the input value block's layers) -> hidden_block (MLP over layer_sizes[:-1], then a DuelingNetworkBlock
of layer_sizes[-1] units)), its weights regenerated from seeds instead of stored, and the sampled n-step items.  Imported by the generator and by the
Rainbow-on-flat-observations tests; pure numpy, identical on every platform."""
import numpy as np

SEED_ONLINE, SEED_TARGET = 7, 8  # (with these both networks' arg-max varies over the items in every case)
B, D, A = 32, 4, 2
ENDS = (5, 19)  # the items whose episode ends inside the window: `terminated` is 1 at step 1, the steps behind it are padding (rainbow.py:358-371)
GREEDY_SHARE = 0.6  # of the taken actions at steps >= 1 that are set to the greedy one (the retrace coefficient stays non-zero there)

# name -> input value block layers, the hidden block's layer_sizes, dueling_type, multisteps, retrace_h, double DQN
CASES = {
    "d512_n3_dd1": dict(in_sizes=(), layer_sizes=(512,), dueling_type="average", n=3, retrace_h=1.0, double_dqn=True),  # rainbow.Config()'s block
    "d512_n3_dd0": dict(in_sizes=(), layer_sizes=(512,), dueling_type="average", n=3, retrace_h=1.0, double_dqn=False),
    "i32_d64x64_n3_dd1": dict(in_sizes=(32,), layer_sizes=(64, 64), dueling_type="average", n=3, retrace_h=1.0, double_dqn=True),  # a trunk layer from each block
    "i32_d64x64_n3_dd0": dict(in_sizes=(32,), layer_sizes=(64, 64), dueling_type="average", n=3, retrace_h=1.0, double_dqn=False),
    "d512_n1_dd1": dict(in_sizes=(), layer_sizes=(512,), dueling_type="average", n=1, retrace_h=1.0, double_dqn=True),  # Rainbow_no_multisteps
    "d64x64_naive_n5_h05_dd1": dict(in_sizes=(), layer_sizes=(64, 64), dueling_type="", n=5, retrace_h=0.5, double_dqn=True),
}


def trunk_of(case):
    """(input value block layers, the hidden block's layer_sizes[:-1], dueling units)."""
    return tuple(case["in_sizes"]), tuple(case["layer_sizes"][:-1]), int(case["layer_sizes"][-1])


def keys_shapes(case):
    """The reference module tree's state_dict keys and shapes, in its order."""
    ins, hid, H = trunk_of(case)
    out, prev = [], D
    for k, w in enumerate(ins):  # in_block.hidden_layers = [Flatten, Linear, ReLU, ...]
        out += [(f"in_block.hidden_layers.{1 + 2 * k}.weight", (w, prev)), (f"in_block.hidden_layers.{1 + 2 * k}.bias", (w,))]
        prev = w
    for k, w in enumerate(hid):
        out += [(f"hidden_block.hidden_layers.{2 * k}.weight", (w, prev)), (f"hidden_block.hidden_layers.{2 * k}.bias", (w,))]
        prev = w
    head = f"hidden_block.hidden_layers.{2 * len(hid)}"
    for branch, units in (("v_layers", 1), ("adv_layers", A)):
        out += [(f"{head}.{branch}.0.weight", (H, prev)), (f"{head}.{branch}.0.bias", (H,)), (f"{head}.{branch}.2.weight", (units, H)),
                (f"{head}.{branch}.2.bias", (units,))]
    return out


def recipe_state_dict(case, seed: int):
    """Every weight uniform in +-1 / sqrt(fan_in), every bias a tenth of that with fan_in = its length (with full-size biases of 1 or 2 entries the arg-max
    hardly depends on the observation), drawn in key order from one PCG64 stream."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for key, shape in keys_shapes(case):
        fan_in = int(shape[1]) if len(shape) > 1 else int(shape[0])
        t = rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), size=shape).astype(np.float32)
        out[key] = t if len(shape) > 1 else (t * np.float32(0.1)).astype(np.float32)
    return out


def forward64(case, sd, x):
    """The network in float64 numpy (this module's own: it only decides which actions the items take)."""
    ins, hid, _ = trunk_of(case)
    keys = [k for k, _ in keys_shapes(case)]
    p = [sd[k].astype(np.float64) for k in keys]
    h = np.asarray(x, np.float64)
    nt = len(ins) + len(hid)
    for l in range(nt):
        h = np.maximum(h @ p[2 * l].T + p[2 * l + 1], 0.0)
    q = p[2 * nt:]
    v = np.maximum(h @ q[0].T + q[1], 0.0) @ q[2].T + q[3]
    adv = np.maximum(h @ q[4].T + q[5], 0.0) @ q[6].T + q[7]
    return v + adv - adv.mean(-1, keepdims=True) if case["dueling_type"] == "average" else v + adv


def make_items(case, seed: int = 31):
    """states float32 [B][n + 1][D] (twice CartPole's scales, a slow walk), actions int32 [B][n], rewards float32 [B][n], terminated float32 [B][n], importance
    weights float32 [B].  Items ENDS end their episode at step 1 (n > 1: the steps behind repeat the last state with reward 0, terminated 1 and a random
    action, rainbow.py:358-371; n = 1: item ENDS[0] alone, terminated at step 0).  About GREEDY_SHARE of the actions at steps m >= 1 equal the arg-max of the
    selecting network's Q on s_{m+1} (the online network under double DQN, the target network otherwise) -- the comparison rainbow.py:267 makes -- and the
    others are its complement, so retrace chains of every length occur."""
    n = int(case["n"])
    rng = np.random.default_rng(seed)
    scale = np.array([2.0, 3.0, 0.2, 3.0], np.float32)
    states = np.zeros((B, n + 1, D), np.float32)
    states[:, 0] = (rng.standard_normal((B, D)) * scale).astype(np.float32)
    for m in range(1, n + 1):
        states[:, m] = (states[:, m - 1] + 0.05 * rng.standard_normal((B, D)) * scale).astype(np.float32)
    actions = rng.integers(0, A, (B, n)).astype(np.int32)
    rewards = np.ones((B, n), np.float32)
    rewards[::7, 0] = 0.0
    terminated = np.zeros((B, n), np.float32)
    if n == 1:
        terminated[ENDS[0], 0] = 1.0
    else:
        for b in ENDS:
            terminated[b, 1:] = 1.0
            rewards[b, 2:] = 0.0
            states[b, 3:] = states[b, 2]
    sel = recipe_state_dict(case, SEED_ONLINE if case["double_dqn"] else SEED_TARGET)
    greedy = forward64(case, sel, states[:, 1:].reshape(B * n, D)).argmax(-1).reshape(B, n)  # [:, m] = the arg-max on s_{m+1}
    take = rng.random((B, n)) < GREEDY_SHARE
    for m in range(1, n):
        actions[:, m] = np.where(take[:, m], greedy[:, m], (greedy[:, m] + 1) % A).astype(np.int32)
    weights = (0.3 + 0.7 * rng.random(B)).astype(np.float32)
    return states, actions, rewards, terminated, weights
