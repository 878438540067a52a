"""The inputs of tests/golden/train_step_rainbow_noisy_vec.npz (oracle/gen_golden_rainbow_noisy_vec.py): Rainbow's network with `enable_noisy_dense` on a flat
Box(4) observation with 2 actions (rainbow/model_torch.py:15-29 -- the input value block's layers stay Linear; the hidden block's MLP layers and the four
layers of the dueling head are NoisyLinear, srl/rl/torch_/modules/noisy_linear.py:8-52), its mu and sigma tensors regenerated from seeds instead of stored, and
the sampled n-step items.  Imported by the generator and by the noisy Rainbow-on-flat-observations tests; pure numpy, identical on every platform."""
import numpy as np

import rainbow_vec_recipe as RC

SEED_ONLINE, SEED_TARGET = 17, 18
B, D, A = RC.B, RC.D, RC.A
ENDS = RC.ENDS
GREEDY_SHARE = RC.GREEDY_SHARE

# name -> input value block layers (plain), the hidden block's layer_sizes (noisy), dueling_type, multisteps, retrace_h, double DQN
CASES = {
    "d64_n3_dd1": dict(in_sizes=(), layer_sizes=(64,), dueling_type="average", n=3, retrace_h=1.0, double_dqn=True),  # the noisy head on the raw observation
    "i32_d64x64_naive_n2_dd0": dict(in_sizes=(32,), layer_sizes=(64, 64), dueling_type="", n=2, retrace_h=1.0, double_dqn=False),  # plain, noisy, then the head
}

trunk_of = RC.trunk_of


def layer_keys(case):
    """(reference key of the layer, noisy?, (out, in)) of every dense layer in the reference's order."""
    plain = RC.keys_shapes(case)
    n_in = len(case["in_sizes"])
    return [(plain[2 * l][0][: -len(".weight")], l >= n_in, plain[2 * l][1]) for l in range(len(plain) // 2)]


def keys_shapes(case):
    """The reference module tree's state_dict keys and shapes, in its order (a NoisyLinear's parameters: w_mu, w_sigma, b_mu, b_sigma)."""
    out = []
    for key, noisy, (o, i) in layer_keys(case):
        if noisy:
            out += [(key + ".w_mu", (o, i)), (key + ".w_sigma", (o, i)), (key + ".b_mu", (o,)), (key + ".b_sigma", (o,))]
        else:
            out += [(key + ".weight", (o, i)), (key + ".bias", (o,))]
    return out


def mu_keys(case):
    """The keys of EngineMLPQNet.kernel_parameters(): weight / bias of a plain layer, w_mu / b_mu of a noisy one."""
    out = []
    for key, noisy, _ in layer_keys(case):
        out += [key + ".w_mu", key + ".b_mu"] if noisy else [key + ".weight", key + ".bias"]
    return out


def sigma_keys(case):
    """One entry per mu_keys() entry: the sigma tensor's key, None for a plain layer's tensors."""
    out = []
    for key, noisy, _ in layer_keys(case):
        out += [key + ".w_sigma", key + ".b_sigma"] if noisy else [None, None]
    return out


def recipe_state_dict(case, seed: int):
    """Weights and w_mu uniform in +-1 / sqrt(in), biases and b_mu a tenth of +-1 / sqrt(out) (rainbow_vec_recipe's rule), every sigma uniform in
    [0.25, 0.75] / sqrt(in) -- around the reference's initial 0.5 / sqrt(in), but different in every element, so a swapped or shifted eps shows -- drawn in key
    order from one PCG64 stream."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for key, noisy, (o, i) in layer_keys(case):
        names = (".w_mu", ".w_sigma", ".b_mu", ".b_sigma") if noisy else (".weight", ".bias")
        for nm in names:
            shape = (o, i) if nm in (".w_mu", ".w_sigma", ".weight") else (o,)
            if "sigma" in nm:
                out[key + nm] = (rng.uniform(0.25, 0.75, size=shape) / np.sqrt(i)).astype(np.float32)
            elif len(shape) == 2:
                out[key + nm] = rng.uniform(-1.0 / np.sqrt(i), 1.0 / np.sqrt(i), size=shape).astype(np.float32)
            else:
                out[key + nm] = (rng.uniform(-1.0 / np.sqrt(o), 1.0 / np.sqrt(o), size=shape).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    return out


def _mu_as_plain(case, sd):
    return {pk: sd[mk] for (pk, _), mk in zip(RC.keys_shapes(case), mu_keys(case))}


def make_items(case, seed: int = 41):
    """rainbow_vec_recipe.make_items's items (states a slow walk at twice CartPole's scales, items ENDS ending at step 1 with padding behind).  The taken actions
    at steps m >= 1 follow the arg-max of the selecting network's MU tensors on s_{m+1} for about GREEDY_SHARE of the entries and its complement otherwise:
    the noise of the recorded step is not known here, so the retrace comparison (rainbow.py:267) agrees with this choice often, not always -- chains of every
    length still occur (tests/test_rainbow_noisy_vector_cpu.py checks it on the recorded draws)."""
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
    for b in ENDS:
        terminated[b, 1:] = 1.0
        rewards[b, 2:] = 0.0
        states[b, 3:] = states[b, 2]
    sel = _mu_as_plain(case, recipe_state_dict(case, SEED_ONLINE if case["double_dqn"] else SEED_TARGET))
    greedy = RC.forward64(case, sel, states[:, 1:].reshape(B * n, D)).argmax(-1).reshape(B, n)
    take = rng.random((B, n)) < GREEDY_SHARE
    for m in range(1, n):
        actions[:, m] = np.where(take[:, m], greedy[:, m], (greedy[:, m] + 1) % A).astype(np.int32)
    weights = (0.3 + 0.7 * rng.random(B)).astype(np.float32)
    return states, actions, rewards, terminated, weights
