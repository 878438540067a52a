"""The yardstick of the SAC-Discrete engine's two launches (srlx_sacd_act, srlx_sacd_ring_batch): a float64 numpy mirror written as another
program -- whole arrays where the kernel has one thread per element, the keyed uniforms from the oracle's restatement of the counter generator
(oracle/hot_path_oracle.py: rng_uniform), the batch assembly by plain indexing.  It reads nothing from the library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from hot_path_oracle import rng_uniform  # noqa: E402


def uniforms(seed, counter, n_rows, A):
    """U[r][a]: what srlx_rng_uniform(seed, counter, n_rows * A) writes at r * A + a."""
    return rng_uniform(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), counter, n_rows * A).reshape(n_rows, A)


def random_actions(U, A):
    """The Worker's sample_action() while start_steps last, from each row's FIRST uniform: min(A - 1, floor(U A))."""
    return np.minimum(A - 1, np.floor(np.asarray(U, np.float64)[:, 0] * A).astype(np.int64)).astype(np.int32)


def rescaled(U):
    """rng.uniform(1e-6, 1.0): low + (high - low) * U."""
    return 1e-6 + (1.0 - 1e-6) * np.asarray(U, np.float64)


def scores(logits, U):
    """gumbel_max_sample's argument (algorithms/sac.py:140-143) in float64: logits - log(-log(u))."""
    return np.asarray(logits, np.float64) - np.log(-np.log(rescaled(U)))


def first_argmax(s):
    return np.argmax(s, axis=1).astype(np.int32)  # numpy's argmax returns the first maximum


def top_two_gap(s):
    t = np.sort(np.asarray(s, np.float64), axis=1)
    return t[:, -1] - t[:, -2]


def act(logits, seed, counter, random_until, A):
    """(actions, scores) of srlx_sacd_act for rows whose logits are given."""
    U = uniforms(seed, counter, len(logits), A)
    s = scores(logits, U)
    return (random_actions(U, A) if counter < random_until else first_argmax(s)), s


def ring_batch(ring, offsets, actions, terminated, D, A):
    """The drawn items as the update's tensors, by indexing: `ring` the flat float32 ring, `offsets` int64 [B][2] in floats."""
    offsets = np.asarray(offsets, np.int64)
    states = np.stack([ring[o:o + D] for o in offsets[:, 0]])
    next_states = np.stack([ring[o:o + D] for o in offsets[:, 1]])
    onehot = (np.arange(A)[None, :] == np.asarray(actions).reshape(-1, 1)).astype(np.float32)
    done = (np.asarray(terminated).reshape(-1) != 0).astype(np.uint8)
    return states, next_states, onehot, done
