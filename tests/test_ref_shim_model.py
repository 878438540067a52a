"""The shim's reference model (tests/ref_shim.py) against the reference's own recorded runs.  CPU only.

Every golden trace whose script draws from `random` only through the memory is replayed through
RefShim under random.seed(seed): the model must reproduce the reference's indices, weights, final
tree and the generator's next value -- its uniform accounting (rejected draws included) is the
reference's before any GPU result is compared with it (tests/test_per_shim_edges_gpu.py)."""
import glob
import os
import random

import numpy as np
import pytest

from oracle_bindings import iter_trace
from ref_shim import W_RTOL, RefShim

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "per_trace_*.npz"))) if int(np.load(p)["script_uses_random"]) == 0]


def test_there_are_traces_to_replay():
    assert len(TRACES) >= 5


@pytest.mark.parametrize("path", TRACES, ids=[os.path.basename(p)[10:-4] for p in TRACES])
def test_ref_shim_replays_reference_trace(path):
    z = np.load(path)
    m = RefShim(int(z["capacity"]), float(z["alpha"]), float(z["beta_initial"]), float(z["beta_steps"]), bool(z["has_duplicate"]), float(z["epsilon"]))
    cap = int(z["capacity"])
    random.seed(int(z["seed"]))
    item, n_samples = 0, 0
    for kind, p in iter_trace(z):
        if kind == "add":
            m.add(("item", item), p["priority"])
            item += 1
        elif kind == "sample":
            batches, w, idx = m.sample(p["batch_size"], p["step"])
            assert idx == p["indices"].tolist()
            np.testing.assert_allclose(w, p["weights"], rtol=W_RTOL, atol=0)
            # the batch objects are the items added at the sampled leaves (leaf j <-> tree index j + capacity - 1)
            assert all(b is not None and b[1] % cap == i - (cap - 1) for b, i in zip(batches, idx))
            n_samples += 1
        else:
            m.update(p["indices"].tolist(), p["priorities"])
    assert n_samples > 0
    assert random.random() == float(z["final_next_random"])
    mp, size, write, tree = m.state()
    np.testing.assert_array_equal(tree, z["final_tree"])
    assert (mp, size, write) == (float(z["final_max_priority"]), int(z["final_size"]), int(z["final_write"]))
    assert m.length() == int(z["final_size"])
