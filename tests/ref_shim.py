"""A reference model of the ProportionalMemory shim (test infrastructure).

`RefShim` is what the reference's ProportionalMemory (proportional_memory.py:95-205) does under
Python's `random`: the C restatement of its sum-tree (OraclePER, oracle/per_oracle.c) plus a host
list that mirrors the data ring.  It shares no code with the shim: priorities are transformed on
the host with the expressions the shim documents as the reference's (:124 for `add`, :172 for
`update`), and `sample` draws one `random.random()` per descent attempt (:146-158), leaving the
generator where the reference would.  tests/test_ref_shim_model.py replays the reference's own
golden traces through it; tests/test_per_shim_edges_gpu.py runs it side by side with the shim.
"""
import math
import random
from array import array

import numpy as np

from oracle_bindings import ADD_NONE, ADD_RAW, OraclePER

W_RTOL = 1e-13
NO_DUP_UNIFORM_CAP = 8192  # the shim walks at most this many uniforms per call when has_duplicate=False


class RefShim:
    def __init__(self, capacity, alpha=0.6, beta_initial=0.4, beta_steps=1_000_000, has_duplicate=True, epsilon=0.0001, host_transform=True):
        # host_transform=False: the kernel transforms, and only alpha = 0.5 (a correctly rounded sqrt on both sides) is bit-exact by construction
        assert host_transform or alpha == 0.5, "host_transform=False is modelled at alpha = 0.5 only"
        self.capacity = int(capacity)
        self.alpha = alpha
        self.epsilon = epsilon
        self.has_duplicate = bool(has_duplicate)
        self.host_transform = host_transform
        self.oracle = OraclePER(self.capacity, alpha, beta_initial, beta_steps, has_duplicate, epsilon)
        self.data = [None] * self.capacity
        self._write = 0

    def length(self):
        return self.oracle.length()

    def add(self, batch, priority=None):
        self.data[self._write] = batch
        self._write = (self._write + 1) % self.capacity
        if priority is None:
            self.oracle.add(None, mode=ADD_NONE)
            return
        p = float(priority)
        if self.host_transform:
            self.oracle.add((abs(p) + self.epsilon) ** self.alpha, mode=ADD_RAW)
        else:
            self.oracle.add(math.sqrt(abs(p) + self.epsilon), mode=ADD_RAW)

    def update(self, indices, priorities):
        idx = np.asarray(indices, np.int64)
        if self.host_transform:
            pr = np.frombuffer(array("d", priorities), np.float64) if type(priorities) is list else np.asarray(priorities)
            tx = np.ascontiguousarray((np.abs(pr) + self.epsilon) ** self.alpha, dtype=np.float64)
            self.oracle.update(idx, tx[: idx.size], raw=True)
        else:
            pr = np.asarray(priorities)
            if pr.dtype != np.float32:
                pr = pr.astype(np.float64)
            self.oracle.update(idx, pr[: idx.size])

    def sample(self, batch_size, step):
        """(batches, float64 weights, list of tree indices); `random` ends where the reference's would."""
        s0 = random.getstate()
        n = batch_size + 64
        while True:
            random.setstate(s0)
            u = [random.random() for _ in range(n)]
            used, idx, w, _ = self.oracle.sample(batch_size, step, u)
            if used >= 0:
                break
            n *= 2
        if not self.has_duplicate:
            assert used < NO_DUP_UNIFORM_CAP, f"the script left the regime the model covers: {used} uniforms for a batch of {batch_size}"
        random.setstate(s0)
        for _ in range(used):
            random.random()
        return [self.data[i - (self.capacity - 1)] for i in idx.tolist()], w, idx.tolist()

    def state(self):
        """(max_priority, size, write, tree) as backup() lays them out."""
        return self.oracle.get_state()
