"""The descending radix sort behind srlx_rank_select / srlx_rank_set (csrc/srlx_rank.hip) over the envelope it admits: every key population of
tests/rank_cases.py at the sizes that sit on the borders of the kernel's groups, wave chunks, tiles and scan rounds, with EVERY rank queried against
np.argsort(-p[:n_live], kind="stable") -- NaN last, -0.0 equal to +0.0, ties in index order (include/srlx.h) -- and compared exactly.  One handle
serves every case, so each select runs over ping-pong buffers some other size left behind, with priorities that would outrank the live ones parked in
the slots at and past n_live.  tests/test_rank_envelope_cpu.py shows that the NaN and signed-zero cases fail under the parent's key image."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rank_cases as C  # noqa: E402

from simple_distributed_rl_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = C.CAPACITY


class _DeviceWords:
    """`n` 32-bit words of device memory at `ptr` (torch.as_tensor reads __cuda_array_interface__)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<i4", data=(int(ptr), False), version=2)


class Handle:
    def __init__(self, capacity):
        self.lib, self.h, self.capacity = N.lib(), N.c_p(), capacity
        N.check(self.lib.srlx_rank_create(ctypes.byref(self.h), capacity, 0))
        p = N.c_p()
        N.check(self.lib.srlx_rank_priorities(self.h, ctypes.byref(p)))
        self.prio = torch.as_tensor(_DeviceWords(p.value, capacity), device="cuda")  # the handle's priority array, as bit patterns

    def bits(self):
        torch.cuda.synchronize()
        return self.prio.cpu().numpy().view(np.uint32)

    def set(self, values, start=0, idx=None):
        """srlx_rank_set's status for float32 `values`; add path at `start`, or update path at int64 `idx`."""
        d = torch.from_numpy(np.ascontiguousarray(values, np.float32)).cuda()
        di = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.int64)).cuda()
        status = self.lib.srlx_rank_set(self.h, len(values), N.tptr(di), N.tptr(d), start, None)
        torch.cuda.synchronize()
        return status

    def fill(self, p):
        """The live keys in slots [0, len(p)), rank_cases.poison in every slot behind them."""
        whole = np.concatenate([np.asarray(p, np.float32), C.poison(self.capacity - len(p))])
        N.check(self.set(whole))
        return whole

    def select_all(self, n_live):
        ranks = torch.arange(n_live, dtype=torch.int64, device="cuda")
        out = torch.full((n_live + 1,), -7, dtype=torch.int64, device="cuda")
        N.check(self.lib.srlx_rank_select(self.h, n_live, n_live, N.tptr(ranks), N.tptr(out), None))
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert out[n_live] == -7, "a store past the output"
        return out[:n_live]

    def close(self):
        self.lib.srlx_rank_destroy(self.h)


@pytest.fixture(scope="module")
def handle():
    h = Handle(CAP)
    yield h
    h.close()


def _check(got, p, what=""):
    want = C.yardstick(p)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        g, w = int(got[bad[0]]), int(want[bad[0]])
        g_bits = f"{int(C.bits(p)[g]):#010x}" if 0 <= g < len(p) else "outside the live slots"
        raise AssertionError(f"{what}: {len(bad)} of {len(p)} ranks differ from np.argsort(-p, kind='stable'); first at rank {bad[0]}: slot {g} ({g_bits}) "
                             f"for slot {w} ({int(C.bits(p)[w]):#010x})")


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_every_rank_matches_the_stable_numpy_order(handle, c):
    p = C.keys(c)
    whole = handle.fill(p)
    _check(handle.select_all(c.n), p, f"{c.population}-{c.n}")
    assert np.array_equal(handle.bits(), C.bits(whole)), "a select leaves the priorities alone"


def test_small_select_after_a_large_one_and_a_repeat(handle):
    """20481 live keys, then 65, 2 and 1 of the same array on the same handle: the ping-pong buffers and the histogram hold the larger sort's
    leftovers.  Each select twice: equal results."""
    p = C.keys(C.Case("nans", 20481))
    handle.fill(p)
    for n_live in (20481, 65, 2, 1, 4097, 20481):
        a = handle.select_all(n_live)
        b = handle.select_all(n_live)
        assert np.array_equal(a, b), n_live
        _check(a, p[:n_live], f"n_live {n_live}")


def test_a_sample_of_ranks_in_any_order(handle):
    """What the memory asks for: a few ranks, unsorted, with repeats; the first and the last rank among them."""
    p = C.keys(C.Case("zeros", 16385))
    handle.fill(p)
    ranks = np.concatenate([[16384, 0, 0, 16384], np.random.default_rng(1).integers(0, 16385, 253)])
    d = torch.from_numpy(ranks).cuda()
    out = torch.full((len(ranks) + 1,), -7, dtype=torch.int64, device="cuda")
    N.check(handle.lib.srlx_rank_select(handle.h, 16385, len(ranks), N.tptr(d), N.tptr(out), None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.append(C.yardstick(p)[ranks], -7))


# ---- srlx_rank_set ------------------------------------------------------------------------------------------------------------------------------------------------
def _values(n, seed):
    """Values whose bits must arrive untouched: ordinary floats, NaN payloads, -0.0, a denormal."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    odd = np.array(C.NAN_BITS + (0x80000000, C.TINY), np.int64).astype(np.uint32).view(np.float32)
    v[:: 3] = np.resize(odd, len(v[:: 3]))
    return v


@pytest.mark.parametrize("n,start", [(1, CAP - 1), (1, CAP), (1, 2 * CAP + 5), (255, CAP - 100), (256, CAP - 255), (257, CAP - 1), (257, 3 * CAP - 129), (CAP, 17)])
def test_add_path_wraps_the_ring(handle, n, start):
    mirror = handle.fill(C.keys(C.Case("distinct", 1025))).copy()
    v = _values(n, n + start)
    N.check(handle.set(v, start=start))
    mirror[(start + np.arange(n)) % CAP] = v
    assert n == 1 or n == CAP or (start % CAP) + n > CAP, "the write crosses the capacity"
    assert np.array_equal(handle.bits(), C.bits(mirror))


@pytest.mark.parametrize("n", [1, 257])
def test_update_path_writes_distinct_slots(handle, n):
    mirror = handle.fill(C.keys(C.Case("distinct", 1025))).copy()
    idx = np.random.default_rng(n).permutation(CAP)[:n]
    idx[0] = CAP - 1  # the last slot
    if n > 1:
        idx[1] = 0
    v = _values(n, n)
    N.check(handle.set(v, idx=idx))
    mirror[idx] = v
    assert len(np.unique(idx)) == n
    assert np.array_equal(handle.bits(), C.bits(mirror))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(handle):
    lib = handle.lib
    for capacity in (0, 1 << 31):
        h = N.c_p(0xDEAD)
        assert lib.srlx_rank_create(ctypes.byref(h), capacity, 0) != N.OK and not h.value, capacity
    whole = handle.fill(C.keys(C.Case("distinct", 4097)))
    ranks = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -7, dtype=torch.int64, device="cuda")
    for n_live, n in ((0, 8), (CAP + 1, 8), (-1, 8), (4097, 0), (4097, -1)):
        assert lib.srlx_rank_select(handle.h, n_live, n, N.tptr(ranks), N.tptr(out), None) != N.OK, (n_live, n)
    assert lib.srlx_rank_select(handle.h, 4097, 8, None, N.tptr(out), None) != N.OK
    assert lib.srlx_rank_select(handle.h, 4097, 8, N.tptr(ranks), None, None) != N.OK
    v = torch.full((CAP + 1,), 123.0, dtype=torch.float32, device="cuda")
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.srlx_rank_set(handle.h, 0, None, N.tptr(v), 0, None) != N.OK
    assert lib.srlx_rank_set(handle.h, 0, N.tptr(idx), N.tptr(v), 0, None) != N.OK
    assert lib.srlx_rank_set(handle.h, 8, None, N.tptr(v), -1, None) != N.OK
    assert lib.srlx_rank_set(handle.h, 8, None, None, 0, None) != N.OK
    assert lib.srlx_rank_set(handle.h, CAP + 1, None, N.tptr(v), 0, None) != N.OK, "an add of more than the capacity: two threads would write one slot"
    with pytest.raises(N.SrlxError):
        N.check(lib.srlx_rank_set(handle.h, CAP + 1, None, N.tptr(v), 0, None))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    assert np.array_equal(handle.bits(), C.bits(whole))
    N.check(lib.srlx_rank_set(handle.h, CAP, None, N.tptr(v), 0, None))  # exactly the capacity is an add of every slot
    assert (handle.bits() == C.bits(np.float32(123.0))).all()


# ---- through the class --------------------------------------------------------------------------------------------------------------------------------------------
def test_memory_with_unprioritised_adds_samples_like_the_reference():
    """RankBasedMemory.add(item, None) stores NaN (every non-distributed R2D2 / Agent57 / Rainbow worker adds that way) between adds with a priority;
    sample() under a numpy seed against oracle/hot_path_oracle.py: rankbased_sample on the same live priorities under the same seed.  Equal weights;
    equal indices at the ranks below the finite count; at the ranks at or past it exactly the NaN slots the stable order names (numpy's default sort
    leaves the order inside the NaN tail unspecified, so there the oracle's `order` is no reference)."""
    import hot_path_oracle as H
    from simple_distributed_rl_amd.rl.memories.priority_memories.rankbased_memory import RankBasedMemory

    cap, n_add, B, alpha, beta0, steps = 3000, 2600, 64, 0.6, 0.4, 1000
    rng = np.random.default_rng(7)
    mem = RankBasedMemory(cap, alpha, beta0, steps)
    finite = rng.permutation(n_add).astype(np.float32) / 7 - 100  # distinct, both signs
    none = rng.random(n_add) < 0.27
    none[:2] = (True, False)
    for k in range(n_add):
        mem.add(k, None if none[k] else float(finite[k]))
    live = np.where(none, np.float32(np.nan), finite).astype(np.float32)
    assert np.array_equal(C.bits(mem.priorities[:n_add]), C.bits(live))
    n_finite = int((~none).sum())
    stable = C.yardstick(live)
    assert np.array_equal(np.sort(stable[n_finite:]), np.flatnonzero(none)) and np.array_equal(stable[n_finite:], np.flatnonzero(none))
    tail_drawn = 0
    for rnd, step in enumerate((0, 400, 5000)):
        np.random.seed(100 + rnd)
        batches, weights, idx = mem.sample(B, step)
        np.random.seed(100 + rnd)
        want_idx, want_w = H.rankbased_sample(live, B, alpha, min(1, beta0 + (1 - beta0) * step / steps))
        np.random.seed(100 + rnd)
        probs = (1 / np.arange(1, n_add + 1)) ** alpha
        ranks = np.random.choice(n_add, size=B, p=probs / probs.sum(), replace=False)  # the draw both sides made
        assert np.array_equal(weights, want_w)
        head = ranks < n_finite
        assert np.array_equal(np.asarray(idx)[head], want_idx[head])
        assert np.array_equal(np.asarray(idx), stable[ranks]), "every drawn rank, the NaN tail in index order"
        assert none[np.asarray(idx)[~head]].all() and not none[np.asarray(idx)[head]].any()
        assert batches == [int(i) for i in idx]
        tail_drawn += int((~head).sum())
    assert tail_drawn > 0, "the draws reach the NaN tail"
