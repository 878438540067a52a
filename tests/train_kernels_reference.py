"""Shared by tests/test_train_kernels_cpu.py, tests/test_train_kernels_gpu.py and tests/test_ngu_envelope_gpu.py: the cases, the guarded device buffers and
the comparison helpers for the kernels of csrc/srlx_train.hip (n-step TD dense and packed, 1-step DQN target, GAE scan, multi-tensor Adam) and the three entry
points of csrc/srlx_ngu.hip that tests/test_agent57_kernels_gpu.py leaves out (episodic memory, lifelong reward, srlx_agent57_seq_td).

The yardsticks are the functions of oracle/hot_path_oracle.py (pinned to the reference by tests/test_hot_path_oracle_golden.py); nothing here restates one of
them, except `nstep_target_in_kernel_order`, which restates the KERNEL's order of operations in float32 numpy so that the CPU module can show, without a GPU,
that this order is the oracle's at every n and that the order it replaced was not.  Every condition a case builder promises is asserted on the oracle alone in
tests/test_train_kernels_cpu.py."""
import ctypes
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import hot_path_oracle as H  # noqa: E402
from agent57_kernels_reference import F32, I32, U8  # noqa: E402

I64, F64 = np.int64, np.float64
GUARD = 64
SENTINEL = {"f": -12345.0, "i": -777, "u": 0xA5}
RTOL = 1e-5  # the project's bar (tests/test_hot_path_gpu.py, tests/test_agent57_gpu.py)


# ---- device buffers --------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """A device array with GUARD sentinel elements behind it (as in tests/test_agent57_kernels_gpu.py); get() synchronises, checks the guard and returns the
    host copy.  Without `init` the array itself is sentinels too, so `untouched()` shows that a refused call wrote nothing."""

    def __init__(self, shape, dtype=F32, init=None):
        import torch

        self.shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(shape)
        self.n, self.dt = int(np.prod(self.shape)), np.dtype(dtype)
        self.sentinel = SENTINEL[self.dt.kind]
        host = np.full(self.n + GUARD, self.sentinel, self.dt)
        if init is not None:
            host[:self.n] = np.asarray(init, self.dt).reshape(-1)
        self.t = torch.from_numpy(host).to("cuda:0")

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.t.data_ptr() + offset * self.dt.itemsize)

    def get(self):
        import torch

        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[self.n:] == self.sentinel).all(), "a kernel wrote behind the end of a buffer"
        return h[:self.n].reshape(self.shape).copy()

    def untouched(self):
        return bool((self.get() == self.sentinel).all())


def D(a):
    """A read-only input on the device (None stays None)."""
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=what)


def bit_equal_share(got, want):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return float(np.mean(got.view(np.uint32) == want.view(np.uint32)))


def refused(N, lib, status, text):
    """The entry point returned ERR_INVALID (so it launched nothing) and its message names the reason."""
    assert status == N.ERR_INVALID, status
    msg = lib.srlx_last_error().decode("utf-8", "replace")
    assert text in msg, msg


def bar_fraction(got, want, rtol, atol=0.0):
    """The worst |got - want| as a fraction of the bar atol + rtol |want| (what np.testing.assert_allclose allows); entries that are the same infinity or both
    NaN count as 0, as they do there."""
    got, want = np.asarray(got, F64).reshape(-1), np.asarray(want, F64).reshape(-1)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(got - want) / (atol + rtol * np.abs(want))
    frac = np.where(same, 0.0, frac)
    return float(np.nan_to_num(frac, nan=np.inf).max()) if frac.size else 0.0


def check(name, got, want, rtol, atol=0.0, want64=None, where=""):
    """assert_allclose against the float32 yardstick, after printing the distance as a fraction of the bar -- and, where a float64 run of the same yardstick
    exists, the float32 yardstick's own distance from it: a case in which that second figure is large is ill-conditioned, not a finding about the kernel."""
    line = "ENVELOPE %s %s: kernel vs float32 yardstick %.3g of the bar (rtol %g atol %g)" % (where, name, bar_fraction(got, want, rtol, atol), rtol, atol)
    if want64 is not None:
        line += "; kernel vs float64 %.3g; float32 yardstick vs float64 %.3g" % (bar_fraction(got, want64, rtol, atol), bar_fraction(want, want64, rtol, atol))
    print(line)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=f"{where} {name}")


class _Float64Numpy:
    """numpy with float32 spelled float64, for `in_float64`."""
    float32 = np.float64

    def __getattr__(self, name):
        return getattr(np, name)


def in_float64(fn, *args):
    """A yardstick of oracle/hot_path_oracle.py that has no np_dtype argument, run in float64: the SAME function, evaluated while the module's `np.float32` reads
    np.float64 -- every cast it makes and every array it builds is float64 then.  Printed next to the float32 distance, never asserted against."""
    saved = H.np
    H.np = _Float64Numpy()
    try:
        with np.errstate(invalid="ignore"):
            out = fn(*args)
    finally:
        H.np = saved
    assert out.dtype == F64, out.dtype
    return out


# ---- thinning a cross product ----------------------------------------------------------------------------------------------------------------------------------
def pairwise_cover(axes, allowed=lambda c: True):
    """A subset of the cross product of `axes` (name -> values) in which every value of every axis meets every value of every other axis at least once, among
    the combinations `allowed` admits.  Greedy and deterministic: always the first combination that covers the most pairs still missing."""
    names = list(axes)
    combos = [dict(zip(names, v)) for v in itertools.product(*axes.values())]
    combos = [c for c in combos if allowed(c)]
    pairs_of = [frozenset(((a, repr(c[a])), (b, repr(c[b]))) for a, b in itertools.combinations(names, 2)) for c in combos]
    missing = set().union(*pairs_of)
    out = []
    while missing:
        gain = [len(p & missing) for p in pairs_of]
        i = int(np.argmax(gain))
        out.append(combos[i])
        missing -= pairs_of[i]
    return out


def all_pairs(axes, allowed=lambda c: True):
    names = list(axes)
    combos = [dict(zip(names, v)) for v in itertools.product(*axes.values()) if allowed(dict(zip(names, v)))]
    return set().union(*[frozenset(((a, repr(c[a])), (b, repr(c[b]))) for a, b in itertools.combinations(names, 2)) for c in combos])


def case_id(c):
    return "-".join(f"{k}{'x'.join(str(x) for x in v) if isinstance(v, tuple) else v}" for k, v in c.items())


def quantised(rng, shape):
    """Q values on the grid of multiples of 0.25 in [-2, 2]: exact in float32, and equal values are common."""
    return (rng.integers(-8, 9, shape) * 0.25).astype(F32)


def tie_rows(q, invalid, rng):
    """Makes the maximum over the valid actions of two rows in three occur twice (A >= 2 and two valid actions given); changes q in place, rows = all but the
    last axis."""
    A = q.shape[-1]
    flat = np.ascontiguousarray(q).reshape(-1, A)
    inv = np.zeros(flat.shape, bool) if invalid is None else np.asarray(invalid, bool).reshape(-1, A)
    for i in range(len(flat)):
        valid = np.nonzero(~inv[i])[0]
        if i % 3 == 2 or len(valid) < 2:
            continue
        j = rng.choice(valid, 2, replace=False)
        flat[i, j] = flat[i, valid].max()  # both are now the maximum; the first of them must win
    q[...] = flat.reshape(q.shape)  # (q may be a view)


def tied(q, invalid):
    """Per row: does the maximum over the valid actions (all actions where none is valid, every value then being -inf) occur more than once?"""
    A = q.shape[-1]
    v = np.array(q, F32).reshape(-1, A)
    if invalid is not None:
        v[np.asarray(invalid, bool).reshape(-1, A)] = -np.inf
    return (v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1


# ---- 1. n-step TD ----------------------------------------------------------------------------------------------------------------------------------------------
NSTEP_AXES = dict(B=(1, 255, 256, 257), n=(1, 2, 7, 8, 9, 32), A=(1, 2, 18), dd=(1, 0), rs=(0, 1), mask=(0, 1), dh=((0.99, 0.95), (1.0, 1.0), (0.0, 0.0)))
NSTEP_CASES = pairwise_cover(NSTEP_AXES)
# without rescale the target must be the float32 oracle's bits at every n; these shapes make sure of every n at a full batch, double DQN on and off
NSTEP_ORDER_CASES = [dict(B=257, n=n, A=4, dd=dd, rs=0, mask=n % 2, dh=(0.99, 1.0)) for n in NSTEP_AXES["n"] for dd in (1, 0)]
# mask given and double DQN off WITHOUT the all-invalid step ("whole" 0): in every other case of that pair row 0's target is -inf or NaN, and the batch's
# loss with it on both sides -- here the loss is a number and is compared
NSTEP_FINITE_CASES = [dict(B=257, n=9, A=18, dd=0, rs=rs, mask=1, dh=(0.99, 0.95), whole=0) for rs in (0, 1)]


def nstep_greedy(c, q_on, q_tg, inv):
    """The greedy next action of every step, the way both the oracle and the kernel choose it: the first maximum of the masked selecting net."""
    sel = np.array(q_on if c["dd"] else q_tg, F32)
    if inv is not None:
        sel[inv] = -np.inf
    return np.argmax(sel, axis=2)


def nstep_oracle(c, d, np_dtype=F32):
    discount, h = c["dh"]
    n = c["n"]
    with np.errstate(invalid="ignore"):  # an all-invalid step without double DQN: -inf times a 0 there as in the reference
        return H.nstep_target(d["q_on"] if c["dd"] else d["q_on"][:, : n - 1], d["q_tg"], d["act"], d["rew"], d["done"], d["inv"], discount, h, bool(c["dd"]),
                              bool(c["rs"]), np_dtype=np_dtype)


def nstep_case(c, seed=0):
    """Inputs of one n-step TD case.  What they promise (asserted in the CPU module; each where the shape leaves room for it):
      ties      A >= 2: the masked maximum of the selecting net is repeated in at least a third of the B n argmax rows;
      masks     mask given: row 0 has every action of step 0 invalid (so action 0 too), every other step of the batch keeps a valid action; from B >= 2 row 1 has only action 0 of its last step invalid;
      cuts      A >= 2 and B >= n: row m (m = 1..n-1) takes its first off-greedy action exactly at step m, row 0 is greedy throughout;
      ends      n >= 2 and B >= 2: the last row terminates at step 0, others at random steps;
      weights   B >= 2: row 0 weighs 0, row 1 weighs 1.5;
      Huber     B >= 255: at least a quarter of the rows in each of |diff| < 1, diff > 1, diff < -1 (diff = target w - q0 w), set through q0's taken entry."""
    B, n, A = c["B"], c["n"], c["A"]
    rng = np.random.default_rng([seed, B, n, A, c["dd"], c["rs"], c["mask"]])
    inv = None
    if c["mask"]:
        inv = rng.random((B, n, A)) < 0.15
        inv[np.arange(B)[:, None], np.arange(n)[None, :], rng.integers(0, A, (B, n))] = False  # a valid action everywhere ...
        if c.get("whole", 1):
            inv[0, 0, :] = True  # ... but here
        if B >= 2:
            inv[1, n - 1, :] = False
            inv[1, n - 1, 0] = True
    q_on, q_tg = quantised(rng, (B, n, A)), quantised(rng, (B, n, A))
    if A >= 2:
        tie_rows(q_on, inv, rng)
        tie_rows(q_tg, inv, rng)
    greedy = nstep_greedy(c, q_on, q_tg, inv)
    act = np.where(rng.random((B, n)) < 0.8, greedy, rng.integers(0, A, (B, n))).astype(I32)
    act[:, 0] = rng.integers(0, A, B)
    for m in range(min(B, n)):  # row 0 greedy throughout; row m leaves the greedy policy at step m and not before
        act[m, 1:] = greedy[m, 1:]
        if m >= 1 and A >= 2:
            act[m, m] = (greedy[m, m] + 1) % A
    rew = rng.standard_normal((B, n)).astype(F32)
    done = (rng.random((B, n)) < 0.1).astype(F32)
    if n >= 2 and B >= 2:
        done[B - 1, 0] = 1.0
    w = (rng.random(B) * 1.5).astype(F32)
    if B >= 2:
        w[0], w[1] = 0.0, 1.5
    d = dict(q_on=q_on, q_tg=q_tg, act=act, rew=rew, done=done, inv=inv, w=w)
    target = nstep_oracle(c, d).astype(F64)
    # q0's taken entry puts target w - q0 w into the three regions of the Huber loss in turn; the other entries are free
    delta = np.choose(np.arange(B) % 3, [rng.uniform(-0.9, 0.9, B), rng.uniform(1.5, 3.0, B), rng.uniform(-3.0, -1.5, B)])
    q0 = rng.standard_normal((B, A)).astype(F32)
    ok = np.isfinite(target) & (w > 0.05)
    q0[np.arange(B)[ok], act[ok, 0]] = (target[ok] - delta[ok] / w[ok].astype(F64)).astype(F32)
    d["q0"] = q0
    return d


def first_cut(c, d):
    """Per row: the first step m >= 1 whose action is not the greedy one (n: greedy throughout)."""
    if c["n"] == 1:
        return np.ones(c["B"], np.int64)
    off = d["act"][:, 1:] != nstep_greedy(c, d["q_on"], d["q_tg"], d["inv"])[:, 1:]
    return np.where(off.any(axis=1), off.argmax(axis=1) + 1, c["n"])


def pack_q(d):
    """The online net's rows as the packed entry point reads them: [B][n+1][A], row 0 = the state the action was taken in."""
    return np.ascontiguousarray(np.concatenate([d["q0"][:, None, :], d["q_on"]], axis=1))


def np_pairwise_f32(x):
    """numpy's float32 pairwise sum of up to 128 terms written out (numpy/_core/src/umath/loops_utils.h.src), rows of a [B][n] array."""
    x = np.asarray(x, F32)
    n = x.shape[1]
    assert n <= 128
    if n < 8:
        acc = np.zeros(len(x), F32)
        for i in range(n):
            acc = acc + x[:, i]
        return acc
    r = [x[:, j].copy() for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + x[:, i + j]
        i += 8
    acc = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(i, n):
        acc = acc + x[:, k]
    return acc


def nstep_target_in_kernel_order(c, d, pairwise=True):
    """csrc/srlx_td_math.h:td_rows restated in float32 numpy, operation by operation (pairwise=False: every n added one term after another, the order the
    kernel had before it followed numpy's from 8 terms up).  For the CPU module only -- the GPU tests compare with the oracle."""
    discount, h = c["dh"]
    B, n, A = c["B"], c["n"], c["A"]
    greedy = nstep_greedy(c, d["q_on"], d["q_tg"], d["inv"])
    rows = np.arange(B)
    disc_f = F32(discount)
    terms = np.zeros((B, n), F32)
    coef = np.ones(B, F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(n):
            maxq = d["q_tg"][rows, m, greedy[:, m]].astype(F32)
            if not c["dd"] and d["inv"] is not None:
                maxq = np.where(d["inv"][rows, m, greedy[:, m]], F32(-np.inf), maxq)
            if c["rs"]:
                maxq = H.inverse_rescaling(maxq).astype(F32)
            gain = d["rew"][:, m] + ((F32(1) - d["done"][:, m]) * disc_f) * maxq
            if c["rs"]:
                gain = H.rescaling(gain).astype(F32)
            qsel = np.zeros(B, F32) if m == 0 else d["q_on"][rows, m - 1, d["act"][:, m]]
            if m > 0:
                coef = coef * (h * (d["act"][:, m] == greedy[:, m]).astype(F64))
            terms[:, m] = (((gain - qsel) * F32(discount ** m)).astype(F64) * coef).astype(F32)
        if pairwise:
            return np_pairwise_f32(terms)
        acc = np.zeros(B, F32)
        for m in range(n):
            acc = acc + terms[:, m]
        return acc


# ---- 2. the 1-step DQN target ----------------------------------------------------------------------------------------------------------------------------------
DQN_AXES = dict(B=(1, 255, 256, 257, 1000), A=(1, 2, 18), dd=(1, 0), rs=(0, 1), f64=(0, 1), ps=(0, 1), mask=("none", "some", "rows"))


def _dqn_allowed(c):
    return not (c["f64"] and c["ps"])  # refused by the entry point (asserted on its own)


DQN_CASES = pairwise_cover(DQN_AXES, _dqn_allowed)


def dqn_case(c, seed=0, min_masked=False):
    """Inputs of one srlx_dqn_target case.  The masked net (online with double DQN, else target) has one entry below every other, -3, in the LAST row, which
    has no invalid action from B >= 2 (`min_masked`: that entry is itself invalid, so it is replaced by its own value); the rows it decides are others.
    mask "some": a third of the entries, never a whole row -- the replacement must lose every argmax; "rows": as "some", and every fifth row (row 0 included)
    wholly invalid -- without double DQN the target of such a row is made of the minimum itself, with double DQN of the target net's entry 0."""
    B, A = c["B"], c["A"]
    rng = np.random.default_rng([seed, B, A, c["dd"], c["rs"], c["f64"], c["ps"], len(c["mask"])])
    q_on, q_tg = quantised(rng, (B, A)), quantised(rng, (B, A))
    if A >= 2:
        tie_rows(q_on, None, rng)
        tie_rows(q_tg, None, rng)
    masked_net = q_on if c["dd"] else q_tg
    inv = None
    if c["mask"] != "none":
        inv = rng.random((B, A)) < 1 / 3
        inv[np.arange(B), rng.integers(0, A, B)] = False
        if c["mask"] == "rows":
            inv[0::5] = True
        if B >= 2:
            inv[B - 1] = False
    masked_net[B - 1, A - 1] = -3.0
    if min_masked:
        assert inv is not None
        inv[B - 1, A - 1] = True
    return dict(q_on=q_on, q_tg=q_tg, inv=inv, rew=rng.standard_normal(B).astype(F32), undone=(rng.random(B) < 0.8).astype(F32), discount=0.997,
                disc_ps=(0.9 + 0.099 * rng.random(B)).astype(F32) if c["ps"] else None)


def dqn_oracle(c, d, f64=False):
    if f64:  # the same two functions with every float32 read as float64 (f64_accum's integer `undone` stays what it is)
        if c["ps"]:
            return in_float64(H.agent57_target, d["q_on"], d["q_tg"], d["rew"], d["undone"], d["disc_ps"], d["inv"], bool(c["dd"]), bool(c["rs"]))
        return in_float64(H.dqn_target, d["q_on"], d["q_tg"], d["rew"], d["undone"], d["inv"], d["discount"], bool(c["dd"]), bool(c["rs"]), bool(c["f64"]))
    if c["ps"]:
        return H.agent57_target(d["q_on"], d["q_tg"], d["rew"], d["undone"], d["disc_ps"], d["inv"], bool(c["dd"]), bool(c["rs"]))
    return H.dqn_target(d["q_on"], d["q_tg"], d["rew"], d["undone"], d["inv"], d["discount"], bool(c["dd"]), bool(c["rs"]), bool(c["f64"]))


# ---- 3. GAE ----------------------------------------------------------------------------------------------------------------------------------------------------
GAE_AXES = dict(E=(1, 255, 256, 257), T=(1, 2, 33), boot=(1, 0), done=("none", "all", "last", "some"), gl=((0.9, 0.95), (1.0, 1.0), (0.99, 0.0)))
GAE_CASES = pairwise_cover(GAE_AXES)


def gae_case(c, seed=0):
    """done "last": every environment ends on the last step -- with bootstrap values present these must be ignored; "some": one step in ten."""
    E, T = c["E"], c["T"]
    rng = np.random.default_rng([seed, E, T, c["boot"], len(c["done"])])
    done = np.zeros((T, E), U8)
    if c["done"] == "all":
        done[:] = 1
    elif c["done"] == "last":
        done[T - 1] = 1
    elif c["done"] == "some":
        done = (rng.random((T, E)) < 0.1).astype(U8)
    return dict(rew=rng.standard_normal((T, E)).astype(F32), val=rng.standard_normal((T, E)).astype(F32), done=done,
                last=(10.0 + rng.standard_normal(E)).astype(F32) if c["boot"] else None)


# ---- 5. srlx_agent57_seq_td ------------------------------------------------------------------------------------------------------------------------------------
SEQ_AXES = dict(B=(1, 255, 256, 257, 513), S=(1, 2, 80), A=(1, 2, 18), dd=(1, 0), rs=(0, 1), mask=(0, 1))
SEQ_CASES = pairwise_cover(SEQ_AXES)
SEQ_FINITE_CASES = [dict(B=257, S=80, A=18, dd=0, rs=rs, mask=1, whole=0) for rs in (0, 1)]  # as NSTEP_FINITE_CASES: a finite loss with mask given, double DQN off


def seq_case(c, seed=0):
    """As tests/test_agent57_gpu.py's Atari-shape case at any shape: about 70 % of the actions greedy, `dones` 0 at about 3 % of the steps (and at step 0 of
    the last row), quantised Q values with ties; mask given and double DQN off: row 0 has every action of its last step invalid."""
    B, S, A = c["B"], c["S"], c["A"]
    rng = np.random.default_rng([seed, B, S, A, c["dd"], c["rs"], c["mask"]])
    q = quantised(rng, (B, S + 1, A))
    qt = (q + quantised(rng, (B, S + 1, A)) * F32(0.25)).astype(F32)
    inv = None
    if c["mask"]:
        inv = rng.random((B, S, A)) < 0.15
        inv[np.arange(B)[:, None], np.arange(S)[None, :], rng.integers(0, A, (B, S))] = False  # a valid action everywhere ...
        if not c["dd"]:
            inv[0, S - 1, :] = c.get("whole", 1) == 1  # ... but here
    if A >= 2:
        tie_rows(q[:, 1:], inv, rng)
        tie_rows(qt[:, 1:], inv, rng)
    sel = np.array(q[:, 1:] if c["dd"] else qt[:, 1:], F32)
    if inv is not None:
        sel[inv] = -np.inf
    greedy = np.argmax(sel, axis=2)
    act = np.where(rng.random((B, S)) < 0.7, greedy, rng.integers(0, A, (B, S))).astype(I32)
    dones = (rng.random((B, S)) < 0.97).astype(F32)
    dones[B - 1, 0] = 0.0
    return dict(q=q, qt=qt, act=act, rew=rng.standard_normal((B, S)).astype(F32), dones=dones, inv=inv, disc=(0.99 + 0.009 * rng.random(B)).astype(F32),
                w=(rng.random(B) * 1.5).astype(F32), greedy=greedy)


# ---- 6. lifelong reward ----------------------------------------------------------------------------------------------------------------------------------------
LIFELONG_N = (1, 255, 256, 257)
LIFELONG_D = (1, 7, 8, 9, 128, 129, 1000)  # the block edges of numpy's pairwise sum
LIFELONG_MAX = 5.0


def lifelong_case(n, Dm, seed=0):
    """Rows in turn: error 0 exactly (clips at 1 from below: 1 + 0), a small error, and an error beyond lifelong_max - 1 (clips at lifelong_max)."""
    rng = np.random.default_rng([seed, n, Dm])
    target = rng.standard_normal((n, Dm)).astype(F32)
    scale = np.choose(np.arange(n) % 3, [0.0, 0.5, 4.0]).astype(F32)
    train = (target + scale[:, None] * (1.0 + rng.random((n, Dm)))).astype(F32)
    return target, train


# ---- 7. episodic memory ----------------------------------------------------------------------------------------------------------------------------------------
NGU_CONSTANTS = (0.001, 0.008, 0.1)  # epsilon, cluster_distance, pseudo_counts: the defaults
EPISODIC_CASES = dict(
    a=dict(E=1, lanes=(0,), cap=1024, k=3, D=2, T=1300, split=1),    # up to 4 entries per thread, 276 overwrites of the ring
    b=dict(E=1024, lanes=(0, 511, 1023), cap=4352, k=10, D=2, T=4700, split=1),  # 17 entries per thread: the list overflows; the ring wraps
    c=dict(E=1, lanes=(0,), cap=2100, k=16, D=3, T=2400, split=3),   # k at its maximum, three candidate lists merged, ring wrap under split > 1
    d=dict(E=1, lanes=(0,), cap=15400, k=10, D=4, T=4400, split=16),  # the stride loop's second round from 4097 live entries
    e1=dict(E=1, lanes=(0,), cap=300, k=10, D=1, T=40, split=1),
    e256=dict(E=1, lanes=(0,), cap=300, k=10, D=256, T=40, split=1),
    f=dict(E=1, lanes=(0,), cap=2100, k=10, D=3, T=600, split=3, points=5),  # exact zero distances, ave == 0, ties across threads and parts
    g=dict(E=1, lanes=(0,), cap=2100, k=10, D=3, T=1000, split=3, reset_at=700),
    # not uniform: every 256th embedding of the active lane lies in [0.5, 0.51), the others in [2, 3) -- with a ring of 17 x 256 slots the near ones all belong
    # to ONE thread, so the 16 nearest of a near query fill that thread's 16-slot list to its last slot and the 17th is turned away by the rejection test
    # (uniform data never needs more than a few slots of any one thread)
    h=dict(E=1024, lanes=(700,), cap=4352, k=16, D=1, T=9000, split=1, near_every=256),
)


def ngu_split(E, cap):
    """srlx_ngu_create's workgroups per environment."""
    return int(min(max(min(-(-cap // 1024), -(-1024 // E)), 1), 16))


def episodic_embeddings(name):
    """float32 [T][E][D], uniform in [0, 1)^D (case f: each drawn from 5 fixed points)."""
    c = EPISODIC_CASES[name]
    rng = np.random.default_rng([7, sorted(EPISODIC_CASES).index(name)])
    if "points" in c:
        pts = rng.random((c["points"], c["D"])).astype(F32)
        return pts[rng.integers(0, c["points"], (c["T"], c["E"]))]
    emb = rng.random((c["T"], c["E"], c["D"])).astype(F32)
    if "near_every" in c:
        near = np.arange(c["T"]) % c["near_every"] == 5
        for lane in c["lanes"]:
            emb[:, lane, 0] = np.where(near, F32(0.5) + F32(0.01) * emb[:, lane, 0], F32(2.0) + emb[:, lane, 0])
    return emb


class RingEpisodicOracle(H.EpisodicMemoryOracle):
    """EpisodicMemoryOracle.step(exact_dot=False) with the bounded deque kept as rows of one array instead of a Python list of arrays: the same distance
    expression on the same live entries and the same `ngu_episodic_from_distances`, so the same bits (the k nearest are taken after a sort: the order of the
    entries does not matter) -- tests/test_train_kernels_cpu.py holds it to its parent step by step, ring wraps and a reset included.  The parent stacks
    its list on every step, 1 ms at 4000 entries: 15 s for case b, against 2 s here."""

    def __init__(self, capacity, dim, *a):
        super().__init__(capacity, *a)
        self.ring, self.count = np.zeros((capacity, dim), F32), 0

    def reset(self):
        self.count = 0

    def step(self, emb, exact_dot=False):
        assert not exact_dot
        emb = np.asarray(emb, F32)
        live = min(self.count, self.capacity)
        diff = self.ring[:live] - emb
        self.ring[self.count % self.capacity] = emb
        self.count += 1
        if live == 0:
            return F32(1 / self.c)
        dist = np.sqrt(np.einsum("ij,ij->i", diff, diff)).astype(F32)
        return H.ngu_episodic_from_distances(dist, self.k, self.epsilon, self.cluster_distance, self.c)


def episodic_expected(name, emb, oracle=RingEpisodicOracle):
    """The rewards of the active lanes, [T][len(lanes)], from one oracle memory per lane, stepped with exact_dot=False."""
    c = EPISODIC_CASES[name]
    out = np.zeros((c["T"], len(c["lanes"])), F32)
    for j, lane in enumerate(c["lanes"]):
        mem = H.EpisodicMemoryOracle(c["cap"], c["k"], *NGU_CONSTANTS) if oracle is H.EpisodicMemoryOracle else oracle(c["cap"], c["D"], c["k"], *NGU_CONSTANTS)
        for t in range(c["T"]):
            if t == c.get("reset_at", -1):
                mem.reset()
            out[t, j] = mem.step(emb[t, lane], exact_dot=False)
    return out


def knn_sensitivity(name, emb, lane=0, every=7, move=1e-4):
    """On the oracle alone: at every `every`-th step with more than k live entries, does the reward move by at least `move` (relative) when any one of the k
    nearest neighbours is dropped and the (k+1)-th moves up -- which covers the nearest dropped (j = 0) and the k-th replaced by the (k+1)-th (j = k-1)?
    Returns (steps that pass, steps checked)."""
    c = EPISODIC_CASES[name]
    eps, cl, pc = NGU_CONSTANTS
    k, cap = c["k"], c["cap"]
    x = emb[:, lane]
    passed = checked = 0
    for t in range(0, c["T"], every):
        lo = max(0, t - cap)
        if t - lo <= k:
            continue
        diff = x[lo:t] - x[t]
        near = np.sort(np.sqrt(np.einsum("ij,ij->i", diff, diff)).astype(F32))[: k + 1]
        base = float(H.ngu_episodic_from_distances(near[:k], k, eps, cl, pc))
        moved = [abs(float(H.ngu_episodic_from_distances(np.delete(near, j), k, eps, cl, pc)) - base) / base for j in range(k)]
        checked += 1
        passed += min(moved) >= move
    return passed, checked
