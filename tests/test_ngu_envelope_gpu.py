"""The three entry points of csrc/srlx_ngu.hip that tests/test_agent57_kernels_gpu.py leaves out, over the envelope they admit, through the C ABI:
srlx_agent57_seq_td against hot_path_oracle.agent57_seq_target / agent57_seq_loss, srlx_ngu_lifelong_reward bit for bit against the oracle at the block edges
of numpy's pairwise sum, and the episodic k-nearest-neighbour memory step by step against EpisodicMemoryOracle at the sizes where a thread holds several
entries, its 16-slot list overflows, several workgroups' candidates are merged and the ring wraps.  The cases and what they promise: tests/
train_kernels_reference.py and tests/test_train_kernels_cpu.py.  Every buffer a kernel writes has 64 sentinel elements behind it."""
import ctypes

import numpy as np
import pytest

import train_kernels_reference as R
from train_kernels_reference import F32, U8, Buf, D, H, P, refused, same_bits

pytestmark = pytest.mark.gpu


def _env():
    from simple_distributed_rl_amd import _native as N

    return N, N.lib()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 5. srlx_agent57_seq_td ------------------------------------------------------------------------------------------------------------------------------------
def _seq_run(N, lib, c, keep):
    B, S, A = c["B"], c["S"], c["A"]
    out = dict(target=Buf((S, B)), loss=Buf(1), grad=Buf((B, S + 1, A)), td=Buf(B), scratch=Buf(2 * B * S))  # the scratch: exactly what include/srlx.h names
    N.check(lib.srlx_agent57_seq_td(B, S, A, *[P(x) for x in keep], 0.95, c["dd"], c["rs"], out["target"].ptr(), out["loss"].ptr(), out["grad"].ptr(), out["td"].ptr(),
                                    out["scratch"].ptr(), None))
    return {k: b.get() for k, b in out.items()}


@pytest.mark.parametrize("c", R.SEQ_CASES + R.SEQ_FINITE_CASES, ids=R.case_id)
def test_agent57_seq_td_envelope(c):
    """Thinned cross product of B x S x A x double_dqn x rescale x mask (B = 257 and 513: a second and third workgroup, the loss an atomicAdd across them).
    Without rescale the target is agent57_seq_target's bits, with rescale rtol 1e-5 / atol 1e-6; loss, grad_q and td_mean at the bars of
    test_agent57_sequence_td_kernel_matches_reference; every grad_q entry of step S and of an untaken action is +0.  Mask given and double DQN off: row 0 has
    every action of its last step invalid -- the reference reads -inf there, so that row's targets, and the batch's loss, are not finite here as there and the loss
    assertion of those cases compares nothing; the two "whole0" cases give that pair without the all-invalid step, with a loss that is a number."""
    N, lib = _env()
    d = R.seq_case(c)
    B, S, A = c["B"], c["S"], c["A"]
    where = R.case_id(c)
    keep = [D(d["q"]), D(d["qt"]), D(d["act"]), D(d["rew"]), D(d["dones"]), D(None if d["inv"] is None else d["inv"].astype(U8)), D(d["disc"]), D(d["w"])]
    got = _seq_run(N, lib, c, keep)
    with np.errstate(invalid="ignore"):
        want = H.agent57_seq_target(d["q"], d["qt"], d["act"], d["rew"], d["dones"], d["inv"], d["disc"], 0.95, bool(c["dd"]), bool(c["rs"]))
        want64 = R.in_float64(H.agent57_seq_target, d["q"], d["qt"], d["act"], d["rew"], d["dones"], d["inv"], d["disc"], 0.95, bool(c["dd"]), bool(c["rs"]))
        R.check("target", got["target"], want, R.RTOL, 1e-6, want64, where)
        fin = np.isfinite(want)
        if c["rs"]:
            print("ENVELOPE %s target: %.0f %% of the entries bit-equal" % (where, 100 * R.bit_equal_share(got["target"], want)))
        else:
            same_bits(got["target"][fin], want[fin], where)
        o_loss, o_grad, o_td = H.agent57_seq_loss(d["q"], want, d["act"], d["w"])
        R.check("loss", got["loss"][0], o_loss, R.RTOL, 0.0, None, where)
        R.check("grad_q", got["grad"], o_grad, 1e-4, 1e-8, None, where)
        R.check("td_mean", got["td"], o_td, 1e-4, 2e-6, None, where)
    off = np.ones((B, S + 1, A), bool)
    off[np.arange(B)[:, None], np.arange(S)[None, :], d["act"]] = False
    assert (_u32(got["grad"])[off] == 0).all(), where + ": a grad_q entry of step S or of an untaken action is not +0"
    again = _seq_run(N, lib, c, keep)
    for k in ("target", "grad", "td") + (("loss",) if B <= 256 else ()):  # from B = 257 the loss is an atomicAdd across workgroups: its order is not fixed
        assert np.array_equal(_u32(again[k]), _u32(got[k])), f"{where}: a second call gives another {k}"


def test_agent57_seq_td_refusals_write_nothing():
    N, lib = _env()
    c = dict(B=3, S=2, A=2, dd=1, rs=0, mask=0)
    d = R.seq_case(c)
    keep = [D(d["q"]), D(d["qt"]), D(d["act"]), D(d["rew"]), D(d["dones"]), None, D(d["disc"]), D(d["w"])]
    out = [Buf((2, 3)), Buf(1), Buf((3, 3, 2)), Buf(3), Buf(12)]
    for B, S, A, null_scratch in ((0, 2, 2, False), (3, 0, 2, False), (3, 2, 0, False), (3, 2, 2, True)):
        ptrs = [b.ptr() for b in out]
        if null_scratch:
            ptrs[4] = None
        refused(N, lib, lib.srlx_agent57_seq_td(B, S, A, *[P(x) for x in keep], 0.95, 1, 0, *ptrs, None), "agent57_seq_td")
    assert all(b.untouched() for b in out)


# ---- 6. srlx_ngu_lifelong_reward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.LIFELONG_N)
def test_lifelong_reward_envelope(n):
    """D in {1, 7, 8, 9, 128, 129, 1000}: a plain loop, 8 partial sums, the tail behind them, the recursive halves.  Rows that clip at 1 (error 0) and at
    lifelong_max.  Bit-equal to the oracle."""
    N, lib = _env()
    for Dm in R.LIFELONG_D:
        target, train = R.lifelong_case(n, Dm)
        keep = [D(target), D(train)]
        out = Buf(n)
        N.check(lib.srlx_ngu_lifelong_reward(n, Dm, P(keep[0]), P(keep[1]), R.LIFELONG_MAX, out.ptr(), None))
        same_bits(out.get(), H.ngu_lifelong_reward(target, train, R.LIFELONG_MAX), f"n={n} D={Dm}")
    untouched = Buf(n)
    refused(N, lib, lib.srlx_ngu_lifelong_reward(n, 0, P(keep[0]), P(keep[1]), R.LIFELONG_MAX, untouched.ptr(), None), "ngu_lifelong_reward")
    refused(N, lib, lib.srlx_ngu_lifelong_reward(0, 8, P(keep[0]), P(keep[1]), R.LIFELONG_MAX, untouched.ptr(), None), "ngu_lifelong_reward")
    assert untouched.untouched()


# ---- 7. the episodic memory ------------------------------------------------------------------------------------------------------------------------------------
class _DeviceInt64:
    """n int64 at a raw device address, as torch reads foreign device memory (the CUDA array interface)."""

    def __init__(self, dev_ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<i8", data=(int(dev_ptr), False), version=2)


def _read_i64(dev_ptr, n):
    import torch

    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceInt64(dev_ptr, n), device="cuda:0").cpu().numpy().copy()


def _episodic_run(N, lib, name):
    """Every embedding uploaded once as [T][E][D], every step's rewards written to their own row of a [T][E] device array; -> rewards, the lanes' counters."""
    c = R.EPISODIC_CASES[name]
    E, T, Dm = c["E"], c["T"], c["D"]
    emb = R.episodic_embeddings(name)
    d_emb = D(emb)
    active = np.zeros(E, U8)
    active[list(c["lanes"])] = 1
    d_active = D(active) if E > 1 else None
    reward = Buf((T, E))
    h = N.c_p()
    N.check(lib.srlx_ngu_create(ctypes.byref(h), E, Dm, c["cap"], c["k"], *R.NGU_CONSTANTS, 0))
    try:
        for t in range(T):
            if t == c.get("reset_at", -1):
                N.check(lib.srlx_ngu_reset(h, None))
            N.check(lib.srlx_ngu_episodic_reward(h, ctypes.c_void_p(d_emb.data_ptr() + 4 * t * E * Dm), None, P(d_active), reward.ptr(t * E), None))
        got = reward.get()
        cnt = N.c_p()
        N.check(lib.srlx_ngu_counts(h, ctypes.byref(cnt)))
        counts = _read_i64(cnt.value, E)
    finally:
        lib.srlx_ngu_destroy(h)
    return c, emb, got, counts


@pytest.mark.parametrize("name", sorted(R.EPISODIC_CASES))
def test_episodic_memory_envelope(name):
    """Step by step against EpisodicMemoryOracle (exact_dot=False; its ring form, held to it on the CPU), rtol 1e-5, the default constants, embeddings uniform
    in [0, 1)^D.  a: split 1, up to 4 entries per thread, 276 overwrites of the ring.  b: E = 1024 with lanes 0, 511 and 1023 active, split 1 with 17 entries
    per thread -- a thread's 16-slot list overflows and the rejection test decides; the other lanes' rewards and counters must stay as they were.  c: split 3,
    k = 16, three candidate lists merged, the ring wraps.  d: split 16, the stride loop's second round.  e1 / e256: the edges of D.  f: five fixed points --
    exact zero distances, ave == 0, ties across threads and parts.  g: a reset at step 700; what lies behind the counter must not be read.  h: k = 16 with the
    16 nearest entries all in one thread's list and a 17th turned away -- the only case that needs the list's last slot."""
    N, lib = _env()
    c, emb, got, counts = _episodic_run(N, lib, name)
    lanes = list(c["lanes"])
    want = R.episodic_expected(name, emb)
    R.check("reward", got[:, lanes], want, R.RTOL, 0.0, None, "episodic case " + name)
    assert (counts[lanes] == (c["T"] - c.get("reset_at", 0))).all(), counts[lanes]
    idle = np.ones(c["E"], bool)
    idle[lanes] = False
    assert (got[:, idle] == F32(R.SENTINEL["f"])).all() and (counts[idle] == 0).all(), "an inactive lane was touched"


def test_episodic_memory_create_refusals():
    N, lib = _env()
    for Dm, cap, k in ((257, 300, 10), (0, 300, 10), (8, 300, 0), (8, 300, 17), (8, 0, 10)):
        h = N.c_p(1)
        refused(N, lib, lib.srlx_ngu_create(ctypes.byref(h), 1, Dm, cap, k, *R.NGU_CONSTANTS, 0), "ngu_create")
        assert not h.value, (Dm, cap, k)
