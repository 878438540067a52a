"""The kernels of csrc/srlx_agent57.hip and the two Agent57 kernels of csrc/srlx_ngu.hip (ucb_step, priority) over the envelope their entry points admit, through
the C ABI: the actor-side and batch-side pointwise kernels bit for bit against the numpy mirrors of tests/agent57_kernels_reference.py (themselves held to
hand-worked literals in tests/test_agent57_kernels_cpu.py), the two learner tails against float64 autograd on the CPU at every stride boundary of their loops, the
UCB bank against the plugin's host controller.  Every buffer a kernel writes has 64 guard elements behind it, filled with a sentinel that must survive; where an
argument selects a row of a larger array the neighbouring rows are sentinels too."""
import ctypes

import numpy as np
import pytest

import agent57_kernels_reference as R

pytestmark = pytest.mark.gpu

F32, I32, U8, I64, F64 = np.float32, np.int32, np.uint8, np.int64, np.float64
GUARD = 64
SENTINEL = {"f": -12345.0, "i": -777, "u": 0xA5}
E_LIST = (1, 255, 256, 257, 513)  # the 256-thread guard on either side, and a third workgroup
SEED = 0x5EED


def _env():
    import torch

    from simple_distributed_rl_amd import _native as N

    return N, N.lib(), torch, torch.device("cuda:0")


class Buf:
    """A device array with GUARD sentinel elements behind it; get() synchronises, checks the guard and returns the host copy."""

    def __init__(self, shape, dtype, init=None):
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
    """A read-only input on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=what)


def refused(N, lib, status, text):
    """The entry point returned an error (so it launched nothing) and its message names the reason."""
    assert status == N.ERR_INVALID, status
    msg = lib.srlx_last_error().decode("utf-8", "replace")
    assert text in msg, msg


# ---- 1. policy -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", E_LIST)
def test_policy_bit_equal_to_the_mirror(E):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(100 + E)
    beta_list = (np.arange(32) / 64.0).astype(F32)
    eps_list = np.tile(np.array([0.0, 1.0, 0.3, 0.3], F32), 8)  # exactly 0, exactly 1, and 0.3
    arm = rng.integers(0, 32, E).astype(I32)
    d_arm, d_beta, d_eps = D(arm), D(beta_list), D(eps_list)
    for A in (1, 2, 18):
        q_ext = rng.integers(-3, 4, (E, A)).astype(F32)  # small integers: ties
        q_int = rng.standard_normal((E, A)).astype(F32)
        q_int[0::2] = 0.0  # every second lane: q = q_ext, and its maximum is repeated (the first one counts, as for np.argmax)
        if A > 1:
            for e in range(0, E, 2):
                j = np.sort(rng.choice(A, 2, replace=False))
                q_ext[e, j] = q_ext[e].max() + 1.0
        d_qe, d_qi = D(q_ext), D(q_int)
        for counter in (0, 2 ** 40 + 3):
            d_counter = D(np.array([counter], I64))
            for training in (True, False):
                want_a, want_q, rnd = R.policy(q_ext, q_int, arm if training else None, beta_list, eps_list, 0.25, 0.3, SEED, counter)
                if E == 513 and training:  # both branches are taken among the lanes whose arm has epsilon 0.3 -- asserted on the mirror alone
                    share = rnd[eps_list[arm] == F32(0.3)].mean()
                    assert 0.1 <= share <= 0.9, share
                    assert rnd[eps_list[arm] == 1.0].all() and not rnd[eps_list[arm] == 0.0].any()
                    if A > 1:
                        tied = (~rnd)[0::2]
                        assert tied.sum() > 20  # greedy lanes with a repeated maximum
                for with_q in (True, False):
                    act, q_out = Buf(E, I32), Buf((E, A), F32)
                    N.check(lib.srlx_agent57_policy(E, A, P(d_qe), P(d_qi), P(d_arm) if training else None, P(d_beta) if training else None,
                                                    P(d_eps) if training else None, 0.25, 0.3, SEED, P(d_counter), act.ptr(), q_out.ptr() if with_q else None, None))
                    where = f"A={A} counter={counter} training={training} q_out={with_q}"
                    same_bits(act.get(), want_a, where)
                    if with_q:
                        same_bits(q_out.get(), want_q, where)
                    else:
                        assert q_out.untouched(), where
    refused(N, lib, lib.srlx_agent57_policy(E, 2, P(d_qe), P(d_qi), P(d_arm), None, P(d_eps), 0.25, 0.3, SEED, P(d_counter), Buf(E, I32).ptr(), None, None), "agent57_policy")


# ---- 2. post_step ----------------------------------------------------------------------------------------------------------------------------------------------
STATE = (("prev_action", I32), ("prev_r_ext", F32), ("prev_r_int", F32), ("episode_reward", F32))
XROWS = (("x_r_int", F32), ("x_prev_r_ext", F32), ("x_prev_r_int", F32), ("x_actor", I32), ("x_prev_action", I32))


def _state(rng, E, A=18):
    return dict(prev_action=rng.integers(0, A, E).astype(I32), prev_r_ext=rng.standard_normal(E).astype(F32), prev_r_int=rng.random(E).astype(F32),
                episode_reward=(10 * rng.standard_normal(E)).astype(F32))


@pytest.mark.parametrize("E", E_LIST)
def test_post_step_nine_arrays_bit_equal_over_three_calls(E):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(200 + E)
    for intrinsic in (True, False):
        for pattern in ("mixed", "none", "all"):
            s = _state(rng, E)
            first_reward = s["episode_reward"].copy()
            sb = {k: Buf(E, dt, s[k]) for k, dt in STATE}
            xb = {k: Buf((3, E), dt) for k, dt in XROWS}  # the kernel is handed row 1
            moved = np.zeros(E, bool)
            for call in range(3):
                actions, arm, rewards = rng.integers(0, 18, E).astype(I32), rng.integers(0, 32, E).astype(I32), rng.integers(-2, 3, E).astype(F32) + F32(0.1)
                reset = {"mixed": (rng.random(E) < 0.4), "none": np.zeros(E, bool), "all": np.ones(E, bool)}[pattern].astype(U8)
                epi, lif = rng.random(E).astype(F32), (1 + 4 * rng.random(E)).astype(F32)
                keep = [D(actions), D(arm), D(rewards), D(reset), D(epi), D(lif)]
                N.check(lib.srlx_agent57_post_step(E, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]) if intrinsic else None, P(keep[5]) if intrinsic else None,
                                                   sb["prev_action"].ptr(), sb["prev_r_ext"].ptr(), sb["prev_r_int"].ptr(), sb["episode_reward"].ptr(),
                                                   xb["x_r_int"].ptr(E), xb["x_prev_r_ext"].ptr(E), xb["x_prev_r_int"].ptr(E), xb["x_actor"].ptr(E), xb["x_prev_action"].ptr(E), None))
                s, x = R.post_step(s, actions, arm, rewards, reset, epi if intrinsic else None, lif if intrinsic else None)
                where = f"intrinsic={intrinsic} reset={pattern} call={call}"
                for k, _ in STATE:
                    same_bits(sb[k].get(), s[k], f"{where} {k}")
                for k, _ in XROWS:
                    got = xb[k].get()
                    same_bits(got[1], x[k], f"{where} {k}")
                    assert (got[0] == xb[k].sentinel).all() and (got[2] == xb[k].sentinel).all(), f"{where} {k}: a neighbouring ring row was written"
                moved |= reset == 0
            # the episode reward accumulated over the calls on the lanes that acted, and only there
            assert (s["episode_reward"][~moved] == first_reward[~moved]).all()
            if pattern != "all":
                assert (s["episode_reward"][moved] != first_reward[moved]).all()
    got = lib.srlx_agent57_post_step(E, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), None, sb["prev_action"].ptr(), sb["prev_r_ext"].ptr(), sb["prev_r_int"].ptr(),
                                     sb["episode_reward"].ptr(), xb["x_r_int"].ptr(E), xb["x_prev_r_ext"].ptr(E), xb["x_prev_r_int"].ptr(E), xb["x_actor"].ptr(E),
                                     xb["x_prev_action"].ptr(E), None)
    refused(N, lib, got, "agent57_post_step")
    got = lib.srlx_agent57_post_step(E, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), None, P(keep[5]), sb["prev_action"].ptr(), sb["prev_r_ext"].ptr(), sb["prev_r_int"].ptr(),
                                     sb["episode_reward"].ptr(), xb["x_r_int"].ptr(E), xb["x_prev_r_ext"].ptr(E), xb["x_prev_r_int"].ptr(E), xb["x_actor"].ptr(E),
                                     xb["x_prev_action"].ptr(E), None)
    refused(N, lib, got, "agent57_post_step")
    for k, _ in STATE:
        same_bits(sb[k].get(), s[k], f"after the refusals {k}")


# ---- 3. begin_episodes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", E_LIST)
def test_begin_episodes_resets_done_lanes_and_keeps_the_others(E):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(300 + E)
    for A in (1, 18):
        for counter in (0, 2 ** 40 + 3):
            d_counter = D(np.array([counter], I64))
            for with_done in (True, False):
                done = (rng.random(E) < 0.5).astype(U8)
                d_done = D(done)
                for with_reset in (True, False):
                    for with_live in (True, False):
                        s = _state(rng, E)
                        sb = {k: Buf(E, dt, s[k]) for k, dt in STATE}
                        reset, live = Buf(E, U8), Buf(E, U8)
                        N.check(lib.srlx_agent57_begin_episodes(E, A, P(d_done) if with_done else None, SEED, P(d_counter), sb["prev_action"].ptr(), sb["prev_r_ext"].ptr(),
                                                                sb["prev_r_int"].ptr(), sb["episode_reward"].ptr(), reset.ptr() if with_reset else None,
                                                                live.ptr() if with_live else None, None))
                        want, want_reset, want_live = R.begin_episodes(s, A, done if with_done else None, SEED, counter)
                        where = f"A={A} counter={counter} done={with_done} reset_lane={with_reset} live_lane={with_live}"
                        for k, _ in STATE:
                            got = sb[k].get()
                            same_bits(got, want[k], f"{where} {k}")
                            if with_done:
                                same_bits(got[done == 0], s[k][done == 0], f"{where} {k}: a lane that is not done changed")
                        if with_reset:
                            same_bits(reset.get(), want_reset, where)
                        else:
                            assert reset.untouched(), where
                        if with_live:
                            same_bits(live.get(), want_live, where)
                        else:
                            assert live.untouched(), where
        if A == 18 and E == 513:  # the random previous actions spread over the actions (on the mirror alone)
            first = R.begin_episodes(_state(rng, E), A, None, SEED, 0)[0]["prev_action"]
            assert len(set(first.tolist())) == 18


# ---- 4. gather_inputs ------------------------------------------------------------------------------------------------------------------------------------------
GATHER_OUT = (("on_r_ext", F32, 2), ("on_r_int", F32, 2), ("on_action", I32, 2), ("on_actor", I32, 2), ("tg_r_ext", F32, 1), ("tg_r_int", F32, 1), ("tg_action", I32, 1),
              ("tg_actor", I32, 1), ("discount", F32, 1), ("r_int", F32, 1))


@pytest.mark.parametrize("B", (1, 63, 64, 65))
def test_gather_inputs_equals_numpy_indexing(B):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(400 + B)
    L = 7
    for E in (4, 300):
        x = dict(x_r_int=rng.random((L, E)).astype(F32), x_prev_r_ext=rng.standard_normal((L, E)).astype(F32), x_prev_r_int=rng.random((L, E)).astype(F32),
                 x_actor=rng.integers(0, 32, (L, E)).astype(I32), x_prev_action=rng.integers(0, 18, (L, E)).astype(I32))
        dx = {k: D(v) for k, v in x.items()}
        discount_list = (1 - np.arange(1, 33) / 1000.0).astype(F32)
        d_disc = D(discount_list)
        for variant in ("edges", "last everywhere"):
            env, slot = rng.integers(0, E, B).astype(I64), rng.integers(0, L, B).astype(I64)
            env[0], slot[0] = 0, 0  # slot 0 with environment 0 ...
            if variant == "last everywhere":  # ... the last slot with the last environment, in every row
                env[:], slot[:] = E - 1, L - 1
            elif B > 1:
                env[-1], slot[-1] = E - 1, L - 1
            actions, rewards = rng.integers(0, 18, B).astype(I32), rng.standard_normal(B).astype(F32)
            keep = [D(env), D(slot), D(actions), D(rewards)]
            out = {k: Buf(m * B, dt) for k, dt, m in GATHER_OUT}
            N.check(lib.srlx_agent57_gather_inputs(B, E, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(dx["x_r_int"]), P(dx["x_prev_r_ext"]), P(dx["x_prev_r_int"]),
                                                   P(dx["x_actor"]), P(dx["x_prev_action"]), P(d_disc), *[out[k].ptr() for k, _, _ in GATHER_OUT], None))
            want = R.gather_inputs(env, slot, actions, rewards, x, discount_list)
            for k, _, _ in GATHER_OUT:
                same_bits(out[k].get(), want[k], f"E={E} {variant} {k}")
    args = [P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(dx["x_r_int"]), P(dx["x_prev_r_ext"]), P(dx["x_prev_r_int"]), P(dx["x_actor"]), P(dx["x_prev_action"]), P(d_disc)]
    refused(N, lib, lib.srlx_agent57_gather_inputs(B, E, *args, *[out[k].ptr() for k, _, _ in GATHER_OUT][:-1], None, None), "NULL argument")


# ---- 5. pack_record / unpack_fields ----------------------------------------------------------------------------------------------------------------------------
def _pack_args(N, E, v, x, rec_ptr):
    return (E, P(v["actions"]), P(v["rewards"]), P(v["terminated"]), P(v["done"]), P(x["x_r_int"]), P(x["x_actor"]), P(x["x_prev_action"]), P(x["x_prev_r_ext"]),
            P(x["x_prev_r_int"]), rec_ptr, None)


@pytest.mark.parametrize("per", (4, 252, 256, 260))
def test_pack_record_layout_and_unpack_fields_round_trip(per):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(500 + per)
    L = 5
    for records in (1, 3):
        total = records * per
        for stride in (30 * per, 30 * per + 8):
            host, devs = [], []
            for r in range(records):
                v = dict(actions=rng.integers(0, 18, per).astype(I32), rewards=rng.standard_normal(per).astype(F32), terminated=(rng.random(per) < 0.3).astype(U8),
                         done=(rng.random(per) < 0.3).astype(U8))
                x = dict(x_r_int=rng.random(per).astype(F32), x_actor=(np.arange(per) % 32).astype(I32), x_prev_action=((np.arange(per) + r) % 18).astype(I32),
                         x_prev_r_ext=rng.standard_normal(per).astype(F32), x_prev_r_int=(2 + rng.random(per)).astype(F32))
                host.append((v, x))
                devs.append(({k: D(a) for k, a in v.items()}, {k: D(a) for k, a in x.items()}))
            rec = Buf(records * stride, U8)
            want_rec = np.full(records * stride, rec.sentinel, U8)  # the slack behind every record keeps the sentinel
            for r in range(records):
                N.check(lib.srlx_agent57_pack_record(*_pack_args(N, per, devs[r][0], devs[r][1], rec.ptr(r * stride))))
                want_rec[r * stride: r * stride + 30 * per] = R.pack_record(host[r][0]["actions"], host[r][0]["rewards"], host[r][0]["terminated"], host[r][0]["done"], host[r][1])
            got_rec = rec.get()
            same_bits(got_rec, want_rec, f"records={records} stride={stride}")
            for pos in (0, 4, 5, 27, -1):
                d_pos = D(np.array([pos], I64))
                ring = {k: Buf((L, total), dt) for k, dt in XROWS}
                N.check(lib.srlx_agent57_unpack_fields(records, per, rec.ptr(), stride, P(d_pos), L, ring["x_r_int"].ptr(), ring["x_actor"].ptr(), ring["x_prev_action"].ptr(),
                                                       ring["x_prev_r_ext"].ptr(), ring["x_prev_r_int"].ptr(), None))
                want = {k: np.full((L, total), SENTINEL[np.dtype(dt).kind], dt) for k, dt in XROWS}
                slot = R.unpack_fields(got_rec, records, per, stride, pos, want)
                assert slot == {0: 0, 4: 4, 5: 0, 27: 2, -1: 4}[pos]
                for k, _ in XROWS:
                    got = ring[k].get()
                    same_bits(got, want[k], f"records={records} stride={stride} pos={pos} {k}")  # (every other ring row: still the sentinel)
                    same_bits(got[slot], np.concatenate([h[1][k] for h in host]), f"environment g = record * per + lane: {k}")  # arms 0..31, actions 0..17 exact
            same_bits(rec.get(), want_rec, "unpack_fields reads only")
    # refusals: nothing is launched
    v, x = devs[0]
    fresh = Buf(30 * per, U8)
    refused(N, lib, lib.srlx_agent57_pack_record(*_pack_args(N, 6, v, x, fresh.ptr())), "multiples of 4")
    nov = dict(v, rewards=None)
    refused(N, lib, lib.srlx_agent57_pack_record(*_pack_args(N, per, nov, x, fresh.ptr())), "agent57_pack_record")
    refused(N, lib, lib.srlx_agent57_pack_record(*_pack_args(N, per, v, x, None)), "agent57_pack_record")
    assert fresh.untouched()
    ring = {k: Buf((L, total), dt) for k, dt in XROWS}
    rp = [ring[k].ptr() for k in ("x_r_int", "x_actor", "x_prev_action", "x_prev_r_ext", "x_prev_r_int")]
    refused(N, lib, lib.srlx_agent57_unpack_fields(1, 6, rec.ptr(), 30 * per, P(d_pos), L, *rp, None), "multiples of 4")
    refused(N, lib, lib.srlx_agent57_unpack_fields(records, per, rec.ptr(), 30 * per - 4, P(d_pos), L, *rp, None), "record_stride >= 30")
    refused(N, lib, lib.srlx_agent57_unpack_fields(records, per, rec.ptr(), 30 * per + 2, P(d_pos), L, *rp, None), "record_stride in multiples of 4")  # misaligned float loads
    refused(N, lib, lib.srlx_agent57_unpack_fields(records, per, None, stride, P(d_pos), L, *rp, None), "agent57_unpack_fields")
    refused(N, lib, lib.srlx_agent57_unpack_fields(records, per, rec.ptr(), stride, None, L, *rp, None), "agent57_unpack_fields")
    refused(N, lib, lib.srlx_agent57_unpack_fields(records, per, rec.ptr(), stride, P(d_pos), L, *rp[:-1], None, None), "agent57_unpack_fields")
    for k, _ in XROWS:
        assert ring[k].untouched(), k


# ---- 6. emb_tail -----------------------------------------------------------------------------------------------------------------------------------------------
# (B, D, Hd, A) -> seed.  The seeds are the first for which the float64 reference meets the two conditions asserted in _emb_conditions.
EMB_SHAPES = {
    (16, 32, 128, 6): 21,    # the shape of tests/test_agent57_fast_gpu.py
    (1, 1, 1, 2): 0,         # every size at its minimum: three waves idle, LayerNorm over one value
    (3, 5, 63, 1): 0,        # softmax of a single logit
    (5, 7, 65, 3): 0,        # Hd one past a wave's 64 lanes, B one past the four waves' stride
    (4, 4, 256, 32): 3,      # Hd at the 256-thread stride, A at its maximum
    (4, 4, 257, 32): 2,      # ... and one past it
    (2, 8, 128, 4): 0,       # Hd * 2 D = 2048: exactly one pass of the w1 loop's 8 x 256 elements
    (2, 25, 41, 4): 0,       # 2050: two elements more
    (64, 32, 128, 17): 0,    # the largest the LDS check admits: 40,832 floats = 163,328 of 163,840 bytes
}
LR = 5e-4


def _emb_case(shape):
    B, D, Hd, A = shape
    return R.emb_case(B, D, Hd, A, EMB_SHAPES[shape], zero_actions=(A == 1))


def _emb_conditions(shape, r64):
    """On the float64 reference alone: no pre-activation of the hidden layer within 1e-4 of zero (a float32 sign flip across the ReLU is no kernel error), and,
    except for the single-logit shape, between 20 % and 80 % of the hidden units active.  One hidden unit of one row (the all-minimal shape) is active or not:
    there it must be active."""
    B, D, Hd, A = shape
    pre = r64["pre"]
    assert float(pre.abs().min()) > 1e-4, float(pre.abs().min())
    active = float((pre > 0).double().mean())
    if B * Hd == 1:
        assert active == 1.0
    elif A != 1:
        assert 0.2 <= active <= 0.8, active


class EmbRun:
    """The six parameter tensors with gradients and moments in guarded buffers, and one launch per call."""

    def __init__(self, c, m=None, v=None):
        self.c = c
        ps = [p.numpy() for p in c["params"]]
        self.p = [Buf(a.shape, F32, a) for a in ps]
        self.g = [Buf(a.shape, F32) for a in ps]
        self.m = [Buf(a.shape, F32, np.zeros_like(a) if m is None else m[k]) for k, a in enumerate(ps)]
        self.v = [Buf(a.shape, F32, np.zeros_like(a) if v is None else v[k]) for k, a in enumerate(ps)]
        self.emb, self.act = D(c["emb"].numpy()), D(c["actions"].numpy().astype(I32))

    def launch(self, steps_taken=None):
        N, lib, torch, dev = _env()
        c = self.c
        tab = lambda bs: ctypes.cast((N.c_p * 6)(*[b.t.data_ptr() for b in bs]), N.c_p)  # noqa: E731
        loss, d_emb = Buf(1, F32), Buf((2 * c["B"], c["D"]), F32)
        adam = steps_taken is not None
        step = D(np.array([steps_taken if adam else 0], I64))
        N.check(lib.srlx_agent57_emb_tail(c["B"], c["D"], c["Hd"], c["A"], P(self.emb), P(self.act), tab(self.p), tab(self.g), tab(self.m) if adam else None,
                                          tab(self.v) if adam else None, R.LN_EPS, LR, 0.9, 0.999, 1e-8, P(step) if adam else None, loss.ptr(), d_emb.ptr(), None))
        return loss.get()[0], d_emb.get(), [b.get() for b in self.g]


def _torch_adam(torch, params, steps_taken=0, m=None, v=None):
    """torch.optim.Adam on CPU copies of `params` (numpy), its state at `steps_taken` steps with the moments m, v."""
    tp = [torch.from_numpy(p.copy()).requires_grad_(True) for p in params]
    opt = torch.optim.Adam(tp, lr=LR, betas=(0.9, 0.999), eps=1e-8)
    if steps_taken:
        for t in tp:
            t.grad = torch.zeros_like(t)
        opt.step()  # creates the state; a zero gradient on zero moments moves nothing
        with torch.no_grad():
            for k, t in enumerate(tp):
                t.copy_(torch.from_numpy(params[k]))
                st = opt.state[t]
                st["step"].fill_(float(steps_taken))
                st["exp_avg"].copy_(torch.from_numpy(m[k]))
                st["exp_avg_sq"].copy_(torch.from_numpy(v[k]))
    return tp, opt


def _adam_follows(torch, tp, opt, grads, bufs, where):
    """One torch.optim.Adam step on the KERNEL's own gradients (the gradients are held to autograd separately; an optimiser fed autograd's would differ by the
    full learning rate wherever a gradient is a rounding residue: tests/test_agent57_fast_gpu.py), then the parameters at that test's bars."""
    for t, g in zip(tp, grads):
        t.grad = torch.from_numpy(g.copy())
    opt.step()
    for k, (b, t) in enumerate(zip(bufs, tp)):
        torch.testing.assert_close(torch.from_numpy(b.get()), t.detach(), rtol=2e-6, atol=1e-8, msg=lambda m: f"{where} parameter {k}: {m}")


@pytest.mark.parametrize("shape", list(EMB_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_emb_tail_against_float64_autograd_and_adam(shape):
    N, lib, torch, dev = _env()
    B, D, Hd, A = shape
    c = _emb_case(shape)
    r64, r32 = R.emb_reference(c, torch.float64), R.emb_reference(c, torch.float32)
    _emb_conditions(shape, r64)
    before = [p.numpy().copy() for p in c["params"]]
    # gradients only
    run = EmbRun(c)
    loss, d_emb, grads = run.launch()
    where = "emb_tail %dx%dx%dx%d" % shape
    R.check_loss(loss, r64["loss"], where)
    R.check_tensor("d_emb", d_emb, r64["d_emb"], r32["d_emb"], where)
    for name, got, w64, w32 in zip(R.EMB_NAMES, grads, r64["grads"], r32["grads"]):
        R.check_tensor("d " + name, got, w64, w32, where)
    for b, p in zip(run.p, before):
        same_bits(b.get(), p, "gradients only: a parameter changed")
    for b in run.m + run.v:
        assert (b.get() == 0).all()
    if A == 1:  # the one-hot target of a single action is the softmax itself: everything is exactly zero
        assert loss == 0.0 and (d_emb == 0.0).all() and all((g == 0.0).all() for g in grads)
    else:  # run to run: the same bits
        loss2, d_emb2, grads2 = EmbRun(c).launch()
        same_bits(np.array([loss2]), np.array([loss]), "loss, second run")
        same_bits(d_emb2, d_emb, "d_emb, second run")
        for a, b in zip(grads2, grads):
            same_bits(a, b, "gradients, second run")
    # three Adam steps from steps_taken = 0
    run = EmbRun(c)
    tp, opt = _torch_adam(torch, before)
    for step in range(3):
        l, de, gs = run.launch(steps_taken=step)
        if step == 0:  # what the kernel differentiates does not depend on whether it then steps
            same_bits(np.array([l]), np.array([loss]), "loss with Adam")
            same_bits(de, d_emb, "d_emb with Adam")
            for a, b in zip(gs, grads):
                same_bits(a, b, "gradients with Adam")
        assert np.isfinite(l) and all(np.isfinite(g).all() for g in gs)
        _adam_follows(torch, tp, opt, gs, run.p, f"{where} step {step}")
    if A == 1:
        for b, p in zip(run.p, before):
            same_bits(b.get(), p, "zero gradients: three Adam steps must leave the parameters as they are")
    for b, p, g0 in zip(run.p, before, grads):  # (a LayerNorm over one value passes no gradient down: those parameters rightly stay)
        assert (b.get() != p).any() == bool((g0 != 0).any())
    # one Adam step at steps_taken = 1,000,000: bias corrections ~ 1, the integer power's long path; moments as a long run leaves them
    g = torch.Generator().manual_seed(7)
    m = [(0.01 * torch.randn(p.shape, generator=g)).numpy() for p in before]
    v = [(1e-4 * torch.rand(p.shape, generator=g)).numpy() for p in before]
    run = EmbRun(c, m=m, v=v)
    tp, opt = _torch_adam(torch, before, 1_000_000, m, v)
    l, de, gs = run.launch(steps_taken=1_000_000)
    same_bits(de, d_emb, "d_emb at step 1,000,000")
    _adam_follows(torch, tp, opt, gs, run.p, f"{where} step 1,000,000")
    assert all((b.get() != p).any() for b, p in zip(run.p, before))
    for k, b in enumerate(run.m):
        torch.testing.assert_close(torch.from_numpy(b.get()), opt.state[tp[k]]["exp_avg"], rtol=2e-6, atol=1e-8)


def test_emb_tail_refusals():
    N, lib, torch, dev = _env()

    def call(B, D, Hd, A, null_param=None):
        c = R.emb_case(B, D, Hd, A, 1)
        run = EmbRun(c)
        ptrs = [b.t.data_ptr() for b in run.p]
        if null_param is not None:
            ptrs[null_param] = None
        tab = lambda xs: ctypes.cast((N.c_p * 6)(*xs), N.c_p)  # noqa: E731
        loss, d_emb = Buf(1, F32), Buf((2 * B, D), F32)
        st = lib.srlx_agent57_emb_tail(B, D, Hd, A, P(run.emb), P(run.act), tab(ptrs), tab([b.t.data_ptr() for b in run.g]), None, None, R.LN_EPS, LR, 0.9, 0.999, 1e-8, None,
                                       loss.ptr(), d_emb.ptr(), None)
        assert loss.untouched() and d_emb.untouched() and all(b.untouched() for b in run.g)
        return st

    refused(N, lib, call(64, 32, 128, 18), "164096 bytes of LDS")
    refused(N, lib, call(65, 4, 8, 2), "batch <= 64")
    refused(N, lib, call(4, 4, 8, 33), "n_actions <= 32")
    refused(N, lib, call(4, 4, 8, 2, null_param=3), "parameter / gradient 3 is NULL")


# ---- 7. rnd_tail -----------------------------------------------------------------------------------------------------------------------------------------------
RND_SHAPES = ((1, 1, 1), (3, 63, 63), (5, 65, 130), (4, 256, 512), (4, 257, 300), (16, 128, 256), (64, 127, 127))  # (B, D, row_stride)


def _strided(a, ld, fill):
    """Rows of `a` ld floats apart in a buffer of exactly (B - 1) ld + D floats (plus the guard), everything between them `fill`."""
    B, Dm = a.shape
    flat = np.full((B - 1) * ld + Dm, fill, F32)
    for b in range(B):
        flat[b * ld: b * ld + Dm] = a[b]
    return flat


class RndRun:
    def __init__(self, c, ld, fill=1e30):
        self.c, self.ld = c, ld
        Dm = c["D"]
        self.h, self.target = (Buf(len(_strided(c[k].numpy(), ld, fill)), F32, _strided(c[k].numpy(), ld, fill)) for k in ("h", "target"))
        for b in (self.h, self.target):  # what lies behind the last row is as foreign as what lies between the rows
            b.sentinel = F32(fill)
            b.t[b.n:] = float(fill)
        self.w, self.b = Buf(Dm, F32, c["ln_w"].numpy()), Buf(Dm, F32, c["ln_b"].numpy())
        self.gw, self.gb, self.mw, self.mb = Buf(Dm, F32), Buf(Dm, F32), Buf(Dm, F32), Buf(Dm, F32)
        self.m = [Buf(Dm, F32, np.zeros(Dm, F32)) for _ in range(4)]  # exp_avg w, exp_avg_sq w, exp_avg b, exp_avg_sq b

    def launch(self, steps_taken=None, grads=True, mirrors=False):
        N, lib, torch, dev = _env()
        c = self.c
        adam = steps_taken is not None
        step = D(np.array([steps_taken if adam else 0], I64))
        loss, d_h = Buf(1, F32), Buf((c["B"], c["D"]), F32)
        mo = [b.ptr() if adam else None for b in self.m]
        N.check(lib.srlx_agent57_rnd_tail(c["B"], c["D"], self.ld, self.h.ptr(), self.target.ptr(), self.w.ptr(), self.b.ptr(), self.gw.ptr() if grads else None,
                                          self.gb.ptr() if grads else None, mo[0], mo[1], mo[2], mo[3], self.mw.ptr() if mirrors else None, self.mb.ptr() if mirrors else None,
                                          R.LN_EPS, LR, 0.9, 0.999, 1e-8, P(step) if adam else None, loss.ptr(), d_h.ptr(), None))
        self.h.get(), self.target.get()  # (read only)
        return loss.get()[0], d_h.get()


@pytest.mark.parametrize("shape", RND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rnd_tail_against_float64_autograd_and_adam(shape):
    N, lib, torch, dev = _env()
    B, Dm, ld = shape
    c = R.rnd_case(B, Dm, 40 + B + Dm)
    r64, r32 = R.rnd_reference(c, torch.float64), R.rnd_reference(c, torch.float32)
    w0, b0 = c["ln_w"].numpy().copy(), c["ln_b"].numpy().copy()
    where = "rnd_tail %dx%d stride %d" % shape
    # gradients only
    run = RndRun(c, ld)
    loss, d_h = run.launch()
    gw, gb = run.gw.get(), run.gb.get()
    R.check_loss(loss, r64["loss"], where)
    R.check_tensor("d_h", d_h, r64["d_h"], r32["d_h"], where)  # dense [B][D] whatever the row stride
    R.check_tensor("d ln_w", gw, r64["g_w"], r32["g_w"], where)
    R.check_tensor("d ln_b", gb, r64["g_b"], r32["g_b"], where)
    same_bits(run.w.get(), w0, "gradients only: ln_w changed")
    same_bits(run.b.get(), b0, "gradients only: ln_b changed")
    assert run.mw.untouched() and run.mb.untouched()
    # what lies between the strided rows influences nothing
    other = RndRun(c, ld, fill=-3e33)
    loss2, d_h2 = other.launch()
    same_bits(np.array([loss2]), np.array([loss]), "loss with other values between the rows")
    same_bits(d_h2, d_h, "d_h with other values between the rows")
    same_bits(other.gw.get(), gw), same_bits(other.gb.get(), gb)
    # mirrors without Adam: the unchanged parameters
    run = RndRun(c, ld)
    run.launch(mirrors=True)
    same_bits(run.mw.get(), w0, "mirror of ln_w without Adam"), same_bits(run.mb.get(), b0, "mirror of ln_b without Adam")
    same_bits(run.w.get(), w0), same_bits(run.b.get(), b0)
    same_bits(run.gw.get(), gw), same_bits(run.gb.get(), gb)
    # three Adam steps with mirrors
    run = RndRun(c, ld)
    tp, opt = _torch_adam(torch, [w0, b0])
    for step in range(3):
        l, dh = run.launch(steps_taken=step, mirrors=True)
        if step == 0:
            same_bits(np.array([l]), np.array([loss]), "loss with Adam"), same_bits(dh, d_h, "d_h with Adam")
            same_bits(run.gw.get(), gw), same_bits(run.gb.get(), gb)
        _adam_follows(torch, tp, opt, [run.gw.get(), run.gb.get()], [run.w, run.b], f"{where} step {step}")
        same_bits(run.mw.get(), run.w.get(), "mirror of ln_w"), same_bits(run.mb.get(), run.b.get(), "mirror of ln_b")
    assert (run.w.get() != w0).any() == bool((gw != 0).any()) and (run.b.get() != b0).any()  # (the LayerNorm of one value is 0: its weight has no gradient)
    three_w, three_b = run.w.get(), run.b.get()
    # the same three steps without gradient outputs and without mirrors: the steps are still taken
    run = RndRun(c, ld)
    for step in range(3):
        run.launch(steps_taken=step, grads=False)
    same_bits(run.w.get(), three_w, "Adam without gradient outputs"), same_bits(run.b.get(), three_b, "Adam without gradient outputs")
    assert run.gw.untouched() and run.gb.untouched() and run.mw.untouched() and run.mb.untouched()


def test_rnd_tail_refusals():
    N, lib, torch, dev = _env()

    def call(B, Dm, ld):
        run = RndRun(R.rnd_case(B, Dm, 1), max(ld, Dm))
        loss, d_h = Buf(1, F32), Buf((B, Dm), F32)
        st = lib.srlx_agent57_rnd_tail(B, Dm, ld, run.h.ptr(), run.target.ptr(), run.w.ptr(), run.b.ptr(), run.gw.ptr(), run.gb.ptr(), None, None, None, None, None, None, R.LN_EPS,
                                       LR, 0.9, 0.999, 1e-8, None, loss.ptr(), d_h.ptr(), None)
        assert loss.untouched() and d_h.untouched() and run.gw.untouched()
        return st

    refused(N, lib, call(64, 128, 128), "65808 bytes of LDS")
    refused(N, lib, call(65, 8, 8), "batch <= 64")
    refused(N, lib, call(4, 8, 7), "row_stride >= dim")


# ---- 8. ucb_step -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((5, 4, 9), (257, 4, 9), (3, 1, 2), (3, 6, 4), (4, 3, 2)), ids=lambda s: "x".join(map(str, s)))
def test_ucb_step_equals_the_host_controllers(shape):
    """(E, arms, window): the thread guard; one arm and the smallest legal window; a window no larger than the arm count (the round of every arm once never ends)."""
    N, lib, torch, dev = _env()
    E, Na, window = shape
    beta = 0.7
    top = np.nextafter(1.0, 0.0)
    for eps in (0.0, 1.0, 0.2):
        for with_done in (False, True):
            rng = np.random.default_rng(800 + E + Na)
            ring_arm, ring_reward, head, n_recent = Buf((E, window), I32, np.zeros((E, window))), Buf((E, window), F32, np.zeros((E, window))), Buf(E, I32, np.zeros(E)), Buf(E, I32, np.zeros(E))
            count, total, arm = Buf((E, Na), I32, np.ones((E, Na))), Buf((E, Na), F64, np.zeros((E, Na))), Buf(E, I32, np.full(E, -1))
            hosts = R.HostUcbBank(E, Na, window, eps, beta)
            last = np.zeros(E, F32)
            where = f"epsilon={eps} done={with_done}"
            for it in range(40):
                done = (rng.random(E) < 0.7).astype(U8)
                u = rng.random((E, 3))
                u[rng.random(E) < 0.2, 1] = top  # the largest double below 1: floor(u * n) must be clamped to n - 1
                u[rng.random(E) < 0.2, 2] = top
                keep = [D(done), D(last), D(u)]
                N.check(lib.srlx_agent57_ucb_step(E, Na, window, ring_arm.ptr(), ring_reward.ptr(), head.ptr(), n_recent.ptr(), count.ptr(), total.ptr(), arm.ptr(),
                                                  P(keep[0]) if with_done else None, P(keep[1]), P(keep[2]), eps, beta, None))
                want = hosts.step(done if with_done else None, last, u)
                np.testing.assert_array_equal(arm.get(), want.astype(I32), err_msg=f"{where} iteration {it}")
                last = rng.integers(-3, 4, E).astype(F32)  # small integers: ties between arms do occur
            np.testing.assert_array_equal(count.get(), np.array([h.count for h in hosts.hosts], I32), err_msg=where)
            same_bits(total.get(), np.array([h.reward for h in hosts.hosts], F64), where)
            np.testing.assert_array_equal(n_recent.get(), np.array([len(h.recent) for h in hosts.hosts], I32), err_msg=where)
            assert int(n_recent.get().max()) == window - 1  # the window slid
            h = head.get()
            assert (0 <= h).all() and (h < window).all()
            ring_arm.get(), ring_reward.get()
    refused(N, lib, lib.srlx_agent57_ucb_step(E, Na, 1, ring_arm.ptr(), ring_reward.ptr(), head.ptr(), n_recent.ptr(), count.ptr(), total.ptr(), arm.ptr(), None, P(keep[1]), P(keep[2]),
                                              0.2, beta, None), "agent57_ucb_step")


# ---- 9. priority -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 255, 256, 257))
def test_priority_four_modes_bit_equal_to_the_mirror(B):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(900 + B)
    beta_list = (np.arange(32) / 100.0).astype(F32)
    d_beta = D(beta_list)
    for A in (1, 18):
        te, ti = rng.standard_normal(B).astype(F32), rng.standard_normal(B).astype(F32)
        qe, qi = rng.standard_normal((B, A)).astype(F32), rng.standard_normal((B, A)).astype(F32)
        act, idx = rng.integers(0, A, B).astype(I32), rng.integers(0, 32, B).astype(I32)
        d = dict(te=D(te), ti=D(ti), qe=D(qe), qi=D(qi), act=D(act), idx=D(idx))
        for with_q in (True, False):
            for intrinsic in (True, False):
                want_te, want_ti, want_p = R.priority(te, qe if with_q else None, ti if intrinsic else None, qi if with_q else None, act, idx, beta_list)
                for with_td in (True, False):
                    o_te, o_ti, pri = Buf(B, F32), Buf(B, F32), Buf(B, F32)
                    N.check(lib.srlx_agent57_priority(B, A, P(d["te"]), P(d["qe"]) if with_q else None, P(d["ti"]) if intrinsic else None,
                                                      P(d["qi"]) if with_q and intrinsic else None, P(d["act"]) if with_q else None, P(d["idx"]) if intrinsic else None,
                                                      P(d_beta) if intrinsic else None, o_te.ptr() if with_td else None, o_ti.ptr() if with_td else None, pri.ptr(), None))
                    where = f"A={A} q={with_q} intrinsic={intrinsic} td outputs={with_td}"
                    same_bits(pri.get(), want_p, where)
                    if with_td:
                        same_bits(o_te.get(), want_te, where)
                    else:
                        assert o_te.untouched(), where
                    if with_td and intrinsic:
                        same_bits(o_ti.get(), want_ti, where)
                    else:
                        assert o_ti.untouched(), where
    pri = Buf(B, F32)
    refused(N, lib, lib.srlx_agent57_priority(B, A, P(d["te"]), P(d["qe"]), None, None, None, None, None, None, None, pri.ptr(), None), "agent57_priority: bad argument")
    refused(N, lib, lib.srlx_agent57_priority(B, A, P(d["te"]), None, P(d["ti"]), None, None, None, P(d_beta), None, None, pri.ptr(), None), "intrinsic inputs incomplete")
    refused(N, lib, lib.srlx_agent57_priority(B, A, P(d["te"]), None, P(d["ti"]), None, None, P(d["idx"]), None, None, None, pri.ptr(), None), "intrinsic inputs incomplete")
    refused(N, lib, lib.srlx_agent57_priority(B, A, P(d["te"]), P(d["qe"]), P(d["ti"]), None, P(d["act"]), P(d["idx"]), P(d_beta), None, None, pri.ptr(), None), "intrinsic inputs incomplete")
    refused(N, lib, lib.srlx_agent57_priority(B, A, P(d["te"]), None, P(d["ti"]), P(d["qi"]), None, P(d["idx"]), P(d_beta), None, None, pri.ptr(), None), "intrinsic inputs incomplete")
    assert pri.untouched()
