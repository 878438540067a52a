"""The numpy mirrors of tests/agent57_kernels_reference.py on tiny cases worked by hand, the expected values written as literals: a mirror copied from a wrong
kernel cannot agree with the kernel by construction.  And the two torch evaluations of the tails (float64, float32) against each other."""
import numpy as np

import agent57_kernels_reference as R

F32, I32, U8 = np.float32, np.int32, np.uint8
f = lambda *v: np.array(v, F32)  # noqa: E731
i = lambda *v: np.array(v, I32)  # noqa: E731
b = lambda *v: np.array(v, U8)  # noqa: E731


def test_keyed_generator_draws_used_below():
    """The draws the cases below are worked from (seed 7): key (counter, index) -> uniform."""
    want = {(0, 0): 0.7215081806049702, (0, 2): 0.6210743749957076, (0, 3): 0.46486406263663593, (0, 4): 0.6767898732408049, (5, 0): 0.942822051884815,
            (5, 2): 0.5802164673270307}
    for (c, k), u in want.items():
        assert float(R.u53(R.rng_u64(7, c, k))) == u


def test_policy_three_lanes_by_hand():
    """A = 3, seed 7, counter 0; beta_list (0.5, 2, 0.25), eps_list (0, 1, 0.5).
    lane 0, arm 2: q = (1 + .25 * 4, 2 + 0, 1.5 + .25 * 2) = (2, 2, 2), an exact tie; draw(0) = 0.72 >= 0.5 -> greedy -> the FIRST maximum, 0.
    lane 1, arm 1: epsilon 1.0: draw(2) = 0.62 < 1 -> random: floor(draw(3) * 3) = floor(1.39) = 1 (greedy would be 2: q = (2, 2, 7)).
    lane 2, arm 0: epsilon 0.0: draw(4) = 0.68 is not < 0 -> greedy: q = (-1 + .5, .5 - .5, .25 + 1) = (-.5, 0, 1.25) -> 2."""
    q_ext = np.array([[1, 2, 1.5], [0, 0, 5], [-1, 0.5, 0.25]], F32)
    q_int = np.array([[4, 0, 2], [1, 1, 1], [1, -1, 2]], F32)
    act, q, rnd = R.policy(q_ext, q_int, i(2, 1, 0), f(0.5, 2.0, 0.25), f(0.0, 1.0, 0.5), 9.0, 9.0, 7, 0)
    assert act.dtype == I32 and act.tolist() == [0, 1, 2]
    assert q.dtype == F32 and q.tolist() == [[2.0, 2.0, 2.0], [2.0, 2.0, 7.0], [-0.5, 0.0, 1.25]]
    assert rnd.tolist() == [False, True, False]
    # evaluation: arm None -> test_beta 1.0 / test_epsilon 0.0 for every lane: q = q_ext + q_int, greedy
    act, q, rnd = R.policy(q_ext, q_int, None, None, None, 1.0, 0.0, 7, 0)
    assert q.tolist() == [[5.0, 2.0, 3.5], [1.0, 1.0, 6.0], [0.0, -0.5, 2.25]] and act.tolist() == [0, 2, 2] and not rnd.any()


def test_post_step_by_hand():
    """Lane 0 acted (live), lane 1 only received a new episode's first frame: it keeps its state and earns no intrinsic reward; the item fields are what the lanes
    held BEFORE the step."""
    s = dict(prev_action=i(4, 5), prev_r_ext=f(0.5, 0.25), prev_r_int=f(2.0, 3.0), episode_reward=f(10.0, 20.0))
    new, x = R.post_step(s, i(1, 2), i(7, 8), f(1.5, -1.0), b(0, 1), f(0.5, 0.5), f(3.0, 3.0))
    assert x["x_actor"].tolist() == [7, 8] and x["x_prev_action"].tolist() == [4, 5] and x["x_prev_r_ext"].tolist() == [0.5, 0.25]
    assert x["x_prev_r_int"].tolist() == [2.0, 3.0] and x["x_r_int"].tolist() == [1.5, 0.0]
    assert new["prev_action"].tolist() == [1, 5] and new["prev_r_ext"].tolist() == [1.5, 0.25] and new["prev_r_int"].tolist() == [1.5, 3.0]
    assert new["episode_reward"].tolist() == [11.5, 20.0]
    new, x = R.post_step(s, i(1, 2), i(7, 8), f(1.5, -1.0), b(0, 0), None, None)  # no intrinsic reward
    assert x["x_r_int"].tolist() == [0.0, 0.0] and new["prev_r_int"].tolist() == [0.0, 0.0] and new["episode_reward"].tolist() == [11.5, 19.0]


def test_begin_episodes_by_hand():
    """A = 4, seed 7, counter 5: lanes 0 and 2 are done: floor(0.9428 * 4) = 3, floor(0.5802 * 4) = 2; lane 1 keeps everything."""
    s = dict(prev_action=i(1, 1, 1), prev_r_ext=f(0.5, 0.5, 0.5), prev_r_int=f(2.0, 2.0, 2.0), episode_reward=f(9.0, 9.0, 9.0))
    new, reset, live = R.begin_episodes(s, 4, b(1, 0, 1), 7, 5)
    assert new["prev_action"].tolist() == [3, 1, 2] and new["prev_r_ext"].tolist() == [0.0, 0.5, 0.0] and new["prev_r_int"].tolist() == [0.0, 2.0, 0.0]
    assert new["episode_reward"].tolist() == [0.0, 9.0, 0.0] and reset.tolist() == [1, 0, 1] and live.tolist() == [0, 1, 0]
    new, reset, live = R.begin_episodes(s, 1, None, 7, 5)  # done NULL: every lane; one action: always 0
    assert new["prev_action"].tolist() == [0, 0, 0] and new["episode_reward"].tolist() == [0.0, 0.0, 0.0] and reset.tolist() == [0, 0, 0] and live.tolist() == [1, 1, 1]


def test_gather_inputs_by_hand():
    """L = 2 slots of E = 3 lanes; rows (slot 1, env 2) and (slot 0, env 0)."""
    x = dict(x_r_int=np.array([[1, 2, 3], [4, 5, 6]], F32), x_prev_r_ext=np.array([[10, 20, 30], [40, 50, 60]], F32), x_prev_r_int=np.array([[.1, .2, .3], [.4, .5, .6]], F32),
             x_actor=np.array([[0, 1, 2], [2, 1, 0]], I32), x_prev_action=np.array([[7, 8, 9], [10, 11, 12]], I32))
    o = R.gather_inputs(np.array([2, 0]), np.array([1, 0]), i(3, 4), f(-1.0, -2.0), x, f(0.99, 0.98, 0.97))
    assert o["on_r_ext"].tolist() == [60.0, -1.0, 10.0, -2.0] and o["on_r_int"].tolist() == [F32(.6), 6.0, F32(.1), 1.0]
    assert o["on_action"].tolist() == [12, 3, 7, 4] and o["on_actor"].tolist() == [0, 0, 0, 0]
    assert o["tg_r_ext"].tolist() == [-1.0, -2.0] and o["tg_r_int"].tolist() == [6.0, 1.0] and o["tg_action"].tolist() == [3, 4] and o["tg_actor"].tolist() == [0, 0]
    assert o["discount"].tolist() == [F32(0.99), F32(0.99)] and o["r_int"].tolist() == [6.0, 1.0]


RECORD_E4 = bytes.fromhex(
    "01000000" "02000000" "03000000" "11000000"      # actions 1, 2, 3, 17 (int32, little endian)
    "0000803f" "000000c0" "0000003f" "00000000"      # rewards 1.0, -2.0, 0.5, 0.0
    "00010000"                                       # terminated 0, 1, 0, 0
    "00010001"                                       # done 0, 1, 0, 1
    "0000803e" "0000f841" "00008841" "000080bf" "0000403f"   # lane 0: r_int 0.25, arm 31, previous action 17, previous r_ext -1.0, previous r_int 0.75
    "00000000" "00000000" "00000000" "00000040" "00000000"   # lane 1: 0.0, 0, 0, 2.0, 0.0
    "0000c03f" "00004040" "00008040" "0000003f" "000000bf"   # lane 2: 1.5, 3, 4, 0.5, -0.5
    "00000041" "00008041" "0000a040" "00008040" "0000803f")  # lane 3: 8.0, 16, 5, 4.0, 1.0
X_E4 = dict(x_r_int=f(0.25, 0.0, 1.5, 8.0), x_actor=i(31, 0, 3, 16), x_prev_action=i(17, 0, 4, 5), x_prev_r_ext=f(-1.0, 2.0, 0.5, 4.0), x_prev_r_int=f(0.75, 0.0, -0.5, 1.0))


def test_packed_record_layout_byte_by_byte():
    rec = R.pack_record(i(1, 2, 3, 17), f(1.0, -2.0, 0.5, 0.0), b(0, 1, 0, 0), b(0, 1, 0, 1), X_E4)
    assert rec.dtype == U8 and len(rec) == 120 == R.RECORD_BYTES_PER_ENV * 4
    assert rec.tobytes() == RECORD_E4


def test_unpack_fields_by_hand():
    """Two records of 4 lanes, 124 bytes apart, into row (-2 mod 3) = 1 of [3][8] arrays; record 1 is record 0 with the lanes' fields reversed."""
    rev = {k: v[::-1].copy() for k, v in X_E4.items()}
    rec1 = R.pack_record(i(0, 0, 0, 0), f(0, 0, 0, 0), b(0, 0, 0, 0), b(0, 0, 0, 0), rev)
    buf = np.full(2 * 124, 0xA5, U8)
    buf[:120], buf[124:244] = np.frombuffer(RECORD_E4, U8), rec1
    ring = {k: np.full((3, 8), -9, v.dtype) for k, v in X_E4.items()}
    assert R.unpack_fields(buf, 2, 4, 124, -2, ring) == 1
    for k, v in X_E4.items():
        assert ring[k][1].tolist() == v.tolist() + v[::-1].tolist(), k
        assert (ring[k][0] == -9).all() and (ring[k][2] == -9).all(), k
    assert ring["x_actor"].dtype == I32 and ring["x_r_int"].dtype == F32


def test_priority_four_modes_on_two_rows():
    """target_ext (1.5, -2), Q_ext rows (.5, 1), (.25, -.5), actions (1, 0): td_ext = (.5, -2.25); target_int (.5, 1), Q_int rows (0, .25), (2, 0): td_int =
    (.25, -1); beta (2, .5): |.5 + 2 * .25| = 1, |-2.25 + .5 * -1| = 2.75.  Without Q rows the targets ARE the errors: |1.5 + 2 * .5| = 2.5, |-2 + .5 * 1| = 1.5."""
    te, qe, ti, qi = f(1.5, -2.0), np.array([[0.5, 1.0], [0.25, -0.5]], F32), f(0.5, 1.0), np.array([[0.0, 0.25], [2.0, 0.0]], F32)
    act, idx, beta = i(1, 0), i(2, 1), f(0.0, 0.5, 2.0)
    a, c, p = R.priority(te, qe, ti, qi, act, idx, beta)
    assert a.tolist() == [0.5, -2.25] and c.tolist() == [0.25, -1.0] and p.tolist() == [1.0, 2.75] and p.dtype == F32
    a, c, p = R.priority(te, qe, None, None, act, None, None)
    assert a.tolist() == [0.5, -2.25] and c is None and p.tolist() == [0.5, 2.25]
    a, c, p = R.priority(te, None, ti, None, None, idx, beta)
    assert a.tolist() == [1.5, -2.0] and c.tolist() == [0.5, 1.0] and p.tolist() == [2.5, 1.5]
    a, c, p = R.priority(te, None, None, None, None, None, None)
    assert a.tolist() == [1.5, -2.0] and c is None and p.tolist() == [1.5, 2.0]


def test_host_ucb_bank_walks_the_arms_once_then_follows_its_uniforms():
    """4 arms, window 9, epsilon 1: arms 0..3 in order whatever the uniforms; then floor(u1 * 4), and the largest double below 1 clamps to arm 3.  A lane that is
    not done keeps its arm."""
    bank = R.HostUcbBank(2, 4, 9, 1.0, 0.7)
    u = np.array([[0.5, 0.6, 0.0], [0.5, np.nextafter(1.0, 0.0), 0.0]])
    rows = [bank.step(None, np.zeros(2), u).tolist() for _ in range(5)]
    assert rows == [[0, 0], [1, 1], [2, 2], [3, 3], [2, 3]]
    assert bank.step(np.array([0, 1], np.uint8), np.zeros(2), np.array([[0.5, 0.0, 0.0], [0.5, 0.3, 0.0]])).tolist() == [2, 1]


def test_float64_and_float32_tail_references_agree_to_float32_rounding():
    """At the shape of tests/test_agent57_fast_gpu.py (B = 16, D = 32, Hd = 128, A = 6; RND: B = 16, D = 128).  Every sum here has at most 128 terms of like
    size: float32 (unit roundoff 6e-8) stays within 1e-5 of the tensor's largest entry -- the project's standing atol -- and the losses within 1e-5 relative."""
    import torch

    c = R.emb_case(16, 32, 128, 6, 21)
    r64, r32 = R.emb_reference(c, torch.float64), R.emb_reference(c, torch.float32)
    assert r32["loss"].dtype == torch.float32 and r64["loss"].dtype == torch.float64
    assert abs(float(r32["loss"]) - float(r64["loss"])) <= 1e-5 * float(r64["loss"])
    for name, a, w in [("d_emb", r32["d_emb"], r64["d_emb"])] + [(n, x, y) for n, x, y in zip(R.EMB_NAMES, r32["grads"], r64["grads"])]:
        assert float((a.double() - w).abs().max()) <= 1e-5 * float(w.abs().max()), name
        assert float(w.abs().max()) > 0, name
    c = R.rnd_case(16, 128, 22)
    r64, r32 = R.rnd_reference(c, torch.float64), R.rnd_reference(c, torch.float32)
    assert abs(float(r32["loss"]) - float(r64["loss"])) <= 1e-5 * float(r64["loss"])
    for k in ("d_h", "g_w", "g_b"):
        assert float((r32[k].double() - r64[k]).abs().max()) <= 1e-5 * float(r64[k].abs().max()), k
