"""What tests/train_kernels_reference.py promises about its cases, checked on the oracle alone (no GPU): a GPU test that compares a kernel with the oracle on
these inputs can only notice a wrong tie-break, a wrong retrace cut, a wrong Huber region or a wrong neighbour if the inputs contain one -- so each of those
is counted here.  Also here: the order of operations csrc/srlx_td_math.h states, restated in float32 numpy, is the oracle's at every n, and the order it
replaced was not from 8 terms up."""
import numpy as np
import pytest

import train_kernels_reference as R
from train_kernels_reference import F32, H


# ---- the thinned cross products --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes,cases,allowed", [(R.NSTEP_AXES, R.NSTEP_CASES, None), (R.DQN_AXES, R.DQN_CASES, R._dqn_allowed), (R.GAE_AXES, R.GAE_CASES, None),
                                                (R.SEQ_AXES, R.SEQ_CASES, None)], ids=["nstep", "dqn", "gae", "seq"])
def test_every_value_meets_every_value_of_every_other_axis(axes, cases, allowed):
    allowed = allowed or (lambda c: True)
    want = R.all_pairs(axes, allowed)
    names = list(axes)
    got = set()
    for c in cases:
        assert allowed(c)
        got |= {((a, repr(c[a])), (b, repr(c[b]))) for i, a in enumerate(names) for b in names[i + 1:]}
    assert got == want
    assert len(cases) < 60, len(cases)  # thinned: the full products have 1728, 720, 288 and 360 members
    print("%d cases cover %d pairs" % (len(cases), len(want)))


# ---- 1. n-step TD ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.NSTEP_CASES + R.NSTEP_ORDER_CASES + R.NSTEP_FINITE_CASES, ids=R.case_id)
def test_nstep_case_conditions(c):
    d = R.nstep_case(c)
    B, n, A = c["B"], c["n"], c["A"]
    sel = d["q_on"] if c["dd"] else d["q_tg"]
    assert (sel * 4 == np.round(sel * 4)).all() and (d["q_tg"] * 4 == np.round(d["q_tg"] * 4)).all()  # multiples of 0.25
    if A >= 2:
        share = R.tied(sel, d["inv"]).mean()
        assert share >= 1 / 3, share
    if c["mask"]:
        # one all-invalid step, in row 0, or none (with a single action, row 1's step with action 0 invalid is a second one)
        assert d["inv"].all(axis=2).sum() == c.get("whole", 1) + (A == 1 and B >= 2) and d["inv"][0, 0].all() == c.get("whole", 1)
        if B >= 2:
            assert d["inv"][1, n - 1, 0] and (A == 1 or not d["inv"][1, n - 1, 1:].any())
    else:
        assert d["inv"] is None
    cut = R.first_cut(c, d)
    if A >= 2 and B >= n:
        assert cut[0] == n  # greedy throughout
        for m in range(1, n):
            assert cut[m] == m, (m, cut[m])
        assert set(range(1, n + 1)) <= set(cut.tolist())
    elif A == 1:
        assert (cut == n).all()  # one action: always greedy
    if n >= 2 and B >= 2:
        assert d["done"][B - 1, 0] == 1.0 and d["done"][:, : n - 1].any()
    if B >= 2:
        assert d["w"][0] == 0.0 and d["w"].max() > 1.0
    if B >= 255:
        target = R.nstep_oracle(c, d)
        q0 = d["q0"][np.arange(B), d["act"][:, 0]]
        diff = target * d["w"] - q0 * d["w"]
        with np.errstate(invalid="ignore"):
            shares = [(np.abs(diff) < 1).mean(), (diff > 1).mean(), (diff < -1).mean()]
        assert min(shares) >= 0.25, shares
        if not c["mask"] or c["dd"] or not c.get("whole", 1):
            assert np.isfinite(target).all()
        else:  # the all-invalid step without double DQN reads -inf from the masked target net, as in the reference
            assert not np.isfinite(target[0])


@pytest.mark.parametrize("c", R.NSTEP_CASES + R.NSTEP_ORDER_CASES + R.NSTEP_FINITE_CASES, ids=R.case_id)
def test_nstep_kernel_order_is_the_oracle_order(c):
    """td_rows' order of operations, restated, against hot_path_oracle.nstep_target in float32: the same bits without rescale at every n (with rescale the
    oracle's np.sqrt runs on float32 arrays where the kernel rounds a float64 square root once: the bar, and the bit-equal share printed)."""
    d = R.nstep_case(c)
    want = R.nstep_oracle(c, d)
    got = R.nstep_target_in_kernel_order(c, d)
    want64 = R.nstep_oracle(c, d, np.float64)
    if c["rs"]:
        print("bit-equal share %.3f" % R.bit_equal_share(got, want))
        R.check("target", got, want, R.RTOL, 1e-6, want64, R.case_id(c))
    else:
        R.same_bits(got, want.astype(F32), R.case_id(c))


def test_the_sequential_order_differs_from_8_terms_up():
    """The inputs can tell the two orders apart: below 8 terms they are one order, from 8 up a share of the rows differs in the last bit."""
    for c in R.NSTEP_ORDER_CASES:
        d = R.nstep_case(c)
        want = R.nstep_oracle(c, d)
        seq = R.nstep_target_in_kernel_order(c, d, pairwise=False)
        share = R.bit_equal_share(seq, want)
        print("n=%d dd=%d: sequential sum bit-equal to the oracle in %.0f %% of the rows" % (c["n"], c["dd"], 100 * share))
        if c["n"] < 8:
            assert share == 1.0
        else:
            assert share < 0.9, (c, share)


# ---- 2. DQN target ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.DQN_CASES, ids=R.case_id)
def test_dqn_case_conditions(c):
    d = R.dqn_case(c)
    B, A = c["B"], c["A"]
    net = d["q_on"] if c["dd"] else d["q_tg"]
    assert np.argmin(net) == B * A - 1 and (net.reshape(-1)[:-1] > net[B - 1, A - 1]).all()  # one minimum, in the last row
    if c["mask"] == "none":
        assert d["inv"] is None
    else:
        if B >= 2:
            assert not d["inv"][B - 1].any()  # the minimum decides other rows than its own
        assert d["inv"].all(axis=1).any() == (c["mask"] == "rows")
    if A >= 2 and B >= 255:
        assert R.tied(net, None).mean() >= 1 / 3
    want = R.dqn_oracle(c, d)
    assert want.dtype == F32 and np.isfinite(want).all()
    if B >= 255 and c["mask"] == "rows" and not c["dd"]:  # the value of the minimum matters: with another one the wholly invalid rows come out differently
        e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        e["q_tg"][B - 1, A - 1] = -9.0
        whole = d["inv"].all(axis=1) & (d["undone"] > 0)
        assert whole.sum() >= 10 and (R.dqn_oracle(c, e)[whole] != want[whole]).all()


def test_dqn_minimum_inside_a_masked_entry():
    c = dict(B=257, A=18, dd=1, rs=0, f64=0, ps=0, mask="some")
    d = R.dqn_case(c, min_masked=True)
    assert d["inv"][256, 17] and d["q_on"][256, 17] == d["q_on"].min() == -3.0


# ---- 5. sequence TD --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.SEQ_CASES + R.SEQ_FINITE_CASES, ids=R.case_id)
def test_seq_case_conditions(c):
    d = R.seq_case(c)
    B, S, A = c["B"], c["S"], c["A"]
    if B * S >= 255 and A >= 2:
        share = (d["act"] == d["greedy"]).mean()
        assert 0.6 <= share <= 0.9, share  # 70 % by choice, and a random action is the greedy one now and then
        assert R.tied(d["q"][:, 1:] if c["dd"] else d["qt"][:, 1:], d["inv"]).mean() >= 1 / 3
    assert d["dones"][B - 1, 0] == 0.0
    if S >= 2 and B >= 255:
        assert (d["dones"][:, : S - 1] == 0).any()  # zeros mid-sequence
    if c["mask"]:
        whole = d["inv"].all(axis=2)
        assert whole.sum() == (0 if c["dd"] else c.get("whole", 1)), c
        if not c["dd"] and c.get("whole", 1):
            assert whole[0, S - 1]
    with np.errstate(invalid="ignore"):
        want = H.agent57_seq_target(d["q"], d["qt"], d["act"], d["rew"], d["dones"], d["inv"], d["disc"], 0.95, bool(c["dd"]), bool(c["rs"]))
    assert want.shape == (S, B)
    assert np.isfinite(want).all() == (not (c["mask"] and not c["dd"] and c.get("whole", 1))), c


# ---- 6. lifelong -----------------------------------------------------------------------------------------------------------------------------------------------
def test_lifelong_rows_clip_at_both_ends():
    for n in R.LIFELONG_N:
        for Dm in R.LIFELONG_D:
            t, p = R.lifelong_case(n, Dm)
            want = H.ngu_lifelong_reward(t, p, R.LIFELONG_MAX)
            assert want[0] == 1.0
            if n >= 3:
                assert 1.0 < want[1] < R.LIFELONG_MAX and want[2] == F32(R.LIFELONG_MAX)


# ---- 7. episodic memory ----------------------------------------------------------------------------------------------------------------------------------------
def test_episodic_cases_reach_what_they_are_for():
    for name, c in R.EPISODIC_CASES.items():
        assert R.ngu_split(c["E"], c["cap"]) == c["split"], name
    per_thread = lambda name: -(-min(R.EPISODIC_CASES[name]["T"] - 1, R.EPISODIC_CASES[name]["cap"]) // (256 * R.EPISODIC_CASES[name]["split"]))  # noqa: E731
    assert per_thread("a") == 4 and R.EPISODIC_CASES["a"]["T"] - R.EPISODIC_CASES["a"]["cap"] == 276
    assert per_thread("b") == 17 and R.EPISODIC_CASES["b"]["T"] > R.EPISODIC_CASES["b"]["cap"]  # more than the 16 slots of a thread's list
    assert R.EPISODIC_CASES["c"]["k"] == 16 and R.EPISODIC_CASES["c"]["T"] > R.EPISODIC_CASES["c"]["cap"]
    assert R.EPISODIC_CASES["d"]["T"] - 1 > 16 * 256  # the stride loop's second round
    emb = R.episodic_embeddings("f")
    assert len(np.unique(emb.reshape(-1, 3), axis=0)) == 5
    want = R.episodic_expected("f", emb)
    assert np.isfinite(want).all() and len(np.unique(want)) > 5 and (want[300:] == want[-1]).all()  # ten exact zeros: ave == 0


def test_episodic_case_h_fills_one_thread_to_its_last_slot():
    """From the 17th near embedding on, the 16 nearest entries of a near query sit at ring slots of one residue mod 256 -- one thread of the single workgroup
    -- and a 17th near entry is live as well once the ring is full; dropping the 16th neighbour for the nearest far entry moves the reward by far more than
    the bar."""
    c = R.EPISODIC_CASES["h"]
    assert c["cap"] % 256 == 0 and c["cap"] // 256 == 17 and c["k"] == 16 and R.ngu_split(c["E"], c["cap"]) == 1
    x = R.episodic_embeddings("h")[:, c["lanes"][0], 0]
    checked = 0
    for t in range(5 + 16 * 256, c["T"], 256):
        lo = max(0, t - c["cap"])
        dist = np.abs(x[lo:t] - x[t])
        order = np.argsort(dist, kind="stable")
        assert (((order[:16] + lo) % c["cap"]) % 256 == 5).all(), t
        if t - lo == c["cap"]:
            assert ((order[16] + lo) % c["cap"]) % 256 == 5  # 17 near entries live: one more than the list holds
        full = float(H.ngu_episodic_from_distances(dist, 16, *R.NGU_CONSTANTS))
        far = np.sort(dist[(np.arange(lo, t) % 256) != 5])[0]
        short = float(H.ngu_episodic_from_distances(np.concatenate([np.sort(dist)[:15], [far]]), 16, *R.NGU_CONSTANTS))
        assert abs(short - full) / full > 1e-3, (t, full, short)
        checked += 1
    assert checked >= 2


@pytest.mark.parametrize("name", ["a", "c", "e1", "e256", "f", "g"])
def test_the_ring_form_of_the_episodic_oracle_is_the_oracle(name):
    """RingEpisodicOracle (what the GPU module steps, for speed) gives EpisodicMemoryOracle's bits at every step: first step, fewer than k entries, a full
    ring overwritten (a, c), exact zero distances (f), a reset (g)."""
    emb = R.episodic_embeddings(name)
    R.same_bits(R.episodic_expected(name, emb), R.episodic_expected(name, emb, H.EpisodicMemoryOracle), name)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_the_reward_is_a_witness_of_one_wrong_neighbour(name):
    """The reward depends on the k nearest distances only through the pseudo-count formula; with these constants and this data it moves by ten times the bar
    when any one neighbour is exchanged, at half of the checked steps at least."""
    passed, checked = R.knn_sensitivity(name, R.episodic_embeddings(name), lane=R.EPISODIC_CASES[name]["lanes"][-1])
    print("case %s: %d of %d checked steps (%.0f %%) move the reward by 1e-4 under each single-neighbour change" % (name, passed, checked, 100.0 * passed / checked))
    assert checked >= 100 and passed >= 0.5 * checked, (passed, checked)
