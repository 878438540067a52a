"""tests/store_reference.py checked where there is no GPU: the completed store model is consistent with the pinned base class, and the scripted episode schedules
that tests/test_store_envelope_gpu.py runs really meet the edges they are there for (asserted on the model, per case; a schedule that misses one is changed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import store_reference as R  # noqa: E402
from store_reference import H  # noqa: E402
from test_hot_path_oracle_golden import replay_log_into_store  # noqa: E402

GOLDEN = os.path.join(R.ROOT, "tests", "golden")


def _effective_ends(m, done):
    """lanes whose `done` of this lock-step really ends an episode (a lane in its reset step ignores its inputs)."""
    return [e for e in range(m.E) if done[e] and not m.needs_reset[e]]


def _walk(g, planted=None):
    """Applies a geometry's events to the model, checks the model's consistency at every step and returns what the roll-out met.  With `planted` only items whose
    first transition lies at or after that position count as gathered (the GPU suite compares those alone)."""
    m = R.make_model(g)
    L, n = m.L, m.n
    tables = g.u8 or m.W == 1
    seen = dict(jd=set(), len1=False, two_ends=False, end_during_reset=False, truncated=False, short_terminal=False, minus_one=False, end_last_slot=False,
                end_slot0_after_wrap=False, resets=0, commits=0, gathers_on_full_ring=0, full_ring_before_reset=False, mid_run_reset=False, clamp_q0=False,
                before_first_commit=False, ahead=0, padded_q=[], q=[])
    for ev in R.events(g, planted):
        if ev[0] == "reset":
            seen["resets"] += 1
            seen["mid_run_reset"] |= seen["commits"] > 0
            seen["full_ring_before_reset"] |= seen["commits"] > 0 and bool(m.written.all())
        if ev[0] == "commit":
            a, r, term, done, nxt = ev[2]
            lead = ev[3] if ev[1] == "at" else 0
            own, p = m.pos, m.pos + lead  # (lagged mode: the commit lands at the host's position, `lead` ahead of the store's)
            seen["ahead"] += lead
            ends = _effective_ends(m, done)
            seen["two_ends"] |= len(ends) >= 2
            seen["end_during_reset"] |= bool(ends) and bool(m.needs_reset.any())
            for e in ends:
                seen["len1"] |= m.step_in_ep[e, p % L] == 0
                seen["truncated"] |= not term[e]
                seen["end_last_slot"] |= p % L == L - 1
                seen["end_slot0_after_wrap"] |= p % L == 0 and p >= L
            seen["commits"] += 1
            got = R.apply_to_model(m, ev)
            assert m.pos == own + (ev[1] in ("plain", "ex1"))
            if tables and got[1] is not None:  # the next pass's table is what frame_table_current gives once the position has moved there
                assert np.array_equal(got[1], m._table_at(p + 1))
            continue
        R.apply_to_model(m, ev)
        if ev[0] == "policy":
            # frames read from `obs` through the current table, normalised == stack_at
            np.testing.assert_array_equal(m.frames_from_table(m.frame_table_current()), m.stack_current())
        if ev[0] == "gather":
            idx = R.all_indices(m)
            it = m.gather_all(idx)
            env, slot, prev = m.locate_slots(idx)
            for b, ti in enumerate(idx):  # locate_slots agrees with locate
                e, q = m.locate(ti)
                assert (env[b], slot[b]) == (e, q % L) and q == it["q"][b]
                assert prev[b] == (-1 if m.step_in_ep[e, q % L] == 0 else (q - 1) % L)
            full = m.frame_tables(idx, 0, n + 1)
            np.testing.assert_array_equal(m.frames_from_table(full), it["obs"])  # == gather_item's observations, zero channels at -1 included
            for kb, kc in ((0, 1), (1, n), (n, 1)):
                np.testing.assert_array_equal(m.frame_tables(idx, kb, kc), full[:, kb:kb + kc])
            if seen["commits"] == 0 or m.pos == 0:
                seen["before_first_commit"] = True
            if m.written.all():
                seen["gathers_on_full_ring"] += 1
                for b in range(len(idx)):
                    jd, q = int(it["jd"][b]), it["q"][b]
                    if planted is not None and q < planted:
                        continue
                    seen["jd"].add(jd)
                    seen["q"].append(q)
                    seen["minus_one"] |= bool((full[b] < 0).any())
                    if jd < n and (full[b, jd + 1] < 0).any():  # the terminal state of an episode that ended with fewer than W frames
                        seen["short_terminal"] = True
                    if jd < n - 1:
                        seen["padded_q"].append(q)  # an item with padding actions, which are keyed on q
                    seen["clamp_q0"] |= q == 0
    seen["model"] = m
    return seen


@pytest.mark.parametrize("g", R.GEOMS, ids=R.GEOM_IDS)
def test_schedule_meets_its_edges_and_model_is_consistent(g):
    seen = _walk(g)
    m = seen["model"]
    L, n, W, E = m.L, m.n, m.W, m.E
    assert seen["commits"] == 2 * L + 3
    assert seen["resets"] == 2 and seen["mid_run_reset"]  # a reset_all happens mid-run
    # every ring slot has been written before the unfiltered comparisons start: the ring is full before the second reset_all already, and at least L + 1 gathers
    # of all items follow the first one made on a full ring
    assert seen["full_ring_before_reset"] and seen["gathers_on_full_ring"] >= L + 2
    assert seen["jd"] == set(range(n + 1)), sorted(seen["jd"])  # every jd in 0..n occurs among the gathered items
    assert seen["len1"]  # an episode of length 1
    assert seen["truncated"]  # a done without terminated
    assert seen["end_last_slot"] and seen["end_slot0_after_wrap"]  # an end in the last ring slot before a wrap, another in slot 0
    assert seen["before_first_commit"] and seen["clamp_q0"]
    if E >= 2:  # (what needs two lanes)
        assert seen["two_ends"] and seen["end_during_reset"]
    # An episode shorter than W frames: its terminal state s_{jd+1} has -1 offsets.  An episode has at least two frames, so W >= 3 (W = 4 in the case list)
    # is where one exists; at W = 2 the -1 offsets come from the first state of an episode alone, at W = 1 there is no history.
    if W >= 3:
        assert seen["short_terminal"]
    if W >= 2:
        assert seen["minus_one"]
    if g.mode == "at":  # the lagged arrangement: every commit but the first after a reset_all lands one ahead of the store's position
        assert g.slack == 1 and seen["ahead"] == 2 * L + 3 - 2


@pytest.mark.parametrize("bits", [31, 32])
@pytest.mark.parametrize("g", R.LARGE, ids=[g.name for g in R.LARGE])
def test_large_position_runs_hold_what_they_are_there_for(g, bits):
    """The planted runs have no second reset_all (it would rewind the position), so `a reset_all mid-run` does not apply, and only items that start at or after the
    planted position count.  Among those: every jd, items on both sides of 2^bits, and items beyond it that carry padding actions (keyed on the position's low
    32 bits); the schedule's other edges as in the plain runs."""
    L = R.ring_len(g)
    planted = R.planted_position(L, bits)
    assert planted % L == 0 and planted < 2 ** bits - L <= planted + L
    seen = _walk(g, planted)
    m = seen["model"]
    assert m.pos == planted + 2 * L + 3 and seen["resets"] == 1
    assert seen["jd"] == set(range(m.n + 1)), sorted(seen["jd"])
    assert min(seen["q"]) < 2 ** bits <= max(seen["q"])
    assert any(q >= 2 ** bits for q in seen["padded_q"]) and any(q < 2 ** bits for q in seen["padded_q"])
    assert seen["len1"] and seen["truncated"] and seen["two_ends"] and seen["end_during_reset"] and seen["minus_one"]
    assert seen["end_last_slot"] and seen["end_slot0_after_wrap"]


def test_the_other_gpu_runs_hold_what_they_are_there_for():
    """The runs of tests/test_store_envelope_gpu.py outside GEOMS and what is asserted of each (the actor-priority store has its own test below).
    * The packed commit and the gather_train edges use the first phase of a schedule without its reset_all: record decoding and the workgroup edge are their subject.
      Asserted: completed and uncompleted items (both mask values), terminations and truncations, lanes in their reset step, every jd, a full ring.
    * The two grid-cap runs last 2 and W + 2 lock-steps: their subject is the grid-stride loop.  Asserted: the sizes are the smallest past their caps, and lanes 0
      and 1 end at once so that masks, reset steps and zero history occur in them.  Ring wrap, jd coverage and the mid-run reset do not apply to runs that short.
    * The synthetic-environment runs follow the environment's own episodes (length 4), not a scripted schedule.  Asserted: episodes end, lanes pass through their
      reset step while others act, and from the second lock-step on the host's position is one ahead of the store's."""
    for g, steps_of in ((R.PACKED_GEOM, lambda L: 2 * L + 3), (R.GEOMS[0], None)):
        m = R.make_model(g)
        firsts, steps, t_reset = R.inputs(g)
        m.reset_all(firsts[0])
        masks, jds, trunc, term_, resetting = set(), set(), False, False, False
        for s in steps[:t_reset if steps_of is None else steps_of(m.L)]:
            ends = _effective_ends(m, s[3])
            trunc |= any(not s[2][e] for e in ends)
            term_ |= any(s[2][e] for e in ends)
            resetting |= bool(m.needs_reset.any())
            masks |= set(int(v) for v in m.commit_step(*s))
            jds |= set(int(j) for j in m.gather_all(R.all_indices(m))["jd"])
        assert masks == {0, 1} and trunc and term_ and resetting and jds == set(range(m.n + 1)) and m.written.all()
    g = R.CAP_NO_ADVANCE
    assert (g.E - 1) * (g.F // 16 + 1) <= 2048 * 256 < g.E * (g.F // 16 + 1)
    g = R.CAP_F32
    assert g.E * g.W * g.F // 4 == 256 * 32 * 256 + 1 and 65 * 2 * g.W * (g.F // 4) > 256 * 32 * 256 >= 64 * 2 * g.W * (g.F // 4)
    for g in (R.CAP_NO_ADVANCE, R.CAP_F32):
        term, done, _ = R.schedule(g.E, R.ring_len(g), g.n, g.W)
        assert done[0, :2].all() and not done[0, 2:].any() and not done[1, :2].any()
    for u8, F in R.SYNTH_SHAPES:
        g = R.SYNTH_GEOM(u8, F)
        m = R.make_model(g)
        m.reset_all(np.zeros((g.E, F), np.uint8 if u8 else np.float32))
        ends = resets_beside_actors = 0
        for step in range(2 * m.L + 3):
            host = m.pos + (1 if step else 0)
            nxt, rew, term, done = R.synth_at(m, host)
            resets_beside_actors += bool(m.needs_reset.any() and not m.needs_reset.all())
            ends += int(done.sum())
            m.commit_step(np.full(g.E, step % 5, np.int32), rew, term, done, nxt, position=host)
            if step:
                m.advance()
            assert m.pos == host - (1 if step else 0) + (1 if step else 0) and (host == m.pos if step else host == m.pos == 0)
        assert g.slack == 1 and ends >= g.E and (u8 or not (nxt == 0).all())


@pytest.mark.parametrize("n", [1, 2, 5, 16, 17, 1000])
def test_permutation_model(n):
    """rng_permutation is a permutation, keyed on seed and counter, and the batched form's y-th row is the single form's at counter + y.  At n = 2 the network
    is spelled out by hand: one bit per half, four rounds of (l, r) -> (r, l ^ f(r))."""
    p = R.rng_permutation(4242, 9, n)
    assert p.dtype == np.int64 and sorted(p) == list(range(n))
    if n > 2:
        assert not np.array_equal(p, R.rng_permutation(4242, 10, n)) or n < 5
    np.testing.assert_array_equal(R.rng_permutations(4242, 9, n, 3)[2], R.rng_permutation(4242, 11, n))
    if n == 2:
        want = []
        for x in range(2):
            while True:
                left, right = x >> 1, x & 1
                for rnd in range(4):
                    f = int(H.rng_u64((4242 + 0x9E3779B97F4A7C15 * (rnd + 1)) % 2 ** 64, np.uint64(9), np.uint64(right))) & 1
                    left, right = right, left ^ f
                x = (left << 1) | right
                if x < 2:
                    break
            want.append(x)
        assert list(p) == want


@pytest.mark.parametrize("name", ["terminated", "truncated"])
def test_subclass_replays_the_golden_rollouts_like_the_base_class(name):
    z = np.load(os.path.join(GOLDEN, f"rollout_items_{name}.npz"))
    base = H.StoreOracle(1, 128, 64, 4, 3, 4, True, 123)
    sub = R.StoreModel(1, 128, 64, 4, 3, 4, True, 123)
    replay_log_into_store(z, base)
    replay_log_into_store(z, sub)
    for k in ("obs", "action", "reward", "flags", "step_in_ep", "needs_reset"):
        np.testing.assert_array_equal(getattr(sub, k), getattr(base, k))
    assert sub.pos == base.pos and sub.item_len == base.item_len
    valid = [q for q in range(sub.pos) if not (sub.flags[0, q] & sub.INVALID)]
    n_items = z["item_obs"].shape[0]
    for i in range(n_items):
        obs, act, rew, ter, jd = sub.gather_item(0, valid[i])
        np.testing.assert_array_equal(obs, z["item_obs"][i])
        np.testing.assert_array_equal(rew, z["item_rewards"][i])
        np.testing.assert_array_equal(ter, z["item_terminated"][i])
        np.testing.assert_array_equal(act[:min(jd + 1, 3)], z["item_actions"][i][:min(jd + 1, 3)])
        ti = ((valid[i] + sub.n - 1) % sub.item_len) + sub.N - 1
        if sub.locate(ti) == (0, valid[i]):  # (still in the ring's live range): the recorded frames through the offset table
            np.testing.assert_array_equal(sub.frames_from_table(sub.frame_tables([ti], 0, sub.n + 1))[0], z["item_obs"][i])


@pytest.mark.parametrize("per,k,pad", [(4, 0, 0), (4, 1, 8), (8, 3, 0), (8, 1, 36)])
def test_pack_records_round_trips(per, k, pad):
    rng = np.random.default_rng(per * 10 + k)
    E = 16
    a = rng.integers(-3, 9, E).astype(np.int32)
    r = rng.standard_normal(E).astype(np.float32)
    t, d = (rng.random(E) < 0.5).astype(np.uint8), (rng.random(E) < 0.5).astype(np.uint8)
    x = rng.standard_normal((E, k)).astype(np.float32)
    stride = (10 + 4 * k) * per + pad
    rec = R.StoreModel.pack_records(a, r, t, d, x, per, stride)
    assert rec.shape == (E // per, stride) and rec.dtype == np.uint8
    assert not rec[:, (10 + 4 * k) * per:].any()
    # the documented byte layout, spelled out for one environment
    e = per + 1
    assert rec[1, 4:8].view(np.int32)[0] == a[e] and rec[1, 4 * per + 4:4 * per + 8].view(np.float32)[0] == r[e]
    assert rec[1, 8 * per + 1] == t[e] and rec[1, 9 * per + 1] == d[e]
    if k:
        assert rec[1, 10 * per + 4 * k:10 * per + 4 * k + 4].view(np.float32)[0] == x[e, 0]
    for got, want in zip(R.StoreModel.unpack_records(rec, per, k), (a, r, t, d, x)):
        np.testing.assert_array_equal(got, want)


def test_packed_commit_equals_the_separate_array_commit_and_fills_the_estimate_column():
    g = R.PACKED_GEOM
    firsts, steps, _ = R.inputs(g)
    m, ref = R.make_model(g), R.make_model(g)
    m.reset_all(firsts[0])
    ref.reset_all(firsts[0])
    rng = np.random.default_rng(5)
    for t, (a, r, term, done, nxt) in enumerate(steps[:8]):
        x = rng.standard_normal((g.E, 1)).astype(np.float32)
        rec = m.pack_records(a, r, term, done, x, 4, 64)
        mask, est = m.commit_step_packed(rec, 4, 1, nxt, est_records=rec if t % 2 else None)
        np.testing.assert_array_equal(mask, ref.commit_step(a, r, term, done, nxt))
        np.testing.assert_array_equal(est, np.where(mask == 0, -2.0, x[:, 0] if t % 2 else -1.0).astype(np.float32))
        for k in ("obs", "action", "reward", "flags", "step_in_ep", "needs_reset"):
            np.testing.assert_array_equal(getattr(m, k), getattr(ref, k))
    with pytest.raises(ValueError):
        m.commit_step_packed(rec, 6, 1, nxt)


def test_slack_and_refusals_of_the_model():
    with pytest.raises(ValueError):
        R.StoreModel(2, 5, 4, 2, 3, 3, True, 1)  # ring_len == n_step + window
    m = R.StoreModel(2, 8, 4, 2, 3, 3, True, 1)
    assert (m.item_len, m.per_capacity()) == (3, 6)
    m.set_item_slack(2)
    assert (m.item_len, m.per_capacity()) == (1, 2)
    with pytest.raises(ValueError):
        m.set_item_slack(3)
    m.reset_all(np.zeros((2, 4), np.uint8), pos=8 * 12345678901)
    assert m.pos == 8 * 12345678901 and m.frame_offset(1, m.pos, 1) == (1 * 8 + 0) * 4


def _actor_td_by_hand(rows, act, rew, ter, discount, h, rescale):
    """rainbow.py:185-287 for one item with the online rows in both roles, written out term by term in Python floats (float64), without nstep_target:
    target = sum_k discount^k c_k (gain_k - [k > 0] Q(s_k, a_k)), gain_k = r_k + (1 - ter_k) discount max Q(s_{k+1}), c_k = prod_{j=1..k} h [a_j == argmax Q(s_{j+1})]."""
    n = len(act)
    target, c = 0.0, 1.0
    for k in range(n):
        nxt = [float(v) for v in rows[k + 1]]
        greedy = nxt.index(max(nxt))
        maxq = nxt[greedy]
        if rescale:
            maxq = float(H.inverse_rescaling(np.float64(maxq)))
        gain = float(rew[k]) + (1.0 - float(ter[k])) * discount * maxq
        if rescale:
            gain = float(H.rescaling(np.float64(gain)))
        if k > 0:
            c *= h * (1.0 if int(act[k]) == greedy else 0.0)
        target += discount ** k * c * (gain - (float(rows[k][act[k]]) if k > 0 else 0.0))
    return abs(target - float(rows[0][act[0]]))


def test_actor_td_is_the_reference_formula():
    """The golden actor_priority_{n1,n3}.npz hold the network's weights, the action log and the priorities the reference's worker computed -- no Q rows.  The rows
    would have to come from a forward pass of the image network on the stacked frames of the recorded episodes, which is no part of the store and is what
    tests/test_plugin_gpu.py::test_distributed_actor_initial_priorities_match_the_reference checks end to end; actor_td cannot be fed from these files alone.
    Checked here instead: actor_td in float64 equals |calc_target_q([item]) - q[action]| (rainbow.py:389-398) written out by hand above, without nstep_target, with
    and without rescale and retrace, on a roll-out with masked lanes and windows that hold an episode end; and its float32 evaluation is nstep_target's float32,
    which tests/test_hot_path_oracle_golden.py pins bit for bit against the recorded calc_target_q."""
    g = R.Geom("td", True, 16, 1, 3, 3, 6, 0, "plain")
    firsts, steps, _ = R.inputs(g)
    m = R.make_model(g, clip=False)
    m.reset_all(firsts[0])
    rng = np.random.default_rng(3)
    codes = set()
    for t, s in enumerate(steps[:9]):
        mask = m.commit_step(*s)
        mask[t % g.E] = 0
        qh = rng.standard_normal((g.n + 1, g.E, R.N_ACTIONS)).astype(np.float32)
        base = t % (g.n + 1)
        first_slot = (t * g.E) % m.per_capacity()
        for h, rescale in ((0.9, False), (1.0, True), (0.0, False)):
            got = m.actor_td(qh, base, first_slot, mask, 0.99, h, rescale, np.float64)
            got32 = m.actor_td(qh, base, first_slot, mask, 0.99, h, rescale, np.float32)
            assert got.dtype == np.float64 and got32.dtype == np.float32
            for e in range(g.E):
                if not mask[e]:
                    assert got[e] == -2 and got32[e] == -2
                    codes.add(-2)
                    continue
                obs, act, rew, ter, jd = m.gather_item(e, max(m.pos - g.n, 0))
                if jd < g.n:
                    assert got[e] == -1 and got32[e] == -1
                    codes.add(-1)
                    continue
                rows = np.stack([qh[(base + k) % (g.n + 1), e] for k in range(g.n + 1)])
                np.testing.assert_allclose(got[e], _actor_td_by_hand(rows, act, rew, ter, 0.99, h, rescale), rtol=1e-12, atol=1e-12)
                want32 = np.abs(H.nstep_target(rows[None, 1:], rows[None, 1:], act[None], rew[None], ter[None], None, 0.99, h, True, rescale)[0] - rows[0, act[0]])
                assert got32[e] == want32 and got32[e] >= 0
                codes.add(0)
    assert codes == {-2, -1, 0}


@pytest.mark.parametrize("A", R.ACTOR_TD_A)
@pytest.mark.parametrize("n", R.ACTOR_TD_N)
def test_actor_td_cases_hold_what_they_are_there_for(n, A):
    """The cases tests/test_store_envelope_gpu.py::test_actor_td runs: both codes occur, masked lanes occur, values occur, and from n = 2 up there are rows whose
    taken actions are all greedy (retrace_h = 1 keeps every term) and rows where one is not (the later terms vanish).  Also: float32 is within the standing
    tolerance's reach of float64, so the GPU comparison is one of values, not of codes alone."""
    m = R.actor_td_model(n, A)
    codes, greedy, evaluations = set(), set(), 0
    for t, (s, ev) in enumerate(R.actor_td_case(n, A)):
        if ev is None and t == 0:
            m.reset_all(s)
            continue
        mask = m.commit_step(*s)
        if ev is None:
            continue
        ev = R.actor_td_finish(m, ev)
        mask[ev["mask_zero"]] = 0
        assert (mask == 0).any() and (mask != 0).any()
        qh, base = ev["q_hist"], ev["base_slot"]
        assert ev["first_slot"] == ((m.pos - 1) * m.E) % m.per_capacity() and 0 <= base <= n
        for rescale in (False, True):
            w64 = m.actor_td(qh, base, ev["first_slot"], mask, 0.99, 1.0, rescale, np.float64)
            w32 = m.actor_td(qh, base, ev["first_slot"], mask, 0.99, 1.0, rescale, np.float32)
            assert w32.dtype == np.float32 and np.array_equal(w64 < 0, w32 < 0) and np.array_equal(w64[w64 < 0], w32[w32 < 0])
            codes |= set(int(c) for c in w64[w64 < 0])
            assert (w64 >= 0).sum() >= 4
            # (a bound on the MODEL, not a tolerance for the kernel: check_tensor's second clause admits twice the model's float32 error, so that error must be a
            # rounding error -- at most 500 float32 roundings of an O(10) value through inverse_rescaling's division by 2 * 0.001 -- and not a different quantity)
            np.testing.assert_allclose(w32[w64 >= 0], w64[w64 >= 0], rtol=1e-3, atol=1e-3)
        w0 = m.actor_td(qh, base, ev["first_slot"], mask, 0.99, 0.0, False, np.float64)
        w1 = m.actor_td(qh, base, ev["first_slot"], mask, 0.99, 1.0, False, np.float64)
        for e in np.nonzero(w1 >= 0)[0]:
            act = m.gather_item(int(e), m.pos - n)[1]
            rows = [qh[(base + k) % (n + 1), e] for k in range(n + 1)]
            greedy.add(all(act[k] == int(np.argmax(rows[k + 1])) for k in range(1, n)))
        if n >= 2:
            assert not np.array_equal(w0, w1)  # retrace_h matters
        evaluations += 1
    assert evaluations == 2 and codes == {-2, -1}
    assert greedy == ({True, False} if n >= 2 else {True})
