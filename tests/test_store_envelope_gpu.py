"""Every entry point of csrc/srlx_rollout.hip through the C ABI against tests/store_reference.py (the store model), over the envelope the kernels admit.
Integer, byte, mask, offset and float32-frame outputs are bit-equal; the actor-side priority follows tests/lstm_reference.py::check_tensor.  Every output is
allocated with a sentinel row past its end that must stay untouched.  tests/test_store_envelope_cpu.py asserts that the scripted schedules used here meet the
edges they are there for.

Left out, and why: the handle's create, destroy and accessors have no case of their own (every case goes through them); a shape that needs an unaligned or out-of-contract pointer (the C ABI takes whole tensors); the int64 division arm of item_meta (N >= 2^31
items: a ring of that many slots does not fit a test); the `frames >= 2^31` fall-backs of stack_current / gather_nstep for 16-byte uint8 frames (2^31 workgroups)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import store_reference as R  # noqa: E402
from store_reference import H  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = {"float32": -12345.0, "float64": -12345.0, "int32": -12345, "int64": -12345, "uint8": 0xA5}


def _env():
    import torch

    from simple_distributed_rl_amd import _native as N

    return N, N.lib(), torch, torch.device("cuda:0")


def _guarded(rows, rest, dtype):
    """[rows + 1, *rest] filled with the sentinel: the kernels own the first `rows` rows, the last one must stay as it is (tests/test_lstm_gpu.py::_guard_ok)."""
    N, lib, torch, dev = _env()
    return torch.full((rows + 1,) + tuple(rest), SENT[str(dtype).split(".")[-1]], dtype=dtype, device=dev)


def _take(name, t, rows):
    sent = SENT[str(t.dtype).split(".")[-1]]
    assert bool((t[rows:] == sent).all()), (name, "the row past the end was written")
    return t[:rows].cpu().numpy()


def _untouched(name, t):
    assert bool((t == SENT[str(t.dtype).split(".")[-1]]).all()), (name, "a refused call wrote its output")


class _DevI64:
    """int64 device memory behind a raw pointer, for torch.as_tensor (test-side only: the ring position of srlx_store_views)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<i8", data=(int(ptr), False), version=2)


class Dev:
    def __init__(self, m):
        N, lib, torch, dev = _env()
        self.N, self.lib, self.tt, self.dev, self.m = N, lib, torch, dev, m
        self.E, self.L, self.F, self.W, self.n, self.u8 = m.E, m.L, m.F, m.W, m.n, m.u8
        self.h = N.c_p()
        N.check(lib.srlx_store_create(ctypes.byref(self.h), m.E, m.L, m.F, N.OBS_U8 if m.u8 else N.OBS_F32, m.W, m.n, m.A, int(m.reward_clip), int(m.seed), 0))
        if m.slack:
            N.check(lib.srlx_store_set_item_slack(self.h, m.slack))
        self.fdt = torch.uint8 if m.u8 else torch.float32
        self.bump = _guarded(1, (), torch.int64)
        self.bump[0] = 7
        self.bumps = 7

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.srlx_store_destroy(self.h)
            self.h = None

    def T(self, x, dtype):
        return self.tt.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.dev)

    def sync(self):
        self.tt.cuda.synchronize()

    def pos_tensor(self):
        p = self.N.c_p()
        self.N.check(self.lib.srlx_store_views(self.h, ctypes.byref(p), None, None))
        return self.tt.as_tensor(_DevI64(p.value, 1), device=self.dev)

    def position(self):
        self.sync()
        return int(self.pos_tensor()[0].item())

    def plant(self, pos):
        t = self.pos_tensor()
        t[0] = pos
        self.sync()
        assert self.position() == pos  # read back before going on

    def reset_all(self, first):
        f = self.T(first, self.fdt)
        self.N.check(self.lib.srlx_store_reset_all(self.h, self.N.tptr(f), None))
        self.sync()

    def advance(self):
        self.N.check(self.lib.srlx_store_advance(self.h, None))
        self.sync()

    def stack_current(self):
        out = _guarded(self.E, (self.W, self.F), self.tt.float32)
        self.N.check(self.lib.srlx_store_stack_current(self.h, self.N.tptr(out), None))
        self.sync()
        return _take("stack_current", out, self.E)

    def frame_table_current(self):
        out = _guarded(self.E, (self.W,), self.tt.int64)
        self.N.check(self.lib.srlx_store_frame_table_current(self.h, self.N.tptr(out), None))
        self.sync()
        return _take("frame_table_current", out, self.E)

    def commit(self, kind, s, tables, position=None):
        """Returns (item mask, next frame table or None)."""
        tt, N = self.tt, self.N
        a, r, t_, d, o = self.T(s[0], tt.int32), self.T(s[1], tt.float32), self.T(s[2], tt.uint8), self.T(s[3], tt.uint8), self.T(s[4], self.fdt)
        mask = _guarded(self.E, (), tt.uint8)
        nt = _guarded(self.E, (self.W,), tt.int64) if (tables and kind != "plain") else None
        if kind == "plain":
            N.check(self.lib.srlx_store_commit_step(self.h, N.tptr(a), N.tptr(r), N.tptr(t_), N.tptr(d), N.tptr(o), N.tptr(mask), None))
        elif kind in ("ex0", "ex1"):
            N.check(self.lib.srlx_store_commit_step_ex(self.h, N.tptr(a), N.tptr(r), N.tptr(t_), N.tptr(d), N.tptr(o), N.tptr(mask), N.tptr(nt), int(kind == "ex1"),
                                                       N.tptr(self.bump), None))
            self.bumps += 1
        else:
            N.check(self.lib.srlx_store_commit_step_at(self.h, int(position), N.tptr(a), N.tptr(r), N.tptr(t_), N.tptr(d), N.tptr(o), N.tptr(mask), N.tptr(nt),
                                                       N.tptr(self.bump), None))
            self.bumps += 1
        self.sync()
        assert _take("bump", self.bump, 1)[0] == self.bumps  # `bump` advances by exactly one
        return _take("item_mask", mask, self.E), (None if nt is None else _take("next_table", nt, self.E))

    def commit_packed(self, rec, stride, per, k, next_obs, est_rec, want_est, advance):
        tt, N = self.tt, self.N
        r, o = self.T(rec, tt.uint8), self.T(next_obs, self.fdt)
        er = None if est_rec is None else self.T(est_rec, tt.uint8)
        mask = _guarded(self.E, (), tt.uint8)
        est = _guarded(self.E, (), tt.float32) if want_est else None
        N.check(self.lib.srlx_store_commit_step_packed(self.h, N.tptr(r), stride, per, k, N.tptr(o), N.tptr(mask), N.tptr(er), N.tptr(est), int(advance), None))
        self.sync()
        return _take("item_mask", mask, self.E), (None if est is None else _take("est", est, self.E))

    def gather_nstep(self, idx):
        tt, N, B, n = self.tt, self.N, len(idx), self.n
        i = self.T(idx, tt.int64)
        obs, act = _guarded(B, (n + 1, self.W, self.F), tt.float32), _guarded(B, (n,), tt.int32)
        rew, ter = _guarded(B, (n,), tt.float32), _guarded(B, (n,), tt.float32)
        N.check(self.lib.srlx_store_gather_nstep(self.h, B, N.tptr(i), N.tptr(obs), N.tptr(act), N.tptr(rew), N.tptr(ter), None))
        self.sync()
        return _take("obs", obs, B), _take("actions", act, B), _take("rewards", rew, B), _take("terminated", ter, B)

    def locate(self, idx, with_prev):
        tt, N, B = self.tt, self.N, len(idx)
        i = self.T(idx, tt.int64)
        env, slot = _guarded(B, (), tt.int64), _guarded(B, (), tt.int64)
        prev = _guarded(B, (), tt.int64) if with_prev else None
        N.check(self.lib.srlx_store_locate(self.h, B, N.tptr(i), N.tptr(env), N.tptr(slot), N.tptr(prev), None))
        self.sync()
        return _take("env", env, B), _take("slot", slot, B), (None if prev is None else _take("prev_slot", prev, B))

    def gather_items(self, idx, kb, kc):
        tt, N, B, n = self.tt, self.N, len(idx), self.n
        i = self.T(idx, tt.int64)
        off, act = _guarded(B, (kc, self.W), tt.int64), _guarded(B, (n,), tt.int32)
        rew, ter = _guarded(B, (n,), tt.float32), _guarded(B, (n,), tt.float32)
        N.check(self.lib.srlx_store_gather_items(self.h, B, N.tptr(i), kb, kc, N.tptr(off), N.tptr(act), N.tptr(rew), N.tptr(ter), None))
        self.sync()
        return _take("frame_off", off, B), _take("actions", act, B), _take("rewards", rew, B), _take("terminated", ter, B)

    def gather_obs(self, B, kb, kc):
        out = _guarded(B, (kc, self.W, self.F), self.tt.float32)
        self.N.check(self.lib.srlx_store_gather_obs(self.h, B, kb, kc, self.N.tptr(out), None))
        self.sync()
        return _take("gather_obs", out, B)

    def gather_train(self, idx, with_next):
        tt, N, B, n = self.tt, self.N, len(idx), self.n
        i = self.T(idx, tt.int64)
        off_all, act = _guarded(B, (n + 1, self.W), tt.int64), _guarded(B, (n,), tt.int32)
        off_next = _guarded(B, (n, self.W), tt.int64) if with_next else None
        rew, ter = _guarded(B, (n,), tt.float32), _guarded(B, (n,), tt.float32)
        N.check(self.lib.srlx_store_gather_train(self.h, B, N.tptr(i), N.tptr(off_all), N.tptr(off_next), N.tptr(act), N.tptr(rew), N.tptr(ter), None))
        self.sync()
        return (_take("off_all", off_all, B), None if off_next is None else _take("off_next", off_next, B), _take("actions", act, B), _take("rewards", rew, B),
                _take("terminated", ter, B))

    def synth(self, episode_len, position=None):
        tt, N, E = self.tt, self.N, self.E
        o = _guarded(E, (self.F,), self.fdt)
        r, t_, d = _guarded(E, (), tt.float32), _guarded(E, (), tt.uint8), _guarded(E, (), tt.uint8)
        if position is None:
            N.check(self.lib.srlx_synth_env_step(self.h, episode_len, N.tptr(o), N.tptr(r), N.tptr(t_), N.tptr(d), None))
        else:
            N.check(self.lib.srlx_synth_env_step_at(self.h, int(position), episode_len, N.tptr(o), N.tptr(r), N.tptr(t_), N.tptr(d), None))
        self.sync()
        return _take("next_obs", o, E), _take("rewards", r, E), _take("terminated", t_, E), _take("done", d, E)


def _eq(name, got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (where, name, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":  # bit-equal
        got, want = got.view(np.uint32 if got.dtype == np.float32 else np.uint64), want.view(np.uint32 if want.dtype == np.float32 else np.uint64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s %s: %d of %d entries differ, first at %s: got %r, want %r" % (where, name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                                           want[tuple(bad[0])]))


def _ranges(n):
    return sorted({(0, 1), (1, n), (0, n + 1), (n, 1)})


def _compare_gather(m, d, where, planted=None):
    """Every tree index of the store plus the clamps, through every gathering entry point.  `planted`: compare only items whose first transition lies at or
    after that position.  Float frames are compared where the ring slot has been written (the ring's frame memory is not cleared at create)."""
    idx = R.all_indices(m)
    want = m.gather_all(idx)
    keep = np.ones(len(idx), bool) if planted is None else np.array([q >= planted for q in want["q"]])
    if not keep.any():
        keep = None
    n = m.n
    full = m.frame_tables(idx, 0, n + 1)
    ok = m.frames_written(full)
    sel = (lambda a: a) if keep is None or keep.all() else (lambda a: a[keep])

    def scalars(got, tag):
        if keep is None:
            return
        for name, g in zip(("actions", "rewards", "terminated"), got):
            _eq(name, sel(g), sel(want[name]), where + " " + tag)

    def frames(got, kb, kc, tag):
        if keep is None:
            return
        mk = ok[:, kb:kb + kc] & keep[:, None, None]
        _eq("obs", got[mk], want["obs"][:, kb:kb + kc][mk], where + " " + tag)

    obs, *sc = d.gather_nstep(idx)
    scalars(sc, "gather_nstep")
    frames(obs, 0, n + 1, "gather_nstep")
    env, slot, prev = m.locate_slots(idx)
    g_env, g_slot, g_prev = d.locate(idx, True)
    g_env2, g_slot2, _ = d.locate(idx, False)
    if keep is not None:
        for name, g, w in (("env", g_env, env), ("slot", g_slot, slot), ("prev_slot", g_prev, prev), ("env (prev NULL)", g_env2, env), ("slot (prev NULL)", g_slot2, slot)):
            _eq(name, sel(g), sel(w), where + " locate")
    if not (m.u8 or m.W == 1):
        return
    for kb, kc in _ranges(n):
        tag = "gather_items(%d,%d)" % (kb, kc)
        off, *sc = d.gather_items(idx, kb, kc)
        scalars(sc, tag)
        if keep is not None:
            _eq("frame_off", sel(off), sel(full[:, kb:kb + kc]), where + " " + tag)
        if m.u8 and m.F % 16 == 0:
            frames(d.gather_obs(len(idx), kb, kc), kb, kc, "gather_obs(%d,%d)" % (kb, kc))
    for with_next in (True, False):
        tag = "gather_train(next=%d)" % with_next
        off_all, off_next, *sc = d.gather_train(idx, with_next)
        scalars(sc, tag)
        if keep is not None:
            _eq("off_all", sel(off_all), sel(full), where + " " + tag)
            if with_next:
                _eq("off_next", sel(off_next), sel(full[:, 1:]), where + " " + tag)
    if m.u8 and m.F % 16 == 0:  # gather_train's metadata serves a following gather_obs
        frames(d.gather_obs(len(idx), 0, n + 1), 0, n + 1, "gather_obs after gather_train")


def _roll(g, planted=None, episode_len=3):
    m = R.make_model(g)
    d = Dev(m)
    tables = m.u8 or m.W == 1
    assert d.lib.srlx_store_item_len(d.h) == m.item_len and d.lib.srlx_store_per_capacity(d.h) == m.per_capacity()
    n_ahead = 0
    next_tables, step = {}, 0  # position -> the table a commit announced for it
    for ev in R.events(g, planted):
        where = "%s step %d pos %d" % (g.name, step, m.pos)
        if ev[0] == "reset":
            R.apply_to_model(m, ev)
            d.reset_all(ev[1])
            assert d.position() == 0
            next_tables = {}
        elif ev[0] == "plant":
            R.apply_to_model(m, ev)
            d.plant(ev[1])
        elif ev[0] == "advance":
            R.apply_to_model(m, ev)
            d.advance()
            assert d.position() == m.pos
        elif ev[0] == "policy":
            _eq("stack_current", d.stack_current(), m.stack_current(), where)
            if tables:
                cur = d.frame_table_current()
                _eq("frame_table_current", cur, m.frame_table_current(), where)
                if m.pos in next_tables:
                    _eq("next_table vs the later frame_table_current", next_tables.pop(m.pos), cur, where)
            for name, got, want in zip(("next_obs", "rewards", "terminated", "done"), d.synth(episode_len), H.synth_env_step(m, episode_len)):
                _eq(name, got, want, where + " synth_env_step")
        elif ev[0] == "commit":
            kind = ev[1]
            before = m.pos
            host = before + (ev[3] if kind == "at" else 0)  # lagged mode: the host's position runs one ahead of the store's from the second commit on
            want_mask, want_table = R.apply_to_model(m, ev)
            mask, table = d.commit(kind, ev[2], tables, position=host)
            _eq("item_mask", mask, want_mask, where + " commit " + kind)
            if want_table is not None:
                _eq("next_table", table, want_table, where + " commit " + kind)
                next_tables[host + 1] = table
            assert d.position() == m.pos == before + (kind in ("plain", "ex1")), (where, kind)  # commit_step_ex(advance = 0) and commit_step_at leave it alone
            if kind == "at":
                n_ahead += ev[3]
            step += 1
        elif ev[0] == "gather":
            _compare_gather(m, d, where, planted)
    if g.mode == "at":
        assert n_ahead >= 2 * m.L  # all but the first commit after each reset_all landed one ahead of the store's position
    return m, d


@pytest.mark.parametrize("g", R.GEOMS, ids=R.GEOM_IDS)
def test_rollout_every_item_every_entry_point(g):
    """2 L + 3 scripted lock-steps with a reset_all mid-run: stack_current, frame_table_current, the synthetic environment, the commit variant of the case
    (commit_step / commit_step_ex with advance 1 and 0 + srlx_store_advance, next_table, bump / commit_step_at in the lagged arrangement, the host's position
    one ahead of the store's), set_item_slack, and
    after every commit all N = E item_len tree indices plus the clamps through gather_nstep, locate, gather_items, gather_obs and gather_train."""
    _roll(g)


LARGE = R.LARGE


@pytest.mark.parametrize("bits", [31, 32])
@pytest.mark.parametrize("g", LARGE, ids=[g.name for g in LARGE])
def test_positions_across_2_31_and_2_32(g, bits):
    """The ring position planted at the largest multiple of L below 2^bits - L: the 2 L + 3 lock-steps cross the boundary.  Gathers, tables, locate, the padding
    action and the synthetic environment key on the position; only items whose first transition lies at or after the planted position are compared."""
    L = R.ring_len(g)
    planted = R.planted_position(L, bits)
    assert planted % L == 0 and planted < 2 ** bits - L <= planted + L
    m, d = _roll(g, planted=planted)
    assert m.pos == planted + 2 * L + 3 and m.pos > 2 ** bits and d.position() == m.pos


def test_commit_without_advance_past_its_2048_workgroup_cap():
    """E (frame_bytes / 16 + 1) = 1021 x 514 = 524 794 > 2048 x 256: the advance = 0 commit loops its grid.  Two lock-steps, W = n = 1."""
    g = R.CAP_NO_ADVANCE
    m = R.make_model(g)
    d = Dev(m)
    rng = np.random.default_rng(0)
    frame = lambda: rng.integers(0, 256, (g.E, g.F), dtype=np.uint8)  # noqa: E731
    f0 = frame()
    m.reset_all(f0)
    d.reset_all(f0)
    term, done, _ = R.schedule(g.E, m.L, g.n, g.W)
    for t in range(2):
        s = (rng.integers(0, 5, g.E).astype(np.int32), rng.standard_normal(g.E).astype(np.float32), term[t], done[t], frame())
        want_mask, want_table = m.commit_step(*s, advance=False, next_table=True)
        mask, table = d.commit("ex0", s, True)
        _eq("item_mask", mask, want_mask, "step %d" % t)
        _eq("next_table", table, want_table, "step %d" % t)
        assert d.position() == m.pos
        m.advance()
        d.advance()
        _eq("stack_current", d.stack_current(), m.stack_current(), "step %d" % t)
    idx = R.all_indices(m)[::16]
    want = m.gather_all(idx)
    obs, act, rew, ter = d.gather_nstep(idx)
    ok = m.frames_written(m.frame_tables(idx, 0, 2))
    _eq("obs", obs[ok], want["obs"][ok], "gather")
    for name, got in (("actions", act), ("rewards", rew), ("terminated", ter)):
        _eq(name, got, want[name], "gather")


def test_float32_movers_past_their_grid_cap():
    """The smallest E W F / 4 above 256 x 32 x 256 = 2 097 152 float4 units is 2 097 153 = 129 x 3 x 5419: k_stack_current<true> loops past its cap, and a gather
    of 65 items (65 x 2 x 3 x 5419 units) takes k_gather_obs<true> past the same cap.  W + 2 lock-steps only."""
    g = R.CAP_F32
    assert g.E * g.W * g.F // 4 == 256 * 32 * 256 + 1
    m = R.make_model(g)
    d = Dev(m)
    rng = np.random.default_rng(1)
    frame = lambda: rng.standard_normal((g.E, g.F), dtype=np.float32)  # noqa: E731
    f0 = frame()
    m.reset_all(f0)
    d.reset_all(f0)
    term, done, _ = R.schedule(g.E, m.L, g.n, g.W)
    for t in range(g.W + 2):
        _eq("stack_current", d.stack_current(), m.stack_current(), "step %d" % t)
        s = (rng.integers(0, 5, g.E).astype(np.int32), rng.standard_normal(g.E).astype(np.float32), term[t], done[t], frame())
        _eq("item_mask", d.commit("plain", s, False)[0], m.commit_step(*s), "step %d" % t)
    idx = R.all_indices(m)[:65]
    assert len(idx) * 2 * g.W * (g.F // 4) > 256 * 32 * 256
    want = m.gather_all(idx)
    obs, act, rew, ter = d.gather_nstep(idx)
    ok = m.frames_written(m.frame_tables(idx, 0, 2))
    _eq("obs", obs[ok], want["obs"][ok], "gather")
    for name, got in (("actions", act), ("rewards", rew), ("terminated", ter)):
        _eq(name, got, want[name], "gather")


@pytest.mark.parametrize("per,k,pad,est,advance", [(4, 0, 0, None, 1), (4, 1, 8, "records", 0), (8, 3, 0, "records", 1), (8, 1, 36, "out", 0), (4, 3, 12, "out", 1)])
def test_packed_commit(per, k, pad, est, advance):
    """est: None = no estimate output; "out" = the output without an estimate buffer (-1 where an item completed); "records" = estimates from another packed
    buffer's first extra field.  The ring that results equals the model's, whose state the separate-array commit defines."""
    g = R.PACKED_GEOM
    firsts, steps, _ = R.inputs(g)
    m = R.make_model(g)
    d = Dev(m)
    m.reset_all(firsts[0])
    d.reset_all(firsts[0])
    rng = np.random.default_rng(per + k)
    stride = (10 + 4 * k) * per + pad
    for t, (a, r, term, done, nxt) in enumerate(steps[:2 * m.L + 3]):
        x = rng.standard_normal((g.E, k)).astype(np.float32)
        rec = m.pack_records(a, r, term, done, x, per, stride)
        rec[:, (10 + 4 * k) * per:] = 0xEE  # the padding between records is not read
        erec = m.pack_records(a[::-1], r, done, term, rng.standard_normal((g.E, k)).astype(np.float32), per, stride) if est == "records" else None
        want_mask, want_est = m.commit_step_packed(rec, per, k, nxt, est_records=erec, advance=bool(advance))
        mask, got_est = d.commit_packed(rec, stride, per, k, nxt, erec, est is not None, advance)
        _eq("item_mask", mask, want_mask, "step %d" % t)
        if est is not None:
            _eq("est", got_est, want_est, "step %d" % t)
        if not advance:
            m.advance()
            d.advance()
        assert d.position() == m.pos
        _compare_gather(m, d, "packed step %d" % t)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_gather_train_workgroup_edges(B):
    """64 items per workgroup: B on either side of it, off_next given and NULL, and the metadata it leaves serves a following gather_obs."""
    g = R.GEOMS[0]
    m, d = _case_after_rollout()
    rng = np.random.default_rng(B)
    pool = R.all_indices(m)
    idx = [pool[i] for i in rng.integers(0, len(pool), B)]
    want = m.gather_all(idx)
    full = m.frame_tables(idx, 0, g.n + 1)
    for with_next in (True, False):
        off_all, off_next, act, rew, ter = d.gather_train(idx, with_next)
        _eq("off_all", off_all, full, "B=%d" % B)
        if with_next:
            _eq("off_next", off_next, full[:, 1:], "B=%d" % B)
        for name, got in (("actions", act), ("rewards", rew), ("terminated", ter)):
            _eq(name, got, want[name], "B=%d" % B)
        _eq("gather_obs", d.gather_obs(B, 0, g.n + 1), want["obs"], "B=%d" % B)
        _eq("frames through the table", m.frames_from_table(off_all), want["obs"], "B=%d" % B)


_AFTER = {}


def _case_after_rollout():
    """The model and the device store of GEOMS[0] after the first phase of its schedule (ring written all the way round), built once and left unchanged."""
    if "md" not in _AFTER:
        g = R.GEOMS[0]
        m = R.make_model(g)
        d = Dev(m)
        firsts, steps, t_reset = R.inputs(g)
        m.reset_all(firsts[0])
        d.reset_all(firsts[0])
        for s in steps[:t_reset]:
            _eq("item_mask", d.commit("plain", s, True)[0], m.commit_step(*s), "prepare")
        assert m.written.all()
        _AFTER["md"] = (m, d)
    return _AFTER["md"]


@pytest.mark.parametrize("rows,fb", [(1, 16), (1, 8208), (5, 16), (5, 8208)])
def test_pack_frames(rows, fb):
    N, lib, torch, dev = _env()
    rng = np.random.default_rng(rows + fb)
    base = rng.integers(0, 256, 8 * fb, dtype=np.uint8)
    off = (rng.permutation(8)[:rows] * fb).astype(np.int64)
    if rows > 1:
        off[1] = off[rows - 1] = -1  # rows with offset -1 leave their output bytes untouched
    out, rel = _guarded(rows, (fb,), torch.uint8), _guarded(rows, (), torch.int64)
    tb, to = torch.as_tensor(base).to(dev), torch.as_tensor(off).to(dev)
    N.check(lib.srlx_pack_frames(N.tptr(tb), N.tptr(to), rows, fb, N.tptr(out), N.tptr(rel), None))
    torch.cuda.synchronize()
    want = np.full((rows, fb), SENT["uint8"], np.uint8)
    for r in range(rows):
        if off[r] >= 0:
            want[r] = base[off[r]:off[r] + fb]
    _eq("packed", _take("packed", out, rows), want, "pack_frames")
    _eq("rel", _take("rel", rel, rows), np.where(off < 0, -1, np.arange(rows) * fb).astype(np.int64), "pack_frames")


@pytest.mark.parametrize("n", [8192, 8193])
def test_rng_uniform_on_either_side_of_the_kernel_switch(n):
    N, lib, torch, dev = _env()
    counter = _guarded(1, (), torch.int64)
    counter[0] = 2 ** 33 + 5
    out = _guarded(n, (), torch.float64)
    N.check(lib.srlx_rng_uniform(99, N.tptr(counter), n, N.tptr(out), None))
    torch.cuda.synchronize()
    _eq("uniforms", _take("uniforms", out, n), H.rng_uniform(99, 2 ** 33 + 5, n), "n=%d" % n)
    assert _take("counter", counter, 1)[0] == 2 ** 33 + 6


def test_epsilon_greedy_edges():
    N, lib, torch, dev = _env()
    top = 1.0 - 2.0 ** -53
    rng = np.random.default_rng(4)
    for A in (1, 6):
        E = 40
        q = rng.standard_normal((E, A)).astype(np.float32)
        eps = (np.arange(E) % 2).astype(np.float32)  # eps = 0 and eps = 1
        u = rng.random((E, 2))
        u[:8] = top  # u = 1 - 2^-53 in both columns: the last valid action at eps = 1, the greedy one at eps = 0
        u[8:12, 0], u[12:16, 1] = top, top
        invalid = np.zeros((E, A), bool)
        if A > 1:
            invalid[: E // 2] = True  # rows with a single valid action
            invalid[np.arange(E // 2), np.arange(E // 2) % A] = False
            invalid[E // 2:] = rng.random((E - E // 2, A)) < 0.3
            invalid[E // 2:, 3] = False
        for inv in (None, invalid):
            out = _guarded(E, (), torch.int32)
            tq, te, tu = torch.as_tensor(q).to(dev), torch.as_tensor(eps).to(dev), torch.as_tensor(u).to(dev)
            ti = None if inv is None else torch.as_tensor(inv.astype(np.uint8)).to(dev)
            N.check(lib.srlx_policy_epsilon_greedy(E, A, N.tptr(tq), N.tptr(te), N.tptr(tu), N.tptr(ti), N.tptr(out), None))
            torch.cuda.synchronize()
            _eq("actions", _take("actions", out, E), H.epsilon_greedy(q, eps, u, inv), "A=%d" % A)


@pytest.mark.parametrize("u8,F", [(True, 16), (True, 10), (False, 6)], ids=["u8-F16-one-launch", "u8-F10-two-launches", "f32-F6-two-launches"])
def test_synthetic_environment_and_its_positioned_form(u8, F):
    """A lagged store (slack 1): the environments step at the HOST's position with srlx_synth_env_step_at and commit_step_at lands there, one ahead of the
    store's own position from the second lock-step on; srlx_synth_env_step reads the trailing position.  Both against H.synth_env_step on the model.
    tests/test_store_envelope_cpu.py walks the same loop on the model: episodes end, lanes pass through their reset step."""
    g = R.SYNTH_GEOM(u8, F)
    m = R.make_model(g)
    d = Dev(m)
    f0 = np.zeros((g.E, F), np.uint8 if u8 else np.float32)
    m.reset_all(f0)
    d.reset_all(f0)
    names = ("next_obs", "rewards", "terminated", "done")
    for step in range(2 * m.L + 3):
        own = m.pos
        host = own + (1 if step else 0)
        assert d.position() == own
        for name, got, w in zip(names, d.synth(R.SYNTH_EPISODE), H.synth_env_step(m, R.SYNTH_EPISODE)):
            _eq(name, got, w, "synth (trailing position) step %d" % step)
        want = R.synth_at(m, host)
        for name, got, w in zip(names, d.synth(R.SYNTH_EPISODE, position=host), want):
            _eq(name, got, w, "synth_at step %d" % step)
        s = (np.full(g.E, step % 5, np.int32), want[1], want[2], want[3], want[0])
        _eq("item_mask", d.commit("at", s, u8, position=host)[0], m.commit_step(*s, position=host), "step %d" % step)
        assert d.position() == own
        if step:
            m.advance()
            d.advance()
        _compare_gather(m, d, "synth step %d" % step)


@pytest.mark.parametrize("A", R.ACTOR_TD_A)
@pytest.mark.parametrize("n", R.ACTOR_TD_N)
def test_actor_td(n, A):
    """The -2 / -1 codes are exact; the values follow tests/lstm_reference.py::check_tensor against the model in float64, with the model's own float32 evaluation as
    the measure of what float32 costs (from n = 8 up the kernel adds its n terms one after another while the model's float32 sum is numpy's pairwise one).
    tests/test_store_envelope_cpu.py asserts what the cases hold: both codes, masked lanes, greedy and non-greedy rows."""
    import lstm_reference as LR
    N, lib, torch, dev = _env()
    m = R.actor_td_model(n, A)
    d = Dev(m)
    E = m.E
    evaluated = 0
    for t, (s, ev) in enumerate(R.actor_td_case(n, A)):
        if ev is None and t == 0:
            m.reset_all(s)
            d.reset_all(s)
            continue
        want_mask = m.commit_step(*s)
        mask, _ = d.commit("plain", s, True)
        _eq("item_mask", mask, want_mask, "n=%d step %d" % (n, t - 1))
        if ev is None:
            continue
        ev = R.actor_td_finish(m, ev)
        mask = mask.copy()
        mask[ev["mask_zero"]] = 0
        qh, base, first_slot = ev["q_hist"], ev["base_slot"], ev["first_slot"]
        tq, tm = torch.as_tensor(qh).to(dev), torch.as_tensor(mask).to(dev)
        for rescale in (0, 1):
            for h in (0.0, 1.0):
                where = "actor_td n=%d A=%d rescale=%d h=%g" % (n, A, rescale, h)
                est = _guarded(E, (), torch.float32)
                N.check(lib.srlx_store_actor_td(d.h, first_slot, m.per_capacity(), N.tptr(tq), base, N.tptr(tm), 0.99, h, 1, rescale, N.tptr(est), None))
                torch.cuda.synchronize()
                got = _take("est", est, E)
                w64 = m.actor_td(qh, base, first_slot, mask, 0.99, h, bool(rescale), np.float64)
                w32 = m.actor_td(qh, base, first_slot, mask, 0.99, h, bool(rescale), np.float32)
                code = w64 < 0
                _eq("codes", got[code], w64[code].astype(np.float32), where)
                assert (~code).any() and (got[~code] >= 0).all(), where
                LR.check_tensor("est", torch.as_tensor(got[~code]), torch.as_tensor(w64[~code]), torch.as_tensor(w32[~code]), where)
                evaluated += 1
    assert evaluated == 8


@pytest.mark.parametrize("n", [1, 2, 5, 16, 17, 1000, 65537, 256 * 16 * 256 + 1])
def test_rng_permutation_vs_model(n):
    """The keyed Feistel permutation: values and the counter's advance (+1, and +count for the batched form, whose y-th permutation is the one the counter + y
    gives).  n on either side of a power of four (the cycle walk), n = 1, and one past the grid cap of 256 x 16 workgroups."""
    N, lib, torch, dev = _env()
    c0 = 2 ** 32 + 9
    counter = _guarded(1, (), torch.int64)
    counter[0] = c0
    out = _guarded(n, (), torch.int64)
    N.check(lib.srlx_rng_permutation(4242, N.tptr(counter), n, N.tptr(out), None))
    torch.cuda.synchronize()
    _eq("permutation", _take("permutation", out, n), R.rng_permutation(4242, c0, n), "n=%d" % n)
    assert _take("counter", counter, 1)[0] == c0 + 1
    if n <= 65537:
        for count in (1, 3):
            counter[0] = c0
            outs = _guarded(count, (n,), torch.int64)
            N.check(lib.srlx_rng_permutations(4242, N.tptr(counter), n, count, N.tptr(outs), None))
            torch.cuda.synchronize()
            _eq("permutations", _take("permutations", outs, count), R.rng_permutations(4242, c0, n, count), "n=%d count=%d" % (n, count))
            assert _take("counter", counter, 1)[0] == c0 + count


def test_refusals():
    """Each returns an error status; where the call has an output, the output stays untouched (nothing was launched)."""
    N, lib, torch, dev = _env()
    h = N.c_p()
    assert lib.srlx_store_create(ctypes.byref(h), 2, 3 + 2, 16, N.OBS_U8, 2, 3, 4, 1, 0, 0) != N.OK  # ring_len == n_step + window
    assert not h.value
    m = R.StoreModel(8, 3 + 2 + 2, 16, 2, 3, 4, True, 1, True)
    d = Dev(m)
    assert lib.srlx_store_set_item_slack(d.h, 2) != N.OK and lib.srlx_store_item_len(d.h) == 2  # a slack that leaves no item
    assert lib.srlx_store_set_item_slack(d.h, -1) != N.OK
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    o_obs = _guarded(4, (1, 2, 16), torch.float32)
    assert lib.srlx_store_gather_obs(d.h, 4, 0, 1, N.tptr(o_obs), None) != N.OK  # before any gather
    _untouched("gather_obs", o_obs)
    off, act, rew, ter = _guarded(4, (5, 2), torch.int64), _guarded(4, (3,), torch.int32), _guarded(4, (3,), torch.float32), _guarded(4, (3,), torch.float32)
    assert lib.srlx_store_gather_items(d.h, 4, N.tptr(idx), 1, 4, N.tptr(off), N.tptr(act), N.tptr(rew), N.tptr(ter), None) != N.OK  # k_begin + k_count > n + 1
    for name, t in (("off", off), ("act", act), ("rew", rew), ("ter", ter)):
        _untouched(name, t)
    # a packed commit with envs_per_record no multiple of 4, or one that does not divide E
    rec, nxt, mask = torch.zeros(8 * 64, dtype=torch.uint8, device=dev), torch.zeros((8, 16), dtype=torch.uint8, device=dev), _guarded(8, (), torch.uint8)
    for per in (2, 6, 12, 16):
        assert lib.srlx_store_commit_step_packed(d.h, N.tptr(rec), 16 * per, per, 0, N.tptr(nxt), N.tptr(mask), None, None, 1, None) != N.OK, per
    torch.cuda.synchronize()
    _untouched("item_mask", mask)
    assert d.position() == 0
    # float32 store with W > 1: no frame tables, gather_items or gather_train; gather_obs wants 16-byte uint8 frames
    mf = R.StoreModel(4, 3 + 2 + 2, 8, 2, 3, 4, True, 1, False)
    df = Dev(mf)
    tab = _guarded(4, (2,), torch.int64)
    assert lib.srlx_store_frame_table_current(df.h, N.tptr(tab), None) != N.OK
    a, r, t_, dn = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, device=dev), torch.zeros(4, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.uint8, device=dev)
    nf, mk = torch.zeros((4, 8), device=dev), _guarded(4, (), torch.uint8)
    assert lib.srlx_store_commit_step_ex(df.h, N.tptr(a), N.tptr(r), N.tptr(t_), N.tptr(dn), N.tptr(nf), N.tptr(mk), N.tptr(tab), 1, None, None) != N.OK
    assert lib.srlx_store_commit_step_at(df.h, 0, N.tptr(a), N.tptr(r), N.tptr(t_), N.tptr(dn), N.tptr(nf), N.tptr(mk), N.tptr(tab), None, None) != N.OK
    off4 = _guarded(4, (4, 2), torch.int64)
    assert lib.srlx_store_gather_items(df.h, 4, N.tptr(idx), 0, 4, N.tptr(off4), N.tptr(act), N.tptr(rew), N.tptr(ter), None) != N.OK
    assert lib.srlx_store_gather_train(df.h, 4, N.tptr(idx), N.tptr(off4), None, N.tptr(act), N.tptr(rew), N.tptr(ter), None) != N.OK
    obs4 = _guarded(4, (4, 2, 8), torch.float32)
    N.check(lib.srlx_store_gather_nstep(df.h, 4, N.tptr(idx), N.tptr(obs4), N.tptr(_guarded(4, (3,), torch.int32)), N.tptr(_guarded(4, (3,), torch.float32)),
                                        N.tptr(_guarded(4, (3,), torch.float32)), None))  # (a gather has now preceded: the refusal below is the frame size's)
    assert lib.srlx_store_gather_obs(df.h, 4, 0, 1, N.tptr(o_obs), None) != N.OK  # a float32 store
    m12 = R.StoreModel(4, 3 + 2 + 2, 12, 2, 3, 4, True, 1, True)
    d12 = Dev(m12)
    off12 = _guarded(4, (1, 2), torch.int64)
    N.check(lib.srlx_store_gather_items(d12.h, 4, N.tptr(idx), 0, 1, N.tptr(off12), N.tptr(act), N.tptr(rew), N.tptr(ter), None))
    torch.cuda.synchronize()
    act.fill_(SENT["int32"]), rew.fill_(SENT["float32"]), ter.fill_(SENT["float32"])
    o12 = _guarded(4, (1, 2, 12), torch.float32)
    assert lib.srlx_store_gather_obs(d12.h, 4, 0, 1, N.tptr(o12), None) != N.OK  # F % 16 != 0
    # actor_td with n = 33
    m33 = R.StoreModel(4, 33 + 1 + 1, 16, 1, 33, 4, True, 1, True)
    d33 = Dev(m33)
    est, qh, mk4 = _guarded(4, (), torch.float32), torch.zeros((34, 4, 4), device=dev), torch.ones(4, dtype=torch.uint8, device=dev)
    assert lib.srlx_store_actor_td(d33.h, 0, 4, N.tptr(qh), 0, N.tptr(mk4), 0.99, 1.0, 1, 0, N.tptr(est), None) != N.OK
    torch.cuda.synchronize()
    for name, t in (("tab", tab), ("mask", mk), ("off4", off4), ("act", act), ("rew", rew), ("ter", ter), ("o_obs", o_obs), ("o12", o12), ("est", est)):
        _untouched(name, t)
