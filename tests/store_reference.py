"""The transition store's model, completed: oracle/hot_path_oracle.StoreOracle (commit_step, stack_at, locate and gather_item are pinned against recordings of the
reference and stay the source of truth) plus everything else the C ABI of csrc/srlx_rollout.hip has -- frame-offset tables, slot location, item slack, the
commit variants (host position, no advance, next frame table), the packed commit and its estimate column, and the actor-side initial priority.  Plain numpy and
Python integers: a ring position is an unbounded int here, nothing is reduced to 32 bits.

Also the case list and the scripted episode schedules that tests/test_store_envelope_cpu.py (conditions on the schedules, model consistency) and
tests/test_store_envelope_gpu.py (every entry point against this model) share."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hot_path_oracle as H  # noqa: E402


class StoreModel(H.StoreOracle):
    def __init__(self, n_envs, ring_len, obs_elems, window, n_step, n_actions, reward_clip, seed, u8=True, slack=0):
        if ring_len <= n_step + window:
            raise ValueError("ring_len must exceed n_step + window")
        super().__init__(n_envs, ring_len, obs_elems, window, n_step, n_actions, reward_clip, seed, u8)
        self.written = np.zeros(ring_len, bool)  # ring slots whose frame has been written (the device does not clear its frame memory at create)
        self.set_item_slack(slack)

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------------------------------------
    @property
    def N(self):
        return self.E * self.item_len

    def set_item_slack(self, s):
        if s < 0 or self.L - (self.n + self.W) - s < 1:
            raise ValueError("a slack that leaves no item")
        self.slack = s
        self.item_len = self.L - (self.n + self.W) - s

    def per_capacity(self):
        return self.E * self.item_len

    def reset_all(self, first_obs, pos=0):
        """`pos`: the position the ring continues from, any non-negative multiple of L, so that the first frame sits in slot 0 (the device's reset writes 0:
        a test plants the other values)."""
        super().reset_all(first_obs)
        self.written[0] = True
        self.set_pos(pos)

    def set_pos(self, pos):
        assert pos >= 0 and pos % self.L == 0, "a planted position is a multiple of the ring length"
        self.pos = int(pos)

    def advance(self):
        self.pos += 1

    # ---- frame offsets -----------------------------------------------------------------------------------------------------------------------------------
    def frame_offset(self, e, x, c):
        back = self.W - 1 - c
        if back > self.step_in_ep[e, x % self.L]:
            return -1
        return (e * self.L + (x - back) % self.L) * self.F

    def frame_table_current(self):
        return self._table_at(self.pos)

    def _table_at(self, x):
        return np.array([[self.frame_offset(e, x, c) for c in range(self.W)] for e in range(self.E)], np.int64).reshape(self.E, self.W)

    def item_jd(self, e, q):
        for k in range(self.n):
            if self.flags[e, (q + k) % self.L] & self.DONE:
                return k
        return self.n

    def frame_tables(self, idx, k_begin, k_count):
        """int64 [B][k_count][W]: states after the terminal one repeat it, min(k, jd + 1) (rainbow.py:358)."""
        out = np.zeros((len(idx), k_count, self.W), np.int64)
        for b, ti in enumerate(idx):
            e, q = self.locate(ti)
            jd = self.item_jd(e, q)
            for i in range(k_count):
                kk = min(k_begin + i, jd + 1)
                for c in range(self.W):
                    out[b, i, c] = self.frame_offset(e, q + kk, c)
        return out

    def frames_written(self, table):
        """bool like `table`: True where the entry is -1 (the kernels write zeros there) or points at a ring slot that has been written."""
        t = np.asarray(table)
        slot = (np.maximum(t, 0) // self.F) % self.L
        return (t < 0) | self.written[slot]

    def frames_from_table(self, table):
        """float32 [..., F]: the frames a table points at, read from the ring and normalised; zeros at -1."""
        t = np.asarray(table)
        out = np.zeros(t.shape + (self.F,), np.float32)
        flat = self.obs.reshape(self.E * self.L, self.F)
        for i in np.ndindex(t.shape):
            if t[i] >= 0:
                assert t[i] % self.F == 0
                out[i] = self._norm(flat[t[i] // self.F])
        return out

    # ---- location ----------------------------------------------------------------------------------------------------------------------------------------
    def locate_slots(self, idx):
        env, slot, prev = (np.zeros(len(idx), np.int64) for _ in range(3))
        for b, ti in enumerate(idx):
            e, q = self.locate(ti)
            env[b], slot[b] = e, q % self.L
            prev[b] = -1 if self.step_in_ep[e, q % self.L] == 0 else (q - 1) % self.L
        return env, slot, prev

    def gather_all(self, idx):
        """gather_item of every index (clamped ones included): obs [B][n+1][W][F], actions, rewards, terminated [B][n], jd [B], q (Python ints)."""
        memo = {}
        rows = []
        for ti in idx:
            key = self.locate(ti)
            if key not in memo:
                memo[key] = self.gather_item(*key)
            rows.append(memo[key] + (key[1],))
        obs, act, rew, ter = (np.stack([r[i] for r in rows]) for i in range(4))
        return dict(obs=obs, actions=act, rewards=rew, terminated=ter, jd=np.array([r[4] for r in rows]), q=[r[5] for r in rows])

    # ---- commit variants ---------------------------------------------------------------------------------------------------------------------------------
    def commit_step(self, actions, rewards, terminated, done, next_obs, position=None, advance=True, next_table=False):
        """position: a host-given ring position (srlx_store_commit_step_at): the commit lands there and the model's own position is left alone.
        advance=False: the position stays (srlx_store_commit_step_ex(advance=0)).  next_table: also return the frame table of the next policy pass,
        frame_offset(e, p + 1, c)."""
        own = self.pos
        p = own if position is None else int(position)
        self.pos = p
        mask = super().commit_step(actions, rewards, terminated, done, next_obs)
        self.written[(p + 1) % self.L] = True
        self.pos = own + 1 if (advance and position is None) else own
        if next_table:
            return mask, self._table_at(p + 1)
        return mask

    @staticmethod
    def pack_records(actions, rewards, term, done, extras, per, stride):
        """uint8 [E / per][stride]: a record = [action int32 x per | reward float32 x per | terminated u8 x per | done u8 x per | extra float32 x per x k],
        environment e = (record e // per, lane e % per) -- the layout documented above k_commit_step."""
        actions, rewards = np.ascontiguousarray(actions, np.int32), np.ascontiguousarray(rewards, np.float32)
        term, done = np.ascontiguousarray(term, np.uint8), np.ascontiguousarray(done, np.uint8)
        E = len(actions)
        extras = np.zeros((E, 0), np.float32) if extras is None else np.asarray(extras, np.float32).reshape(E, -1)
        k = extras.shape[1]
        assert E % per == 0 and stride >= (10 + 4 * k) * per
        out = np.zeros((E // per, stride), np.uint8)
        for r in range(E // per):
            s = slice(r * per, (r + 1) * per)
            out[r, 0:4 * per] = actions[s].view(np.uint8)
            out[r, 4 * per:8 * per] = rewards[s].view(np.uint8)
            out[r, 8 * per:9 * per] = term[s]
            out[r, 9 * per:10 * per] = done[s]
            out[r, 10 * per:(10 + 4 * k) * per] = np.ascontiguousarray(extras[s]).view(np.uint8).reshape(-1)
        return out

    @staticmethod
    def unpack_records(records, per, k):
        records = np.ascontiguousarray(records)
        f = lambda a, b, dt: np.concatenate([np.ascontiguousarray(r[a:b]).view(dt) for r in records])  # noqa: E731
        extras = np.concatenate([np.ascontiguousarray(r[10 * per:(10 + 4 * k) * per]).view(np.float32).reshape(per, k) for r in records])
        return f(0, 4 * per, np.int32), f(4 * per, 8 * per, np.float32), f(8 * per, 9 * per, np.uint8), f(9 * per, 10 * per, np.uint8), extras

    def commit_step_packed(self, records, per, extra_floats, next_obs, est_records=None, advance=True):
        """Returns (item mask, estimate column): -2 where the commit completed no item, -1 with no estimate buffer, the first extra field of `est_records`
        otherwise."""
        if per <= 0 or per % 4 != 0 or self.E % per != 0:
            raise ValueError("environments do not split into records")
        a, r, t, d, _ = self.unpack_records(records, per, extra_floats)
        mask = self.commit_step(a, r, t != 0, d != 0, next_obs, advance=advance)
        est = np.full(self.E, -1.0, np.float32)
        if est_records is not None:
            est[:] = self.unpack_records(est_records, per, extra_floats)[4][:, 0]
        est[mask == 0] = -2.0
        return mask, est

    # ---- actor-side initial priority (rainbow.py:389-398) ------------------------------------------------------------------------------------------------
    def actor_td(self, q_hist, base_slot, first_slot, mask, discount, retrace_h, rescale, dtype=np.float64):
        """q_hist [n+1][E][A]: row k of lane e is q_hist[(base_slot + k) % (n + 1), e].  -2 where the mask is 0, -1 where the episode ends inside the window
        (or the slot is not the lane's), otherwise |nstep_target(rows 1..n in both roles) - row0[a0]| evaluated in `dtype`."""
        n, cap = self.n, self.per_capacity()
        out = np.zeros(self.E, dtype)
        for e in range(self.E):
            if not mask[e]:
                out[e] = -2
                continue
            le, q = self.locate((first_slot + e) % cap + (cap - 1))
            _, act, rew, ter, jd = self.gather_item(le, q)
            if jd < n or le != e:
                out[e] = -1
                continue
            rows = np.stack([q_hist[(base_slot + k) % (n + 1), e] for k in range(n + 1)]).astype(dtype)
            nxt = rows[None, 1:]
            tgt = H.nstep_target(nxt, nxt, act[None], rew[None], ter[None], None, discount, retrace_h, True, rescale, np_dtype=dtype)
            out[e] = np.abs(tgt[0] - rows[0, act[0]])
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# cases: every geometry runs 2 L + 3 lock-steps of its scripted schedule
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
Geom = namedtuple("Geom", "name u8 F W n extra E slack mode")  # ring_len = n + W + extra; item_len = extra - slack


def ring_len(g):
    return g.n + g.W + g.extra


# mode: which commit entry point the roll-out uses.  "plain" srlx_store_commit_step; "ex" srlx_store_commit_step_ex alternating advance = 1 with advance = 0 +
# srlx_store_advance, with next_table (where the store has frame tables) and bump; "at" the lagged mode (needs slack 1).
GEOMS = [
    Geom("u8-F16", True, 16, 4, 3, 6, 5, 0, "ex"),
    Geom("u8-F48", True, 48, 2, 1, 1, 1, 0, "plain"),
    Geom("u8-F1040", True, 1040, 4, 3, 2, 5, 1, "at"),
    Geom("u8-F8192", True, 8192, 2, 3, 1, 5, 0, "ex"),
    Geom("u8-F8208-E129", True, 8208, 2, 1, 1, 129, 0, "plain"),  # E (F / 16 + 1) = 66 306 > 65 536: the advance commit loops its 256 workgroups twice over
    Geom("u8-F12", True, 12, 4, 8, 6, 5, 0, "ex"),
    Geom("u8-F1-E257", True, 1, 1, 3, 1, 257, 0, "plain"),
    Geom("u8-F17-n32", True, 17, 2, 32, 1, 8, 0, "ex"),
    Geom("u8-F16-E300", True, 16, 1, 1, 1, 300, 0, "ex"),
    Geom("u8-F16-E256", True, 16, 2, 1, 2, 256, 1, "at"),
    Geom("f32-F1-E257", False, 1, 1, 1, 1, 257, 0, "ex"),
    Geom("f32-F3", False, 3, 2, 3, 1, 5, 0, "plain"),
    Geom("f32-F4", False, 4, 1, 3, 2, 5, 1, "at"),
    Geom("f32-F6", False, 6, 4, 8, 6, 5, 0, "ex"),
    Geom("f32-F8-n32", False, 8, 1, 32, 1, 8, 0, "plain"),
    Geom("f32-F260", False, 260, 2, 3, 1, 1, 0, "ex"),
]
GEOM_IDS = [g.name for g in GEOMS]
# runs outside the list: ring positions planted below 2^31 and 2^32, the packed commit, and the sizes past the commit's and the float32 movers' grid caps
LARGE = [Geom("u8-F16-large", True, 16, 4, 3, 6, 5, 0, "ex"), Geom("f32-F6-large", False, 6, 2, 3, 2, 3, 1, "at")]
PACKED_GEOM = Geom("packed", True, 16, 2, 3, 2, 8, 0, "plain")
CAP_NO_ADVANCE = Geom("u8-F8208-E1021", True, 8208, 1, 1, 1, 1021, 0, "ex")  # E (F / 16 + 1) = 524 794 > 2048 x 256
CAP_F32 = Geom("f32-cap", False, 4 * 5419, 3, 1, 1, 129, 0, "plain")  # E W F / 4 = 2 097 153 = 256 x 32 x 256 + 1


def planted_position(L, bits):
    """The largest multiple of L below 2^bits - L."""
    return ((2 ** bits - L - 1) // L) * L
N_ACTIONS = 5
SEED = 77


def schedule(E, L, n, W):
    """Scripted (terminated, done) uint8 [T][E] for T = 2 L + 3 lock-steps and the lock-step before which reset_all runs again.

    Phase 1 is lock-steps 0 .. L + 1 (positions 0 .. L + 1: the ring wraps), then reset_all, then phase 2 with positions 0 .. L.
    Phase 1: lanes 0 and 1 end at position 0 (episodes of length 1, two lanes in one lock-step); lane 0 ends again in the last ring slot (position L - 1) and
    lane 1 in slot 0 (position L), while lane 0 is in its reset step.  Every other lane ends at position 2 + (e mod (L - 1)).
    Phase 2: the item gathered after the commit at position p starts at q = p - (n - 1), so q only reaches 0 .. L + 1 - n, Q = L + 2 - n values; an episode
    end at position d gives jd = d - q.  Lane e ends at d = (Q - 1) + (e mod ceil(n / Q)) Q: between them the lanes meet every jd in 0 .. n - 1.  A single
    lane also ends at position L (slot 0) where that is no reset step.  Where the tiling leaves a lane over, the last lane ends at positions 0 and 2 instead.
    An end is a truncation (done without terminated) where position + lane is odd."""
    T1, T2 = L + 2, L + 1
    done = np.zeros((T1 + T2, E), np.uint8)
    for e in range(E):
        if e < 2:
            done[0, e] = 1
            done[L - 1 + e, e] = 1
        else:
            done[2 + e % (L - 1), e] = 1
    Q = L + 2 - n
    lanes = -(-n // Q)
    for e in range(E):
        if E > lanes and e == E - 1:  # a lane the tiling does not need: two episodes of length 1 (fewer than W frames at W >= 3), gathered from a full ring
            done[T1, e] = done[T1 + 2, e] = 1
            continue
        d = (Q - 1) + (e % lanes) * Q
        if d <= L:
            done[T1 + d, e] = 1
        if E == 1 and d <= L - 2:
            done[T1 + L, e] = 1
    term = done.copy()
    for t in range(T1 + T2):
        p = t if t < T1 else t - T1
        for e in range(E):
            if (p + e) % 2 == 1:
                term[t, e] = 0
    return term, done, T1


def inputs(g, seed=0):
    """Deterministic per-lock-step inputs of a geometry: first frames of both resets, then (actions, rewards, terminated, done, next_obs) per lock-step."""
    L = ring_len(g)
    term, done, t_reset = schedule(g.E, L, g.n, g.W)
    rng = np.random.default_rng(1000 + seed)

    def frame():
        return rng.integers(0, 256, (g.E, g.F), dtype=np.uint8) if g.u8 else rng.standard_normal((g.E, g.F)).astype(np.float32)

    firsts = [frame(), frame()]
    steps = []
    for t in range(len(done)):
        a = rng.integers(0, N_ACTIONS, g.E).astype(np.int32)
        r = (rng.standard_normal(g.E) * 2).astype(np.float32)
        r[rng.random(g.E) < 0.2] = 0.0
        steps.append((a, r, term[t], done[t], frame()))
    return firsts, steps, t_reset


def make_model(g, clip=True):
    return StoreModel(g.E, ring_len(g), g.F, g.W, g.n, N_ACTIONS, clip, SEED, g.u8, g.slack)


def all_indices(m):
    """Every tree index of the store, one below N - 1 and one at or above 2 N - 1 (the clamps)."""
    N = m.N
    return [N - 2] + list(range(N - 1, 2 * N - 1)) + [2 * N - 1, 2 * N + 5]


def events(g, planted=None):
    """The roll-out of a geometry as a list of steps that the CPU suite applies to the model alone and the GPU suite to the model and the device:
    ("reset", first_obs) | ("plant", position) | ("policy",) | ("commit", kind, inputs) | ("advance",) | ("gather",).
    kind: "plain" | "ex1" (commit_step_ex, advance = 1) | "ex0" (advance = 0; a gather at the trailing position and srlx_store_advance follow) |
    "at" (commit_step_at at the host's position, a fourth field giving its lead over the store's own position: DeviceReplay's lagged mode.  The first commit after
    a reset_all is made at lead 0 and no advance follows it, so every later one lands ONE AHEAD of the store's position -- two commit_step_at before the first
    srlx_store_advance --; the gather between a commit and its advance sees the trailing position, and one more advance at the end lets the store catch up).
    `planted`: the ring position written after the first reset_all (the large-position runs; they have no second reset_all, which would rewind it)."""
    firsts, steps, t_reset = inputs(g)
    yield ("reset", firsts[0])
    if planted is not None:
        yield ("plant", planted)
    yield ("gather",)  # before the first commit
    lead = 0
    for t, s in enumerate(steps):
        if t == t_reset and planted is None:
            yield ("reset", firsts[1])
            yield ("gather",)
            lead = 0
        yield ("policy",)
        if g.mode == "plain":
            yield ("commit", "plain", s)
        elif g.mode == "ex" and t % 2 == 0:
            yield ("commit", "ex1", s)
        elif g.mode == "ex":
            yield ("commit", "ex0", s)
            yield ("gather",)
            yield ("advance",)
        else:
            yield ("commit", "at", s, lead)
            yield ("gather",)
            if lead:
                yield ("advance",)
            lead = 1
        yield ("gather",)
    if g.mode == "at":
        yield ("advance",)
        yield ("gather",)


def apply_to_model(m, ev):
    """Applies one step of events() to the model; a commit returns (item mask, next frame table or None)."""
    if ev[0] == "reset":
        m.reset_all(ev[1])
    elif ev[0] == "plant":
        m.set_pos(ev[1])
    elif ev[0] == "advance":
        m.advance()
    elif ev[0] == "commit":
        kind, s = ev[1], ev[2]
        tables = m.u8 or m.W == 1
        if kind == "plain":
            return m.commit_step(*s), None
        kw = dict(position=m.pos + ev[3]) if kind == "at" else dict(advance=(kind == "ex1"))
        if tables:
            return m.commit_step(*s, next_table=True, **kw)
        return m.commit_step(*s, **kw), None
    return None


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# srlx_store_actor_td: a roll-out of n + 3 lock-steps on a small uint8 store; the last two are evaluated
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
ACTOR_TD_N = [1, 3, 7, 8, 32]
ACTOR_TD_A = [2, 6]
ACTOR_TD_E = 24


def actor_td_model(n, A):
    return StoreModel(ACTOR_TD_E, n + 1 + 3, 16, 1, n, A, False, 11, True)


def actor_td_case(n, A):
    """Yields (first_obs, None) once, then per lock-step (commit inputs, evaluation or None).  An evaluation is made on the state AFTER the commit and holds
    mask_zero (lanes to clear in the item mask), q_hist [n+1][E][A], base_slot and first_slot.  Lanes 3 mod 4 end their episode in the lock-step before the
    last: their windows hold an episode end (and at n = 1 the lane is in its reset step in the last one, so the commit's own mask is 0 there).  Even lanes take
    the greedy action at every step of the window, so retrace keeps all their terms; odd lanes act as drawn.  The model passed in is read, not changed."""
    E = ACTOR_TD_E
    rng = np.random.default_rng(100 * n + A)
    yield rng.integers(0, 256, (E, 16), dtype=np.uint8), None
    T = n + 3
    for t in range(T):
        done = np.zeros(E, np.uint8)
        if t == T - 2:
            done[3::4] = 1
        s = (rng.integers(0, A, E).astype(np.int32), (rng.standard_normal(E) * 2).astype(np.float32), done, done, rng.integers(0, 256, (E, 16), dtype=np.uint8))
        if t < T - 2:
            yield s, None
            continue
        qh = (rng.standard_normal((n + 1, E, A)) * 2).astype(np.float32)
        yield s, dict(mask_zero=slice(1, None, 6), q_hist=qh, base_slot=(t + 1) % (n + 1), t=t)


def actor_td_finish(m, ev):
    """Completes an evaluation once the model holds the commit: first_slot, and the greedy rows of the even lanes (which need the item's stored actions)."""
    n, qh, base = m.n, ev["q_hist"], ev["base_slot"]
    ev["first_slot"] = (ev["t"] * m.E) % m.per_capacity()  # ((commits - 1) E) mod capacity, as the engine passes it
    for e in range(0, m.E, 2):
        act = m.gather_item(e, max(m.pos - n, 0))[1]
        for k in range(1, n):  # td_rows compares a_k with the greedy action of row k + 1
            qh[(base + k + 1) % (n + 1), e, act[k]] += 10.0
    return ev


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# srlx_rng_permutation / srlx_rng_permutations: a keyed permutation of 0..n-1 -- a four-round Feistel network over the smallest even number of bits that
# holds n - 1, walked until it lands below n.  Key = (seed, counter); the y-th permutation of a batched call uses counter + y.
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def rng_permutation(seed, counter, n):
    bits = 2
    while (1 << bits) < n:
        bits += 2
    half = bits // 2
    mask = np.uint64((1 << half) - 1)
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    while todo.any():
        v = x[todo]
        left, right = v >> np.uint64(half), v & mask
        for rnd in range(4):
            key = (int(seed) + 0x9E3779B97F4A7C15 * (rnd + 1)) & 0xFFFFFFFFFFFFFFFF
            f = H.rng_u64(key, np.uint64(counter), right) & mask
            left, right = right, left ^ f
        x[todo] = (left << np.uint64(half)) | right
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def rng_permutations(seed, counter, n, count):
    return np.stack([rng_permutation(seed, counter + y, n) for y in range(count)])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the synthetic environment on a lagged store
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
SYNTH_EPISODE = 4
SYNTH_SHAPES = [(True, 16), (True, 10), (False, 6)]


def SYNTH_GEOM(u8, F):
    return Geom("synth", u8, F, 2, 3, 2, 7, 1, "at")


def synth_at(m, position):
    """H.synth_env_step as the environments of a lagged store see it: at the host's position."""
    own, m.pos = m.pos, position
    try:
        return H.synth_env_step(m, SYNTH_EPISODE)
    finally:
        m.pos = own
