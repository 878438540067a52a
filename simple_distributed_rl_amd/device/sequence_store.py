"""Agent57's sequence replay in HBM: a float32 frame ring, one packed record per stored sequence, and one libsrlx launch
(`srlx_seq_gather`) that assembles a sampled batch into the tensors `agent57.Trainer.train` feeds the networks.

The worker emits the whole window of L = burnin + sequence_length + 1 steps on every environment step, and consecutive windows share L - 1 of their L
observation OBJECTS (`agent57.Worker._add_memory` copies the list, not the arrays).  `SequenceLedger` (host, numpy only) recognises a frame by object identity
against the frames of the previous add, so every distinct observation is uploaded once; `DeviceSequenceStore` owns the HBM tensors and the pinned staging.

Contract on mutation: a frame is snapshotted when its object is first seen.  An observation array that is mutated in place after it was handed to `add` is
outside the contract (the later windows that share the object keep the snapshot).  The reference's own `compress=False` memory keeps references to the same
objects and has the same exposure, in the other direction (there every stored window would change).

The E-lane engine (device/agent57.py) has a store of its own below: `LaneLedger` / `LaneSequenceStore` keep every per-step field once in time-major
rings `[T][E]`, and a window is a view of them (`srlx_seq_lane_push`, `srlx_seq_lane_gather`).  `R2D2LaneStore` (device/r2d2.py) is the same
ring with R2D2's fields over the same ledger (`srlx_r2d2_lane_push`, `srlx_r2d2_lane_gather`)."""
from typing import Any, List, Optional

import numpy as np

_NO_REF = np.iinfo(np.int64).max


def _round4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def fill_invalid_mask(mask: np.ndarray, invalid_lists) -> bool:
    """mask uint8 [n][A] := 0, then mask[i, a] = 1 for every action id a in invalid_lists[i]; returns whether any bit was set.  numpy only: the one loop behind
    every invalid-action mask the plugins and the sequence store hand to libsrlx."""
    mask[...] = 0
    any_invalid = False
    for i, lst in enumerate(invalid_lists):
        for a in lst:
            mask[i, a] = 1
            any_invalid = True
    return any_invalid


class RecordLayout:
    """Dword offsets of one packed sequence record (include/srlx.h, "Agent57 sequence store")."""

    def __init__(self, L: int, S: int, A: int, H: int):
        self.L, self.S, self.A, self.H = int(L), int(S), int(A), int(H)
        L, S, A, H = self.L, self.S, self.A, self.H
        self.table, self.actions, self.r_ext, self.r_int, self.undone = 0, L, 2 * L, 3 * L, 4 * L
        self.actor = 4 * L + S
        self.hidden = self.actor + 1
        self.invalid = self.hidden + 4 * H  # dwords; the mask is S * A bytes from here
        self.dwords = _round4(self.invalid + (S * A + 3) // 4)

    def pack(self, row: np.ndarray, table: np.ndarray, item) -> bool:
        """Writes `item` (the list `agent57.Worker._add_memory` builds) with its frame table into `row` (int32 [dwords]); returns whether any step has an
        invalid action.  Values are converted exactly as `SequenceBatch.from_items` converts them on the host path (float32 casts, argmax of the one-hot actions)."""
        L, S, A, H = self.L, self.S, self.A, self.H
        f32, u8 = row.view(np.float32), row.view(np.uint8)
        row[:L] = table
        row[self.actions : self.actions + L] = np.argmax(np.asarray(item[1]), axis=1)
        f32[self.r_ext : self.r_ext + L] = item[2]
        f32[self.r_int : self.r_int + L] = item[3]
        f32[self.undone : self.undone + S] = item[4]
        row[self.actor] = item[5]
        for k, part in enumerate((item[7][0], item[7][1], item[8][0], item[8][1])):
            f32[self.hidden + k * H : self.hidden + (k + 1) * H] = np.asarray(part, dtype=np.float32).reshape(-1)
        return fill_invalid_mask(u8[4 * self.invalid : 4 * self.invalid + S * A].reshape(S, A), item[6])


class LedgerError(RuntimeError):
    """The frame ring cannot take this add without overwriting a frame a live sequence still references."""


class Plan:
    """What one add does: `uploads` = [(frame slot, frame object)], `table` = int32 [L] frame slots (-1: an all-zero frame), `seq_slot` = serial % seq_capacity."""

    __slots__ = ("serial", "seq_slot", "table", "uploads")

    def __init__(self, serial, seq_slot, table, uploads):
        self.serial, self.seq_slot, self.table, self.uploads = serial, seq_slot, table, uploads


class SequenceLedger:
    """Decides, for the stream of items `memory.add` receives, which frames are new, the frame slot of each, the item's frame table and its sequence slot.

    Invariant: no live sequence (one of the last `seq_capacity` adds) references a frame slot that has been overwritten.  Upload number u takes slot
    u % frame_capacity and is overwritten by upload u + frame_capacity; `plan` refuses (LedgerError, before anything is changed) an add whose uploads would
    overwrite an upload that a live sequence, the new one included, references.

    Ring size: in the in-order worker stream an episode of n steps makes n + L - 1 adds and n + 1 uploads (the reset observation and one per step; the padding
    is all-zero and takes no slot), so any run of W consecutive adds makes at most W + 1 uploads (whole episodes at most one per add since L >= 2, a trailing
    partial episode of k adds k + 1).  The oldest live sequence references a frame uploaded at most L - 1 adds before it, so every live reference is among the
    last seq_capacity + L uploads: frame_capacity >= seq_capacity + L + 1 is enough, and the default seq_capacity + 2 L leaves L - 1 slots of slack.

    An object that stays around (an environment that hands out one array again and again) is uploaded again once it is older than `refresh_age` uploads:
    half of what the ring holds beyond seq_capacity, L - 1 at the default size, which an in-order stream never reaches.  Items that share no frame objects
    (unpickled ones) make L uploads per add and need frame_capacity >= (seq_capacity + 1) L."""

    def __init__(self, seq_capacity: int, window: int, frame_capacity: Optional[int] = None):
        self.seq_capacity, self.L = int(seq_capacity), int(window)
        if self.seq_capacity < 1 or self.L < 2:
            raise ValueError(f"SequenceLedger: seq_capacity {seq_capacity} >= 1 and window {window} >= 2 required")
        need = self.seq_capacity + 2 * self.L
        self.frame_capacity = need if frame_capacity is None else int(frame_capacity)
        if self.frame_capacity < need:
            raise ValueError(f"SequenceLedger: frame_capacity {self.frame_capacity} below seq_capacity + 2 * window = {need}")
        self.refresh_age = (self.frame_capacity - self.seq_capacity - 2) // 2
        self.serial = 0  # adds so far
        self.uploads = 0  # frame uploads so far
        self._known = {}  # id(frame) -> (frame, upload number or -1) for the frames of the previous add; holding the objects keeps the ids valid
        self._seq_min = np.full(self.seq_capacity, _NO_REF, np.int64)  # per sequence slot: the oldest upload it references
        self._floor = _NO_REF  # a lower bound of min(_seq_min over live sequences): exact after a recount, lowered by every add in between

    def is_live(self, serial: int) -> bool:
        return self.serial - self.seq_capacity <= serial < self.serial

    def plan(self, frames) -> Plan:
        L, F = self.L, self.frame_capacity
        if len(frames) != L:
            raise ValueError(f"SequenceLedger: an item of {len(frames)} frames, window is {L}")
        U, known, seen, uploads = self.uploads, self._known, {}, []
        table = np.empty(L, np.int32)
        mine = _NO_REF
        for l, f in enumerate(frames):
            k = id(f)
            e = seen.get(k)
            if e is None:
                e = known.get(k)
                if e is not None and (e[0] is not f or (e[1] >= 0 and U - e[1] > self.refresh_age)):
                    e = None  # (a long-lived object: upload it again before its slot comes up for reuse)
                if e is None:
                    if np.asarray(f).any():
                        e = (f, U)
                        uploads.append((U % F, f))
                        U += 1
                    else:
                        e = (f, -1)
                seen[k] = e
            u = e[1]
            table[l] = u % F if u >= 0 else -1
            if 0 <= u < mine:
                mine = u
        slot = self.serial % self.seq_capacity
        oldest_kept = U - F  # uploads below this number are overwritten once this add's uploads are made
        floor = self._floor
        if oldest_kept > min(floor, mine):
            live = self._seq_min.copy()
            live[slot] = _NO_REF  # the sequence this add evicts
            floor = int(live.min())
            if oldest_kept > min(floor, mine):
                raise LedgerError(
                    f"SequenceLedger: add {self.serial} needs {len(uploads)} new frame slots, and upload {U - 1} would overwrite a frame that a live sequence still "
                    f"references (frame ring {F} slots, {self.seq_capacity} live sequences of {L} frames). Items that share no frame objects with their "
                    f"predecessor, such as unpickled ones, need {L} slots per add: frame_capacity >= {(self.seq_capacity + 1) * L}.")
        self._floor = min(floor, mine)
        self._seq_min[slot] = mine
        self._known = seen
        self.uploads = U
        plan = Plan(self.serial, slot, table, uploads)
        self.serial += 1
        return plan

    def state(self) -> dict:
        """Everything but the identity cache (objects do not survive a backup: the first add after a restore uploads its whole window)."""
        return dict(seq_capacity=self.seq_capacity, window=self.L, frame_capacity=self.frame_capacity, serial=self.serial, uploads=self.uploads,
                    seq_min=self._seq_min.copy())

    def load_state(self, st: dict) -> None:
        if (st["seq_capacity"], st["window"], st["frame_capacity"]) != (self.seq_capacity, self.L, self.frame_capacity):
            raise ValueError("SequenceLedger: the backup was taken with another capacity or window")
        self.serial, self.uploads = int(st["serial"]), int(st["uploads"])
        self._seq_min = np.array(st["seq_min"], np.int64)
        self._known = {}
        live = self._seq_min.copy()
        if self.serial < self.seq_capacity:
            live[self.serial :] = _NO_REF
        self._floor = int(live.min())


class SequenceBatch:
    """A gathered batch: the device tensors `agent57.Trainer.train` would have built from a list of items.  `any_invalid` tells whether any gathered step
    has an invalid action (the host path passes `invalid=None` to the TD kernel when none has)."""

    __slots__ = ("states", "act_idx", "r_ext", "r_int", "dones", "invalid", "actor", "h_ext", "c_ext", "h_int", "c_int", "any_invalid")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __len__(self) -> int:
        return int(self.actor.shape[0])

    def tensors(self) -> dict:
        return {k: getattr(self, k) for k in self.__slots__ if k != "any_invalid"}

    @classmethod
    def from_items(cls, items, S: int, A: int, device) -> "SequenceBatch":
        """The same batch from a list of items (the lists `agent57.Worker._add_memory` builds, as the host memory samples them), with the reference's
        conversions (model_torch.py:300-346): float32 casts, argmax of the one-hot actions.  Every tensor goes to `device` ("cpu" works) in one copy."""
        import torch

        states, onehot_actions, r_ext, r_int, dones, actors, invalid_lists, hidden_ext, hidden_int = zip(*items)
        f32 = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32), device=device)  # noqa: E731
        hid = lambda hs, k: f32([h[k] for h in hs]).flatten(1)  # noqa: E731  ([B][1][H], as the worker keeps them, -> [B][H])
        inv = np.empty((len(items), S, A), np.uint8)
        any_invalid = fill_invalid_mask(inv.reshape(-1, A), [lst for per_step in invalid_lists for lst in per_step])
        return cls(states=f32(states), act_idx=torch.as_tensor(np.argmax(np.asarray(onehot_actions), axis=2).astype(np.int64), device=device), r_ext=f32(r_ext),
                   r_int=f32(r_int), dones=f32(dones), invalid=torch.from_numpy(inv).to(device), actor=torch.as_tensor(np.asarray(actors, dtype=np.int64), device=device),
                   h_ext=hid(hidden_ext, 0), c_ext=hid(hidden_ext, 1), h_int=hid(hidden_int, 0), c_int=hid(hidden_int, 1), any_invalid=any_invalid)


class DeviceSequenceStore:
    """The HBM side: frame ring [frame_capacity][stride] float32 (stride = frame_elems rounded up to 4 floats: rows start on 16 bytes), records
    [seq_capacity][dwords] int32, one host flag per sequence slot, and pinned staging rows.

    `add` applies a ledger plan with asynchronous copies on torch's current stream: one frame copy per new frame and one packed record copy, and it does not
    synchronise (a staging row is reused only after the copy that read it last has completed; that wait is over long before the row comes round again).
    `gather` is one `srlx_seq_gather` launch on the current stream, so adds and gathers issued on one stream are ordered."""

    FORMAT = "srlx-agent57-seqstore-1"

    def __init__(self, device, seq_capacity: int, window: int, sequence_length: int, n_actions: int, units: int, frame_shape, frame_capacity: Optional[int] = None):
        import torch

        from simple_distributed_rl_amd import _native as N
        from simple_distributed_rl_amd.algorithms._device_ops import require_gpu

        self.device = require_gpu(str(device))
        self._N, self._lib = N, N.lib()
        self.frame_shape = tuple(int(d) for d in frame_shape)
        self.frame_elems = int(np.prod(self.frame_shape, dtype=np.int64))
        self.stride = _round4(self.frame_elems)
        self.layout = RecordLayout(window, sequence_length, n_actions, units)
        lay = self.layout
        if self._lib.srlx_seq_record_dwords(lay.L, lay.S, lay.A, lay.H) != lay.dwords:
            raise ValueError(f"sequence store: window {lay.L}, sequence {lay.S}, actions {lay.A}, units {lay.H} are outside srlx_seq_gather's envelope (srlx.h)")
        if not 1 <= self.frame_elems <= 1 << 20:
            raise ValueError(f"sequence store: a frame of {self.frame_elems} elements is outside srlx_seq_gather's envelope (1..2^20)")
        self.ledger = SequenceLedger(seq_capacity, window, frame_capacity)
        led = self.ledger
        self.ring = torch.empty((led.frame_capacity, self.stride), dtype=torch.float32, device=self.device)
        self.records = torch.zeros((led.seq_capacity, lay.dwords), dtype=torch.int32, device=self.device)
        self.any_invalid = np.zeros(led.seq_capacity, bool)
        self._stage_frames = torch.empty((max(4 * lay.L, 16), self.stride), dtype=torch.float32, pin_memory=True)
        self._stage_records = torch.zeros((64, lay.dwords), dtype=torch.int32, pin_memory=True)
        self._np_frames, self._np_records = self._stage_frames.numpy(), self._stage_records.numpy()
        self._frame_fence: List[Any] = [None] * self._stage_frames.shape[0]  # per staging row: the event after the copy that read it last
        self._record_fence: List[Any] = [None] * self._stage_records.shape[0]
        self._next_frame_row = self._next_record_row = 0
        self.h2d_bytes = 0  # counted, for the probe

    # ---- adds --------------------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _claim(fences, row):
        ev = fences[row]
        if ev is not None:
            ev.synchronize()  # (returns at once unless the copy issued a whole staging ring ago is still pending)
            fences[row] = None

    def add(self, item) -> int:
        """Plans and uploads one item; returns its serial (the opaque item the priority memory keeps)."""
        import torch

        plan = self.ledger.plan(item[0])
        n_frame_rows, elems = len(self._frame_fence), self.frame_elems
        if len(plan.uploads) > n_frame_rows:
            raise LedgerError(f"sequence store: {len(plan.uploads)} new frames in one add, staging holds {n_frame_rows}")
        used_f = []
        for slot, frame in plan.uploads:
            a = np.asarray(frame)
            if a.size != elems:
                raise ValueError(f"sequence store: a frame of shape {a.shape}, the store holds {self.frame_shape}")
            r = self._next_frame_row
            self._next_frame_row = (r + 1) % n_frame_rows
            self._claim(self._frame_fence, r)
            np.copyto(self._np_frames[r, :elems], a.reshape(-1), casting="unsafe")  # (the float32 cast of np.asarray(states, dtype=np.float32))
            self.ring[slot].copy_(self._stage_frames[r], non_blocking=True)
            used_f.append(r)
        r = self._next_record_row
        self._next_record_row = (r + 1) % len(self._record_fence)
        self._claim(self._record_fence, r)
        self.any_invalid[plan.seq_slot] = self.layout.pack(self._np_records[r], plan.table, item)
        self.records[plan.seq_slot].copy_(self._stage_records[r], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._record_fence[r] = ev
        for fr in used_f:
            self._frame_fence[fr] = ev
        self.h2d_bytes += 4 * (len(used_f) * self.stride + self.layout.dwords)
        return plan.serial

    # ---- batches -----------------------------------------------------------------------------------------------------------------------------------------
    def gather_serials(self, serials) -> SequenceBatch:
        led = self.ledger
        for s in serials:
            if not led.is_live(int(s)):
                raise LedgerError(f"sequence store: sequence {s} is not among the last {led.seq_capacity} adds ({led.serial} so far)")
        return self.gather([int(s) % led.seq_capacity for s in serials])

    def gather(self, slots) -> SequenceBatch:
        import torch

        N, lay, led, d = self._N, self.layout, self.ledger, self.device
        slots = [int(s) for s in slots]
        B = len(slots)
        if B < 1 or min(slots) < 0 or max(slots) >= led.seq_capacity:
            raise ValueError(f"sequence store: {B} slots, each in 0..{led.seq_capacity - 1}, required")
        idx = torch.tensor(slots, dtype=torch.int64, device=d)
        L, S, A, H = lay.L, lay.S, lay.A, lay.H
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=d)  # noqa: E731
        out = dict(states=f32(B, L, *self.frame_shape), act_idx=torch.empty((B, L), dtype=torch.int64, device=d), r_ext=f32(B, L), r_int=f32(B, L), dones=f32(B, S),
                   invalid=torch.empty((B, S, A), dtype=torch.uint8, device=d), actor=torch.empty(B, dtype=torch.int64, device=d), h_ext=f32(B, H), c_ext=f32(B, H),
                   h_int=f32(B, H), c_int=f32(B, H))
        self.gather_into(idx, out)
        self._keep = idx  # alive until the stream has run the launch
        return SequenceBatch(any_invalid=bool(self.any_invalid[slots].any()), **out)

    def gather_into(self, idx, out: dict) -> None:
        """The launch alone: `idx` int64 [B] on the device, `out` the eleven output tensors by SequenceBatch's names."""
        N, lay, led = self._N, self.layout, self.ledger
        N.check(self._lib.srlx_seq_gather(int(idx.shape[0]), lay.L, lay.S, lay.A, lay.H, self.frame_elems, self.stride, led.frame_capacity, led.seq_capacity, lay.dwords,
                                          N.tptr(idx), N.tptr(self.ring), N.tptr(self.records), *[N.tptr(out[k]) for k in SequenceBatch.__slots__[:-1]],
                                          N.torch_stream_ptr()))

    # ---- backup / restore (a format of this store: ring rows in use, records, flags, the ledger's counters) --------------------------------------------------
    def backup(self) -> dict:
        led = self.ledger
        used = min(led.uploads, led.frame_capacity)
        return dict(format=self.FORMAT, frame_shape=self.frame_shape, layout=(self.layout.L, self.layout.S, self.layout.A, self.layout.H),
                    ring=self.ring[:used].cpu().numpy(), records=self.records.cpu().numpy(), any_invalid=self.any_invalid.copy(), ledger=led.state())

    def restore(self, data: dict) -> None:
        import torch

        lay = self.layout
        if data.get("format") != self.FORMAT:
            raise ValueError(f"sequence store: not a backup of this store (format {data.get('format')!r})")
        if tuple(data["frame_shape"]) != self.frame_shape or tuple(data["layout"]) != (lay.L, lay.S, lay.A, lay.H):
            raise ValueError("sequence store: the backup was taken with another frame shape, window, action count or unit count")
        self.ledger.load_state(data["ledger"])
        ring = torch.from_numpy(np.ascontiguousarray(data["ring"], dtype=np.float32))
        self.ring[: ring.shape[0]].copy_(ring)
        self.records.copy_(torch.from_numpy(np.ascontiguousarray(data["records"], dtype=np.int32)))
        self.any_invalid = np.array(data["any_invalid"], bool)
        torch.cuda.synchronize(self.device)


# ---- E lock-stepped lanes: a window is a view of time-major rings ---------------------------------------------------------------------------------
def pad_action(seed: int, lane, position, n_actions: int):
    """The keyed pad action of lane position `position` (srlx.h, "Agent57 lane sequence ring"): rng_u64(seed, lane, position) % A, numpy, any shapes."""
    m64 = lambda z: _mix64(z)  # noqa: E731
    with np.errstate(over="ignore"):
        s = np.uint64(seed) + np.asarray(lane).astype(np.uint64) * np.uint64(0xD1342543DE82EF95)
        x = m64(m64(s) + np.asarray(position).astype(np.int64).astype(np.uint64) * np.uint64(0xAEF17502108EF2D9))
    return (x % np.uint64(n_actions)).astype(np.int64)


def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


class LaneLedger:
    """Host bookkeeping of the lane ring (numpy only): which ring position a lock-step takes, the serial of every emitted window and serial -> (lane e, absolute
    position t of the window's last real entry, flush offset k).

    Order: serials follow the lock-steps, lane-major within a lock-step; within a lane the step's window (k = 0) comes first, then, when the step ended the
    episode, its flush windows (k = 1..L-1 by default) -- the order `agent57.Worker.on_step` adds them in.  A lane that is `first` in a lock-step (it only delivers
    a new episode's first frame) emits nothing.

    Invariant: no live window (one of the last `seq_capacity` serials) references a ring position that has been overwritten.  Window (e, t, k) references the
    positions max(t - (L - 1) + k, t - age[t][e]) .. t; position t sits in row t % T and is overwritten by push t + T.  `push` refuses (LedgerError, before
    anything is changed) a lock-step that would overwrite a position one of the live windows references.

    Flush windows: `flush` is the number of windows a lane emits after the step that ended its episode, k = 1..flush.  The default is L - 1 (Agent57's worker
    shifts the whole window out); R2D2 passes sequence_length - 1 (`r2d2.Worker.on_step` flushes len(recent_rewards) - 1 times), which is 0 at S = 1.

    Ring length, for a flush count F.  Let w be the oldest live window, emitted at lock-step t0 by lane e0 with flush offset k0, and let the ring be at
    lock-step t = t0 + D.  w references positions >= t0 - (L - 1 - k0), and push t + 1 overwrites position t + 1 - T, which must be older:
    T >= D + L - k0 + 1.  Every window emitted after w up to lock-step t is live next to it, so there are at most seq_capacity - 1 = C - 1 of them; how large
    D - k0 can get is a question of how FEW windows a stream can emit after w.  An episode of n >= 1 steps takes n + 1 lock-steps (the one that delivers its
    first frame, then its steps) and emits n + F windows; serials are lane-major within a lock-step, so the other lanes' windows of t0 come after w only for
    the lanes behind e0: the fewest follow when e0 is the last lane.
      F >= 1: an episode emits at least as many windows as it takes lock-steps, so a lane emits at least D - 1 windows in lock-steps t0 + 1 .. t, and D - 1
              only if it is `first` at t0 + 1, that is, if its step at t0 ended an episode.  For lane e0 itself that costs the F - k0 >= 1 flush windows behind
              w, more than the one window it saves, and a later k0 lowers D - k0; so k0 = 0, lane e0 plays on (D windows), the other E - 1 lanes end an
              episode at t0 (D - 1 each): (E - 1)(D - 1) + D <= C - 1, D <= floor((C - 2) / E) + 1.
      F = 0:  a lane is never `first` in two consecutive lock-steps (an episode has at least one step), so it emits at least floor(D / 2) windows in lock-steps
              t0 + 1 .. t, reached by episodes of one step behind an episode that ended at t0, which costs lane e0 nothing here:
              E floor(D / 2) <= C - 1, floor(D / 2) <= floor((C - 1) / E) = c - 1 with c = ceil(C / E), D <= 2 c - 1.
    So
      F >= 1: T >= floor((C - 2) / E) + L + 2         F = 0: T >= 2 c + L
    is enough and is reached (`min_ring_len`): by a last lane that plays one long episode while the others end an episode of at least L - 1 steps together,
    and for F = 0 by lanes that end such an episode together and then play episodes of one step.  floor((C - 2) / E) + 1 <= c, so c + L + 1 rows are enough
    for every F >= 1 (one more than needed when E divides C - 1); the default adds L - 1 rows to that: c + 2 L, and 2 c + 2 L - 1 at F = 0."""

    def __init__(self, n_lanes: int, seq_capacity: int, window: int, ring_len: Optional[int] = None, flush: Optional[int] = None):
        self.E, self.seq_capacity, self.L = int(n_lanes), int(seq_capacity), int(window)
        self.flush = self.L - 1 if flush is None else int(flush)
        if not 0 <= self.flush <= self.L - 1:
            raise ValueError(f"LaneLedger: flush count {flush} outside 0..window - 1 = {self.L - 1}")
        if self.E < 1 or self.L < 2 or self.seq_capacity < self.E * (1 + self.flush):
            raise ValueError(f"LaneLedger: lanes {n_lanes} >= 1, window {window} >= 2 and seq_capacity {seq_capacity} >= lanes * {'window' if flush is None else '(1 + flush)'} "
                             "(one lock-step's windows) required")
        self.ring_len = self.default_ring_len(self.E, self.seq_capacity, self.L, self.flush) if ring_len is None else int(ring_len)
        if self.ring_len < self.L:
            raise ValueError(f"LaneLedger: ring_len {self.ring_len} below the window {self.L}")
        self.t = 0  # lock-steps pushed so far = the next position
        self.serial = 0  # windows emitted so far
        self.age = np.zeros(self.E, np.int64)  # of the last pushed position
        self._owes_first = np.zeros(self.E, bool)  # lanes whose last step ended their episode
        self._emitted = True  # (every push is followed by one emit)
        C = self.seq_capacity
        self._e, self._t, self._k, self._lo = (np.zeros(C, np.int64) for _ in range(4))  # per serial % seq_capacity; _lo: the oldest position the window references

    @staticmethod
    def min_ring_len(n_lanes: int, seq_capacity: int, window: int, flush: Optional[int] = None) -> int:
        """The shortest ring that never refuses an in-order stream (the class docstring's derivation); `flush` None: window - 1."""
        E, C, L = int(n_lanes), int(seq_capacity), int(window)
        span = (C - 2) // E + 1 if flush is None or int(flush) >= 1 else 2 * -(-C // E) - 1
        return span + L + 1

    @staticmethod
    def default_ring_len(n_lanes: int, seq_capacity: int, window: int, flush: Optional[int] = None) -> int:
        c = -(-int(seq_capacity) // int(n_lanes))
        return (c if flush is None or int(flush) >= 1 else 2 * c - 1) + 2 * int(window)

    def is_live(self, serial: int) -> bool:
        return self.serial - self.seq_capacity <= serial < self.serial

    def window_counts(self, first, done) -> np.ndarray:
        """Windows each lane emits in a lock-step: 1 per stepping lane, + `flush` (L - 1 by default) when its step ended the episode, 0 for `first` lanes."""
        first, done = np.asarray(first, bool), np.asarray(done, bool)
        return np.where(first, 0, 1 + done * self.flush).astype(np.int64)

    def push(self, first) -> int:
        """Claims the next ring position for a lock-step whose `first` lanes (bool [E]) only deliver a new episode's first frame; returns the position."""
        first = np.asarray(first, bool).reshape(-1)
        if first.shape[0] != self.E:
            raise ValueError(f"LaneLedger: a first mask of {first.shape[0]} lanes, the ring has {self.E}")
        if not self._emitted:
            raise RuntimeError("LaneLedger: push without the emit of the previous lock-step")
        if self.t == 0 and not first.all():
            raise ValueError("LaneLedger: every lane begins an episode at position 0")
        if (self._owes_first & ~first).any():
            raise ValueError(f"LaneLedger: lanes {np.nonzero(self._owes_first & ~first)[0].tolist()} ended their episode and must be first in this lock-step")
        t, C = self.t, self.seq_capacity
        gone = t - self.ring_len  # the position this push overwrites
        oldest = max(0, self.serial - C)
        if gone >= 0 and oldest < self.serial and gone >= self._t[oldest % C] - (self.L - 1):  # (serials are ordered by t: the cheap bound first)
            lo = self._lo[np.arange(oldest, self.serial) % C]
            if int(lo.min()) <= gone:
                s = oldest + int(np.argmax(lo <= gone))
                raise LedgerError(f"LaneLedger: lock-step {t} would overwrite position {gone}, which live window {s} (lane {self._e[s % C]}, position "
                                  f"{self._t[s % C]}, flush {self._k[s % C]}) still references (ring of {self.ring_len} rows, {C} live windows of {self.L} entries, "
                                  f"{self.E} lanes; {self.default_ring_len(self.E, C, self.L, self.flush)} rows never refuse)")
        self.age = np.where(first, 0, self.age + 1)
        self._first = first
        self.t = t + 1
        self._emitted = False
        return t

    def emit(self, done) -> np.ndarray:
        """Registers the windows of the lock-step just pushed, given which lanes' steps ended their episode (bool [E]); returns their serials, in order."""
        if self._emitted:
            raise RuntimeError("LaneLedger: emit without a push")
        done = np.asarray(done, bool).reshape(-1) & ~self._first
        counts = self.window_counts(self._first, done)
        n, t, C, L = int(counts.sum()), self.t - 1, self.seq_capacity, self.L
        lanes = np.repeat(np.arange(self.E), counts)
        k = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
        slots = (self.serial + np.arange(n)) % C
        self._e[slots], self._t[slots], self._k[slots] = lanes, t, k
        self._lo[slots] = t - np.minimum(L - 1 - k, self.age[lanes])
        serials = self.serial + np.arange(n)
        self.serial += n
        self._owes_first = done
        self._emitted = True
        return serials

    def descriptors(self, serials) -> np.ndarray:
        """int64 [B][3]: (lane, position, flush offset) of live serials."""
        s = np.asarray(serials, np.int64).reshape(-1)
        if s.size and (s.min() < self.serial - self.seq_capacity or s.max() >= self.serial):
            bad = int(s[(s < self.serial - self.seq_capacity) | (s >= self.serial)][0])
            raise LedgerError(f"lane store: window {bad} is not among the last {self.seq_capacity} emitted ({self.serial} so far)")
        i = s % self.seq_capacity
        return np.stack([self._e[i], self._t[i], self._k[i]], axis=1)


class LaneSequenceStore:
    """The HBM side of the lane ring: frames [T][E][stride] float32 (stride = frame_elems rounded up to 4 floats), scalars [T][E][8] int32, invalid masks
    [T][E][A] uint8, recurrent vectors [T][E][4][H] float32, and a `LaneLedger`.  `push` is one `srlx_seq_lane_push` launch and `gather` one
    `srlx_seq_lane_gather` launch on torch's current stream, so pushes and gathers issued on one stream are ordered; neither synchronises."""

    def __init__(self, device, n_lanes: int, seq_capacity: int, window: int, sequence_length: int, n_actions: int, units: int, frame_shape, seed: int = 0,
                 ring_len: Optional[int] = None):
        import torch

        from simple_distributed_rl_amd import _native as N
        from simple_distributed_rl_amd.algorithms._device_ops import require_gpu

        self.device = require_gpu(str(device))
        self._N, self._lib = N, N.lib()
        self.frame_shape = tuple(int(d) for d in frame_shape)
        self.frame_elems = int(np.prod(self.frame_shape, dtype=np.int64))
        self.stride = _round4(self.frame_elems)
        self.layout = RecordLayout(window, sequence_length, n_actions, units)  # (L, S, A, H and the envelope check; the lane ring keeps no records)
        lay = self.layout
        if self._lib.srlx_seq_record_dwords(lay.L, lay.S, lay.A, lay.H) != lay.dwords:
            raise ValueError(f"lane store: window {lay.L}, sequence {lay.S}, actions {lay.A}, units {lay.H} are outside srlx_seq_lane_gather's envelope (srlx.h)")
        if not 1 <= self.frame_elems <= 1 << 20:
            raise ValueError(f"lane store: a frame of {self.frame_elems} elements is outside srlx_seq_lane_gather's envelope (1..2^20)")
        self.seed = int(seed) & ((1 << 64) - 1)
        self.ledger = LaneLedger(n_lanes, seq_capacity, window, ring_len)
        T, E, d = self.ledger.ring_len, self.ledger.E, self.device
        if T * E > 2**31 - 1:
            raise ValueError(f"lane store: {T} rows of {E} lanes are outside srlx_seq_lane_gather's envelope (T * E <= 2^31-1)")
        self.frames = torch.empty((T, E, self.stride), dtype=torch.float32, device=d)
        self.scalars = torch.zeros((T, E, 8), dtype=torch.int32, device=d)
        self.invalid = torch.zeros((T, E, lay.A), dtype=torch.uint8, device=d)
        self.hidden = torch.zeros((T, E, 4, lay.H), dtype=torch.float32, device=d)
        self.any_invalid = False  # whether any push has carried an invalid-action mask

    @staticmethod
    def ring_bytes(n_lanes: int, seq_capacity: int, window: int, n_actions: int, units: int, frame_elems: int, ring_len: Optional[int] = None) -> int:
        """HBM bytes of the four rings (host arithmetic)."""
        T = LaneLedger.default_ring_len(n_lanes, seq_capacity, window) if ring_len is None else int(ring_len)
        return T * int(n_lanes) * (4 * _round4(frame_elems) + 32 + int(n_actions) + 16 * int(units))

    def push(self, frames, action, r_ext, r_int, undone, actor, h_ext, c_ext, h_int, c_int, first, first_dev=None, invalid=None) -> int:
        """One lock-step of all lanes: device tensors frames float32 [E, ...], action / actor int32 [E], r_ext / r_int / undone float32 [E], the four recurrent
        vectors float32 [E][H] as they were before the networks consumed `frames`, `first` a host bool [E] (`first_dev`: the same mask as device uint8, uploaded
        here when not given), `invalid` uint8 [E][A] or None.  Returns the position; `emit(done)` then names the windows."""
        import torch

        N, lay, led = self._N, self.layout, self.ledger
        E = led.E
        first = np.asarray(first, bool).reshape(-1)
        want = {"frames": (torch.float32, E * self.frame_elems), "action": (torch.int32, E), "r_ext": (torch.float32, E), "r_int": (torch.float32, E),
                "undone": (torch.float32, E), "actor": (torch.int32, E), "h_ext": (torch.float32, E * lay.H), "c_ext": (torch.float32, E * lay.H),
                "h_int": (torch.float32, E * lay.H), "c_int": (torch.float32, E * lay.H)}
        got = dict(frames=frames, action=action, r_ext=r_ext, r_int=r_int, undone=undone, actor=actor, h_ext=h_ext, c_ext=c_ext, h_int=h_int, c_int=c_int)
        for k, (dt, n) in want.items():
            v = got[k]
            if v.dtype != dt or v.numel() != n or not v.is_contiguous() or v.device != self.device:
                raise ValueError(f"lane store: push argument {k} must be a contiguous {dt} tensor of {n} elements on {self.device}")
        if invalid is not None and (invalid.dtype != torch.uint8 or invalid.numel() != E * lay.A or not invalid.is_contiguous() or invalid.device != self.device):
            raise ValueError(f"lane store: push argument invalid must be a contiguous uint8 tensor of {E * lay.A} elements on {self.device}")
        t = led.push(first)  # (refuses before anything is written)
        if first_dev is None:
            first_dev = torch.from_numpy(first.astype(np.uint8)).to(self.device)
        self._keep_push = (got, first_dev, invalid)  # alive until the stream has run the launch
        self.any_invalid = self.any_invalid or invalid is not None
        N.check(self._lib.srlx_seq_lane_push(E, lay.A, lay.H, self.frame_elems, self.stride, led.ring_len, t, self.seed, N.tptr(frames), N.tptr(action), N.tptr(r_ext),
                                             N.tptr(r_int), N.tptr(undone), N.tptr(actor), N.tptr(invalid), N.tptr(h_ext), N.tptr(c_ext), N.tptr(h_int), N.tptr(c_int),
                                             N.tptr(first_dev), N.tptr(self.frames), N.tptr(self.scalars), N.tptr(self.invalid), N.tptr(self.hidden),
                                             N.torch_stream_ptr()))
        return t

    def emit(self, done) -> np.ndarray:
        return self.ledger.emit(done)

    def gather_serials(self, serials) -> SequenceBatch:
        return self.gather(self.ledger.descriptors(serials))

    def gather(self, descriptors) -> SequenceBatch:
        """descriptors: int64 [B][3] (lane, position, flush offset), host or device."""
        import torch

        lay, d = self.layout, self.device
        desc = torch.as_tensor(np.ascontiguousarray(descriptors, dtype=np.int64) if not torch.is_tensor(descriptors) else descriptors).to(d).contiguous()
        if desc.dim() != 2 or desc.shape[1] != 3 or desc.shape[0] < 1 or desc.dtype != torch.int64:
            raise ValueError("lane store: descriptors are int64 [B][3] with B >= 1")
        B, L, S, A, H = int(desc.shape[0]), lay.L, lay.S, lay.A, lay.H
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=d)  # noqa: E731
        out = dict(states=f32(B, L, *self.frame_shape), act_idx=torch.empty((B, L), dtype=torch.int64, device=d), r_ext=f32(B, L), r_int=f32(B, L), dones=f32(B, S),
                   invalid=torch.empty((B, S, A), dtype=torch.uint8, device=d), actor=torch.empty(B, dtype=torch.int64, device=d), h_ext=f32(B, H), c_ext=f32(B, H),
                   h_int=f32(B, H), c_int=f32(B, H))
        self.gather_into(desc, out)
        self._keep = desc  # alive until the stream has run the launch
        return SequenceBatch(any_invalid=self.any_invalid, **out)

    def gather_into(self, desc, out: dict) -> None:
        """The launch alone: `desc` int64 [B][3] on the device, `out` the eleven output tensors by SequenceBatch's names."""
        N, lay, led = self._N, self.layout, self.ledger
        N.check(self._lib.srlx_seq_lane_gather(int(desc.shape[0]), lay.L, lay.S, lay.A, lay.H, led.E, led.ring_len, self.frame_elems, self.stride, self.seed,
                                               N.tptr(desc), N.tptr(self.frames), N.tptr(self.scalars), N.tptr(self.invalid), N.tptr(self.hidden),
                                               *[N.tptr(out[k]) for k in SequenceBatch.__slots__[:-1]], N.torch_stream_ptr()))

    def backup(self) -> dict:
        raise RuntimeError("lane store: the lane ring has no backup format yet (its windows are views of rings the running lanes still write); back up a "
                           "'host' memory or the plugin's device store instead")


class R2D2LaneStore:
    """R2D2's lane ring in HBM (srlx.h, "R2D2 lane sequence ring"): frames [T][E][stride] float32, scalars [T][E][8] int32 (action, mu, reward,
    done, age), invalid masks [T][E][A] uint8 of each position's OWN observation, recurrent vectors [T][E][2][H] float32, and a `LaneLedger` with
    sequence_length - 1 flush windows.  `push` is one `srlx_r2d2_lane_push` launch and `gather` one `srlx_r2d2_lane_gather` launch on torch's current stream,
    so pushes and gathers issued on one stream are ordered; neither synchronises.  `gather` returns an `r2d2.SequenceBatch`."""

    def __init__(self, device, n_lanes: int, seq_capacity: int, window: int, sequence_length: int, n_actions: int, units: int, frame_shape, seed: int = 0,
                 ring_len: Optional[int] = None):
        import torch

        from simple_distributed_rl_amd import _native as N
        from simple_distributed_rl_amd.algorithms._device_ops import require_gpu

        self.device = require_gpu(str(device))
        self._N, self._lib = N, N.lib()
        self.frame_shape = tuple(int(d) for d in frame_shape)
        self.frame_elems = int(np.prod(self.frame_shape, dtype=np.int64))
        self.stride = _round4(self.frame_elems)
        self.L, self.S, self.A, self.H = int(window), int(sequence_length), int(n_actions), int(units)
        if self._lib.srlx_seq_record_dwords(self.L, self.S, self.A, self.H) < 0:  # (host arithmetic: the SRLX_SEQ_MAX_* envelope the R2D2 gather shares)
            raise ValueError(f"r2d2 lane store: window {self.L}, sequence {self.S}, actions {self.A}, units {self.H} are outside srlx_r2d2_lane_gather's envelope (srlx.h)")
        if not 1 <= self.frame_elems <= 1 << 20:
            raise ValueError(f"r2d2 lane store: a frame of {self.frame_elems} elements is outside srlx_r2d2_lane_gather's envelope (1..2^20)")
        self.seed = int(seed) & ((1 << 64) - 1)
        self.ledger = LaneLedger(n_lanes, seq_capacity, self.L, ring_len, flush=self.S - 1)
        T, E, d = self.ledger.ring_len, self.ledger.E, self.device
        if E > 65536 or T * E > 2**31 - 1:
            raise ValueError(f"r2d2 lane store: {T} rows of {E} lanes are outside srlx_r2d2_lane_gather's envelope (E <= 65536, T * E <= 2^31-1)")
        self.frames = torch.empty((T, E, self.stride), dtype=torch.float32, device=d)
        self.scalars = torch.zeros((T, E, 8), dtype=torch.int32, device=d)
        self.invalid = torch.zeros((T, E, self.A), dtype=torch.uint8, device=d)
        self.hidden = torch.zeros((T, E, 2, self.H), dtype=torch.float32, device=d)
        self.any_invalid = False  # whether any push has carried an invalid-action mask

    @staticmethod
    def ring_bytes(n_lanes: int, seq_capacity: int, window: int, sequence_length: int, n_actions: int, units: int, frame_elems: int,
                   ring_len: Optional[int] = None) -> int:
        """HBM bytes of the four rings (host arithmetic)."""
        T = LaneLedger.default_ring_len(n_lanes, seq_capacity, window, int(sequence_length) - 1) if ring_len is None else int(ring_len)
        return T * int(n_lanes) * (4 * _round4(frame_elems) + 32 + int(n_actions) + 8 * int(units))

    def push(self, frames, action, mu, reward, done, h, c, first, first_dev=None, invalid=None) -> int:
        """One lock-step of all lanes: device tensors frames float32 [E, ...], action int32 [E], mu / reward float32 [E], done uint8 [E] (the step terminated),
        h / c float32 [E][H] as they were before the network consumed `frames`, `first` a host bool [E] (`first_dev`: the same mask as device uint8, uploaded
        here when not given), `invalid` uint8 [E][A] (the masks of `frames`) or None.  Returns the position; `emit(done)` then names the windows."""
        import torch

        N, led = self._N, self.ledger
        E, A, H = led.E, self.A, self.H
        first = np.asarray(first, bool).reshape(-1)
        want = {"frames": (torch.float32, E * self.frame_elems), "action": (torch.int32, E), "mu": (torch.float32, E), "reward": (torch.float32, E),
                "done": (torch.uint8, E), "h": (torch.float32, E * H), "c": (torch.float32, E * H)}
        got = dict(frames=frames, action=action, mu=mu, reward=reward, done=done, h=h, c=c)
        for k, (dt, n) in want.items():
            v = got[k]
            if v.dtype != dt or v.numel() != n or not v.is_contiguous() or v.device != self.device:
                raise ValueError(f"r2d2 lane store: push argument {k} must be a contiguous {dt} tensor of {n} elements on {self.device}")
        if invalid is not None and (invalid.dtype != torch.uint8 or invalid.numel() != E * A or not invalid.is_contiguous() or invalid.device != self.device):
            raise ValueError(f"r2d2 lane store: push argument invalid must be a contiguous uint8 tensor of {E * A} elements on {self.device}")
        t = led.push(first)  # (refuses before anything is written)
        if first_dev is None:
            first_dev = torch.from_numpy(first.astype(np.uint8)).to(self.device)
        self._keep_push = (got, first_dev, invalid)  # alive until the stream has run the launch
        self.any_invalid = self.any_invalid or invalid is not None
        N.check(self._lib.srlx_r2d2_lane_push(E, A, H, self.frame_elems, self.stride, led.ring_len, t, self.seed, N.tptr(frames), N.tptr(action), N.tptr(mu),
                                              N.tptr(reward), N.tptr(done), N.tptr(invalid), N.tptr(h), N.tptr(c), N.tptr(first_dev), N.tptr(self.frames),
                                              N.tptr(self.scalars), N.tptr(self.invalid), N.tptr(self.hidden), N.torch_stream_ptr()))
        return t

    def emit(self, done) -> np.ndarray:
        return self.ledger.emit(done)

    def gather_serials(self, serials):
        return self.gather(self.ledger.descriptors(serials))

    def gather(self, descriptors):
        """descriptors: int64 [B][3] (lane, position, flush offset), host or device -> r2d2.SequenceBatch (`invalid_actions` None while no push has carried a
        mask, as `SequenceBatch.from_items` returns None when no item has an invalid action)."""
        import torch

        from simple_distributed_rl_amd.algorithms.r2d2 import SequenceBatch as R2D2Batch

        d = self.device
        desc = torch.as_tensor(np.ascontiguousarray(descriptors, dtype=np.int64) if not torch.is_tensor(descriptors) else descriptors).to(d).contiguous()
        if desc.dim() != 2 or desc.shape[1] != 3 or desc.shape[0] < 1 or desc.dtype != torch.int64:
            raise ValueError("r2d2 lane store: descriptors are int64 [B][3] with B >= 1")
        B, L, S, A, H = int(desc.shape[0]), self.L, self.S, self.A, self.H
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=d)  # noqa: E731
        out = dict(states=f32(B, L, *self.frame_shape), actions=torch.empty((B, S), dtype=torch.int32, device=d), probs=f32(B, S), rewards=f32(B, S),
                   dones=torch.empty((B, S), dtype=torch.uint8, device=d), invalid=torch.empty((B, S + 1, A), dtype=torch.uint8, device=d), h=f32(1, B, H), c=f32(1, B, H))
        self.gather_into(desc, out)
        self._keep = desc  # alive until the stream has run the launch
        return R2D2Batch(states=out["states"], actions=out["actions"], probs=out["probs"], rewards=out["rewards"], dones=out["dones"],
                         invalid_actions=out["invalid"] if self.any_invalid else None, hidden_states=(out["h"], out["c"]))

    GATHER_OUTPUTS = ("states", "actions", "probs", "rewards", "dones", "invalid", "h", "c")

    def gather_into(self, desc, out: dict) -> None:
        """The launch alone: `desc` int64 [B][3] on the device, `out` the eight output tensors by `GATHER_OUTPUTS`' names."""
        N, led = self._N, self.ledger
        N.check(self._lib.srlx_r2d2_lane_gather(int(desc.shape[0]), self.L, self.S, self.A, self.H, led.E, led.ring_len, self.frame_elems, self.stride, self.seed,
                                                N.tptr(desc), N.tptr(self.frames), N.tptr(self.scalars), N.tptr(self.invalid), N.tptr(self.hidden),
                                                *[N.tptr(out[k]) for k in self.GATHER_OUTPUTS], N.torch_stream_ptr()))

    def backup(self) -> dict:
        raise RuntimeError("r2d2 lane store: the lane ring has no backup format yet (its windows are views of rings the running lanes still write); back up a "
                           "plugin-path memory instead")
