"""Agent57's sequence replay in HBM: a float32 frame ring, one packed record per stored sequence, and one libsrlx launch
(`srlx_seq_gather`) that assembles a sampled batch into the tensors `agent57.Trainer.train` feeds the networks.

The worker emits the whole window of L = burnin + sequence_length + 1 steps on every environment step, and consecutive windows share L - 1 of their L
observation OBJECTS (`agent57.Worker._add_memory` copies the list, not the arrays).  `SequenceLedger` (host, numpy only) recognises a frame by object identity
against the frames of the previous add, so every distinct observation is uploaded once; `DeviceSequenceStore` owns the HBM tensors and the pinned staging.

Contract on mutation: a frame is snapshotted when its object is first seen.  An observation array that is mutated in place after it was handed to `add` is
outside the contract (the later windows that share the object keep the snapshot).  The reference's own `compress=False` memory keeps references to the same
objects and has the same exposure, in the other direction (there every stored window would change)."""
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
