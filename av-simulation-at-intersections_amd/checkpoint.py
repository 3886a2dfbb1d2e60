"""Checkpoints of a running loop: the slabs that hold a loop's whole live state at every C-th tick
(history.CHECKPOINT states the layout), written between two calls of the loop's entry point by one launch
(jsim_loop_checkpoint_save), put back by the same launch the other way round (restore), gathered row by row into a new loop
(jsim_loop_checkpoint_load: the warm forks of closed_loop.py) and written to / read from one .npz.  No loop kernel knows of it: the
fused K-tick launches are bit-identical to shorter launches back to back, so a run is cut at the checkpoint ticks
(history.checkpoint_cuts) and the state is copied between the pieces."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _cabi, history

_TORCH = {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}


def _table(ptrs):
    """A host array of device pointers as the entry points take it."""
    return np.ascontiguousarray(ptrs, dtype=np.uint64)


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def check_every(every, record) -> int:
    """checkpoint_every of a loop's constructor, before any device work: an integer >= 1, and only with a recorder."""
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"checkpoint_every must be an integer >= 1, got {every!r}")
    if not record:
        raise ValueError("checkpoint_every needs a recorder: record must be a positive number of ticks")
    return int(every)


def live(owners: dict, a) -> Optional[torch.Tensor]:
    """The live tensor of array `a` (a history.CHECKPOINT row) among a loop's `owners`, or None when the loop has none."""
    t = getattr(owners.get(a.owner), a.attr, None)
    return t if (t is not None and t.numel() > 0) else None


class Checkpoints:
    """The checkpoint slabs of one loop.  owners: the objects history.CHECKPOINT names ("loop", "eng" and, for a glue loop, "pre"
    and "obst"); every: C; cap: the recorder's; n_slots: default cap // C + 1 (more, to set a smaller C after a restore).
    slabs[name] is a device tensor [n_slots] + the array's shape; slot_tick[s] the tick slot s holds (-1: not written); t the loop's
    tick count, kept on the host."""

    def __init__(self, owners: dict, every: int, cap: int, n_slots: Optional[int] = None):
        self.owners, self.every, self.cap = owners, int(every), int(cap)
        need = history.checkpoint_slots(self.every, self.cap)
        self.n_slots = need if n_slots is None else int(n_slots)
        if self.n_slots < need:
            raise ValueError(f"checkpoint_slots={n_slots} holds fewer than the {need} slots of checkpoint_every={every} over {cap} ticks")
        eng = self.eng = owners["eng"]
        self.arrays = [a for a in history.CHECKPOINT if self._live(a) is not None]
        if len(self.arrays) > history.CHECKPOINT_MAX_ARRAYS:
            raise ValueError(f"{len(self.arrays)} arrays in one checkpoint (max {history.CHECKPOINT_MAX_ARRAYS})")
        self.slabs = {a.name: torch.zeros(self.n_slots, *self._live(a).shape, dtype=_TORCH[a.dtype], device=eng.device)
                      for a in self.arrays}
        self._bytes = np.array([self.slabs[a.name][0].numel() * self.slabs[a.name].element_size() for a in self.arrays], dtype=np.int64)
        self.slot_tick = np.full(self.n_slots, -1, dtype=np.int64)
        self.t = 0

    def _live(self, a) -> Optional[torch.Tensor]:
        return live(self.owners, a)

    def _copy(self, slot: int, save: bool):
        """One launch: every array into its slot (save), or out of it."""
        live = _table([self._live(a).data_ptr() for a in self.arrays])
        slab = _table([self.slabs[a.name].data_ptr() for a in self.arrays]) + (self._bytes * slot).astype(np.uint64)
        src, dst = (live, slab) if save else (slab, live)
        eng = self.eng
        _cabi.check(eng.lib.jsim_loop_checkpoint_save(eng._ctx, len(self.arrays), _vp(src), _vp(dst), _vp(self._bytes), eng._stream()),
                    eng._ctx, "jsim_loop_checkpoint_save")

    def save(self, slot: int):
        """The live state into slot `slot`, as the state at the start of tick t."""
        self._copy(slot, True)
        self.slot_tick[slot] = self.t

    def pieces(self, n: int):
        """run(n) in pieces (history.checkpoint_cuts): yields each piece's ticks for the caller to issue, a slot saved ahead of it
        where one is due."""
        for slot, m in history.checkpoint_cuts(self.t, n, self.every, self.cap):
            if slot >= 0:
                self.save(slot)
            yield m
            self.t += m

    def written(self):
        return [(int(s), int(self.slot_tick[s])) for s in np.flatnonzero(self.slot_tick >= 0)]

    def check_slot(self, slot) -> int:
        if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.n_slots \
                or self.slot_tick[slot] < 0:
            raise ValueError(f"slot {slot!r} holds no checkpoint (written slots and their ticks: {self.written()})")
        return int(slot)

    def restore(self, slot):
        """Slot `slot` back into the live tensors, the device tick counter among them; the host tick count follows, and the slots of
        later ticks, which belong to what was undone, hold nothing any more."""
        slot = self.check_slot(slot)
        self._copy(slot, False)
        self.t = int(self.slot_tick[slot])
        self.slot_tick[self.slot_tick > self.t] = -1

    def set_every(self, every):
        every = check_every(every, self.cap)
        need = history.checkpoint_slots(every, self.cap)
        if need > self.n_slots:
            raise ValueError(f"checkpoint_every={every} over {self.cap} recorded ticks needs {need} slots, the loop has {self.n_slots} "
                             f"(construct it with checkpoint_slots={need})")
        self.every = every

    def load_into(self, owners: dict, ego, slot, veh_src, veh_slot):
        """jsim_loop_checkpoint_load: rows (ego[r], slot[r]) of these slabs into the live tensors of a new loop (`owners`: its
        objects, as this loop's), and the vehicles (veh_src[o], veh_slot[o]) into its scripted vehicles' states."""
        theirs = [a for a in history.CHECKPOINT if a.per == "ego" and live(owners, a) is not None]
        per_ego = [a for a in self.arrays if a in theirs]
        missing = [a.name for a in theirs if a not in self.arrays]
        if missing:
            raise ValueError(f"the source loop has no checkpoint of {missing}")
        B = self.eng.B
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
        ego, slot, veh_src, veh_slot = i32(ego), i32(slot), i32(veh_src), i32(veh_slot)
        slab = _table([self.slabs[a.name].data_ptr() for a in per_ego])
        dst = _table([live(owners, a).data_ptr() for a in per_ego])
        row_bytes = np.array([self.slabs[a.name][0, 0].numel() * self.slabs[a.name].element_size() for a in per_ego], dtype=np.int64)
        written = i32(self.slot_tick >= 0)
        obs = self.slabs.get("obs_state")
        obst = owners.get("obst")
        n_veh = int(veh_src.size)
        if n_veh and (obs is None or obst is None or obst.n != n_veh):
            raise ValueError(f"{n_veh} vehicles to load, but the source holds {'none' if obs is None else obs.shape[1]} and the new "
                             f"loop {0 if obst is None else obst.n}")
        eng = owners["eng"]
        _cabi.check(eng.lib.jsim_loop_checkpoint_load(
            eng._ctx, B, self.n_slots, _vp(written), int(ego.size), _vp(ego), _vp(slot), len(per_ego), _vp(slab), _vp(dst), _vp(row_bytes),
            0 if obs is None else int(obs.shape[1]), None if obs is None else C.c_void_p(obs.data_ptr()), n_veh, _vp(veh_src),
            _vp(veh_slot), C.c_void_p(obst.state.data_ptr()) if n_veh else None, eng._stream()), eng._ctx, "jsim_loop_checkpoint_load")

    # ---- one .npz of the slabs and the layout names
    def to_file(self, path, kind: str):
        np.savez(path, **history.checkpoint_file({k: v.cpu().numpy() for k, v in self.slabs.items()}, self.every, self.cap,
                                                 self.slot_tick, kind))

    def from_file(self, path, kind: str):
        slabs, meta = history.read_checkpoint_file(path)
        if meta["kind"] != kind:
            raise ValueError(f"{path} holds the checkpoints of a {meta['kind']}, this loop is a {kind}")
        if list(slabs) != [a.name for a in self.arrays]:
            raise ValueError(f"{path} holds {list(slabs)}, this loop's state is {[a.name for a in self.arrays]}")
        for k, a in slabs.items():
            if tuple(a.shape) != tuple(self.slabs[k].shape):
                raise ValueError(f"{path}: {k} is {a.shape}, this loop's slab {tuple(self.slabs[k].shape)}")
        if meta["cap"] != self.cap:
            raise ValueError(f"{path} was recorded with record={meta['cap']}, this loop with record={self.cap}")
        for k, a in slabs.items():
            self.slabs[k].copy_(torch.from_numpy(a))
        self.slot_tick[:] = meta["slot_tick"]


class Checkpointed:
    """What ClosedLoop and the glue loops share of checkpoints: `_ck` is the loop's Checkpoints, or None."""

    _ck: Optional[Checkpoints] = None

    def _pieces(self, n: int):
        """The pieces run(n) issues: n itself without checkpoints (a tuple of one: no generator on the path of a loop that keeps none)."""
        return (int(n),) if self._ck is None else self._ck.pieces(int(n))

    def _need_ck(self) -> Checkpoints:
        if self._ck is None:
            raise ValueError("this loop keeps no checkpoints (checkpoint_every=..., together with record=...)")
        return self._ck

    @property
    def checkpoint_every(self) -> Optional[int]:
        return None if self._ck is None else self._ck.every

    @checkpoint_every.setter
    def checkpoint_every(self, every):
        """Another C for the ticks that follow (after a restore: 1 makes a window dense, so that any tick of it can be forked).  Slot
        t // C is written at tick t; the slots' ticks are listed in `checkpoints`.  ValueError: the loop's n_slots do not hold it."""
        self._need_ck().set_every(every)

    @property
    def checkpoints(self):
        """[(slot, tick)] of the written slots."""
        return [] if self._ck is None else self._ck.written()

    def restore(self, slot: int):
        """Put slot `slot` back into this loop, the device tick counter included: the loop stands at the slot's tick again and the
        recorder goes on writing there.  ValueError: no checkpoints, a slot that is not written."""
        self._need_ck().restore(slot)

    def save_checkpoints(self, path):
        """The slabs and the layout names as one .npz (history.checkpoint_file): a loop built the same way in another process takes
        them with load_checkpoints and goes on from any slot with restore.  The state the loop stands at is saved first when its tick
        is a checkpoint tick.  Synchronises (device -> host copies)."""
        ck = self._need_ck()
        if ck.t % ck.every == 0 and ck.t <= ck.cap:
            ck.save(ck.t // ck.every)
        ck.to_file(path, type(self).__name__)

    def load_checkpoints(self, path):
        """Take the slabs of a file save_checkpoints wrote into this loop's (same class, batch, horizon, vehicles and record);
        restore(slot) then continues from one.  ValueError: a file of another loop."""
        self._need_ck().from_file(path, type(self).__name__)
