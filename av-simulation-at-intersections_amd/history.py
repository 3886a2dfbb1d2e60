"""Per-tick History of every ego, as the reference's scenario scripts keep it (lib.simulation.History,
main/lib/simulation.py:50-88, and `obstacles_positions`, main/scenarios/mpc_intersection.py:95-96,159-161), rebuilt from what
the device recorder wrote (jsim_loop_set_recorder): rec [n][B][7] = x, y, yaw, v, delta, a, xref_deviation per tick, flags
[n][B] (FAILED / GOAL / AGE bits), obs [n][n_obs][6] = the scripted vehicles' get() tuples.  Pure numpy: the host-side half of
the recorder, testable without a device.  reason_series does the same for the per-tick stakeholder reasons,
conflict_episodes for the clearance and first contact of every episode (section 17), static_episodes for the static obstacles
(section 18), episode_rows for the per-episode table that is reduced on the device (section 19), cutoff_episodes for the glue's
collision cut-off of every tick (section 21); fork_rows, join and reasons_carry_at are the host side of a fork (section 22);
gap_episodes for the time gap between an ego and each vehicle (section 23); path_table and tracking_episodes for the projection of
every recorded pose onto a path (section 24); headway_episodes for the space headway, time headway and time to collision between
an ego and the vehicles on its path (section 25); prediction_curve and prediction_places for the error of every recorded prediction
against what the vehicle then did (section 28); CHECKPOINT, checkpoint_cuts, checkpoint_at and the checkpoint file are the host
side of a loop's checkpoints (section 30)."""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np

from ._header import constant as _c     # the limits and flags below are include/jsim_mpc.h's

FIELDS = ("x", "y", "yaw", "v", "delta", "a", "xref_deviation")
FAILED, GOAL, AGE = _c("JSIM_REC_FAILED"), _c("JSIM_REC_GOAL"), _c("JSIM_REC_AGE")
END_RUNNING, END_GOAL, END_AGE = 0, 1, 2  # how an episode ended (episodes())
# the columns of the episode table (Recorder.summary), in the order of JSIM_EP_* of include/jsim_mpc.h
EP_INT = ("ego", "k0", "n", "end", "failed", "dev_tick", "veh_tick", "veh_who", "veh_hit_tick", "veh_hit_frame", "st_tick", "st_who",
          "st_off_tick", "st_obstacle", "st_ticks_off", "replan_tick")
EP_DOUBLE = ("length", "v_mean", "v_max", "a_min", "a_max", "delta_absmax", "dev_max", "dev_mean", "veh_clear", "veh_hit_x",
             "veh_hit_y", "st_clear", "pm_min", "driver_min", "cyclist_min", "dist_min")
GAP_NONE, GAP_MAX_WINDOW = _c("JSIM_GAP_NONE"), _c("JSIM_GAP_MAX_WINDOW")
# the columns of Recorder.tracking's ep_i and ep_d, in the order of the JSIM_TRK_* enumerators of include/jsim_mpc.h
TRK_INT = ("ticks", "d_max_tick")
TRK_DOUBLE = ("d_max", "d2_mean", "yaw_max", "s_first", "s_last")
# the columns of Recorder.headway's ep_i and ep_d, in the order of the JSIM_HW_* enumerators of include/jsim_mpc.h
HW_INT = ("ticks", "lead_ticks", "gap_tick", "gap_who", "thw_tick", "ttc_tick", "ttc_who")
HW_DOUBLE = ("gap_min", "thw_min", "ttc_min", "thw_mean")
MAX_OBS = _c("JSIM_MAX_OBS")   # obstacles one ego's glue can hold (scripted vehicles, then group mates)


class Evaluator(NamedTuple):
    """One evaluator of the recorder: its entry point and its per-tick outputs [n][B]... as (key, numpy dtype, trailing shape), in
    the order of the entry point's declaration in include/jsim_mpc.h; `optional`: the keys the call takes as NULL, as a whole."""
    entry: str
    outputs: tuple
    optional: tuple = ()

    def keys(self, skip=()):
        return tuple(k for k, _, _ in self.outputs if k not in skip)


_F, _I = np.float64, np.int32
# what the Recorder allocates, hands to the entry point and reads back, what the tools time and what tests/test_recorder_outputs_cpu.py holds
# against the header.  Outputs that are not [n][B]... (first and carry of reasons, carry of cutoffs) stay with
# their methods.
EVALUATORS = {
    "reasons": Evaluator("jsim_loop_eval_reasons", (("val", _F, (4,)), ("timers", _F, (2,)), ("trig", _I, ()))),
    "conflicts": Evaluator("jsim_loop_eval_conflicts", (("clear", _F, ()), ("who", _I, ()), ("row", _I, ()), ("hit_tick", _I, ()),
                                                        ("hit_frame", _I, ()), ("hit_xy", _F, (2,)))),
    "gaps": Evaluator("jsim_loop_eval_gaps", (("off", np.int8, (MAX_OBS,)), ("ep_gap", _I, ()), ("ep_tick", _I, ()), ("ep_who", _I, ()),
                                              ("ep_off", _I, ()))),
    "static": Evaluator("jsim_loop_eval_static", (("clear", _F, ()), ("who", _I, ()), ("hit", _I, ()), ("off_tick", _I, ()))),
    "tracking": Evaluator("jsim_loop_eval_tracking", (("idx", _I, ()), ("seg", _I, ()), ("s", _F, ()), ("d", _F, ()), ("e_yaw", _F, ()),
                                                      ("ep_i", _I, (len(TRK_INT),)), ("ep_d", _F, (len(TRK_DOUBLE),)))),
    "headway": Evaluator("jsim_loop_eval_headway", (("lead", _I, ()), ("lead_gap", _F, ()), ("thw", _F, ()), ("ttc", _F, ()),
                                                    ("ttc_who", _I, ()), ("u_ego", _F, ()), ("ep_i", _I, (len(HW_INT),)),
                                                    ("ep_d", _F, (len(HW_DOUBLE),)), ("gap", _F, (MAX_OBS,)), ("lat", _F, (MAX_OBS,)),
                                                    ("rate", _F, (MAX_OBS,))), optional=("gap", "lat", "rate")),
    "cutoffs": Evaluator("jsim_loop_eval_cutoffs", (("status", _I, ()), ("idx", _I, ()), ("cut", _I, ()), ("hit", _I, ()),
                                                    ("first", _I, ()), ("col_xy", _F, (2,)))),
}


class RowOutputs(NamedTuple):
    """The outputs of an entry point whose rows are not the egos: (key, numpy dtype, leading axes, trailing shape) each, in the order
    of the declaration in include/jsim_mpc.h.  Leading "tick": [n][V]..., "row": [V]...; a trailing "n_steps" is the call's n_steps;
    `optional`: the keys the call takes as NULL."""
    entry: str
    outputs: tuple
    optional: tuple = ()

    def keys(self, skip=()):
        return tuple(k for k, _, _, _ in self.outputs if k not in skip)


# the columns of Recorder.predictions' pt_i and pt_d, in the order of the JSIM_PS_* enumerators of include/jsim_mpc.h
PS_INT = ("n", "hold", "max_at")
PS_DOUBLE = ("ade", "fde", "max", "lon", "lat", "yaw")
MAX_PRED = _c("JSIM_MAX_PRED")   # the longest prediction
# jsim_loop_score_predictions' outputs: rows are the recorded vehicles and then the egos, [n][V], so they stand
# beside EVALUATORS, not in it
PREDICTION_OUTPUTS = RowOutputs("jsim_loop_score_predictions",
                                (("pt_i", _I, "tick", (len(PS_INT),)), ("pt_d", _F, "tick", (len(PS_DOUBLE),)),
                                 ("step_sum", _F, "row", ("n_steps",)), ("step_cnt", _I, "row", ("n_steps",)),
                                 ("err", _F, "tick", ("n_steps",))), optional=("err",))
# The plan record (jsim_loop_set_plan_recorder): (key, numpy dtype, trailing shape) of its buffers [cap][B]...,
# in the order of the declaration; "T" is the engine's horizon.  Slot k holds eng.oa, eng.od, eng.status at the start of tick k.
# jsim_loop_score_plan_predictions scores them into PREDICTION_OUTPUTS' columns, rows = the egos.
PLAN_RECORD = (("plan_oa", _F, ("T",)), ("plan_od", _F, ("T",)), ("plan_status", _I, ()))


class CheckpointArray(NamedTuple):
    """One array of a loop's live state: its slab is [n_slots] + shape of dtype (`B`, `T`, `n_obs` are the loop's); the live tensor is
    attribute `attr` of the loop's `owner` -- "loop" (ClosedLoop), "eng" (BatchedMPC), "pre" (PreTick), "obst" (ScriptedObstacles).
    per: whose rows the leading axis counts -- "ego" (a fork gathers them row by row), "vehicle" (gathered per (source set, slot)) or
    "loop" (one value for the whole loop: restored, never gathered; a fork starts its own)."""
    name: str
    dtype: type
    shape: tuple
    owner: str
    attr: str
    per: str


_L = np.int64
# The checkpoint record (jsim_loop_checkpoint_save / _load): every buffer that a tick writes and a later tick
# reads -- from the argument lists of the entry points (_loop_args, _run_args, _advance_args), run_host_ticks and the stores of the
# kernels they launch.  Slot s holds them as they stand at the start of the slot's tick.  An array whose owner the loop does not have
# (a ClosedLoop has no glue) or whose tensor is None (cv_cut without the speed cut-off glue) or empty (no vehicles) has no slab.
# Not state: the step outputs (ox, oy, ov, oyaw, xref, active_mask, n_iter), hist, col_xy / first_idx / get_buf (written, never read
# by a tick) and x0_first (the recorder's, written once).
CHECKPOINT = (
    CheckpointArray("x0", _F, ("B", 4), "loop", "x0", "ego"),
    CheckpointArray("x0_spawn", _F, ("B", 4), "loop", "x0_spawn", "ego"),
    CheckpointArray("target_spawn", _L, ("B",), "loop", "target_spawn", "ego"),
    CheckpointArray("age", _I, ("B",), "loop", "age", "ego"),
    CheckpointArray("tick_counter", _I, (1,), "loop", "tick_counter", "loop"),
    CheckpointArray("n_respawn", _L, (1,), "loop", "n_respawn", "loop"),
    CheckpointArray("target_ind", _L, ("B",), "eng", "target_ind", "ego"),
    CheckpointArray("oa", _F, ("B", "T"), "eng", "oa", "ego"),
    CheckpointArray("od", _F, ("B", "T"), "eng", "od", "ego"),
    CheckpointArray("di_ai", _F, ("B", 2), "eng", "di_ai", "ego"),
    CheckpointArray("status", _I, ("B",), "eng", "status", "ego"),
    CheckpointArray("path_len", _I, ("B",), "eng", "path_len", "ego"),
    CheckpointArray("cv_cut", _I, ("B",), "eng", "cv_cut", "ego"),
    CheckpointArray("traj_idx", _L, ("B",), "pre", "traj_idx", "ego"),
    CheckpointArray("prev_len", _I, ("B",), "pre", "prev_len", "ego"),
    CheckpointArray("col_flag", _I, ("B",), "pre", "col_flag", "ego"),
    CheckpointArray("pre_status", _I, ("B",), "pre", "status", "ego"),
    CheckpointArray("obs_state", _F, ("n_obs", 4), "obst", "state", "vehicle"),
)
CHECKPOINT_MAX_ARRAYS = _c("JSIM_CKPT_MAX_ARRAYS")
CHECKPOINT_META = ("_names", "_every", "_cap", "_slot_tick", "_kind")   # what a checkpoint file holds beside the slabs


def checkpoint_slots(every: int, cap: int) -> int:
    """n_slots of a loop that records cap ticks and checkpoints every `every`: the ticks 0, every, .. <= cap."""
    return int(cap) // int(every) + 1


def checkpoint_cuts(t0: int, n: int, every: int, cap: int):
    """How run(n) of a loop that stands at tick t0 issues its entry point: a list of (slot, ticks) pieces, in
    order -- `slot` is saved ahead of the piece's ticks (-1: nothing is).  A piece ends at the next multiple of `every`; tick t is
    saved to slot t // every when t is such a multiple and t <= cap (ticks beyond cap save nothing, and are not cut).  The ticks of
    the pieces add up to n; n = 0 gives no piece."""
    t0, n, every, cap = int(t0), int(n), int(every), int(cap)
    if t0 < 0 or n < 0 or every < 1 or cap < 0:
        raise ValueError(f"checkpoint_cuts needs t0 >= 0, n >= 0, every >= 1, cap >= 0, got {t0}, {n}, {every}, {cap}")
    out, t, end = [], t0, t0 + n
    while t < end:
        nxt = (t // every + 1) * every                     # the next tick that could be saved
        stop = min(end, nxt) if nxt <= cap else end
        out.append((t // every if (t % every == 0 and t <= cap) else -1, stop - t))
        t = stop
    return out


def checkpoint_at(slot_tick, at):
    """The slot of every tick in `at` among the written slots of a loop (slot_tick [n_slots]: the tick each slot holds, -1: not
    written; of two slots with one tick the lower).  ValueError: a tick that is not checkpointed, naming the nearest checkpointed
    ticks on either side."""
    st = np.asarray(slot_tick).reshape(-1)
    have = np.unique(st[st >= 0])
    out = np.empty(np.size(at), dtype=np.int32)
    for r, k in enumerate(np.asarray(at).reshape(-1).tolist()):
        hit = np.flatnonzero(st == k)
        if k < 0 or hit.size == 0:
            below, above = have[have < k], have[have > k]
            near = " and ".join(str(int(v)) for v in ([below[-1]] if below.size else []) + ([above[0]] if above.size else []))
            raise ValueError(f"row {r}: tick {k} is not checkpointed (the nearest checkpointed ticks: {near or 'none'})")
        out[r] = hit[0]
    return out


def checkpoint_file(slabs: dict, every: int, cap: int, slot_tick, kind: str) -> dict:
    """What loop.save_checkpoints writes with numpy.savez: the slabs under their CHECKPOINT names and CHECKPOINT_META -- the names in
    CHECKPOINT's order, `every`, `cap`, the tick every slot holds (-1: not written) and the loop's class name."""
    names = [a.name for a in CHECKPOINT if a.name in slabs]
    if set(names) != set(slabs):
        raise ValueError(f"slabs that are not in history.CHECKPOINT: {sorted(set(slabs) - set(names))}")
    d = {k: np.ascontiguousarray(slabs[k]) for k in names}
    d.update(_names=np.array(names), _every=np.int64(every), _cap=np.int64(cap), _slot_tick=np.asarray(slot_tick, dtype=np.int64),
             _kind=np.array(kind))
    return d


def read_checkpoint_file(path):
    """(slabs, meta) of a file written by loop.save_checkpoints: the slabs as numpy arrays by name, in the file's order, and meta =
    dict(every, cap, slot_tick, kind).  ValueError: a file without the layout names, a name CHECKPOINT does not know, a slab of
    another dtype or with another number of slots than slot_tick."""
    known = {a.name: a for a in CHECKPOINT}
    with np.load(path, allow_pickle=False) as z:
        if any(k not in z.files for k in CHECKPOINT_META):
            raise ValueError(f"{path}: not a checkpoint file (it lacks {[k for k in CHECKPOINT_META if k not in z.files]})")
        names = [str(v) for v in z["_names"]]
        st = z["_slot_tick"].astype(np.int64)
        slabs = {}
        for k in names:
            if k not in known or k not in z.files:
                raise ValueError(f"{path}: array {k!r} is not in history.CHECKPOINT, or missing from the file")
            a = z[k]
            if a.dtype != np.dtype(known[k].dtype) or a.shape[0] != st.size or a.ndim != 1 + len(known[k].shape):
                raise ValueError(f"{path}: array {k!r} is {a.dtype} {a.shape}; expected {np.dtype(known[k].dtype)} [{st.size}]{known[k].shape}")
            slabs[k] = a
        meta = {"every": int(z["_every"]), "cap": int(z["_cap"]), "slot_tick": st, "kind": str(z["_kind"])}
    return slabs, meta


class History:
    """lib.simulation.History's fields and meaning: Python float lists x, y, yaw, v, t, delta, a, xref_deviation; t grows by
    repeated `+ sample_time` from 0 (the first entry is at t = sample_time), as History.store does it."""

    def __init__(self, sample_time: float):
        self.x: List[float] = []
        self.y: List[float] = []
        self.yaw: List[float] = []
        self.v: List[float] = []
        self.t: List[float] = []
        self.delta: List[float] = []
        self.a: List[float] = []
        self.xref_deviation: List[float] = []
        self._sample_time = sample_time

    def store(self, x: float, y: float, yaw: float, v: float, a: float, delta: float, xref_deviation: float):
        self.x.append(float(x))
        self.y.append(float(y))
        self.yaw.append(float(yaw))
        self.v.append(float(v))
        self.t.append(self.get_current_time() + self._sample_time)
        self.delta.append(float(delta))
        self.a.append(float(a))
        self.xref_deviation.append(float(xref_deviation))

    def get_current_time(self) -> float:
        return self.t[-1] if len(self.t) > 0 else 0.

    def __len__(self):
        return len(self.x)


def episode_bounds(flags_b: np.ndarray):
    """Episodes of one ego from its flags [n]: a list of (first tick, end tick (exclusive), END_*).  An episode ends with the
    record whose GOAL or AGE bit is set (the ego respawns after it); the last one is still running (END_RUNNING), and has no
    ticks yet when the last record ended the one before.  A tick with both bits counts as GOAL."""
    f = np.asarray(flags_b).reshape(-1)
    out, start = [], 0
    for k in np.flatnonzero(f & (GOAL | AGE)):
        out.append((start, int(k) + 1, END_GOAL if f[k] & GOAL else END_AGE))
        start = int(k) + 1
    out.append((start, f.size, END_RUNNING))      # the running one (just respawned: its spawn entry only)
    return out


def ego_histories(rec_b: np.ndarray, flags_b: np.ndarray, dt: float, x0_first, x0_spawn) -> List[History]:
    """One History per episode of one ego.  rec_b [n][7], flags_b [n]: the ego's recorded ticks; x0_first / x0_spawn: its state at
    the first recorded tick's start and its respawn state, both in the MPC's order (x, y, v, yaw).  Each History starts with the
    episode's spawn entry (a = delta = xref_deviation = 0, HistorySimulation.__init__), then one entry per tick."""
    rec_b = np.asarray(rec_b, dtype=np.float64).reshape(-1, 7)
    out = []
    for e, (k0, k1, _) in enumerate(episode_bounds(flags_b)):
        s = np.asarray(x0_first if e == 0 else x0_spawn, dtype=np.float64).reshape(4)
        h = History(dt)
        h.store(s[0], s[1], s[3], s[2], 0.0, 0.0, 0.0)
        for r in rec_b[k0:k1].tolist():
            h.store(r[0], r[1], r[2], r[3], r[5], r[4], r[6])
        out.append(h)
    return out


def episodes(flags: np.ndarray):
    """Per ego (flags [n][B]): dict count [B] (episodes), ticks (B arrays: ticks per episode), end (B arrays of END_*)."""
    f = np.asarray(flags).reshape(np.shape(flags)[0], -1)
    ticks, end = [], []
    for b in range(f.shape[1]):
        eb = episode_bounds(f[:, b])
        ticks.append(np.array([k1 - k0 for k0, k1, _ in eb], dtype=np.int64))
        end.append(np.array([x for _, _, x in eb], dtype=np.int8))
    return {"count": np.array([len(t) for t in ticks], dtype=np.int64), "ticks": ticks, "end": end}


def obstacle_positions(obs: Optional[np.ndarray], first_tick: int = 0):
    """The scripts' obstacles_positions from obs [n][n_obs][6]: per vehicle, the list of (i, get() tuple) of every tick i."""
    if obs is None:
        return []
    obs = np.asarray(obs, dtype=np.float64)
    return [[(first_tick + i, tuple(obs[i, o].tolist())) for i in range(obs.shape[0])] for o in range(obs.shape[1])]


def recorded_ticks(ticks_run: int, cap: int):
    """(ticks held by a recorder of capacity cap after ticks_run ticks, whether ticks were dropped)."""
    return min(int(ticks_run), int(cap)), int(ticks_run) > int(cap)


def _per_episode(flags: np.ndarray, make):
    """A list over egos (flags [n][B]) of lists over an ego's episodes (episode_bounds) of make(b, k0, k1)."""
    f = np.asarray(flags).reshape(np.shape(flags)[0], -1)
    return [[make(b, k0, k1) for k0, k1, _ in episode_bounds(f[:, b])] for b in range(f.shape[1])]


def _min_clear(clear: np.ndarray, who: np.ndarray, b: int, k0: int, k1: int):
    """(the smallest clearance of ego b over ticks [k0, k1), its first tick, `who` at that tick); (NaN, -1, -1) without one."""
    c = clear[k0:k1, b]
    if k1 <= k0 or np.isnan(c).all():
        return float("nan"), -1, -1
    k = int(np.nanargmin(c))
    return float(c[k]), k0 + k, int(who[k0 + k, b])


def reason_series(values: dict, flags: np.ndarray, dt: float):
    """The four lists the overtaking script keeps per run (main/scenarios/overtaking_cyclist_bidirectional_road.py:54-60,
    :2447-2451: time_values, reasons_policymaker_values, reasons_driver_values, reasons_cyclist_values), per ego and episode, from
    the per-tick values of a recorder (Recorder.reasons: `policymaker`, `driver`, `cyclist` [n][B]) and its flags [n][B], split
    where ego_histories splits (episode_bounds).  time_values is i * dt for tick i of the episode, as the script computes it.
    Returns a list over egos of lists over episodes of dicts of Python float lists."""
    series = {"reasons_" + k + "_values": np.asarray(values[k], dtype=np.float64) for k in ("policymaker", "driver", "cyclist")}

    def make(b, k0, k1):
        return {"time_values": [i * float(dt) for i in range(k1 - k0)], **{key: v[k0:k1, b].tolist() for key, v in series.items()}}
    return _per_episode(flags, make)


def conflict_episodes(result: dict, flags: np.ndarray):
    """The clearance and first contact of a recorder (Recorder.conflicts: `clear`, `who`, `hit_tick`, `hit_frame`, `hit_xy`) per
    ego and episode, split where ego_histories splits (episode_bounds).  Returns a list over egos of lists over episodes of dicts:
    contact (bool), tick (the first tick whose frame touches, -1: none), frame and xy (the reference's first_frame_idx and (x, y);
    -1 / None), collision_xy (what check_collision_moving_cars / check_collision_moving_bicycle return for the episode: None or
    (x, y, frame)), min_clear and min_clear_tick (the episode's smallest clearance and its first tick; NaN / -1 for an ego without
    vehicles or an episode without a tick yet), closest_vehicle (the place in the ego's list of the vehicle that came closest)."""
    clear, who = np.asarray(result["clear"], dtype=np.float64), np.asarray(result["who"])

    def make(b, k0, k1):
        ep = {"contact": False, "tick": -1, "frame": -1, "xy": None, "collision_xy": None}
        tick = int(result["hit_tick"][k0, b]) if k1 > k0 else -1
        if tick >= 0:
            x, y = (float(v) for v in result["hit_xy"][k0, b])
            frame = int(result["hit_frame"][k0, b])
            ep.update(contact=True, tick=tick, frame=frame, xy=(x, y), collision_xy=(x, y, frame))
        ep["min_clear"], ep["min_clear_tick"], ep["closest_vehicle"] = _min_clear(clear, who, b, k0, k1)
        return ep
    return _per_episode(flags, make)


def gap_per_tick(off: np.ndarray):
    """(gap, who) [n][B] int32 of Recorder.gaps' `off` [n][B][8]: the smallest |offset| over an ego's places on a tick and the lowest
    place that has it; -1 / -1 where no place has an offset (GAP_NONE)."""
    off = np.asarray(off).astype(np.int32)
    mag = np.where(off == GAP_NONE, GAP_MAX_WINDOW + 1, np.abs(off))
    who = np.argmin(mag, axis=2).astype(np.int32)                          # the lowest place on ties
    gap = np.take_along_axis(mag, who[:, :, None], axis=2)[:, :, 0]
    none = gap > GAP_MAX_WINDOW
    return np.where(none, -1, gap).astype(np.int32), np.where(none, -1, who).astype(np.int32)


def gap_episodes(result: dict, flags: np.ndarray, dt: float):
    """The time gaps of a recorder (Recorder.gaps: `off`, `ep_gap`, `ep_tick`, `ep_who`, `ep_off`) per ego and episode, split where
    ego_histories splits (episode_bounds).  Returns a list over egos of lists over episodes of dicts: gap (the episode's smallest
    |offset| in ticks, -1: nothing within the window), seconds (gap * dt, None without a gap), tick (the first tick that has it,
    -1), vehicle (the lowest place in the ego's list that has it on that tick, -1), first ("vehicle": it stood in the place before
    the ego did, "ego": the ego did, None: the same tick, or no gap) and per_vehicle: for each of the eight places (gap, offset,
    tick) -- its own smallest |offset| over the episode's ticks, that signed offset and the first tick that has it, (-1, None, -1)
    without one -- the table a gap-acceptance plot is drawn from."""
    off = np.asarray(result["off"]).astype(np.int32)
    mag = np.where(off == GAP_NONE, GAP_MAX_WINDOW + 1, np.abs(off))

    def make(b, k0, k1):
        ep = {"gap": -1, "seconds": None, "tick": -1, "vehicle": -1, "first": None, "per_vehicle": [(-1, None, -1)] * off.shape[2]}
        if k1 <= k0:
            return ep
        g = int(result["ep_gap"][k0, b])
        if g >= 0:
            o = int(result["ep_off"][k0, b])
            ep.update(gap=g, seconds=g * float(dt), tick=int(result["ep_tick"][k0, b]), vehicle=int(result["ep_who"][k0, b]),
                      first="vehicle" if o > 0 else "ego" if o < 0 else None)
        m = mag[k0:k1, b]                                                  # [ticks][places]
        k = np.argmin(m, axis=0)                                           # the first tick of each place's smallest
        ep["per_vehicle"] = [(int(m[k[i], i]), int(off[k0 + k[i], b, i]), k0 + int(k[i])) if m[k[i], i] <= GAP_MAX_WINDOW else (-1, None, -1)
                             for i in range(off.shape[2])]
        return ep
    return _per_episode(flags, make)


def path_table(paths) -> dict:
    """A list of paths -- (M, >= 3) arrays x, y, yaw, M >= 1 -- as jsim_loop_eval_tracking takes them: x, y, yaw (all points, path
    after path), off [n_paths + 1] (int64, as pack_paths makes it), arc (a list: the arc length at every point of each path, 0 at its
    first, arc[i + 1] = arc[i] + sqrt(dx * dx + dy * dy) added one after the other) and arc_flat (the same, path after path).
    ValueError: no path, a path that is not such an array, entries that are not finite."""
    paths = [np.asarray(p, dtype=np.float64) for p in paths]
    if not paths:
        raise ValueError("tracking needs at least one path")
    for i, p in enumerate(paths):
        if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 3:
            raise ValueError(f"path {i} must be an (M, >= 3) array x, y, yaw with M >= 1, got shape {p.shape}")
        if not np.isfinite(p[:, :3]).all():
            raise ValueError(f"path {i} has entries that are not finite")
    arc = []
    for p in paths:
        dx, dy = np.diff(p[:, 0]), np.diff(p[:, 1])
        arc.append(np.concatenate([[0.0], np.cumsum(np.sqrt(dx * dx + dy * dy))]))   # (cumsum adds in order)
    cat = np.concatenate([p[:, :3] for p in paths], axis=0)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return {"x": np.ascontiguousarray(cat[:, 0]), "y": np.ascontiguousarray(cat[:, 1]), "yaw": np.ascontiguousarray(cat[:, 2]),
            "off": off, "arc": arc, "arc_flat": np.ascontiguousarray(np.concatenate(arc))}


def tracking_episodes(result: dict, flags: np.ndarray, dt: float, stations=None, free_speed=None):
    """The path tracking of a recorder (Recorder.tracking: `s`, `ep_i`, `ep_d`) per ego and episode, split where ego_histories
    splits (episode_bounds).  Returns a list over egos of lists over episodes of dicts: k0, n (first tick, ticks), d_max (the largest
    |d|), d_max_tick (the first tick that has it, -1), d_rms (sqrt of the mean of d * d), yaw_max (the largest |e_yaw|), s_first,
    s_last (the arc length at the episode's first and last tick) and progress = s_last - s_first; NaN / -1 in an episode without a
    tick.  With stations (arc lengths): t_station, a list with, per station, the seconds from the episode's first tick to its first
    tick with s >= the station, NaN if it never is -- the travel time between two stations is the difference of two entries, the
    rows of a time-space diagram are (k * dt, s[k]).  With free_speed (m/s): delay = n * dt - progress / free_speed, the time lost
    against driving the same stretch at that speed.  The ticks at which |d| crosses a bound are threshold_crossings(-abs(d[:, b]),
    -bound) for leaving it and threshold_crossings(abs(d[:, b]), bound) for returning: that function applies as it is."""
    s = np.asarray(result["s"], dtype=np.float64)
    ep_i, ep_d = np.asarray(result["ep_i"]), np.asarray(result["ep_d"], dtype=np.float64)
    stations = None if stations is None else [float(v) for v in np.asarray(stations, dtype=np.float64).reshape(-1)]
    nan = float("nan")

    def make(b, k0, k1):
        n = k1 - k0
        ep = {"k0": k0, "n": n, "d_max": nan, "d_max_tick": -1, "d_rms": nan, "yaw_max": nan, "s_first": nan, "s_last": nan, "progress": nan}
        if n > 0:
            row = dict(zip(TRK_DOUBLE, ep_d[k0, b].tolist()))
            ep.update(d_max=row["d_max"], d_max_tick=int(ep_i[k0, b, 1]), d_rms=float(np.sqrt(row["d2_mean"])), yaw_max=row["yaw_max"],
                      s_first=row["s_first"], s_last=row["s_last"], progress=row["s_last"] - row["s_first"])
        if stations is not None:
            with np.errstate(invalid="ignore"):
                reached = [np.flatnonzero(s[k0:k1, b] >= v) for v in stations]
            ep["t_station"] = [float(r[0]) * float(dt) if r.size else nan for r in reached]
        if free_speed is not None:
            ep["delay"] = n * float(dt) - ep["progress"] / float(free_speed)
        return ep
    return _per_episode(flags, make)


def headway_episodes(result: dict, flags: np.ndarray, dt: float):
    """The headway of a recorder (Recorder.headway: `ep_i`, `ep_d`) per ego and episode, split where ego_histories splits
    (episode_bounds).  Returns a list over egos of lists over episodes of dicts: k0, n (first tick, ticks), lead_ticks (ticks with a
    leader on the path) and time_following = lead_ticks * dt (what evaluate_time_following of
    main/scenarios/overtaking_cyclist_bidirectional_road.py counts within a Euclidean range); gap_min (the smallest space headway to
    a leader, in metres), gap_tick, gap_t (the first tick that has it; seconds from the episode's first tick) and gap_who (the
    leader's place there); thw_min, thw_tick, thw_t and thw_mean (time headway, in seconds; the mean over the ticks where it is
    finite); ttc_min, ttc_tick, ttc_t and ttc_who (time to collision, in seconds; inf: never closing).  NaN / -1 without one and in
    an episode without a tick."""
    ep_i, ep_d = np.asarray(result["ep_i"]), np.asarray(result["ep_d"], dtype=np.float64)
    nan = float("nan")

    def make(b, k0, k1):
        n = k1 - k0
        ep = {"k0": k0, "n": n, "lead_ticks": 0, "time_following": 0.0, "gap_min": nan, "gap_tick": -1, "gap_t": nan, "gap_who": -1,
              "thw_min": nan, "thw_tick": -1, "thw_t": nan, "thw_mean": nan, "ttc_min": nan, "ttc_tick": -1, "ttc_t": nan, "ttc_who": -1}
        if n > 0:
            i = dict(zip(HW_INT, (int(v) for v in ep_i[k0, b])))
            d = dict(zip(HW_DOUBLE, ep_d[k0, b].tolist()))
            secs = lambda tick: (tick - k0) * float(dt) if tick >= 0 else nan
            ep.update(lead_ticks=i["lead_ticks"], time_following=i["lead_ticks"] * float(dt),
                      gap_min=d["gap_min"], gap_tick=i["gap_tick"], gap_t=secs(i["gap_tick"]), gap_who=i["gap_who"],
                      thw_min=d["thw_min"], thw_tick=i["thw_tick"], thw_t=secs(i["thw_tick"]), thw_mean=d["thw_mean"],
                      ttc_min=d["ttc_min"], ttc_tick=i["ttc_tick"], ttc_t=secs(i["ttc_tick"]), ttc_who=i["ttc_who"])
        return ep
    return _per_episode(flags, make)


def static_episodes(result: dict, flags: np.ndarray):
    """The static-obstacle clearance and contact of a recorder (Recorder.static_conflicts: `clear`, `who`, `hit`, `off_tick`) per
    ego and episode, split where ego_histories splits (episode_bounds).  Returns a list over egos of lists over episodes of dicts:
    contact (bool), tick (the first tick that touches an obstacle, -1: none), obstacle (the `hit` of that tick, -1), min_clear and
    min_clear_tick (the episode's smallest clearance and its first tick; NaN / -1 for an ego without obstacles or an episode without
    a tick yet), closest_obstacle (the place in its set of the obstacle that came closest), ticks_off (how many ticks touch)."""
    clear, who, hit = np.asarray(result["clear"], dtype=np.float64), np.asarray(result["who"]), np.asarray(result["hit"])

    def make(b, k0, k1):
        ep = {"contact": False, "tick": -1, "obstacle": -1}
        ticks_off = 0
        tick = int(result["off_tick"][k0, b]) if k1 > k0 else -1
        if tick >= 0:
            ep.update(contact=True, tick=tick, obstacle=int(hit[tick, b]))
            ticks_off = int((hit[k0:k1, b] >= 0).sum())
        ep["min_clear"], ep["min_clear_tick"], ep["closest_obstacle"] = _min_clear(clear, who, b, k0, k1)
        ep["ticks_off"] = ticks_off
        return ep
    return _per_episode(flags, make)


def cutoff_episodes(result: dict, flags: np.ndarray):
    """The collision cut-off of a recorder (Recorder.cutoffs: `status`, `idx`, `cut`, `hit`, `first`, `col_xy`) per ego and episode,
    split where ego_histories splits (episode_bounds).  Returns a list over egos of lists over episodes of dicts: the six series of
    the episode's ticks as numpy arrays under their names, first_cut_tick (the first tick of the run whose path was cut off, -1:
    none), n_cut (how many of the episode's ticks were cut off) and longest_cut (the longest run of consecutive cut-off ticks within
    the episode: a run that reaches the episode's last tick ends there, whatever the next episode starts with)."""
    series = {k: np.asarray(result[k]) for k in EVALUATORS["cutoffs"].keys()}

    def make(b, k0, k1):
        ep = {k: v[k0:k1, b] for k, v in series.items()}
        h = ep["hit"] != 0
        edges = np.flatnonzero(np.diff(np.concatenate([[0], h.astype(np.int8), [0]])))   # starts and ends of the runs, alternating
        runs = edges[1::2] - edges[0::2]
        ep.update(first_cut_tick=k0 + int(edges[0]) if runs.size else -1, n_cut=int(h.sum()), longest_cut=int(runs.max(initial=0)))
        return ep
    return _per_episode(flags, make)


def episode_rows(summary: dict):
    """The episode table of a recorder (Recorder.summary) as a list over egos of lists over episodes (in order of time) of dicts:
    every column of EP_INT and EP_DOUBLE under its name as a Python int / float, `duration` (n * dt) where the summary has it, and,
    where the summary evaluated that group, under `conflicts` the dict conflict_episodes gives for the episode and under `static`
    the one static_episodes gives (the two share key names, so each is a dict of its own)."""
    off = np.asarray(summary["ep_off"]).reshape(-1)
    cols = [(k, np.asarray(summary[k])) for k in EP_INT + EP_DOUBLE + (("duration",) if "duration" in summary else ())]
    out = []
    for b in range(off.size - 1):
        eps = []
        for e in range(int(off[b]), int(off[b + 1])):
            ep = {k: (int(a[e]) if a.dtype.kind in "iu" else float(a[e])) for k, a in cols}
            if summary.get("conflicts") is not None:
                hit = ep["veh_hit_tick"] >= 0
                xy = (ep["veh_hit_x"], ep["veh_hit_y"]) if hit else None
                ep["conflicts"] = {"contact": hit, "tick": ep["veh_hit_tick"] if hit else -1, "frame": ep["veh_hit_frame"] if hit else -1,
                                   "xy": xy, "collision_xy": (*xy, ep["veh_hit_frame"]) if hit else None, "min_clear": ep["veh_clear"],
                                   "min_clear_tick": ep["veh_tick"], "closest_vehicle": ep["veh_who"] if ep["veh_tick"] >= 0 else -1}
            if summary.get("static") is not None:
                hit = ep["st_off_tick"] >= 0
                ep["static"] = {"contact": hit, "tick": ep["st_off_tick"] if hit else -1, "obstacle": ep["st_obstacle"] if hit else -1,
                                "min_clear": ep["st_clear"], "min_clear_tick": ep["st_tick"],
                                "closest_obstacle": ep["st_who"] if ep["st_tick"] >= 0 else -1,
                                "ticks_off": ep["st_ticks_off"] if hit else 0}
            eps.append(ep)
        out.append(eps)
    return out


def fork_rows(B: int, n: int, ego, at):
    """The rows of a fork (Recorder.fork_state) as two int32 arrays [R]: ego and at, one integer each or
    sequences of one length (a single one is repeated).  ValueError: not integers, not one-dimensional, lengths that differ, an ego
    outside [0, B), a tick outside [0, n]."""
    e, a = np.asarray(ego), np.asarray(at)
    whole = lambda v: v.dtype.kind in "iu" or v.size == 0                            # noqa: E731  (an empty list has no type)
    if not whole(e) or not whole(a) or e.ndim > 1 or a.ndim > 1:
        raise ValueError(f"ego and at must be integers, one each or one-dimensional, got {e.dtype} {e.shape} and {a.dtype} {a.shape}")
    R = a.size if e.ndim == 0 else e.size if a.ndim == 0 else max(e.size, a.size)
    if (e.ndim and e.size != R) or (a.ndim and a.size != R):
        raise ValueError(f"ego holds {e.size} rows, at {a.size}")
    e, a = np.broadcast_to(e.reshape(-1), (R,)), np.broadcast_to(a.reshape(-1), (R,))
    if R and (e.min() < 0 or e.max() >= B):
        r = int(np.argmax((e < 0) | (e >= B)))
        raise ValueError(f"row {r}: ego {int(e[r])} outside [0, {B})")
    if R and (a.min() < 0 or a.max() > n):
        r = int(np.argmax((a < 0) | (a > n)))
        raise ValueError(f"row {r}: tick {int(a[r])} outside [0, {n}] (the recorded ticks)")
    return np.ascontiguousarray(e, dtype=np.int32), np.ascontiguousarray(a, dtype=np.int32)


def join(head: History, tail: History) -> History:
    """One History of a run that was forked (ScenarioLoop.fork): `head`, the source episode's History up to and
    including the entry for the start of the fork tick (its spawn entry and one entry per tick before the fork), then the forked
    loop's first History `tail` without its spawn entry, which is that same state again.  t goes on by repeated `+ sample_time`, as
    History.store counts it.  ValueError: an empty head or tail, two sample times."""
    if len(head) < 1 or len(tail) < 1:
        raise ValueError("join needs a head and a tail with at least their first entries")
    if head._sample_time != tail._sample_time:
        raise ValueError(f"the head's sample time is {head._sample_time}, the tail's {tail._sample_time}")
    out = History(head._sample_time)
    for h, first in ((head, 0), (tail, 1)):
        for i in range(first, len(h)):
            out.store(h.x[i], h.y[i], h.yaw[i], h.v[i], h.a[i], h.delta[i], h.xref_deviation[i])
    return out


def reasons_carry_at(result: dict, ego, at, ends=None) -> np.ndarray:
    """The carry [R][3] that tick at[r] of ego ego[r] meets in an evaluation of the per-tick reasons (Recorder.reasons, DESIGN.md
    section 16): the two timers as the tick before left them and the tracker = whether any value was below the threshold on the
    tick before; zeros on tick 0 (the evaluation's own default start) and behind a record that ended an episode; at = the number
    of evaluated ticks: the evaluation's own `carry`.  Handed to the forked loop's `recorder.reasons(carry=...)` it continues the
    three series across the fork.  result: Recorder.reasons' dict (`timers`, `below`, `carry`, `ends`); ends: [n][B] bool, the
    records that ended an episode, for a result without that key.  ValueError: bad rows (fork_rows), no `ends`."""
    timers, below = np.asarray(result["timers"], dtype=np.float64), np.asarray(result["below"])
    n, B = timers.shape[:2]
    e, a = fork_rows(B, n, ego, at)
    ends = result.get("ends") if ends is None else ends
    if ends is None:
        raise ValueError("the result holds no `ends` (the records that ended an episode): pass ends=")
    ends = np.asarray(ends).reshape(n, B) != 0
    out = np.zeros((e.size, 3))
    for r, (b, k) in enumerate(zip(e.tolist(), a.tolist())):
        if k == n:
            out[r] = np.asarray(result["carry"], dtype=np.float64)[b]
        elif k > 0 and not ends[k - 1, b]:
            out[r] = (timers[k - 1, b, 0], timers[k - 1, b, 1], 1.0 if below[k - 1, b].any() else 0.0)
    return out


def prediction_curve(result: dict, dt: float):
    """The mean displacement error by look-ahead of a recorder's predictions (Recorder.predictions: `step_sum`, `step_cnt` [V][n_steps]):
    (t [n_steps], mean [V][n_steps]) with t[j] = (j + 1) * dt, the time sample j lies ahead, and mean[r][j] = step_sum[r][j] /
    step_cnt[r][j], NaN where no tick of row r scored sample j."""
    s, c = np.asarray(result["step_sum"], dtype=np.float64), np.asarray(result["step_cnt"])
    if s.ndim != 2 or s.shape != c.shape:
        raise ValueError(f"step_sum and step_cnt must be [V][n_steps] alike, got {s.shape} and {c.shape}")
    t = (np.arange(s.shape[1]) + 1) * float(dt)
    return t, np.where(c > 0, s / np.where(c > 0, c, 1), np.nan)


def prediction_places(result: dict, veh_range, mate_range) -> dict:
    """The per-tick outputs of a recorder's predictions (Recorder.predictions: the columns PS_INT and PS_DOUBLE [n][V], `n_obs`,
    `egos`) gathered per ego into the eight places of its list in Recorder.conflicts' order -- its recorded vehicles
    [veh_range[b][0], veh_range[b][1]), then its group mates [mate_range[b][0], mate_range[b][1]) without itself -- as one array
    [n][B][8] per column.  A place without a vehicle, a mate when the egos were not scored and a place beyond the eighth are not
    there: -1 in the integer columns, NaN in the others.  `row` [B][8] is the row each place was taken from (-1: none)."""
    veh, mate = np.asarray(veh_range), np.asarray(mate_range)
    n_obs, egos = int(result["n_obs"]), bool(result["egos"])
    if veh.ndim != 2 or veh.shape[1] != 2 or mate.shape != veh.shape:
        raise ValueError(f"veh_range and mate_range must be [B][2] alike, got {veh.shape} and {mate.shape}")
    B = veh.shape[0]
    V = np.asarray(result[PS_INT[0]]).shape[1]
    row = np.full((B, MAX_OBS), -1, dtype=np.int64)
    for b in range(B):
        rows = list(range(int(veh[b, 0]), int(veh[b, 1])))
        if egos:
            rows += [n_obs + m for m in range(int(mate[b, 0]), int(mate[b, 1])) if m != b]
        rows = rows[:MAX_OBS]
        if rows and (min(rows) < 0 or max(rows) >= V):
            raise ValueError(f"ego {b}: a place outside the {V} scored rows")
        row[b, :len(rows)] = rows
    there = row >= 0
    out = {"row": row.astype(np.int32)}
    for k in PS_INT + PS_DOUBLE:
        a = np.asarray(result[k])
        g = a[:, np.where(there, row, 0)] if V else np.zeros((a.shape[0], B, MAX_OBS), dtype=a.dtype)   # [n][B][8]
        out[k] = np.where(there[None], g, -1 if k in PS_INT else np.nan).astype(a.dtype)
    return out


def threshold_crossings(series, value: float):
    """The ticks i >= 1 with series[i] <= value < series[i - 1]: where plot_distance of
    main/scenarios/overtaking_cyclist_bidirectional_road.py (:2390-2400) draws the line of a distance threshold.  For one ego's
    `clear` (Recorder.conflicts) or `distance` (Recorder.reasons) series; a NaN is on neither side.  Returns an int64 array."""
    s = np.asarray(series, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((s[1:] <= value) & (s[:-1] > value)) + 1
