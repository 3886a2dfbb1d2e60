"""The device History recorder of a closed loop and its evaluators: what the loops' kernels wrote per tick (jsim_loop_set_recorder),
read back as the reference's History objects or evaluated on the device, one launch per question (jsim_loop_eval_*).  Each
evaluator's per-tick outputs are stated once, in history.EVALUATORS: the Recorder allocates, passes and reads back from that table.
The predictions' scores (jsim_loop_score_predictions), whose rows are the recorded vehicles and then the egos, stand beside it in
history.PREDICTION_OUTPUTS, and so does the plan record of an InteractingLoop (jsim_loop_set_plan_recorder), history.PLAN_RECORD."""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _cabi, history
from .batched import BatchedMPC, _ptr
from .history import MAX_OBS
from .vehicle import vehicle_shape

_TORCH = {np.float64: torch.float64, np.int32: torch.int32, np.int8: torch.int8}   # the table's dtypes on the device


class Recorder:
    """The device History recorder of a loop (jsim_loop_set_recorder): every tick of every ego -- state after the plant step
    (before a respawn), applied (delta, a), xref deviation, flags -- and the scripted vehicles' get() tuples, written by the loop's
    kernels into [cap] tick slots (slot = the loop's device tick counter; ticks beyond cap are dropped).  The engine's context
    holds one recorder: the one of the loop constructed last on it; an earlier one is marked `superseded` and warns when read.
    `plans`: the plan record of InteractingLoop(record_plans=True) -- plan_oa, plan_od [cap][B][T] and plan_status [cap][B]
    (history.PLAN_RECORD): the engine's oa, od, status at the start of every tick -- or None.

    histories(b): lib.simulation.History objects, one per episode of ego b; obstacle_positions(): the scripts'
    obstacles_positions; episodes(): per-ego episode counts, lengths and ends.  These synchronise (device -> host copies)."""

    def __init__(self, loop: "ClosedLoop", cap: int, n_obs: int = 0, groups=None):
        eng = loop.eng
        if cap < 1:
            raise ValueError("record must be a positive number of ticks")
        self.loop, self.cap, self.n_obs = loop, int(cap), int(n_obs)
        dev = eng.device
        self.rec = torch.zeros(self.cap, eng.B, 7, dtype=torch.float64, device=dev)
        self.flags = torch.zeros(self.cap, eng.B, dtype=torch.int32, device=dev)
        # one row more than registered: the slot host ticks of ScenarioLoop write beyond cap (dropped)
        self._obs = torch.zeros(self.cap + 1, self.n_obs, 6, dtype=torch.float64, device=dev) if self.n_obs > 0 else None
        self.obs = self._obs[: self.cap] if self._obs is not None else None
        self.x0_first = loop.x0.clone()
        self.traffic = eng.traffic_layout  # (set_of, obs_off) of the loop's traffic sets, or None: whose vehicle is whose
        self.groups = None if groups is None else np.array(groups, dtype=np.int32)   # InteractingLoop's group offsets: whose mate is who
        self.superseded = False          # set when a later loop on the same engine registers its own recorder (or none)
        self.glue = None                 # a _GlueLoop's frame_window, margin, n_steps, mode and interacting (cutoffs()); None: no glue
        self._tracking_table = None      # the engine's paths as tracking() takes them, made at its first call
        self.plans = None                # the plan record of an InteractingLoop(record_plans=True): history.PLAN_RECORD's tensors
        _register_recorder(eng, self)

    def _record_plans(self):
        """The plan record (jsim_loop_set_plan_recorder) beside this recorder: every tick's eng.oa, eng.od and
        eng.status as they stand at the start of the tick, [cap] slots like rec."""
        eng = self.loop.eng
        self.plans = {k: torch.zeros(self.cap, eng.B, *(eng.T if s == "T" else s for s in shape), dtype=_TORCH[dt], device=eng.device)
                      for k, dt, shape in history.PLAN_RECORD}
        _cabi.check(eng.lib.jsim_loop_set_plan_recorder(eng._ctx, eng.B, self.cap, *map(_ptr, self.plans.values())), eng._ctx,
                    "jsim_loop_set_plan_recorder")

    def _record_obstacles(self, get: torch.Tensor):
        """Host ticks of ScenarioLoop: this tick's get() tuples (ahead of step()) to the slot of the tick just advanced."""
        k = (self.loop.tick_counter.to(torch.int64) - 1).clamp_(0, self.cap)
        self._obs.index_copy_(0, k, get.unsqueeze(0))

    @property
    def ticks_run(self) -> int:
        return int(self.loop.tick_counter.item())

    @property
    def overflow(self) -> bool:
        """True once more ticks ran than the recorder holds (the later ones were dropped)."""
        return history.recorded_ticks(self.ticks_run, self.cap)[1]

    def _n(self, stacklevel: int = 3) -> int:
        if self.superseded:
            warnings.warn("a later loop on this engine replaced this recorder: its records stopped at that point",
                          RuntimeWarning, stacklevel=stacklevel)
        n, over = history.recorded_ticks(self.ticks_run, self.cap)
        if over:
            warnings.warn(f"the recorder holds {self.cap} ticks, {self.ticks_run} ran: the last {self.ticks_run - self.cap} are not "
                          "recorded", RuntimeWarning, stacklevel=stacklevel)
        return n

    def _buffers(self):
        """rec, flags, x_first, x_spawn as the entry points that read the recorder take them."""
        return _ptr(self.rec), _ptr(self.flags), _ptr(self.x0_first), _ptr(self.loop.x0_spawn)

    def _outputs(self, name: str, n: int, skip=()) -> dict:
        """The outputs [n][B]... of evaluator `name` (history.EVALUATORS) as device tensors, in the entry point's order: its pointer
        arguments are map(_ptr, these).  A key in `skip` (an optional group the call does without) is None.  (No ticks yet: still
        valid pointers -- one row, and _rows gives none of it.)"""
        eng = self.loop.eng
        return {k: None if k in skip else torch.empty(max(n, 1), eng.B, *shape, dtype=_TORCH[dt], device=eng.device)
                for k, dt, shape in history.EVALUATORS[name].outputs}

    @staticmethod
    def _rows(out: dict, n: int, first: int = 0) -> dict:
        """The rows [first, n) of the outputs that were not skipped: what a call on _outputs(name, n) wrote."""
        return {k: t[first:n] for k, t in out.items() if t is not None}

    @staticmethod
    def _host(d: dict, keys) -> dict:
        """The read-back of what an _X_device method returned: the outputs `keys` as numpy arrays, the arguments used as they are."""
        return {k: v.cpu().numpy() if k in keys else v for k, v in d.items()}

    def _ego_shape(self):
        """(cc_front, cc_rear, radius) of the egos: the engine's registered shape, else the reference car's at its wheelbase."""
        eng = self.loop.eng
        return eng.ego_shape if eng.ego_shape is not None else vehicle_shape(L=eng.L)[:3]

    def _call(self, name: str, *args):
        """Entry point `name` on the engine's context and stream; a refusal raises with the library's message."""
        eng = self.loop.eng
        _cabi.check(getattr(eng.lib, name)(eng._ctx, *args, eng._stream()), eng._ctx, name)

    def histories(self, b: int):
        n = self._n()
        eng = self.loop.eng
        return history.ego_histories(self.rec[:n, b].cpu().numpy(), self.flags[:n, b].cpu().numpy(), eng.dt,
                                     self.x0_first[b].cpu().numpy(), self.loop.x0_spawn[b].cpu().numpy())

    def obstacle_positions(self):
        n = self._n()
        return history.obstacle_positions(self.obs[:n].cpu().numpy() if self.obs is not None else None)

    def episodes(self):
        return history.episodes(self.flags[: self._n()].cpu().numpy())

    def default_cyclist(self) -> np.ndarray:
        """Each ego's moving_obstacles[0] among the recorded vehicles ([B] int32): vehicle 0 of a shared list, the first vehicle of
        the ego's own set under a traffic layout, -1 for an ego whose set is empty."""
        B = self.loop.eng.B
        if self.traffic is None:
            return np.zeros(B, dtype=np.int32)
        set_of, obs_off = self.traffic
        return np.where(obs_off[set_of + 1] > obs_off[set_of], obs_off[set_of], -1).astype(np.int32)

    def reasons(self, par=None, threshold=0.7, cyclist=None, carry=None) -> dict:
        """The stakeholder reasons of every recorded tick and the replan trigger (jsim_loop_eval_reasons):
        what evaluate_reasons and reasons_evaluation of main/scenarios/overtaking_cyclist_bidirectional_road.py (:2007-2027,
        :1907-1940) give when called in the loop, computed in one launch from the records.

        par: one reasons.par_row or [B] rows (default: the reference's values with DT = the loop's sample time); threshold: one
        number or [B] (ReasonParameters.REASONS_THRESHOLD); cyclist: the recorded vehicle that is each ego's moving_obstacles[0],
        one index or [B], -1 = none (default: default_cyclist()); carry: [B][3] = time_elapsed_driver, time_passed_cyclist and the
        replan tracker (0 / 1) the first recorded tick starts from (default: zeros).
        Returns numpy arrays: policymaker, driver, cyclist, distance [n][B]; timers [n][B][2]; replan [n][B] bool; below [n][B][3]
        bool (policymaker, driver, cyclist under the threshold); first_replan [B] (-1: none); carry [B][3] as the next tick would
        meet it; ends [n][B] bool (the records that ended an episode: history.reasons_carry_at gives the carry any tick meets);
        and the par, threshold and veh_of used.  An ego without a cyclist has NaN in driver, cyclist and distance and
        never triggers on them.  ValueError: no vehicles recorded, a bad par / threshold / carry, a cyclist index out of range."""
        d = self._reasons_device(par, threshold, cyclist, carry)
        h = self._host(d, history.EVALUATORS["reasons"].keys() + ("first", "carry"))
        val, trig = h["val"], h["trig"]
        return {"policymaker": val[:, :, 0], "driver": val[:, :, 1], "cyclist": val[:, :, 2], "distance": val[:, :, 3],
                "timers": h["timers"], "replan": (trig & 1) != 0, "below": ((trig[:, :, None] >> np.arange(1, 4)) & 1) != 0,
                "first_replan": h["first"], "carry": h["carry"],
                "ends": (self.flags[: val.shape[0]].cpu().numpy() & (history.GOAL | history.AGE)) != 0, "par": np.array(d["par"]),
                "threshold": np.array(d["threshold"]), "veh_of": np.array(d["veh_of"], dtype=np.int32)}

    def _reasons_device(self, par=None, threshold=0.7, cyclist=None, carry=None, n=None) -> dict:
        """reasons() up to the launch: the outputs as device tensors (val [n][B][4], timers, trig, first, carry) and the host
        arguments used (par, threshold, veh_of).  n: the recorded ticks, where the caller has asked for them already."""
        from . import reasons as _reasons
        eng = self.loop.eng
        B = eng.B
        if self.obs is None:
            raise ValueError("this recorder holds no vehicle records (a loop without scripted vehicles): there is no cyclist to evaluate")
        par, thr, veh, car = _reasons.tick_inputs(B, self.n_obs, eng.dt, par, threshold, cyclist, carry, self.default_cyclist)
        n = self._n(4) if n is None else n
        dev = eng.device
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        d_par, d_thr, d_veh, d_car = up(par, np.float64), up(thr, np.float64), up(veh, np.int32), up(car, np.float64)
        out = self._outputs("reasons", n)
        first = torch.full((B,), -1, dtype=torch.int32, device=dev)
        rec, flags, x_first, x_spawn = self._buffers()
        self._call("jsim_loop_eval_reasons", B, n, rec, flags, self.n_obs, _ptr(self.obs), x_first, x_spawn, _ptr(d_veh), _ptr(d_par),
                   _ptr(d_thr), _ptr(d_car), *map(_ptr, out.values()), _ptr(first))
        return {**self._rows(out, n), "first": first, "carry": d_car, "par": par, "threshold": thr, "veh_of": veh}

    def vehicle_ranges(self) -> np.ndarray:
        """Each ego's vehicles [lo, hi) among the recorded ones ([B][2] int32): all of a shared list, its set's slice under a traffic
        layout (empty for an empty set or a recorder without vehicles)."""
        B = self.loop.eng.B
        if self.traffic is None:
            return np.tile(np.array([0, self.n_obs], dtype=np.int32), (B, 1))
        set_of, obs_off = self.traffic
        return np.stack([obs_off[set_of], obs_off[set_of + 1]], axis=1).astype(np.int32)

    def mate_ranges(self) -> np.ndarray:
        """Each ego's group as a batch range [mlo, mhi) ([B][2] int32): its group of an InteractingLoop, else empty."""
        B = self.loop.eng.B
        if self.groups is None:
            return np.zeros((B, 2), dtype=np.int32)
        g = np.repeat(np.arange(len(self.groups) - 1), np.diff(self.groups))
        return np.stack([self.groups[g], self.groups[g + 1]], axis=1).astype(np.int32)

    def _vehicle_lists(self, shapes=None, mates=None):
        """What conflicts() and gaps() meet: (ego_shape, shapes [n_obs][4] or None, veh_range, mate_range), checked."""
        eng = self.loop.eng
        B, n_obs = eng.B, self.n_obs
        ego = self._ego_shape()
        if shapes is None:
            shapes = eng.vehicle_shapes
        if shapes is not None:
            shapes = np.ascontiguousarray(shapes, dtype=np.float64)
            if shapes.shape != (n_obs, 4) or not (np.isfinite(shapes).all() and (shapes[:, 2] > 0).all()):
                raise ValueError(f"shapes must be [n_obs = {n_obs}, 4] vehicle_shape rows with finite offsets and positive radii")
        veh = self.vehicle_ranges()
        mate = self.mate_ranges() if mates is None else np.ascontiguousarray(mates, dtype=np.int32)
        if mate.shape != (B, 2):
            raise ValueError(f"mates must be [B = {B}, 2] batch ranges, got {mate.shape}")
        if (veh < 0).any() or (veh > n_obs).any() or (mate < 0).any() or (mate > B).any():
            raise ValueError("a vehicle range outside [0, n_obs] or a mate range outside [0, B]")
        me = np.arange(B)
        count = np.maximum(veh[:, 1] - veh[:, 0], 0) + np.maximum(mate[:, 1] - mate[:, 0], 0) - ((me >= mate[:, 0]) & (me < mate[:, 1]))
        if (count > MAX_OBS).any():
            b = int(np.argmax(count))
            raise ValueError(f"ego {b} would meet {int(count[b])} vehicles and mates (max {MAX_OBS})")
        return ego, shapes, veh, mate

    def _vehicle_args(self, shapes=None, mates=None):
        """_vehicle_lists as conflicts, gaps and headway hand it on: (the eight arguments that follow rec and flags -- n_obs, obs_rec,
        x_first, x_spawn, veh_range, mate_range, shapes, ego_shape --, the veh_range, mate_range and ego_shape entries of the result,
        the arrays those pointers point into: the caller holds them until its call has returned)."""
        dev = self.loop.eng.device
        ego, shapes, veh, mate = self._vehicle_lists(shapes, mates)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        d_veh, d_mate, ego_c = up(veh), up(mate), (C.c_double * 3)(*ego)
        _, _, x_first, x_spawn = self._buffers()
        args = (self.n_obs, _ptr(self.obs) if self.obs is not None else None, x_first, x_spawn, _ptr(d_veh), _ptr(d_mate),
                shapes.ctypes.data_as(C.c_void_p) if shapes is not None and self.n_obs else None, C.cast(ego_c, C.c_void_p))
        return args, {"veh_range": veh, "mate_range": mate, "ego_shape": tuple(float(v) for v in ego)}, (d_veh, d_mate, shapes, ego_c)

    def conflicts(self, frame_window: int = 0, shapes=None, mates=None) -> dict:
        """Clearance and first contact of every recorded tick and episode (jsim_loop_eval_conflicts): what
        check_collision_moving_cars / check_collision_moving_bicycle of main/lib/collision_avoidance.py (:85-166) return for an
        episode's driven poses against the vehicles' recorded ones, computed in one launch from the records.

        frame_window: the reference's frame_window, 0..20.  shapes: [n_obs][4] vehicle_shape rows (default: the loop's registered
        table, else every vehicle has the ego's shape).  mates: [B][2] batch ranges [mlo, mhi) of each ego's group mates, itself
        skipped (default: the groups of an InteractingLoop, else none).  An ego meets its recorded vehicles (vehicle_ranges()) and
        then its mates, eight in all.
        Returns numpy arrays: clear [n][B] (the smallest circle distance minus the threshold at offset 0; negative: overlap), who
        (that vehicle's place in the ego's list), row (the first touching row of the tick's frame over all offsets, -1: none),
        contact (row >= 0); and at the slot of an episode's first tick hit_tick (-1: no contact), hit_frame, hit_xy [n][B][2] (the
        reference's return value; -1 / NaN elsewhere); and the frame_window, veh_range, mate_range and ego_shape used.  An ego
        without vehicles and mates has NaN / -1 everywhere.  history.conflict_episodes splits the result into episodes.
        ValueError: a frame_window outside 0..20, a bad shapes table, a range outside its table, more than eight vehicles."""
        out = self._host(self._conflicts_device(frame_window, shapes, mates), history.EVALUATORS["conflicts"].keys())
        out["contact"] = out["row"] >= 0
        return out

    def _conflicts_device(self, frame_window: int = 0, shapes=None, mates=None, n=None) -> dict:
        """conflicts() up to the launch: the outputs as device tensors (clear, who, row, hit_tick, hit_frame, hit_xy) and the host
        arguments used (frame_window, veh_range, mate_range, ego_shape)."""
        eng = self.loop.eng
        w = int(frame_window)
        if w != frame_window or not 0 <= w <= 20:
            raise ValueError(f"frame_window must be an integer in 0..20, got {frame_window!r}")
        veh_args, used, keep = self._vehicle_args(shapes, mates)
        n = self._n(4) if n is None else n
        out = self._outputs("conflicts", n)
        self._call("jsim_loop_eval_conflicts", eng.B, n, _ptr(self.rec), _ptr(self.flags), *veh_args, w, *map(_ptr, out.values()))
        return {**self._rows(out, n), "frame_window": w, **used}

    def gaps(self, window: int = 20, within: str = "episode", shapes=None, mates=None) -> dict:
        """The time gap between every ego and each vehicle it meets, per recorded tick and episode (jsim_loop_eval_gaps, DESIGN.md
        section 23): how many ticks lay between the ego occupying a place and a vehicle occupying it, and who went first -- the
        post-encroachment time of a crossing, the time headway to a leader.  An episode's smallest gap is the least frame_window at
        which check_collision_moving_cars / check_collision_moving_bicycle (main/lib/collision_avoidance.py:68-166) report a hit
        on it.  One launch from the records.

        window: the largest offset tried, 0..63.  within: "episode" (only vehicle ticks inside the ego's own episode count: the
        reference's rule) or "record" (every recorded tick counts, so the vehicle that passed a spawn point just before the ego
        respawned there is found).  shapes, mates: as for conflicts(); the list is the same, eight places in all.
        Returns numpy arrays: off [n][B][8] int8 (per place the touching offset of smallest |off|; > 0: the vehicle was here first,
        < 0: the ego was; -o in front of +o; history.GAP_NONE = -128: nothing within the window, or no such place), gap [n][B] (the
        smallest |off| over the places, -1: none), who (the lowest place that has it); at the slot of an episode's first tick
        ep_gap (the episode's smallest gap, -1: none), ep_tick (the first tick that has it), ep_who (the lowest place that has it
        there), ep_off (its signed offset, -128: none), -1 / -1 / -1 / -128 elsewhere; and the window, within, veh_range, mate_range
        and ego_shape used.  history.gap_episodes splits the result into episodes.
        ValueError: a window outside 0..63, another within, and what conflicts() refuses of shapes and mates."""
        out = self._host(self._gaps_device(window, within, shapes, mates), history.EVALUATORS["gaps"].keys())
        out["gap"], out["who"] = history.gap_per_tick(out["off"])
        return out

    def _gaps_device(self, window: int = 20, within: str = "episode", shapes=None, mates=None, n=None) -> dict:
        """gaps() up to the launch: the outputs as device tensors (off, ep_gap, ep_tick, ep_who, ep_off) and the host arguments used
        (window, within, veh_range, mate_range, ego_shape)."""
        eng = self.loop.eng
        w = int(window)
        if w != window or not 0 <= w <= history.GAP_MAX_WINDOW:
            raise ValueError(f"window must be an integer in 0..{history.GAP_MAX_WINDOW}, got {window!r}")
        if within not in ("episode", "record"):
            raise ValueError(f'within must be "episode" or "record", got {within!r}')
        veh_args, used, keep = self._vehicle_args(shapes, mates)
        n = self._n(4) if n is None else n
        out = self._outputs("gaps", n)
        self._call("jsim_loop_eval_gaps", eng.B, n, _ptr(self.rec), _ptr(self.flags), *veh_args, w, int(within == "record"),
                   *map(_ptr, out.values()))
        return {**self._rows(out, n), "window": w, "within": within, **used}

    def static_conflicts(self, obstacles, set_of=None, margin=None, include_hidden: bool = False) -> dict:
        """Clearance to and contact with the scenario's static obstacles on every recorded tick (jsim_loop_eval_static, DESIGN.md
        section 18): check_collision on Obstacle.to_convex(margin) (main/lib/obstacles.py:157-176, the planner's collision test) and
        distance_to_point at the two collision circle centres of the poses that were driven, computed in one launch from the records.

        obstacles: one set -- a scenario's obstacles list: the reference's BoxObstacle / CircleObstacle objects or the primitives of
        planner.intersection_obstacles -- or a list of such sets (an empty list: one empty set).  set_of: the set of every ego, one
        index or [B] (default 0).  margin: what to_convex inflates by (default: the ego radius, as the scenario scripts pass it to the
        planner).  include_hidden: also test the hidden obstacles (the planner's lane-closing boxes).
        Returns numpy arrays [n][B]: clear (the smallest distance_to_point(centre) - radius over the included obstacles and the two
        centres; -radius: a centre inside an obstacle), who (that obstacle's place in its set), hit (the lowest place of a touched
        obstacle, -1: none), contact (hit >= 0), off_tick (at the slot of an episode's first tick the episode's first touching tick
        or -1; -1 elsewhere); and the margin, include_hidden, ego_shape and set_of used.  An ego whose set has no included obstacle
        has NaN / -1 / -1.  history.static_episodes splits the result into episodes.
        ValueError: an obstacle that is neither kind, a set_of outside the sets, a margin that is not finite and >= 0."""
        out = self._host(self._static_device(obstacles, set_of, margin, include_hidden), history.EVALUATORS["static"].keys())
        out["contact"] = out["hit"] >= 0
        return out

    def _static_device(self, obstacles, set_of=None, margin=None, include_hidden: bool = False, n=None) -> dict:
        """static_conflicts() up to the launch: the outputs as device tensors (clear, who, hit, off_tick) and the host arguments
        used (margin, include_hidden, ego_shape, set_of)."""
        from . import planner
        eng = self.loop.eng
        B = eng.B
        ego = self._ego_shape()
        margin = float(ego[2] if margin is None else margin)
        obstacles = list(obstacles)
        is_one = lambda o: (isinstance(o, (tuple, list)) and len(o) > 0 and isinstance(o[0], str)) or hasattr(o, "to_convex")
        sets = [obstacles] if (not obstacles or is_one(obstacles[0])) else [list(s) for s in obstacles]
        tables = [planner.static_obstacle_rows(s, margin) for s in sets]
        rows = np.ascontiguousarray(np.concatenate(tables))
        n_rows = len(rows)
        if n_rows == 0:
            rows = np.zeros((1, planner.STATIC_ROW))                 # (a valid pointer; no row of it is read)
        set_off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int32)
        sof = np.zeros(B, dtype=np.int64) if set_of is None else np.asarray(set_of)
        if sof.dtype.kind not in "iu" or sof.shape not in ((), (B,)):
            raise ValueError(f"set_of must be one integer or [B = {B}] integers, got {sof.dtype} {sof.shape}")
        sof = np.ascontiguousarray(np.broadcast_to(sof, (B,)), dtype=np.int32)
        if ((sof < 0) | (sof >= len(sets))).any():
            raise ValueError(f"set_of outside [0, {len(sets)})")
        n = self._n(4) if n is None else n
        d_set = torch.from_numpy(sof).to(eng.device)
        out = self._outputs("static", n)
        ego_c = (C.c_double * 3)(*ego)
        self._call("jsim_loop_eval_static", B, n, *self._buffers(), _ptr(d_set), len(sets), set_off.ctypes.data_as(C.c_void_p), n_rows,
                   rows.ctypes.data_as(C.c_void_p), C.cast(ego_c, C.c_void_p), int(bool(include_hidden)), *map(_ptr, out.values()))
        return {**self._rows(out, n), "margin": margin, "include_hidden": bool(include_hidden),
                "ego_shape": tuple(float(v) for v in ego), "set_of": sof}

    def _path_args(self, paths=None, path_id=None):
        """What tracking() and headway() meet of paths and path_id, checked: (the path table on the device -- x, y, yaw, off, arc --,
        n_paths, path_id [B] on the host, the same on the device, arc as a list)."""
        eng = self.loop.eng
        B, dev = eng.B, eng.device
        table = self._tracking_table if paths is None else None
        if table is None:
            table = history.path_table(eng.paths if paths is None else paths)
            table["dev"] = [torch.from_numpy(table[k]).to(dev) for k in ("x", "y", "yaw", "off", "arc_flat")]
            if paths is None:
                self._tracking_table = table
        n_paths = len(table["arc"])
        own = paths is None and path_id is None                     # the engine's own: its path_id is on the device already
        if path_id is None:
            if paths is not None and n_paths != 1:
                raise ValueError("paths of one's own need a path_id per ego")
            pid = eng.path_id.cpu().numpy() if own else np.zeros(B, dtype=np.int32)
        else:
            pid = np.asarray(path_id)
            if pid.dtype.kind not in "iu" or pid.shape not in ((), (B,)):
                raise ValueError(f"path_id must be one integer or [B = {B}] integers, got {pid.dtype} {pid.shape}")
            pid = np.array(np.broadcast_to(pid, (B,)), dtype=np.int32)
        if ((pid < 0) | (pid >= n_paths)).any():
            raise ValueError(f"path_id outside [0, {n_paths})")
        d_pid = eng.path_id if own else torch.from_numpy(pid).to(dev)
        return table["dev"], n_paths, pid, d_pid, table["arc"]

    def tracking(self, paths=None, path_id=None) -> dict:
        """Every recorded pose projected onto a path (jsim_loop_eval_tracking): how far along its route each
        ego was on every tick, how far beside it and how far off its heading -- what plot_trajectories_comparison of
        main/scenarios/mpc_sensitivity_analysis*.py draws against the reference trajectory -- computed in one launch from the records.
        The pose of tick k is the record itself (History.x[k], .y[k], .yaw[k]: after the plant step).

        paths: a list of (M, >= 3) arrays x, y, yaw (M >= 1; the yaw as the controller sees it: unwrapped, as engine.paths hold it),
        default: the engine's paths (their device copy is made once and kept on the recorder); path_id: each ego's path, one index or
        [B], default: the engine's path_id (with paths given: required unless there is one path).  Any paths will do: the original
        route of a fork, a lane centreline.  The context's own tables are not read, so a superseded recorder gives the same result.
        Returns numpy arrays [n][B]: idx (calc_nearest_index(state, cx, cy, 0) of main/lib/trajectories.py:89-97, relative to the
        path), seg (the segment that holds the foot), s (arc length of the foot), d (signed lateral offset, left of the direction of
        travel positive; |d| is the distance to the polyline), e_yaw (heading error wrapped to [-pi, pi)); -1 / NaN for a pose that
        is not finite; at the slot of an episode's first tick ep_i [n][B][2] (history.TRK_INT: ticks, d_max_tick) and ep_d [n][B][5]
        (history.TRK_DOUBLE: d_max, d2_mean, yaw_max, s_first, s_last), -1 / NaN elsewhere; arc (a list: the arc length at every
        point of every path) and the path_id used.  history.tracking_episodes splits the result into episodes and gives travel
        times between stations and the delay against free flow.
        ValueError: a path_id out of range or of another shape, a path without a point or with fewer than three columns,
        path entries that are not finite."""
        return self._host(self._tracking_device(paths, path_id), history.EVALUATORS["tracking"].keys())

    def _tracking_device(self, paths=None, path_id=None, n=None) -> dict:
        """tracking() up to the launch: the outputs as device tensors (idx, seg, s, d, e_yaw, ep_i, ep_d) and the host arguments
        used (arc, path_id)."""
        B = self.loop.eng.B
        (px, py, pyaw, off, d_arc), n_paths, pid, d_pid, arc = self._path_args(paths, path_id)
        n = self._n(4) if n is None else n
        out = self._outputs("tracking", n)
        self._call("jsim_loop_eval_tracking", B, n, _ptr(self.rec), _ptr(self.flags), _ptr(d_pid), int(px.numel()), _ptr(px), _ptr(py),
                   _ptr(pyaw), n_paths, _ptr(off), _ptr(d_arc), *map(_ptr, out.values()))
        return {**self._rows(out, n), "arc": arc, "path_id": pid}

    def headway(self, paths=None, path_id=None, shapes=None, mates=None, margin: float = 0.0, places: bool = True) -> dict:
        """Every recorded vehicle projected onto the ego's path (jsim_loop_eval_headway): how much road lay
        between the ego and each vehicle it meets, how fast it closed and how long until it is gone -- the distance along the road
        that create_following_trajectory, evaluate_time_following and plot_distance of
        main/scenarios/overtaking_cyclist_bidirectional_road.py approximate with a Euclidean range -- computed in one launch from
        the records, everything taken at the start of each tick.

        paths, path_id: as for tracking() (default: the engine's own, whose device copy is kept on the recorder).  shapes, mates:
        as for conflicts(); the list is the same, eight places in all.  margin (>= 0): added to a vehicle's threshold (the ego's
        radius + its own) when deciding whether it is on the path.  places=False: the three per-place arrays are neither written
        nor read back.
        Returns numpy arrays.  Per place [n][B][8] (places=True): gap (> 0: the vehicle is ahead by that much road, < 0: behind,
        0: alongside), lat (its nearer circle centre's signed offset from the path, left positive), rate (its speed along the path
        minus the ego's; an oncoming vehicle's own is negative); NaN for an empty place or a pose that is not finite.  Per tick
        [n][B]: lead (the on-path place with the smallest gap >= 0, -1: none), lead_gap, thw (lead_gap / u_ego; inf for a standing
        ego, 0 alongside), ttc (the smallest time to collision over the on-path places; inf: none is closing; NaN: none is on the
        path), ttc_who, u_ego (the ego's speed along the path).  At the slot of an episode's first tick ep_i [n][B][7]
        (history.HW_INT) and ep_d [n][B][4] (history.HW_DOUBLE), -1 / NaN elsewhere.  And arc, path_id, veh_range, mate_range,
        ego_shape and margin as used.  An ego without vehicles and mates has -1 / NaN everywhere.  history.headway_episodes splits
        the result into episodes.
        ValueError: what tracking() refuses of paths and path_id, what conflicts() refuses of shapes and mates, a margin that is
        not finite and >= 0."""
        return self._host(self._headway_device(paths, path_id, shapes, mates, margin, places), history.EVALUATORS["headway"].keys())

    def _headway_device(self, paths=None, path_id=None, shapes=None, mates=None, margin: float = 0.0, places: bool = True, n=None) -> dict:
        """headway() up to the launch: the outputs as device tensors (lead, lead_gap, thw, ttc, ttc_who, u_ego, ep_i, ep_d and, with
        places, gap, lat, rate) and the host arguments used (arc, path_id, veh_range, mate_range, ego_shape, margin)."""
        B = self.loop.eng.B
        margin = float(margin)
        if not (math.isfinite(margin) and margin >= 0.0):
            raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
        (px, py, pyaw, off, d_arc), n_paths, pid, d_pid, arc = self._path_args(paths, path_id)
        veh_args, used, keep = self._vehicle_args(shapes, mates)
        n = self._n(4) if n is None else n
        out = self._outputs("headway", n, skip=() if places else history.EVALUATORS["headway"].optional)
        self._call("jsim_loop_eval_headway", B, n, _ptr(self.rec), _ptr(self.flags), *veh_args,
                   _ptr(d_pid), int(px.numel()), _ptr(px), _ptr(py), _ptr(pyaw), n_paths, _ptr(off), _ptr(d_arc), margin,
                   *map(_ptr, out.values()))
        return {**self._rows(out, n), "arc": arc, "path_id": pid, **used, "margin": margin}

    def cutoffs(self, chunk_ticks: int = 0, carry=None) -> dict:
        """The glue's decision on every recorded tick (jsim_loop_eval_cutoffs): what the loop ahead of MPC.step
        found and did -- main/scenarios/mpc_intersection.py:104-143: the progress index, check_collision_moving_cars /
        check_collision_moving_bicycle on the predicted traffic, get_cutoff_curve_by_position_idx(...) - EXTRA_CUTOFF_MARGIN -- and
        what visualize_frame shows of it (collision_xy, the length of tmp_trajectory), computed again after the run from the records
        by the loops' own device function: every value is the live loop's, bit for bit.

        chunk_ticks: ticks per launch (0: from a 512 MiB budget of predictions).  carry: [B][3] int32 = the progress index, the
        previous path length (-1: none) and the cut-off the first recorded tick starts from (default: the loops' own start).
        Returns numpy arrays over the recorded ticks [n][B]: status (the glue's pre_status: 0, or the tick kept idx and cut as they
        were), idx (the progress index after the tick's update), cut (what the loop wrote to path_len, under mode="speed_cutoff" to
        the speed cut-off), hit (bool), first (the hit's index on the remaining path, -1: none), col_xy [n][B][2] (NaN: none); and
        carry [B][3] as the next tick would meet it.  history.cutoff_episodes splits the result into episodes.
        A recording of an InteractingLoop with mate_prediction="plan" is replayed from its plan record (record_plans=True;
        jsim_loop_eval_cutoffs_plan): the mates are predicted again from the plans they were predicted from.
        ValueError: a recorder of a ClosedLoop (it has no glue), a plan-mode recording without its plans (the replay would predict
        the group mates from their recorded steering, and the plans the live loop predicted them from -- every ego's oa, od of
        the tick -- are not recorded), a superseded recorder (the context's tables are no longer its loop's), a bad chunk_ticks or
        carry."""
        out = self._host(self._cutoffs_device(chunk_ticks, carry), history.EVALUATORS["cutoffs"].keys() + ("carry",))
        out["hit"] = out["hit"] != 0
        return out

    def _cutoffs_device(self, chunk_ticks: int = 0, carry=None, n=None, first_tick: int = 0) -> dict:
        """cutoffs() up to the launches: the outputs as device tensors (status, idx, cut, hit, first, col_xy, carry).  n: the recorded
        ticks, where the caller has asked for them already, or fewer; first_tick: evaluate the ticks [first_tick, n) only, from the
        carry the ticks before left (the outputs are those ticks' rows)."""
        eng = self.loop.eng
        B, dev = eng.B, eng.device
        if self.glue is None:
            raise ValueError("this recorder's loop has no glue (ClosedLoop): there is no cut-off to evaluate")
        plans = getattr(self, "plans", None)
        plan = self.glue.get("mate_prediction", "constant") != "constant"
        if plan and plans is None:
            raise ValueError("this recording is of an InteractingLoop with mate_prediction='plan': the replay predicts the group "
                             "mates from their recorded steering, and the plans they were predicted from are not recorded")
        if self.superseded:
            raise ValueError("a later loop on this engine replaced this recorder: the context's tables are no longer its loop's")
        c = int(chunk_ticks)
        if c != chunk_ticks or c < 0:
            raise ValueError(f"chunk_ticks must be an integer >= 0, got {chunk_ticks!r}")
        if carry is None:
            d_car = None
        else:
            car = np.asarray(carry)
            if car.shape != (B, 3) or car.dtype.kind not in "iu":
                raise ValueError(f"carry must be [B = {B}, 3] integers, got {car.dtype} {car.shape}")
            d_car = torch.from_numpy(np.ascontiguousarray(car, dtype=np.int32)).to(dev)
        n = self._n(4) if n is None else n
        k0 = int(first_tick)
        if not 0 <= k0 <= n:
            raise ValueError(f"first_tick must be in [0, {n}], got {first_tick!r}")
        g = self.glue
        if d_car is None:      # the loops' own start: what a NULL carry of the entry point stands for, as a tensor to hand back
            full = eng.full_len
            d_car = torch.stack([torch.zeros_like(full), torch.full_like(full, -1), full], dim=1).contiguous()
        out = self._outputs("cutoffs", n)
        rec, flags, x_first, x_spawn = self._buffers()
        # a plan-mode recording: the same call with the plan record behind it, the mates predicted from their recorded plans
        self._call("jsim_loop_eval_cutoffs_plan" if plan else "jsim_loop_eval_cutoffs", B, n, rec, flags, self.n_obs,
                   _ptr(self.obs) if self.obs is not None else None, x_first, x_spawn, g["frame_window"], g["margin"], g["n_steps"],
                   int(g["mode"] == "speed_cutoff"), int(g["interacting"]), c, k0, _ptr(d_car), *map(_ptr, out.values()),
                   *(map(_ptr, plans.values()) if plan else ()))
        return {**self._rows(out, n, k0), "carry": d_car}

    def predictions(self, n_steps=None, tol=None, egos=None, steps: bool = False) -> dict:
        """Every recorded prediction against what the vehicle then did (jsim_loop_score_predictions): the loops
        predict every vehicle with MovingObstaclesPrediction(x, y, v, yaw, a, steer) (main/lib/moving_obstacles_prediction.py:21-47) --
        a constant arc for n_steps * dt seconds -- and every cut-off rests on it.  The recorded get() tuples are the exact inputs of
        those predictions, the next ticks' tuples and the egos' records what then happened: one launch makes each prediction again in
        registers and measures its displacement error.

        n_steps: samples per prediction, 1..64 (default: the glue's, else 35).  tol: the displacement a prediction may be off while it
        still `holds` (default: the ego radius).  egos: None scores the egos of an InteractingLoop as its mates predicted them --
        the constant rule under mate_prediction="constant", the plan rule under "plan" where the plans are recorded
        (record_plans=True), no egos where they are not; True asks for it (ValueError on a plan-mode recording without its plans);
        "constant" scores the constant rule on any recording -- the baseline the plan rule is meant to beat; "plan" scores the plan
        rule on any recording that holds plans (jsim_loop_score_plan_predictions, DESIGN.md section 29: the egos' rows come from
        that call, the vehicles' from the other, joined on the device; ValueError without plans); False leaves the egos out (1 / 0
        and numpy's booleans stand for True / False; anything else raises).  steps=True also returns every sample's error.
        Rows: V = n_obs + (B with the egos): the recorded vehicles in the recorder's order, then the egos.  Returns numpy arrays
        [n][V]: n (the scored samples: those whose truth is recorded, for an ego within its episode), hold (the leading samples
        within tol), max_at (the first sample of the largest error, -1: none), ade, fde, max, lon, lat (the last scored sample's
        error along and across the true heading; lon > 0: predicted farther ahead than the vehicle got), yaw (its heading error,
        wrapped to [-pi, pi)); NaN where n = 0; step_sum, step_cnt [V][n_steps] (history.prediction_curve gives the mean error by
        look-ahead); err [n][V][n_steps] with steps=True (NaN: not scored); and n_steps, tol, egos (bool), rule ("constant" /
        "plan" / None: how the egos' rows were predicted), n_obs and dt as used.
        history.prediction_places gathers an ego's eight places.
        ValueError: an n_steps outside 1..64, a tol that is not finite and >= 0, another egos, egos=True on a plan-mode recording
        without plans, egos="plan" on a recorder that holds none, a superseded recorder (the context's wheelbases are no longer its loop's)."""
        d = self._predictions_device(n_steps, tol, egos, steps)
        h = self._host(d, history.PREDICTION_OUTPUTS.keys())
        pt_i, pt_d = h.pop("pt_i"), h.pop("pt_d")
        h.update({k: np.ascontiguousarray(pt_i[:, :, j]) for j, k in enumerate(history.PS_INT)})
        h.update({k: np.ascontiguousarray(pt_d[:, :, j]) for j, k in enumerate(history.PS_DOUBLE)})
        return h

    def _predictions_device(self, n_steps=None, tol=None, egos=None, steps: bool = False, n=None) -> dict:
        """predictions() up to the launch: the outputs as device tensors (pt_i [n][V][3], pt_d [n][V][6], step_sum, step_cnt
        [V][n_steps] and, with steps, err [n][V][n_steps]) and the host arguments used (n_steps, tol, egos, rule, n_obs, dt)."""
        eng = self.loop.eng
        B, dev = eng.B, eng.device
        glue = self.glue or {}
        S = glue.get("n_steps", 35) if n_steps is None else n_steps
        if isinstance(S, (bool, np.bool_)) or not (isinstance(S, (int, float, np.integer, np.floating)) and math.isfinite(S) and int(S) == S
                                                   and 1 <= int(S) <= history.MAX_PRED):
            raise ValueError(f"n_steps must be an integer in 1..{history.MAX_PRED}, got {n_steps!r}")
        S = int(S)
        tol = float(self._ego_shape()[2] if tol is None else tol)
        if not (math.isfinite(tol) and tol >= 0.0):
            raise ValueError(f"tol must be finite and >= 0, got {tol!r}")
        plan = glue.get("mate_prediction", "constant") != "constant"
        plans = getattr(self, "plans", None)
        if isinstance(egos, (np.bool_, int, np.integer)) and egos in (0, 1):     # True / False and what the entry point takes for them
            egos = bool(egos)
        if egos is None:                      # what the mates really predicted, where the recording can tell
            rule = None if not glue.get("interacting") or (plan and plans is None) else "plan" if plan else "constant"
        elif egos is True:
            if plan and plans is None:
                raise ValueError("this recording is of an InteractingLoop with mate_prediction='plan': its egos were predicted from "
                                 "their plans, which are not recorded (egos='constant' scores the constant rule instead)")
            rule = "plan" if plan else "constant"
        elif egos is False:
            rule = None
        elif isinstance(egos, str) and egos == "constant":
            rule = "constant"
        elif isinstance(egos, str) and egos == "plan" and plans is not None:
            rule = "plan"
        elif isinstance(egos, str) and egos == "plan":
            raise ValueError("egos='plan' needs the plan record of InteractingLoop(record=..., record_plans=True): this recorder "
                             "holds no plans")
        else:
            raise ValueError(f"egos must be None, True / False (or 1 / 0), 'constant' or 'plan', got {egos!r}")
        if self.superseded:
            raise ValueError("a later loop on this engine replaced this recorder: the context's tables are no longer its loop's")
        n = self._n(4) if n is None else n
        rec, flags, x_first, x_spawn = self._buffers()

        def outputs(V):
            """PREDICTION_OUTPUTS' tensors for V rows and what a call takes of them."""
            shape = {"tick": (max(n, 1), max(V, 1)), "row": (max(V, 1),)}
            out = {k: None if (k == "err" and not steps) else
                   torch.empty(*shape[lead], *(S if s == "n_steps" else s for s in trail), dtype=_TORCH[dt], device=dev)
                   for k, dt, lead, trail in history.PREDICTION_OUTPUTS.outputs}
            if n == 0 or V == 0:              # (the call writes nothing: no tick has scored a sample)
                out["step_sum"].zero_(); out["step_cnt"].zero_()
            return out, [_ptr(t) if t is not None else None for t in out.values()]

        def rows(out, V):
            cut = {"tick": lambda t: t[:n, :V], "row": lambda t: t[:V]}
            return {k: cut[lead](out[k]) for k, _, lead, _ in history.PREDICTION_OUTPUTS.outputs if out[k] is not None}

        # the vehicles' rows, and with them the egos' under the constant rule: the one call
        V0 = self.n_obs + (B if rule == "constant" else 0)
        out, ptrs = outputs(V0)
        self._call("jsim_loop_score_predictions", B, n, rec, flags, self.n_obs, _ptr(self.obs) if self.obs is not None else None,
                   x_first, x_spawn, int(rule == "constant"), S, tol, *ptrs)
        res = rows(out, V0)
        if rule == "plan":                    # the egos' rows under the plan rule, joined behind the vehicles' on the device
            ego, ptrs = outputs(B)
            self._call("jsim_loop_score_plan_predictions", B, n, rec, flags, x_first, x_spawn, *map(_ptr, plans.values()), S, tol, *ptrs)
            ego = rows(ego, B)
            axis = {k: 1 if lead == "tick" else 0 for k, _, lead, _ in history.PREDICTION_OUTPUTS.outputs}
            res = {k: torch.cat([res[k], ego[k]], dim=axis[k]) for k in res}
        return {**res, "n_steps": S, "tol": tol, "egos": rule is not None, "rule": rule, "n_obs": self.n_obs, "dt": float(eng.dt)}

    def fork_state(self, ego, at):
        """Where a loop forked off this recording starts (jsim_loop_fork_state): for every row r the state
        (x, y, v, yaw) of ego ego[r] at the start of recorded tick at[r] -- at = the number of recorded ticks: after the last one --
        by the rule the cut-off replay reads its states by, and the first tick of the episode that tick belongs to.

        ego, at: one integer each or [R]; one ego may stand in several rows.  Returns x0 (a device tensor [R, 4]), k0 and
        age = at - k0 (int32 numpy arrays [R]).  ValueError: rows that are not integers of one length, an ego outside the batch, a
        tick outside 0 .. recorded ticks, a superseded recorder (its records stopped when the later loop was built)."""
        eng = self.loop.eng
        if self.superseded:
            raise ValueError("a later loop on this engine replaced this recorder: its records stopped at that point")
        n = self._n()
        ego, at = history.fork_rows(eng.B, n, ego, at)
        R = ego.size
        x0 = torch.empty(max(R, 1), 4, dtype=torch.float64, device=eng.device)[:R]
        k0 = torch.empty(max(R, 1), dtype=torch.int32, device=eng.device)[:R]
        self._call("jsim_loop_fork_state", eng.B, n, *self._buffers(), R, ego.ctypes.data_as(C.c_void_p), at.ctypes.data_as(C.c_void_p),
                   _ptr(x0), _ptr(k0))
        k0 = k0.cpu().numpy()
        return x0, k0, at - k0

    def summary(self, conflicts=None, static=None, reasons=None) -> dict:
        """One row per recorded episode of every ego (jsim_loop_summarise_episodes): did the ego arrive, how
        many ticks it took, how far it drove and deviated, how close it came to a vehicle and to an obstacle, whether it touched
        either, whether the replan trigger fired -- reduced on the device; the per-tick series are not read back.

        conflicts / static / reasons: None (the group's columns stay NaN / -1 / 0), True (conflicts() / static_conflicts() /
        reasons() with their defaults; `static` has no default for its obstacles) or a dict of that method's keyword arguments.
        Returns numpy arrays: ep_off [B + 1] (ego b's rows are [ep_off[b], ep_off[b + 1]), in order of time) and one array [E] per
        column of history.EP_INT and history.EP_DOUBLE (ego, k0, n, end, failed, dev_tick, veh_tick, veh_who, veh_hit_tick,
        veh_hit_frame, st_tick, st_who, st_off_tick, st_obstacle, st_ticks_off, replan_tick; length, v_mean, v_max, a_min, a_max,
        delta_absmax, dev_max, dev_mean, veh_clear, veh_hit_x, veh_hit_y, st_clear, pm_min, driver_min, cyclist_min, dist_min);
        duration [E] = n * dt; dt; and under `conflicts`, `static`, `reasons` the arguments that evaluation used (None: not
        requested).  history.episode_rows turns the result into per-ego lists of dicts.
        ValueError: what the three methods raise, a `static` without obstacles, an argument that is none of None / True / dict."""
        eng = self.loop.eng
        B, dev = eng.B, eng.device

        def kwargs(name, arg):
            if arg is None or arg is True:
                return {}
            if not isinstance(arg, dict):
                raise ValueError(f"{name} must be None, True or a dict of keyword arguments, got {arg!r}")
            return dict(arg)

        kw_c, kw_s, kw_r = kwargs("conflicts", conflicts), kwargs("static", static), kwargs("reasons", reasons)
        if static is not None and "obstacles" not in kw_s:
            raise ValueError("static needs its obstacles: static=dict(obstacles=...)")
        n = self._n()
        c = self._conflicts_device(n=n, **kw_c) if conflicts is not None else None
        s = self._static_device(n=n, **kw_s) if static is not None else None
        r = self._reasons_device(n=n, **kw_r) if reasons is not None else None
        # the table's size, exactly: every ego's running episode and one more per end flag
        ends = int(((self.flags[:n] & (history.GOAL | history.AGE)) != 0).sum().item()) if n else 0
        cap = B + ends
        ep_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        ep_i = torch.empty(max(cap, 1), len(history.EP_INT), dtype=torch.int32, device=dev)
        ep_d = torch.empty(max(cap, 1), len(history.EP_DOUBLE), dtype=torch.float64, device=dev)
        # each group is its evaluator's outputs but those the table of episodes does not take: conflicts' row, reasons' timers
        group = lambda d, name, skip=(): [_ptr(d[k]) if d is not None else None for k in history.EVALUATORS[name].keys(skip)]
        self._call("jsim_loop_summarise_episodes", B, n, *self._buffers(), *group(c, "conflicts", ("row",)), *group(s, "static"),
                   *group(r, "reasons", ("timers",)), cap, _ptr(ep_off), _ptr(ep_i), _ptr(ep_d))
        off, I, D = ep_off.cpu().numpy(), ep_i[:cap].cpu().numpy(), ep_d[:cap].cpu().numpy()
        if int(off[B]) != cap:
            raise RuntimeError(f"the episode table has {int(off[B])} rows, {cap} were counted")
        out = {"ep_off": off, "dt": float(eng.dt)}
        out.update({k: np.ascontiguousarray(I[:, j]) for j, k in enumerate(history.EP_INT)})
        out.update({k: np.ascontiguousarray(D[:, j]) for j, k in enumerate(history.EP_DOUBLE)})
        out["duration"] = out["n"] * float(eng.dt)
        meta = lambda d, keys: None if d is None else {k: d[k] for k in keys}
        out["conflicts"] = meta(c, ("frame_window", "veh_range", "mate_range", "ego_shape"))
        out["static"] = meta(s, ("margin", "include_hidden", "ego_shape", "set_of"))
        out["reasons"] = None if r is None else {"par": np.array(r["par"]), "threshold": np.array(r["threshold"]),
                                                 "veh_of": np.array(r["veh_of"], dtype=np.int32)}
        return out


def _register_recorder(engine: BatchedMPC, rec: Optional[Recorder]):
    """jsim_loop_set_recorder (None: clear).  The engine keeps the registered buffers alive; the recorder it replaces is marked
    superseded."""
    old = engine._recorder
    if old is not None and old is not rec:
        old.superseded = True
    if rec is None:
        _cabi.check(engine.lib.jsim_loop_set_recorder(engine._ctx, engine.B, 0, None, None, 0, None), engine._ctx,
                    "jsim_loop_set_recorder")
    else:
        _cabi.check(engine.lib.jsim_loop_set_recorder(engine._ctx, engine.B, rec.cap, _ptr(rec.rec), _ptr(rec.flags), rec.n_obs,
                                                      _ptr(rec.obs) if rec.obs is not None else None), engine._ctx,
                    "jsim_loop_set_recorder")
    engine._recorder = rec
