"""Closed-loop driver for a batch of egos: the reference's per-vehicle loop
(main/scenarios/mpc_intersection.py:99-163) with the B-ego `for` replaced by one MPC launch + one
bookkeeping launch per tick, nothing leaving the device between ticks."""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _cabi, history
from .batched import BatchedMPC, _ptr


class Recorder:
    """The device History recorder of a loop (jsim_loop_set_recorder): every tick of every ego -- state after the plant step
    (before a respawn), applied (delta, a), xref deviation, flags -- and the scripted vehicles' get() tuples, written by the loop's
    kernels into [cap] tick slots (slot = the loop's device tick counter; ticks beyond cap are dropped).  The engine's context
    holds one recorder: the one of the loop constructed last on it; an earlier one is marked `superseded` and warns when read.

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
        _register_recorder(eng, self)

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

    def _new(self, n: int, *shape, dtype=torch.float64, count: Optional[int] = None):
        """An output [n][B]...: `count` of them as a tuple, or one.  (No ticks yet: still valid pointers.)"""
        eng = self.loop.eng
        out = tuple(torch.empty(max(n, 1), eng.B, *shape, dtype=dtype, device=eng.device)[:n] for _ in range(count or 1))
        return out if count else out[0]

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
        val, trig = d["val"].cpu().numpy(), d["trig"].cpu().numpy()
        return {"policymaker": val[:, :, 0], "driver": val[:, :, 1], "cyclist": val[:, :, 2], "distance": val[:, :, 3],
                "timers": d["timers"].cpu().numpy(), "replan": (trig & 1) != 0, "below": ((trig[:, :, None] >> np.arange(1, 4)) & 1) != 0,
                "first_replan": d["first"].cpu().numpy(), "carry": d["carry"].cpu().numpy(),
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
        val, tim, trig = self._new(n, 4), self._new(n, 2), self._new(n, dtype=torch.int32)
        first = torch.full((B,), -1, dtype=torch.int32, device=dev)
        rec, flags, x_first, x_spawn = self._buffers()
        self._call("jsim_loop_eval_reasons", B, n, rec, flags, self.n_obs, _ptr(self.obs), x_first, x_spawn, _ptr(d_veh), _ptr(d_par),
                   _ptr(d_thr), _ptr(d_car), _ptr(val), _ptr(tim), _ptr(trig), _ptr(first))
        return {"val": val, "timers": tim, "trig": trig, "first": first, "carry": d_car, "par": par, "threshold": thr, "veh_of": veh}

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
        d = self._conflicts_device(frame_window, shapes, mates)
        row = d["row"].cpu().numpy()
        return {"clear": d["clear"].cpu().numpy(), "who": d["who"].cpu().numpy(), "row": row, "contact": row >= 0,
                "hit_tick": d["hit_tick"].cpu().numpy(), "hit_frame": d["hit_frame"].cpu().numpy(), "hit_xy": d["hit_xy"].cpu().numpy(),
                "frame_window": d["frame_window"], "veh_range": d["veh_range"], "mate_range": d["mate_range"], "ego_shape": d["ego_shape"]}

    def _conflicts_device(self, frame_window: int = 0, shapes=None, mates=None, n=None) -> dict:
        """conflicts() up to the launch: the outputs as device tensors (clear, who, row, hit_tick, hit_frame, hit_xy) and the host
        arguments used (frame_window, veh_range, mate_range, ego_shape)."""
        eng = self.loop.eng
        w = int(frame_window)
        if w != frame_window or not 0 <= w <= 20:
            raise ValueError(f"frame_window must be an integer in 0..20, got {frame_window!r}")
        veh_args, used, keep = self._vehicle_args(shapes, mates)
        n = self._n(4) if n is None else n
        clear, hit_xy = self._new(n), self._new(n, 2)
        who, row, hit_tick, hit_frame = self._new(n, dtype=torch.int32, count=4)
        self._call("jsim_loop_eval_conflicts", eng.B, n, _ptr(self.rec), _ptr(self.flags), *veh_args, w,
                   _ptr(clear), _ptr(who), _ptr(row), _ptr(hit_tick), _ptr(hit_frame), _ptr(hit_xy))
        return {"clear": clear, "who": who, "row": row, "hit_tick": hit_tick, "hit_frame": hit_frame, "hit_xy": hit_xy,
                "frame_window": w, **used}

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
        d = self._gaps_device(window, within, shapes, mates)
        off = d["off"].cpu().numpy()
        gap, who = history.gap_per_tick(off)
        return {"off": off, "gap": gap, "who": who,
                "ep_gap": d["ep_gap"].cpu().numpy(), "ep_tick": d["ep_tick"].cpu().numpy(), "ep_who": d["ep_who"].cpu().numpy(),
                "ep_off": d["ep_off"].cpu().numpy(), "window": d["window"], "within": d["within"], "veh_range": d["veh_range"],
                "mate_range": d["mate_range"], "ego_shape": d["ego_shape"]}

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
        off = self._new(n, 8, dtype=torch.int8)
        ep_gap, ep_tick, ep_who, ep_off = self._new(n, dtype=torch.int32, count=4)
        self._call("jsim_loop_eval_gaps", eng.B, n, _ptr(self.rec), _ptr(self.flags), *veh_args, w, int(within == "record"),
                   _ptr(off), _ptr(ep_gap), _ptr(ep_tick), _ptr(ep_who), _ptr(ep_off))
        return {"off": off, "ep_gap": ep_gap, "ep_tick": ep_tick, "ep_who": ep_who, "ep_off": ep_off, "window": w, "within": within,
                **used}

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
        d = self._static_device(obstacles, set_of, margin, include_hidden)
        hit = d["hit"].cpu().numpy()
        return {"clear": d["clear"].cpu().numpy(), "who": d["who"].cpu().numpy(), "hit": hit, "contact": hit >= 0,
                "off_tick": d["off_tick"].cpu().numpy(), "margin": d["margin"], "include_hidden": d["include_hidden"],
                "ego_shape": d["ego_shape"], "set_of": d["set_of"]}

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
        clear = self._new(n)
        who, hit, off_tick = self._new(n, dtype=torch.int32, count=3)
        ego_c = (C.c_double * 3)(*ego)
        self._call("jsim_loop_eval_static", B, n, *self._buffers(), _ptr(d_set), len(sets), set_off.ctypes.data_as(C.c_void_p), n_rows,
                   rows.ctypes.data_as(C.c_void_p), C.cast(ego_c, C.c_void_p), int(bool(include_hidden)),
                   _ptr(clear), _ptr(who), _ptr(hit), _ptr(off_tick))
        return {"clear": clear, "who": who, "hit": hit, "off_tick": off_tick, "margin": margin, "include_hidden": bool(include_hidden),
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
        d = self._tracking_device(paths, path_id)
        out = {k: d[k].cpu().numpy() for k in ("idx", "seg", "s", "d", "e_yaw", "ep_i", "ep_d")}
        out.update(arc=d["arc"], path_id=d["path_id"])
        return out

    def _tracking_device(self, paths=None, path_id=None, n=None) -> dict:
        """tracking() up to the launch: the outputs as device tensors (idx, seg, s, d, e_yaw, ep_i, ep_d) and the host arguments
        used (arc, path_id)."""
        B = self.loop.eng.B
        (px, py, pyaw, off, d_arc), n_paths, pid, d_pid, arc = self._path_args(paths, path_id)
        n = self._n(4) if n is None else n
        idx, seg = self._new(n, dtype=torch.int32, count=2)
        s, d, e_yaw = self._new(n, count=3)
        ep_i, ep_d = self._new(n, len(history.TRK_INT), dtype=torch.int32), self._new(n, len(history.TRK_DOUBLE))
        self._call("jsim_loop_eval_tracking", B, n, _ptr(self.rec), _ptr(self.flags), _ptr(d_pid), int(px.numel()), _ptr(px), _ptr(py),
                   _ptr(pyaw), n_paths, _ptr(off), _ptr(d_arc), _ptr(idx), _ptr(seg), _ptr(s), _ptr(d), _ptr(e_yaw), _ptr(ep_i), _ptr(ep_d))
        return {"idx": idx, "seg": seg, "s": s, "d": d, "e_yaw": e_yaw, "ep_i": ep_i, "ep_d": ep_d, "arc": arc, "path_id": pid}

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
        d = self._headway_device(paths, path_id, shapes, mates, margin, places)
        keys = ("lead", "lead_gap", "thw", "ttc", "ttc_who", "u_ego", "ep_i", "ep_d") + (("gap", "lat", "rate") if places else ())
        out = {k: d[k].cpu().numpy() for k in keys}
        out.update({k: d[k] for k in ("arc", "path_id", "veh_range", "mate_range", "ego_shape", "margin")})
        return out

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
        lead, ttc_who = self._new(n, dtype=torch.int32, count=2)
        lead_gap, thw, ttc, u_ego = self._new(n, count=4)
        ep_i, ep_d = self._new(n, len(history.HW_INT), dtype=torch.int32), self._new(n, len(history.HW_DOUBLE))
        per_place = self._new(n, MAX_OBS, count=3) if places else (None, None, None)
        self._call("jsim_loop_eval_headway", B, n, _ptr(self.rec), _ptr(self.flags), *veh_args,
                   _ptr(d_pid), int(px.numel()), _ptr(px), _ptr(py), _ptr(pyaw), n_paths, _ptr(off), _ptr(d_arc), margin,
                   _ptr(lead), _ptr(lead_gap), _ptr(thw), _ptr(ttc), _ptr(ttc_who), _ptr(u_ego), _ptr(ep_i), _ptr(ep_d),
                   *[_ptr(t) if t is not None else None for t in per_place])
        out = {"lead": lead, "lead_gap": lead_gap, "thw": thw, "ttc": ttc, "ttc_who": ttc_who, "u_ego": u_ego, "ep_i": ep_i, "ep_d": ep_d,
               "arc": arc, "path_id": pid, **used, "margin": margin}
        if places:
            out.update(gap=per_place[0], lat=per_place[1], rate=per_place[2])
        return out

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
        ValueError: a recorder of a ClosedLoop (it has no glue), a superseded recorder (the context's tables are no longer its
        loop's), a bad chunk_ticks or carry."""
        d = self._cutoffs_device(chunk_ticks, carry)
        out = {k: d[k].cpu().numpy() for k in ("status", "idx", "cut", "first", "col_xy", "carry")}
        out["hit"] = d["hit"].cpu().numpy() != 0
        return out

    def _cutoffs_device(self, chunk_ticks: int = 0, carry=None, n=None, first_tick: int = 0) -> dict:
        """cutoffs() up to the launches: the outputs as device tensors (status, idx, cut, hit, first, col_xy, carry).  n: the recorded
        ticks, where the caller has asked for them already, or fewer; first_tick: evaluate the ticks [first_tick, n) only, from the
        carry the ticks before left (the outputs are those ticks' rows)."""
        eng = self.loop.eng
        B, dev = eng.B, eng.device
        if self.glue is None:
            raise ValueError("this recorder's loop has no glue (ClosedLoop): there is no cut-off to evaluate")
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
        rows = max(n, 1)       # (no ticks yet: still valid pointers)
        status, idx, cut, hit, first = (torch.empty(rows, B, dtype=torch.int32, device=dev) for _ in range(5))
        col_xy = torch.empty(rows, B, 2, dtype=torch.float64, device=dev)
        rec, flags, x_first, x_spawn = self._buffers()
        self._call("jsim_loop_eval_cutoffs", B, n, rec, flags, self.n_obs, _ptr(self.obs) if self.obs is not None else None,
                   x_first, x_spawn, g["frame_window"], g["margin"], g["n_steps"], int(g["mode"] == "speed_cutoff"),
                   int(g["interacting"]), c, k0, _ptr(d_car), _ptr(status), _ptr(idx), _ptr(cut), _ptr(hit), _ptr(first), _ptr(col_xy))
        status, idx, cut, hit, first, col_xy = (t[k0:n] for t in (status, idx, cut, hit, first, col_xy))
        return {"status": status, "idx": idx, "cut": cut, "hit": hit, "first": first, "col_xy": col_xy, "carry": d_car}

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
        group = lambda d, keys: [_ptr(d[k]) if d is not None else None for k in keys]
        self._call("jsim_loop_summarise_episodes", B, n, *self._buffers(),
                   *group(c, ("clear", "who", "hit_tick", "hit_frame", "hit_xy")), *group(s, ("clear", "who", "hit", "off_tick")),
                   *group(r, ("val", "trig")), cap, _ptr(ep_off), _ptr(ep_i), _ptr(ep_d))
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


class ClosedLoop:
    """tick(): jsim_mpc_step then jsim_loop_advance (plant, history, respawn of finished egos).

    hist_cap: ticks of (di, ai) history kept on the device ([hist_cap, B, 2]); max_age: safety respawn
    after that many ticks (<= 0: only MPC.is_goal ends an ego's run); record: ticks of the full History kept on the device
    (`recorder`, a Recorder; 0: none)."""

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, hist_cap: int = 0, max_age: int = 0, record: int = 0):
        eng = self.eng = engine
        eng._check_x0(x0)
        self.x0 = x0
        dev = eng.device
        self.x0_spawn = x0.clone()
        self.target_spawn = eng.target_ind.clone()
        self.age = torch.zeros(eng.B, dtype=torch.int32, device=dev)
        self.max_age = int(max_age)
        self.hist_cap = int(hist_cap)
        self.hist = torch.zeros(max(hist_cap, 1), eng.B, 2, dtype=torch.float64, device=dev) if hist_cap > 0 else None
        self.tick_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_respawn = torch.zeros(1, dtype=torch.int64, device=dev)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._graph_ticks = 0
        self.recorder: Optional[Recorder] = None
        if eng._recorder is not None:
            _register_recorder(eng, None)            # an earlier loop's recorder on this engine stops recording
        if record:
            self.recorder = Recorder(self, record)

    def _advance_args(self):
        """What tick() passes to jsim_loop_advance after (ctx, B)."""
        eng = self.eng
        return (_ptr(self.x0), _ptr(eng.oa), _ptr(eng.od), _ptr(eng.status), _ptr(eng.di_ai), _ptr(eng.target_ind),
                _ptr(eng.path_id), _ptr(eng.path_len), _ptr(self.x0_spawn), _ptr(self.target_spawn), _ptr(self.age), self.max_age,
                _ptr(self.hist), _ptr(self.tick_counter), self.hist_cap, _ptr(self.n_respawn), eng._stream())

    def tick(self):
        eng = self.eng
        eng.solve(self.x0)
        _cabi.check(eng.lib.jsim_loop_advance(eng._ctx, eng.B, *self._advance_args()), eng._ctx, "jsim_loop_advance")

    def _loop_args(self):
        """Checks x0; returns the step and advance buffers the multi-tick entry points take after (ctx, B, n_ticks)."""
        eng = self.eng
        eng._check_x0(self.x0)
        return (_ptr(self.x0), _ptr(eng.path_id), _ptr(eng.path_len), _ptr(eng.speed), _ptr(eng.target_ind), _ptr(eng.oa),
                _ptr(eng.od), _ptr(eng.ox), _ptr(eng.oy), _ptr(eng.ov), _ptr(eng.oyaw), _ptr(eng.xref), _ptr(eng.active_mask),
                _ptr(eng.status), _ptr(eng.n_iter), _ptr(eng.di_ai), _ptr(self.x0_spawn), _ptr(self.target_spawn),
                _ptr(self.age), self.max_age, _ptr(self.hist), _ptr(self.tick_counter), self.hist_cap, _ptr(self.n_respawn))

    def run(self, n_ticks: int):
        """n_ticks ticks in one call (jsim_mpc_run_ticks): for T = 13 / 20 a single launch in which each wavefront
        advances its own ego n_ticks times -- same results as n_ticks x tick(), without per-tick synchronisation."""
        eng = self.eng
        _cabi.check(eng.lib.jsim_mpc_run_ticks(eng._ctx, eng.B, int(n_ticks), *self._loop_args(), eng._stream()), eng._ctx,
                    "jsim_mpc_run_ticks")

    # ---- hipGraph: a launch-bound inner loop (two short kernels per tick) replayed without host work
    def capture(self, ticks: int):
        """Capture `ticks` consecutive ticks into one hipGraph (all pointers are fixed device buffers and the
        history slot comes from the device tick counter, so replays continue the same simulation)."""
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=self.eng.device)
        s.wait_stream(torch.cuda.current_stream(self.eng.device))
        with torch.cuda.stream(s):
            self.tick()                      # warm-up outside capture (lazy module load)
        torch.cuda.current_stream(self.eng.device).wait_stream(s)
        torch.cuda.synchronize(self.eng.device)
        with torch.cuda.graph(g, stream=s):
            for _ in range(ticks):
                self.tick()
        self._graph, self._graph_ticks = g, ticks
        return g

    def replay(self):
        self._graph.replay()
        return self._graph_ticks


def car_circles(L: float = 2.86, width: float = 2.0, extra_length: float = 0.64):
    """Collision circles of the reference's BicycleModelDimensions (main/lib/car_dimensions.py:62-79,82-90): bounding
    box (width, L + 0.64), radius = width / sqrt(2), two centres on the body axis at L/2 +- (length/2 - width/2) from the
    rear axle.  Returns (radius, (front_offset, rear_offset))."""
    length = L + extra_length
    offset = length / 2 - width / 2
    return width / (2 ** .5), (L / 2 + offset, L / 2 - offset)


DIMS_KEYS = ("L", "width", "extra_length")


def vehicle_shape(dims=None, L: float = 2.86, width: float = 2.0, extra_length: float = 0.64):
    """One row of the shape table of jsim_loop_set_vehicle_shapes, (cc_front, cc_rear, radius, wheelbase), from the fields of
    `obstacle_dims`: dims = dict(L=..., width=..., extra_length=...) (any missing key: the keyword's value) through car_circles.
    Raises ValueError on an unknown key or a size that is not positive (extra_length: negative)."""
    if dims is not None:
        unknown = sorted(set(dims) - set(DIMS_KEYS))
        if unknown:
            raise ValueError(f"unknown dims key(s) {unknown}: a vehicle's dims holds {list(DIMS_KEYS)}")
        L, width, extra_length = (float(dims.get(k, d)) for k, d in zip(DIMS_KEYS, (L, width, extra_length)))
    if not (L > 0 and width > 0 and extra_length >= 0 and math.isfinite(L + width + extra_length)):
        raise ValueError(f"a vehicle's L and width must be positive and its extra_length not negative (L={L}, width={width}, "
                         f"extra_length={extra_length})")
    radius, (c0, c1) = car_circles(L, width, extra_length)
    return (c0, c1, radius, L)


def shape_table(specs, default_shape):
    """The [n, 4] float64 shape table of a flat list of vehicle specs, or None when no spec carries `dims` (nothing to
    register).  A vehicle without dims has default_shape (a vehicle_shape row)."""
    specs = list(specs)
    rows = [vehicle_shape(s["dims"]) if s.get("dims") is not None else None for s in specs]
    if all(r is None for r in rows):
        return None
    return np.array([default_shape if r is None else r for r in rows], dtype=np.float64).reshape(len(specs), 4)


def _register_shapes(engine: BatchedMPC, table):
    """jsim_loop_set_vehicle_shapes (table None: clear the context's table, when it has one)."""
    if table is None:
        if engine.vehicle_shapes is not None:
            _cabi.check(engine.lib.jsim_loop_set_vehicle_shapes(engine._ctx, 0, None), engine._ctx, "jsim_loop_set_vehicle_shapes")
        engine.vehicle_shapes = None
        return
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.ndim != 2 or table.shape[1] != 4 or table.shape[0] < 1:
        raise ValueError("a shape table is [n >= 1, 4]: (cc_front, cc_rear, radius, wheelbase) per vehicle")
    if not (np.isfinite(table).all() and (table[:, 2:] > 0).all()):
        raise ValueError("a shape table needs finite circle offsets and positive radii and wheelbases")
    _cabi.check(engine.lib.jsim_loop_set_vehicle_shapes(engine._ctx, table.shape[0], table.ctypes.data_as(C.c_void_p)),
                engine._ctx, "jsim_loop_set_vehicle_shapes")
    engine.vehicle_shapes = table


class PreTick:
    """The loop glue ahead of MPC.step (main/scenarios/mpc_intersection.py:104-143) for the whole batch: progress index,
    ego-path resampling, obstacle prediction, collision check, cut-off -> writes the engine's `path_len`, i.e. the batched
    `mpc.set_trajectory_fromarray(trajectory_full[:cutoff_idx])`.  Obstacles are shared by all egos of the batch.

    mode = "speed_cutoff" is the glue of main/scenarios/mpc_intersection_new_ref.py (:122-139, FRAME_WINDOW = 20 there): the
    path is never truncated, the cut-off index goes to the mpc_with_speed controller instead
    (`mpc.set_trajectory_fromarray(trajectory_full, cutoff_idx=...)`: the speed reference is zeroed from it on) -- the
    engine must carry a speed reference (`cv`)."""

    def __init__(self, engine: BatchedMPC, frame_window: int = 10, time_horizon: float = 7.0, car_width: float = 2.0,
                 extra_length: float = 0.64, mode: str = "truncate", obstacle_dims: Optional[dict] = None,
                 margin_factor: int = 4):
        """obstacle_dims = dict(L=1.0, width=0.45, extra_length=0.64) gives the obstacles their own shape (the cyclist's
        BicycleRealDimensions of main/scenarios/overtaking_cyclist_bidirectional_road.py: prediction with that wheelbase,
        `check_collision_moving_bicycle`); margin_factor: EXTRA_CUTOFF_MARGIN = margin_factor * ceil(radius / dl) (4 in
        mpc_intersection.py:88-89, 2 in the cyclist scenario :94-95)."""
        if mode not in ("truncate", "speed_cutoff"):
            raise ValueError("mode must be 'truncate' or 'speed_cutoff'")
        if mode == "speed_cutoff" and engine.cv is None:
            raise ValueError("mode='speed_cutoff' needs an engine with a speed reference (cv)")
        self.mode = mode
        eng = self.eng = engine
        self.radius, (c0, c1) = car_circles(eng.L, car_width, extra_length)
        self.frame_window = int(frame_window)
        self.n_steps = int(math.ceil(time_horizon / eng.dt - 1e-9))          # len(np.arange(0, horizon, dt))
        self.margin = int(margin_factor) * int(math.ceil(self.radius / eng.dl))   # EXTRA_CUTOFF_MARGIN, :88-89
        # the shape of a vehicle without dims of its own in a loop's table: obstacle_dims if given, else the ego's shape
        self.default_shape = (c0, c1, self.radius, float(eng.L))
        _register_shapes(eng, None)                          # an earlier loop's table on this engine does not carry over
        _cabi.check(eng.lib.jsim_loop_set_geometry(eng._ctx, c0, c1, self.radius), eng._ctx, "jsim_loop_set_geometry")
        eng.ego_shape = (c0, c1, self.radius)
        if obstacle_dims is not None:
            oL = float(obstacle_dims["L"])
            orad, (o0, o1) = car_circles(oL, float(obstacle_dims.get("width", 2.0)), float(obstacle_dims.get("extra_length", 0.64)))
            _cabi.check(eng.lib.jsim_loop_set_obstacle_geometry(eng._ctx, o0, o1, orad, oL), eng._ctx,
                        "jsim_loop_set_obstacle_geometry")
            self.default_shape = (o0, o1, orad, oL)
        dev, B = eng.device, eng.B
        self.traj_idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.prev_len = torch.full((B,), -1, dtype=torch.int32, device=dev)   # tmp_trajectory is None
        self.col_flag = torch.zeros(B, dtype=torch.int32, device=dev)
        self.col_xy = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        self.first_idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.pred = None
        self.n_obs = 0
        self.cut = None
        if mode == "speed_cutoff":
            self.full_len = eng.path_len.clone()
            self.cut = eng.path_len.clone()              # = "no cut-off" (the reference's 999)
            eng.set_speed_cutoff(self.cut)
            self.cut = eng.cv_cut                        # the buffer the controller reads; updated in place every tick
        self.predict(torch.zeros(0, 6, dtype=torch.float64, device=dev))

    def predict(self, obst: torch.Tensor, shapes=None):
        """obst: device float64 [n_obs, 6] = (x, y, v, yaw, a, steer) per obstacle, as MovingObstacle*.get() returns.
        shapes: [n_obs, 4] rows (vehicle_shape) -- each obstacle predicted and tested with its own circles and wheelbase;
        registered when it differs from the engine's table and kept for later calls (None: the table stays as it is)."""
        eng = self.eng
        if not (obst.is_cuda and obst.dtype == torch.float64 and obst.dim() == 2 and obst.shape[1] == 6 and obst.is_contiguous()):
            raise ValueError("obst must be a contiguous float64 device tensor [n_obs, 6]")
        if shapes is not None:
            shapes = np.asarray(shapes, dtype=np.float64)
            if shapes.shape != (int(obst.shape[0]), 4):
                raise ValueError(f"shapes must be [n_obs = {int(obst.shape[0])}, 4], got {shapes.shape}")
            cur = eng.vehicle_shapes
            if cur is None or cur.shape != shapes.shape or not np.array_equal(cur, shapes):
                _register_shapes(eng, shapes)
        self.n_obs = int(obst.shape[0])
        self.pred = torch.zeros(max(self.n_obs, 1), self.n_steps, 3, dtype=torch.float64, device=eng.device)
        _cabi.check(eng.lib.jsim_loop_predict_obstacles(eng._ctx, self.n_obs, _ptr(obst) if self.n_obs else None,
                                                        self.n_steps, _ptr(self.pred), eng._stream()), eng._ctx,
                    "jsim_loop_predict_obstacles")
        return self.pred[: self.n_obs]

    def run(self, x0: torch.Tensor, debug: Optional[dict] = None):
        """Updates traj_idx and the engine's path_len for this tick (then remembers it as the previous truncated path)."""
        eng = self.eng
        eng._check_x0(x0)
        dbg_idx = dbg_n = None
        if debug is not None:
            dbg_idx, dbg_n = debug["res_idx"], debug["n_res"]
        out = eng.path_len if self.mode == "truncate" else self.cut
        _cabi.check(eng.lib.jsim_loop_pre_tick(
            eng._ctx, eng.B, _ptr(x0), _ptr(eng.path_id), _ptr(self.traj_idx), _ptr(self.prev_len), _ptr(out),
            _ptr(self.col_flag), _ptr(self.col_xy), _ptr(self.first_idx), _ptr(self.status), self.frame_window,
            self.margin, _ptr(dbg_idx), _ptr(dbg_n), eng._stream()), eng._ctx, "jsim_loop_pre_tick")
        # the previous tmp_trajectory: the truncated path, or always the full one (mpc_intersection_new_ref.py:131)
        self.prev_len.copy_(eng.path_len if self.mode == "truncate" else self.full_len)


class ScriptedObstacles:
    """Device-resident scripted obstacle vehicles of main/lib/moving_obstacles.py.
    specs: list of dicts like the scenarios build them (main/scenarios/mpc_intersection.py:46-49):
      kind="t_intersection" (default) | "roundabout": direction=+-1, turning=bool, speed=float, offset=float|None
      kind="arterial": x_init, y_init, speed, initial_speed, offset=float|None   (drives straight up)"""

    KINDS = {"t_intersection": 0.0, "roundabout": 1.0, "arterial": 2.0}

    def __init__(self, engine: BatchedMPC, specs, dt: Optional[float] = None):
        """A spec may carry dims=dict(L=..., width=..., extra_length=...): the vehicle's own shape (vehicle_shape; `shapes`
        holds each vehicle's row or None).  The loops register the table (shape_table); a caller that steps the vehicles itself
        passes it to PreTick.predict(shapes=...)."""
        specs = list(specs)
        self.shapes = [vehicle_shape(s["dims"]) if s.get("dims") is not None else None for s in specs]
        self.eng = engine
        dt = engine.dt if dt is None else dt
        st, pr = [], []
        for s in specs:
            kind = s.get("kind", "t_intersection")
            if kind not in self.KINDS:
                raise ValueError(f"unknown obstacle kind {kind!r}")
            off = s.get("offset", None)
            off = float(off) if (off is not None and off > 0) else 0.0
            if kind == "arterial":
                st.append([float(s["x_init"]), float(s["y_init"]), math.pi / 2, 0.0])
                pr.append([1.0, 0.0, float(s["speed"]), off, 0.0, float(dt), self.KINDS[kind], float(s["initial_speed"])])
                continue
            d = 1.0 if s.get("direction", 1) >= 0 else -1.0
            if d > 0:
                st.append([-30.0, -3.0, 0.0, 0.0]); x_turn = -10.0
            else:
                st.append([30.0, 3.0, math.pi, 0.0]); x_turn = 12.0
            pr.append([d, 1.0 if s.get("turning", False) else 0.0, float(s["speed"]), off, x_turn, float(dt), self.KINDS[kind], 0.0])
        dev = engine.device
        self.n = len(specs)
        self.state = torch.tensor(st, dtype=torch.float64, device=dev).reshape(self.n, 4)
        self.param = torch.tensor(pr, dtype=torch.float64, device=dev).reshape(self.n, 8)
        self.get_buf = torch.zeros(max(self.n, 1), 6, dtype=torch.float64, device=dev)
        self._state0 = self.state.clone()

    def reset(self):
        """Send the vehicles in again from their start poses (asynchronous device copy on the current stream)."""
        self.state.copy_(self._state0)

    def get(self, step: bool = False) -> torch.Tensor:
        """The `o.get()` tuples of all obstacles ([n, 6] device tensor); step=True also applies `o.step()` afterwards."""
        eng = self.eng
        _cabi.check(eng.lib.jsim_loop_obstacles(eng._ctx, self.n, _ptr(self.state), _ptr(self.param), _ptr(self.get_buf),
                                                1 if step else 0, eng._stream()), eng._ctx, "jsim_loop_obstacles")
        return self.get_buf[: self.n]


MAX_OBS = 8            # JSIM_MAX_OBS: obstacles one ego's glue can hold (scripted vehicles, then group mates)


def traffic_layout(B: int, sets, traffic_of, group_off=None):
    """The traffic-set layout of jsim_loop_set_traffic as (set_of [B], obs_off [n_sets + 1]), int32 host arrays.  sets: a list of
    per-set spec lists (0..8 vehicles each, ScriptedObstacles' dicts); traffic_of: the set of every ego ([B]), or with group_off
    ([n_groups + 1], InteractingLoop) the set of every group, expanded to its egos.  Raises ValueError on a wrong length, a set
    index out of range, a set of more than 8 vehicles, or (groups) a set's vehicles + the group mates exceeding 8."""
    sets = [list(st) for st in sets]
    if not sets:
        raise ValueError("need at least one traffic set")
    sizes = np.array([len(st) for st in sets], dtype=np.int64)
    if sizes.max() > MAX_OBS:
        raise ValueError(f"traffic set {int(sizes.argmax())} has {int(sizes.max())} vehicles (max {MAX_OBS})")
    tof = np.asarray(traffic_of).reshape(-1)
    n_units = B if group_off is None else len(group_off) - 1
    if tof.size != n_units or (tof.size and not np.issubdtype(tof.dtype, np.integer)):
        raise ValueError(f"traffic_of must hold {n_units} set indices ({'one per group' if group_off is not None else 'one per ego'}), "
                         f"got {tof.size}")
    if tof.size and (tof.min() < 0 or tof.max() >= len(sets)):
        raise ValueError(f"traffic_of holds set indices {tof.min()}..{tof.max()}, but there are {len(sets)} sets")
    if group_off is not None:
        gs = np.diff(np.asarray(group_off))
        over = sizes[tof] + gs - 1 > MAX_OBS
        if over.any():
            g = int(np.argmax(over))
            raise ValueError(f"group {g}: {int(sizes[tof[g]])} vehicles of set {int(tof[g])} + {int(gs[g]) - 1} group mates > {MAX_OBS}")
        tof = np.repeat(tof, gs)
    obs_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return tof.astype(np.int32), obs_off


def _register_traffic(engine: BatchedMPC, set_of, obs_off, chunk_ticks: int = 0):
    """jsim_loop_set_traffic (set_of None: clear the context's layout)."""
    if set_of is None:
        _cabi.check(engine.lib.jsim_loop_set_traffic(engine._ctx, engine.B, 0, None, None, 0), engine._ctx, "jsim_loop_set_traffic")
        engine.traffic_layout = None
        return
    _cabi.check(engine.lib.jsim_loop_set_traffic(engine._ctx, engine.B, len(obs_off) - 1, set_of.ctypes.data_as(C.c_void_p),
                                                 obs_off.ctypes.data_as(C.c_void_p), int(chunk_ticks)), engine._ctx,
                "jsim_loop_set_traffic")
    engine.traffic_layout = (set_of, obs_off)


class _GlueLoop:
    """What ScenarioLoop and InteractingLoop share: construction, run() and the recorder.  The loop constructed last on an engine
    owns its context's tables: ClosedLoop and PreTick clear an earlier recorder and shape table, the rest is registered here."""

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, obstacle_specs, hist_cap, max_age, frame_window, mode, traffic_of,
                 chunk_ticks, record, group_off=None):
        layout = None
        if traffic_of is not None:
            layout = traffic_layout(engine.B, obstacle_specs, traffic_of, group_off=group_off)   # before any device work
            obstacle_specs = [sp for st in obstacle_specs for sp in st]
        obstacle_specs = list(obstacle_specs)
        shape_table(obstacle_specs, vehicle_shape())                              # validates every dims, before any device work
        self.loop = ClosedLoop(engine, x0, hist_cap=hist_cap, max_age=max_age)
        self.pre = PreTick(engine, frame_window=frame_window, mode=mode)
        self.obst = ScriptedObstacles(engine, obstacle_specs)
        self.specs = obstacle_specs                  # the flat list (fork() hands each row its ego's vehicles)
        self.traffic = layout
        self._register_groups()
        _register_traffic(engine, *(layout if layout else (None, None)), chunk_ticks)
        shapes = self.shapes = shape_table(obstacle_specs, self.pre.default_shape)   # no dims: the glue's default shape
        if shapes is not None:
            _register_shapes(engine, shapes)
        if record:
            self.loop.recorder = Recorder(self.loop, record, n_obs=self.obst.n, groups=group_off)   # last: it records obst.n vehicles
            self.loop.recorder.glue = {"frame_window": self.pre.frame_window, "margin": self.pre.margin, "n_steps": self.pre.n_steps,
                                       "mode": self.pre.mode, "interacting": group_off is not None}

    def _register_groups(self):
        """Only InteractingLoop has groups."""

    @property
    def recorder(self) -> Optional[Recorder]:
        return self.loop.recorder

    def _run_args(self, n_obs: Optional[int] = None, speed_cutoff: Optional[int] = None):
        """What run() passes to the entry point after (ctx, B, n_ticks); n_obs / speed_cutoff: a value other than the loop's own."""
        loop, pre, ob = self.loop, self.pre, self.obst
        if speed_cutoff is None:
            speed_cutoff = 1 if pre.mode == "speed_cutoff" else 0
        return (*loop._loop_args(), _ptr(pre.traj_idx), _ptr(pre.prev_len), _ptr(pre.col_flag), _ptr(pre.status), pre.frame_window,
                pre.margin, ob.n if n_obs is None else n_obs, _ptr(ob.state) if ob.n else None, _ptr(ob.param) if ob.n else None,
                _ptr(ob.get_buf) if ob.n else None, pre.n_steps, speed_cutoff, loop.eng._stream())

    def run(self, n_ticks: int):
        """n_ticks ticks in one call (_ENTRY), same results as n_ticks x tick().  jsim_loop_run_scenario with a register kernel
        (config.ONE_WAVE_HORIZONS / FOUR_WAVE_HORIZONS) and MAX_ITER = 1: three launches -- the scripted obstacles rolled forward
        n_ticks ticks, their predictions for every tick, one fused launch of n_ticks x (glue + solve + plant) per wavefront."""
        eng, lib = self.loop.eng, self.loop.eng.lib
        _cabi.check(getattr(lib, self._ENTRY)(eng._ctx, eng.B, int(n_ticks), *self._run_args()), eng._ctx, self._ENTRY)
        self.pre.n_obs = self.obst.n


class ScenarioLoop(_GlueLoop):
    """The reference scenario loop for a batch, entirely on the device (main/scenarios/mpc_intersection.py:99-163):
    obstacle get() -> prediction -> progress index / resample / collision / cut-off -> MPC.step -> plant, history, goal ->
    obstacle step().

    traffic_of ([B] set indices): every ego meets its own scripted vehicles -- obstacle_specs is then a list of traffic sets
    (per-set spec lists, traffic_layout), all of whose vehicles step every tick; ego e's results are those of a ScenarioLoop
    whose obstacle_specs are set traffic_of[e], bit for bit.  chunk_ticks: ticks per fused launch (0: from a 512 MiB budget).
    record: ticks of the full History kept on the device, the vehicles' get() tuples included (`recorder`; 0: none).
    A spec with dims=dict(L=..., width=..., extra_length=...) gives that vehicle its own shape (vehicle_shape): a car and a
    cyclist in one loop, or per set.  Vehicles without dims have the ego's shape; no dims anywhere: no table is registered."""

    _ENTRY = "jsim_loop_run_scenario"

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, obstacle_specs, hist_cap: int = 0, max_age: int = 0,
                 frame_window: int = 10, mode: str = "truncate", traffic_of=None, chunk_ticks: int = 0, record: int = 0):
        super().__init__(engine, x0, obstacle_specs, hist_cap, max_age, frame_window, mode, traffic_of, chunk_ticks, record)

    def tick(self):
        if self.traffic is not None:             # the vehicles of all sets: the gridded kernels of run()
            self.run(1)
            return
        g = self.obst.get(step=False)
        self.pre.predict(g)
        self.pre.run(self.loop.x0)
        self.loop.tick()
        resp = self.loop.age == 0                    # respawned this tick: the glue starts over like for a new run
        self.pre.traj_idx.masked_fill_(resp, 0)
        self.pre.prev_len.masked_fill_(resp, -1)
        g = self.obst.get(step=True)
        rec = self.loop.recorder
        if rec is not None and rec.n_obs:
            rec._record_obstacles(g)

    def fork(self, ego, at, paths=None, path_id=None, speed=None, record: int = 0, max_age: Optional[int] = None,
             chunk_ticks: int = 0, cv=None) -> "ScenarioLoop":
        """A new ScenarioLoop on a new engine whose row r starts where ego ego[r] of this loop's recording stood at the start of
        recorded tick at[r], on a path of its own and with a cold controller: what perform_replan of
        main/scenarios/overtaking_cyclist_bidirectional_road.py (:394-402) does when it builds a fresh MPC on the chosen trajectory
        and lets the same simulation and the same cyclist go on.  Rows, not egos: one ego forked at its trigger tick onto each of
        its candidates drives them all in one batch.

        paths / path_id: the new engine's route table and every row's route (paths=None: this engine's paths, path_id defaulting
        to the ego's own); speed: per row (default: the ego's own); cv: the speed references of new paths under
        mode="speed_cutoff" (paths=None: this engine's).  T, config, dt, dl, L, the egos' rows of a per-ego table
        (set_ego_configs), frame_window, mode and hist_cap are this loop's; max_age too unless given.  x0 and x0_spawn are the fork
        states (Recorder.fork_state), loop.age = at - k0, the glue starts as for a new run and the controller cold: no warm start,
        path index 0 -- but a row that starts its ego's episode (age 0) on the ego's own route is that ego's respawn and has the
        path index this loop respawns it with, so that it replays the episode.  Row r meets the vehicles of its ego's
        traffic set (the whole list of a loop without sets; dims carried over) where they stood at tick at[r]
        (jsim_loop_obstacles_at); obst.reset() returns there.  Rows of one source set and one tick share a set.
        This loop, its engine and its recorder are left as they are.
        ValueError: no recorder; what fork_state, BatchedMPC and traffic_layout raise; new paths without path_id."""
        src, eng, rec = self.loop, self.loop.eng, self.recorder
        if rec is None:
            raise ValueError("fork needs the loop's recording (record=...)")
        x0, k0, age = rec.fork_state(ego, at)
        ego, at = history.fork_rows(eng.B, rec._n(), ego, at)
        R = ego.size
        if R < 1:
            raise ValueError("fork needs at least one row")
        idx = torch.from_numpy(ego.astype(np.int64)).to(eng.device)
        own_paths = paths is None
        if own_paths:
            paths, cv, smooth = [p.copy() for p in eng.paths], eng.cv, False        # (unwrapped already)
            if path_id is None:
                path_id = eng.path_id[idx].cpu().numpy()
        else:
            smooth = True
            if path_id is None:
                raise ValueError("new paths need a path_id per row")
        pid = np.asarray(path_id)
        pid = np.broadcast_to(pid, (R,)) if pid.ndim == 0 else pid
        if pid.shape != (R,):
            raise ValueError(f"path_id must hold one route per row ({R}), got {pid.shape}")
        spd = eng.speed[idx].cpu().numpy() if speed is None else np.asarray(speed, dtype=np.float64)
        if spd.shape not in ((), (R,)):
            raise ValueError(f"speed must be one number or one per row ({R}), got {spd.shape}")
        new = BatchedMPC(paths, pid, dl=eng.dl, L=eng.L, speed=spd, dt=eng.dt, T=eng.T, config=eng.config, device=eng.device,
                         smooth=smooth, cv=cv)
        pe = getattr(eng, "_pe", None)
        if pe is not None:
            new.set_ego_configs(pe[idx])
        # traffic: one set per (source set, tick) among the rows, the rows' own order of first appearance
        n_src = self.obst.n
        if self.traffic is None:
            src_set, src_off = np.zeros(eng.B, dtype=np.int64), np.array([0, n_src])
        else:
            src_set, src_off = self.traffic
        keys, tof = {}, np.empty(R, dtype=np.int32)
        for r in range(R):
            tof[r] = keys.setdefault((int(src_set[ego[r]]), int(at[r])), len(keys))
        veh = [np.arange(src_off[s], src_off[s + 1]) for s, _ in keys]                # each new set's vehicles among the source's
        sets = [[self.specs[o] for o in v] for v in veh]
        shared = self.traffic is None and len(keys) == 1
        fork = ScenarioLoop(new, x0, sets[0] if shared else sets, hist_cap=src.hist_cap,
                            max_age=src.max_age if max_age is None else max_age, frame_window=self.pre.frame_window, mode=self.pre.mode,
                            traffic_of=None if shared else tof, chunk_ticks=chunk_ticks, record=record)
        fork.loop.age.copy_(torch.from_numpy(np.ascontiguousarray(age, dtype=np.int32)))
        if own_paths:
            # a row that starts its ego's episode on the ego's own route is that ego's respawn: the path index it respawns with
            again = torch.from_numpy((age == 0) & (pid == eng.path_id[idx].cpu().numpy())).to(eng.device)
            new.target_ind.copy_(torch.where(again, src.target_spawn[idx], new.target_ind))
            fork.loop.target_spawn.copy_(new.target_ind)
        if fork.obst.n:
            pick = torch.from_numpy(np.concatenate(veh).astype(np.int64)).to(eng.device)
            ticks = np.ascontiguousarray(np.concatenate([np.full(len(v), k, dtype=np.int32) for v, (_, k) in zip(veh, keys)]))
            state0 = self.obst._state0[pick].contiguous()
            wheel = None if fork.shapes is None else torch.from_numpy(np.ascontiguousarray(fork.shapes[:, 3])).to(eng.device)
            state = torch.empty_like(state0)
            _cabi.check(new.lib.jsim_loop_obstacles_at(new._ctx, fork.obst.n, _ptr(state0), _ptr(fork.obst.param), _ptr(wheel),
                                                       ticks.ctypes.data_as(C.c_void_p), _ptr(state), new._stream()), new._ctx,
                        "jsim_loop_obstacles_at")
            fork.obst.state.copy_(state)
            fork.obst._state0.copy_(state)
        return fork


MAX_GROUP = MAX_OBS    # the obstacles of an ego are the scripted ones plus its group mates


def group_offsets(B: int, group_off=None, group_sizes=None) -> np.ndarray:
    """The group layout of InteractingLoop as offsets [n_groups + 1] (int32): group_off itself, or the running sum of
    group_sizes.  Raises ValueError unless exactly one is given, the groups cover 0..B contiguously and each has 1..8 egos."""
    if (group_off is None) == (group_sizes is None):
        raise ValueError("pass exactly one of group_off and group_sizes")
    if group_sizes is not None:
        sizes = np.asarray(group_sizes).reshape(-1)
        if sizes.size == 0 or not np.issubdtype(sizes.dtype, np.integer):
            raise ValueError("group_sizes must be a non-empty sequence of integers")
        off = np.concatenate([[0], np.cumsum(sizes)])
    else:
        off = np.asarray(group_off).reshape(-1)
        if off.size < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError("group_off must hold n_groups + 1 >= 2 integers")
    sizes = np.diff(off)
    if off[0] != 0 or off[-1] != B:
        raise ValueError(f"the groups must cover egos 0..{B}: offsets run {off[0]}..{off[-1]}")
    if sizes.min() < 1 or sizes.max() > MAX_GROUP:
        raise ValueError(f"every group needs 1..{MAX_GROUP} egos (sizes {sizes.min()}..{sizes.max()})")
    return off.astype(np.int32)


class InteractingLoop(_GlueLoop):
    """Several automated vehicles at one intersection that react to each other (main/scenarios/interactive_mpc.py:117-190):
    ScenarioLoop's tick, where the obstacles of an ego are the scripted vehicles (spec order) and then the OTHER egos of its
    group (ascending batch index), every ego predicted like an obstacle from its tick-start state with a = 0 and the steering
    it applied last tick.  A tick is a Jacobi step: all egos solve, then all advance.  Groups are contiguous batch ranges
    (group_off [n_groups + 1], or group_sizes), 1..8 egos each; n_obs + largest group - 1 <= 8.  Egos in different groups
    never affect each other; a group of one ego is ScenarioLoop.  Only the truncate glue.  Scripted vehicles have the ego's shape
    unless their spec carries dims= (a cyclist beside the egos); the group mates always have the ego's.
    run(n_ticks): n_ticks ticks in one call (jsim_loop_run_interacting; separate launches per tick).
    traffic_of ([n_groups] set indices): every group meets its own scripted vehicles -- obstacle_specs is then a list of traffic
    sets (traffic_layout); the vehicles of a group's set + the group - 1 <= 8, per group.
    record: ticks of the full History kept on the device (`recorder`, as ScenarioLoop's); the egos are recorded like any other."""

    _ENTRY = "jsim_loop_run_interacting"

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, group_off=None, obstacle_specs=(), hist_cap: int = 0,
                 max_age: int = 0, frame_window: int = 20, group_sizes=None, traffic_of=None, record: int = 0):
        off = self.group_off = group_offsets(engine.B, group_off, group_sizes)        # before any device work
        n_obs, big = len(obstacle_specs), int(np.diff(off).max())
        if traffic_of is None and n_obs + big - 1 > MAX_GROUP:
            raise ValueError(f"{n_obs} scripted obstacles + the largest group ({big}) - 1 > {MAX_GROUP}")
        super().__init__(engine, x0, obstacle_specs, hist_cap, max_age, frame_window, "truncate", traffic_of, 0, record,
                         group_off=off)

    def _register_groups(self):
        eng, off = self.loop.eng, self.group_off
        _cabi.check(eng.lib.jsim_loop_set_groups(eng._ctx, eng.B, len(off) - 1, off.ctypes.data_as(C.c_void_p)), eng._ctx,
                    "jsim_loop_set_groups")

    def pred_egos(self) -> torch.Tensor:
        """[B, n_steps, 3] (x, y, yaw): every ego's prediction from its current state, as the next tick will make it."""
        eng = self.loop.eng
        pred = torch.zeros(eng.B, self.pre.n_steps, 3, dtype=torch.float64, device=eng.device)
        _cabi.check(eng.lib.jsim_loop_predict_egos(eng._ctx, eng.B, _ptr(self.loop.x0), _ptr(eng.di_ai), self.pre.n_steps,
                                                   _ptr(pred), eng._stream()), eng._ctx, "jsim_loop_predict_egos")
        return pred

    def tick(self):
        self.run(1)

    def fork(self, *args, **kwargs):
        """Refused: a forked ego's group mates would have to go on with the controllers they had."""
        raise ValueError("an InteractingLoop cannot be forked: the group mates' warm starts (oa, od) are not recorded, so their "
                         "controllers cannot be continued from a recorded tick")
