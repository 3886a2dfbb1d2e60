"""Closed-loop driver for a batch of egos: the reference's per-vehicle loop
(main/scenarios/mpc_intersection.py:99-163) with the B-ego `for` replaced by one MPC launch + one
bookkeeping launch per tick, nothing leaving the device between ticks."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _cabi, history
from .batched import BatchedMPC, _ptr
from .checkpoint import Checkpointed, Checkpoints, check_every
from .history import MAX_OBS
from .recorder import Recorder, _register_recorder
from .synth import pack_paths, smooth_yaw_inplace
from .vehicle import car_circles, vehicle_shape


class ClosedLoop(Checkpointed):
    """tick(): jsim_mpc_step then jsim_loop_advance (plant, history, respawn of finished egos).

    hist_cap: ticks of (di, ai) history kept on the device ([hist_cap, B, 2]); max_age: safety respawn
    after that many ticks (<= 0: only MPC.is_goal ends an ego's run); record: ticks of the full History kept on the device
    (`recorder`, a Recorder; 0: none).
    checkpoint_every=C (with record): the loop's whole live state (history.CHECKPOINT) is kept at the start of every C-th tick
     -- run(n) is issued in pieces that end at those ticks, the results are the same bit for bit;
    `checkpoints` lists the written slots, restore(slot) rewinds the loop, save_checkpoints / load_checkpoints carry the slabs to
    another process.  checkpoint_slots: more slots than record // C + 1 (for a smaller C after a restore)."""

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, hist_cap: int = 0, max_age: int = 0, record: int = 0,
                 checkpoint_every: Optional[int] = None, checkpoint_slots: Optional[int] = None):
        if checkpoint_every is not None:
            check_every(checkpoint_every, record)      # before any device work
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
        if checkpoint_every is not None:
            self._ck = Checkpoints({"loop": self, "eng": eng}, checkpoint_every, record, checkpoint_slots)

    def _advance_args(self):
        """What tick() passes to jsim_loop_advance after (ctx, B)."""
        eng = self.eng
        return (_ptr(self.x0), _ptr(eng.oa), _ptr(eng.od), _ptr(eng.status), _ptr(eng.di_ai), _ptr(eng.target_ind),
                _ptr(eng.path_id), _ptr(eng.path_len), _ptr(self.x0_spawn), _ptr(self.target_spawn), _ptr(self.age), self.max_age,
                _ptr(self.hist), _ptr(self.tick_counter), self.hist_cap, _ptr(self.n_respawn), eng._stream())

    def tick(self):
        eng = self.eng
        for _ in self._pieces(1):
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
        for n in self._pieces(n_ticks):      # (without checkpoints: n_ticks itself)
            _cabi.check(eng.lib.jsim_mpc_run_ticks(eng._ctx, eng.B, n, *self._loop_args(), eng._stream()), eng._ctx,
                        "jsim_mpc_run_ticks")

    # ---- hipGraph: a launch-bound inner loop (two short kernels per tick) replayed without host work
    def capture(self, ticks: int):
        """Capture `ticks` consecutive ticks into one hipGraph (all pointers are fixed device buffers and the
        history slot comes from the device tick counter, so replays continue the same simulation).  ValueError on a loop with
        checkpoints: a replayed graph advances ticks the host does not see."""
        if self._ck is not None:
            raise ValueError("a loop with checkpoints cannot be captured: a replayed graph advances ticks the host does not count")
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


ROUTE_ENDS = {"leave": 0.0, "stop": 1.0}
ROUTE_PARK = float(_cabi._K["JSIM_ROUTE_PARK"])     # where a route vehicle that has left stands


def route_array(route) -> np.ndarray:
    """A route spec's polyline as the [N, 3] float64 array (x, y, yaw) the table takes (a copy): two columns get the yaw of the
    segment ahead (the last point the last segment's), and the yaw is made continuous (smooth_yaw).  ValueError: not [N >= 1, 2 or
    3], or a value that is not finite."""
    r = np.array(route, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] not in (2, 3) or r.shape[0] < 1:
        raise ValueError(f"a route is an array [N >= 1, 3] (x, y, yaw) or [N, 2] (x, y), got {r.shape}")
    if not np.isfinite(r).all():
        raise ValueError("a route holds a value that is not finite")
    if r.shape[1] == 2:
        yaw = np.zeros(r.shape[0])
        if r.shape[0] >= 2:
            d = np.diff(r, axis=0)
            yaw[:-1] = np.arctan2(d[:, 1], d[:, 0])
            yaw[-1] = yaw[-2]
        r = np.column_stack([r, yaw])
    smooth_yaw_inplace(r[:, 2])
    return np.ascontiguousarray(r)


def route_table(specs, dt: float):
    """The route table of a flat list of vehicle specs: (routes, rows) -- the distinct route arrays (route_array) of its
    kind="route" specs, equal arrays shared, and each such spec's param row (route, end, speed, offset, s0, dt, 3, period_ticks)
    of include/jsim_mpc.h's rule (None for a spec of another kind).  Needs no device.  ValueError: what route_array raises, an
    unknown `end`, s0 < 0, speed < 0 (or either not finite), a period that is no whole number of ticks >= 1."""
    routes, index, rows = [], {}, []
    for i, s in enumerate(specs):
        if s.get("kind", "t_intersection") != "route":
            rows.append(None)
            continue
        r = route_array(s["route"])
        end = s.get("end", "leave")
        if end not in ROUTE_ENDS:
            raise ValueError(f"vehicle {i}: end must be one of {sorted(ROUTE_ENDS)}, got {end!r}")
        speed, s0 = float(s["speed"]), float(s.get("s0", 0.0))
        if not (math.isfinite(speed) and speed >= 0):
            raise ValueError(f"vehicle {i}: speed={speed} (a route vehicle never reverses)")
        if not (math.isfinite(s0) and s0 >= 0):
            raise ValueError(f"vehicle {i}: s0={s0} (an arc length from the route's first point)")
        off = s.get("offset", None)
        off = float(off) if (off is not None and off > 0) else 0.0
        ticks = 0
        if s.get("period") is not None:
            ticks = int(round(float(s["period"]) / dt))
            if ticks < 1 or abs(float(s["period"]) / dt - ticks) > 1e-9:
                raise ValueError(f"vehicle {i}: period={s['period']} s is no whole number of ticks >= 1 of dt={dt}")
        key = (r.shape[0], r.tobytes())
        if key not in index:
            index[key] = len(routes)
            routes.append(r)
        rows.append([float(index[key]), ROUTE_ENDS[end], speed, off, s0, float(dt), ScriptedObstacles.KINDS["route"], float(ticks)])
    return routes, rows


def _register_routes(engine: BatchedMPC, routes):
    """jsim_loop_set_traffic_routes (no routes: clear the context's table, when it has one)."""
    if not routes:
        if engine.traffic_routes is not None:
            _cabi.check(engine.lib.jsim_loop_set_traffic_routes(engine._ctx, 0, None, None, None, None), engine._ctx,
                        "jsim_loop_set_traffic_routes")
        engine.traffic_routes = None
        return
    x, y, yaw, off = pack_paths(routes)
    off = np.ascontiguousarray(off, dtype=np.int32)
    _cabi.check(engine.lib.jsim_loop_set_traffic_routes(engine._ctx, len(routes), *(a.ctypes.data_as(C.c_void_p) for a in (x, y, yaw, off))),
                engine._ctx, "jsim_loop_set_traffic_routes")
    engine.traffic_routes = routes


def traffic_on_routes(routes, speed: float, headway_s: float, n: int, **spec):
    """A stream of arrivals on every route: n kind="route" specs per route, the k-th entering k * headway_s seconds after the
    first (offset).  routes: arrays [N, 3] or [N, 2] (typically PlannedRoute.trajectory); spec: further keys of every spec (end,
    period, s0, dims).  Returns the flat list, route after route."""
    if n < 0 or not headway_s >= 0:
        raise ValueError(f"n={n}, headway_s={headway_s}")
    return [dict(kind="route", route=r, speed=speed, offset=(k * headway_s) or None, **spec) for r in routes for k in range(int(n))]


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
      kind="arterial": x_init, y_init, speed, initial_speed, offset=float|None   (drives straight up)
      kind="route": route=array [N, 3] (x, y, yaw) or [N, 2], speed, offset=float|None, s0=0.0, end="leave"|"stop",
        period=seconds|None -- a vehicle that follows the polyline (typically a PlannedRoute.trajectory) from arc length s0 at
        `speed` after `offset` seconds, stops at or leaves from its end and enters again every `period` seconds
        (include/jsim_mpc.h states the rule).  The distinct route arrays of the specs are the engine's route
        table (`routes`), registered here; without a route spec an earlier table of the engine is cleared."""

    KINDS = {"t_intersection": 0.0, "roundabout": 1.0, "arterial": 2.0, "route": 3.0}

    def __init__(self, engine: BatchedMPC, specs, dt: Optional[float] = None):
        """A spec may carry dims=dict(L=..., width=..., extra_length=...): the vehicle's own shape (vehicle_shape; `shapes`
        holds each vehicle's row or None).  The loops register the table (shape_table); a caller that steps the vehicles itself
        passes it to PreTick.predict(shapes=...)."""
        specs = list(specs)
        self.shapes = [vehicle_shape(s["dims"]) if s.get("dims") is not None else None for s in specs]
        self.eng = engine
        dt = engine.dt if dt is None else dt
        for s in specs:
            if s.get("kind", "t_intersection") not in self.KINDS:
                raise ValueError(f"unknown obstacle kind {s.get('kind')!r}")
        self.routes, route_rows = route_table(specs, dt)         # validates every route spec, before any device work
        st, pr = [], []
        for s, row in zip(specs, route_rows):
            kind = s.get("kind", "t_intersection")
            if row is not None:
                st.append([0.0, 0.0, 0.0, 0.0])                  # (the pose slots are outputs of the first call)
                pr.append(row)
                continue
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
        _register_routes(engine, self.routes)

    def reset(self):
        """Send the vehicles in again from their start poses (asynchronous device copy on the current stream)."""
        self.state.copy_(self._state0)

    def get(self, step: bool = False) -> torch.Tensor:
        """The `o.get()` tuples of all obstacles ([n, 6] device tensor); step=True also applies `o.step()` afterwards."""
        eng = self.eng
        _cabi.check(eng.lib.jsim_loop_obstacles(eng._ctx, self.n, _ptr(self.state), _ptr(self.param), _ptr(self.get_buf),
                                                1 if step else 0, eng._stream()), eng._ctx, "jsim_loop_obstacles")
        return self.get_buf[: self.n]


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


class _GlueLoop(Checkpointed):
    """What ScenarioLoop and InteractingLoop share: construction, run(), the recorder and the checkpoints (checkpoint_every,
    checkpoint_slots: as ClosedLoop's, the glue's and the scripted vehicles' state included).  The loop constructed last on an engine
    owns its context's tables: ClosedLoop and PreTick clear an earlier recorder and shape table, the rest is registered here."""

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, obstacle_specs, hist_cap, max_age, frame_window, mode, traffic_of,
                 chunk_ticks, record, group_off=None, record_plans=False, checkpoint_every=None, checkpoint_slots=None):
        if checkpoint_every is not None:
            check_every(checkpoint_every, record)                                     # before any device work
        layout = None
        if traffic_of is not None:
            layout = traffic_layout(engine.B, obstacle_specs, traffic_of, group_off=group_off)   # before any device work
            obstacle_specs = [sp for st in obstacle_specs for sp in st]
        obstacle_specs = list(obstacle_specs)
        shape_table(obstacle_specs, vehicle_shape())                              # validates every dims, before any device work
        for sp in obstacle_specs:
            if sp.get("kind", "t_intersection") not in ScriptedObstacles.KINDS:
                raise ValueError(f"unknown obstacle kind {sp.get('kind')!r}")
        route_table(obstacle_specs, engine.dt)                                    # and every route spec
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
                                       "mode": self.pre.mode, "interacting": group_off is not None,
                                       "mate_prediction": getattr(self, "mate_prediction", "constant"),
                                       "record_plans": bool(record_plans)}
            if record_plans:
                self.loop.recorder._record_plans()
        if checkpoint_every is not None:
            self._ck = Checkpoints(self._owners(), checkpoint_every, record, checkpoint_slots)

    def _owners(self) -> dict:
        """The objects that own this loop's live state, under history.CHECKPOINT's names."""
        return {"loop": self.loop, "eng": self.loop.eng, "pre": self.pre, "obst": self.obst}

    def _register_groups(self):
        """Only InteractingLoop has groups."""

    # ---- what the forks share (DESIGN.md sections 22 and 30)
    def _fork_engine(self, idx: torch.Tensor, paths, pid, speed, smooth: bool, cv, config, ego_configs) -> BatchedMPC:
        """The new engine of a fork whose rows are this engine's egos idx: T, dt, dl, L are this engine's; speed, config and the rows
        of the per-ego table too unless given."""
        eng, R = self.loop.eng, int(idx.numel())
        spd = eng.speed[idx].cpu().numpy() if speed is None else np.asarray(speed, dtype=np.float64)
        if spd.shape not in ((), (R,)):
            raise ValueError(f"speed must be one number or one per row ({R}), got {spd.shape}")
        new = BatchedMPC(paths, pid, dl=eng.dl, L=eng.L, speed=spd, dt=eng.dt, T=eng.T, config=eng.config if config is None else config,
                         device=eng.device, smooth=smooth, cv=cv)
        pe = getattr(eng, "_pe", None)
        if ego_configs is not None:
            new.set_ego_configs(ego_configs)
        elif pe is not None:
            new.set_ego_configs(pe[idx])
        return new

    def _fork_traffic(self, set_of_row, at):
        """The traffic of a fork: one set per (source set, tick) among the rows, in the rows' own order of first appearance.  Returns
        (keys, tof [rows], veh: each new set's vehicles among the source's, sets: their specs, shared: one set for a loop without
        sets -- the fork is then a loop like the source, with one shared list)."""
        src_off = np.array([0, self.obst.n]) if self.traffic is None else self.traffic[1]
        keys, tof = {}, np.empty(len(at), dtype=np.int32)
        for r in range(len(at)):
            tof[r] = keys.setdefault((int(set_of_row[r]), int(at[r])), len(keys))
        veh = [np.arange(src_off[s], src_off[s + 1]) for s, _ in keys]
        sets = [[self.specs[o] for o in v] for v in veh]
        return keys, tof, veh, sets, self.traffic is None and len(keys) == 1

    def _source_sets(self) -> np.ndarray:
        """The traffic set of every ego of this loop (all 0 for a loop without sets)."""
        return np.zeros(self.loop.eng.B, dtype=np.int64) if self.traffic is None else self.traffic[0]

    def _warm_rows(self, n_units: int, unit, at):
        """The rows of a warm fork, checked: (unit [R], at [R], slot [R]) -- every tick must be a checkpointed one."""
        ck = self._need_ck()
        unit, at = history.fork_rows(n_units, ck.t, unit, at)
        if unit.size < 1:
            raise ValueError("fork needs at least one row")
        return unit, at, history.checkpoint_at(ck.slot_tick, at)

    def _load_warm(self, fork: "_GlueLoop", ego, slot, keys, veh):
        """Every row of `fork` continues ego ego[r] from slot slot[r], its vehicles from the slots of their ticks
        (jsim_loop_checkpoint_load); obst.reset() returns there."""
        ck = self._ck
        veh_src = np.concatenate(veh) if veh else np.zeros(0, dtype=np.int64)
        key_slot = history.checkpoint_at(ck.slot_tick, [k for _, k in keys])
        veh_slot = np.concatenate([np.full(len(v), s) for v, s in zip(veh, key_slot)]) if veh else np.zeros(0, dtype=np.int64)
        ck.load_into(fork._owners(), ego, slot, veh_src, veh_slot)
        if fork.obst.n:
            fork.obst._state0.copy_(fork.obst.state)

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
        for n in self._pieces(n_ticks):          # (without checkpoints: n_ticks itself)
            _cabi.check(getattr(lib, self._ENTRY)(eng._ctx, eng.B, n, *self._run_args()), eng._ctx, self._ENTRY)
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
    cyclist in one loop, or per set.  Vehicles without dims have the ego's shape; no dims anywhere: no table is registered.
    checkpoint_every, checkpoint_slots: as ClosedLoop's, with the glue's and the vehicles' state; such a loop
    can be rewound (restore) and forked warm (fork(..., warm=True)): rows that continue egos from checkpointed ticks."""

    _ENTRY = "jsim_loop_run_scenario"

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, obstacle_specs, hist_cap: int = 0, max_age: int = 0,
                 frame_window: int = 10, mode: str = "truncate", traffic_of=None, chunk_ticks: int = 0, record: int = 0,
                 checkpoint_every: Optional[int] = None, checkpoint_slots: Optional[int] = None):
        super().__init__(engine, x0, obstacle_specs, hist_cap, max_age, frame_window, mode, traffic_of, chunk_ticks, record,
                         checkpoint_every=checkpoint_every, checkpoint_slots=checkpoint_slots)

    def tick(self):
        if self.traffic is not None:             # the vehicles of all sets: the gridded kernels of run()
            self.run(1)
            return
        for _ in self._pieces(1):                # (a checkpoint that is due is saved first)
            self._host_tick()

    def _host_tick(self):
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
             chunk_ticks: int = 0, cv=None, warm: bool = False, config=None, ego_configs=None,
             checkpoint_every: Optional[int] = None, checkpoint_slots: Optional[int] = None) -> "ScenarioLoop":
        """warm=True (a loop with checkpoints): every row CONTINUES ego ego[r] from the checkpoint at tick
        at[r] -- state, age, spawn state, the controller's warm start and remembered path index, the glue's progress index, previous
        path length and cut-off, and its traffic set's vehicles, all as they stood (jsim_loop_checkpoint_load) -- so that, with
        nothing changed, the fork's records are the source's from that tick on, bit for bit; with another speed, max_age, config or
        ego_configs it is the counterfactual from that tick.  at[r] must be a checkpointed tick (`checkpoints`); paths, path_id and
        cv are refused: a warm start belongs to its path.  record, checkpoint_every, checkpoint_slots: the new loop's own.
        config / ego_configs (either kind of fork): the new engine's configuration and per-ego table (default: this engine's, the
        table's rows of the forked egos).

        warm=False, the cold fork:
        A new ScenarioLoop on a new engine whose row r starts where ego ego[r] of this loop's recording stood at the start of
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
        ValueError: no recorder; what fork_state, BatchedMPC and traffic_layout raise; new paths without path_id; warm=True without
        checkpoints, with paths / path_id / cv, or at a tick that is not checkpointed (the message names the nearest ones)."""
        src, eng, rec = self.loop, self.loop.eng, self.recorder
        kw = dict(hist_cap=src.hist_cap, max_age=src.max_age if max_age is None else max_age, frame_window=self.pre.frame_window,
                  mode=self.pre.mode, chunk_ticks=chunk_ticks, record=record, checkpoint_every=checkpoint_every,
                  checkpoint_slots=checkpoint_slots)
        if warm:
            if paths is not None or path_id is not None or cv is not None:
                raise ValueError("a warm fork keeps every ego on its own path (a warm start belongs to its path): paths, path_id and "
                                 "cv are the cold fork's")
            ego, at, slot = self._warm_rows(eng.B, ego, at)
            idx, sl = (torch.from_numpy(v.astype(np.int64)).to(eng.device) for v in (ego, slot))
            new = self._fork_engine(idx, [p.copy() for p in eng.paths], eng.path_id[idx].cpu().numpy(), speed, False, eng.cv, config,
                                    ego_configs)
            keys, tof, veh, sets, shared = self._fork_traffic(self._source_sets()[ego], at)
            fork = ScenarioLoop(new, self._ck.slabs["x0"][sl, idx].contiguous(), sets[0] if shared else sets,
                                traffic_of=None if shared else tof, **kw)
            self._load_warm(fork, ego, slot, keys, veh)
            return fork
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
        new = self._fork_engine(idx, paths, pid, speed, smooth, cv, config, ego_configs)
        # traffic: one set per (source set, tick) among the rows, the rows' own order of first appearance
        keys, tof, veh, sets, shared = self._fork_traffic(self._source_sets()[ego], at)
        fork = ScenarioLoop(new, x0, sets[0] if shared else sets, traffic_of=None if shared else tof, **kw)
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
    record: ticks of the full History kept on the device (`recorder`, as ScenarioLoop's); the egos are recorded like any other.
    mate_prediction: "constant" (above), or "plan": the egos share their MPC plans -- an ego is predicted
    by rolling the controls its controller holds at the start of the tick (eng.oa, eng.od of its last solve, from element 1 on,
    then the last steering held at constant speed; after a failed solve the steering applied last tick at constant speed) through
    the plant's own step, so an ego that has planned to stop in front of a conflict is predicted to stop there.  The loop
    constructed last on an engine sets the engine's mode.
    record_plans (with record, under either mate_prediction): every tick's plans -- eng.oa, eng.od, eng.status as they stand at the
    start of the tick -- are kept on the device beside the History (`recorder.plans`); the run itself is the
    same bit for bit.  With them Recorder.cutoffs() replays a plan-mode recording and Recorder.predictions(egos="plan") scores the
    plan rule against what each ego then did; a plan-mode recording without them has neither.
    checkpoint_every, checkpoint_slots: as ScenarioLoop's; fork(group, at, warm=True) then continues whole
    groups from a checkpointed tick, under this or the other mate_prediction."""

    _ENTRY = "jsim_loop_run_interacting"

    def __init__(self, engine: BatchedMPC, x0: torch.Tensor, group_off=None, obstacle_specs=(), hist_cap: int = 0,
                 max_age: int = 0, frame_window: int = 20, group_sizes=None, traffic_of=None, record: int = 0,
                 mate_prediction: str = "constant", record_plans: bool = False, checkpoint_every: Optional[int] = None,
                 checkpoint_slots: Optional[int] = None):
        if mate_prediction not in _cabi.MATE_PREDICTION:                              # before any device work
            raise ValueError(f"mate_prediction must be one of {sorted(_cabi.MATE_PREDICTION)}, got {mate_prediction!r}")
        if record_plans and not record:
            raise ValueError("record_plans needs a recorder: record must be a positive number of ticks")
        if checkpoint_every is not None:
            check_every(checkpoint_every, record)
        self.mate_prediction = mate_prediction
        off = self.group_off = group_offsets(engine.B, group_off, group_sizes)
        n_obs, big = len(obstacle_specs), int(np.diff(off).max())
        if traffic_of is None and n_obs + big - 1 > MAX_GROUP:
            raise ValueError(f"{n_obs} scripted obstacles + the largest group ({big}) - 1 > {MAX_GROUP}")
        super().__init__(engine, x0, obstacle_specs, hist_cap, max_age, frame_window, "truncate", traffic_of, 0, record,
                         group_off=off, record_plans=record_plans, checkpoint_every=checkpoint_every, checkpoint_slots=checkpoint_slots)

    def _register_groups(self):
        """The groups and, every time, how their egos predict each other: a later loop on the same engine has its own mode."""
        eng, off = self.loop.eng, self.group_off
        _cabi.check(eng.lib.jsim_loop_set_groups(eng._ctx, eng.B, len(off) - 1, off.ctypes.data_as(C.c_void_p)), eng._ctx,
                    "jsim_loop_set_groups")
        _cabi.check(eng.lib.jsim_loop_set_mate_prediction(eng._ctx, _cabi.MATE_PREDICTION[self.mate_prediction]), eng._ctx,
                    "jsim_loop_set_mate_prediction")

    def pred_egos(self) -> torch.Tensor:
        """[B, n_steps, 3] (x, y, yaw): every ego's prediction from its current state, as the next tick will make it (under the
        loop's mate_prediction)."""
        eng = self.loop.eng
        pred = torch.zeros(eng.B, self.pre.n_steps, 3, dtype=torch.float64, device=eng.device)
        if self.mate_prediction == "plan":
            _cabi.check(eng.lib.jsim_loop_predict_egos_plan(eng._ctx, eng.B, _ptr(self.loop.x0), _ptr(eng.oa), _ptr(eng.od),
                                                            _ptr(eng.status), _ptr(eng.di_ai), self.pre.n_steps, _ptr(pred),
                                                            eng._stream()), eng._ctx, "jsim_loop_predict_egos_plan")
            return pred
        _cabi.check(eng.lib.jsim_loop_predict_egos(eng._ctx, eng.B, _ptr(self.loop.x0), _ptr(eng.di_ai), self.pre.n_steps,
                                                   _ptr(pred), eng._stream()), eng._ctx, "jsim_loop_predict_egos")
        return pred

    def tick(self):
        self.run(1)

    def fork(self, group=None, at=None, warm: bool = False, mate_prediction: Optional[str] = None, record: int = 0,
             max_age: Optional[int] = None, speed=None, config=None, ego_configs=None, record_plans: Optional[bool] = None,
             checkpoint_every: Optional[int] = None, checkpoint_slots: Optional[int] = None, **cold) -> "InteractingLoop":
        """A new InteractingLoop on a new engine whose rows are whole groups, continued from checkpoints: every
        ego of group group[r] goes on from the checkpoint at tick at[r] -- the mates' controllers as they were, so that the group's
        records are the source's from that tick on, bit for bit, until something is changed: mate_prediction (default: this
        loop's), speed (per ego of the new batch), max_age, config, ego_configs.  The groups lie contiguously in the new batch, in the
        rows' order; a group meets its traffic set's vehicles where they stood (rows of one source set and one tick share a set).
        record, record_plans (default: this loop's, with record), checkpoint_every, checkpoint_slots: the new loop's own.
        ValueError: without warm=True or on a loop without checkpoints -- a cold fork of a group is refused (section 22): the mates
        would have to go on with the controllers they had, and the recorder does not hold them; a group outside the loop's; a tick
        that is not checkpointed."""
        if not warm or self._ck is None or cold:
            raise ValueError("an InteractingLoop cannot be forked cold: the group mates' warm starts (oa, od) are not recorded, so their "
                             "controllers cannot be continued from a recorded tick; a loop with checkpoints (checkpoint_every=...) "
                             "forks whole groups from a checkpointed tick with warm=True")
        src, eng, off = self.loop, self.loop.eng, self.group_off
        group, at, _ = self._warm_rows(len(off) - 1, group, at)
        ego = np.concatenate([np.arange(off[g], off[g + 1]) for g in group]).astype(np.int32)
        sizes = np.diff(off)[group]
        slot = history.checkpoint_at(self._ck.slot_tick, np.repeat(at, sizes))
        idx, sl = (torch.from_numpy(v.astype(np.int64)).to(eng.device) for v in (ego, slot))
        new = self._fork_engine(idx, [p.copy() for p in eng.paths], eng.path_id[idx].cpu().numpy(), speed, False, eng.cv, config, ego_configs)
        keys, tof, veh, sets, shared = self._fork_traffic(self._source_sets()[off[group]], at)
        if record_plans is None:
            record_plans = bool(record) and self.recorder is not None and bool(self.recorder.glue.get("record_plans"))
        fork = InteractingLoop(new, self._ck.slabs["x0"][sl, idx].contiguous(), group_sizes=sizes, obstacle_specs=sets[0] if shared else sets,
                               hist_cap=src.hist_cap, max_age=src.max_age if max_age is None else max_age,
                               frame_window=self.pre.frame_window, traffic_of=None if shared else tof, record=record,
                               mate_prediction=self.mate_prediction if mate_prediction is None else mate_prediction,
                               record_plans=record_plans, checkpoint_every=checkpoint_every, checkpoint_slots=checkpoint_slots)
        self._load_warm(fork, ego, slot, keys, veh)
        return fork
