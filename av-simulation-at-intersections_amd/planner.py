"""Route planner on the MI355X: the reference's A* over motion primitives
(main/lib/mp_search_ww_generic.py + main/lib/a_star.py) for a batch of route queries, one wavefront per route
(csrc/planner.inc behind `jsim_plan_routes` / `jsim_plan_routes_weighted`).  The (M, 3) [x, y, yaw] trajectories it returns are what `MPC(cx, cy, cyaw, ...)`
/ `BatchedMPC(paths, ...)` take -- exactly the hand-over of main/scenarios/mpc_intersection.py:63-76.

The motion primitives are regenerated from the reference's recipe (main/create_motion_primitives_bicycle_model.py:12-27:
explicit-Euler kinematic bicycle from the origin, 8.3 m/s, nine steering angles, 61 states 0.01 s apart -- 4.98 m, 0.083 m
between points); the reference's pickled primitives are never loaded.  Scenario geometry restates main/envs/intersection.py
and main/envs/intersection_multi_lanes.py (boxes and circles, turned into half-plane sets like Obstacle.to_convex).
There is no CPU fallback: without the HIP library / a HIP device `plan_routes` raises."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _cabi, _header

MP_NAMES = ("straight", "left1", "left2", "left3", "left4", "right1", "right2", "right3", "right4")
MP_STEER = (0.0, 0.1, 0.2, 0.3, 0.4, -0.1, -0.2, -0.3, -0.4)     # main/create_motion_primitives_prius.py:19-29
WH_DEFAULT = (1.0, 2.7, 15.0, 0.0, 0.0)                            # mp_search_ww_generic.py:29-31
WC_DEFAULT = (1.0, 5.0, 0.1, 0.0)                                  # :33
FORM_GENERIC, FORM_MULTI = 0, 1    # cost terms of main/lib/mp_search_ww_generic.py / main/planner/multi_trajectory_planner.py
# the kernel's tables (csrc/planner.inc JPL_MAX_OBS, JPL_MAX_HP, JPL_MAX_PRIM, JPL_MAX_CC): a route beyond them ends with status 5
MAX_OBSTACLES, MAX_HALFPLANES, MAX_PRIMITIVES, MAX_COLLISION_POINTS = 64, 512, 16, 16


def make_motion_primitives(L: float = 2.86, v: float = 8.3, n_steps: int = 60, dt: float = 0.01):
    """(points [9, 61, 3], total_length [9]) in MP_NAMES order: Bicycle.step (main/bicycle/main.py:28-41) from the origin, the
    state recorded before every step."""
    pts = np.zeros((len(MP_STEER), n_steps + 1, 3))
    for k, delta in enumerate(MP_STEER):
        x = y = th = 0.0
        for i in range(n_steps + 1):
            pts[k, i] = (x, y, th)
            xd = v * np.cos(th); yd = v * np.sin(th); thd = (v / L) * np.tan(delta)
            x += xd * dt; y += yd * dt; th += thd * dt
    length = np.array([np.linalg.norm(p[:-1, :2] - p[1:, :2], axis=1).sum() for p in pts])
    return pts, length


def car_circles(L: float = 2.86, width: float = 2.0, extra_length: float = 0.64):
    """(radius, circle centres [2, 2]) of BicycleModelDimensions (main/lib/car_dimensions.py:52-90)."""
    length = L + extra_length
    off = length / 2 - width / 2
    return width / (2 ** .5), np.array([[L / 2 + off, 0.0], [L / 2 - off, 0.0]])


def collision_points(mp_points: np.ndarray, circle_centers: np.ndarray, radius: float) -> np.ndarray:
    """_create_collision_points for one primitive (mp_search_ww_generic.py:118-136): resample_curve at dl = radius keeping the
    last point (main/lib/trajectories.py:58-86), then each collision circle's trajectory (:11-55); xy only."""
    step = np.append(0.0, np.linalg.norm(mp_points[1:, :2] - mp_points[:-1, :2], axis=1))
    k = np.floor(step.cumsum() / radius).astype(int)
    mask = np.append(True, (k[1:] - k[:-1]) >= 1.0)
    mask[-1] = True
    p = mp_points[mask]
    th = p[:, 2]
    out = [np.vstack([np.cos(th) * cx - np.sin(th) * cy, np.sin(th) * cx + np.cos(th) * cy]).T + p[:, :2] for cx, cy in circle_centers]
    return np.concatenate(out, axis=0)


def box_halfplanes(xy_width, xy_center, margin: float) -> np.ndarray:
    """BoxObstacle.to_convex (main/lib/obstacles.py:80-93)."""
    cx, cy = xy_center
    w, h = xy_width
    x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    return np.array([[1, 0, -(x2 + margin)], [-1, 0, x1 - margin], [0, 1, -(y2 + margin)], [0, -1, y1 - margin]], dtype=np.float64)


def circle_halfplanes(radius: float, xy_center, margin: float) -> np.ndarray:
    """CircleObstacle.to_convex (main/lib/obstacles.py:127-142): the octagon around the circle."""
    cx, cy = xy_center
    r = radius
    return np.array([[1, 0, -(cx + r + margin)], [-1, 0, cx - r - margin], [0, 1, -(cy + r + margin)], [0, -1, cy - r - margin],
                     [-1, 1, cx - cy - r * np.sqrt(2) - 2 * margin], [1, -1, -cx + cy - r * np.sqrt(2) - 2 * margin],
                     [-1, -1, cx + cy - r * np.sqrt(2) - 2 * margin], [1, 1, -cx - cy - r * np.sqrt(2) - 2 * margin]], dtype=np.float64)


@dataclass
class RouteQuery:
    start: Tuple[float, float, float]
    goal: Tuple[float, float, float]
    goal_box: Tuple[float, float, float, float]     # (x1, y1, x2, y2) of the goal area
    tol: float                                      # allowed_goal_theta_difference
    obstacles: List[np.ndarray]                     # half-plane sets [a, b, c], one array per obstacle (margin included)


def _intersection_scene(start_pos: int, turn_indicator: int, start_lane: int, goal_lane: int, number_of_lanes: int):
    """(start, goal, goal box, obstacle primitives) of the reference's intersection builders: what intersection_query and
    intersection_obstacles share."""
    pi = np.pi
    if number_of_lanes == 0:
        road, island, pav, length, corner = 4, 2, 5, 30, 6
        dc = corner + road + island
        lat = island / 2 + road / 2
        starts = {1: (lat, -30, 0.5 * pi), 2: (-30, -lat, 0), 3: (-lat, 30, -0.5 * pi), 4: (30, lat, pi)}
        g = (island + road) / 2
        gd = 30
        half_road = island / 2 + road
        corner_r = dc - island / 2 - road
        goal_w = (road * 1.8, road)
    else:
        lane_w, island, pav, length, corner = 4, 2, 5, 30, 6
        dc = corner + lane_w * number_of_lanes + island
        lat = island / 2 + (start_lane - 1) * lane_w + lane_w / 2
        starts = {1: (lat, -30, 0.5 * pi), 2: (-30, -lat, 0), 3: (-lat, 30, -0.5 * pi), 4: (30, lat, pi)}
        g = (island + lane_w) / 2 + (goal_lane - 1) * lane_w
        gd = 30
        half_road = island / 2 + number_of_lanes * lane_w
        corner_r = dc - island / 2 - number_of_lanes * lane_w
        goal_w = (lane_w * 1.8, 1.5)
    W, N_, E, S_ = (-gd, g, -pi), (g, gd, 0.5 * pi), (gd, -g, 0), (-g, -gd, -0.5 * pi)
    goals = {1: {1: W, 2: N_, 3: E}, 2: {1: N_, 2: E, 3: S_}, 3: {1: E, 2: S_, 3: W}, 4: {1: S_, 2: W, 3: N_}}
    start, goal = starts[start_pos], goals[start_pos][turn_indicator]
    if (start_pos in (1, 3) and turn_indicator in (1, 3)) or (start_pos in (2, 4) and turn_indicator in (2, 4)):
        gw = goal_w
    else:
        gw = (goal_w[1], goal_w[0])
    gb = (goal[0] - gw[0] / 2, goal[1] - gw[1] / 2, goal[0] + gw[0] / 2, goal[1] + gw[1] / 2)
    far = length / 2 + dc
    side = half_road + pav / 2
    obs = [
        ("box", (island, length), (0, -far), False), ("circle", island / 2, (0, -dc), False),          # south median
        ("box", (island, length), (0, far), False), ("circle", island / 2, (0, dc), False),            # north median
        ("box", (length, island), (-far, 0), False), ("circle", island / 2, (-dc, 0), False),          # west median
        ("box", (length, island), (far, 0), False), ("circle", island / 2, (dc, 0), False),            # east median
        ("circle", corner_r, (-dc, -dc), False), ("circle", corner_r, (-dc, dc), False),                # corners
        ("circle", corner_r, (dc, dc), False), ("circle", corner_r, (dc, -dc), False),
        ("box", (pav, length), (-side, -far), False), ("box", (pav, length), (side, -far), False),       # pavements: south
        ("box", (length, pav), (-far, -side), False), ("box", (length, pav), (-far, side), False),       # west
        ("box", (pav, length), (-side, far), False), ("box", (pav, length), (side, far), False),         # north
        ("box", (length, pav), (far, -side), False), ("box", (length, pav), (far, side), False),         # east
    ]
    # the hidden boxes that close the oncoming lanes of the four arms (envs/intersection.py:150-208, intersection_multi_lanes.py
    # :183-213): lateral sign per (start_pos, arm W / E / S / N); the multi-lane file's east box for start_pos 4 is centred with
    # lane_width instead of number_of_lanes * lane_width (kept as written)
    road_total = road if number_of_lanes == 0 else number_of_lanes * lane_w
    gl_ = (road_total + island) / 2
    sign = {1: (-1, 1, -1, -1), 2: (1, 1, 1, -1), 3: (-1, 1, 1, 1), 4: (-1, -1, 1, -1)}[start_pos]
    ge = (lane_w + island) / 2 if (number_of_lanes and start_pos == 4) else gl_
    obs += [("box", (length, road_total), (-far, sign[0] * gl_), True), ("box", (length, road_total), (far, sign[1] * ge), True),
            ("box", (road_total, length), (sign[2] * gl_, -far), True), ("box", (road_total, length), (sign[3] * gl_, far), True)]
    return start, goal, gb, obs


def intersection_obstacles(start_pos: int, turn_indicator: int, start_lane: int = 1, goal_lane: int = 1,
                           number_of_lanes: int = 0) -> list:
    """The obstacles list of the reference's intersection scenarios (intersection_query's, in list order) as primitives:
    ("box", xy_width, xy_center, hidden) and ("circle", radius, xy_center, hidden), the arguments of BoxObstacle / CircleObstacle
    (main/lib/obstacles.py).  The last four are the hidden boxes that close the oncoming lanes.  static_obstacle_rows takes them."""
    return _intersection_scene(start_pos, turn_indicator, start_lane, goal_lane, number_of_lanes)[3]


def primitive_halfplanes(obstacle, margin: float) -> np.ndarray:
    """to_convex(margin) of one ("box", ...) / ("circle", ...) primitive."""
    kind, size, centre = obstacle[:3]
    if kind == "box":
        return box_halfplanes(size, centre, margin)
    if kind == "circle":
        return circle_halfplanes(size, centre, margin)
    raise ValueError(f"an obstacle primitive is ('box', xy_width, xy_center[, hidden]) or ('circle', radius, xy_center[, hidden]), got {obstacle!r}")


def intersection_query(start_pos: int, turn_indicator: int, margin: float, start_lane: int = 1, goal_lane: int = 1,
                       number_of_lanes: int = 0) -> RouteQuery:
    """The reference's scenarios as a route query: number_of_lanes = 0 -> main/envs/intersection.py:10-160 (one lane per
    direction, 4 m road, 2 m island, corner radius 6); number_of_lanes >= 1 -> main/envs/intersection_multi_lanes.py:9-170
    (lane_width 4, median 2, as mpc_intersection_multi_lane.py builds it with number_of_lanes = 2)."""
    start, goal, gb, prims = _intersection_scene(start_pos, turn_indicator, start_lane, goal_lane, number_of_lanes)
    return RouteQuery(start=tuple(float(v) for v in start), goal=tuple(float(v) for v in goal), goal_box=tuple(float(v) for v in gb),
                      tol=float(np.pi / 16), obstacles=[primitive_halfplanes(o, margin) for o in prims])


def _arterial_scene(num_lanes: int, goal_lane: int, replan, width_road: float, length: float, x_goal: float, y_goal: float,
                    width_pavement: float, car_L: float, car_width: float, car_extra_length: float, cyclist_box_width: float):
    """(start, goal, goal box, obstacle primitives) of the reference's arterial road: what arterial_query and arterial_obstacles
    share.  A straight road along y of num_lanes lanes centred on x = 0, a pavement on either side; the ego starts in the middle of
    the lane right of the centre at the road's lower end and the goal is a point, with a box of the car's bounding box around it."""
    if num_lanes < 1:
        raise ValueError("the road needs at least one lane")
    if goal_lane > num_lanes:
        raise ValueError(f"goal lane {goal_lane} of {num_lanes} lanes")
    half = num_lanes * width_road / 2
    start = (width_road * (num_lanes / 2 - 0.5), -length / 2, np.pi / 2)
    goal = (x_goal, y_goal, np.pi / 2)
    gw = (car_width, car_L + car_extra_length)
    gb = (goal[0] - gw[0] / 2, goal[1] - gw[1] / 2, goal[0] + gw[0] / 2, goal[1] + gw[1] / 2)
    obs = [("box", (width_pavement, length), (-half - width_pavement / 2, 0), False),                    # left pavement
           ("box", (width_pavement, length), (half + width_pavement / 2, 0), False)]                     # right pavement
    if replan is None:
        obs.append(("box", (width_road, length), (-start[0], 0), False))                                 # the closed left road
    else:
        # the replan at the trigger: from where the AV stands, the left road open, and one box over the cyclist and everywhere its
        # prediction takes it -- as long as the prediction's extent in y, laid from the cyclist's position onwards
        traj = np.asarray(replan["trajectory"], dtype=np.float64)
        if traj.ndim != 2 or traj.shape[0] < 1 or traj.shape[1] < 2:
            raise ValueError("replan['trajectory'] is the cyclist's predicted trajectory [n][>= 2] (x, y, ...)")
        (sx, sy), (ax, ay) = replan["spawn"], replan["av"]
        reach = traj[-1][1] - traj[0][1]
        start = (ax, ay, np.pi / 2)
        obs.append(("box", (cyclist_box_width, reach), (sx, sy + reach / 2), False))
    return start, goal, gb, obs


_ARTERIAL = dict(width_road=4.0, length=44.0, x_goal=2.0, y_goal=22.0, width_pavement=3, car_L=2.86, car_width=2.0,
                 car_extra_length=0.64, cyclist_box_width=1.64)


def arterial_obstacles(num_lanes: int = 2, goal_lane: int = 1, replan=None, **constants) -> list:
    """The obstacles list of the reference's arterial road (arterial_query's, in list order) as primitives ("box", xy_width,
    xy_center, hidden): the two pavements and the closed left road, or with replan= the two pavements and the cyclist's box.
    static_obstacle_rows takes them."""
    return _arterial_scene(num_lanes, goal_lane, replan, **{**_ARTERIAL, **constants})[3]


def arterial_query(margin: float, num_lanes: int = 2, goal_lane: int = 1, replan=None, **constants) -> RouteQuery:
    """main/envs/arterial_multi_lanes.py's ArterialMultiLanes(num_lanes, goal_lane).create_scenario as a route query: the road of
    the overtaking study (main/scenarios/overtaking_cyclist_bidirectional_road.py:1978-1979).  replan=dict(trajectory=the cyclist's
    predicted trajectory [n][>= 2], spawn=(x, y) of the cyclist, av=(x, y) of the ego) is the form perform_replan asks for
    (:318-326, is_following=False): the start moved to the ego, the left road open, a box 1.64 m wide over the cyclist's prediction.
    constants: lib/parameters.py's ScenarioParameters and the shapes, by keyword -- width_road (WIDTH_ROAD, 4.0), length (LENGTH,
    44.0), x_goal (X_LOC_EGO, 2.0), y_goal (Y_LOC_GOAL, 22.0), width_pavement (3), car_L / car_width / car_extra_length (the goal
    box: BicycleModelDimensions' bounding box), cyclist_box_width (1.64).  ValueError: no lane, a goal lane beyond the lanes."""
    start, goal, gb, prims = _arterial_scene(num_lanes, goal_lane, replan, **{**_ARTERIAL, **constants})
    return RouteQuery(start=tuple(float(v) for v in start), goal=tuple(float(v) for v in goal), goal_box=tuple(float(v) for v in gb),
                      tol=float(np.pi / 16), obstacles=[primitive_halfplanes(o, margin) for o in prims])


STATIC_ROW = _header.constant("JSIM_STATIC_ROW")   # doubles per obstacle row of jsim_loop_eval_static


def static_obstacle_rows(obstacles, margin: float) -> np.ndarray:
    """[n][32] rows of jsim_loop_eval_static for one obstacle list: 0 kind (0 box, 1 circle), 1 hidden,
    2 n_hp, 3-6 geometry (box: x1, y1, x2, y2 as BoxObstacle.__init__ computes xy1 / xy2; circle: cx, cy, r, 0), 8-31 the half-planes
    of to_convex(margin) in the reference's row order.  An obstacle is one of the reference's objects, duck-typed (.xy1 / .xy2 or
    .radius / .xy_center, .hidden, its own .to_convex(margin)), or a primitive ("box", xy_width, xy_center[, hidden]) /
    ("circle", radius, xy_center[, hidden]).  ValueError: anything else, a margin that is not finite and >= 0, more than eight
    half-planes."""
    margin = float(margin)
    if not (math.isfinite(margin) and margin >= 0.0):
        raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
    obstacles = list(obstacles)
    rows = np.zeros((len(obstacles), STATIC_ROW))
    for r, o in zip(rows, obstacles):
        if isinstance(o, (tuple, list)):
            hp = primitive_halfplanes(o, margin)
            hidden = bool(o[3]) if len(o) > 3 else False
            if o[0] == "box":
                (w, h), (cx, cy) = o[1], o[2]
                kind, geom = 0, (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
            else:
                kind, geom = 1, (o[2][0], o[2][1], o[1], 0.0)
        elif hasattr(o, "xy1") and hasattr(o, "xy2"):
            kind, geom, hidden, hp = 0, (*o.xy1, *o.xy2), bool(o.hidden), o.to_convex(margin)
        elif hasattr(o, "radius") and hasattr(o, "xy_center"):
            kind, geom, hidden, hp = 1, (*o.xy_center, o.radius, 0.0), bool(o.hidden), o.to_convex(margin)
        else:
            raise ValueError(f"not a box (.xy1 / .xy2), a circle (.radius / .xy_center) or a primitive tuple: {o!r}")
        hp = np.asarray(hp, dtype=np.float64)
        if hp.ndim != 2 or hp.shape[1] != 3 or not 1 <= hp.shape[0] <= 8:
            raise ValueError(f"to_convex(margin) must give 1..8 half-planes [a, b, c], got shape {hp.shape}")
        r[0], r[1], r[2], r[3:7] = kind, hidden, hp.shape[0], geom
        r[8:8 + 3 * hp.shape[0]] = hp.reshape(-1)
    return rows


def scenario_obstacles(scenario) -> list:
    """The obstacles list of a reference Scenario (main/lib/scenario.py), in list order: what static_obstacle_rows and
    Recorder.static_conflicts take as one set."""
    return list(scenario.obstacles)


@dataclass
class PlannedRoute:
    status: int
    cost: float
    prims: np.ndarray          # primitive index per segment (into MP_NAMES)
    nodes: np.ndarray          # (n_prims + 1, 3) poses of the path
    trajectory: np.ndarray     # (n_prims * 60, 3) [x, y, yaw]: what MPC(cx, cy, cyaw) takes
    n_expanded: int


def weight_tables(n_routes: int, wh=WH_DEFAULT, wc=WC_DEFAULT, form=FORM_GENERIC):
    """(wh [R, 5], wc [R, 4], form [R] int32) from one row each (repeated for every route) or R rows each; raises ValueError for
    any other shape, a form outside {0, 1} or a weight that is not finite.  No device is touched."""
    R = int(n_routes)

    def table(a, width, name):
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (width,):
            a = np.broadcast_to(a, (R, width))
        if a.shape != (R, width):
            raise ValueError(f"{name} must have shape ({width},) or ({R}, {width}) for {R} routes, got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name} must be finite")
        return np.ascontiguousarray(a)

    f = np.asarray(form)
    if f.dtype.kind not in "iub" or f.shape not in ((), (R,)):
        raise ValueError(f"form must be an integer or {R} integers (one per route), got {f.dtype} {f.shape}")
    f = np.ascontiguousarray(np.broadcast_to(f.astype(np.int32), (R,)))
    if not np.all((f == FORM_GENERIC) | (f == FORM_MULTI)):
        raise ValueError(f"form must be {FORM_GENERIC} (mp_search_ww_generic) or {FORM_MULTI} (multi_trajectory_planner)")
    return table(wh, 5, "wh"), table(wc, 4, "wc"), f


def plan_routes(queries: Sequence[RouteQuery], L: float = 2.86, wh=WH_DEFAULT, wc=WC_DEFAULT, max_path: int = 32,
                device: int = 0, primitives=None, node_cap: int = 1 << 17, retry_node_cap: int = 1 << 21, circles=None,
                form=FORM_GENERIC) -> List[PlannedRoute]:
    """All queries in ONE launch (one wavefront per route).  wh (5,), wc (4,) and form hold for every route; given as (R, 5),
    (R, 4) and (R,) they are per route -- a weight sweep is the same query R times with one row each.  form 0: the cost terms of
    mp_search_ww_generic.py, 1: those of multi_trajectory_planner.py (wh[:3] = e, p, o).  Routes whose search outgrows `node_cap`
    nodes (status 4) are planned again, together, each with its own rows, with `retry_node_cap` (0: no second attempt).
    primitives = (points [P, n, 3], total_length [P]) and circles = (radius, centres [k, 2]) replace the regenerated
    bicycle-model set / BicycleModelDimensions' circles."""
    wh, wc, form = weight_tables(len(queries), wh, wc, form)
    out = _plan(queries, L, wh, wc, form, max_path, device, primitives, node_cap, circles)
    again = [i for i, r in enumerate(out) if r.status == 4]
    if again and retry_node_cap > node_cap:
        for i, r in zip(again, _plan([queries[i] for i in again], L, wh[again], wc[again], form[again], max_path, device, primitives,
                                     retry_node_cap, circles)):
            out[i] = r
    return out


class MotionPrimitiveSearch:
    """Drop-in for the reference's planner class (main/lib/mp_search_ww_generic.py:26-58 constructor, :136-140 run): the same
    arguments -- a scenario (.start, .goal_point, .goal_area with .xy1 / .xy2, .allowed_goal_theta_difference, .obstacles whose
    .to_convex(margin) gives half-planes), car dimensions (.radius, .circle_centers), the motion primitives the CALLER holds (a
    dict name -> object with .points (n, 3) and .total_length; iteration order = expansion order, as in the reference) and the
    nine weights -- and run() -> (cost, path, trajectory) with path a list of (x, y, theta) tuples.  The search itself is
    plan_astar_kernel on the GPU (one route = one wavefront; use plan_routes for many routes at once).  Like the reference,
    run() raises Exception("No solution found.") when the open list runs empty (main/lib/a_star.py:78); debug=True (the
    reference's matplotlib trace of the expansion) is not offered."""

    def __init__(self, scenario, car_dimensions, mps, margin: float,
                 wh_dist: float = 1.0, wh_theta: float = 2.7, wh_steering: float = 15.0, wh_obstacle: float = 0.0, wh_center: float = 0.0,
                 wc_dist: float = 1.0, wc_steering: float = 5.0, wc_obstacle: float = 0.1, wc_center: float = 0.0, device: int = 0,
                 max_path: int = 32, node_cap: int = 1 << 17, retry_node_cap: int = 1 << 21):
        # max_path: longest path in primitives the output arrays hold (status 6 beyond); node_cap / retry_node_cap: node table of
        # the first / second attempt (status 4 beyond) -- the reference's dict and heap grow without bound, these do not
        self.max_path, self.node_cap, self.retry_node_cap = int(max_path), int(node_cap), int(retry_node_cap)
        self._names, self._primitives, self._circles = _scenario_primitives(mps, car_dimensions)
        self._query = _scenario_query(scenario, margin)
        self._wh = (wh_dist, wh_theta, wh_steering, wh_obstacle, wh_center)
        self._wc = (wc_dist, wc_steering, wc_obstacle, wc_center)
        self._device = device
        self._points_to_mp_names = {}
        self.last = None       # the PlannedRoute of the last run (status, primitive indices, expansion count)

    def run(self, debug: bool = False):
        if debug:
            raise NotImplementedError("debug=True (the reference's expansion trace) is not offered by the GPU planner")
        r = plan_routes([self._query], wh=self._wh, wc=self._wc, primitives=self._primitives, circles=self._circles, device=self._device,
                        max_path=self.max_path, node_cap=self.node_cap, retry_node_cap=self.retry_node_cap)[0]
        self.last = r
        _raise_unless_found(r, self.max_path)
        path = [tuple(float(v) for v in n) for n in r.nodes]
        for a, b, k in zip(path[:-1], path[1:], r.prims):
            self._points_to_mp_names[a, b] = self._names[int(k)]
        return r.cost, path, r.trajectory


def _scenario_query(scenario, margin: float) -> RouteQuery:
    ga = scenario.goal_area
    if not (hasattr(ga, "xy1") and hasattr(ga, "xy2")):
        # the reference accepts any Obstacle with distance_to_point as goal area (main/lib/mp_search_ww_generic.py:101-103); every
        # scenario builder it ships uses a BoxObstacle, and the kernel's goal test is the box test
        raise ValueError(f"goal_area must be a box (.xy1 / .xy2), got {type(ga).__name__}: the GPU planner's goal test is the "
                         "reference's BoxObstacle.distance_to_point(...) <= 0")
    (x1, y1), (x2, y2) = ga.xy1, ga.xy2
    return RouteQuery(start=tuple(float(v) for v in scenario.start), goal=tuple(float(v) for v in scenario.goal_point),
                      goal_box=(float(x1), float(y1), float(x2), float(y2)), tol=float(scenario.allowed_goal_theta_difference),
                      obstacles=[np.asarray(o.to_convex(margin=margin), dtype=np.float64) for o in scenario.obstacles])


def _scenario_primitives(mps, car_dimensions):
    names = list(mps.keys())
    pts = [np.asarray(mps[n].points, dtype=np.float64) for n in names]
    if not pts or any(p.shape != pts[0].shape or p.ndim != 2 or p.shape[1] != 3 for p in pts):
        raise ValueError("motion primitives must be (n, 3) arrays of one common length")
    return (names, (np.stack(pts), np.array([float(mps[n].total_length) for n in names])),
            (float(car_dimensions.radius), np.asarray(car_dimensions.circle_centers, dtype=np.float64).reshape(-1, 2)))


def _raise_unless_found(r: PlannedRoute, max_path: int) -> None:
    if r.status == 1:
        raise Exception("No solution found.")                        # main/lib/a_star.py:78
    if r.status == 5:
        raise RuntimeError(f"route planner: status 5 -- the obstacle / primitive set is larger than the kernel's tables: at most "
                           f"{MAX_OBSTACLES} obstacles and {MAX_HALFPLANES} half-planes per route, {MAX_PRIMITIVES} primitives, "
                           f"{MAX_COLLISION_POINTS} collision points per primitive (for every car circle, one per circle radius of the "
                           "primitive's length and two more: a small vehicle's circles on a 5 m primitive exceed it).  max_path "
                           "has no part in it")
    if r.status != 0:
        raise RuntimeError(f"route planner: status {r.status} (4: node table full -- raise node_cap / retry_node_cap; 6: path "
                           f"longer than max_path = {max_path} primitives)")


class MultiTrajectorySearch:
    """Drop-in for the reference's multi-trajectory planner class (main/planner/multi_trajectory_planner.py:44-269, the class
    main/scenarios/overtaking_cyclist_bidirectional_road.py:337 calls run_all of): the same constructor -- scenario, car
    dimensions, the caller's motion primitives, margin, the heuristic's weights as three LISTS wh_ego / wh_policy / wh_other and
    the four edge-cost weights -- with
      run()      one search with the sums of the lists (:94-96, :228-240) -> (cost, path, trajectory);
      run_all()  one search per (e, p, o), e over wh_ego, p over wh_policy, o over wh_other in that nesting (:253-267) ->
                 [(cost, path, trajectory, e, p, o), ...] -- ALL of them in ONE launch of jsim_plan_routes_weighted (form 1: one
                 wavefront per combination).  An empty list gives [] and the reference's message (:249-251).
    Like the reference's loop, run_all() raises Exception("No solution found.") at the first combination, in its order, whose
    open list runs empty.  debug=True (the expansion trace) is not offered."""

    def __init__(self, scenario, car_dimensions, mps, margin: float, wh_ego=None, wh_policy=None, wh_other=None,
                 wc_dist: float = 1.0, wc_steering: float = 5.0, wc_obstacle: float = 0.1, wc_center: float = 0.0, device: int = 0,
                 max_path: int = 32, node_cap: int = 1 << 17, retry_node_cap: int = 1 << 21):
        self.max_path, self.node_cap, self.retry_node_cap = int(max_path), int(node_cap), int(retry_node_cap)
        self._names, self._primitives, self._circles = _scenario_primitives(mps, car_dimensions)
        self._query = _scenario_query(scenario, margin)
        self._wh_ego = wh_ego if wh_ego is not None else []
        self._wh_policy = wh_policy if wh_policy is not None else []
        self._wh_other = wh_other if wh_other is not None else []
        self._sum_ego, self._sum_policy, self._sum_other = sum(self._wh_ego), sum(self._wh_policy), sum(self._wh_other)
        self._wc = (wc_dist, wc_steering, wc_obstacle, wc_center)
        self._device = device
        self._points_to_mp_names = {}
        self.last = None       # the PlannedRoutes of the last run / run_all

    def combinations(self):
        """[(e, p, o), ...] in the reference's loop order (:253-255)."""
        return [(e, p, o) for e in self._wh_ego for p in self._wh_policy for o in self._wh_other]

    def _search(self, combos):
        wh = np.array([[e, p, o, 0.0, 0.0] for e, p, o in combos], dtype=np.float64).reshape(len(combos), 5)
        routes = plan_routes([self._query] * len(combos), wh=wh, wc=self._wc, form=FORM_MULTI, primitives=self._primitives,
                             circles=self._circles, device=self._device, max_path=self.max_path, node_cap=self.node_cap,
                             retry_node_cap=self.retry_node_cap)
        self.last = routes
        out = []
        for r in routes:
            _raise_unless_found(r, self.max_path)
            path = [tuple(float(v) for v in n) for n in r.nodes]
            for a, b, k in zip(path[:-1], path[1:], r.prims):
                self._points_to_mp_names[a, b] = self._names[int(k)]
            out.append((r.cost, path, r.trajectory))
        return out

    def run(self, debug: bool = False):
        if debug:
            raise NotImplementedError("debug=True (the reference's expansion trace) is not offered by the GPU planner")
        return self._search([(self._sum_ego, self._sum_policy, self._sum_other)])[0]

    def run_all(self, debug: bool = False):
        if debug:
            raise NotImplementedError("debug=True (the reference's expansion trace) is not offered by the GPU planner")
        if not self._wh_ego or not self._wh_policy or not self._wh_other:
            print("One or more weight lists are empty; no solutions returned.")
            return []
        combos = self.combinations()
        return [(c, path, traj, e, p, o) for (c, path, traj), (e, p, o) in zip(self._search(combos), combos)]


def _plan(queries, L, wh, wc, form, max_path, device, primitives, node_cap, circles=None, launch_wide: bool = False) -> List[PlannedRoute]:
    """One launch.  launch_wide: through jsim_plan_routes with row 0 for every route (tools/bench_planner_sweep.py times it)."""
    lib = _cabi.load()
    pts, length = primitives if primitives is not None else make_motion_primitives(L=L)
    radius, centres = circles if circles is not None else car_circles(L=L)
    cc = [collision_points(p, centres, radius) for p in pts]
    cc_off = np.concatenate([[0], np.cumsum([len(c) for c in cc])]).astype(np.int32)
    cc_flat = np.ascontiguousarray(np.concatenate(cc, axis=0), dtype=np.float64)
    R = len(queries)
    hp_list, hp_off, r_off = [], [0], [0]
    for q in queries:
        for o in q.obstacles:
            o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
            hp_list.append(o)
            hp_off.append(hp_off[-1] + len(o))
        r_off.append(len(hp_off) - 1)
    hp = np.ascontiguousarray(np.concatenate(hp_list, axis=0) if hp_list else np.zeros((0, 3)), dtype=np.float64)
    hp_off = np.array(hp_off, dtype=np.int32); r_off = np.array(r_off, dtype=np.int32)
    start = np.ascontiguousarray([q.start for q in queries], dtype=np.float64).reshape(R, 3)
    goal = np.ascontiguousarray([q.goal for q in queries], dtype=np.float64).reshape(R, 3)
    box = np.ascontiguousarray([q.goal_box for q in queries], dtype=np.float64).reshape(R, 4)
    tol = np.ascontiguousarray([q.tol for q in queries], dtype=np.float64)
    mp = np.ascontiguousarray(pts, dtype=np.float64); ml = np.ascontiguousarray(length, dtype=np.float64)
    whv = np.ascontiguousarray(wh, dtype=np.float64); wcv = np.ascontiguousarray(wc, dtype=np.float64)
    formv = np.ascontiguousarray(form, dtype=np.int32)
    assert whv.shape == (R, 5) and wcv.shape == (R, 4) and formv.shape == (R,)
    n_prim, n_pts = mp.shape[0], mp.shape[1]
    seg = n_pts - 1
    status = np.zeros(R, dtype=np.int32); cost = np.zeros(R); n_prims = np.zeros(R, dtype=np.int32)
    prims = np.zeros((R, max_path), dtype=np.int32); nodes = np.zeros((R, max_path + 1, 3)); traj = np.zeros((R, max_path * seg, 3))
    n_exp = np.zeros(R, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    if launch_wide:
        _cabi.check(lib.jsim_plan_routes(int(device), R, p(start), p(goal), p(box), p(tol), p(hp), p(hp_off), len(hp_off) - 1, p(r_off), p(mp),
                                         p(ml), n_prim, n_pts, p(cc_flat), p(cc_off), p(whv), p(wcv), int(max_path), int(node_cap), p(status),
                                         p(cost), p(n_prims), p(prims), p(nodes), p(traj), p(n_exp)), None, "jsim_plan_routes")
    else:
        _cabi.check(lib.jsim_plan_routes_weighted(int(device), R, p(start), p(goal), p(box), p(tol), p(hp), p(hp_off), len(hp_off) - 1, p(r_off),
                                                  p(mp), p(ml), n_prim, n_pts, p(cc_flat), p(cc_off), p(whv), p(wcv), p(formv), int(max_path),
                                                  int(node_cap), p(status), p(cost), p(n_prims), p(prims), p(nodes), p(traj), p(n_exp)),
                    None, "jsim_plan_routes_weighted")
    out = []
    for i in range(R):
        k = int(n_prims[i])
        out.append(PlannedRoute(status=int(status[i]), cost=float(cost[i]), prims=prims[i, :k].copy(), nodes=nodes[i, :k + 1].copy(),
                                trajectory=traj[i, :k * seg].copy(), n_expanded=int(n_exp[i])))
    return out
