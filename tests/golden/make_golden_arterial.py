#!/usr/bin/env python3
"""Fixture for the arterial road of the overtaking study: the REFERENCE's envs/arterial_multi_lanes.py
(ArterialMultiLanes.create_scenario) built for several (num_lanes, goal_lane) pairs and for three replan situations
(moving_obstacles=True, is_following=False: the start at the AV, a box over the cyclist's predicted trajectory), written to
tests/golden/arterial.npz, data only: per scene the start, the goal point, the goal box, the angle tolerance and every obstacle's
constructor arguments (xy_width, xy_center, hidden); for the plain two-lane road and the replan situations also the route of the
reference's lib/mp_search_ww_generic.MotionPrimitiveSearch in planner_envs.npz's format (obstacle half-planes from the scenario
objects' own to_convex(margin = car radius) -> cost, node path, primitive sequence, trajectory, expansion count).

The reference file's one cvxpy import (`from cvxpy import length`, unused) is served by a placeholder module where cvxpy is absent.
The cyclist's prediction of a replan situation is the straight line its constant-speed prediction gives: 70 points 0.1 s apart at
5 km/h from its position.  The oracle's restatement is checked against every route right here.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_arterial.py"""
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("JSIM_REFERENCE") or os.path.join(os.path.dirname(REPO), "reference", "main")
os.environ["JSIM_REFERENCE"] = REF                                   # (make_golden_planner reads it too)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
os.environ.setdefault("MPLBACKEND", "Agg")

try:
    import cvxpy                                                     # noqa: F401
except Exception:
    stub = types.ModuleType("cvxpy")
    stub.length = None
    sys.modules["cvxpy"] = stub

from envs.arterial_multi_lanes import ArterialMultiLanes             # noqa: E402  (reference)
from lib.car_dimensions import BicycleModelDimensions                # noqa: E402
from lib.mp_search_ww_generic import MotionPrimitiveSearch           # noqa: E402

import planner_oracle as PO                                          # noqa: E402
from make_golden_planner import reference_primitives                 # noqa: E402

LANES = ((1, 1), (2, 1), (2, 2), (3, 2), (4, 4))
CYCLIST_V, PRED_DT, PRED_N = 5 / 3.6, 0.1, 70
# (cyclist x, y), (AV x, y)
REPLANS = (((2.0, -2.3), (2.0, -9.0)), ((2.0, 3.1), (2.05, -8.7)), ((1.8, -6.0), (1.95, -17.0)))


def prediction(x, y):
    return np.array([[x, y + CYCLIST_V * PRED_DT * k, np.pi / 2] for k in range(PRED_N)])


def main():
    car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    mps = reference_primitives(car)
    mine = PO.make_motion_primitives()
    out = {"radius": np.float64(car.radius), "circle_centers": np.array(car.circle_centers)}
    scenes = []
    for nl, gl in LANES:
        scenes.append((f"arterial/lanes{nl}/goal{gl}", nl, gl, None, ArterialMultiLanes(num_lanes=nl, goal_lane=gl).create_scenario(),
                       (nl, gl) == (2, 1)))
    for j, ((cx, cy), (ax, ay)) in enumerate(REPLANS):
        traj = prediction(cx, cy)
        sc = ArterialMultiLanes(num_lanes=2, goal_lane=1).create_scenario(
            moving_obstacles=True, moving_obstacles_trajectory=[traj], spawn_location_x=cx, spawn_location_y=cy, av_location_x=ax,
            av_location_y=ay, is_following=False)
        scenes.append((f"arterial/replan{j}", 2, 1, (traj, (cx, cy), (ax, ay)), sc, True))
    names, n_routes = [], 0
    for i, (label, nl, gl, rp, sc, route) in enumerate(scenes):
        ga = sc.goal_area
        box = (ga.xy1[0], ga.xy1[1], ga.xy2[0], ga.xy2[1])
        out[f"s{i}_lanes"] = np.array([nl, gl], dtype=np.int64)
        out[f"s{i}_start"] = np.array(sc.start, dtype=np.float64)
        out[f"s{i}_goal"] = np.array(sc.goal_point, dtype=np.float64)
        out[f"s{i}_goal_box"] = np.array(box, dtype=np.float64)
        out[f"s{i}_tol"] = np.float64(sc.allowed_goal_theta_difference)
        out[f"s{i}_obs"] = np.array([[o.xy_width[0], o.xy_width[1], o.xy_center[0], o.xy_center[1], float(o.hidden)] for o in sc.obstacles])
        out[f"s{i}_replan"] = np.int64(rp is not None)
        if rp is not None:
            out[f"s{i}_trajectory"], out[f"s{i}_spawn"], out[f"s{i}_av"] = rp[0], np.array(rp[1]), np.array(rp[2])
        out[f"s{i}_route"] = np.int64(n_routes if route else -1)
        names.append(label)
        if not route:
            print(f"scene {i} {label}: {len(sc.obstacles)} obstacles", flush=True)
            continue
        t0 = time.time()
        search = MotionPrimitiveSearch(sc, car, mps, margin=car.radius)
        cost, path, traj = search.run(debug=True)
        dt_ref = time.time() - t0
        pnames = [search._points_to_mp_names[a, b] for a, b in zip(path[:-1], path[1:])]
        hps = [np.asarray(h, dtype=np.float64) for h in search._obstacles_hp]
        orc = PO.PlannerOracle(sc.start, sc.goal_point, box, sc.allowed_goal_theta_difference, hps, mine, car.circle_centers, car.radius)
        c2, p2, t2 = orc.run(max_expansions=10 ** 7)
        assert c2 == cost and p2 == path and np.array_equal(t2, traj), label
        assert [PO.MP_NAMES[k] for k in orc.prim_sequence(p2)] == pnames and orc.n_expanded == len(search.debug_data), label
        r = n_routes
        out[f"r{r}_hp"] = np.concatenate(hps, axis=0)
        out[f"r{r}_hp_off"] = np.concatenate([[0], np.cumsum([len(h) for h in hps])]).astype(np.int64)
        out[f"r{r}_start"] = np.array(sc.start, dtype=np.float64)
        out[f"r{r}_goal"] = np.array(sc.goal_point, dtype=np.float64)
        out[f"r{r}_goal_box"] = np.array(box, dtype=np.float64)
        out[f"r{r}_tol"] = np.float64(sc.allowed_goal_theta_difference)
        out[f"r{r}_cost"] = np.float64(cost)
        out[f"r{r}_path"] = np.array(path, dtype=np.float64)
        out[f"r{r}_prims"] = np.array([PO.MP_NAMES.index(x) for x in pnames], dtype=np.int32)
        out[f"r{r}_traj"] = np.asarray(traj, dtype=np.float64)
        out[f"r{r}_n_expanded"] = np.int64(orc.n_expanded)
        out[f"r{r}_max_open"] = np.int64(orc.max_open)
        out[f"r{r}_scene"] = np.int64(i)
        n_routes += 1
        print(f"scene {i} {label}: route {r}: cost {cost:.3f}, {len(path)} nodes, {len(traj)} points, x from {np.min(traj[:, 0]):.2f} to "
              f"{np.max(traj[:, 0]):.2f}, {orc.n_expanded} expansions, reference {dt_ref:.1f} s", flush=True)
    out["n_scenes"] = np.int64(len(scenes))
    out["n_routes"] = np.int64(n_routes)
    out["labels"] = np.array(names)          # fixed-width unicode array: plain data, no pickling
    np.savez_compressed(os.path.join(HERE, "arterial.npz"), **out)


if __name__ == "__main__":
    main()
