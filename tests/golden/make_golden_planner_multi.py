#!/usr/bin/env python3
"""G1 fixture for the multi-trajectory planner (the kernel's form 1): the REFERENCE's own class -- MotionPrimitiveSearch of
main/planner/multi_trajectory_planner.py:44-269, everything from :275 on sits under __main__, so the file imports cleanly -- run
here with run_all() on its own scenarios and written to tests/golden/planner_multi.npz, data only: per scenario the obstacle
half-planes (margin = car_dimensions.radius, as the script passes), start, goal point, goal box, angle tolerance and the four
edge-cost weights; per (e, p, o) of wh_ego x wh_policy x wh_other, in run_all's loop order, the weights, cost, path nodes,
primitive sequence, trajectory and expansion count.

CORRECTION: the copy of that class in main/lib/multi_trajectory_generator.py is NOT used -- it calls
AStar.run(start_node=...), a keyword main/lib/a_star.py:31 does not accept, so it cannot run; the planner/ file passes the start
positionally and is the one that works.

The scenarios and weight lists:
  s0  two-lane intersection (envs/intersection_multi_lanes.py, number_of_lanes = 2), start_pos 1, turn 2, lane 1 -> 2 with the
      script's own lists (:304-306) wh_ego = [1.0, 1.5, 10.0], wh_policy = [2.7], wh_other = [15]: three different primitive sequences
  s1  the same lists on the two-lane left turn (turn 1, lane 1 -> 1): three different sequences
  s2  single-lane intersection (envs/intersection.py), start_pos 1, turn 1, the 2 x 2 x 2 grid wh_ego = [1.0, 3.0],
      wh_policy = [2.7, 0.5], wh_other = [15, 2]: six different sequences among the eight
The reference's A* has no expansion cap; every candidate was screened first with the capped numpy restatement
(tests/planner_multi_numpy.py) and only combinations that stay under EXPANSION_CAP = 2000 expansions (<= 18001 nodes, far below
the planner's first-attempt node_cap of 131072) are kept -- all of the above do (463 at most); the assertion below holds it.
The restatement is checked against every combination right here: identical cost, node tuples, primitive sequence, expansion
count, bit-identical trajectory.

The motion primitives are regenerated with make_golden_planner.reference_primitives (the pickles are never loaded).

usage (needs the reference checkout; from the repo root):  python tests/golden/make_golden_planner_multi.py"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden_planner as G                                     # noqa: E402  (puts oracle/ and the reference on sys.path)
from planner_multi_numpy import MultiTrajectoryOracle               # noqa: E402
import planner_oracle as PO                                         # noqa: E402

EXPANSION_CAP = 2000
LISTS_SCRIPT = ([1.0, 1.5, 10.0], [2.7], [15])                       # multi_trajectory_planner.py:304-306
LISTS_GRID = ([1.0, 3.0], [2.7, 0.5], [15, 2])
WC = (1.0, 5.0, 0.1, 0.0)                                            # :307-310


def reference_class():
    spec = importlib.util.spec_from_file_location("ref_multi_trajectory_planner", os.path.join(G.REF, "planner", "multi_trajectory_planner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MotionPrimitiveSearch


def main():
    Search = reference_class()
    car = G.BicycleModelDimensions(skip_back_circle_collision_checking=False)
    mps = G.reference_primitives(car)
    mine = PO.make_motion_primitives()
    scen = [("two-lane straight 1->2", G.intersection_ml(start_pos=1, turn_indicator=2, start_lane=1, goal_lane=2, number_of_lanes=2), LISTS_SCRIPT),
            ("two-lane left 1->1", G.intersection_ml(start_pos=1, turn_indicator=1, start_lane=1, goal_lane=1, number_of_lanes=2), LISTS_SCRIPT),
            ("single-lane left", G.intersection(start_pos=1, turn_indicator=1), LISTS_GRID)]
    out = {"n_scenarios": np.int64(len(scen)), "mp_points": np.array([mps[n].points for n in PO.MP_NAMES]),
           "mp_length": np.array([mps[n].total_length for n in PO.MP_NAMES]), "radius": np.float64(car.radius),
           "circle_centers": np.array(car.circle_centers), "expansion_cap": np.int64(EXPANSION_CAP)}
    for i, (label, sc, (we, wp, wo)) in enumerate(scen):
        search = Search(sc, car, mps, margin=car.radius, wh_ego=we, wh_policy=wp, wh_other=wo,
                        wc_dist=WC[0], wc_steering=WC[1], wc_obstacle=WC[2], wc_center=WC[3])
        # is_goal is called once per expansion (a_star.py:57) and returns True once per search: the count per combination
        counts, n = [], [0]
        is_goal = search.is_goal

        def counting(node):
            n[0] += 1
            hit = is_goal(node)
            if hit:
                counts.append(n[0]); n[0] = 0
            return hit
        search.is_goal = counting
        sols = search.run_all()
        assert len(sols) == len(we) * len(wp) * len(wo) == len(counts)
        hps = [np.asarray(h, dtype=np.float64) for h in search._obstacles_hp]
        ga = sc.goal_area
        box = (ga.xy1[0], ga.xy1[1], ga.xy2[0], ga.xy2[1])
        out[f"s{i}_hp"] = np.concatenate(hps, axis=0)
        out[f"s{i}_hp_off"] = np.concatenate([[0], np.cumsum([len(h) for h in hps])]).astype(np.int64)
        out[f"s{i}_start"] = np.array(sc.start, dtype=np.float64)
        out[f"s{i}_goal"] = np.array(sc.goal_point, dtype=np.float64)
        out[f"s{i}_goal_box"] = np.array(box, dtype=np.float64)
        out[f"s{i}_tol"] = np.float64(sc.allowed_goal_theta_difference)
        out[f"s{i}_wc"] = np.array(WC, dtype=np.float64)
        out[f"s{i}_wh_ego"] = np.array(we, dtype=np.float64)
        out[f"s{i}_wh_policy"] = np.array(wp, dtype=np.float64)
        out[f"s{i}_wh_other"] = np.array(wo, dtype=np.float64)
        out[f"s{i}_n_comb"] = np.int64(len(sols))
        seqs = set()
        for j, ((cost, path, traj, e, p, o), n_exp) in enumerate(zip(sols, counts)):
            assert n_exp <= EXPANSION_CAP, (label, e, p, o, n_exp)
            names = [search._points_to_mp_names[a, b] for a, b in zip(path[:-1], path[1:])]
            orc = MultiTrajectoryOracle(sc.start, sc.goal_point, box, sc.allowed_goal_theta_difference, hps, mine, car.circle_centers, car.radius,
                                        wh=(e, p, o, 0.0, 0.0), wc=WC)
            c2, p2, t2 = orc.run(max_expansions=EXPANSION_CAP)
            assert c2 == cost and p2 == path and np.array_equal(t2, traj), (label, e, p, o)
            assert [PO.MP_NAMES[k] for k in orc.prim_sequence(p2)] == names and orc.n_expanded == n_exp
            out[f"s{i}_c{j}_wh"] = np.array([e, p, o], dtype=np.float64)
            out[f"s{i}_c{j}_cost"] = np.float64(cost)
            out[f"s{i}_c{j}_path"] = np.array(path, dtype=np.float64)
            out[f"s{i}_c{j}_prims"] = np.array([PO.MP_NAMES.index(m) for m in names], dtype=np.int32)
            out[f"s{i}_c{j}_traj"] = np.asarray(traj, dtype=np.float64)
            out[f"s{i}_c{j}_n_expanded"] = np.int64(n_exp)
            seqs.add(tuple(names))
            print(f"scenario {i} ({label}) e {e} p {p} o {o}: cost {cost:8.3f}, {len(path) - 1:2d} primitives, {n_exp} expansions")
        assert len(seqs) >= 2, label                                 # (a test against this scenario fails with the weights ignored)
    np.savez_compressed(os.path.join(HERE, "planner_multi.npz"), **out)


if __name__ == "__main__":
    main()
