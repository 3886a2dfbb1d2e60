#!/usr/bin/env python3
"""Fixture for the static-obstacle evaluation: the REFERENCE's own BoxObstacle / CircleObstacle
(main/lib/obstacles.py: to_convex, distance_to_point), check_collision (:157-176), car_trajectory_to_collision_point_trajectories
(main/lib/trajectories.py:40-55) with BicycleModelDimensions, and its scenario builders envs.intersection.intersection,
envs.roundabout.roundabout and envs.t_intersection.t_intersection, on the synthetic pose series of tests/static_cases.py.  Written to
tests/golden/static.npz, data only.

Per set: the rows [32] made from the objects' own xy1 / xy2 / radius / xy_center / hidden and to_convex(margin = the ego radius),
and the objects' constructor arguments (`prims`: kind, hidden, then xy_width + xy_center or radius + xy_center), from which the CPU
test rebuilds the rows with planner.static_obstacle_rows.  Per case, tick and hidden setting, reference-made: `hit` = the first
obstacle of the scenario's list for which check_collision(to_convex(margin), the two circle centres) holds, `clear` = the smallest
distance_to_point(centre) - radius and `who` = the first obstacle that attains it; with include_hidden = 0 the hidden obstacles are
passed over (their indices still count).  Every per-tick value depends on its own tick alone, so the whole run's arrays serve every
cut of static_cases.TICK_COUNTS as a prefix.

`intersection_rows`: for every (number_of_lanes, start_pos, turn_indicator, start_lane, goal_lane) of envs.intersection.intersection
(number_of_lanes stored as 0) and of envs.intersection_multi_lanes.intersection with two lanes, the SHA-256 of the rows made the same
way (`intersection_digests`), which pins planner.intersection_obstacles -- the hidden flags included -- without storing 60 tables.
No pose series is held against the two-lane sets.  Not called: envs/arterial_multi_lanes.py (it imports lib.mpc and with it cvxpy,
which is not installed where this runs).

Conditions asserted here and stored (`hp_margin`, `who_margin` per case and hidden setting; a case that breaks one is replaced, not
excused): outside the cases flagged `exact`, every half-plane value that decides whether a (centre, obstacle) pair touches is at
least 1e-9 from 0, and the two smallest per-obstacle clearances of every tick differ by at least 1e-9.  For every stored point and
obstacle of its set, check_collision's matrix product gives the same booleans as the unfused (a * x + b * y) + c <= 0.  The exact
case's two half-plane values are asserted to be 0.0 and one ulp of the edge coordinate (4.44e-16).

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_static.py"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import static_cases as SC                                             # noqa: E402
import static_numpy as SN                                             # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from envs.intersection import intersection
            from envs.intersection_multi_lanes import intersection as intersection_multi_lanes
            from envs.roundabout import roundabout
            from envs.t_intersection import t_intersection
            from lib.car_dimensions import BicycleModelDimensions
            from lib.obstacles import BoxObstacle, CircleObstacle, check_collision
            from lib.trajectories import car_trajectory_to_collision_point_trajectories
            return dict(intersection=intersection, intersection_multi_lanes=intersection_multi_lanes, roundabout=roundabout,
                        t_intersection=t_intersection, BoxObstacle=BoxObstacle, CircleObstacle=CircleObstacle, check_collision=check_collision, Dims=BicycleModelDimensions,
                        circles=car_trajectory_to_collision_point_trajectories)
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    ref = load_reference()
    Box, Circle, check = ref["BoxObstacle"], ref["CircleObstacle"], ref["check_collision"]
    car = ref["Dims"](skip_back_circle_collision_checking=False)
    assert (car.circle_centers[0, 0], car.circle_centers[1, 0], car.radius) == SC.CAR and not car.circle_centers[:, 1].any()
    margin = car.radius

    def built(p):
        return Box(xy_width=p[1], height=0.5, xy_center=p[2], hidden=p[3]) if p[0] == "box" else Circle(radius=p[1], height=0.5, xy_center=p[2], hidden=p[3])

    sets = [ref["intersection"](1, 1).obstacles, ref["roundabout"](1, 1, "small").obstacles, ref["t_intersection"](1, 1).obstacles]
    sets += [[built(p) for p in SC.SYNTHETIC[s]] for s in range(3, len(SC.SET_NAMES))]
    for want, s in zip(((24, 16, 8, 4), (29, None, None, 8), (16, None, None, 3)), sets):
        got = (len(s), sum(hasattr(o, "xy1") for o in s), sum(hasattr(o, "radius") for o in s), sum(o.hidden for o in s))
        assert all(w is None or w == g for w, g in zip(want, got)), (want, got)

    def row_of(o):
        hp = np.asarray(o.to_convex(margin), dtype=np.float64)
        r = np.zeros(SN.ROW)
        if hasattr(o, "xy1"):
            r[:7] = 0, o.hidden, len(hp), *o.xy1, *o.xy2
        else:
            r[:7] = 1, o.hidden, len(hp), *o.xy_center, o.radius, 0.0
        r[8:8 + hp.size] = hp.reshape(-1)
        return r

    rows, prims, set_off = [], [], [0]
    for s in sets:
        for o in s:
            rows.append(row_of(o))
            prims.append((0, o.hidden, *o.xy_width, *o.xy_center) if hasattr(o, "xy1") else (1, o.hidden, o.radius, *o.xy_center, 0.0))
        set_off.append(len(rows))
    rows, prims, set_off = np.array(rows), np.array(prims, dtype=np.float64), np.array(set_off, dtype=np.int32)

    # every intersection the library restates, as digests of the reference-made rows
    keys, digests = [], []
    for nl, sp, tn, sl, gl in SC.intersection_configs():
        sc = ref["intersection"](tn, sp) if nl == 0 else ref["intersection_multi_lanes"](tn, sp, sl, gl, nl)
        keys.append((nl, sp, tn, sl, gl))
        digests.append(hashlib.sha256(np.array([row_of(o) for o in sc.obstacles]).tobytes()).hexdigest())

    cs = SC.cases()
    B = len(cs)
    hit = np.full((2, SC.N, B), -1, dtype=np.int16)
    who = np.full((2, SC.N, B), -1, dtype=np.int16)
    clear = np.full((2, SC.N, B), np.nan)
    same = 0
    for b, c in enumerate(cs):
        front, rear = ref["circles"](c["ego"], car)
        objs = sets[c["set"]]
        planes = [o.to_convex(margin) for o in objs]
        for k in range(SC.N):
            pts = np.array([[front[k, 0], rear[k, 0]], [front[k, 1], rear[k, 1]]])
            touched = [check(hp, pts) for hp in planes]
            dist = [min(o.distance_to_point(pts[:, 0]), o.distance_to_point(pts[:, 1])) - car.radius for o in objs]
            for hp, t in zip(planes, touched):                        # the matrix product against the unfused expression
                v = SN.halfplane_values(hp, pts[0], pts[1])
                assert bool(((v <= 0.0).all(axis=0)).any()) == t, (c["label"], k)
                same += v.size
            for hidden in SC.HIDDEN:
                inc = [i for i, o in enumerate(objs) if hidden or not o.hidden]
                hit[hidden, k, b] = next((i for i in inc if touched[i]), -1)
                if inc:
                    best = min(dist[i] for i in inc)
                    clear[hidden, k, b], who[hidden, k, b] = best, next(i for i in inc if dist[i] == best)

    # the restatement against what the reference made, and the conditions
    A = SC.recorder_arrays(cs)
    g = {"set_off": set_off, "rows": rows}
    hp_margin, who_margin = np.zeros((2, B)), np.zeros((2, B))
    for hidden in SC.HIDDEN:
        stats = {}
        mine = SC.restate(A, g, hidden, stats=stats)
        assert np.array_equal(mine["hit"], hit[hidden]) and np.array_equal(mine["who"], who[hidden]), hidden
        assert np.array_equal(np.isnan(mine["clear"]), np.isnan(clear[hidden]))
        ok = ~np.isnan(clear[hidden])
        err = np.max(np.abs(mine["clear"][ok] - clear[hidden][ok]) / np.maximum(1.0, np.abs(clear[hidden][ok])))
        assert err <= 1e-12, err
        hp_margin[hidden], who_margin[hidden] = stats["hp_margin"], stats["who_margin"]
        print(f"include_hidden = {hidden}: restatement equals the reference-made hit / who, clear within {err:.3g}")
    exact = np.array([c["exact"] for c in cs])
    for b, c in enumerate(cs):
        print(f"case {b:2d} set {c['set']} ({c['label']}): ticks touching {[(int((hit[h, :, b] >= 0).sum())) for h in SC.HIDDEN]}, "
              f"hit {sorted(set(hit[1, :, b].tolist()))}, clear {np.nanmin(clear[0, :, b]) if c['set'] != 3 and not np.isnan(clear[0, :, b]).all() else float('nan'):+.3f} "
              f"... {np.nanmax(clear[0, :, b]) if not np.isnan(clear[0, :, b]).all() else float('nan'):+.3f}, "
              f"hp margin {hp_margin[:, b].min():.3g}, who margin {who_margin[:, b].min():.3g}{' (exact)' if c['exact'] else ''}")
    assert (hp_margin[:, ~exact] >= 1e-9).all() and (who_margin[:, ~exact] >= 1e-9).all()
    # the exact case: the two half-plane values
    on, off = SC.exact_edge_poses()
    right = rows[set_off[8]][8:11]
    v = [float((right[0] * (p[0] + 1.0 * SC.CAR[1]) + right[1] * 0.0) + right[2]) for p in (on, off)]
    assert v[0] == 0.0 and v[1] == 4.440892098500626e-16, v
    b = B - 1
    assert cs[b]["set"] == 8 and np.all(hit[0, 0::2, b] == 0) and np.all(hit[0, 1::2, b] == -1)
    print(f"{B} cases, {len(rows)} rows in {len(sets)} sets, {same} half-plane values checked against the matrix product; "
          f"edge values {v}")

    out = {"n_cases": np.int64(B), "labels": np.array([c["label"] for c in cs]), "exact": exact, "set_names": np.array(SC.SET_NAMES),
           "ego": np.stack([c["ego"] for c in cs]), "flags": np.stack([c["flags"] for c in cs]), "set_of": A["set_of"],
           "set_off": set_off, "rows": rows, "prims": prims, "car_shape": np.array(SC.CAR), "margin": np.float64(margin),
           "hit": hit, "who": who, "clear": clear, "hp_margin": hp_margin, "who_margin": who_margin, "edge_values": np.array(v),
           "intersection_rows": np.array(keys, dtype=np.int32), "intersection_digests": np.array(digests)}
    path = os.path.join(HERE, "static.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
