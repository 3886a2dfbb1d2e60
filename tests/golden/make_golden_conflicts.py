#!/usr/bin/env python3
"""Fixture for the clearance and first-contact evaluation: the REFERENCE's own
check_collision_moving_cars and check_collision_moving_bicycle (main/lib/collision_avoidance.py:85-166) with
BicycleModelDimensions and BicycleRealDimensions, called the way main/planner/moving_obstacle_avoidance.py:44-76 calls them -- once
per episode on the episode's arrays, traj_agent = path_agent_detailed = the ego's poses, the vehicles' poses of the same ticks --
on the synthetic pose series of tests/conflict_cases.py, for every frame_window of conflict_cases.WINDOWS and every case cut to
every length of conflict_cases.TICK_COUNTS.  Written to tests/golden/conflicts.npz, data only.

`records` holds one row per (window, tick count, case, episode): window, ticks, case, the episode's first tick, hit (the reference
did not return None), hit_tick, first_frame_idx, x, y.  hit_tick is reference-made too, at window 0: the first prefix length of the
episode for which the reference does not return None, minus one (every prefix is tried; a cut episode's prefixes are prefixes of
the whole one, so the whole run's value serves every cut that reaches it).  At the other windows the column holds -2.

Restatement-made and flagged (`restated`): a car and a cyclist in one list, and egos that are each other's vehicles -- no reference
function takes either; their rows come from tests/conflicts_numpy.py.  The restatement is checked against every reference-made
row right here, and has to regenerate its own rows bit for bit in the CPU test.

Condition asserted here and stored (`margin`; a case that breaks it is replaced, not excused): every distance the evaluation
compares -- every row of every frame at window 20, and every frame of the ego's circle trajectories against a hit position -- is at
least 1e-9 away from its threshold.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_conflicts.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import conflict_cases as TC                                           # noqa: E402
import conflicts_numpy as CN                                          # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
            from lib.collision_avoidance import check_collision_moving_bicycle, check_collision_moving_cars
            car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
            bike = BicycleRealDimensions(skip_back_circle_collision_checking=False)
            return car, bike, check_collision_moving_cars, check_collision_moving_bicycle
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    car, bike, check_cars, check_bicycle = load_reference()
    for dims, mine in ((car, TC.CAR), (bike, TC.BIKE)):
        assert (dims.circle_centers[0, 0], dims.circle_centers[1, 0], dims.radius) == mine and not dims.circle_centers[:, 1].any()
    cs = TC.cases()
    B = len(cs)
    A = TC.recorder_arrays(cs)

    def reference(c, k0, k1, w):
        ego = c["ego"][k0:k1 + 1]
        trajs = [v[k0:k1 + 1] for v in c["vehicles"]]
        if c["kinds"] and c["kinds"][0] == "bike":
            return check_bicycle(car, bike, ego, ego, trajs, frame_window=w)
        return check_cars(car, ego, ego, trajs, frame_window=w)

    stats = {}
    records, n_hit = [], 0
    for w in TC.WINDOWS:
        for n in sorted(TC.TICK_COUNTS, reverse=True):                # (the whole run first: its hit_tick serves the cuts)
            mine = TC.restate(A, w, n=n, stats=stats)
            whole = TC.restate(A, 0) if w == 0 else None
            for b, c in enumerate(cs):
                for k0, k1 in CN.episodes_of(c["flags"][:n]):
                    if c["restated"]:
                        hit = mine["hit_tick"][k0, b] >= 0
                        records.append((w, n, b, k0, hit, mine["hit_tick"][k0, b], mine["hit_frame"][k0, b], *mine["hit_xy"][k0, b]))
                        continue
                    assert len(set(c["kinds"])) <= 1, c["label"]
                    got = reference(c, k0, k1, w)
                    tick = -2
                    if w == 0:
                        tick = -1
                        if n == TC.N:
                            for length in range(1, k1 - k0 + 2):
                                if reference(c, k0, k0 + length - 1, 0) is not None:
                                    tick = k0 + length - 1
                                    break
                            c.setdefault("hit_tick", {})[k0] = tick
                        else:                                         # the whole run's value, where the cut reaches it
                            tick = c["hit_tick"][k0] if 0 <= c["hit_tick"][k0] < n else -1
                        assert (tick >= 0) == (got is not None), (c["label"], w, n, k0)
                        assert tick == mine["hit_tick"][k0, b] and tick == (whole["hit_tick"][k0, b] if 0 <= whole["hit_tick"][k0, b] < n else -1)
                    # the restatement, which is also what `clear`, `who` and `row` of the launch are compared with
                    assert (got is not None) == (mine["hit_tick"][k0, b] >= 0), (c["label"], w, n, k0)
                    if got is None:
                        records.append((w, n, b, k0, 0, tick, -1, np.nan, np.nan))
                        assert mine["hit_frame"][k0, b] == -1 and np.isnan(mine["hit_xy"][k0, b]).all()
                    else:
                        n_hit += 1
                        records.append((w, n, b, k0, 1, tick, int(got[2]), float(got[0]), float(got[1])))
                        assert (mine["hit_frame"][k0, b], *mine["hit_xy"][k0, b]) == (int(got[2]), float(got[0]), float(got[1])), (c["label"], w, n, k0)
    margin = stats["margin"]
    print(f"{B} cases, {len(records)} episode records, {n_hit} reference-made with a contact; smallest |dist - threshold| {margin:.3g}")
    full = {w: TC.restate(A, w) for w in TC.WINDOWS}
    for b, c in enumerate(cs):
        print(f"case {b:2d} ({c['label']}): episodes {CN.episodes_of(c['flags'])}, per window (hit_tick, hit_frame) "
              f"{[[(int(full[w]['hit_tick'][k0, b]), int(full[w]['hit_frame'][k0, b])) for k0, _ in CN.episodes_of(c['flags'])] for w in TC.WINDOWS]}")
    assert margin >= 1e-9, margin
    n_veh = max(len(c["vehicles"]) for c in cs)
    veh = np.full((B, n_veh, TC.N, 3), np.nan)
    for b, c in enumerate(cs):
        for i, v in enumerate(c["vehicles"]):
            veh[b, i] = v
    out = {"n_cases": np.int64(B), "labels": np.array([c["label"] for c in cs]), "restated": np.array([c["restated"] for c in cs]),
           "ego": np.stack([c["ego"] for c in cs]), "vehicles": veh, "n_vehicles": np.array([len(c["vehicles"]) for c in cs]),
           "bike": np.array([bool(c["kinds"]) and c["kinds"][0] == "bike" for c in cs]), "flags": np.stack([c["flags"] for c in cs]),
           "car_shape": np.array(TC.CAR), "bike_shape": np.array(TC.BIKE), "records": np.array(records, dtype=np.float64),
           "margin": np.float64(margin)}
    path = os.path.join(HERE, "conflicts.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
