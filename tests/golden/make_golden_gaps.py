#!/usr/bin/env python3
"""Fixture for the time gap per recorded tick: the REFERENCE's own check_collision_moving_cars and
check_collision_moving_bicycle (main/lib/collision_avoidance.py:68-166) with BicycleModelDimensions and BicycleRealDimensions,
called the way main/planner/moving_obstacle_avoidance.py:59-76 calls them -- once per episode on the episode's arrays, traj_agent =
path_agent_detailed = the ego's poses, the vehicles' poses of the same ticks -- on the synthetic pose series of tests/gap_cases.py,
at every frame_window 0 .. 63, for every case cut to every length of gap_cases.TICK_COUNTS.  Written to tests/golden/gaps.npz, data
only.

`records` holds one row per (tick count, case, episode): ticks, case, the episode's first tick, and the least frame_window at which
the reference does not return None, or -1 when it returns None up to 63.

Restatement-made and flagged (`restated`): a car and a cyclist in one list, and egos that are each other's vehicles -- no reference
function takes either; their rows are tests/gaps_numpy.py's ep_gap at window 63 under the episode rule.  The restatement is checked
against every reference-made row right here, and has to regenerate its own rows bit for bit in the CPU test.

Condition asserted here and stored (`margin`; a case that breaks it is replaced, not excused): every distance that is compared at
any offset within +-63, under both rules, is at least 1e-9 away from its threshold.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_gaps.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gap_cases as GC                                                # noqa: E402
import gaps_numpy as GN                                               # noqa: E402
from make_golden_conflicts import load_reference                      # noqa: E402


def main():
    car, bike, check_cars, check_bicycle = load_reference()
    for dims, mine in ((car, GC.CAR), (bike, GC.BIKE)):
        assert (dims.circle_centers[0, 0], dims.circle_centers[1, 0], dims.radius) == mine and not dims.circle_centers[:, 1].any()
    cs = GC.cases()
    B = len(cs)
    A = GC.recorder_arrays(cs)

    def reference(c, k0, k1, w):
        ego = c["ego"][k0:k1 + 1]
        trajs = [v[k0:k1 + 1] for v in c["vehicles"]]
        if c["kinds"] and c["kinds"][0] == "bike":
            return check_bicycle(car, bike, ego, ego, trajs, frame_window=w)
        return check_cars(car, ego, ego, trajs, frame_window=w)

    stats = {}
    GC.restate(A, GN.MAX_WINDOW, "record", stats=stats)               # every tick pair within +-63 that either rule admits
    records, calls = [], 0
    for n in GC.TICK_COUNTS:
        mine = GC.restate(A, GN.MAX_WINDOW, "episode", n=n)
        for b, c in enumerate(cs):
            for k0, k1 in GN.episodes_of(c["flags"][:n]):
                if c["restated"]:
                    records.append((n, b, k0, int(mine["ep_gap"][k0, b])))
                    continue
                assert len(set(c["kinds"])) <= 1, c["label"]
                least = -1
                for w in range(GN.MAX_WINDOW + 1):
                    calls += 1
                    if reference(c, k0, k1, w) is not None:
                        least = w
                        break
                assert least == mine["ep_gap"][k0, b], (c["label"], n, k0, least, int(mine["ep_gap"][k0, b]))
                records.append((n, b, k0, least))
    margin = stats["margin"]
    print(f"{B} cases, {len(records)} episode records, {calls} reference calls; smallest |dist - threshold| {margin:.3g}")
    whole = GC.expected({"n_cases": B, "records": np.array(records)}, GC.N)[1]
    for b, c in enumerate(cs):
        print(f"case {b:2d} ({c['label']}): least window per episode {[int(whole[k0, b]) for k0, _ in GN.episodes_of(c['flags'])]}")
    assert margin >= 1e-9, margin
    n_veh = max(len(c["vehicles"]) for c in cs)
    veh, kinds = np.full((B, n_veh, GC.N, 3), np.nan), np.full((B, n_veh), -1, dtype=np.int8)
    for b, c in enumerate(cs):
        for i, v in enumerate(c["vehicles"]):
            veh[b, i], kinds[b, i] = v, ("car", "bike").index(c["kinds"][i])
    out = {"n_cases": np.int64(B), "labels": np.array([c["label"] for c in cs]), "restated": np.array([c["restated"] for c in cs]),
           "ego": np.stack([c["ego"] for c in cs]), "vehicles": veh, "kinds": kinds, "flags": np.stack([c["flags"] for c in cs]),
           "car_shape": np.array(GC.CAR), "bike_shape": np.array(GC.BIKE), "records": np.array(records, dtype=np.int32),
           "margin": np.float64(margin)}
    path = os.path.join(HERE, "gaps.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
