#!/usr/bin/env python3
"""Fixture for the projection of every recorded vehicle onto the ego's path, on the cases of
tests/headway_cases.py.  Written to tests/golden/headway.npz, data only.

Reference-made, two pieces:
  `centres` [cases][ticks / 5][9][2][2] -- the REFERENCE's own car_trajectory_to_collision_point_trajectories
    (main/lib/trajectories.py:40-55) with BicycleModelDimensions and BicycleRealDimensions on every finite pose of the ego (row 0)
    and of every place of its list (row 1 + i): front and rear circle centre, x and y; NaN where there is no such place or the pose
    is not finite.  Every tick is made and compared here; every fifth (CENTRE_STRIDE) is stored, which keeps the file small;
  `idx` [cases][ticks][9][2] -- the REFERENCE's own calc_nearest_index (main/lib/trajectories.py:89-97), start_index = 0, on each
    of those centres and the case's path; -1 where there is none.
The restatement (tests/headway_numpy.py) is checked against both right here: its centres within 1e-12 (numpy's vectorised cos and
sin against math.cos and math.sin: a last bit), its indices exactly.  Everything else -- intervals, gap, lat, rate, TTC, the leader
and the episode values -- is restatement-made: no reference function computes a distance along a path between two vehicles.  The
restatement's lead, ttc_who, ep_i and ep_d are stored beside the two, with the cases' labels, paths, flags, speeds and ranges, so that
the CPU test can tell a changed case or restatement from a changed result.  The condition of headway_cases.condition() is asserted here and its smallest margin stored.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_headway.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import headway_cases as HC                                            # noqa: E402
import headway_numpy as HN                                            # noqa: E402
from conflicts_numpy import vehicle_list                              # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
            from lib.simulation import State
            from lib.trajectories import calc_nearest_index, car_trajectory_to_collision_point_trajectories
            car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
            bike = BicycleRealDimensions(skip_back_circle_collision_checking=False)
            return car, bike, State, calc_nearest_index, car_trajectory_to_collision_point_trajectories
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    car, bike, State, calc_nearest_index, to_circles = load_reference()
    for dims, mine in ((car, HC.CAR), (bike, HC.BIKE)):
        assert (dims.circle_centers[0, 0], dims.circle_centers[1, 0], dims.radius) == mine and not dims.circle_centers[:, 1].any()
    cs, paths = HC.cases(), HC.paths()
    A = HC.recorder_arrays(cs)
    mine = HC.restate(A)
    margin = HC.condition(cs, mine)
    B, N = len(cs), HC.N
    st = HN.start_states(A["rec"], A["flags"], A["x_first"], A["x_spawn"])
    centres = np.full((B, N, 9, 2, 2), np.nan)
    idx = np.full((B, N, 9, 2), -1, dtype=np.int32)
    calls = 0
    for b, c in enumerate(cs):
        path = paths[c["path"]]
        cx, cy = np.ascontiguousarray(path[:, 0]), np.ascontiguousarray(path[:, 1])
        lst = vehicle_list(b, B, A["obs"].shape[1], A["veh_range"], A["mate_range"])
        if not lst:
            continue
        series = [(st[:, b], car)]                                    # [N][4] x, y, yaw, v and the dimensions, ego first
        for kind, j in lst:
            if kind == "veh":
                series.append((A["obs"][:, j][:, [0, 1, 3, 2]], car if A["shapes"][j, 3] == 2.86 else bike))
            else:
                series.append((st[:, j], car))
        ego_ok = np.isfinite(st[:, b]).all(axis=1)
        for slot, (tr, dims) in enumerate(series):
            ok = ego_ok & np.isfinite(tr).all(axis=1)
            if not ok.any():
                continue
            circles = to_circles(np.ascontiguousarray(tr[ok, :3]), dims)
            assert len(circles) == 2
            for which, circ in enumerate(circles):
                centres[b, ok, slot, which] = circ[:, :2]
                idx[b, ok, slot, which] = [calc_nearest_index(State(x=x, y=y, yaw=0.0, v=0.0), cx, cy, 0) for x, y in circ[:, :2].tolist()]
                calls += int(ok.sum())
        got = mine["centres"][:, b]
        assert np.array_equal(np.isnan(got), np.isnan(centres[b])), c["label"]
        assert np.nanmax(np.abs(got - centres[b])) <= 1e-12, (c["label"], float(np.nanmax(np.abs(got - centres[b]))))
        assert np.array_equal(mine["idx"][:, b], idx[b]), (c["label"], np.argwhere(mine["idx"][:, b] != idx[b])[:5])
        print(f"case {b} ({c['label']}): path {c['path']} of {len(path)} points, {len(lst)} places, idx {idx[b][idx[b] >= 0].min()} .. {idx[b].max()}")
    print(f"{B} cases, {calls} reference calls of calc_nearest_index; smallest margin apart from the ties {margin:.3g}")
    T = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 0))         # [ticks][cases]... -> [cases][ticks]...
    out = {"n_cases": np.int64(B), "labels": np.array([c["label"] for c in cs]), "v_ego": np.array([c["v_ego"] for c in cs]),
           "flags": np.stack([c["flags"] for c in cs]).astype(np.int8), "path": np.array([c["path"] for c in cs], dtype=np.int32),
           "veh_range": A["veh_range"], "mate_range": A["mate_range"], "centres": centres[:, ::HC.CENTRE_STRIDE], "idx": idx.astype(np.int16),
           "margin": np.float64(margin), "launch_margin": np.float64(HC.LAUNCH_MARGIN),
           **{k: T(mine[k]) for k in ("lead", "ttc_who", "ep_i", "ep_d")}}
    path = os.path.join(HERE, "headway.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
