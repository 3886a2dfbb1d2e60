#!/usr/bin/env python3
"""Fixture for the collision cut-off glue at its chunk edges and table limits: the situations of
tests/pre_tick_edge_cases.py, written to tests/golden/pre_tick_edges.npz, data only.

A case goes through the REFERENCE's own functions when the reference can express it -- one shape for all obstacles, frame_window <=
n_steps (beyond that its _offset_trajectories_by_frames changes the trajectory length), no status:
    lib.trajectories.resample_curve / calc_nearest_index_in_direction,
    lib.moving_obstacles_prediction.MovingObstaclesPrediction.state_prediction,
    lib.collision_avoidance.check_collision_moving_cars / check_collision_moving_bicycle / get_cutoff_curve_by_position_idx
chained as main/scenarios/mpc_intersection.py:104-140 chains them; ref_made says so.  Every other case -- mixed shapes, frame_window
above n_steps, the table refusals (status 4), the nearest-three anomaly, the egos of the interacting groups (stored after the cases) -- is stored as the numpy
restatement (pre_tick_edge_cases.run) makes it.  The decoded first row (frame, ego circle, obstacle, offset, obstacle circle) is the
restatement's for every case: the reference returns the point only.  The restatement is checked against every reference-made case
right here, exactly.  Only expected outputs and a digest of the regenerated inputs are stored.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_pre_tick_edges.py"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import pre_tick_edge_cases as E                                      # noqa: E402


def reference_main():
    for p in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if p and os.path.isdir(p):
            return p
    raise SystemExit("reference not present")


def by_reference(c, lib):
    """mpc_intersection.py:104-140 with the reference's own functions: (traj_idx, kept indices, hit, first, (x, y), path_len)."""
    car, bike = lib["car"], lib["bike"]
    full, (x, y, v, yaw) = c["path"], c["state"]
    idx = c["idx"]
    if c["prev"] < 0 or idx != c["prev"] - 1:
        idx = int(lib["nearest"](lib["State"](x=x, y=y, yaw=yaw, v=v), full[:, 0], full[:, 1], start_index=idx, forward=True))
    traj = full[idx:]
    if v < lib["MAX_SPEED"]:
        rdl = np.cumsum(np.zeros((traj.shape[0],)) + E.AMAX) + v
        res = lib["resample"](traj, dl=E.DT * np.minimum(rdl, lib["MAX_SPEED"]))
    else:
        res = lib["resample"](traj, dl=E.DT * lib["MAX_SPEED"])
    kept, k = [], 0
    for p in res:                                                     # rows of a path are distinct points, kept in order
        while not (traj[k, 0] == p[0] and traj[k, 1] == p[1]):
            k += 1
        kept.append(k)
        k += 1
    bikes = bool(c["obst"]) and c["shapes"][0] == E.BIKE
    dims = bike if bikes else car
    preds = [np.vstack(lib["Prediction"](*o, sample_time=E.DT, car_dimensions=dims).state_prediction(E.horizon_of(c["n_steps"]))).T for o in c["obst"]]
    if bikes:
        col = lib["check_bicycle"](car, bike, res, traj, preds, frame_window=c["w"])
    else:
        col = lib["check_cars"](car, res, traj, preds, frame_window=c["w"])
    if col is None:
        return idx, kept, False, -1, (0.0, 0.0), len(full)
    cut = lib["cutoff"](full, col[0], col[1])
    assert isinstance(cut, (int, np.integer))
    margin = c["margin_factor"] * int(math.ceil(car.radius / c["dl"]))
    return idx, kept, True, int(col[2]), (float(col[0]), float(col[1])), max(idx + 1, int(cut) - margin)


def record(r):
    return dict(status=np.int64(r["status"]), traj_idx=np.int64(r["traj_idx"]), n_res=np.int64(r["n_res"]), kept=np.asarray(r["kept"], dtype=np.int32),
                hit=np.bool_(r["hit"]), first_idx=np.int64(r["first_idx"]), col_xy=np.array(r["col_xy"], dtype=np.float64),
                path_len=np.int64(-1 if r["path_len"] is None else r["path_len"]),
                row=np.array(r["row"] if r["row"] is not None else (-1,) * 5, dtype=np.int64))


def main():
    sys.path.insert(0, reference_main())
    import matplotlib
    matplotlib.use("Agg")
    from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
    from lib.collision_avoidance import check_collision_moving_bicycle, check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    from lib.simulation import Simulation, State
    from lib.trajectories import calc_nearest_index_in_direction, resample_curve
    lib = dict(car=BicycleModelDimensions(skip_back_circle_collision_checking=False), bike=BicycleRealDimensions(skip_back_circle_collision_checking=False),
               check_cars=check_collision_moving_cars, check_bicycle=check_collision_moving_bicycle, cutoff=get_cutoff_curve_by_position_idx,
               Prediction=MovingObstaclesPrediction, MAX_SPEED=Simulation.MAX_SPEED, State=State, nearest=calc_nearest_index_in_direction,
               resample=resample_curve)
    assert lib["MAX_SPEED"] == E.VMAX and lib["car"].radius == E.EGO_R and tuple(lib["car"].circle_centers[:, 0]) == tuple(E.EGO_OFFS)
    assert lib["bike"].radius == E.BIKE[2] and tuple(lib["bike"].circle_centers[:, 0]) == E.BIKE[:2]
    cases, restated = E.cases(), E.restated()
    recs, labels, made_flags, digests = [], [], [], []
    n_ref = 0
    for i, (c, r) in enumerate(zip(cases, restated)):
        rec = record(r)
        made = E.reference_made(c, r)
        if made:
            idx, kept, hit, first, xy, plen = by_reference(c, lib)
            assert (idx, kept, hit, first, xy, plen) == (r["traj_idx"], r["kept"].tolist(), r["hit"], r["first_idx"], tuple(r["col_xy"]), r["path_len"]), c["label"]
            rec.update(traj_idx=np.int64(idx), n_res=np.int64(len(kept)), kept=np.array(kept, dtype=np.int32), hit=np.bool_(hit), first_idx=np.int64(first),
                       col_xy=np.array(xy, dtype=np.float64), path_len=np.int64(plen))
            n_ref += 1
        recs.append(rec); labels.append(c["label"]); made_flags.append(made); digests.append(E.digest(c))
        print(f"case {i:2d} ({c['label']}): {'reference' if made else 'restatement'}, status {r['status']}, n_res {r['n_res']}, row {r['row']}, path_len {r['path_len']}")
    for g in E.group_cases():                                         # the egos of the interacting groups follow the cases
        for c in E.group_ego_cases(g):
            recs.append(record(E.run(c))); labels.append(c["label"]); made_flags.append(False); digests.append(E.digest(c))
    out = {"n_cases": np.int64(len(cases)), "label": np.array(labels), "ref_made": np.array(made_flags), "digest": np.array(digests),
           "kept_off": np.concatenate([[0], np.cumsum([len(r["kept"]) for r in recs])]).astype(np.int64),
           "kept": np.concatenate([r["kept"] for r in recs]).astype(np.int32)}
    for k in ("status", "traj_idx", "n_res", "hit", "first_idx", "col_xy", "path_len", "row"):
        out[k] = np.stack([r[k] for r in recs])
    print("reference-made:", n_ref, "of", len(cases))
    path = os.path.join(HERE, "pre_tick_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
