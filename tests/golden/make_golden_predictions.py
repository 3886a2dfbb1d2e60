#!/usr/bin/env python3
"""Fixture for the error of every recorded prediction: the REFERENCE's own
MovingObstaclesPrediction(x, y, v, yaw, a, steer, sample_time=dt, car_dimensions=...).state_prediction((n_steps - 0.5) * dt)
(main/lib/moving_obstacles_prediction.py:10-47) -- BicycleModelDimensions for the cars and the egos, BicycleRealDimensions for the
cyclist's wheelbase -- from the tuple of every tick of every row of tests/prediction_cases.py, at n_steps 1, 35, 63 and 64, for the
series cut to every length of prediction_cases.TICK_COUNTS.  (That horizon gives exactly n_steps samples; n_steps * dt gives 64 at
n_steps = 63.  The length is asserted.)  The error arithmetic on those samples is tests/predictions_numpy.py, in the rule's order.
Written to tests/golden/predictions.npz, data only: expected outputs and the digest of the inputs.

Conditions asserted here (a case that breaks one is replaced, not excused): no scored error lies within 1e-6 of the tolerance; on
every tick the largest error beats the next largest by at least 1e-6, or equals it bit for bit.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_predictions.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import prediction_cases as PC                                         # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
            from lib.moving_obstacles_prediction import MovingObstaclesPrediction
            return MovingObstaclesPrediction, BicycleModelDimensions(), BicycleRealDimensions()
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    Prediction, car, bike = load_reference()
    assert (car.distance_back_to_front_wheel, bike.distance_back_to_front_wheel) == (PC.L_CAR, PC.L_BIKE)
    dims = {PC.L_CAR: car, PC.L_BIKE: bike}
    calls = [0]

    def reference(tup, L, dt, n_steps):
        x, y, v, yaw, a, steer = (float(t) for t in tup)
        xs, ys, yaws, _ = Prediction(x, y, v, yaw, a, steer, sample_time=dt, car_dimensions=dims[float(L)]).state_prediction((n_steps - 0.5) * dt)
        assert len(xs) == len(ys) == len(yaws) == n_steps, (len(xs), n_steps)
        calls[0] += 1
        return np.stack([xs, ys, yaws], axis=1)

    A = PC.recorder_arrays()
    predictor = PC.cached(reference)
    results, tol_margin, max_margin = {}, np.inf, np.inf
    for S in PC.STEPS:
        for n in PC.TICK_COUNTS:
            r = results[n, S] = PC.restate(A, n, S, predictor=predictor)
            e = r["err"]
            scored = ~np.isnan(e)
            if scored.any():
                tol_margin = min(tol_margin, float(np.abs(e[scored] - PC.TOL).min()))
            if S < 2:
                continue
            top2 = np.sort(np.where(scored, e, -np.inf), axis=2)[:, :, -2:]             # [n][V][2]: the next largest, the largest
            two = np.isfinite(top2[:, :, 0])
            gap = top2[:, :, 1][two] - top2[:, :, 0][two]
            if gap[gap != 0.0].size:
                max_margin = min(max_margin, float(gap[gap != 0.0].min()))
    print(f"{calls[0]} reference predictions; smallest |e - tol| {tol_margin:.3g}; smallest nonzero gap between a tick's two largest errors {max_margin:.3g}")
    assert tol_margin >= 1e-6 and max_margin >= 1e-6, (tol_margin, max_margin)
    full = results[max(PC.TICK_COUNTS), 64]
    for r in range(PC.N_OBS + PC.B):
        i, d = full["pt_i"][:, r], full["pt_d"][:, r]
        print(f"row {r:2d}: hold {i[:, 1].min()}..{i[:, 1].max()}, ticks with an error {int((d[:, 2] > 0).sum())}, largest {np.nanmax(d[:, 2]):.4g}, "
              f"mean ade {np.nanmean(d[:, 0]):.4g}")
    assert (full["pt_d"][:-1, 0, 2] == 0).all() and (full["pt_i"][:-64, 0, 1] == 64).all()      # the straight vehicle: error 0, hold = m
    assert full["pt_i"][0, 5, 1] == 0 and full["pt_i"][0, 6, 1] == 63                             # the tolerance at samples 0 and 63
    out = PC.pack(results)
    out.update(digest=np.array(PC.digest(A)), tol=np.float64(PC.TOL), dt=np.float64(PC.DT), tol_margin=np.float64(tol_margin),
               max_margin=np.float64(max_margin))
    np.savez_compressed(PC.FIXTURE, **out)
    size = os.path.getsize(PC.FIXTURE)
    print("wrote", PC.FIXTURE, size, "bytes")
    assert size < 100000, size
    g = PC.fixture()
    for (n, S), r in results.items():
        ex = PC.expected(g, n, S)
        assert all(PC.same_bits(np.ascontiguousarray(ex[k]), np.ascontiguousarray(r[k])) for k in ex), (n, S)


if __name__ == "__main__":
    main()
