#!/usr/bin/env python3
"""Fixture for the error of every recorded plan-rule prediction: the REFERENCE's own
lib.simulation.Simulation.step rolled out under the rule's inputs (as tests/golden/make_golden_mate_plan.py rolls it) from the
tick-start state and the recorded plan of every tick of every row of tests/plan_prediction_cases.py, at n_steps 1, 35, 63 and 64, for the
series cut to every length of plan_prediction_cases.TICK_COUNTS.  The rule decides only WHICH input every step gets; the step is
Simulation.step, executed unmodified.  Every ego's records are first integrated again by Simulation.step and must equal the cases'
bit for bit.  The error arithmetic on the samples is tests/predictions_numpy.py, in the rule's order.  Written to
tests/golden/plan_predictions.npz, data only: expected outputs and the digest of the inputs.

Conditions asserted here (a case that breaks one is replaced, not excused): no scored error lies within 1e-6 of the tolerance; on
every tick the largest error beats the next largest by at least 1e-6, or equals it bit for bit.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_plan_predictions.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import plan_prediction_cases as PC                                    # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from lib.car_dimensions import BicycleModelDimensions
            from lib.simulation import Simulation, State
            return Simulation, State, BicycleModelDimensions()
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    Simulation, State, car = load_reference()
    assert car.distance_back_to_front_wheel == PC.L_CAR
    assert (float(Simulation.MAX_STEER), Simulation.MAX_SPEED, Simulation.MIN_SPEED) == (PC.MAX_STEER, PC.MAX_SPEED, PC.MIN_SPEED)
    calls = [0]

    def reference(state, oa, od, status, delta_last, n_steps, dt, L):
        x, y, v, yaw = (float(t) for t in state)
        sim = Simulation(car_dimensions=car, sample_time=dt, initial_state=State(x=x, y=y, yaw=yaw, v=v))
        T, out = len(oa), np.zeros((n_steps, 3))
        for i in range(n_steps):
            j = i + 1
            if status == 0:
                a, d = (float(oa[j]), float(od[j])) if j <= T - 1 else (0.0, float(od[T - 1]))
            else:
                a, d = 0.0, float(delta_last)
            s = sim.step(a=a, delta=d)
            out[i] = (s.x, s.y, s.yaw)
        calls[0] += 1
        return out

    groups = PC.all_groups()
    # every record is the reference's own plant step from the recorded controls
    for T, A in groups.items():
        rec, flags = A["rec"], A["flags"]
        for b in range(rec.shape[1]):
            x, y, v, yaw = A["x_first"][b]
            sim = Simulation(car_dimensions=car, sample_time=PC.DT, initial_state=State(x=x, y=y, yaw=yaw, v=v))
            for k in range(PC.N):
                s = sim.step(a=float(rec[k, b, 5]), delta=float(rec[k, b, 4]))
                assert PC.same_bits(np.array([s.x, s.y, s.yaw, s.v]), rec[k, b, :4].copy()), (T, b, k)
                if flags[k, b] & (PC.GOAL | PC.AGE):
                    x, y, v, yaw = A["x_spawn"][b]
                    sim = Simulation(car_dimensions=car, sample_time=PC.DT, initial_state=State(x=x, y=y, yaw=yaw, v=v))
    predictor = PC.cached(reference)
    results, tol_margin, max_margin = {}, np.inf, np.inf
    for T, A in groups.items():
        for S in PC.STEPS:
            for n in PC.TICK_COUNTS:
                r = results[T, n, S] = PC.restate(A, n, S, predictor=predictor)
                e = r["err"]
                scored = ~np.isnan(e)
                if scored.any():
                    tol_margin = min(tol_margin, float(np.abs(e[scored] - PC.TOL).min()))
                if S < 2:
                    continue
                top2 = np.sort(np.where(scored, e, -np.inf), axis=2)[:, :, -2:]             # [n][B][2]: the next largest, the largest
                two = np.isfinite(top2[:, :, 0])
                gap = top2[:, :, 1][two] - top2[:, :, 0][two]
                if gap[gap != 0.0].size:
                    max_margin = min(max_margin, float(gap[gap != 0.0].min()))
    print(f"{calls[0]} reference rollouts; smallest |e - tol| {tol_margin:.3g}; smallest nonzero gap between a tick's two largest errors {max_margin:.3g}")
    assert tol_margin >= 1e-6 and max_margin >= 1e-6, (tol_margin, max_margin)
    for T in PC.HORIZONS:
        full = results[T, max(PC.TICK_COUNTS), 64]
        for b in range(full["pt_i"].shape[1]):
            i, d = full["pt_i"][:, b], full["pt_d"][:, b]
            print(f"T {T:2d} row {b}: hold {i[:, 1].min()}..{i[:, 1].max()}, ticks with an error {int((d[:, 2] > 0).sum())}, largest {np.nanmax(d[:, 2]):.4g}, "
                  f"mean ade {np.nanmean(d[:, 0]):.4g}")
        assert (full["pt_d"][:, 0, 2] == 0).all() and (full["pt_i"][:, 0, 1] == full["pt_i"][:, 0, 0]).all()      # the plan followed: error 0, hold = m
    # every case does what it is there for
    A = groups[13]
    v = A["rec"][:, :, 3]
    roll = lambda b, k: reference(np.r_[A["rec"][k - 1, b, [0, 1]], A["rec"][k - 1, b, 3], A["rec"][k - 1, b, 2]], A["plan_oa"][k, b], A["plan_od"][k, b],
                                  A["plan_status"][k, b], A["rec"][k - 1, b, 4], 64, PC.DT, PC.L_CAR)
    p = roll(1, 50)
    assert (p[5:, 0] == p[5, 0]).all() and (np.diff(A["rec"][:, 1, 0]) > 0.9).all()                          # braked to a stand; the ego drives on
    assert np.abs(A["plan_od"][PC.WAKE:, 5]).max() > PC.MAX_STEER and abs(A["plan_od"][PC.WAKE + 1, 5, -1]) > PC.MAX_STEER  # (also the held tail's)
    assert (A["plan_status"][:, 8] == 1).all() and (A["plan_status"][:, 9] == 2).all() and abs(A["rec"][PC.WAKE, 9, 4]) > PC.MAX_STEER
    assert np.abs(A["plan_oa"][:, 8]).max() > 1 and (A["plan_oa"][[63, 64, 65, 128, 129, 130], 2:5] == 0).all()
    full = results[13, 200, 64]["pt_d"]
    # (sample 0 uses nothing of the plan: the last tick, which scores that one sample, has no error)
    assert (full[PC.WAKE:-1, 5:, 2] > 0).all() and (full[:PC.WAKE, 5:, 2] == 0).all() and (full[118:124, 2:5, 2] > 0).all()
    out = PC.pack(results)
    out.update(digest=np.array(PC.digest(groups)), tol=np.float64(PC.TOL), dt=np.float64(PC.DT), tol_margin=np.float64(tol_margin),
               max_margin=np.float64(max_margin))
    np.savez_compressed(PC.FIXTURE, **out)
    size = os.path.getsize(PC.FIXTURE)
    print("wrote", PC.FIXTURE, size, "bytes")
    assert size <= os.path.getsize(os.path.join(HERE, "loop_interact_T13.npz")), size
    g = PC.fixture()
    for (T, n, S), r in results.items():
        ex = PC.expected(g, T, n, S)
        assert all(PC.same_bits(np.ascontiguousarray(ex[k]), np.ascontiguousarray(r[k])) for k in ex), (T, n, S)


if __name__ == "__main__":
    main()
