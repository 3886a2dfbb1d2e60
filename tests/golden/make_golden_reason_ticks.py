#!/usr/bin/env python3
"""Fixture for the per-tick stakeholder reasons and the replan trigger: the REFERENCE's own evaluate_reasons
(main/scenarios/overtaking_cyclist_bidirectional_road.py:2007-2027, with lib/reasons_evaluation.py inside) and reasons_evaluation
(:1907-1940), driven tick by tick and episode by episode on the synthetic position series of tests/reason_ticks_cases.py, written to
tests/golden/reason_ticks.npz, data only: the series, and per tick the three values, the distance, the two timers, replan_needed,
replan_tracker and the reference's own comparison results.

The scenario file is loaded as tests/golden/make_golden_reasons.py loads it.  The functions read their parameters from the classes
of lib/parameters.py; a case with another parameter row sets those attributes for its run and puts them back.  Per episode the
timers start at 0 and the tracker at False, as the script's main() starts them; episode 0 starts from the case's carry-in.  The
objects handed over are minimal: a state with .x and .y, a vehicle with get(), car dimensions with bounding_box_size.

Conditions asserted here and stored (a case that breaks one is replaced, not excused):
  every |dist - (ref + buffer)| >= 1e-9 for both ranges; every in-range timer value >= 1e-9 from its threshold, or within 1e-9 of it
  by the additions themselves (counted; the reference's comparison result is what is stored); every value >= 1e-9 from the
  threshold; x - width / 2 - centre >= 1e-9 from 0.
Restatement-made and flagged as such (`restated`, `split_*`): the case without a cyclist, the case that follows another case's
cyclist, and the carries of the two-call splits.  The restatement (tests/reason_ticks_numpy.py) is checked against every
reference-made case right here.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_reason_ticks.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reason_ticks_cases as TC                                       # noqa: E402
from make_golden_reasons import load_reference                        # noqa: E402


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Vehicle:
    def __init__(self):
        self.t = (0.0,) * 6

    def get(self):
        return self.t


def run_reference(O, P, case):
    """Per tick: values, distance (as the script's distance_values computes it), timers, needed, tracker, and the comparisons."""
    par, pos, cyc, fl = case["par"], case["pos"], case["cyc"], case["flags"]
    SP, DP, CP, RP = P.ScenarioParameters, P.DriverParameters, P.CyclistParameters, P.ReasonParameters
    saved = [(SP, "DT"), (SP, "CENTERLINE_LOCATION"), (DP, "DISTANCE_REF"), (DP, "DISTANCE_BUFFER"), (DP, "TIME_THRESHOLD"),
             (CP, "DISTANCE_REF"), (CP, "DISTANCE_BUFFER"), (CP, "TIME_THRESHOLD"), (RP, "REASONS_THRESHOLD")]
    saved = [(c, a, getattr(c, a)) for c, a in saved]
    SP.DT, SP.CENTERLINE_LOCATION = float(par[0]), float(par[3])
    DP.DISTANCE_REF, DP.DISTANCE_BUFFER, DP.TIME_THRESHOLD = float(par[5]), float(par[6]), float(par[7])
    CP.DISTANCE_REF, CP.DISTANCE_BUFFER, CP.TIME_THRESHOLD = float(par[8]), float(par[9]), float(par[10])
    RP.REASONS_THRESHOLD = case["threshold"]
    car = Obj(bounding_box_size=(float(par[4]), 4.0))
    veh = Vehicle()
    n = len(pos)
    val, timers = np.empty((n, 4)), np.empty((n, 2))
    needed, tracker_after, on = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros((n, 2), dtype=bool)
    try:
        t_d, t_c, tracker = float(case["carry"][0]), float(case["carry"][1]), bool(case["carry"][2])
        for k in range(n):
            if k > 0 and fl[k - 1] & (TC.GOAL | TC.AGE):      # a new run of the script
                t_d, t_c, tracker = 0, 0, False
            state = Obj(x=float(pos[k, 0]), y=float(pos[k, 1]))
            veh.t = (float(cyc[k, 0]), float(cyc[k, 1]), TC.V_CYC, np.pi / 2, 0.0, 0.0)
            pol, drv, cyv, t_d, t_c = O.evaluate_reasons(state, [veh], car, t_d, t_c)
            need, tracker = O.reasons_evaluation(cyv, drv, pol, False, tracker)
            val[k] = pol, drv, cyv, np.linalg.norm([veh.get()[0] - state.x, veh.get()[1] - state.y])
            timers[k] = t_d, t_c
            needed[k], tracker_after[k] = need, tracker
            on[k] = t_d >= DP.TIME_THRESHOLD, t_c >= CP.TIME_THRESHOLD   # the comparison of evaluate_time_following, same operands
    finally:
        for c, a, v in saved:
            setattr(c, a, v)
    return val, timers, needed, tracker_after, on


def main():
    cs = TC.cases()
    O = load_reference()
    import lib.parameters as P
    assert np.array_equal(TC.par_row()[[0, 3, 5, 6, 7, 8, 9, 10]],
                          [P.ScenarioParameters.DT, P.ScenarioParameters.CENTERLINE_LOCATION, P.DriverParameters.DISTANCE_REF,
                           P.DriverParameters.DISTANCE_BUFFER, P.DriverParameters.TIME_THRESHOLD, P.CyclistParameters.DISTANCE_REF,
                           P.CyclistParameters.DISTANCE_BUFFER, P.CyclistParameters.TIME_THRESHOLD])
    assert P.ReasonParameters.REASONS_THRESHOLD == 0.7
    B, N = len(cs), TC.N
    A = TC.recorder_arrays(cs)
    mine = TC.restate(A)
    val, timers = np.full((B, N, 4), np.nan), np.zeros((B, N, 2))
    needed, tracker, on = np.zeros((B, N), dtype=bool), np.zeros((B, N), dtype=bool), np.zeros((B, N, 2), dtype=bool)
    margins = {"range": np.inf, "timer": np.inf, "value": np.inf, "centre": np.inf}
    on_grid = 0
    for b, c in enumerate(cs):
        par = c["par"]
        if c["restated"]:
            val[b], timers[b] = mine["val"][:, b], mine["timers"][:, b]
            needed[b] = (mine["trig"][:, b] & 1) != 0
        else:
            val[b], timers[b], needed[b], tracker[b], on[b] = run_reference(O, P, c)
            # the restatement, which is also the source of what the launch is compared with
            assert np.array_equal(timers[b], mine["timers"][:, b]), c["label"]
            assert np.array_equal(needed[b], (mine["trig"][:, b] & 1) != 0), c["label"]
            assert np.allclose(val[b], mine["val"][:, b], rtol=1e-13, atol=0), c["label"]
            below = np.stack([val[b, :, q] < c["threshold"] for q in range(3)], axis=1)
            assert np.array_equal(below, ((mine["trig"][:, b, None] >> np.arange(1, 4)) & 1) != 0), c["label"]
            f = int(np.argmax(needed[b])) if needed[b].any() else -1
            assert f == mine["first"][b], (c["label"], f, mine["first"][b])
        if c["veh"] < 0:
            continue
        dist = val[b, :, 3]
        rng = np.array([par[5] + par[6], par[8] + par[9]])
        gap = np.abs(dist[:, None] - rng).min()
        inr = dist[:, None] < rng
        tm = np.abs(timers[b] - par[[7, 10]])[inr]
        on_grid += int((tm < 1e-9).sum())
        margins["range"] = min(margins["range"], gap)
        if (tm >= 1e-9).any():
            margins["timer"] = min(margins["timer"], tm[tm >= 1e-9].min())
        margins["value"] = min(margins["value"], np.abs(val[b, :, :3] - c["threshold"]).min())
        margins["centre"] = min(margins["centre"], np.abs((c["pos"][:, 0] - par[4] / 2) - par[3]).min())
        print(f"case {b:2d} ({c['label']}): in range {inr.sum(0).tolist()}, first on {[int(np.argmax(on[b, :, q] & inr[:, q])) if (on[b, :, q] & inr[:, q]).any() else -1 for q in range(2)]}, "
              f"needed on {np.flatnonzero(needed[b]).tolist()}")
    print("margins:", margins, " in-range timer values within 1e-9 of their threshold by the additions:", on_grid)
    assert all(m >= 1e-9 for m in margins.values()), margins
    assert on_grid > 0
    out = {"n_cases": np.int64(B), "labels": np.array([c["label"] for c in cs]), "restated": np.array([c["restated"] for c in cs]),
           "pos": np.stack([c["pos"] for c in cs]), "cyc": np.stack([c["cyc"] for c in cs]), "flags": np.stack([c["flags"] for c in cs]),
           "par": A["par"], "threshold": A["threshold"], "carry": A["carry"], "veh": np.array([c["veh"] for c in cs], dtype=np.int32),
           "val": val, "timers": timers, "needed": needed, "tracker": tracker, "on": on,
           "margins": np.array([margins["range"], margins["timer"], margins["value"], margins["centre"]]), "on_grid": np.int64(on_grid)}
    for s in TC.SPLITS:                                               # restatement-made: the carry a first piece of s ticks hands on
        out[f"split_{s}_carry"] = TC.restate(A, n=s)["carry"]
    path = os.path.join(HERE, "reason_ticks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
