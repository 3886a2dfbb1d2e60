#!/usr/bin/env python3
"""Fixture for the stakeholder-reasons scoring at its chunk edges and table limits: the situations of
tests/reasons_edge_cases.py, written to tests/golden/reasons_edges.npz, data only.

A case goes through the REFERENCE's own evaluate_trajectories_for_reasons (:1233-1428), evaluate_trajectories_with_weights
(:1641-1864) and calculate_trajectory_completion_time (:1867-1905) of main/scenarios/overtaking_cyclist_bidirectional_road.py, loaded
as tests/golden/make_golden_reasons.py loads them, when it has the reference's parameters, the reference's layout (planned
candidates, the following one last), no candidate with a status and at most 4000 Euler steps; c{i}_ref_made says so, and the same keys
as in reasons.npz are stored (detail arrays trimmed to the longest candidate).  Every other case -- another parameter row, another
layout, a candidate with a status, the 65536 / 65537 step pair -- is stored as the numpy restatement (tests/reasons_numpy.py) makes it.
For every case the restatement's scores under all weight rows of reasons_edge_cases.ROWS are stored too, and for three cases the
1025-row sweep and the rows under another ideal.  Raw points are not stored: reasons_edge_cases.py makes them, c{i}_digest pins them.

The conditions (floor, ceil, range, timer and top-two margins) are asserted by reasons_edge_cases.cases() and their minima stored;
the restatement is checked against every reference-made case right here (1e-13).

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_reasons_edges.py"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import make_golden_reasons as MG                                     # noqa: E402
import reasons_edge_cases as E                                       # noqa: E402

KEYS = ("policymaker", "driver", "cyclist_comfort", "cyclist_time", "cyclist_combined")


def restated_arrays(res):
    """status, m, ct, avg, nb, detail, cyclist indices and in-range flags of one case's candidates as arrays (NaN / -1 / False padded)."""
    C = len(res)
    top = max([r["n_samples"] for r in res if r["status"] == 0], default=0)
    det, idx, rng = np.full((C, 5, top), np.nan), np.full((C, top), -1, dtype=np.int64), np.zeros((C, 2, top), dtype=np.bool_)
    for c, r in enumerate(res):
        if r["status"] == 0:
            m = r["n_samples"]
            for q, k in enumerate(KEYS):
                det[c, q, :len(r["detail"][k])] = r["detail"][k]
            idx[c, :m], rng[c, 0, :m], rng[c, 1, :m] = r["cyc_idx"], r["in_d"], r["in_c"]
    return {"status": np.array([r["status"] for r in res], dtype=np.int64), "m": np.array([r["n_samples"] for r in res], dtype=np.int64),
            "ct": np.array([r["ct"] if r["status"] == 0 else np.nan for r in res], dtype=np.float64), "avg": np.array([r["avg"] for r in res], dtype=np.float64).reshape(C, 4),
            "nb": np.array([r.get("nb", -1) for r in res], dtype=np.int64), "detail": det, "cyc_idx": idx, "in_range": rng}


def main():
    warnings.simplefilter("ignore", RuntimeWarning)                   # exp of a distance kilometres out of range, a division by MAX_SPEED = 0
    cases, restated = E.cases(), E.restated()
    made = [E.reference_made(c, r[0]) for c, r in zip(cases, restated)]
    O = MG.load_reference()
    from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
    from lib.simulation import State
    car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    bike = BicycleRealDimensions(skip_back_circle_collision_checking=False)
    out = {"n_cases": np.int64(len(cases)), "rows_w": np.array(E.ROWS_W), "rows_form": np.array(E.ROWS_F, dtype=np.int64), "w_fixed": np.array(E.W_FIXED),
           "other_ideal": np.array(E.OTHER_IDEAL), "sweep_cases": np.array(E.sweep_cases(), dtype=np.int64)}
    least = {k: np.inf for k in E.MARGIN}
    for i, (c, (res, scores, best)) in enumerate(zip(cases, restated)):
        for k, v in E.margins(c, res, scores).items():
            least[k] = min(least[k], v)
        mine = restated_arrays(res)
        C = len(res)
        rec = dict(mine, scores=scores[0], best=np.int64(best[0]), w_scores=scores[1], w_best=np.int64(best[1]), ct0=np.float64(res[0]["ct"] if C else np.nan))
        if made[i]:
            ego, now = c["ego"], c["now"]
            state = State(x=ego[0], y=ego[1], yaw=ego[2], v=ego[3])
            ob = [MG.Cyclist(*c["cyclist"])]
            cands = [(t, None) for t in c["candidates"]]
            _, r0 = MG.quiet(O.evaluate_trajectories_for_reasons, cands, ob, state, car, bike, now[2], now[1], now[0], time_elapsed_driver=now[3], time_passed_cyclist=now[4])
            r1 = MG.quiet(O.evaluate_trajectories_with_weights, cands, ob, state, car, bike, now[2], now[1], now[0], E.W_FIXED[0], E.W_FIXED[1], E.W_FIXED[2], now[3], now[4])
            ev, evw = r0["all_evaluations"], r1["all_evaluations"]
            rec["scores"], rec["best"] = np.array(r0["scores"], dtype=np.float64), np.int64(r0["best_idx"])
            rec["w_scores"], rec["w_best"] = np.array(r1["scores"], dtype=np.float64), np.int64(r1["best_idx"])
            rec["ct0"] = np.float64(O.calculate_trajectory_completion_time(O.compute_predicted_trajectory(state, c["candidates"][0]), state))
            rec["ct"] = np.array([e["completion_time"] for e in ev], dtype=np.float64)
            rec["avg"] = np.array([[e["avg_scores"]["policymaker"], w["avg_scores"]["policymaker"], e["avg_scores"]["driver"], e["avg_scores"]["cyclist"]]
                                   for e, w in zip(ev, evw)], dtype=np.float64)
            rec["m"] = np.array([len(e["detailed_scores"]["cyclist_comfort"]) for e in ev], dtype=np.int64)
            det = np.full((C, 5, int(rec["m"].max())), np.nan)
            for k, e in enumerate(ev):
                for q, name in enumerate(KEYS):
                    a = np.asarray(e["detailed_scores"][name], dtype=np.float64)
                    det[k, q, :len(a)] = a
            rec["detail"] = det
            # the restatement against the reference, as in make_golden_reasons.py
            assert np.array_equal(rec["m"], mine["m"]) and rec["best"] == best[0] and rec["w_best"] == best[1], c["label"]
            pairs = [(scores[0], rec["scores"]), (scores[1], rec["w_scores"]), (mine["ct"], rec["ct"]), (mine["avg"], rec["avg"]), (res[0]["ct"], rec["ct0"])]
            for a, b in pairs:
                assert np.allclose(a, b, rtol=1e-13, atol=0), (c["label"], a, b)
            assert np.allclose(mine["detail"], det, rtol=1e-13, atol=0, equal_nan=True), c["label"]
        out[f"c{i}_label"] = np.array(c["label"])
        out[f"c{i}_ref_made"] = np.bool_(made[i])
        out[f"c{i}_digest"] = np.array(E.digest(c))
        out[f"c{i}_ego"], out[f"c{i}_cyc"], out[f"c{i}_now"], out[f"c{i}_par"] = np.array(c["ego"]), np.array(c["cyclist"]), np.array(c["now"]), c["par"]
        for k, v in rec.items():
            out[f"c{i}_{k}"] = v
        out[f"c{i}_rows_scores"], out[f"c{i}_rows_best"] = scores, best.astype(np.int64)
        print(f"case {i:2d} ({c['label']}): {'reference' if made[i] else 'restatement'}, status {mine['status'].tolist()}, m {mine['m'].tolist()}, nb {mine['nb'].tolist()}")
    for k, ((_, sc, best), (_, isc, ibest)) in enumerate(zip(E.restated_sweep(), E.restated_ideal())):
        out[f"sweep{k}_scores"], out[f"sweep{k}_best"] = sc, best.astype(np.int64)
        out[f"ideal{k}_scores"], out[f"ideal{k}_best"] = isc, ibest.astype(np.int64)
    out["margins"] = np.array([least[k] for k in E.MARGIN])
    print("reference-made:", sum(made), "of", len(cases), " margins:", least)
    path = os.path.join(HERE, "reasons_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
