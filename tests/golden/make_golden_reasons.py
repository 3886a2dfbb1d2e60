#!/usr/bin/env python3
"""Fixture for the stakeholder-reasons scoring: the REFERENCE's own functions of
main/scenarios/overtaking_cyclist_bidirectional_road.py -- create_following_trajectory (:410-445), evaluate_trajectories_for_reasons
(:1233-1428), evaluate_trajectories_with_weights (:1641-1864), generate_stakeholder_weight_table (:1431-1604, weight_step = 0.1) and
calculate_trajectory_completion_time (:1867-1905) -- run here on a dozen situations and written to tests/golden/reasons.npz, data
only: the inputs, every number the functions return, the per-sample detail arrays, the table rows and labels, and for case 0 the
wall time of the reference's 1326-triple table (weight_step = 0.02) on the machine that made the fixture.

The scenario file is loaded with importlib from CWD = main/scenarios, with a placeholder envs.arterial_multi_lanes (the real one
cannot be imported), an empty cvxpy placeholder where cvxpy is absent and matplotlib on Agg.

Candidates: synthetic lane changes at 0.083 m spacing (stored once in a pool) and trajectories of tests/golden/planner_multi.npz
(named, not stored again); the last candidate of every case is the reference's own following trajectory.

Conditions asserted here and stored (a case that breaks one is replaced, not excused):
  every sample's |dist - (ref + buffer)| >= 1e-9 for the driver's and the cyclist's range (the one discontinuous decision);
  ct / DT at least 1e-9 from an integer; no two scores of a table row with ||delta| - 1e-6| < 1e-9; the top two scores of every
  row exactly equal or >= 1e-9 apart.
The numpy restatement (tests/reasons_numpy.py) is checked against every case right here.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_reasons.py"""
import contextlib
import importlib.util
import io
import logging
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import reasons_numpy as RN                                           # noqa: E402

DL = 0.083


def find_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "scenarios")):
            return cand
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def load_reference():
    ref = find_reference()
    sys.path.insert(0, ref)
    os.chdir(os.path.join(ref, "scenarios"))
    import matplotlib
    matplotlib.use("Agg")
    try:
        import cvxpy                                                  # noqa: F401
    except Exception:
        sys.modules["cvxpy"] = types.ModuleType("cvxpy")
    import envs                                                       # noqa: F401
    stub = types.ModuleType("envs.arterial_multi_lanes")
    stub.ArterialMultiLanes = object
    sys.modules["envs.arterial_multi_lanes"] = stub
    spec = importlib.util.spec_from_file_location("ref_overtaking", os.path.join(ref, "scenarios", "overtaking_cyclist_bidirectional_road.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    logging.disable(logging.CRITICAL)
    return mod


def lane_change(n, x0, x1, y0, start=3.0, length=10.0):
    s = np.arange(n) * DL
    y = y0 + s
    x = x0 + (x1 - x0) * 0.5 * (1 - np.cos(np.pi * np.clip((s - start) / length, 0, 1)))
    th = np.arctan2(np.gradient(y), np.gradient(x))
    return np.stack([x, y, th], 1)


class Cyclist:
    def __init__(self, *a):
        self.a = tuple(float(v) for v in a)

    def get(self):
        return self.a


# pool of synthetic candidates: (n, x0, x1, y0); raw lengths 63, 64, 65, 129 sit on the edges of a wavefront's 64-point chunks
POOL = [(500, 2.0, -2.0, -20.0), (420, 2.0, -0.5, -20.0), (480, 2.0, 2.0, -20.0), (63, 2.0, 1.0, -20.0), (64, 2.0, 0.5, -20.0),
        (65, 2.0, 2.0, -20.0), (129, 2.0, -1.0, -20.0), (1000, 2.0, -2.0, -20.0), (1900, 2.0, -1.5, -20.0), (300, 2.0, -3.0, -20.0),
        (350, 2.0, 0.2, -20.0), (380, 2.0, 1.2, -20.0), (330, 2.0, -1.2, -20.0), (310, 2.0, 3.0, -20.0)]
N = np.pi / 2
# (label, candidate sources, ego (x, y, yaw, v), cyclist get() tuple, (now_p, now_d, now_c, t_driver, t_cyclist), table?)
CASES = [
    ("base: C = 4, both timers cross their thresholds", ["pool:0", "pool:1", "pool:2"], (2.0, -20.0, N, 1.4), (2.0, -12.0, 5 / 3.6, N, 0.0, 0.0), (0.9, 0.8, 1.0, 7.5, 4.0), True),
    ("v above MAX_SPEED, raw 63 / 64 / 65", ["pool:3", "pool:4", "pool:5"], (2.0, -20.0, N, 8.5), (2.0, -17.0, 5 / 3.6, N, 0.0, 0.0), (1.0, 0.95, 0.7, 2.0, 1.0), True),
    ("raw 129 and 1900 (more than 128 kept)", ["pool:6", "pool:8", "pool:0"], (2.0, -20.0, N, 3.0), (2.0, -10.37, 5 / 3.6, N, 0.0, 0.0), (0.8, 0.9, 0.85, 0.0, 0.0), False),
    ("planner trajectories", ["pm:s0_c0_traj", "pm:s0_c1_traj", "pm:s0_c2_traj"], (3.0, -30.0, N, 2.0), (3.0, -22.0, 5 / 3.6, N, 0.0, 0.0), (1.0, 1.0, 1.0, 6.0, 4.5), True),
    ("cyclist accelerating and steering", ["pool:0", "pool:1", "pool:2"], (2.0, -20.0, N, 1.0), (2.5, -13.0, 1.2, N + 0.1, 0.3, -0.05), (0.9, 0.9, 0.9, 7.9, 4.9), False),
    ("cyclist out of range of every candidate", ["pool:0", "pool:2"], (2.0, -20.0, N, 4.0), (60.0, -12.0, 5 / 3.6, N, 0.0, 0.0), (0.6, 0.7, 0.8, 9.0, 6.0), False),
    ("far left of the centreline", ["pool:9", "pool:12", "pool:13"], (2.0, -20.0, N, 5.0), (2.0, -14.0, 5 / 3.6, N, 0.0, 0.0), (0.75, 0.85, 0.95, 7.95, 4.95), False),
    ("slow ego, 1000 raw points (more than 64 kept)", ["pool:7", "pool:0"], (2.0, -20.0, N, 0.2), (2.0, -15.0, 5 / 3.6, N, 0.0, 0.0), (0.9, 0.8, 1.0, 3.0, 1.0), False),
    ("C = 2", ["pool:1"], (2.0, -20.0, N, 2.5), (2.0, -12.0, 5 / 3.6, N, 0.0, 0.0), (0.9, 0.8, 1.0, 7.0, 3.0), False),
    ("C = 8", ["pool:0", "pool:1", "pool:2", "pool:9", "pool:10", "pool:11", "pool:12"], (2.0, -20.0, N, 1.7), (2.0, -11.0, 5 / 3.6, N, 0.0, 0.0), (0.9, 0.8, 1.0, 7.5, 4.0), False),
    ("v exactly MAX_SPEED", ["pool:0", "pool:10", "pool:11"], (2.0, -20.0, N, 30.0 / 3.6), (2.0, -5.23, 5 / 3.6, N, 0.0, 0.0), (0.9, 0.8, 1.0, 7.8, 4.7), False),
    ("planner left turns, timers far past their thresholds", ["pm:s1_c0_traj", "pm:s1_c2_traj", "pm:s2_c4_traj"], (3.0, -30.0, N, 1.2), (3.0, -25.31, 5 / 3.6, N, 0.0, 0.0), (0.5, 0.4, 0.3, 12.0, 9.0), False),
]
W_FIXED = (0.2, 0.5, 0.3)                                            # (policy, driver, cyclist) of the evaluate_trajectories_with_weights call


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    pm = np.load(os.path.join(HERE, "planner_multi.npz"))
    pool = [lane_change(*p) for p in POOL]
    O = load_reference()
    from lib.car_dimensions import BicycleModelDimensions, BicycleRealDimensions
    from lib.parameters import CyclistParameters as CP, DriverParameters as DP, ScenarioParameters as SP
    from lib.simulation import State
    car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    bike = BicycleRealDimensions(skip_back_circle_collision_checking=False)
    par = np.array([SP.DT, O.MAX_ACCEL, O.Simulation.MAX_SPEED, SP.CENTERLINE_LOCATION, car.bounding_box_size[0], DP.DISTANCE_REF, DP.DISTANCE_BUFFER,
                    DP.TIME_THRESHOLD, CP.DISTANCE_REF, CP.DISTANCE_BUFFER, CP.TIME_THRESHOLD, bike.distance_back_to_front_wheel], dtype=np.float64)
    assert np.array_equal(par, RN.DEFAULT_PAR), par
    out = {"n_cases": np.int64(len(CASES)), "par": par, "w_fixed": np.array(W_FIXED), "n_pool": np.int64(len(pool))}
    for k, p in enumerate(pool):
        out[f"pool_{k}"] = p
    margins = {"range": np.inf, "ct": np.inf, "label": np.inf, "top": np.inf}
    keys = ("policymaker", "driver", "cyclist_comfort", "cyclist_time", "cyclist_combined")

    def check_rows(rows):
        for r in rows:
            s = np.sort(np.asarray(r, dtype=np.float64))
            for a in range(len(s)):
                for b in range(a + 1, len(s)):
                    margins["label"] = min(margins["label"], abs(abs(s[b] - s[a]) - 1e-6))
            if len(s) > 1 and s[-1] != s[-2]:
                margins["top"] = min(margins["top"], s[-1] - s[-2])

    for i, (label, src, ego, cyc, now, table) in enumerate(CASES):
        planned = [pool[int(s[5:])] if s.startswith("pool:") else np.asarray(pm[s[3:]], dtype=np.float64) for s in src]
        state = State(x=ego[0], y=ego[1], yaw=ego[2], v=ego[3])
        ob = [Cyclist(*cyc)]
        cands = [(t, None) for t in planned]
        follow = O.create_following_trajectory(state, cands)
        cands.append((follow, (0.0,) * 5))
        C = len(cands)
        _, res = quiet(O.evaluate_trajectories_for_reasons, cands, ob, state, car, bike, now[2], now[1], now[0], time_elapsed_driver=now[3], time_passed_cyclist=now[4])
        rw = quiet(O.evaluate_trajectories_with_weights, cands, ob, state, car, bike, now[2], now[1], now[0], W_FIXED[0], W_FIXED[1], W_FIXED[2], now[3], now[4])
        ct0 = O.calculate_trajectory_completion_time(O.compute_predicted_trajectory(state, planned[0]), state)
        out[f"c{i}_label"] = np.array(label)
        out[f"c{i}_src"] = np.array(src)
        out[f"c{i}_follow"] = np.asarray(follow, dtype=np.float64)
        out[f"c{i}_ego"] = np.array(ego, dtype=np.float64)
        out[f"c{i}_cyc"] = np.array(cyc, dtype=np.float64)
        out[f"c{i}_now"] = np.array(now, dtype=np.float64)
        out[f"c{i}_scores"] = np.array(res["scores"], dtype=np.float64)
        out[f"c{i}_best"] = np.int64(res["best_idx"])
        out[f"c{i}_w_scores"] = np.array(rw["scores"], dtype=np.float64)
        out[f"c{i}_w_best"] = np.int64(rw["best_idx"])
        out[f"c{i}_ct0"] = np.float64(ct0)
        ev, evw = res["all_evaluations"], rw["all_evaluations"]
        out[f"c{i}_ct"] = np.array([e["completion_time"] for e in ev], dtype=np.float64)
        out[f"c{i}_avg"] = np.array([[e["avg_scores"]["policymaker"], w["avg_scores"]["policymaker"], e["avg_scores"]["driver"], e["avg_scores"]["cyclist"]]
                                     for e, w in zip(ev, evw)], dtype=np.float64)
        m = np.array([len(e["detailed_scores"]["cyclist_comfort"]) for e in ev], dtype=np.int64)
        out[f"c{i}_m"] = m
        det = np.full((C, 5, int(m.max())), np.nan)
        for c, e in enumerate(ev):
            for q, name in enumerate(keys):
                a = np.asarray(e["detailed_scores"][name], dtype=np.float64)
                det[c, q, :len(a)] = a
        out[f"c{i}_detail"] = det
        check_rows([res["scores"], rw["scores"]])
        # the restatement on the same inputs (also the source of the per-sample distances the range condition is about)
        modes, tf = RN.default_layout(C)
        mine, sc, best = RN.score_situation([t for t, _ in cands], modes, tf, ego, cyc, now, par, [(1 / 9, 4 / 9, 4 / 9), W_FIXED], [0, 1])
        assert best[0] == res["best_idx"] and best[1] == rw["best_idx"], label
        assert np.allclose(sc[0], res["scores"], rtol=1e-13, atol=0) and np.allclose(sc[1], rw["scores"], rtol=1e-13, atol=0), label
        cyc_idx = np.full((C, int(m.max())), -1, dtype=np.int64)
        in_rng = np.zeros((C, 2, int(m.max())), dtype=np.bool_)
        for c, r in enumerate(mine):
            assert r["status"] == 0 and r["n_samples"] == m[c], (label, c, r["status"], r["n_samples"], m[c])
            assert np.allclose(r["ct"], out[f"c{i}_ct"][c], rtol=1e-13, atol=0) and np.allclose(r["avg"], out[f"c{i}_avg"][c], rtol=1e-13, atol=0), (label, c)
            for q, name in enumerate(keys):
                assert np.allclose(r["detail"][name], det[c, q, :len(r["detail"][name])], rtol=1e-13, atol=0), (label, c, name)
            gap = min(np.abs(r["dist"] - (par[5] + par[6])).min(), np.abs(r["dist"] - (par[8] + par[9])).min())
            assert gap >= 1e-9, (label, c, gap)
            margins["range"] = min(margins["range"], gap)
            q = r["ct"] / par[0]
            margins["ct"] = min(margins["ct"], abs(q - np.round(q)))
            cyc_idx[c, :m[c]] = r["cyc_idx"]
            in_rng[c, 0, :m[c]], in_rng[c, 1, :m[c]] = r["in_d"], r["in_c"]
        out[f"c{i}_cyc_idx"] = cyc_idx
        out[f"c{i}_in_range"] = in_rng
        out[f"c{i}_has_table"] = np.bool_(table)
        if table:
            tabs = quiet(O.generate_stakeholder_weight_table, cands, ob, state, car, bike, now[2], now[1], now[0], now[3], now[4], weight_step=0.1)
            for name, rows in zip(("policy", "driver", "cyclist"), tabs):
                out[f"c{i}_table_{name}"] = np.array([r[:7] for r in rows], dtype=np.float64).reshape(-1, 7)
                out[f"c{i}_table_{name}_label"] = np.array([r[7] for r in rows])
                check_rows([r[3:3 + min(C, 4)] for r in rows])
            trip, prec = RN.weight_triples(0.1)
            _, sc_t, _ = RN.score_situation([t for t, _ in cands], modes, tf, ego, cyc, now, par, trip, [1] * len(trip))
            for rows, ref_rows in zip(RN.table_rows(trip, sc_t[:, :C], prec), tabs):
                assert [r[:3] + r[7:] for r in rows] == [r[:3] + r[7:] for r in ref_rows], label
                assert np.allclose([r[3:7] for r in rows], [r[3:7] for r in ref_rows], rtol=1e-13, atol=0), label
        if i == 0:
            t0 = time.perf_counter()
            tabs = quiet(O.generate_stakeholder_weight_table, cands, ob, state, car, bike, now[2], now[1], now[0], now[3], now[4], weight_step=0.02)
            out["ref_table_1326_seconds"] = np.float64(time.perf_counter() - t0)
            out["ref_table_1326_rows"] = np.int64(sum(len(t) for t in tabs))
            assert out["ref_table_1326_rows"] == 1326
        print(f"case {i:2d} ({label}): C {C}, m {m.tolist()}, ct {np.round(out[f'c{i}_ct'], 3).tolist()}, best {res['best_idx']} / {rw['best_idx']}")
    print("margins:", margins, " reference 1326-row table:", float(out["ref_table_1326_seconds"]), "s")
    assert margins["range"] >= 1e-9 and margins["ct"] >= 1e-9 and margins["label"] >= 1e-9 and margins["top"] >= 1e-9, margins
    out["margins"] = np.array([margins["range"], margins["ct"], margins["label"], margins["top"]])
    path = os.path.join(HERE, "reasons.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
