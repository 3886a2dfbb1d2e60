"""Stakeholder-reasons scoring (jsim_score_trajectories, reasons.py) -- the checks that need no GPU: the numpy restatement
(tests/reasons_numpy.py, written from the contract of DESIGN.md section 14) reproduces the reference-made fixture
tests/golden/reasons.npz (sample counts, cyclist indices, in-range flags and best exact; reals within 1e-13 relative; table rows and
labels identical), the entry point is declared, exported and documented, every argument error comes from the host before any
device call, and the restatement recognises the inputs the reference has no defined behaviour for (status 2)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
import reasons_cases as RC
import reasons_numpy as RN

RTOL = 1e-13


def test_fixture_conditions_hold():
    g = RC.fixture()
    assert int(g["n_cases"]) == 12 and np.all(g["margins"] >= 1e-9)
    assert np.array_equal(g["par"], RN.DEFAULT_PAR)
    assert float(g["ref_table_1326_seconds"]) > 0 and int(g["ref_table_1326_rows"]) == 1326
    sizes = sorted(len(c["candidates"]) for c in RC.cases())
    assert sizes[0] == 2 and sizes[-1] == 8 and 4 in sizes
    raw = {len(t) for c in RC.cases() for t in c["candidates"]}
    assert {63, 64, 65, 129, 1900} <= raw
    kept = [int(m) for c in RC.cases() for m in c["ref_m"]]
    assert any(64 < m <= 128 for m in kept) and any(m > 128 for m in kept)


@pytest.mark.parametrize("i", range(12))
def test_restatement_reproduces_the_reference(i):
    case = RC.cases()[i]
    res, scores, best = RC.restated()[i]
    assert best[0] == case["ref_best"] and best[1] == case["ref_w_best"]
    assert RC.close(scores[0], case["ref_scores"], RTOL) and RC.close(scores[1], case["ref_w_scores"], RTOL)
    assert RC.close(res[0]["ct"], case["ref_ct0"], RTOL)             # calculate_trajectory_completion_time on candidate 0
    for c, r in enumerate(res):
        m = int(case["ref_m"][c])
        assert r["status"] == 0 and r["n_samples"] == m
        assert np.array_equal(r["cyc_idx"], case["ref_cyc_idx"][c, :m])
        assert np.array_equal(r["in_d"], case["ref_in_range"][c, 0, :m]) and np.array_equal(r["in_c"], case["ref_in_range"][c, 1, :m])
        assert RC.close(r["ct"], case["ref_ct"][c], RTOL) and RC.close(r["avg"], case["ref_avg"][c], RTOL)
        for q, (k, n) in enumerate(zip(RC.KEYS, (m - 1, m - 1, m, m, m - 1))):
            assert len(r["detail"][k]) == n and RC.close(r["detail"][k], case["ref_detail"][c, q, :n], RTOL), k
            assert np.all(np.isnan(case["ref_detail"][c, q, n:]))
    # the following candidate is scored with the time of the one before it
    assert res[-1]["ct"] == res[-2]["ct"]


def test_restatement_reproduces_the_tables():
    n = 0
    for case in RC.cases():
        if case["tables"] is None:
            continue
        n += 1
        C = len(case["candidates"])
        trip, prec = RN.weight_triples(0.1)
        assert len(trip) == 66
        modes, tf = RN.default_layout(C)
        _, sc, _ = RN.score_situation(case["candidates"], modes, tf, case["ego"], case["cyclist"], case["now"], case["par"], trip, [1] * 66)
        for rows, (ref_rows, ref_labels) in zip(RN.table_rows(trip, sc, prec), case["tables"]):
            assert [r[7] for r in rows] == ref_labels
            assert np.array_equal(np.array([r[:3] for r in rows]).reshape(-1, 3), ref_rows[:, :3])
            assert RC.close(np.array([r[3:7] for r in rows]).reshape(-1, 4), ref_rows[:, 3:7], RTOL)
    assert n == 3
    assert len(RN.weight_triples(0.02)[0]) == 1326


def test_restated_resample_is_the_glue_expression():
    """resample_curve keeps first and last and the points where floor(cum / dl) steps; per-point dl below MAX_SPEED."""
    P = np.stack([np.zeros(10), np.arange(10) * 0.5, np.zeros(10)], 1)
    R = RN.resample_curve(P, 1.0)
    assert np.array_equal(R[:, 1], [0.0, 1.0, 2.0, 3.0, 4.0, 4.5])
    dl = RN.resample_step(4, 0, 1.0, RN.DEFAULT_PAR)
    assert np.array_equal(dl, 0.1 * np.minimum(np.array([3.0, 5.0, 7.0, 9.0]), 30.0 / 3.6))
    assert RN.resample_step(4, 0, 9.0, RN.DEFAULT_PAR) == 0.1 * (30.0 / 3.6) and RN.resample_step(4, 1, 2.5, RN.DEFAULT_PAR) == 0.25


def test_entry_point_is_declared_exported_and_documented(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    H = pkg._header.header()
    assert H.functions["jsim_score_trajectories"].ret == "int"
    assert "evaluate_trajectories_for_reasons (:1233-1428" in hdr and "generate_stakeholder_weight_table (:1431-1604" in hdr   # what it replaces
    assert "JSIM_REASON_NPAR" in H.constants and H.constants["JSIM_MAX_CAND"] == 8 and H.constants["JSIM_ABI_VERSION"] == 2
    assert "| `jsim_score_trajectories` |" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    so = ctypes.CDLL(pkg.build.build())
    assert hasattr(so, "jsim_score_trajectories")
    assert len(pkg._cabi.load().jsim_score_trajectories.argtypes) == 23
    assert tuple(pkg.reasons.PAR_NAMES) == tuple(RN.PAR_NAMES) and np.array_equal(pkg.reasons.par_row(), RN.DEFAULT_PAR)
    for name in ("compute_predicted_trajectory", "create_following_trajectory", "balance_function", "evaluate_trajectories_for_reasons",
                 "evaluate_trajectories_with_weights", "generate_stakeholder_weight_table", "score_situations"):
        assert callable(getattr(pkg.reasons, name))


def _set(key, idx, value):
    def edit(t):
        t[key].reshape(-1)[idx] = value
    return edit


def test_argument_errors_without_gpu(pkg):
    """Every refusal of the header's list: -22 from the host, before any device call, nothing written."""
    lib = pkg._cabi.load()
    sits = [RC.situation(RC.cases()[8]), RC.situation(RC.cases()[0])]          # C = 2 and C = 4
    who = b"jsim_score_trajectories: "

    def refused(msg, **kw):
        rc, t = RC.raw_call(pkg, sits, **kw)
        err = lib.jsim_last_error(None)
        assert rc == -22 and err.startswith(who) and msg in err, (msg, rc, err)
        assert np.all(t["status"] == -7) and np.all(t["best"] == -7)
    for k in ("cand_off", "pt_off", "pts", "mode", "time_from", "ego", "cyc", "now", "par", "w", "form", "ideal", "status", "n_samples", "ct",
              "avg", "scores", "best"):
        refused(b"null argument", null=(k,))
    refused(b"cand_off[0] = 1", edit=_set("cand_off", 0, 1))
    refused(b"cand_off decreases at 0", edit=_set("cand_off", 1, -1))
    refused(b"pt_off[0] = 3", edit=_set("pt_off", 0, 3))
    refused(b"pt_off decreases at 2", edit=_set("pt_off", 3, 1))
    refused(b"time_from[1] = 2 outside its situation of 2", edit=_set("time_from", 1, 2))
    refused(b"time_from[2] = -1 outside", edit=_set("time_from", 2, -1))

    def chain(t):                                                      # situation 1: its candidate 3 -> 1 -> 0, so 1 names another
        t["time_from"][3] = 0
        t["time_from"][5] = 1
    refused(b"time_from[5] = 1 names a candidate that names another", edit=chain)
    for bad in (2, -1):
        refused(b"mode[4] = %d" % bad, edit=_set("mode", 4, bad))
        refused(b"form[0] = %d" % bad, edit=_set("form", 0, bad))
    for key, idx, v in (("pts", 7, np.nan), ("ego", 3, np.inf), ("cyc", 11, -np.inf), ("now", 4, np.nan), ("par", 13, np.nan), ("w", 1, np.inf),
                        ("ideal", 2, np.nan)):
        refused(b"a number that is not finite", edit=_set(key, idx, v))
    refused(b"situation 1: DT <= 0", edit=_set("par", 12, 0.0))
    refused(b"situation 0: DT <= 0", edit=_set("par", 0, -0.1))
    refused(b"ideal[0] <= 0", ideal=(0.0, 1 / 3, 1 / 3))                    # balance_function divides by each ideal weight
    refused(b"ideal[2] <= 0", ideal=(1 / 3, 1 / 3, -0.25))
    nine = dict(sits[1], candidates=[sits[1]["candidates"][0]] * 9)
    rc, _ = RC.raw_call(pkg, [nine])
    assert rc == -22 and b"situation 0 has 9 candidates (at most 8)" in lib.jsim_last_error(None)
    rc, _ = RC.raw_call(pkg, [])                                       # nothing to do is not an error
    assert rc == 0


def test_restatement_recognises_the_undefined_inputs():
    case = RC.cases()[0]
    ego, cyc, now, par = case["ego"], case["cyclist"], case["now"], case["par"]
    good = case["candidates"][0]
    assert RN.resample_candidate(good[:1], 0, ego, par)[0] == 2                     # fewer than 2 raw points
    assert RN.resample_candidate(good[:0], 0, ego, par)[0] == 2
    assert RN.resample_candidate(good[:3], 0, ego, par)[0] == 2                     # m < 3 (two kept points)
    assert RN.resample_candidate(good, 1, ego[:3] + (0.0,), par)[0] == 2             # following candidate at v <= 0
    assert RN.resample_candidate(good, 1, ego[:3] + (-1.0,), par)[0] == 2
    st, R = RN.resample_candidate(good, 0, ego, par)
    assert st == 0
    assert RN.score_samples(R, 0.05, cyc, now, par)["status"] == 2                  # nb < 2
    assert RN.score_samples(R, 0.15, cyc, now, par)["status"] == 0                  # nb = 2: one row, every index 0
    dense = np.stack([np.full(4000, 2.0), np.arange(4000) * 0.01, np.zeros(4000)], 1)
    assert RN.resample_candidate(dense, 1, ego[:3] + (0.05,), par)[0] == 4          # more than 320 kept
    # a candidate with a status has NaN everywhere, never wins, and its neighbours are untouched
    res, sc, best = RN.score_situation([good[:1], good, case["candidates"][2]], [0, 0, 0], [0, 1, 2], ego, cyc, now, par)
    alone, sc1, _ = RN.score_situation([good, case["candidates"][2]], [0, 0], [0, 1], ego, cyc, now, par)
    assert res[0]["status"] == 2 and np.all(np.isnan(res[0]["avg"])) and np.isnan(sc[0, 0]) and best[0] in (1, 2)
    assert np.array_equal(sc[0, 1:], sc1[0]) and np.array_equal(res[1]["avg"], alone[0]["avg"])
    _, _, none = RN.score_situation([good[:1]], [0], [0], ego, cyc, now, par)
    assert none[0] == -1
    assert RN.balance_function([1 / 3, 1 / 3, 1 / 3]) == 1.0 and RN.balance_function([0.0, 0.5, 0.5]) == 0.0
