"""Stakeholder-reasons scoring on the GPU (jsim_score_trajectories) at its chunk edges and table limits: the situations of
tests/reasons_edge_cases.py against tests/golden/reasons_edges.npz (reference-made where the reference can make a case, else made by
the numpy restatement tests/reasons_numpy.py) and against the restatement itself; nothing under oracle/ is imported and nothing reads
the reference.

Bar: that of test_gpu_reasons.py -- status, n_samples and best exact, `resampled` bit for bit, ct, averages, scores and the five detail
arrays within RTOL = 1e-12 relative.  Its derivation (a mean or sum of at most 320 O(1) terms accumulated in the reference's order,
behind at most ~200 Euler steps whose sin / cos come from another libm) covers these cases as follows: sample counts go up to the
table's 320; every case with more than 200 Euler rows (320, 374, 615, 284 and 65535 of them) has a cyclist with zero acceleration and
zero steering, so cos(yaw) and sin(yaw) are one constant each, kernel and restatement add the same increment in the same order, and
the only difference is the one libm result's ulp whatever the step count; the steered cyclists stay at or below 130 rows.  The
measured maximum is printed by test_edges_in_one_launch and recorded in DESIGN.md section 14.

n_samples and `resampled` of a candidate are compared wherever the restatement resamples it (status 0, 4, and 2 for too few samples or
a completion time); a candidate with no resampling step at all (fewer than 2 raw points, a step that is not positive) has status 2
and NaN in ct, averages, scores and detail like every other candidate with a status."""
import numpy as np
import pytest

import reasons_cases as RC
import reasons_edge_cases as E
import reasons_numpy as RN
from test_gpu_reasons import RTOL, same

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]   # the restatement's exp of a distance kilometres out of range, a division by MAX_SPEED = 0


@pytest.fixture(scope="module")
def sits():
    return [E.situation(c) for c in E.cases()]


@pytest.fixture(scope="module")
def launch(pkg, sits):
    """Every edge situation under reasons_edge_cases.ROWS in ONE launch, detail and resampled on; shared, never modified."""
    return pkg.reasons.score_situations(sits, E.ROWS_W, E.ROWS_F)


def part(out, i):
    """Situation i of a launch as a launch of its own."""
    a, b = int(out["cand_off"][i]), int(out["cand_off"][i + 1])
    p = {k: out[k][a:b] for k in ("status", "n_samples", "ct", "avg", "detail", "resampled")}
    p["scores"], p["best"] = out["scores"][:, a:b], out["best"][:, i:i + 1]
    return p


def stored(i, key):
    return E.fixture()[f"c{i}_{key}"]


def test_edges_in_one_launch(launch):
    worst = 0.0
    assert launch["best"].shape == (len(E.ROWS), len(E.cases()))
    for i, (c, (res, scores, best)) in enumerate(zip(E.cases(), E.restated())):
        got = part(launch, i)
        C = len(c["candidates"])
        assert got["status"].tolist() == [r["status"] for r in res] == stored(i, "status").tolist(), (c["label"], got["status"])
        assert np.array_equal(got["best"][:, 0], best) and got["best"][0, 0] == stored(i, "best") and got["best"][1, 0] == stored(i, "w_best"), (c["label"], got["best"][:, 0])
        pairs = [(got["scores"][0], stored(i, "scores")), (got["scores"][1], stored(i, "w_scores"))]
        for k, r in enumerate(res):
            R = r["resampled"]
            if R is not None:
                m = len(R)
                assert got["n_samples"][k] == m == stored(i, "m")[k], (c["label"], k, got["n_samples"][k])
                kept = min(m, RN.MAX_RES)
                assert np.array_equal(got["resampled"][k, :kept], R[:kept]) and np.all(np.isnan(got["resampled"][k, kept:])), (c["label"], k)
            if r["status"] != 0:
                assert np.isnan(got["ct"][k]) and np.all(np.isnan(got["avg"][k])) and np.all(np.isnan(got["scores"][:, k])) and np.all(np.isnan(got["detail"][k])), (c["label"], k)
                continue
            m = r["n_samples"]
            pairs += [(got["ct"][k], stored(i, "ct")[k]), (got["avg"][k], stored(i, "avg")[k]), (got["scores"][:, k], scores[:, k])]
            for q, n in enumerate((m - 1, m - 1, m, m, m - 1)):
                pairs.append((got["detail"][k, q, :n], stored(i, "detail")[k, q, :n]))
                assert np.all(np.isnan(got["detail"][k, q, n:])), (c["label"], k, q)
        if C == 0:
            assert np.all(got["best"] == -1)
        for a, b in pairs:
            ok = ~np.isnan(np.atleast_1d(b))                            # a candidate with a status: NaN on both sides, checked above
            assert np.array_equal(np.isnan(np.atleast_1d(a)), ~ok), c["label"]
            worst = max(worst, RC.rel_err(np.atleast_1d(a)[ok], np.atleast_1d(b)[ok]))
            assert RC.close(np.atleast_1d(a)[ok], np.atleast_1d(b)[ok], RTOL), (c["label"], RC.rel_err(np.atleast_1d(a)[ok], np.atleast_1d(b)[ok]))
    print(f"max relative error of the edge launch against the fixture and the restatement: {worst:.3e}")


def test_reverse_order_and_each_situation_alone_are_bit_identical(pkg, sits, launch):
    """Also the mixed-par launch against one launch per situation: the main launch carries every parameter row."""
    back = pkg.reasons.score_situations(sits[::-1], E.ROWS_W, E.ROWS_F)
    assert len({tuple(s["par"]) for s in sits}) >= 6
    for i, s in enumerate(sits):
        assert same(part(back, len(sits) - 1 - i), part(launch, i)), E.cases()[i]["label"]
        one = pkg.reasons.score_situations([s], E.ROWS_W, E.ROWS_F)
        assert same(one, part(launch, i)), E.cases()[i]["label"]


def test_weight_row_counts_around_the_workgroup_stride(pkg, sits):
    w, f = E.sweep_rows()
    three = [sits[i] for i in E.sweep_cases()]
    full = pkg.reasons.score_situations(three, w, f, detail=False, resampled=False)
    assert full["scores"].shape[0] == 1025
    for j, (res, scores, best) in enumerate(E.restated_sweep()):
        a, b = int(full["cand_off"][j]), int(full["cand_off"][j + 1])
        got = full["scores"][:, a:b]
        assert np.array_equal(np.isnan(got), np.isnan(scores)) and np.array_equal(full["best"][:, j], best), j
        assert RC.close(got[~np.isnan(got)], scores[~np.isnan(scores)], RTOL), (j, RC.rel_err(got[~np.isnan(got)], scores[~np.isnan(scores)]))
        for row in range(len(w)):                                       # row by row: the first of equal scores wins
            if not np.all(np.isnan(got[row])):
                assert full["best"][row, j] == int(np.nanargmax(got[row])), (j, row)
    for W in E.SWEEP_W[:-1]:
        head = pkg.reasons.score_situations(three, w[:W], f[:W], detail=False, resampled=False)
        assert head["scores"].shape[0] == W
        assert np.array_equal(head["scores"].view(np.uint64), full["scores"][:W].view(np.uint64)) and np.array_equal(head["best"], full["best"][:W]), W
        assert np.array_equal(head["avg"].view(np.uint64), full["avg"].view(np.uint64))


def test_another_ideal(pkg, sits, launch):
    three = [sits[i] for i in E.sweep_cases()]
    out = pkg.reasons.score_situations(three, E.ROWS_W, E.ROWS_F, ideal=E.OTHER_IDEAL, detail=False, resampled=False)
    for j, (i, (res, scores, best)) in enumerate(zip(E.sweep_cases(), E.restated_ideal())):
        a, b = int(out["cand_off"][j]), int(out["cand_off"][j + 1])
        got = out["scores"][:, a:b]
        assert np.array_equal(np.isnan(got), np.isnan(scores)) and np.array_equal(out["best"][:, j], best), j
        assert RC.close(got[~np.isnan(got)], scores[~np.isnan(scores)], RTOL)
        assert np.array_equal(out["avg"][a:b].view(np.uint64), part(launch, i)["avg"].view(np.uint64))     # the ideal touches the weight stage only
        assert not np.array_equal(got, part(launch, i)["scores"], equal_nan=True)

