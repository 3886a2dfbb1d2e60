"""Stakeholder-reasons scoring at its chunk edges and table limits -- the checks that need no GPU: the numpy restatement
(tests/reasons_numpy.py) reproduces every reference-made case of tests/golden/reasons_edges.npz within the 1e-13 of
test_reasons_cpu.py (statuses, sample counts, cyclist indices, in-range flags and best exact); the restatement-made cases regenerate
from tests/reasons_edge_cases.py bit for bit; what the cases cover is read from the data, not from their labels; and every margin
the cases were built with holds.  No case is left out at run time."""
import numpy as np
import pytest

import reasons_cases as RC
import reasons_edge_cases as E
import reasons_numpy as RN

RTOL = 1e-13
EDGES = (3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320)


pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")   # the restatement's exp of a distance kilometres out of range, a division by MAX_SPEED = 0


def stored(i, key):
    return E.fixture()[f"c{i}_{key}"]


def test_fixture_matches_the_generator():
    g = E.fixture()
    assert int(g["n_cases"]) == len(E.cases()) and np.array_equal(g["rows_w"], np.array(E.ROWS_W)) and g["rows_form"].tolist() == E.ROWS_F
    made = [bool(stored(i, "ref_made")) for i in range(len(E.cases()))]
    for i, (c, (res, _, _)) in enumerate(zip(E.cases(), E.restated())):
        assert str(stored(i, "label")) == c["label"] and str(stored(i, "digest")) == E.digest(c), c["label"]
        assert made[i] == E.reference_made(c, res), c["label"]
        assert np.array_equal(stored(i, "par"), c["par"]) and tuple(stored(i, "now")) == c["now"] and tuple(stored(i, "cyc")) == c["cyclist"]
    assert sum(made) >= 30 and made.count(False) >= 10


def test_restatement_reproduces_every_reference_made_case():
    n = 0
    for i, (c, (res, scores, best)) in enumerate(zip(E.cases(), E.restated())):
        if not bool(stored(i, "ref_made")):
            continue
        n += 1
        assert np.array_equal(c["par"], RN.DEFAULT_PAR) and "modes" not in c
        assert best[0] == stored(i, "best") and best[1] == stored(i, "w_best"), c["label"]
        assert RC.close(scores[0], stored(i, "scores"), RTOL) and RC.close(scores[1], stored(i, "w_scores"), RTOL), c["label"]
        assert RC.close(res[0]["ct"], stored(i, "ct0"), RTOL)
        for k, r in enumerate(res):
            m = int(stored(i, "m")[k])
            assert r["status"] == 0 == stored(i, "status")[k] and r["n_samples"] == m and r["nb"] == stored(i, "nb")[k], (c["label"], k)
            assert np.array_equal(r["cyc_idx"], stored(i, "cyc_idx")[k, :m])
            assert np.array_equal(r["in_d"], stored(i, "in_range")[k, 0, :m]) and np.array_equal(r["in_c"], stored(i, "in_range")[k, 1, :m])
            assert RC.close(r["ct"], stored(i, "ct")[k], RTOL) and RC.close(r["avg"], stored(i, "avg")[k], RTOL), (c["label"], k)
            for q, (key, cnt) in enumerate(zip(RC.KEYS, (m - 1, m - 1, m, m, m - 1))):
                assert len(r["detail"][key]) == cnt and RC.close(r["detail"][key], stored(i, "detail")[k, q, :cnt], RTOL), (c["label"], k, key)
                assert np.all(np.isnan(stored(i, "detail")[k, q, cnt:]))
        assert res[-1]["ct"] == res[-2]["ct"]                            # the following candidate with the time of the one before it
    assert n == sum(bool(stored(i, "ref_made")) for i in range(len(E.cases())))


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_restatement_made_results_regenerate_bit_for_bit():
    for i, (c, (res, scores, best)) in enumerate(zip(E.cases(), E.restated())):
        assert bits(scores, stored(i, "rows_scores")) and np.array_equal(best, stored(i, "rows_best")), c["label"]
        assert np.array_equal([r["status"] for r in res], stored(i, "status")), c["label"]
        if bool(stored(i, "ref_made")):
            continue
        assert np.array_equal([r["n_samples"] for r in res], stored(i, "m")) and np.array_equal([r.get("nb", -1) for r in res], stored(i, "nb"))
        assert bits(scores[0], stored(i, "scores")) and bits(scores[1], stored(i, "w_scores")) and best[0] == stored(i, "best") and best[1] == stored(i, "w_best")
        for k, r in enumerate(res):
            assert bits(r["avg"], stored(i, "avg")[k]), (c["label"], k)
            if r["status"] != 0:
                assert np.isnan(stored(i, "ct")[k]) and np.all(np.isnan(stored(i, "detail")[k])) and np.all(np.isnan(r["avg"])) and np.all(np.isnan(scores[:, k]))
                continue
            m = r["n_samples"]
            assert bits(r["ct"], stored(i, "ct")[k]) and np.array_equal(r["cyc_idx"], stored(i, "cyc_idx")[k, :m])
            assert np.array_equal(r["in_d"], stored(i, "in_range")[k, 0, :m]) and np.array_equal(r["in_c"], stored(i, "in_range")[k, 1, :m])
            for q, key in enumerate(RC.KEYS):
                d = r["detail"][key]
                assert bits(d, stored(i, "detail")[k, q, :len(d)]) and np.all(np.isnan(stored(i, "detail")[k, q, len(d):])), (c["label"], k, key)
    g = E.fixture()
    assert g["sweep_cases"].tolist() == E.sweep_cases() and tuple(g["other_ideal"]) == E.OTHER_IDEAL
    for k, ((_, sc, best), (_, isc, ibest)) in enumerate(zip(E.restated_sweep(), E.restated_ideal())):
        assert bits(sc, g[f"sweep{k}_scores"]) and np.array_equal(best, g[f"sweep{k}_best"]) and sc.shape[0] == 1025
        assert bits(isc, g[f"ideal{k}_scores"]) and np.array_equal(ibest, g[f"ideal{k}_best"])
        thirds = E.restated()[E.sweep_cases()[k]][1]
        assert not np.array_equal(isc, thirds, equal_nan=True)           # the other ideal changes the scores


def candidates():
    """(case, index, raw points, mode, restated result) of every candidate of every case."""
    for c, (res, _, _) in zip(E.cases(), E.restated()):
        modes, tf = E.layout(c)
        for k, (pts, md, r) in enumerate(zip(c["candidates"], modes, res)):
            yield c, k, pts, md, r


def chunks_of(flags):
    return {int(j) // 64 for j in np.nonzero(flags)[0]}


def test_coverage_is_in_the_data():
    ok = [(c, k, pts, md, r) for c, k, pts, md, r in candidates() if r["status"] == 0]
    # sample counts on and next to every chunk edge and at the table's end; one past it is status 4
    assert set(EDGES) <= {r["n_samples"] for *_, r in ok}
    assert any(r["status"] == 4 and r["n_samples"] == 321 for *_, r in candidates())
    big = [(c, md, r) for c, _, _, md, r in ok if r["n_samples"] >= 257]
    assert sum(md == 0 and c["ego"][3] < c["par"][2] for c, md, _ in big) >= 2          # the per-point step is used
    assert any(chunks_of(r["in_d"]) == {0, 1, 2, 3, 4} and chunks_of(r["in_c"]) == {0, 1, 2, 3, 4} for _, _, r in big)
    assert any({3, 4} <= chunks_of(r["in_c"]) for *_, r in ok) and any({3, 4} <= chunks_of(r["in_d"]) for *_, r in ok)
    # raw counts: a last raw chunk of 64, 1, 2 and 3 lanes; the last point kept only because it is the last, on lane 0 of a chunk
    counts = {len(pts) for _, _, pts, _, _ in candidates()}
    assert {2, 3, 64, 65, 128, 129} <= counts and {0, 1, 2, 3} <= {n % 64 for n in counts}
    forced = set()
    for c, _, pts, md, r in ok:
        k = np.floor(E.floor_ratio(pts, md, c["ego"][3], c["par"]))
        if len(pts) % 64 == 1 and k[-1] == k[-2]:
            forced.add(len(pts))
    assert {65, 129} <= forced
    # a step that keeps growing and a speed that keeps growing past the first chunk (MAX_ACCEL carried across chunks)
    assert any(md == 0 and len(pts) > 128 and c["ego"][3] + c["par"][1] * len(pts) < c["par"][2] and r["n_samples"] > 128 for c, _, pts, md, r in ok)
    assert any(md == 0 and 128 < (c["par"][2] - c["ego"][3]) / c["par"][1] < len(pts) for c, _, pts, md, r in ok)   # ... and one that saturates mid-way
    # Euler rows
    rows = {r["nb"] - 1 for *_, r in ok}
    assert {1, 2, 63, 64, 65, 127, 128, 129, RN.MAX_STEPS - 1} <= rows
    assert any(r["status"] == 4 and np.isfinite(r["ct"]) and int(np.ceil(r["ct"] / c["par"][0])) == RN.MAX_STEPS + 1 for c, _, _, _, r in candidates())
    assert any(r["n_samples"] >= 65 and r["n_samples"] > r["nb"] - 1 and len(set(r["cyc_idx"][:64]) & set(r["cyc_idx"][64:])) for *_, r in ok)
    assert any(r["nb"] - 1 > 64 * r["n_samples"] and np.min(np.diff(r["cyc_idx"])) >= 64 for *_, r in ok)
    for c, _, _, _, r in ok:
        if r["nb"] - 1 > 200:                                            # the bar's derivation: no libm call inside a long chain
            assert c["cyclist"][4] == 0.0 and c["cyclist"][5] == 0.0, c["label"]
    assert any(c["cyclist"][4] != 0.0 and c["cyclist"][5] != 0.0 and r["nb"] - 1 > 128 for c, _, _, _, r in ok)
    # timers: where each first reaches its threshold, a first in-range sample behind the first chunk, a lone sample in a chunk,
    # a timer already past its threshold over three chunks
    cross = [E.first_cross(r, c["now"], c["par"]) for c, _, _, _, r in ok]
    assert {63, 64, 128} <= {x[0] for x in cross} and {63, 64, 128} <= {x[1] for x in cross}
    assert any(np.any(r["in_d"]) and np.nonzero(r["in_d"])[0][0] >= 64 for *_, r in ok) and any(np.any(r["in_c"]) and np.nonzero(r["in_c"])[0][0] >= 64 for *_, r in ok)
    assert any(1 in [int(np.sum(r["in_c"][q:q + 64])) for q in range(0, r["n_samples"], 64)] for *_, r in ok)
    assert any(c["now"][3] >= c["par"][7] and len(chunks_of(r["in_d"])) >= 3 for c, _, _, _, r in ok)
    # parameters, layout
    assert {0.05, 0.1, 0.2} <= {float(c["par"][0]) for c in E.cases()} and len({tuple(c["par"]) for c in E.cases()}) >= 6
    for col in range(len(RN.PAR_NAMES)):
        assert len({float(c["par"][col]) for c in E.cases()}) >= 2, RN.PAR_NAMES[col]
    assert any(c["par"][1] == 0.0 and c["ego"][3] == 0.0 and r["status"] == 2 for c, _, _, md, r in candidates() if md == 0)
    assert any(r["status"] == 2 and r["n_samples"] >= 3 and not np.isfinite(RN.completion_time(r["resampled"], c["ego"][3], c["par"])) for c, _, _, _, r in candidates())
    assert sum(len(c["candidates"]) == 0 for c in E.cases()) == 1
    eight = [[r["n_samples"] for r in res] for c, (res, _, _) in zip(E.cases(), E.restated()) if len(c["candidates"]) == 8]
    assert any(len(set(ms)) == 8 and all(any(lo < m <= hi for m in ms) for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 320))) for ms in eight)
    donors = []
    for c, (res, _, _) in zip(E.cases(), E.restated()):
        _, tf = E.layout(c)
        for k, r in enumerate(res):
            if r["status"] == 0 and tf[k] != k and "modes" in c:
                own = int(np.ceil(RN.completion_time(r["resampled"], c["ego"][3], c["par"]) / c["par"][0]))
                donors.append((r["nb"] - 1, own - 1))
    assert any(used % 64 == 0 and own % 64 not in (63, 0, 1) for used, own in donors)
    # weight rows: both clamps of form 1 act on every candidate of a situation, the same rows unclamped in form 0, exact ties
    w = {(tuple(r[0]), r[1]): k for k, r in enumerate(E.ROWS)}
    hi1, lo1, hi0, lo0 = w[((0.4, 0.4, 0.4), 1)], w[((3.0, 3.0, 3.0), 1)], w[((0.4, 0.4, 0.4), 0)], w[((3.0, 3.0, 3.0), 0)]
    clamped = tied = first_ok = 0
    for c, (res, scores, best) in zip(E.cases(), E.restated()):
        good = [k for k, r in enumerate(res) if r["status"] == 0]
        if len(good) >= 2 and np.all(scores[hi0, good] > 1.0) and np.all(scores[lo0, good] < 0.0):
            assert np.all(scores[hi1, good] == 1.0) and np.all(scores[lo1, good] == 0.0) and best[hi1] == good[0] and best[lo1] == good[0]
            clamped += 1
        for a in good:
            for b in good:
                if a < b and np.array_equal(scores[:, a], scores[:, b]) and np.array_equal(res[a]["avg"], res[b]["avg"]):
                    assert not np.any(best == b)
                    tied += 1
        zero = [k for k, r in enumerate(E.ROWS) if r[0] == (0.0, 0.0, 0.0)]
        if res and res[0]["status"] == 2 and good:
            assert all(best[k] == good[0] and np.all(scores[k, good] == 0.0) for k in zero)
            first_ok += 1
    assert clamped >= 5 and tied >= 2 and first_ok >= 1
    ties = E.restated()[E.index_of("ties:")][2]
    assert set(ties.tolist()) == {0, 1}                                  # either of the two distinct candidates wins some row, never its twin
    assert E.SWEEP_W == (1, 511, 512, 513, 1025) and len(E.sweep_rows()[0]) == 1025 and E.sweep_rows()[0][:len(E.ROWS)] == E.ROWS_W
    assert E.OTHER_IDEAL != RN.IDEAL and abs(sum(E.OTHER_IDEAL) - 1.0) < 1e-15


def test_every_margin_holds():
    least = {k: np.inf for k in E.MARGIN}
    for c, (res, scores, _) in zip(E.cases(), E.restated()):
        got = E.margins(c, res, scores)
        assert all(got[k] >= E.MARGIN[k] for k in E.MARGIN), (c["label"], got)
        least = {k: min(least[k], got[k]) for k in least}
    assert np.array_equal(E.fixture()["margins"], np.array([least[k] for k in E.MARGIN]))
    assert E.MARGIN == {"floor": 1e-6, "ct": 1e-9, "range": 1e-9, "timer": 1e-9, "top": 1e-9}
    for i, (res, scores, _) in zip(E.sweep_cases() * 2, E.restated_sweep() + E.restated_ideal()):
        assert E.margins(E.cases()[i], res, scores)["top"] >= 1e-9
    # independently of margins(): the floor ratios straight from the raw points
    for c, _, pts, md, r in candidates():
        if r["status"] in (0, 4) and r["n_samples"] >= 2:
            q = E.floor_ratio(pts, md, c["ego"][3], c["par"])[1:]
            assert np.min(np.abs(q - np.round(q))) >= 1e-6, c["label"]
