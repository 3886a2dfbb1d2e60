"""Stakeholder-reasons scoring on the GPU (jsim_score_trajectories, reasons.py) against the reference-made fixture
tests/golden/reasons.npz and the numpy restatement tests/reasons_numpy.py; nothing under oracle/ is imported.

Bar: status, n_samples and best exact; ct, averages, scores and the five detail arrays within 1e-12 relative.  Derivation: a result
is a mean or a sum of at most 320 O(1) terms accumulated in the reference's order, behind at most ~200 Euler steps whose sin / cos
and the scores' exp come from another libm (a few ulp each, 2.2e-16); errors add at worst linearly: 320 x 4 ulp ~ 3e-13 for a sum
that is then divided by its count, ~1e-14 typical -- 1e-12 leaves about 100 x headroom.  The measured maximum is printed by test_fixture_in_one_launch and recorded in DESIGN.md section 14.
This fixture stays at 191 samples and 191 Euler steps; test_gpu_reasons_edges.py takes the same bar to the table's 320 samples and
to 65535 Euler steps, where every cyclist with more than 200 steps has zero acceleration and steering: sin / cos are then one
constant each, both sides add the same increment in the same order, and the step count does not enter the error."""
import numpy as np
import pytest

import reasons_cases as RC
import reasons_numpy as RN

pytestmark = pytest.mark.gpu
RTOL = 1e-12
OUT_KEYS = ("status", "n_samples", "ct", "avg", "scores", "best", "detail", "resampled")


def same(a, b):
    """Bit for bit, NaN patterns included."""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in OUT_KEYS)


@pytest.fixture(scope="module")
def rows():
    trip, _ = RN.weight_triples(0.1)
    return [RC.FIXED_ROW, tuple(RC.fixture()["w_fixed"])] + trip, [0, 1] + [1] * len(trip)


@pytest.fixture(scope="module")
def sits():
    return [RC.situation(c) for c in RC.cases()]


@pytest.fixture(scope="module")
def launch(pkg, sits, rows):
    """All fixture situations, the two reference rows and the 66-triple table in ONE launch; shared, never modified."""
    return pkg.reasons.score_situations(sits, rows[0], rows[1])


def test_fixture_in_one_launch(launch):
    worst = 0.0
    off = launch["cand_off"]
    for i, case in enumerate(RC.cases()):
        a, b = int(off[i]), int(off[i + 1])
        assert np.all(launch["status"][a:b] == 0) and np.array_equal(launch["n_samples"][a:b], case["ref_m"])
        assert launch["best"][0, i] == case["ref_best"] and launch["best"][1, i] == case["ref_w_best"]
        pairs = [(launch["ct"][a:b], case["ref_ct"]), (launch["avg"][a:b], case["ref_avg"]), (launch["scores"][0, a:b], case["ref_scores"]),
                 (launch["scores"][1, a:b], case["ref_w_scores"])]
        for c in range(b - a):
            m = int(case["ref_m"][c])
            for q, n in enumerate((m - 1, m - 1, m, m, m - 1)):
                pairs.append((launch["detail"][a + c, q, :n], case["ref_detail"][c, q, :n]))
                assert np.all(np.isnan(launch["detail"][a + c, q, n:]))
        for got, want in pairs:
            worst = max(worst, RC.rel_err(got, want))
            assert RC.close(got, want, RTOL), (case["label"], RC.rel_err(got, want))
    print(f"max relative error against the reference: {worst:.3e}")


def test_resampled_is_bit_identical_to_the_restatement(launch):
    off = launch["cand_off"]
    for i, case in enumerate(RC.cases()):
        modes, _ = RN.default_layout(len(case["candidates"]))
        for c, (pts, md) in enumerate(zip(case["candidates"], modes)):
            st, R = RN.resample_candidate(pts, md, case["ego"], case["par"])
            got = launch["resampled"][off[i] + c]
            assert st == 0 and np.array_equal(got[:len(R)], R) and np.all(np.isnan(got[len(R):])), (case["label"], c)


def test_one_launch_equals_one_launch_per_situation(pkg, sits, rows, launch):
    off = launch["cand_off"]
    for i, s in enumerate(sits):
        one = pkg.reasons.score_situations([s], rows[0], rows[1])
        a, b = int(off[i]), int(off[i + 1])
        part = {k: launch[k][a:b] for k in ("status", "n_samples", "ct", "avg", "detail", "resampled")}
        part["scores"], part["best"] = launch["scores"][:, a:b], launch["best"][:, i:i + 1]
        assert same(one, part), i


def test_order_of_situations_and_weight_chunks_do_not_matter(pkg, sits, rows, launch):
    back = pkg.reasons.score_situations(sits[::-1], rows[0], rows[1], detail=False, resampled=False)
    off = launch["cand_off"]
    pos = 0
    for i in reversed(range(len(sits))):
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(back["scores"][:, pos:pos + b - a], launch["scores"][:, a:b]) and np.array_equal(back["avg"][pos:pos + b - a], launch["avg"][a:b])
        assert np.array_equal(back["best"][:, len(sits) - 1 - i], launch["best"][:, i])
        pos += b - a
    trip, _ = RN.weight_triples(0.02)
    assert len(trip) == 1326
    forms = [k % 2 for k in range(1326)]                                   # mixed forms
    three = sits[:3]
    big = pkg.reasons.score_situations(three, trip, forms, detail=False, resampled=False)
    assert big["scores"].shape == (1326, int(big["cand_off"][-1])) and not np.any(np.isnan(big["scores"]))
    for lo, hi in ((0, 1), (1, 67), (67, 1326)):                          # W = 1, 66 and the rest
        part = pkg.reasons.score_situations(three, trip[lo:hi], forms[lo:hi], detail=False, resampled=False)
        assert np.array_equal(part["scores"], big["scores"][lo:hi]) and np.array_equal(part["best"], big["best"][lo:hi])
    # against the restatement, row by row of the full grid for one situation
    c = RC.cases()[0]
    modes, tf = RN.default_layout(len(c["candidates"]))
    _, sc, best = RN.score_situation(c["candidates"], modes, tf, c["ego"], c["cyclist"], c["now"], c["par"], trip, forms)
    n = len(c["candidates"])
    assert RC.close(big["scores"][:, :n], sc, RTOL) and np.array_equal(big["best"][:, 0], best)


def test_time_from(pkg, sits, rows, launch):
    s = sits[0]
    C = len(s["candidates"])
    pair = dict(s, candidates=[s["candidates"][C - 2], s["candidates"][C - 1]], modes=[0, 1], time_from=[0, 0])
    two = pkg.reasons.score_situations([pair], rows[0], rows[1])
    for k in ("ct", "avg", "detail", "resampled", "n_samples"):
        assert np.array_equal(two[k][1], launch[k][C - 1], equal_nan=True) and np.array_equal(two[k][0], launch[k][C - 2], equal_nan=True), k
    assert np.array_equal(two["scores"][:, 1], launch["scores"][:, C - 1]) and two["ct"][1] == two["ct"][0]
    lone = pkg.reasons.score_situations([dict(s, candidates=[s["candidates"][0]], modes=[0], time_from=[0])], rows[0], rows[1])
    assert lone["ct"][0] == launch["ct"][0] and np.array_equal(lone["avg"][0], launch["avg"][0]) and np.all(lone["best"] == 0)
    own = pkg.reasons.score_situations([dict(s, time_from=list(range(C)))], rows[0], rows[1])     # the following one with its own time
    assert own["ct"][C - 1] != launch["ct"][C - 1] and np.array_equal(own["avg"][:C - 1], launch["avg"][:C - 1])


def test_status_2_and_4_give_nan_and_never_win(pkg, rows):
    case = RC.cases()[0]
    ego = case["ego"][:3] + (0.05,)
    good, other = case["candidates"][0], case["candidates"][2]
    dense = np.stack([np.full(4000, 2.0), -20.0 + np.arange(4000) * 0.01, np.full(4000, np.pi / 2)], 1)
    base = {"ego": ego, "cyclist": case["cyclist"], "now": case["now"], "par": case["par"]}
    clean = pkg.reasons.score_situations([dict(base, candidates=[good, other], modes=[0, 0], time_from=[0, 1])], rows[0], rows[1])
    assert np.all(clean["status"] == 0)
    mixed = pkg.reasons.score_situations([dict(base, candidates=[good[:1], good, dense, other, good[:3], good[:0]], modes=[0, 0, 1, 0, 0, 0],
                                               time_from=[0, 1, 2, 3, 4, 5])], rows[0], rows[1])
    assert mixed["status"].tolist() == [2, 0, 4, 0, 2, 2]
    for c in (0, 2, 4, 5):
        assert np.all(np.isnan(mixed["avg"][c])) and np.isnan(mixed["ct"][c]) and np.all(np.isnan(mixed["scores"][:, c])) and np.all(np.isnan(mixed["detail"][c]))
    assert set(np.unique(mixed["best"])) <= {1, 3}
    for k in ("ct", "avg", "detail", "resampled", "n_samples"):
        assert np.array_equal(mixed[k][[1, 3]], clean[k], equal_nan=True), k
    assert np.array_equal(mixed["scores"][:, [1, 3]], clean["scores"]) and np.array_equal(mixed["best"] == 3, clean["best"] == 1)
    # a candidate whose donor has a status, a following candidate at v = 0, a completion time of less than two steps
    dep = pkg.reasons.score_situations([dict(base, candidates=[good[:1], case["candidates"][-1]], modes=[0, 1], time_from=[0, 0])], rows[0], rows[1])
    assert dep["status"].tolist() == [2, 2] and np.all(dep["best"] == -1)
    still = pkg.reasons.score_situations([dict(base, ego=ego[:3] + (0.0,), candidates=[good, good], modes=[0, 1], time_from=[0, 0])], rows[0], rows[1])
    assert still["status"].tolist() == [0, 2]
    fast = ego[:3] + (7.0,)                                             # 0.83 m in steps of 0.7 m: three points, 0.0996 s, one step of DT
    short = pkg.reasons.score_situations([dict(base, ego=fast, candidates=[good[:11]], modes=[1], time_from=[0])], rows[0], rows[1])
    assert short["status"].tolist() == [2] and short["n_samples"][0] == 3
    assert RN.score_situation([good[:11]], [1], [0], fast, case["cyclist"], case["now"], case["par"])[0][0]["status"] == 2
    with pytest.raises(ValueError):
        pkg.reasons.evaluate_trajectories_for_reasons([(good[:1], None), (good, None)], [RC.Cyclist(case["cyclist"])], RC.State(*ego), None, None,
                                                      case["now"][2], case["now"][1], case["now"][0])


def test_python_surface_reproduces_the_reference(pkg):
    R = pkg.reasons
    for case in RC.cases():
        if case["tables"] is None:
            continue
        cands = [(t, None) for t in case["candidates"]]
        state, ob, now = RC.State(*case["ego"]), [RC.Cyclist(case["cyclist"])], case["now"]
        weights, res = R.evaluate_trajectories_for_reasons(cands, ob, state, None, None, now[2], now[1], now[0], time_elapsed_driver=now[3],
                                                           time_passed_cyclist=now[4])
        assert weights == {"policymaker": 1 / 9, "driver": 4 / 9, "cyclist": 4 / 9}
        wf = RC.fixture()["w_fixed"]
        rw = R.evaluate_trajectories_with_weights(cands, ob, state, None, None, now[2], now[1], now[0], wf[0], wf[1], wf[2], now[3], now[4])
        for got, scores, best, col in ((res, case["ref_scores"], case["ref_best"], 0), (rw, case["ref_w_scores"], case["ref_w_best"], 1)):
            assert set(got) == {"scores", "best_idx", "best_trajectory", "best_evaluation", "all_evaluations"}
            assert RC.close(got["scores"], scores, RTOL) and got["best_idx"] == best and got["best_trajectory"] is cands[int(best)]
            assert got["best_evaluation"] is got["all_evaluations"][int(best)]
            for c, e in enumerate(got["all_evaluations"]):
                m = int(case["ref_m"][c])
                assert e["trajectory_idx"] == c and RC.close(e["completion_time"], case["ref_ct"][c], RTOL) and RC.close(e["total_score"], scores[c], RTOL)
                assert RC.close([e["avg_scores"][k] for k in ("policymaker", "driver", "cyclist")], case["ref_avg"][c][[col, 2, 3]], RTOL)
                for q, (k, n) in enumerate(zip(RC.KEYS, (m - 1, m - 1, m, m, m - 1))):
                    assert len(e["detailed_scores"][k]) == n and RC.close(e["detailed_scores"][k], case["ref_detail"][c, q, :n], RTOL)
        tabs = R.generate_stakeholder_weight_table(cands, ob, state, None, None, now[2], now[1], now[0], now[3], now[4], weight_step=0.1)
        for rows_, (ref_rows, ref_labels) in zip(tabs, case["tables"]):
            assert [r[7] for r in rows_] == ref_labels and np.array_equal(np.array([r[:3] for r in rows_]).reshape(-1, 3), ref_rows[:, :3])
            assert RC.close(np.array([r[3:7] for r in rows_]).reshape(-1, 4), ref_rows[:, 3:7], RTOL)
        zero = R.evaluate_trajectories_with_weights(cands, ob, state, None, None, now[2], now[1], now[0], 0.0, 0.0, 0.0)
        assert zero["scores"] == [0.0] * len(cands) and zero["best_idx"] == 0 and zero["all_evaluations"] == []


def test_create_following_trajectory(pkg):
    for case in RC.cases():
        follow = pkg.reasons.create_following_trajectory(RC.State(*case["ego"]), [(t, None) for t in case["candidates"][:-1]])
        assert follow.shape == case["ref_follow"].shape and RC.close(follow, case["ref_follow"], RTOL), case["label"]
    c = RC.cases()[0]
    R0 = pkg.reasons.compute_predicted_trajectory(RC.State(*c["ego"]), c["candidates"][0])
    assert np.array_equal(R0, RN.resample_candidate(c["candidates"][0], 0, c["ego"], c["par"])[1])
    R1 = pkg.reasons.compute_predicted_trajectory(RC.State(*c["ego"]), c["candidates"][-1], last_index=True)
    assert np.array_equal(R1, RN.resample_candidate(c["candidates"][-1], 1, c["ego"], c["par"])[1])


def test_weight_rows_on_the_device(pkg, sits):
    """A row of three zeros: all scores 0 and best 0; the balance factor is the Python function's."""
    w = [(0.0, 0.0, 0.0), (1 / 3, 1 / 3, 1 / 3), (0.5, 0.5, 0.0), (0.2, 0.5, 0.3)]
    out = pkg.reasons.score_situations(sits[:1], w, [1, 1, 0, 0], detail=False, resampled=False)
    assert np.all(out["scores"][0] == 0.0) and out["best"][0, 0] == 0 and np.all(out["scores"][2] == 0.0)
    avg = out["avg"]
    bal = pkg.reasons.balance_function([0.3, 0.5, 0.2], [1 / 3] * 3)
    assert RC.close(out["scores"][3], bal * ((0.2 * avg[:, 0] + 0.5 * avg[:, 2]) + 0.3 * avg[:, 3]), 1e-15)
    assert RC.close(out["scores"][1], np.clip(((1 / 3) * avg[:, 1] + (1 / 3) * avg[:, 2]) + (1 / 3) * avg[:, 3], 0, 1), 1e-15)


@pytest.mark.parametrize("S", [1, 3, 65])
def test_batch_sizes(pkg, sits, rows, launch, S):
    pick = [k % len(sits) for k in range(S)]
    out = pkg.reasons.score_situations([sits[k] for k in pick], rows[0], rows[1], detail=False)
    off, ref_off = out["cand_off"], launch["cand_off"]
    assert out["best"].shape == (len(rows[0]), S)
    for j, k in enumerate(pick):
        a, b, ra, rb = int(off[j]), int(off[j + 1]), int(ref_off[k]), int(ref_off[k + 1])
        assert np.array_equal(out["scores"][:, a:b], launch["scores"][:, ra:rb]) and np.array_equal(out["best"][:, j], launch["best"][:, k])
        assert np.array_equal(out["avg"][a:b], launch["avg"][ra:rb]) and np.array_equal(out["resampled"][a:b], launch["resampled"][ra:rb], equal_nan=True)
