"""Static-obstacle clearance and contact per recorded tick on the device (jsim_loop_eval_static, Recorder.static_conflicts,
DESIGN.md section 18): all fixture cases as one launch -- a different obstacle set per ego -- against the reference-made fixture at
each of the nine tick counts and both hidden settings; the batch layout (every ego alone, the order reversed); a set_of outside the
sets; the empty call; and a ScenarioLoop of four egos, one per start position, each against its own scenario's obstacles, against
the restatement on the recorder's own arrays and against the same ticks driven by tick().

Bars: hit, who and off_tick exact; clear within 1e-12 x max(1, |clear|) -- coordinates below 100 m (ulp 1.4e-14) behind one sincos,
unfused sums and one sqrt, section 17's bar.  The fixture keeps every deciding half-plane value and every pair of competing
clearances 1e-9 apart outside its three exact cases, whose values (yaw 0 and pi / 2, sums that round to the same double on any
sincos that is good to an ulp) are exact on the device as well."""
import numpy as np
import pytest
import torch

import static_cases as SC
import static_numpy as SN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine, sub_batch  # noqa: F401

pytestmark = pytest.mark.gpu
BAR = 1e-12
KEYS = ("clear", "who", "hit", "off_tick")
SPEC = [(k, np.float64, (), -8.5e85) if k == "clear" else (k, np.int32, (), -85) for k in KEYS]   # (the poison: values no output can take)


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return SC.recorder_arrays(SC.cases())


def launch(pkg, eng, A, hidden, n=SC.N, egos=None, set_of=None):
    """jsim_loop_eval_static on the first n ticks of recorder arrays (egos: these egos only, in this order) against the fixture's
    tables, on guarded outputs (gpu_helpers.guarded_outputs).  Returns numpy outputs."""
    g = SC.fixture()
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    B = len(idx)
    dev = eng.device
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    m = max(n, 1)
    rec, flags = up(A["rec"][:m, idx]), up(A["flags"][:m, idx], np.int32)
    xf, xs = up(A["x_first"][idx]), up(A["x_spawn"][idx])
    sof = up(A["set_of"][idx] if set_of is None else set_of, np.int32)
    rows, off, ego = np.ascontiguousarray(g["rows"]), np.ascontiguousarray(g["set_off"], dtype=np.int32), np.array(SC.CAR)
    out, buf = guarded_outputs(SPEC, n, B, dev)
    p = lambda t: t.data_ptr()
    rc = eng.lib.jsim_loop_eval_static(eng._ctx, B, n, p(rec), p(flags), p(xf), p(xs), p(sof), len(off) - 1, off.ctypes.data, len(rows),
                                       rows.ctypes.data, ego.ctypes.data, int(hidden), *[p(out[k]) for k in KEYS], None)
    return check_guarded(pkg, eng, "jsim_loop_eval_static", SPEC, buf, n, rc, nothing=n == 0)


@pytest.fixture(scope="module")
def whole(pkg, eng, arrays):
    return {h: launch(pkg, eng, arrays, h) for h in SC.HIDDEN}


def clear_err(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def test_all_cases_in_one_launch(pkg, eng, arrays, whole):
    g = SC.fixture()
    worst, compared = 0.0, 0
    for hidden in SC.HIDDEN:
        for n in SC.TICK_COUNTS:
            out = whole[hidden] if n == SC.N else launch(pkg, eng, arrays, hidden, n=n)
            hit, who, clear = g["hit"][hidden, :n], g["who"][hidden, :n], g["clear"][hidden, :n]
            assert np.array_equal(out["hit"], hit), (hidden, n, np.argwhere(out["hit"] != hit)[:5].tolist())
            assert np.array_equal(out["who"], who), (hidden, n, np.argwhere(out["who"] != who)[:5].tolist())
            assert np.array_equal(out["off_tick"], SC.expected_off_tick(hit, g["flags"].T)), (hidden, n)
            err = clear_err(out["clear"], clear)
            print(f"include_hidden = {hidden}, {n} ticks: clear against the reference-made fixture, maximum error {err:.3g}")
            assert err <= BAR, (hidden, n, err)
            worst = max(worst, err)
            compared += out["hit"].shape[1]
            if n != SC.N:                                              # a shorter launch is a prefix of the long one
                for k in ("clear", "who", "hit"):
                    assert np.array_equal(out[k], whole[hidden][k][:n], equal_nan=True), (n, k)
    assert compared == 29 * 9 * 2
    print(f"jsim_loop_eval_static against the fixture, 29 cases x {SC.TICK_COUNTS} ticks x include_hidden 0, 1: clear maximum error {worst:.3g}")
    # the exact cases: the ties take the lowest index, the edge touches at 0.0 and not at +4.4e-16
    for hidden in SC.HIDDEN:
        out = whole[hidden]
        assert np.all(out["who"][:, 0] == 0) and np.all(out["who"][:, 26] == 0)
        assert np.all(out["hit"][0::2, 28] == 0) and np.all(out["hit"][1::2, 28] == -1)
        assert np.isnan(out["clear"][:, 10]).all() and np.all(out["who"][:, 10] == -1) and np.all(out["hit"][:, 10] == -1)


def test_batch_layout_is_immaterial(pkg, eng, arrays, whole):
    B = arrays["rec"].shape[1]
    for hidden in SC.HIDDEN:
        rev = launch(pkg, eng, arrays, hidden, egos=np.arange(B)[::-1])
        for k in KEYS:
            assert np.array_equal(rev[k], whole[hidden][k][:, ::-1], equal_nan=True), (hidden, k)
    for b in range(B):
        one = launch(pkg, eng, arrays, 1, egos=[b])
        for k in KEYS:
            assert np.array_equal(one[k], whole[1][k][:, b:b + 1], equal_nan=True), (b, k)


def test_a_set_outside_the_sets_is_an_empty_set(pkg, eng, arrays):
    n_sets = len(SC.SET_NAMES)
    egos = [2, 18, 19, 24]
    out = launch(pkg, eng, arrays, 1, egos=egos, set_of=np.array([-1, n_sets, 2 ** 31 - 1, -2 ** 31]))
    assert np.isnan(out["clear"]).all() and all(np.all(out[k] == -1) for k in ("who", "hit", "off_tick"))
    torch.cuda.synchronize()
    mixed = launch(pkg, eng, arrays, 1, egos=egos, set_of=np.array([0, n_sets, 4, -1]))       # beside egos whose set is there
    ref = launch(pkg, eng, arrays, 1, egos=egos)
    for k in KEYS:
        assert np.array_equal(mixed[k][:, [0, 2]], ref[k][:, [0, 2]], equal_nan=True), k
    assert np.isnan(mixed["clear"][:, [1, 3]]).all() and np.all(mixed["hit"][:, [1, 3]] == -1) and np.all(mixed["off_tick"][:, [1, 3]] == -1)


def test_nothing_to_do_writes_nothing(pkg, eng, arrays):
    launch(pkg, eng, arrays, 1, n=0)                                   # (check_guarded: returns 0, every slot is still poison)


# ---- a loop: four egos, one per start position, each against its own scenario's obstacles ----
CYCLIST_DIMS = dict(L=1.0, width=0.45, extra_length=0.64)
T, K = 13, 70


def _loop(pkg, W, iroutes):
    big = W.ego_batch(iroutes, 64, T, rank=2)
    starts = big.path_id // 3                                       # route_queries: start_pos 1..4 x turn_indicator 1..3
    idx = np.array([int(np.flatnonzero(starts == s)[0]) for s in range(4)])
    batch = sub_batch(big, idx)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    x, y = (float(v) for v in x0[0, :2].cpu())
    cyclist = dict(kind="arterial", x_init=x + 0.5, y_init=y + 6.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST_DIMS)
    sets = [pkg.planner.intersection_obstacles(int(p) // 3 + 1, int(p) % 3 + 1) for p in batch.path_id]
    return pkg.ScenarioLoop(eng, x0, [cyclist], hist_cap=K, max_age=60, frame_window=20, record=K), sets


def _restate_recorder(pkg, r, res, sets):
    tables = [pkg.planner.static_obstacle_rows(s, res["margin"]) for s in sets]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tables])])
    return SN.eval_static(r.rec.cpu().numpy(), r.flags.cpu().numpy(), r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy(),
                          res["set_of"], off, np.concatenate(tables), res["ego_shape"], res["include_hidden"])


def assert_equals_restatement(out, ref, what):
    for k in ("who", "hit", "off_tick"):
        assert np.array_equal(out[k], ref[k]), (what, k)
    err = clear_err(out["clear"], ref["clear"])
    print(f"{what}: clear against the restatement, maximum error {err:.3g}")
    assert err <= BAR, (what, err)


def test_scenario_loop_against_its_own_scenarios(pkg, W, iroutes):
    run, sets = _loop(pkg, W, iroutes)
    assert [s[20:] for s in sets] != [sets[0][20:]] * 4              # the hidden boxes differ with the start position
    run.run(K)
    rec = run.recorder
    res = rec.static_conflicts(sets, set_of=np.arange(4))
    assert res["clear"].shape == (K, 4) and res["margin"] == SC.R and res["ego_shape"] == SC.CAR and res["include_hidden"] is False
    assert res["set_of"].tolist() == [0, 1, 2, 3] and np.isfinite(res["clear"]).all() and np.array_equal(res["contact"], res["hit"] >= 0)
    assert_equals_restatement(res, _restate_recorder(pkg, rec, res, sets), "ScenarioLoop, run(70)")
    hid = rec.static_conflicts(sets, set_of=np.arange(4), include_hidden=True)
    assert_equals_restatement(hid, _restate_recorder(pkg, rec, hid, sets), "ScenarioLoop, run(70), hidden included")
    assert (hid["clear"] <= res["clear"]).all()
    wide = rec.static_conflicts(sets, set_of=np.arange(4), margin=2.5)
    assert_equals_restatement(wide, _restate_recorder(pkg, rec, wide, sets), "ScenarioLoop, run(70), margin 2.5")
    assert np.array_equal(wide["clear"], res["clear"]) and (wide["contact"] | ~res["contact"]).all() and wide["contact"].sum() > res["contact"].sum()
    one = rec.static_conflicts(sets[1], set_of=0)                     # one set for every ego: ego 1's own
    for k in KEYS:
        assert np.array_equal(one[k][:, 1], res[k][:, 1], equal_nan=True), k
    none = rec.static_conflicts([])
    assert np.isnan(none["clear"]).all() and not none["contact"].any() and np.all(none["off_tick"] == -1)
    eps = pkg.history.static_episodes(res, rec.flags.cpu().numpy())
    assert [len(e) for e in eps] == rec.episodes()["count"].tolist()
    print(f"min clearance per ego {[min(e['min_clear'] for e in ep if e['min_clear'] == e['min_clear']) for ep in eps]}, "
          f"ticks off the road {[sum(e['ticks_off'] for e in ep) for ep in eps]}")

    ticks, _ = _loop(pkg, W, iroutes)
    for _ in range(K):
        ticks.tick()
    res_t = ticks.recorder.static_conflicts(sets, set_of=np.arange(4))
    for k in KEYS:
        assert np.array_equal(res[k], res_t[k], equal_nan=True), ("70 x tick()", k)

    for kw in (dict(obstacles=[("cone", 1.0, (0.0, 0.0))]), dict(obstacles=sets, set_of=np.array([0, 1, 2, 4])), dict(obstacles=sets, set_of=-1),
               dict(obstacles=sets, set_of=np.zeros(3, dtype=int)), dict(obstacles=sets, set_of=0.5), dict(obstacles=sets, margin=-1.0),
               dict(obstacles=sets, margin=np.nan), dict(obstacles=sets, margin=np.inf)):
        with pytest.raises(ValueError):
            rec.static_conflicts(**kw)
