"""Per-tick stakeholder reasons and the replan trigger on the device (jsim_loop_eval_reasons, Recorder.reasons, DESIGN.md
section 16): all fixture cases as one launch against the reference-made fixture, at every tick count of the list; the launch shape
(one ego per launch, the order reversed, B = 1, 3, 65); the carry (a run in two pieces, nothing to do); and a ScenarioLoop with a
cyclist: run(70) against the restatement on the recorder's own arrays, against 70 x tick(), against a traffic layout with an ego
that has no cyclist, and on into score_situations.

Bars: timers, trig, first and the carry exact; reals within 1e-12 relative -- one sqrt and at most two exp behind sums that are
exact, libm within a few ulp, about 1000 x headroom (section 14's argument)."""
import numpy as np
import pytest
import torch

import reason_ticks_cases as TC
import reason_ticks_numpy as TN
from gpu_helpers import W, iroutes, loop_engine  # noqa: F401

pytestmark = pytest.mark.gpu
RTOL = 1e-12
KEYS = ("val", "timers", "trig", "first", "carry")


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return TC.recorder_arrays(TC.cases())


def launch(pkg, eng, A, n=TC.N, k0=0, carry=None, egos=None):
    """jsim_loop_eval_reasons on ticks k0 .. k0 + n - 1 of recorder arrays (egos: these egos only, in this order; the vehicle table stays
    whole).  Returns numpy val, timers, trig, first, carry."""
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    B = len(idx)
    x_first = A["x_first"][idx].copy()
    if k0 > 0:
        x_first[:, :2] = TN.start_positions(A["rec"][:k0 + 1], A["flags"][:k0 + 1], A["x_first"], A["x_spawn"])[k0][idx]
    dev = eng.device
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    rec, flags, obs = up(A["rec"][k0:k0 + max(n, 1), idx]), up(A["flags"][k0:k0 + max(n, 1), idx], np.int32), up(A["obs"][k0:k0 + max(n, 1)])
    xf, xs, veh = up(x_first), up(A["x_spawn"][idx]), up(A["veh_of"][idx], np.int32)
    par, thr = up(A["par"][idx]), up(A["threshold"][idx])
    car = up(A["carry"][idx] if carry is None else carry)
    val = torch.full((max(n, 1), B, 4), -7.0, dtype=torch.float64, device=dev)
    tim = torch.full((max(n, 1), B, 2), -7.0, dtype=torch.float64, device=dev)
    trig = torch.full((max(n, 1), B), -7, dtype=torch.int32, device=dev)
    first = torch.full((B,), -7, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    rc = eng.lib.jsim_loop_eval_reasons(eng._ctx, B, n, p(rec), p(flags), A["obs"].shape[1], p(obs), p(xf), p(xs), p(veh), p(par), p(thr),
                                        p(car), p(val), p(tim), p(trig), p(first), None)
    pkg._cabi.check(rc, eng._ctx, "jsim_loop_eval_reasons")
    torch.cuda.synchronize()
    return {"val": val[:n].cpu().numpy(), "timers": tim[:n].cpu().numpy(), "trig": trig[:n].cpu().numpy(), "first": first.cpu().numpy(),
            "carry": car.cpu().numpy()}


@pytest.fixture(scope="module")
def whole(pkg, eng, arrays):
    return launch(pkg, eng, arrays)


def rel_err(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0


def test_all_cases_in_one_launch(pkg, eng, arrays, whole):
    g = TC.fixture()
    cs = TC.cases()
    B = len(cs)
    ref_val, ref_tim = np.swapaxes(g["val"], 0, 1), np.swapaxes(g["timers"], 0, 1)        # [n][B][.]
    needed = g["needed"].T
    with np.errstate(invalid="ignore"):
        below = ref_val[:, :, :3] < g["threshold"][None, :, None]
    trig_ref = (needed.astype(np.int32) | (below * np.array([2, 4, 8])).sum(axis=2)).astype(np.int32)
    mine = TC.restate(arrays)
    worst = 0.0
    for n in TC.TICK_COUNTS:
        out = whole if n == TC.N else launch(pkg, eng, arrays, n=n)
        if n != TC.N:                                               # a shorter launch is a prefix of the long one
            for k in ("val", "timers", "trig"):
                assert np.array_equal(out[k], whole[k][:n], equal_nan=True), (n, k)
        assert np.array_equal(out["timers"], ref_tim[:n]), n
        assert np.array_equal(out["trig"], trig_ref[:n]), n
        err = rel_err(out["val"], ref_val[:n])
        worst = max(worst, err)
        assert err <= RTOL, (n, err)
        first = np.array([int(np.argmax(needed[:n, b])) if needed[:n, b].any() else -1 for b in range(B)])
        assert np.array_equal(out["first"], first), n
        # the carry: what the reference holds after tick n - 1 (restatement-made cases: the restatement's), a fresh episode behind a
        # record that ended one
        cut = TC.restate(arrays, n=n)["carry"]
        for b, c in enumerate(cs):
            if not c["restated"]:
                ended = bool(c["flags"][n - 1] & (TC.GOAL | TC.AGE))
                want = [0.0, 0.0, 0.0] if ended else [g["timers"][b, n - 1, 0], g["timers"][b, n - 1, 1], float(g["tracker"][b, n - 1])]
                assert cut[b].tolist() == want, (n, b)
        assert np.array_equal(out["carry"], cut), n
    print(f"jsim_loop_eval_reasons against the fixture, {B} cases x {TC.TICK_COUNTS} ticks: maximum relative error {worst:.3g}")
    assert rel_err(whole["val"], mine["val"]) <= RTOL and np.array_equal(whole["trig"], mine["trig"])
    assert np.isnan(whole["val"][:, 25, 1:]).all() and not whole["timers"][:, 25].any()      # the ego without a cyclist


def test_launch_shape_is_immaterial(pkg, eng, arrays, whole):
    B = arrays["rec"].shape[1]
    for b in range(B):
        one = launch(pkg, eng, arrays, egos=[b])
        for k in KEYS:
            assert np.array_equal(one[k], whole[k][:, b:b + 1] if whole[k].ndim == 3 or k == "trig" else whole[k][b:b + 1], equal_nan=True), (b, k)
    rev = launch(pkg, eng, arrays, egos=np.arange(B)[::-1])
    for k in KEYS:
        assert np.array_equal(rev[k], whole[k][:, ::-1] if whole[k].ndim == 3 or k == "trig" else whole[k][::-1], equal_nan=True), k
    for n_egos in (1, 3, 65):
        egos = np.arange(n_egos) * 7 % B
        out = launch(pkg, eng, arrays, egos=egos)
        for k in KEYS:
            assert np.array_equal(out[k], whole[k][:, egos] if whole[k].ndim == 3 or k == "trig" else whole[k][egos], equal_nan=True), (n_egos, k)


def test_a_run_in_two_pieces(pkg, eng, arrays, whole):
    g = TC.fixture()
    for s in TC.SPLITS:
        head = launch(pkg, eng, arrays, n=s)
        assert np.array_equal(head["carry"], g[f"split_{s}_carry"]), s
        tail = launch(pkg, eng, arrays, n=TC.N - s, k0=s, carry=head["carry"])
        for k in ("val", "timers", "trig"):
            assert np.array_equal(np.concatenate([head[k], tail[k]]), whole[k], equal_nan=True), (s, k)
        assert np.array_equal(tail["carry"], whole["carry"]), s
        first = np.where(head["first"] >= 0, head["first"], np.where(tail["first"] >= 0, tail["first"] + s, -1))
        assert np.array_equal(first, whole["first"]), s
    none = launch(pkg, eng, arrays, n=0)                                # nothing to do: the carry stays, nothing is written
    assert np.array_equal(none["carry"], arrays["carry"]) and np.all(none["first"] == -7)


# ---- a loop with a cyclist ----
CYCLIST_DIMS = dict(L=1.0, width=0.45, extra_length=0.64)
T, B, K = 13, 3, 70


def _loop(pkg, W, iroutes, traffic=False):
    batch = W.ego_batch(iroutes, B, T, rank=2)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    x, y = (float(v) for v in x0[0, :2].cpu())
    cyclist = dict(kind="arterial", x_init=x + 0.5, y_init=y + 6.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST_DIMS)
    if traffic:                                                     # egos 0 and 1 meet the cyclist, ego 2's set is empty
        return pkg.ScenarioLoop(eng, x0, [[cyclist], []], hist_cap=K, max_age=60, frame_window=20, traffic_of=np.array([0, 0, 1]), record=K)
    return pkg.ScenarioLoop(eng, x0, [cyclist], hist_cap=K, max_age=60, frame_window=20, record=K)


def _restate_recorder(r, res):
    rec, flags, obs = r.rec.cpu().numpy(), r.flags.cpu().numpy(), r.obs.cpu().numpy()
    return TN.eval_ticks(rec, flags, obs, r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy(), res["veh_of"], res["par"],
                         res["threshold"])


def _assert_against_restatement(res, ref, what):
    val = np.stack([res["policymaker"], res["driver"], res["cyclist"], res["distance"]], axis=2)
    err = rel_err(val, ref["val"])
    assert err <= RTOL, (what, err)
    assert np.array_equal(res["timers"], ref["timers"]) and np.array_equal(res["carry"], ref["carry"]), what
    assert np.array_equal(res["replan"], (ref["trig"] & 1) != 0) and np.array_equal(res["first_replan"], ref["first"]), what
    assert np.array_equal(res["below"], ((ref["trig"][:, :, None] >> np.arange(1, 4)) & 1) != 0), what
    return err


def test_scenario_loop_with_a_cyclist(pkg, W, iroutes):
    run = _loop(pkg, W, iroutes)
    run.run(K)
    res = run.recorder.reasons()
    assert res["policymaker"].shape == (K, B) and res["timers"].shape == (K, B, 2) and res["par"][0, 0] == run.loop.eng.dt
    assert res["veh_of"].tolist() == [0, 0, 0] and np.isfinite(res["distance"]).all()
    err = _assert_against_restatement(res, _restate_recorder(run.recorder, res), "run(70)")
    print(f"Recorder.reasons against the restatement on the recorder's arrays: maximum relative error {err:.3g}; "
          f"first_replan {res['first_replan'].tolist()}, ticks in the cyclist's range {(res['distance'] < 10.0).sum(0).tolist()}")
    assert (res["distance"] < 10.0).any()                           # the cyclist is met, not only recorded

    ticks = _loop(pkg, W, iroutes)
    for _ in range(K):
        ticks.tick()
    res_t = ticks.recorder.reasons()
    for k in res:
        assert np.array_equal(res[k], res_t[k], equal_nan=True), ("70 x tick()", k)

    # a traffic layout: egos 0 and 1 see what they saw, ego 2 has no cyclist.  With the centreline out of the way the policymaker
    # value is 1 everywhere, so an ego without a cyclist has nothing that could trigger
    R = pkg.reasons
    par = R.par_row(dt=run.loop.eng.dt, centerline=-1.0e3)
    lay = _loop(pkg, W, iroutes, traffic=True)
    lay.run(K)
    assert lay.recorder.default_cyclist().tolist() == [0, 0, -1]
    res_p, res_l = run.recorder.reasons(par=par), lay.recorder.reasons(par=par)
    _assert_against_restatement(res_l, _restate_recorder(lay.recorder, res_l), "traffic layout")
    for k in ("policymaker", "driver", "cyclist", "distance", "timers", "replan", "below"):
        assert np.array_equal(res_l[k][:, :2], res_p[k][:, :2]), k
    assert np.array_equal(res_l["first_replan"][:2], res_p["first_replan"][:2]) and np.array_equal(res_l["carry"][:2], res_p["carry"][:2])
    assert np.isnan(res_l["driver"][:, 2]).all() and np.isnan(res_l["cyclist"][:, 2]).all() and np.isnan(res_l["distance"][:, 2]).all()
    assert np.all(res_l["policymaker"] == 1.0) and not res_l["replan"][:, 2].any() and res_l["first_replan"][2] == -1
    assert not res_l["timers"][:, 2].any() and not res_l["carry"][2].any()

    # the situation at the trigger, as perform_replan is handed it, into the scoring launch
    trig = np.flatnonzero(res["first_replan"] >= 0)
    b = int(trig[0]) if len(trig) else 0
    k = int(res["first_replan"][b]) if len(trig) else K - 1          # (no trigger within 70 ticks at these shapes: the last tick)
    s = np.arange(120) * 0.083
    sit = R.situation_at(run.recorder, b, k, [], reasons=res)
    x, y = sit["ego"][:2]
    cands = [np.stack([np.full(120, x - dx * np.clip(s / 5.0, 0, 1)), y + s, np.full(120, np.pi / 2)], axis=1) for dx in (0.0, 3.0)]
    cands.append(cands[0][:60].copy())
    sit = R.situation_at(run.recorder, b, k, cands, reasons=res)
    assert sit["now"] == (res["policymaker"][k, b], res["driver"][k, b], res["cyclist"][k, b], res["timers"][k, b, 0], res["timers"][k, b, 1])
    assert sit["cyclist"] == tuple(run.recorder.obs[k, 0].cpu().numpy().tolist()) and np.array_equal(sit["par"], res["par"][b])
    out = R.score_situations([sit], [(1 / 9, 4 / 9, 4 / 9), (0.2, 0.5, 0.3)], [0, 1])
    assert out["status"].shape == (3,) and out["scores"].shape == (2, 3) and out["best"].shape == (2, 1)
    with pytest.raises(ValueError):
        R.situation_at(lay.recorder, 2, 0, cands, reasons=res_l)      # an ego without a cyclist has no situation
    with pytest.raises(ValueError):
        run.recorder.reasons(cyclist=1)
    with pytest.raises(ValueError):
        run.recorder.reasons(par=R.par_row(dt=0.0))


def test_a_loop_without_vehicles_has_no_reasons(pkg, W, iroutes):
    batch = W.ego_batch(iroutes, B, T, rank=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    loop = pkg.ClosedLoop(eng, x0, hist_cap=4, max_age=40, record=4)
    loop.run(2)
    with pytest.raises(ValueError, match="no vehicle records"):
        loop.recorder.reasons()
