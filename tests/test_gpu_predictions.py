"""Every recorded prediction against what the vehicle then did, on the device (jsim_loop_score_predictions, Recorder.predictions,
DESIGN.md section 28): every cut of the fixture through the entry point against the reference-made expectations; a live ScenarioLoop
whose errors are jsim_loop_predict_obstacles' samples against the records, bit for bit; an InteractingLoop driven tick by tick whose
ego rows are pred_egos() against the records, respawn ticks included; traffic sets against shared lists; the refusals, with output
buffers poisoned first and a row of guard slots on either side; the sums by look-ahead step against the restatement."""
import numpy as np
import pytest
import torch

import prediction_cases as PC
import predictions_numpy as PN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine  # noqa: F401

pytestmark = pytest.mark.gpu
ENTRY = "jsim_loop_score_predictions"
POISON_I, POISON_D = -85, 8.5e300                                      # values no output can take
V_ALL = PC.N_OBS + PC.B
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
T = 13


def spec(S):
    return [("pt_i", np.int32, (3,), POISON_I), ("pt_d", np.float64, (6,), POISON_D), ("err", np.float64, (S,), POISON_D)]


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine (the call needs its context, not its batch) with the cases' sample time and wheelbase, the geometry set and the
    cases' shape table registered: vehicle 4 is the cyclist."""
    e = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, T, rank=2), T)[0]
    assert (e.dt, e.L) == (PC.DT, PC.L_CAR)
    pkg.closed_loop.PreTick(e)
    pkg.closed_loop._register_shapes(e, PC.recorder_arrays()["shapes"])
    return e


@pytest.fixture(scope="module")
def arrays():
    return PC.recorder_arrays()


def launch(pkg, eng, A, n, S, n_obs=PC.N_OBS, egos=1, tol=PC.TOL, with_err=True, rc_want=0, **over):
    """The entry point on the first n ticks of recorder arrays, on guarded outputs (gpu_helpers.guarded_outputs with B := V; step_sum
    and step_cnt [V][S] between guard rows of their own).  Returns numpy outputs, or the library's message."""
    B = A["rec"].shape[1]
    V = n_obs + (B if egos == 1 else 0)
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    m = max(n, 1)
    rec, flags, xf, xs = up(A["rec"][:m]), up(A["flags"][:m], np.int32), up(A["x_first"]), up(A["x_spawn"])
    obs = up(A["obs"][:m, :n_obs]) if n_obs > 0 else None
    Sa = S if 1 <= S <= 64 else 1
    views, buf = guarded_outputs(spec(Sa), n, max(V, 1), eng.device)
    rows = {"step_sum": torch.full((max(V, 1) + 2, Sa), POISON_D, dtype=torch.float64, device=eng.device),
            "step_cnt": torch.full((max(V, 1) + 2, Sa), POISON_I, dtype=torch.int32, device=eng.device)}
    p = lambda t: None if t is None else t.data_ptr()
    args = dict(B=B, n_ticks=n, rec=p(rec), flags=p(flags), n_obs=n_obs, obs_rec=p(obs), x_first=p(xf), x_spawn=p(xs), egos=egos, n_steps=S, tol=tol,
                pt_i=p(views["pt_i"]), pt_d=p(views["pt_d"]), step_sum=p(rows["step_sum"][1:]), step_cnt=p(rows["step_cnt"][1:]),
                err=p(views["err"]) if with_err else None)
    args.update(over)
    rc = getattr(eng.lib, ENTRY)(eng._ctx, *[args[k] for k in ("B", "n_ticks", "rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "egos",
                                                                 "n_steps", "tol", "pt_i", "pt_d", "step_sum", "step_cnt", "err")], None)
    nothing = args["n_ticks"] == 0 or args["n_obs"] + (args["B"] if args["egos"] == 1 else 0) == 0
    sp = spec(Sa) if with_err else spec(Sa)[:2]
    if not with_err:
        torch.cuda.synchronize()
        assert bool((buf["err"] == POISON_D).all())
    out = check_guarded(pkg, eng, ENTRY, sp, {k: buf[k] for k, *_ in sp}, n, rc, rc_want, nothing=nothing, what=(S,))
    host = {k: t.cpu().numpy() for k, t in rows.items()}
    for k, t in host.items():
        poison = POISON_D if k == "step_sum" else POISON_I
        if isinstance(out, str):
            assert np.all(t == poison), k
        else:
            assert np.all(t[0] == poison) and np.all(t[V + 1:] == poison) and not np.any(t[1:V + 1] == poison), k
            out[k] = t[1:V + 1]
    return out


@pytest.fixture(scope="module")
def runs(pkg, eng, arrays):
    """Every cut of the fixture at every n_steps, launched once."""
    return {(n, S): launch(pkg, eng, arrays, n, S) for S in PC.STEPS for n in PC.TICK_COUNTS}


def test_every_fixture_cut(runs):
    g = PC.fixture()
    worst = 0.0
    for (n, S), out in runs.items():
        if n == 0:
            assert isinstance(out, str)
            continue
        ex = PC.expected(g, n, S)
        assert np.array_equal(out["pt_i"], ex["pt_i"]), (n, S, np.argwhere(out["pt_i"] != ex["pt_i"])[:5])
        assert np.array_equal(out["step_cnt"], ex["step_cnt"]), (n, S)
        assert np.array_equal(np.isnan(out["pt_d"]), np.isnan(ex["pt_d"])), (n, S)
        scored = ~np.isnan(ex["pt_d"])
        if scored.any():
            worst = max(worst, float(np.abs(out["pt_d"][scored] - ex["pt_d"][scored]).max()))
        assert np.array_equal(np.isnan(out["err"]), np.arange(S)[None, None, :] >= out["pt_i"][:, :, :1]), (n, S)
    print(f"{ENTRY}: {len(runs)} cuts of {V_ALL} rows, largest |pt_d - fixture| {worst:.3g}")
    assert worst <= 1e-9, worst


def test_step_sums_against_the_restatement(runs, arrays):
    """step_sum against the restatement at rtol 4 * n_ticks * 2^-53 (every term is >= 0, so any order of summation stays within that);
    step_cnt exactly.  Where the restatement's sum is 0 the device's is 0 too."""
    worst, worst_own, at = 0.0, 0.0, None
    predictor = PC.prefix_predictor()
    failed = []
    for (n, S), out in runs.items():
        if n == 0:
            continue
        ref = PC.restate(arrays, n, S, predictor=predictor)
        assert np.array_equal(out["step_cnt"], ref["step_cnt"]), (n, S)
        rtol = 4 * n * 2.0 ** -53
        d = np.abs(out["step_sum"] - ref["step_sum"])
        rel = d / np.where(ref["step_sum"] > 0, ref["step_sum"], 1.0)
        assert np.all(d[ref["step_sum"] == 0] == 0), (n, S)
        if rel.max() / rtol > worst:
            worst, at = float(rel.max() / rtol), (n, S, *np.unravel_index(rel.argmax(), rel.shape), float(rel.max()))
        if not np.all(rel <= rtol):
            failed.append((n, S, float(rel.max()), rtol))
        own = np.nansum(out["err"], axis=0)                             # the device's own terms, in numpy's order
        assert np.all(np.abs(out["step_sum"] - own) <= rtol * np.abs(own)), (n, S)
        worst_own = max(worst_own, float((np.abs(out["step_sum"] - own) / np.where(own > 0, own, 1)).max()))
    print(f"step_sum against the restatement: the largest relative difference is {worst:.3g} of its bar, at (n, n_steps, row, step, difference) = {at}; "
          f"against the sum of the call's own err: largest relative difference {worst_own:.3g}")
    assert not failed, failed


def test_rows_do_not_depend_on_the_others(pkg, eng, arrays, runs):
    """n_obs = 0 (the egos alone), the vehicles alone, err = NULL, and the same call twice."""
    n, S = 129, 35
    ref = runs[n, S]
    egos_only = launch(pkg, eng, arrays, n, S, n_obs=0)
    cars_only = launch(pkg, eng, arrays, n, S, egos=0)
    no_err = launch(pkg, eng, arrays, n, S, with_err=False)
    again = launch(pkg, eng, arrays, n, S)
    for k in ("pt_i", "pt_d", "step_sum", "step_cnt", "err"):
        bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
        ax = 1 if k in ("pt_i", "pt_d", "err") else 0
        assert np.array_equal(bits(np.take(ref[k], range(PC.N_OBS, V_ALL), axis=ax)), bits(egos_only[k])), k
        assert np.array_equal(bits(np.take(ref[k], range(PC.N_OBS), axis=ax)), bits(cars_only[k])), k
        assert np.array_equal(bits(ref[k]), bits(again[k])), k
        if k != "err":
            assert np.array_equal(bits(ref[k]), bits(no_err[k])), k


def test_refusals(pkg, eng, arrays):
    who = ENTRY + ": "
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_ticks=-1), "n_ticks=-1"), (dict(n_obs=-1), "n_obs=-1"), (dict(n_steps=0), "n_steps=0"),
                    (dict(n_steps=65), "n_steps=65"), (dict(egos=2), "egos=2"), (dict(egos=-1), "egos=-1"), (dict(tol=-0.5), "tol"),
                    (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"), (dict(obs_rec=None), "null obs_rec"),
                    (dict(rec=None), "null pointer rec"), (dict(flags=None), "null pointer flags"), (dict(x_first=None), "null pointer x_first"),
                    (dict(x_spawn=None), "null pointer x_spawn"), (dict(pt_i=None), "null pointer pt_i"), (dict(pt_d=None), "null pointer pt_d"),
                    (dict(step_sum=None), "null pointer step_sum"), (dict(step_cnt=None), "null pointer step_cnt"),
                    (dict(n_obs=3), "shape table")):
        S = kw.get("n_steps", 35)
        over = {k: v for k, v in kw.items() if k not in ("n_steps", "n_obs", "egos", "tol")}
        direct = {k: kw[k] for k in ("n_obs", "egos", "tol") if k in kw}
        if direct.get("n_obs", 0) < 0 or direct.get("egos", 1) not in (0, 1):      # (launch sizes its buffers from these)
            over.update(direct); direct = {}
        err = launch(pkg, eng, arrays, 64, S, rc_want=-22, **direct, **over)
        assert err.startswith(who) and msg in err, (kw, err)
    launch(pkg, eng, arrays, 0, 35)                                     # nothing to do: returns 0 and writes nothing
    launch(pkg, eng, arrays, 64, 35, n_obs=0, egos=0)


# ---- live recorders ----
def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_scenario_loop_errors_are_the_obstacle_predictors(pkg, W, iroutes):
    B, n = 6, 70
    specs = [dict(direction=1, turning=True, speed=20 / 3.6, offset=None), dict(direction=-1, turning=False, speed=15 / 3.6, offset=4.0, dims=CYCLIST)]
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T)
    loop = pkg.ScenarioLoop(eng, x0, specs, max_age=40, record=n)
    loop.run(n)
    r = loop.recorder
    res = r.predictions(steps=True)
    S = loop.pre.n_steps
    assert (res["n_steps"], res["egos"], res["n_obs"], res["tol"]) == (S, False, 2, r._ego_shape()[2]) and res["err"].shape == (n, 2, S)
    obs = r.obs[:n].cpu().numpy()
    assert np.abs(obs[-1, :, 3] - obs[0, :, 3]).max() > 0.5 and (obs[:10, 1, 2] == 0).all() and obs[-1, 1, 2] > 0   # one turned, one waited
    for k in (0, 1, 5, 63, 64, 69):
        pred = loop.pre.predict(r.obs[k].contiguous()).cpu().numpy()    # jsim_loop_predict_obstacles: [2][S][3]
        m = min(S, n - 1 - k)
        want = np.full((2, S), np.nan)
        for v in range(2):
            dx, dy = pred[v, :m, 0] - obs[k + 1:k + 1 + m, v, 0], pred[v, :m, 1] - obs[k + 1:k + 1 + m, v, 1]
            want[v, :m] = np.sqrt(dx * dx + dy * dy)
        assert bits_equal(res["err"][k], want), (k, np.nanmax(np.abs(res["err"][k] - want)))
        assert (res["n"][k] == m).all()
        if m:
            assert bits_equal(res["ade"][k], np.cumsum(want[:, :m], axis=1)[:, -1] / m) and bits_equal(res["fde"][k], want[:, m - 1])
            assert bits_equal(res["max"][k], want[:, :m].max(axis=1)) and np.array_equal(res["max_at"][k], want[:, :m].argmax(axis=1))
        else:
            assert np.isnan(res["ade"][k]).all() and (res["max_at"][k] == -1).all() and (res["hold"][k] == 0).all()
    t, curve = pkg.history.prediction_curve(res, eng.dt)
    assert t.shape == (S,) and curve.shape == (2, S) and curve[0, -1] > 1.0                                        # the turning car is mispredicted
    print(f"ScenarioLoop, {n} ticks: mean error of the turning car at {t[-1]:.1f} s ahead {curve[0, -1]:.3g} m, of the waiting cyclist {curve[1, -1]:.3g} m")


def test_interacting_loop_ego_rows_are_pred_egos(pkg, W, iroutes):
    B, n = 6, 70
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=2), T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[3, 3], hist_cap=n, max_age=9, frame_window=20, record=n)
    preds = []
    for _ in range(n):
        preds.append(il.pred_egos().cpu().numpy())
        il.tick()
    r = il.recorder
    res = r.predictions(steps=True)
    S = il.pre.n_steps
    assert res["egos"] is True and res["n_obs"] == 0 and res["err"].shape == (n, B, S)
    rec, flags = r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy()
    assert ((flags & 6) != 0).sum() >= 6 * B                            # every ego respawned often
    for k in range(n):
        for b in range(B):
            m = min(S, PN.ego_horizon(flags[:, b], k) - k + 1)
            dx, dy = preds[k][b, :m, 0] - rec[k:k + m, b, 0], preds[k][b, :m, 1] - rec[k:k + m, b, 1]
            want = np.full(S, np.nan)
            want[:m] = np.sqrt(dx * dx + dy * dy)
            assert bits_equal(res["err"][k, b], want), (k, b)
            assert res["n"][k, b] == m
    places = pkg.history.prediction_places(res, r.vehicle_ranges(), r.mate_ranges())
    assert places["row"][:, :2].tolist() == [[1, 2], [0, 2], [0, 1], [4, 5], [3, 5], [3, 4]] and (places["row"][:, 2:] == -1).all()
    assert bits_equal(places["ade"][:, 0, 0], res["ade"][:, 1]) and np.isnan(places["ade"][:, :, 2:]).all()
    for bad in (dict(n_steps=0), dict(n_steps=65), dict(n_steps=2.5), dict(tol=-1.0), dict(tol=float("nan")), dict(egos="plan"), dict(egos=2)):
        with pytest.raises(ValueError):
            r.predictions(**bad)
    assert r.predictions(egos=False)["ade"].shape == (n, 0)


def test_a_plan_mode_recording_scores_the_constant_rule_on_request(pkg, W, iroutes):
    B, n = 6, 12
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=2), T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[3, 3], hist_cap=n, max_age=9, frame_window=20, record=n, mate_prediction="plan")
    il.run(n)
    r = il.recorder
    with pytest.raises(ValueError, match="plan"):
        r.predictions(egos=True)
    assert r.predictions()["egos"] is False and r.predictions()["ade"].shape == (n, 0)
    res = r.predictions(egos="constant")
    assert res["egos"] is True and res["ade"].shape == (n, B) and np.isfinite(res["ade"]).all() and (res["n"] >= 1).all()


def traffic_refusals(pkg, r):
    """Under a registered traffic layout: an n_obs that is not the sets' total and a B that is not the layout's are refused (-22) with
    nothing written."""
    eng = r.loop.eng
    p = lambda t: t.data_ptr()
    i32 = torch.full((4096,), POISON_I, dtype=torch.int32, device=eng.device)
    f64 = torch.full((4096,), POISON_D, dtype=torch.float64, device=eng.device)
    for B_, n_obs, msg in ((eng.B, r.n_obs - 1, "the traffic sets hold 5 vehicles"), (eng.B, r.n_obs + 1, "the traffic sets hold 5 vehicles"),
                           (eng.B - 1, r.n_obs, f"the traffic layout (jsim_loop_set_traffic) is for B={eng.B}")):
        rc = getattr(eng.lib, ENTRY)(eng._ctx, B_, 2, p(r.rec), p(r.flags), n_obs, p(r.obs), p(r.x0_first), p(r.loop.x0_spawn), 1, 3, 1.0,
                                     p(i32), p(f64), p(f64), p(i32), None, None)
        torch.cuda.synchronize()
        err = eng.lib.jsim_last_error(eng._ctx).decode()
        assert rc == -22 and err.startswith(ENTRY + ": ") and msg in err, (B_, n_obs, rc, err)
        assert bool((i32 == POISON_I).all()) and bool((f64 == POISON_D).all())


def test_traffic_sets_against_shared_lists(pkg, W, iroutes):
    B, n = 6, 70
    sets = [[dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(direction=-1, turning=True, speed=25 / 3.6, offset=None, dims=CYCLIST)],
            [dict(kind="roundabout", direction=1, turning=True, speed=20 / 3.6, offset=1.0)],
            [dict(kind="arterial", x_init=1.5, y_init=-30.0, speed=25 / 3.6, initial_speed=5 / 3.6, offset=3.0),
             dict(kind="arterial", x_init=2.0, y_init=-12.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)]]
    keys = ("n", "hold", "max_at", "ade", "fde", "max", "lon", "lat", "yaw", "err")

    def run(refusals=False, **kw):
        eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T)
        loop = pkg.ScenarioLoop(eng, x0, max_age=40, record=n, **kw)
        loop.run(n)
        if refusals:
            traffic_refusals(pkg, loop.recorder)
        return loop.recorder.predictions(steps=True)

    whole = run(refusals=True, obstacle_specs=sets, traffic_of=np.array([0, 1, 2, 0, 1, 2]))
    assert whole["ade"].shape == (n, 5) and np.nanmax(whole["max"]) > 1.0
    lo = 0
    for s in sets:
        alone = run(obstacle_specs=s)
        for k in keys:
            assert bits_equal(whole[k][:, lo:lo + len(s)], alone[k]), (lo, k)
        for k in ("step_sum", "step_cnt"):
            assert bits_equal(whole[k][lo:lo + len(s)], alone[k]), (lo, k)
        lo += len(s)
