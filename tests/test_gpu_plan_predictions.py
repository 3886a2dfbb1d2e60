"""The plan record, its scoring and its replay on the device (jsim_loop_set_plan_recorder, jsim_loop_score_plan_predictions,
jsim_loop_eval_cutoffs_plan, InteractingLoop(record_plans=True)): every cut of the fixture through the scoring
call against the reference-made expectations, one context per horizon; a plan-mode loop driven tick by tick whose plan record is the
engine's oa, od, status of every tick, whose errors are pred_egos() against the records and whose replayed cut-offs are the live
loop's, all bit for bit; the reference's plan-sharing loop with both recorders; a constant-mode loop that the plan recorder leaves
bit-identical; the edges and the refusals, with output buffers poisoned first and guard slots on either side."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import plan_prediction_cases as PC
import predictions_numpy as PN
from gpu_helpers import W, assert_state_equal, check_guarded, guarded_outputs, iroutes, loop_engine, loop_state  # noqa: F401

pytestmark = pytest.mark.gpu
ENTRY = "jsim_loop_score_plan_predictions"
POISON_I, POISON_D = -85, 8.5e300                                      # values no output can take
ARGS = ("B", "n_ticks", "rec", "flags", "x_first", "x_spawn", "plan_oa", "plan_od", "plan_status", "n_steps", "tol", "pt_i", "pt_d", "step_sum",
        "step_cnt", "err")


def spec(S):
    return [("pt_i", np.int32, (3,), POISON_I), ("pt_d", np.float64, (6,), POISON_D), ("err", np.float64, (S,), POISON_D)]


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def engines(pkg, W, iroutes):
    """One engine per horizon of the cases (the call needs its context, not its batch), with their sample time, wheelbase and clamps."""
    out = {}
    for T in PC.HORIZONS:
        e = out[T] = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, T, rank=2), T)[0]
        assert (e.dt, e.L, e.T) == (PC.DT, PC.L_CAR, T)
        c = e.config
        assert (float(c.MAX_STEER_RAD), float(c.MAX_SPEED), float(c.MIN_SPEED)) == (PC.MAX_STEER, PC.MAX_SPEED, PC.MIN_SPEED)
    return out


@pytest.fixture(scope="module")
def groups():
    return PC.all_groups()


def launch(pkg, eng, A, n, S, tol=PC.TOL, with_err=True, rc_want=0, **over):
    """The entry point on the first n ticks of one group's arrays, on guarded outputs (gpu_helpers.guarded_outputs; step_sum and
    step_cnt [B][S] between guard rows of their own).  Returns numpy outputs, or the library's message."""
    B = A["rec"].shape[1]
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    m = max(n, 1)
    rec, flags, xf, xs = up(A["rec"][:m]), up(A["flags"][:m], np.int32), up(A["x_first"]), up(A["x_spawn"])
    oa, od, st = up(A["plan_oa"][:m]), up(A["plan_od"][:m]), up(A["plan_status"][:m], np.int32)
    Sa = S if 1 <= S <= 64 else 1
    views, buf = guarded_outputs(spec(Sa), n, B, eng.device)
    rows = {"step_sum": torch.full((B + 2, Sa), POISON_D, dtype=torch.float64, device=eng.device),
            "step_cnt": torch.full((B + 2, Sa), POISON_I, dtype=torch.int32, device=eng.device)}
    p = lambda t: None if t is None else t.data_ptr()
    args = dict(B=B, n_ticks=n, rec=p(rec), flags=p(flags), x_first=p(xf), x_spawn=p(xs), plan_oa=p(oa), plan_od=p(od), plan_status=p(st), n_steps=S,
                tol=tol, pt_i=p(views["pt_i"]), pt_d=p(views["pt_d"]), step_sum=p(rows["step_sum"][1:]), step_cnt=p(rows["step_cnt"][1:]),
                err=p(views["err"]) if with_err else None)
    args.update(over)
    rc = getattr(eng.lib, ENTRY)(eng._ctx, *[args[k] for k in ARGS], None)
    nothing = args["n_ticks"] == 0 or args["B"] == 0
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
            assert np.all(t[0] == poison) and np.all(t[B + 1:] == poison) and not np.any(t[1:B + 1] == poison), k
            out[k] = t[1:B + 1]
    return out


@pytest.fixture(scope="module")
def runs(pkg, engines, groups):
    """Every cut of the fixture at every n_steps, launched once."""
    return {(T, n, S): launch(pkg, engines[T], groups[T], n, S) for T in PC.HORIZONS for S in PC.STEPS for n in PC.TICK_COUNTS}


def test_every_fixture_cut(runs):
    g = PC.fixture()
    worst = 0.0
    for (T, n, S), out in runs.items():
        if n == 0:
            assert isinstance(out, str)
            continue
        ex = PC.expected(g, T, n, S)
        assert np.array_equal(out["pt_i"], ex["pt_i"]), (T, n, S, np.argwhere(out["pt_i"] != ex["pt_i"])[:5])
        assert np.array_equal(out["step_cnt"], ex["step_cnt"]), (T, n, S)
        assert np.array_equal(np.isnan(out["pt_d"]), np.isnan(ex["pt_d"])), (T, n, S)
        scored = ~np.isnan(ex["pt_d"])
        if scored.any():
            worst = max(worst, float(np.abs(out["pt_d"][scored] - ex["pt_d"][scored]).max()))
        assert np.array_equal(np.isnan(out["err"]), np.arange(S)[None, None, :] >= out["pt_i"][:, :, :1]), (T, n, S)
    print(f"{ENTRY}: {len(runs)} cuts, largest |pt_d - fixture| {worst:.3g}")
    assert worst <= 1e-9, worst


def test_step_sums_against_the_restatement(runs, groups):
    """step_sum against the restatement and against the sum of the call's own err at rtol 4 * n_ticks * 2^-53 (every term is >= 0, so
    any order of summation stays within that); step_cnt exactly.  Where the restatement's sum is 0 every term is a sample whose error
    is 0 there and within the doubles' bar of 1e-9 here (exactly 0 at heading 0 and for a standing ego), and so is the sum."""
    worst, at, failed = 0.0, None, []
    predictor = PC.cached(__import__("plan_predictions_numpy").predict)
    for (T, n, S), out in runs.items():
        if n == 0:
            continue
        ref = PC.restate(groups[T], n, S, predictor=predictor)
        assert np.array_equal(out["step_cnt"], ref["step_cnt"]), (T, n, S)
        rtol = 4 * n * 2.0 ** -53
        d = np.abs(out["step_sum"] - ref["step_sum"])
        rel = d / np.where(ref["step_sum"] > 0, ref["step_sum"], 1.0)
        zero = ref["step_sum"] == 0
        # (a sum that is 0 in the restatement is a sum of exact zeros only where the heading is exactly 0 or the ego stands)
        assert np.all(d[zero] <= 1e-9), (T, n, S)
        if rel[~zero].size and rel[~zero].max() / rtol > worst:
            worst, at = float(rel[~zero].max() / rtol), (T, n, S, float(rel[~zero].max()))
        if not np.all(rel[~zero] <= rtol):
            failed.append((T, n, S, "restatement", float(rel[~zero].max()), rtol))
        own = np.nansum(out["err"], axis=0)                             # the device's own terms, in numpy's order
        if not np.all(np.abs(out["step_sum"] - own) <= rtol * np.abs(own)):
            failed.append((T, n, S, "own err"))
    print(f"step_sum against the restatement: the largest relative difference is {worst:.3g} of the bar 4 n 2^-53, at (T, n, n_steps, difference) = {at}")
    assert not failed, failed


def test_err_null_and_a_second_call_are_bit_identical(pkg, engines, groups, runs):
    for T, n, S in ((13, 129, 35), (40, 200, 64)):
        ref = runs[T, n, S]
        no_err = launch(pkg, engines[T], groups[T], n, S, with_err=False)
        again = launch(pkg, engines[T], groups[T], n, S)
        for k in ("pt_i", "pt_d", "step_sum", "step_cnt", "err"):
            assert bits_equal(ref[k], again[k]), (T, k)
            if k != "err":
                assert bits_equal(ref[k], no_err[k]), (T, k)


def test_refusals_of_the_scoring_call(pkg, engines, groups):
    who = ENTRY + ": "
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_ticks=-1), "n_ticks=-1"), (dict(n_steps=0), "n_steps=0"), (dict(n_steps=65), "n_steps=65"),
                    (dict(tol=-0.5), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
                    *((({k: None}), "null pointer " + k) for k in ARGS[2:9] + ARGS[11:15])):
        S = kw.get("n_steps", 35)
        over = {k: v for k, v in kw.items() if k != "n_steps"}
        err = launch(pkg, engines[13], groups[13], 64, S, rc_want=-22, **over)
        assert err.startswith(who) and msg in err, (kw, err)
    launch(pkg, engines[13], groups[13], 0, 35)                           # nothing to do: returns 0 and writes nothing
    launch(pkg, engines[13], groups[13], 64, 35, B=0)


# ---- live recorders ----
T_LIVE = 13


def plan_loop(pkg, W, iroutes, n, mode="plan", **kw):
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 6, T_LIVE, rank=2), T_LIVE)
    return eng, pkg.InteractingLoop(eng, x0, group_sizes=[3, 3], hist_cap=n, max_age=9, frame_window=20, mate_prediction=mode, **kw)


def test_plan_mode_loop_driven_tick_by_tick(pkg, W, iroutes):
    B, n = 6, 70
    eng, il = plan_loop(pkg, W, iroutes, n, record=n, record_plans=True)
    assert il.recorder.glue["record_plans"] is True and il.recorder.glue["mate_prediction"] == "plan"
    cap, live = [], []
    for _ in range(n):
        cap.append({"oa": eng.oa.clone(), "od": eng.od.clone(), "status": eng.status.clone(), "pred": il.pred_egos()})
        il.tick()
        live.append({"status": il.pre.status.clone(), "idx": il.pre.traj_idx.clone(), "hit": il.pre.col_flag.clone(), "cut": eng.path_len.clone(),
                     "resp": (il.loop.age == 0).clone()})
    torch.cuda.synchronize()
    r = il.recorder
    # the plan record is what the engine held at the start of every tick
    for k, key in (("oa", "plan_oa"), ("od", "plan_od"), ("status", "plan_status")):
        assert torch.equal(r.plans[key], torch.stack([c[k] for c in cap])), key
    assert r.plans["plan_oa"].shape == (n, B, T_LIVE) and r.plans["plan_status"].dtype == torch.int32
    assert bool(r.plans["plan_oa"][1:].any()) and bool(r.plans["plan_od"][1:].any())
    # the scored errors are the live predictions against the records
    res = r.predictions(steps=True)
    S = il.pre.n_steps
    assert res["egos"] is True and res["rule"] == "plan" and res["n_obs"] == 0 and res["err"].shape == (n, B, S)
    rec, flags = r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy()
    assert ((flags & 6) != 0).sum() >= 6 * B                            # every ego respawned often
    preds = [c["pred"].cpu().numpy() for c in cap]
    for k in range(n):
        for b in range(B):
            m = min(S, PN.ego_horizon(flags[:, b], k) - k + 1)
            dx, dy = preds[k][b, :m, 0] - rec[k:k + m, b, 0], preds[k][b, :m, 1] - rec[k:k + m, b, 1]
            want = np.full(S, np.nan)
            want[:m] = np.sqrt(dx * dx + dy * dy)
            assert bits_equal(res["err"][k, b], want), (k, b, np.nanmax(np.abs(res["err"][k, b] - want)))
            assert res["n"][k, b] == m
    for key in ("ade", "n", "err"):
        assert bits_equal(r.predictions(egos="plan", steps=True)[key], res[key]) and bits_equal(r.predictions(egos=True, steps=True)[key], res[key])
    const = r.predictions(egos="constant")
    assert const["rule"] == "constant" and not bits_equal(const["ade"], res["ade"]) and r.predictions(egos=False)["rule"] is None
    places = pkg.history.prediction_places(res, r.vehicle_ranges(), r.mate_ranges())
    assert places["row"][:, :2].tolist() == [[1, 2], [0, 2], [0, 1], [4, 5], [3, 5], [3, 4]] and bits_equal(places["ade"][:, 0, 0], res["ade"][:, 1])
    t, curve = pkg.history.prediction_curve(res, eng.dt)
    assert curve.shape == (B, S) and np.isfinite(curve[:, :9]).all()
    # the replay gives the live loop's decisions
    rep = r.cutoffs()
    stack = lambda key: torch.stack([row[key] for row in live]).cpu().numpy()
    status, resp = stack("status"), stack("resp")
    assert np.array_equal(rep["status"], status) and np.array_equal(rep["cut"], stack("cut"))
    assert np.array_equal(rep["hit"], (stack("hit") != 0) & (status == 0)) and int(rep["hit"].sum()) >= 1
    assert np.array_equal(rep["idx"][~resp], stack("idx")[~resp])     # (a respawned ego's live index has been reset behind the tick)
    assert np.array_equal(r.cutoffs(chunk_ticks=7)["cut"], rep["cut"])
    # the same loop as one run(n)
    eng2, il2 = plan_loop(pkg, W, iroutes, n, record=n, record_plans=True)
    il2.run(n)
    torch.cuda.synchronize()
    assert_state_equal(loop_state(il), loop_state(il2), "run(n) against n ticks")
    for key in r.plans:
        assert torch.equal(r.plans[key], il2.recorder.plans[key]), key
    print(f"plan mode, {n} ticks x {B} egos: {int(rep['hit'].sum())} ego-ticks cut off, {int(resp.sum())} respawns, mean ade plan "
          f"{np.nanmean(res['ade']):.3f} m, constant {np.nanmean(const['ade']):.3f} m")


def test_the_references_plan_sharing_loop_with_both_recorders(pkg):
    g = load_golden("loop_interact_plan_T13.npz")
    ticks = g["ticks"]
    K, n = ticks.shape[:2]
    PL = pkg.planner
    rad, _ = PL.car_circles()
    full = [r.trajectory.copy() for r in PL.plan_routes([PL.intersection_query(int(tn), int(sp), rad) for sp, tn in g["egos"]], device=0)]
    eng = pkg.BatchedMPC([f.copy() for f in full], list(range(n)), dl=float(g["dl"]), T=13)
    x0 = torch.tensor([[f[0, 0], f[0, 1], 0.0, eng.paths[j][0, 2]] for j, f in enumerate(full)], dtype=torch.float64, device=eng.device)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[n], max_age=0, frame_window=int(g["frame_window"]), record=K, record_plans=True,
                             mate_prediction="plan")
    il.run(K)
    r = il.recorder
    oa, od, st = (r.plans[k].cpu().numpy() for k in ("plan_oa", "plan_od", "plan_status"))
    d = max(float(np.abs(oa - g["plan_oa"]).max()), float(np.abs(od - g["plan_od"]).max()))
    assert d <= 1e-6, d
    assert np.array_equal(st == 0, g["plan_ok"] != 0)
    out = r.cutoffs()
    assert not out["status"].any() and np.array_equal(out["idx"], ticks[:, :, 6].astype(np.int64))
    assert np.array_equal(out["cut"], ticks[:, :, 7].astype(np.int64))
    assert np.array_equal(out["hit"], ticks[:, :, 8] != 0) and int(out["hit"].sum()) == int(ticks[:, :, 8].sum()) >= 10
    print(f"interactive_mpc under the plan rule, recorded and replayed: {K} ticks, max plan difference {d:.2e}, {int(out['hit'].sum())} cuts")


def test_constant_mode_is_not_changed_by_the_plan_recorder(pkg, W, iroutes):
    n = 40
    eng_a, a = plan_loop(pkg, W, iroutes, n, mode="constant", record=n)
    eng_b, b = plan_loop(pkg, W, iroutes, n, mode="constant", record=n, record_plans=True)
    live = []
    for _ in range(n):
        a.tick()
        b.tick()
        for x, y in ((a.pre.status, b.pre.status), (a.pre.traj_idx, b.pre.traj_idx), (a.pre.col_flag, b.pre.col_flag), (eng_a.path_len, eng_b.path_len)):
            assert torch.equal(x, y)
        live.append({"status": b.pre.status.clone(), "hit": b.pre.col_flag.clone(), "cut": eng_b.path_len.clone()})
    torch.cuda.synchronize()
    assert_state_equal(loop_state(a), loop_state(b), "with and without record_plans")     # states, History, records
    assert a.recorder.plans is None and b.recorder.glue["record_plans"] is True and a.recorder.glue["record_plans"] is False
    r = b.recorder
    plan, const = r.predictions(egos="plan"), r.predictions(egos="constant")
    assert (plan["rule"], const["rule"], r.predictions()["rule"]) == ("plan", "constant", "constant")
    assert plan["ade"].shape == const["ade"].shape == (n, 6) and np.isfinite(plan["ade"]).all() and not bits_equal(plan["ade"], const["ade"])
    assert np.array_equal(plan["n"], const["n"])
    with pytest.raises(ValueError, match="holds no plans"):
        a.recorder.predictions(egos="plan")
    rep = r.cutoffs()                                                     # still the constant rule's replay
    stack = lambda key: torch.stack([row[key] for row in live]).cpu().numpy()
    assert np.array_equal(rep["status"], stack("status")) and np.array_equal(rep["cut"], stack("cut"))
    assert np.array_equal(rep["hit"], (stack("hit") != 0) & (stack("status") == 0))
    ref = a.recorder.cutoffs()                                            # (each loop has an engine of its own)
    assert all(np.array_equal(ref[k], rep[k]) for k in ("status", "idx", "cut", "hit"))


def test_edges_and_refusals_of_the_plan_recorder_and_the_replay(pkg, W, iroutes):
    cap, B, T = 5, 6, T_LIVE
    eng, il = plan_loop(pkg, W, iroutes, cap + 3, record=cap, record_plans=True)
    lib, ctx, dev = eng.lib, eng._ctx, eng.device
    r = il.recorder
    # caller-owned buffers with a guard slot on either side
    oa = torch.full((cap + 2, B, T), POISON_D, dtype=torch.float64, device=dev)
    od = torch.full((cap + 2, B, T), POISON_D, dtype=torch.float64, device=dev)
    st = torch.full((cap + 2, B), POISON_I, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    for B_, cap_, msg in ((B + 1, cap, f"has B={B} cap={cap}"), (B, cap + 1, f"has B={B} cap={cap}"), (B, cap - 1, f"has B={B} cap={cap}"), (-1, cap, "B=-1")):
        assert lib.jsim_loop_set_plan_recorder(ctx, B_, cap_, p(oa[1:]), p(od[1:]), p(st[1:])) == -22
        assert msg in lib.jsim_last_error(ctx).decode(), (B_, cap_)
    assert lib.jsim_loop_set_plan_recorder(ctx, B, cap, None, p(od[1:]), p(st[1:])) == -22
    assert lib.jsim_loop_set_plan_recorder(ctx, B, cap, p(oa[1:]), p(od[1:]), p(st[1:])) == 0
    il.run(cap + 3)                                                       # three ticks more than the record holds: dropped
    torch.cuda.synchronize()
    for t, poison in ((oa, POISON_D), (od, POISON_D), (st, POISON_I)):
        assert bool((t[0] == poison).all()) and bool((t[cap + 1] == poison).all()) and not bool((t[1:cap + 1] == poison).any())
    assert not bool(r.plans["plan_oa"].any())                             # the recorder's own tensors were replaced before the first tick
    with pytest.warns(RuntimeWarning, match="are not recorded"):
        assert r.ticks_run == cap + 3 and r.cutoffs()["cut"].shape == (cap, B)

    # the replay's refusals: every output still poison
    n = cap
    out_spec = [("status", np.int32, (), POISON_I), ("idx", np.int32, (), POISON_I), ("cut", np.int32, (), POISON_I), ("hit", np.int32, (), POISON_I),
                ("first", np.int32, (), POISON_I), ("col_xy", np.float64, (2,), POISON_D)]
    g = r.glue
    rec, flags, x_first, x_spawn = r._buffers()

    def replay(rc_want, **over):
        views, buf = guarded_outputs(out_spec, n, B, dev)
        a = dict(B=B, n=n, interacting=1, speed=0, plan_oa=p(oa[1:]), plan_od=p(od[1:]), plan_status=p(st[1:]), n_steps=g["n_steps"])
        a.update(over)
        rc = lib.jsim_loop_eval_cutoffs_plan(ctx, a["B"], a["n"], rec, flags, 0, None, x_first, x_spawn, g["frame_window"], g["margin"], a["n_steps"],
                                             a["speed"], a["interacting"], 0, 0, None, *(p(v) for v in views.values()), a["plan_oa"], a["plan_od"],
                                             a["plan_status"], None)
        return check_guarded(pkg, eng, "jsim_loop_eval_cutoffs_plan", out_spec, buf, n, rc, rc_want)
    good = replay(0)
    r.plans = {"plan_oa": oa[1:cap + 1], "plan_od": od[1:cap + 1], "plan_status": st[1:cap + 1]}
    with pytest.warns(RuntimeWarning):
        mine = r.cutoffs()
    assert all(np.array_equal(good[k], mine[k]) for k in ("status", "idx", "cut")) and np.array_equal(good["hit"] != 0, mine["hit"])
    who = "jsim_loop_eval_cutoffs_plan: "
    for kw, msg in ((dict(interacting=0), "interacting=0"), (dict(plan_oa=None), "null plan_oa"), (dict(plan_od=None), "null plan_oa"),
                    (dict(plan_status=None), "null plan_oa"), (dict(B=-1), "B=-1"), (dict(n_steps=65), "n_steps=65"), (dict(speed=1), "speed_cutoff"),
                    (dict(B=B + 1), "no groups set")):
        err = replay(-22, **kw)
        assert err.startswith(who) and msg in err, (kw, err)
    # a plan recorder goes with its recorder: clearing the one clears the other, and so does registering another
    pkg.recorder._register_recorder(eng, None)
    oa.fill_(POISON_D); od.fill_(POISON_D); st.fill_(POISON_I)
    il.run(2)
    torch.cuda.synchronize()
    assert bool((oa == POISON_D).all()) and bool((od == POISON_D).all()) and bool((st == POISON_I).all())
    assert lib.jsim_loop_set_plan_recorder(ctx, B, cap, p(oa[1:]), p(od[1:]), p(st[1:])) == -22     # no recorder to go with
    assert "has B=0 cap=0" in lib.jsim_last_error(ctx).decode()
    assert lib.jsim_loop_set_plan_recorder(ctx, B, 0, None, None, None) == 0
