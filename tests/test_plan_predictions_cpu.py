"""The plan record, its scoring and its replay without a device: the numpy restatement
(tests/plan_predictions_numpy.py) against the reference-made fixture, exactly, and on the reference's plan-sharing loop
(tests/golden/loop_interact_plan_T13.npz); the three exports against the header, the binding and the library; their -22 lists as far
as they need no context; the ValueErrors of Recorder and InteractingLoop ahead of any device work; the fixture's size."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import mate_plan_numpy as MP
import plan_prediction_cases as PC
import plan_predictions_numpy as PPN
import predictions_numpy as PN

NEW_EXPORTS = ("jsim_loop_set_plan_recorder", "jsim_loop_score_plan_predictions", "jsim_loop_eval_cutoffs_plan")


def test_the_restatement_equals_the_fixture_exactly():
    """Both roll Simulation.step's operations through the same libm; the fixture's samples are the reference's own."""
    g, groups = PC.fixture(), PC.all_groups()
    assert float(g["tol"]) == PC.TOL and float(g["dt"]) == PC.DT and float(g["tol_margin"]) >= 1e-6 and float(g["max_margin"]) >= 1e-6
    predictor = PC.cached(PPN.predict)
    for T, A in groups.items():
        for S in PC.STEPS:
            for n in PC.TICK_COUNTS:
                mine, ex = PC.restate(A, n, S, predictor=predictor), PC.expected(g, T, n, S)
                for k in ex:
                    assert PC.same_bits(np.ascontiguousarray(mine[k]), np.ascontiguousarray(ex[k])), (T, n, S, k)
                assert np.array_equal(np.isnan(mine["err"]), np.arange(S)[None, None, :] >= mine["pt_i"][:, :, :1])


def test_the_cases_are_what_they_are_meant_to_be():
    A = PC.recorder_arrays(13)
    r = PC.restate(A, PC.N, 64)
    i, d = r["pt_i"], r["pt_d"]
    n, hold = i[..., 0], i[..., 1]
    assert (d[:, 0, 2] == 0).all() and (hold[:, 0] == n[:, 0]).all() and A["plan_oa"][:10, 0].any()   # followed: error 0, hold = m
    assert (n[:, 0] == np.minimum(64, PC.N - np.arange(PC.N))).all()
    assert (d[:-1, 1, 3] < 0).all() and d[0, 1, 2] > 50 and (hold[:-4, 1] == 4).all()                  # the plan stands, the ego drives on
    for b, (e0, e1) in enumerate(((62, 127), (63, 128), (64, 129))):
        row = 2 + b
        assert (n[:e0 + 1, row] == np.minimum(64, e0 - np.arange(e0 + 1) + 1)).all() and n[e0 + 1, row] == min(64, e1 - e0)
        assert (d[:118, row, 2] == 0).all() and (d[118:124, row, 2] > 0).all() and (d[124:, row, 2] == 0).all()
        assert not A["plan_oa"][[e0 + 1, e1 + 1], row].any() and not A["plan_od"][[e0 + 1, e1 + 1], row].any()   # all zeros behind a respawn
        assert abs(A["x_spawn"][row, 0] - A["rec"][e0, row, 0]) > 300                                   # the spawn pose far away
    w = PC.WAKE
    assert (d[:w, 5:, 2] == 0).all() and (d[w:-1, 5:, 2] > 0).all() and (A["flags"][w - 1, 5:] & PC.AGE).all()
    assert np.abs(A["plan_od"][w:, 5]).max() > PC.MAX_STEER and abs(A["plan_od"][w + 1, 5, -1]) > PC.MAX_STEER
    assert (A["plan_status"][:, 8] == 1).all() and np.abs(A["plan_oa"][w:, 8]).max() > 1
    assert (A["plan_status"][:, 9] == 2).all() and abs(A["rec"][w, 9, 4]) > PC.MAX_STEER              # delta_last of tick w + 1
    # the speed clamps are met inside the predictions
    for b, lim in ((6, PC.MAX_SPEED), (7, PC.MIN_SPEED)):
        v = A["rec"][w + 4, b, 3]
        for a in A["plan_oa"][w + 5, b, 1:]:
            v = max(min(v + a * PC.DT, PC.MAX_SPEED), PC.MIN_SPEED)
        assert v == lim and A["rec"][w + 4, b, 3] != lim
    assert {A["plan_oa"].shape[2] for A in PC.all_groups().values()} == {13, 20, 40} and 35 in PC.STEPS and 64 in PC.STEPS


def test_fixture_stays_within_the_size_of_the_interacting_one():
    assert os.path.getsize(PC.FIXTURE) <= os.path.getsize(os.path.join(REPO, "tests", "golden", "loop_interact_T13.npz"))


def test_the_references_plan_sharing_loop_scored_by_the_restatement():
    """loop_interact_plan_T13.npz as a recording: from the stored plans and tick-start states the restatement makes the predictions the
    other ego saw to 1e-12, and its errors are the distances from those stored predictions to the stored later states."""
    g = load_golden("loop_interact_plan_T13.npz")
    ticks, preds = g["ticks"], g["preds"]
    n, B, S = preds.shape[:3]
    dt, L = 0.2, 2.86
    rec, flags = np.zeros((n, B, 7)), np.zeros((n, B), dtype=np.int32)
    x_first, x_spawn = ticks[0][:, [0, 1, 3, 2]].copy(), ticks[0][:, [0, 1, 3, 2]].copy()
    for k in range(n):
        for b in range(B):
            x, y, yaw, v, d, a = *ticks[k, b, :4], ticks[k, b, 12], ticks[k, b, 13]
            dc = max(min(d, MP.MAX_STEER), -MP.MAX_STEER)                   # the plant's step (mate_plan_numpy.predict_plan's)
            x, y, yaw = x + v * np.cos(yaw) * dt, y + v * np.sin(yaw) * dt, yaw + (v / L) * np.tan(dc) * dt
            v = max(min(v + a * dt, MP.MAX_SPEED), MP.MIN_SPEED)
            rec[k, b] = (x, y, yaw, v, d, a, 0.0)
            if k + 1 < n and ticks[k + 1, b, 14]:
                flags[k, b] = PN.GOAL
                x_spawn[b] = ticks[k + 1, b, [0, 1, 3, 2]]
            elif k + 1 < n:
                assert np.abs(rec[k, b, :4] - ticks[k + 1, b, :4]).max() <= 1e-12, (k, b)
                rec[k, b, :4] = ticks[k + 1, b, :4]                          # the stored state itself
    assert flags.any()
    worst = [0.0]
    at = {}

    def predictor(state, oa, od, status, delta_last, n_steps, dt_, L_):
        p = PPN.predict(state, oa, od, status, delta_last, n_steps, dt_, L_)
        k, b = at[np.asarray(state).tobytes() + np.asarray(oa).tobytes()]
        worst[0] = max(worst[0], float(np.abs(p - preds[k, b]).max()))
        return p
    for k in range(n):
        for b in range(B):
            at[ticks[k, b, [0, 1, 3, 2]].tobytes() + g["plan_oa"][k, b].tobytes()] = (k, b)
    status = np.where(g["plan_ok"] != 0, 0, 1).astype(np.int32)
    r = PPN.eval_plan_predictions(rec, flags, x_first, x_spawn, g["plan_oa"], g["plan_od"], status, S, 1.99, dt, L, predictor=predictor)
    assert worst[0] <= 1e-12, worst[0]
    m = r["pt_i"][:, :, 0]
    checked = 0
    for k in range(n):
        for b in range(B):
            assert m[k, b] == min(S, PN.ego_horizon(flags[:, b], k) - k + 1) >= 1
            for j in range(m[k, b]):
                dx, dy = preds[k, b, j, 0] - rec[k + j, b, 0], preds[k, b, j, 1] - rec[k + j, b, 1]
                assert abs(r["err"][k, b, j] - np.sqrt(dx * dx + dy * dy)) <= 1e-11, (k, b, j)
                checked += 1
    assert checked > 1000 and np.nanmax(r["err"]) > 0.1
    print(f"plan-sharing loop scored: {checked} samples, max prediction difference {worst[0]:.2e}, mean ade {np.nanmean(r['pt_d'][:, :, 0]):.3f} m")


def test_the_exports_against_the_header_the_binding_and_the_library(pkg):
    H = pkg.history
    hdr = pkg._header.header().functions
    pkg.build.build()
    lib = pkg._cabi.load()
    decl = {}
    for name in NEW_EXPORTS:
        decl[name] = [f"{t} {p}".replace("* ", "*") for t, p in hdr[name].params]   # `const double *rec`, `int32_t B`
        fn = getattr(lib, name)                                              # the library exports it
        assert len(fn.argtypes) == len(decl[name]), name
    names = lambda ps: [re.search(r"(\w+)$", p).group(1) for p in ps]
    # the scoring call writes PREDICTION_OUTPUTS' tensors, in that order, and reads the plan record's, in PLAN_RECORD's
    ps = decl["jsim_loop_score_plan_predictions"]
    written = [nm for nm, p in zip(names(ps)[1:-1], ps[1:-1]) if "*" in p and not p.startswith("const ")]
    assert written == list(H.PREDICTION_OUTPUTS.keys()) and names(ps)[-6:-1] == written and (names(ps)[0], names(ps)[-1]) == ("ctx", "stream")
    plan_keys = [k for k, _, _ in H.PLAN_RECORD]
    assert plan_keys == ["plan_oa", "plan_od", "plan_status"] and names(ps)[7:10] == plan_keys
    assert names(decl["jsim_loop_set_plan_recorder"]) == ["ctx", "B", "cap"] + plan_keys
    for (k, dt, trail), p in zip(H.PLAN_RECORD, decl["jsim_loop_set_plan_recorder"][3:]):
        assert p.startswith("int32_t *" if dt == np.int32 else "double *") and trail == (() if dt == np.int32 else ("T",)), k
    # the replay is jsim_loop_eval_cutoffs' argument list plus the three plan pointers
    old = [f"{t} {p}".replace("* ", "*") for t, p in hdr["jsim_loop_eval_cutoffs"].params]
    new = decl["jsim_loop_eval_cutoffs_plan"]
    assert new[:len(old) - 1] == old[:-1] and names(new[len(old) - 1:]) == plan_keys + ["stream"]
    assert all(p.startswith("const ") for p in new[len(old) - 1:-1])
    assert len(lib.jsim_loop_eval_cutoffs.argtypes) == len(old) and lib.jsim_abi_version() == 2
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "\n## 29. " in design and all(e in design[design.index("\n## 29. "):] for e in NEW_EXPORTS)


def test_argument_errors_without_gpu(pkg):
    """The header's -22 lists as far as they need no context: from the host, before any device call; the null ctx is refused last."""
    lib = pkg._cabi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                    # a non-null address; no refused call reads it

    def caller(fn, names, good):
        def call(**over):
            a = {k: p for k in names}
            a.update(good)
            a.update(over)
            rc = getattr(lib, fn)(None, *[a[k] for k in names], *([None] if fn != "jsim_loop_set_plan_recorder" else []))
            return rc, lib.jsim_last_error(None).decode()
        return call

    who = "jsim_loop_score_plan_predictions: "
    names = ("B", "n_ticks", "rec", "flags", "x_first", "x_spawn", "plan_oa", "plan_od", "plan_status", "n_steps", "tol", "pt_i", "pt_d",
             "step_sum", "step_cnt", "err")
    call = caller("jsim_loop_score_plan_predictions", names, dict(B=2, n_ticks=3, n_steps=35, tol=1.5))
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_ticks=-1), "n_ticks=-1"), (dict(n_steps=0), "n_steps=0 outside [1, 64]"),
                    (dict(n_steps=65), "n_steps=65 outside [1, 64]"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"),
                    (dict(tol=float("inf")), "tol")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in ("rec", "flags", "x_first", "x_spawn", "plan_oa", "plan_od", "plan_status", "pt_i", "pt_d", "step_sum", "step_cnt"):
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null pointer " + k, (k, rc, err)
        assert call(n_ticks=0, **{k: None})[0] == -22 and call(B=0, **{k: None})[0] == -22, k     # also with nothing to do
    for kw in ({}, dict(err=None), dict(n_ticks=0), dict(B=0)):           # every argument good: the missing context is what is left
        rc, err = call(**kw)
        assert rc == -22 and err == who + "null ctx", (kw, rc, err)

    who = "jsim_loop_eval_cutoffs_plan: "
    names = ("B", "n_ticks", "rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "frame_window", "margin", "n_steps", "speed_cutoff",
             "interacting", "chunk_ticks", "first_tick", "carry", "status", "idx", "cut", "hit", "first", "col_xy", "plan_oa", "plan_od",
             "plan_status")
    call = caller("jsim_loop_eval_cutoffs_plan", names, dict(B=2, n_ticks=3, n_obs=1, frame_window=20, margin=5, n_steps=35, speed_cutoff=0,
                                                              interacting=1, chunk_ticks=0, first_tick=0))
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_steps=65), "n_steps=65"), (dict(frame_window=33), "frame_window=33"),
                    (dict(first_tick=4), "first_tick=4"), (dict(obs_rec=None), "null obs_rec"), (dict(status=None), "null device pointer"),
                    (dict(plan_oa=None), "null plan_oa"), (dict(plan_od=None), "null plan_oa"), (dict(plan_status=None), "null plan_oa"),
                    (dict(interacting=0), "interacting=0"), (dict(interacting=2), "interacting=2")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for kw in ({}, dict(carry=None), dict(n_obs=0, obs_rec=None)):
        rc, err = call(**kw)
        assert rc == -22 and err == who + "null ctx", (kw, rc, err)
    # the existing export keeps its behaviour: interacting = 0 gets as far as the missing context
    rc = lib.jsim_loop_eval_cutoffs(None, 2, 3, p, p, 1, p, p, p, 20, 5, 35, 0, 0, 0, 0, p, p, p, p, p, p, p, None)
    assert rc == -22 and lib.jsim_last_error(None).decode() == "jsim_loop_eval_cutoffs: null ctx"

    who = "jsim_loop_set_plan_recorder: "
    call = caller("jsim_loop_set_plan_recorder", ("B", "cap", "plan_oa", "plan_od", "plan_status"), dict(B=2, cap=3))
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(cap=-1), "cap=-1"), (dict(plan_oa=None), "needs"), (dict(plan_od=None), "needs"),
                    (dict(plan_status=None), "needs")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for kw in ({}, dict(cap=0), dict(cap=0, plan_oa=None, plan_od=None, plan_status=None)):
        rc, err = call(**kw)
        assert rc == -22 and err == who + "null ctx", (kw, rc, err)


def stand_in(glue, plans=False, superseded=False):
    """A recorder without a device: what _predictions_device and _cutoffs_device read ahead of their first device call."""
    eng = types.SimpleNamespace(B=3, device=torch.device("cpu"), ego_shape=(1.93, 0.93, 1.7), L=2.86, dt=0.2)
    r = types.SimpleNamespace(loop=types.SimpleNamespace(eng=eng), glue=glue, superseded=superseded, n_obs=2, obs=None)
    if plans is not False:
        r.plans = plans
    r._ego_shape = lambda: eng.ego_shape

    def touched(*a, **k):
        raise AssertionError("device work ahead of a bad argument")
    r._n = r._buffers = r._call = touched
    return r


def test_recorder_value_errors_before_any_device_work(pkg):
    P, Cut = pkg.recorder.Recorder._predictions_device, pkg.recorder.Recorder._cutoffs_device
    plan = {"frame_window": 20, "margin": 5, "n_steps": 35, "mode": "truncate", "interacting": True, "mate_prediction": "plan"}
    const = dict(plan, mate_prediction="constant")
    held = {"plan_oa": None, "plan_od": None, "plan_status": None}          # (any object but None: the check is `holds plans`)
    for glue in (plan, const, None, {"n_steps": 35, "interacting": False}):
        for plans in (False, None):                                       # no attribute (an older stand-in), or none held
            with pytest.raises(ValueError, match="holds no plans"):
                P(stand_in(glue, plans), egos="plan")
    with pytest.raises(ValueError, match="not recorded"):                   # as before this record existed
        P(stand_in(plan), egos=True)
    with pytest.raises(ValueError, match="not recorded"):
        Cut(stand_in(plan))
    with pytest.raises(ValueError, match="replaced"):
        P(stand_in(plan, held, superseded=True), egos="plan")
    with pytest.raises(ValueError, match="replaced"):
        Cut(stand_in(plan, held, superseded=True))
    with pytest.raises(ValueError, match="egos must be"):
        P(stand_in(plan, held), egos="Plan")
    # with plans every spelling gets as far as the device
    for glue, kw in ((plan, dict(egos="plan")), (plan, dict(egos=True)), (plan, {}), (const, dict(egos="plan")), (plan, dict(egos="constant")),
                     (plan, dict(egos=False))):
        with pytest.raises(AssertionError, match="device work"):
            P(stand_in(glue, held), **kw)
    with pytest.raises(AssertionError, match="device work"):
        Cut(stand_in(plan, held))


def test_loops_refuse_record_plans_before_any_device_work(pkg):
    """An object with nothing but B stands in for the engine: the keyword is checked before the engine is touched."""
    eng = types.SimpleNamespace(B=4)
    with pytest.raises(ValueError, match="record_plans"):
        pkg.InteractingLoop(eng, None, group_sizes=[4], record_plans=True)
    with pytest.raises(ValueError, match="record_plans"):
        pkg.InteractingLoop(eng, None, group_sizes=[4], record=0, record_plans=True, mate_prediction="plan")
    # ScenarioLoop and ClosedLoop do not take the keyword at all
    with pytest.raises(TypeError, match="record_plans"):
        pkg.ScenarioLoop(eng, None, (), record=8, record_plans=True)
    with pytest.raises(TypeError, match="record_plans"):
        pkg.ClosedLoop(eng, None, record=8, record_plans=True)
