"""Every recorded prediction against what the vehicle then did, without a device: the numpy restatement against
the reference-made fixture, exactly; the two history helpers; the output table against the header's declaration and the binding's
argtypes; the ValueErrors of Recorder.predictions on a stand-in recorder."""
import os
import types

import numpy as np
import pytest
import torch

import prediction_cases as PC
import predictions_numpy as PN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restatement_equals_the_fixture_exactly():
    """Both call the same libm; the fixture's samples are the reference's own state_prediction."""
    assert os.path.getsize(PC.FIXTURE) < 100000
    g, A = PC.fixture(), PC.recorder_arrays()
    assert float(g["tol"]) == PC.TOL and float(g["dt"]) == PC.DT and float(g["tol_margin"]) >= 1e-6 and float(g["max_margin"]) >= 1e-6
    predictor = PC.prefix_predictor()
    for S in PC.STEPS:
        for n in PC.TICK_COUNTS:
            mine, ex = PC.restate(A, n, S, predictor=predictor), PC.expected(g, n, S)
            for k in ex:
                assert PC.same_bits(np.ascontiguousarray(mine[k]), np.ascontiguousarray(ex[k])), (n, S, k)
            assert np.array_equal(np.isnan(mine["err"]), np.arange(S)[None, None, :] >= mine["pt_i"][:, :, :1])


def test_the_cases_are_what_they_are_meant_to_be():
    A = PC.recorder_arrays()
    r = PC.restate(A, PC.N, 64)
    i, d = r["pt_i"], r["pt_d"]
    n, hold, max_at = i[..., 0], i[..., 1], i[..., 2]
    assert (n[:, :PC.N_OBS] == np.minimum(64, PC.N - 1 - np.arange(PC.N))[:, None]).all() and (n[-1, :PC.N_OBS] == 0).all()
    assert np.isnan(d[-1, :PC.N_OBS]).all() and (max_at[-1, :PC.N_OBS] == -1).all()
    assert (d[:-1, 0, 2] == 0).all() and (hold[:, 0] == n[:, 0]).all()              # straight: error 0, hold = m
    assert (hold[:-1, 5] == 0).all() and (hold[:-64, 6] == 63).all()                  # the tolerance at sample 0 and at sample 63
    assert d[0, 1, 2] > 10 and (d[20:-1, 1, 2] == 0).all()                           # parked, then off
    assert d[150, 2, 2] > 1 and d[150, 4, 2] > 0.5 and d[150, 3, 2] > 1             # the turn, the cyclist, the brake
    assert (d[:120, 3, 2] == 0).all() and A['obs'][0, 3, 4] == 0.5                 # a != 0 predicted exactly
    # the egos' horizons stop at their episodes' ends, which stand on ticks 62 / 63 / 64 and 127 / 128 / 129
    for b, (e0, e1) in enumerate(((62, 127), (63, 128), (64, 129))):
        row = PC.N_OBS + 1 + b
        assert (n[:e0 + 1, row] == np.minimum(64, e0 - np.arange(e0 + 1) + 1)).all() and n[e0 + 1, row] == min(64, e1 - e0)
        assert (d[:, row, 2] == 0).all()                                             # a horizon one too long meets the spawn pose
    assert d[30, PC.N_OBS, 3] > 1 and d[30, PC.N_OBS, 4] == 0                        # the braking ego: predicted farther ahead
    assert (d[:171, PC.N_OBS + 4, 2] == 0).all() and d[171, PC.N_OBS + 4, 2] > 0


def test_prediction_curve(pkg):
    res = {"step_sum": np.array([[1.0, 4.0, 0.0], [0.0, 0.0, 0.0]]), "step_cnt": np.array([[2, 2, 0], [5, 0, 0]], dtype=np.int32)}
    t, mean = pkg.history.prediction_curve(res, 0.2)
    assert np.array_equal(t, (np.arange(3) + 1) * 0.2)
    assert np.array_equal(mean[0, :2], [0.5, 2.0]) and np.isnan(mean[0, 2]) and mean[1, 0] == 0.0 and np.isnan(mean[1, 1:]).all()
    with pytest.raises(ValueError):
        pkg.history.prediction_curve({"step_sum": np.zeros((2, 3)), "step_cnt": np.zeros((2, 2))}, 0.2)


def test_prediction_places(pkg):
    """Eight places in conflicts()' order: the ego's vehicles, then its mates without itself; the ninth is not there."""
    H = pkg.history
    n, n_obs, B = 3, 7, 4
    V = n_obs + B
    res = {k: (np.arange(n * V).reshape(n, V) + j).astype(np.int32 if k in H.PS_INT else np.float64) for j, k in enumerate(H.PS_INT + H.PS_DOUBLE)}
    res.update(n_obs=n_obs, egos=True)
    veh = np.array([[0, 7], [0, 3], [3, 7], [7, 7]], dtype=np.int32)
    mate = np.array([[0, 4], [0, 4], [0, 0], [3, 4]], dtype=np.int32)
    out = H.prediction_places(res, veh, mate)
    assert out["row"].tolist() == [[0, 1, 2, 3, 4, 5, 6, 8], [0, 1, 2, 7, 9, 10, -1, -1], [3, 4, 5, 6, -1, -1, -1, -1], [-1] * 8]   # ego 0: 7 + 3 > 8
    for k in H.PS_INT + H.PS_DOUBLE:
        assert out[k].shape == (n, B, 8) and out[k].dtype == res[k].dtype
        assert np.array_equal(out[k][:, 1, :6], res[k][:, [0, 1, 2, 7, 9, 10]])
        gone = out[k][:, 1, 6:]
        assert (gone == -1).all() if k in H.PS_INT else np.isnan(gone).all()
    res["egos"] = False                                                 # the egos were not scored: no mate has a row
    res = {k: (v[:, :n_obs] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    assert H.prediction_places(res, veh, mate)["row"].tolist()[1] == [0, 1, 2, -1, -1, -1, -1, -1]
    with pytest.raises(ValueError):
        H.prediction_places(res, veh, mate[:2])
    with pytest.raises(ValueError):
        H.prediction_places(res, veh + 5, mate)


def test_the_output_table_against_the_header_and_the_binding(pkg):
    H = pkg.history
    T = H.PREDICTION_OUTPUTS
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    params, names = map(list, zip(*pkg._header.header().functions[T.entry].params))       # the types' text, the names
    written = [nm for nm, p in zip(names[1:-1], params[1:-1]) if "*" in p and not p.startswith("const ")]
    assert written == list(T.keys()) and names[-len(written) - 1:-1] == written and (names[0], names[-1]) == ("ctx", "stream")
    for (k, dt, lead, trail), p in zip(T.outputs, params[-len(written) - 1:-1]):
        assert p.startswith("int32_t *" if dt == np.int32 else "double *") and lead in ("tick", "row"), k
    assert len(getattr(pkg._cabi.load(), T.entry).argtypes) == len(params)
    assert T.optional == ("err",) and T.keys(skip=T.optional) == ("pt_i", "pt_d", "step_sum", "step_cnt")
    # the columns are the enumerators, in their order
    for prefix, cols, last in (("JSIM_PS_", H.PS_INT, "NI"), ("JSIM_PS_", H.PS_DOUBLE, "ND")):
        want = ", ".join([f"{prefix}{cols[0].upper()} = 0"] + [prefix + c.upper() for c in cols[1:]] + [prefix + last])
        assert "enum { " + want + " };" in hdr, want
    assert dict((k, tr) for k, _, _, tr in T.outputs)["pt_i"] == (len(H.PS_INT),)
    assert H.MAX_PRED == pkg._header.constant("JSIM_MAX_PRED") == 64
    assert tuple(H.EVALUATORS) == ("reasons", "conflicts", "gaps", "static", "tracking", "headway", "cutoffs")    # that table is left alone
    assert PN.PS_INT == H.PS_INT and PN.PS_DOUBLE == H.PS_DOUBLE
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "\n## 28. " in design and T.entry in design[design.index("\n## 28. "):]


def stand_in(pkg, glue, superseded=False):
    """A recorder without a device: what _predictions_device reads ahead of its first device call."""
    eng = types.SimpleNamespace(B=3, device=torch.device("cpu"), ego_shape=(1.93, 0.93, 1.7), L=2.86, dt=0.2)
    r = types.SimpleNamespace(loop=types.SimpleNamespace(eng=eng), glue=glue, superseded=superseded, n_obs=2, obs=None)
    r._ego_shape = lambda: eng.ego_shape

    def touched(*a, **k):
        raise AssertionError("device work ahead of a bad argument")
    r._n = r._buffers = r._call = touched
    return r


@pytest.mark.parametrize("kw", (dict(n_steps=0), dict(n_steps=65), dict(n_steps=-3), dict(n_steps=3.5), dict(n_steps=True), dict(tol=-1e-9),
                                dict(tol=float("nan")), dict(tol=float("inf")), dict(egos="plan"), dict(egos=2), dict(egos=-1), dict(egos=0.5), dict(egos="yes"),
                                dict(n_steps=float("inf")), dict(n_steps=float("nan")), dict(n_steps="35"), dict(n_steps=np.True_)))
def test_bad_arguments_raise_before_any_device_work(pkg, kw):
    glue = {"n_steps": 35, "interacting": True, "mate_prediction": "constant"}
    with pytest.raises(ValueError):
        pkg.recorder.Recorder._predictions_device(stand_in(pkg, glue), **kw)


def test_plan_mode_and_superseded_recorders(pkg):
    P = pkg.recorder.Recorder._predictions_device
    plan = {"n_steps": 35, "interacting": True, "mate_prediction": "plan"}
    with pytest.raises(ValueError, match="plan"):
        P(stand_in(pkg, plan), egos=True)
    with pytest.raises(ValueError, match="replaced"):
        P(stand_in(pkg, plan, superseded=True), egos="constant")
    # a good call gets as far as the device: the stand-in's first device-side method
    with pytest.raises(ValueError, match="plan"):                       # 1 and numpy's True stand for True
        P(stand_in(pkg, plan), egos=1)
    with pytest.raises(ValueError, match="plan"):
        P(stand_in(pkg, plan), egos=np.True_)
    for glue, kw in ((plan, dict(egos="constant")), (plan, {}), (plan, dict(egos=0)), (plan, dict(egos=np.False_)), (None, {}),
                     (None, dict(n_steps=np.int64(64), egos=1)), (None, dict(n_steps=35.0)), ({"n_steps": 64, "interacting": False}, dict(tol=0.0, egos=True))):
        with pytest.raises(AssertionError, match="device work"):
            P(stand_in(pkg, glue), **kw)


def test_argument_errors_without_gpu(pkg):
    """The header's -22 list as far as it needs no context: from the host, before any device call; the null ctx is refused last."""
    lib = pkg._cabi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                    # a non-null address; no refused call reads it
    names = ("B", "n_ticks", "rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "egos", "n_steps", "tol", "pt_i", "pt_d", "step_sum",
             "step_cnt", "err")

    def call(**over):
        a = {k: p for k in names}
        a.update(B=2, n_ticks=3, n_obs=2, egos=1, n_steps=35, tol=1.5)
        a.update(over)
        rc = lib.jsim_loop_score_predictions(None, *[a[k] for k in names], None)
        return rc, lib.jsim_last_error(None).decode()

    who = "jsim_loop_score_predictions: "
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_ticks=-1), "n_ticks=-1"), (dict(n_obs=-1), "n_obs=-1"), (dict(n_steps=0), "n_steps=0 outside [1, 64]"),
                    (dict(n_steps=65), "n_steps=65 outside [1, 64]"), (dict(egos=2), "egos=2"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"),
                    (dict(obs_rec=None), "null obs_rec with n_obs=2")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in ("rec", "flags", "x_first", "x_spawn", "pt_i", "pt_d", "step_sum", "step_cnt"):
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null pointer " + k, (k, rc, err)
        assert call(n_ticks=0, **{k: None})[0] == -22, k                   # also with nothing to do
    for kw in ({}, dict(err=None), dict(n_ticks=0), dict(n_obs=0, egos=0, obs_rec=None)):   # every argument good: the missing context is what is left
        rc, err = call(**kw)
        assert rc == -22 and err == who + "null ctx", (kw, rc, err)
