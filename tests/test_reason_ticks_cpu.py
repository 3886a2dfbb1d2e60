"""Per-tick stakeholder reasons and the replan trigger (jsim_loop_eval_reasons) without a GPU: the numpy
restatement against the reference-made fixture (tests/golden/reason_ticks.npz), the restatement-made part regenerated bit for bit,
the fixture's conditions, the host-side pieces (history.reason_series, reasons.tick_inputs) and the C entry point's declaration,
binding, documentation and -22 list against the cross-compiled library."""
import os
import re

import numpy as np
import pytest

import reason_ticks_cases as TC
from conftest import REPO


@pytest.fixture(scope="module")
def cs():
    return TC.cases()


@pytest.fixture(scope="module")
def arrays(cs):
    return TC.recorder_arrays(cs)


@pytest.fixture(scope="module")
def restated(arrays):
    return TC.restate(arrays)


def test_cases_are_the_stored_ones(cs):
    g = TC.fixture()
    assert int(g["n_cases"]) == len(cs) == 27 and g["pos"].shape == (27, TC.N, 2)
    for b, c in enumerate(cs):
        assert str(g["labels"][b]) == c["label"] and bool(g["restated"][b]) == c["restated"] and int(g["veh"][b]) == c["veh"]
        for k in ("pos", "cyc", "flags", "par", "carry"):
            assert np.array_equal(g[k][b], c[k]), (b, k)
        assert g["threshold"][b] == c["threshold"]
    assert sorted(np.flatnonzero(g["restated"]).tolist()) == [25, 26]


def test_restatement_reproduces_the_reference(cs, restated):
    g = TC.fixture()
    worst = 0.0
    for b, c in enumerate(cs):
        if c["restated"]:
            continue
        assert np.array_equal(restated["timers"][:, b], g["timers"][b]), c["label"]
        trig = restated["trig"][:, b]
        assert np.array_equal((trig & 1) != 0, g["needed"][b]), c["label"]
        below = np.stack([g["val"][b, :, q] < c["threshold"] for q in range(3)], axis=1)
        assert np.array_equal(((trig[:, None] >> np.arange(1, 4)) & 1) != 0, below), c["label"]
        first = int(np.argmax(g["needed"][b])) if g["needed"][b].any() else -1
        assert restated["first"][b] == first, c["label"]
        # the reference's own comparison of each timer with its threshold, where the tick is in range
        rng = np.array([c["par"][5] + c["par"][6], c["par"][8] + c["par"][9]])
        inr = g["val"][b, :, 3, None] < rng
        on = restated["timers"][:, b] >= c["par"][[7, 10]]
        assert np.array_equal(on & inr, g["on"][b] & inr), c["label"]
        np.testing.assert_allclose(restated["val"][:, b], g["val"][b], rtol=1e-13, atol=0, err_msg=c["label"])
        worst = max(worst, float(np.max(np.abs(restated["val"][:, b] - g["val"][b]) / np.abs(g["val"][b]))))
        # the tracker the reference leaves after every tick is the carry a run cut there hands on
        for n in TC.TICK_COUNTS:
            cut = TC.restate(_one(c), n=n)
            ended = bool(c["flags"][n - 1] & (TC.GOAL | TC.AGE))
            want = (0.0, 0.0, 0.0) if ended else (g["timers"][b, n - 1, 0], g["timers"][b, n - 1, 1], float(g["tracker"][b, n - 1]))
            assert tuple(cut["carry"][0]) == want, (c["label"], n)
            assert cut["first"][0] == (first if 0 <= first < n else -1), (c["label"], n)
    print("restatement against the reference: maximum relative error", worst)


_ONE = {}


def _one(c):
    if c["label"] not in _ONE:
        _ONE[c["label"]] = TC.recorder_arrays([c])
    return _ONE[c["label"]]


def test_restatement_made_cases_regenerate_bit_for_bit(cs, arrays, restated):
    g = TC.fixture()
    for b, c in enumerate(cs):
        if not c["restated"]:
            continue
        assert np.array_equal(restated["val"][:, b], g["val"][b], equal_nan=True), c["label"]
        assert np.array_equal(restated["timers"][:, b], g["timers"][b]) and np.array_equal((restated["trig"][:, b] & 1) != 0, g["needed"][b])
    none = restated["val"][:, 25]
    assert np.isnan(none[:, 1:]).all() and np.array_equal(none[:, 0], restated["val"][:, 0, 0])      # the policymaker is still evaluated
    assert not restated["timers"][:, 25].any() and not (restated["trig"][:, 25] & 0xc).any()
    for s in TC.SPLITS:
        head = TC.restate(arrays, n=s)
        assert np.array_equal(head["carry"], g[f"split_{s}_carry"])
        tail = TC.restate(arrays, n=TC.N - s, carry=head["carry"], k0=s)
        for k in ("val", "timers", "trig"):
            assert np.array_equal(np.concatenate([head[k], tail[k]]), restated[k], equal_nan=True), (s, k)
        assert np.array_equal(tail["carry"], restated["carry"])
        first = np.where(head["first"] >= 0, head["first"], np.where(tail["first"] >= 0, tail["first"] + s, -1))
        assert np.array_equal(first, restated["first"])


def test_fixture_conditions_hold(cs):
    g = TC.fixture()
    assert np.all(g["margins"] >= 1e-9) and int(g["on_grid"]) > 0
    m = {"range": np.inf, "timer": np.inf, "value": np.inf, "centre": np.inf}
    near = 0
    for b, c in enumerate(cs):
        if c["veh"] < 0:
            continue
        par, dist = c["par"], g["val"][b, :, 3]
        rng = np.array([par[5] + par[6], par[8] + par[9]])
        m["range"] = min(m["range"], np.abs(dist[:, None] - rng).min())
        tm = np.abs(g["timers"][b] - par[[7, 10]])[dist[:, None] < rng]
        near += int((tm < 1e-9).sum())
        m["timer"] = min(m["timer"], tm[tm >= 1e-9].min(initial=np.inf))
        m["value"] = min(m["value"], np.abs(g["val"][b, :, :3] - c["threshold"]).min())
        m["centre"] = min(m["centre"], np.abs((c["pos"][:, 0] - par[4] / 2) - par[3]).min())
    assert [m["range"], m["timer"], m["value"], m["centre"]] == g["margins"].tolist() and near == int(g["on_grid"])


def test_fixture_meets_the_kernel_structure(cs):
    """The events each case is named after are where the name says, read from the reference's data."""
    g = TC.fixture()
    inr = lambda b: g["val"][b, :, 3, None] < np.array([cs[b]["par"][5] + cs[b]["par"][6], cs[b]["par"][8] + cs[b]["par"][9]])
    first_on = lambda b, q: int(np.argmax(g["on"][b, :, q] & inr(b)[:, q]))
    assert [(first_on(b, 0), first_on(b, 1)) for b in range(1, 7)] == [(63, 63), (63, 63), (64, 64), (64, 64), (65, 65), (65, 65)]
    assert sorted({float(cs[b]["par"][0]) for b in range(1, 7)}) == [0.1, 0.2] and all(cs[b]["carry"][:2].all() for b in range(1, 7))
    enter = lambda b, q: int(np.argmax(inr(b)[:, q]))
    assert (enter(9, 0), enter(9, 1), enter(10, 0), enter(10, 1)) == (64, 65, 65, 66)
    last = lambda b, q: int(np.flatnonzero(inr(b)[:, q])[-1])
    assert (last(11, 1), last(11, 0), last(12, 1), last(12, 0)) == (63, 64, 64, 65)
    assert np.flatnonzero(inr(13)[:, 0]).tolist() == np.flatnonzero(inr(13)[:, 1]).tolist() == [70, 130]
    below = lambda b: (g["val"][b, :, :3] < cs[b]["threshold"]).any(axis=1)
    assert np.flatnonzero(below(14)).tolist() == [62, 63, 64, 65, 66] and np.flatnonzero(g["needed"][14]).tolist() == [62]
    assert int(np.argmax(below(15))) == 64 and np.flatnonzero(g["needed"][15]).tolist() == [64]
    assert below(16)[63] and not below(16)[64] and np.flatnonzero(g["needed"][16]).tolist() == [60, 100]
    assert [np.flatnonzero(cs[b]["flags"]).tolist() for b in (17, 18, 19, 20)] == [[0, TC.N - 1], [62], [63], [64]]
    assert [np.flatnonzero(g["needed"][b]).tolist() for b in (17, 18, 19, 20)] == [[1], [0, 63], [0, 64], [0, 65]]
    assert g["timers"][19, 63].min() > 6.0 and g["timers"][19, 64].tolist() == [cs[19]["par"][0]] * 2                    # the reset
    rows = np.stack([c["par"] for c in cs])
    for col in (0, 3, 4, 5, 6, 7, 8, 9, 10):
        assert len(set(rows[:, col].tolist())) >= 3, col
    assert sorted(set(g["threshold"].tolist())) == [0.7, 0.95] and g["needed"][23].any() and g["needed"][24].any()


def test_reason_series_splits_like_the_histories(pkg, cs, restated):
    H = pkg.history
    A = TC.recorder_arrays(cs)
    vals = {"policymaker": restated["val"][:, :, 0], "driver": restated["val"][:, :, 1], "cyclist": restated["val"][:, :, 2]}
    series = H.reason_series(vals, A["flags"], 0.1)
    assert len(series) == len(cs)
    for b in (0, 17, 19, 20):
        bounds = H.episode_bounds(A["flags"][:, b])
        hs = H.ego_histories(A["rec"][:, b], A["flags"][:, b], 0.1, A["x_first"][b], A["x_spawn"][b])
        assert len(series[b]) == len(bounds) == len(hs)
        for ep, (k0, k1, _), h in zip(series[b], bounds, hs):
            assert len(h) == k1 - k0 + 1 and set(ep) == {"time_values", "reasons_policymaker_values", "reasons_driver_values", "reasons_cyclist_values"}
            assert ep["time_values"] == [i * 0.1 for i in range(k1 - k0)]
            assert ep["reasons_cyclist_values"] == restated["val"][k0:k1, b, 2].tolist() and ep["reasons_policymaker_values"] == restated["val"][k0:k1, b, 0].tolist()
            assert all(isinstance(v, float) for v in ep["reasons_driver_values"] + ep["time_values"])
    assert [len(e["time_values"]) for e in series[17]] == [1, TC.N - 1, 0]


def test_tick_inputs_refuse_what_the_c_call_cannot_see(pkg):
    R = pkg.reasons
    par, thr, veh, car = R.tick_inputs(3, 2, 0.2)
    assert par.shape == (3, 12) and par[0, 0] == 0.2 and np.array_equal(par[1, 1:], R.par_row()[1:])
    assert thr.tolist() == [0.7] * 3 and veh.tolist() == [0, 0, 0] and veh.dtype == np.int32 and not car.any()
    par, thr, veh, car = R.tick_inputs(3, 2, 0.2, par=np.stack([R.par_row(dt=d) for d in (0.1, 0.2, 0.3)]), threshold=[0.7, 0.8, 0.9],
                                       cyclist=[1, -1, 0], carry=np.ones((3, 3)), default_cyclist=lambda: 1 / 0)
    assert par[:, 0].tolist() == [0.1, 0.2, 0.3] and veh.tolist() == [1, -1, 0] and car.all()
    assert R.tick_inputs(3, 2, 0.2, default_cyclist=lambda: np.array([1, -1, 0], dtype=np.int32))[2].tolist() == [1, -1, 0]
    for kw in (dict(par=np.zeros(11)), dict(par=np.zeros((2, 12))), dict(par=R.par_row(dt=0.0)), dict(par=R.par_row(dt=-0.1)),
               dict(par=R.par_row(dt=np.inf)), dict(par=R.par_row(width=np.nan)), dict(threshold=np.nan), dict(threshold=[0.7, 0.7]),
               dict(cyclist=2), dict(cyclist=-2), dict(cyclist=[0, 0]), dict(cyclist=0.0), dict(carry=np.zeros((3, 2))),
               dict(carry=np.full((3, 3), np.nan))):
        with pytest.raises(ValueError):
            R.tick_inputs(3, 2, 0.2, **kw)


def test_entry_point_is_declared_exported_and_documented(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    H = pkg._header.header()
    assert H.functions["jsim_loop_eval_reasons"].ret == "int" and len(H.functions["jsim_loop_eval_reasons"].params) == 18
    assert "evaluate_reasons (:127-128," in hdr and "reasons_evaluation (:141-142, :1907-1940)" in hdr        # what it replaces
    assert H.constants["JSIM_ABI_VERSION"] == 2
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_eval_reasons.argtypes) == 18 and lib.jsim_abi_version() == 2
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert re.search(r"^\| `jsim_loop_eval_reasons` \|", doc, flags=re.M)
    assert callable(pkg.reasons.situation_at) and callable(pkg.history.reason_series) and callable(pkg.closed_loop.Recorder.reasons)
    src = open(os.path.join(REPO, "av-simulation-at-intersections_amd", "csrc", "jsim_mpc.hip")).read()
    assert '#include "reasons_ticks.inc"' in src


def test_argument_errors_without_gpu(pkg):
    """The header's -22 list: from the host, before any device call (there is no device here and no context to launch on)."""
    lib = pkg._cabi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                 # a non-null address; no refused call reads it
    names = ("rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "veh_of", "par", "threshold", "carry", "val", "timers", "trig", "first")

    def call(B=1, n=1, ctx=None, **over):
        a = {k: p for k in names}
        a["n_obs"] = 1
        a.update(over)
        rc = lib.jsim_loop_eval_reasons(ctx, B, n, *[a[k] for k in names], None)
        return rc, lib.jsim_last_error(None).decode()

    who = "jsim_loop_eval_reasons: "
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n=-1), "n_ticks=-1"), (dict(n_obs=0), "obs_rec given with n_obs=0"),
                    (dict(n_obs=-3), "obs_rec given with n_obs=-3")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in names:
        if k in ("n_obs", "obs_rec"):
            continue
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null device pointer", (k, rc, err)
        rc, err = call(n=0, **{k: None})                                  # also with nothing to do
        assert rc == -22, k
    rc, err = call()                                                      # every argument good: the missing context is what is left
    assert rc == -22 and err == who + "null ctx"
    rc, err = call(obs_rec=None, n_obs=0)                                 # no vehicles recorded is not an error of its own
    assert rc == -22 and err == who + "null ctx"
    assert not buf.any()
