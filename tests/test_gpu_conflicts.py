"""Clearance and first contact per recorded tick on the device (jsim_loop_eval_conflicts, Recorder.conflicts, DESIGN.md section
17): all fixture cases as one launch against the reference-made fixture at each of the nine tick counts and each window; the prefix
property at w = 0; the batch layout (one ego per launch, the order reversed, B = 1, 3, 65); two egos that are each other's only
vehicle; a ScenarioLoop with a cyclist and an InteractingLoop against the restatement on the recorder's own arrays; the empty call.

Bars: row, who, hit_tick, hit_frame exact, hit_xy exact (a copy of a recorded pose); clear within 1e-12 x max(1, |clear|) --
coordinates below 100 m (ulp 1.4e-14) behind one sincos, two unfused sums and one sqrt, more than an order of magnitude of headroom."""
import numpy as np
import pytest
import torch

import conflict_cases as TC
import conflicts_numpy as CN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine  # noqa: F401
from recorder_checks import conflicts_equal_restatement as assert_equals_restatement, conflicts_restate_recorder as _restate_recorder

pytestmark = pytest.mark.gpu
KEYS = ("clear", "who", "row", "hit_tick", "hit_frame", "hit_xy")
POISON_I, POISON_D = -85, -8.5e85                                      # values no output can take
SPEC = [(k, np.float64, (2,) if k == "hit_xy" else (), POISON_D) if k in ("clear", "hit_xy") else (k, np.int32, (), POISON_I) for k in KEYS]


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return TC.recorder_arrays(TC.cases())


def launch(pkg, eng, A, w, n=TC.N, egos=None, mates=None):
    """jsim_loop_eval_conflicts on the first n ticks of recorder arrays (egos: these egos only, in this order, with these mate
    ranges; the vehicle table stays whole), on guarded outputs (gpu_helpers.guarded_outputs).  Returns numpy outputs."""
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    B = len(idx)
    dev = eng.device
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    m = max(n, 1)
    rec, flags, obs = up(A["rec"][:m, idx]), up(A["flags"][:m, idx], np.int32), up(A["obs"][:m])
    xf, xs = up(A["x_first"][idx]), up(A["x_spawn"][idx])
    veh, mate = up(A["veh_range"][idx], np.int32), up(A["mate_range"][idx] if mates is None else mates, np.int32)
    shapes, ego = np.ascontiguousarray(A["shapes"]), np.array(TC.CAR)
    out, buf = guarded_outputs(SPEC, n, B, dev)
    p = lambda t: t.data_ptr()
    rc = eng.lib.jsim_loop_eval_conflicts(eng._ctx, B, n, p(rec), p(flags), A["obs"].shape[1], p(obs), p(xf), p(xs), p(veh), p(mate),
                                          shapes.ctypes.data, ego.ctypes.data, w, *[p(out[k]) for k in KEYS], None)
    return check_guarded(pkg, eng, "jsim_loop_eval_conflicts", SPEC, buf, n, rc, nothing=n == 0)


@pytest.fixture(scope="module")
def whole(pkg, eng, arrays):
    return {w: launch(pkg, eng, arrays, w) for w in TC.WINDOWS}


def test_all_cases_in_one_launch(pkg, eng, arrays, whole):
    g = TC.fixture()
    worst = 0.0
    for w in TC.WINDOWS:
        for n in TC.TICK_COUNTS:
            out = whole[w] if n == TC.N else launch(pkg, eng, arrays, w, n=n)
            made, hit, tick, frame, xy = TC.expected(g, w, n)
            assert np.array_equal(out["hit_tick"] >= 0, hit) and np.array_equal(out["hit_frame"], frame), (w, n)
            assert np.array_equal(out["hit_xy"], xy, equal_nan=True), (w, n)
            have = tick != -2                                          # w = 0, and the restatement-made cases at every w
            assert np.array_equal(out["hit_tick"][have], tick[have]), (w, n)
            assert np.all(out["hit_tick"][~made] == -1)
            # clear, who, row and the hit_tick of w > 0 have no reference function behind them: the restatement, which the CPU suite
            # pins to the reference by what these produce (None / not None, hit_frame, hit_xy, the prefix hit_tick)
            worst = max(worst, assert_equals_restatement(out, TC.restate(arrays, w, n=n), f"w = {w}, {n} ticks"))
            if w == 0 and n != TC.N:                                   # a shorter launch is a prefix of the long one
                for k in ("clear", "who", "row"):
                    assert np.array_equal(out[k], whole[0][k][:n], equal_nan=True), (n, k)
    print(f"jsim_loop_eval_conflicts against the fixture, {len(TC.cases())} cases x {TC.TICK_COUNTS} ticks x w = {TC.WINDOWS}: "
          f"clear maximum error {worst:.3g}")
    none = whole[3]
    assert np.isnan(none["clear"][:, 18]).all() and np.all(none["who"][:, 18] == -1) and np.all(none["row"][:, 18] == -1)      # no vehicles


def test_batch_layout_is_immaterial(pkg, eng, arrays, whole):
    """The egos without mates (a mate range names batch indices, so a group only moves as a whole: the last launch)."""
    solo = np.flatnonzero(arrays["mate_range"][:, 0] == arrays["mate_range"][:, 1])
    none = np.zeros((1, 2), dtype=np.int32)
    w = 3
    for b in solo:
        one = launch(pkg, eng, arrays, w, egos=[b], mates=none)
        for k in KEYS:
            assert np.array_equal(one[k], whole[w][k][:, b:b + 1], equal_nan=True), (b, k)
    rev = launch(pkg, eng, arrays, w, egos=solo[::-1], mates=np.zeros((len(solo), 2), dtype=np.int32))
    for k in KEYS:
        assert np.array_equal(rev[k], whole[w][k][:, solo[::-1]], equal_nan=True), k
    for n_egos in (1, 3, 65):
        egos = solo[np.arange(n_egos) * 7 % len(solo)]
        out = launch(pkg, eng, arrays, w, egos=egos, mates=np.zeros((n_egos, 2), dtype=np.int32))
        for k in KEYS:
            assert np.array_equal(out[k], whole[w][k][:, egos], equal_nan=True), (n_egos, k)
    # the groups, moved to the front of a batch as they are
    grouped = np.flatnonzero(arrays["mate_range"][:, 0] != arrays["mate_range"][:, 1])
    out = launch(pkg, eng, arrays, w, egos=grouped, mates=arrays["mate_range"][grouped] - grouped[0])
    for k in KEYS:
        assert np.array_equal(out[k], whole[w][k][:, grouped], equal_nan=True), k


def test_mates_see_each_other_alike(whole):
    out = whole[0]
    assert np.array_equal(out["clear"][:, 23], out["clear"][:, 24]) and np.isfinite(out["clear"][:, 23]).all()
    assert np.array_equal(out["row"][:, 23] >= 0, out["row"][:, 24] >= 0) and (out["row"][:, 23] >= 0).any()


def test_nothing_to_do_writes_nothing(pkg, eng, arrays):
    launch(pkg, eng, arrays, 3, n=0)                                   # (check_guarded: returns 0, every slot is still poison)


# ---- loops ----
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


def test_scenario_loop_with_a_cyclist(pkg, W, iroutes):
    run = _loop(pkg, W, iroutes)
    run.run(K)
    res = run.recorder.conflicts()
    assert res["clear"].shape == (K, B) and res["hit_xy"].shape == (K, B, 2) and res["frame_window"] == 0
    assert res["veh_range"].tolist() == [[0, 1]] * 3 and not res["mate_range"].any() and np.isfinite(res["clear"]).all()
    assert res["ego_shape"] == TC.CAR and np.array_equal(run.loop.eng.vehicle_shapes[0, :3], TC.BIKE)
    assert np.array_equal(res["contact"], res["row"] >= 0)
    assert_equals_restatement(res, _restate_recorder(run.recorder, res), "ScenarioLoop, run(70), w = 0")
    res3 = run.recorder.conflicts(frame_window=3)
    assert_equals_restatement(res3, _restate_recorder(run.recorder, res3), "ScenarioLoop, run(70), w = 3")
    eps = pkg.history.conflict_episodes(res, run.recorder.flags.cpu().numpy())
    assert [len(e) for e in eps] == run.recorder.episodes()["count"].tolist()
    print(f"min clearance per ego {[min(e['min_clear'] for e in ep if e['min_clear'] == e['min_clear']) for ep in eps]}, "
          f"contacts {[sum(e['contact'] for e in ep) for ep in eps]}")
    assert res["clear"].min() < 8.0                                 # the cyclist is met, not only recorded

    ticks = _loop(pkg, W, iroutes)
    for _ in range(K):
        ticks.tick()
    res_t = ticks.recorder.conflicts()
    for k in KEYS:
        assert np.array_equal(res[k], res_t[k], equal_nan=True), ("70 x tick()", k)

    lay = _loop(pkg, W, iroutes, traffic=True)                      # a traffic layout: ego 2's set is empty
    lay.run(K)
    res_l = lay.recorder.conflicts()
    assert res_l["veh_range"].tolist() == [[0, 1], [0, 1], [1, 1]]
    assert_equals_restatement(res_l, _restate_recorder(lay.recorder, res_l), "traffic layout")
    for k in KEYS:
        assert np.array_equal(res_l[k][:, :2], res[k][:, :2], equal_nan=True), k
    assert np.isnan(res_l["clear"][:, 2]).all() and np.isnan(res_l["hit_xy"][:, 2]).all() and not res_l["contact"][:, 2].any()
    assert all(np.all(res_l[k][:, 2] == -1) for k in ("who", "row", "hit_tick", "hit_frame"))
    for kw in (dict(frame_window=21), dict(frame_window=-1), dict(frame_window=1.5), dict(shapes=np.ones((2, 4))),
               dict(mates=np.array([[0, 4]] * 3)), dict(mates=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            run.recorder.conflicts(**kw)


def test_interacting_loop_with_default_mates(pkg, W, iroutes):
    batch = W.ego_batch(iroutes, 2, T, rank=2)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[2], hist_cap=40, max_age=30, frame_window=20, record=40)
    il.run(40)
    res = il.recorder.conflicts(frame_window=1)
    assert res["mate_range"].tolist() == [[0, 2], [0, 2]] and res["veh_range"].tolist() == [[0, 0], [0, 0]]
    assert np.isfinite(res["clear"]).all() and np.all(res["who"] == 0)
    assert_equals_restatement(res, _restate_recorder(il.recorder, res), "InteractingLoop, two egos, 40 ticks")
    assert np.array_equal(il.recorder.conflicts()["clear"][:, 0], il.recorder.conflicts()["clear"][:, 1])


def test_a_loop_without_vehicles_has_no_conflicts(pkg, W, iroutes):
    batch = W.ego_batch(iroutes, B, T, rank=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    loop = pkg.ClosedLoop(eng, x0, hist_cap=4, max_age=40, record=4)
    loop.run(2)
    res = loop.recorder.conflicts(frame_window=3)
    assert res["clear"].shape == (2, B) and np.isnan(res["clear"]).all() and np.isnan(res["hit_xy"]).all() and not res["contact"].any()
    assert all(np.all(res[k] == -1) for k in ("who", "row", "hit_tick", "hit_frame"))
