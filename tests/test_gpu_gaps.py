"""The time gap per recorded tick on the device (jsim_loop_eval_gaps, Recorder.gaps): all fixture cases as one
launch at windows 0, 1, 20, 62 and 63, under both rules, at each of the nine tick counts, against the restatement and the
reference-made fixture; the exact equivalence with the merged kernel (0 <= gap <= w exactly when Recorder.conflicts has a contact at
frame_window w); a ScenarioLoop with four traffic sets and an InteractingLoop with groups of 1, 3 and 4 against the restatement on
the recorder's own arrays; the refusals that need a context; and, in every launch, output buffers poisoned first with a row of
guard slots on either side.  Every output is an integer: every comparison is exact."""
import numpy as np
import pytest
import torch

import conflict_cases as TC
import gap_cases as GC
import gaps_numpy as GN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine  # noqa: F401
from recorder_checks import GAPS_ALL as ALL, gaps_assert_same as assert_same, gaps_check_recorder as check_recorder  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = ("off", "ep_gap", "ep_tick", "ep_who", "ep_off")
POISON = {"off": 85, "ep_gap": -85, "ep_tick": -85, "ep_who": -85, "ep_off": -85}   # values no output can take
SPEC = [(k, np.int8, (8,), POISON[k]) if k == "off" else (k, np.int32, (), POISON[k]) for k in KEYS]


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return GC.recorder_arrays(GC.cases())


def device_inputs(eng, A, n):
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    m = max(n, 1)
    return [up(A["rec"][:m]), up(A["flags"][:m], np.int32), up(A["obs"][:m]), up(A["x_first"]), up(A["x_spawn"]), up(A["veh_range"], np.int32),
            up(A["mate_range"], np.int32)]


def launch(pkg, eng, A, window, within, n=GC.N, rc_want=0, **over):
    """jsim_loop_eval_gaps on the first n ticks of recorder arrays, on guarded outputs (gpu_helpers.guarded_outputs).  Returns numpy
    outputs with gap and who derived as Recorder.gaps derives them."""
    B = A["rec"].shape[1]
    rec, flags, obs, xf, xs, veh, mate = device_inputs(eng, A, n)
    shapes, ego = np.ascontiguousarray(A["shapes"]), np.array(GC.CAR)
    views, buf = guarded_outputs(SPEC, n, B, eng.device)
    p = lambda t: t.data_ptr()
    args = dict(B=B, n=n, n_obs=A["obs"].shape[1], window=window, within=GN.WITHIN.get(within, within), **{k: p(v) for k, v in views.items()})
    args.update(over)
    rc = eng.lib.jsim_loop_eval_gaps(eng._ctx, args["B"], args["n"], p(rec), p(flags), args["n_obs"], p(obs), p(xf), p(xs), p(veh), p(mate),
                                     shapes.ctypes.data, ego.ctypes.data, args["window"], args["within"], *[args[k] for k in KEYS], None)
    out = check_guarded(pkg, eng, "jsim_loop_eval_gaps", SPEC, buf, n, rc, rc_want, nothing=args["n"] == 0 or args["B"] == 0, what=(window, within))
    if isinstance(out, str):                                           # refused, or nothing to do: the library's message
        return out
    out["gap"], out["who"] = pkg.history.gap_per_tick(out["off"])
    return out


@pytest.mark.parametrize("rule", GC.RULES)
def test_all_cases_in_one_launch(pkg, eng, arrays, rule):
    g = GC.fixture()
    ref_made = ~g["restated"]
    touching = 0
    for n in GC.TICK_COUNTS:
        made, least = GC.expected(g, n)
        for w in GC.WINDOWS:
            out = launch(pkg, eng, arrays, w, rule, n=n)
            assert_same(out, GC.restate(arrays, w, rule, n=n), (rule, w, n))
            assert np.all(out["ep_gap"][~made] == -1) and np.all(out["ep_off"][~made] == GN.NONE)
            if rule == "episode":                                      # the least frame_window at which the reference's own function hits
                m = made & ref_made[None, :]
                assert np.array_equal(out["ep_gap"][m], np.where(least <= w, least, -1)[m]), (w, n)
            touching += int((out["gap"] >= 0).sum())
    print(f"jsim_loop_eval_gaps, rule {rule}: {len(GC.cases())} cases x {GC.TICK_COUNTS} ticks x windows {GC.WINDOWS}, {touching} (ego, tick) with a gap")
    assert touching > 10000


def conflicts_contact(pkg, eng, A, w, n):
    """The merged kernel's `row >= 0` on the same buffers."""
    B = A["rec"].shape[1]
    rec, flags, obs, xf, xs, veh, mate = device_inputs(eng, A, n)
    shapes, ego = np.ascontiguousarray(A["shapes"]), np.array(GC.CAR)
    f64 = [torch.empty(n, B, dtype=torch.float64, device=eng.device), torch.empty(n, B, 2, dtype=torch.float64, device=eng.device)]
    i32 = [torch.empty(n, B, dtype=torch.int32, device=eng.device) for _ in range(4)]
    p = lambda t: t.data_ptr()
    rc = eng.lib.jsim_loop_eval_conflicts(eng._ctx, B, n, p(rec), p(flags), A["obs"].shape[1], p(obs), p(xf), p(xs), p(veh), p(mate),
                                          shapes.ctypes.data, ego.ctypes.data, w, p(f64[0]), *[p(t) for t in i32], p(f64[1]), None)
    pkg._cabi.check(rc, eng._ctx, "jsim_loop_eval_conflicts")
    torch.cuda.synchronize()
    return i32[1].cpu().numpy() >= 0


@pytest.mark.parametrize("which", ("gaps", "conflicts"))
def test_a_gap_within_w_is_the_merged_kernels_contact(pkg, eng, arrays, which):
    """On the same buffers -- these cases and tests/conflict_cases.py's -- 0 <= gap <= w equals jsim_loop_eval_conflicts' contact at
    frame_window w, tick for tick: from one launch at window 20, and from a launch at window w itself."""
    A = arrays if which == "gaps" else TC.recorder_arrays(TC.cases())
    some = 0
    for n in (GC.N, 129, 64):
        wide = launch(pkg, eng, A, 20, "episode", n=n)
        for w in (0, 1, 3, 20):
            contact = conflicts_contact(pkg, eng, A, w, n)
            assert np.array_equal((wide["gap"] >= 0) & (wide["gap"] <= w), contact), (which, n, w)
            assert np.array_equal(launch(pkg, eng, A, w, "episode", n=n)["gap"] >= 0, contact), (which, n, w)
            some += int(contact.sum())
    assert some > 1000


# ---- live recorders ----
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
T = 13


def test_scenario_loop_with_traffic_sets(pkg, W, iroutes):
    B, n = 6, 140
    sets = [[dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(direction=-1, turning=True, speed=25 / 3.6, offset=None)],
            [dict(kind="roundabout", direction=1, turning=True, speed=20 / 3.6, offset=1.0)],
            [dict(kind="arterial", x_init=1.5, y_init=-30.0, speed=25 / 3.6, initial_speed=5 / 3.6, offset=3.0),
             dict(kind="arterial", x_init=2.0, y_init=-12.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)],
            []]
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T)
    loop = pkg.ScenarioLoop(eng, x0, sets, max_age=20, frame_window=20, traffic_of=np.array([0, 1, 2, 3, 0, 2]), record=n)
    loop.run(n)
    r = loop.recorder
    found = check_recorder(pkg, r, n, "ScenarioLoop, 6 egos, four traffic sets, 140 ticks")
    res = r.gaps(window=63)
    assert res["veh_range"].tolist() == [[0, 2], [2, 3], [3, 5], [5, 5], [0, 2], [3, 5]] and not res["mate_range"].any()
    assert (res["off"][:, 3] == GN.NONE).all() and (res["gap"][:, 3] == -1).all() and (res["ep_gap"][:, 3] == -1).all()   # the empty set
    assert (res["off"][:, :, 2:] == GN.NONE).all() and any(v >= 0 for v in found["record", 63])
    for kw in (dict(window=64), dict(window=-1), dict(window=1.5), dict(within="run"), dict(within=0), dict(shapes=np.ones((2, 4))),
               dict(mates=np.array([[0, 7]] * B)), dict(mates=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            r.gaps(**kw)


def test_interacting_loop_with_groups_of_1_3_and_4(pkg, W, iroutes):
    n = 40
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 8, T, rank=2), T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[1, 3, 4], hist_cap=n, max_age=30, frame_window=20, record=n)
    il.run(n)
    check_recorder(pkg, il.recorder, n, "InteractingLoop, groups of 1, 3 and 4, 40 ticks")
    res = il.recorder.gaps(window=63, within="record")
    assert res["mate_range"].tolist() == [[0, 1]] + [[1, 4]] * 3 + [[4, 8]] * 4 and not res["veh_range"].any()
    assert (res["off"][:, 0] == GN.NONE).all() and (res["off"][:, 1:4, 2:] == GN.NONE).all() and (res["off"][:, 4:, 3:] == GN.NONE).all()


def test_a_loop_without_vehicles_has_no_gaps(pkg, W, iroutes):
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, T, rank=1), T)
    loop = pkg.ClosedLoop(eng, x0, hist_cap=4, max_age=40, record=4)
    loop.run(2)
    res = loop.recorder.gaps()
    assert res["off"].shape == (2, 3, 8) and (res["off"] == GN.NONE).all() and (res["ep_off"] == GN.NONE).all() and res["window"] == 20
    assert all(np.all(res[k] == -1) for k in ("gap", "who", "ep_gap", "ep_tick", "ep_who"))


def test_refusals_with_a_context(pkg, eng, arrays):
    who = "jsim_loop_eval_gaps: "
    for kw, msg in ((dict(window=64), "window=64 outside [0, 63]"), (dict(window=-1), "window=-1"), (dict(within=2), "within=2"),
                    (dict(off=None), "null output off"), (dict(ep_gap=None), "null output ep_gap"), (dict(ep_tick=None), "null output ep_tick"),
                    (dict(ep_who=None), "null output ep_who"), (dict(ep_off=None), "null output ep_off"), (dict(B=-1), "B=-1"),
                    (dict(n_obs=-1), "n_obs=-1")):
        err = launch(pkg, eng, arrays, kw.pop("window", 20), kw.pop("within", 0), rc_want=-22, **kw)
        assert err.startswith(who) and msg in err, (kw, err)
    # nothing to do: returns 0 and writes nothing
    launch(pkg, eng, arrays, 63, 1, n=0)
    launch(pkg, eng, arrays, 63, 0, B=0)
