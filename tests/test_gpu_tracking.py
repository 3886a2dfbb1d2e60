"""Every recorded pose projected onto a path on the device (jsim_loop_eval_tracking, Recorder.tracking): all
cases as one launch at each of the ten tick counts against the restatement; a launch cut to n ticks against the long launch;
sub-batches in reverse order and one launch per ego against one launch; a ScenarioLoop, a fork of it and an InteractingLoop
against the restatement on the recorder's own arrays; the refusals that need a context; and, in every launch, output buffers
poisoned first with a row of guard slots on either side.

Bars: idx, seg and ep_i exact; s, d, e_yaw, the episode maxima, s_first, s_last and the mean of d * d (against math.fsum) within
1e-12 * max(1, |value|), DESIGN.md section 19's bar.  The values are at most a dozen correctly rounded operations from inputs
below 1e3, the same operations in the same order on both sides."""
import numpy as np
import pytest
import torch

import tracking_cases as KC
import tracking_numpy as TN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine  # noqa: F401
from recorder_checks import TRACKING_INTS as INTS, tracking_check_recorder as check_recorder, tracking_errors as errors

pytestmark = pytest.mark.gpu
KEYS = ("idx", "seg", "s", "d", "e_yaw", "ep_i", "ep_d")
WIDTH = {"ep_i": TN.NI, "ep_d": TN.ND}
POISON_I, POISON_D = -85, -8.5e85                                      # values no output can take
SPEC = [(k, np.int32 if k in INTS else np.float64, (WIDTH[k],) if k in WIDTH else (), POISON_I if k in INTS else POISON_D) for k in KEYS]


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch or its paths."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return KC.recorder_arrays(KC.cases())


@pytest.fixture(scope="module")
def restated(arrays):
    """The restatement of every tick count, made once."""
    return {n: KC.restate(arrays, n=n) for n in KC.TICK_COUNTS}


def launch(pkg, eng, A, n=KC.N, egos=None, rc_want=0, **over):
    """jsim_loop_eval_tracking on the first n ticks of recorder arrays (egos: a subset, in that order), on guarded outputs
    (gpu_helpers.guarded_outputs).  Returns numpy outputs."""
    e = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    B, dev = len(e), eng.device
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    m = max(n, 1)
    t = pkg.history.path_table(A["paths"])
    rec, flags, pid = up(A["rec"][:m, e]), up(A["flags"][:m, e], np.int32), up(A["path_id"][e], np.int32)
    tab = {"px": up(t["x"]), "py": up(t["y"]), "pyaw": up(t["yaw"]), "path_off": up(t["off"], np.int64), "arc": up(t["arc_flat"])}
    views, buf = guarded_outputs(SPEC, n, B, dev)
    p = lambda x: None if x is None else x.data_ptr()
    a = dict(B=B, n=n, rec=rec, flags=flags, path_id=pid, n_pts=len(t["x"]), n_paths=len(A["paths"]), **tab, **views)
    a.update(over)
    rc = eng.lib.jsim_loop_eval_tracking(eng._ctx, a["B"], a["n"], p(a["rec"]), p(a["flags"]), p(a["path_id"]), a["n_pts"], p(a["px"]), p(a["py"]),
                                         p(a["pyaw"]), a["n_paths"], p(a["path_off"]), p(a["arc"]), *[p(a[k]) for k in KEYS], None)
    return check_guarded(pkg, eng, "jsim_loop_eval_tracking", SPEC, buf, n, rc, rc_want, nothing=a["n"] == 0 or a["B"] == 0)


def same_bits(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def test_all_cases_in_one_launch(pkg, eng, arrays, restated):
    worst = {}
    for n in KC.TICK_COUNTS:
        if n == 0:
            launch(pkg, eng, arrays, n=0)                              # returns 0 and writes nothing
            continue
        for k, v in errors(launch(pkg, eng, arrays, n=n), restated[n], f"{n} ticks").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"jsim_loop_eval_tracking: {len(KC.cases())} cases x {KC.TICK_COUNTS} ticks, largest relative error over all {worst}")
    g = KC.fixture()                                                   # and the reference's own index, directly
    assert np.array_equal(launch(pkg, eng, arrays)["idx"], g["idx"].T)


def test_a_cut_launch_leaves_finished_episodes_as_they_are(pkg, eng, arrays):
    """The per-tick outputs of a launch cut to n ticks are the long launch's; so is the row of every episode that ended before the
    cut, bit for bit; the cut closes the running one."""
    whole = launch(pkg, eng, arrays)
    for n in KC.TICK_COUNTS[1:-1]:
        cut = launch(pkg, eng, arrays, n=n)
        for k in ("idx", "seg", "s", "d", "e_yaw"):
            assert cut[k].tobytes() == whole[k][:n].tobytes(), (n, k)
        checked = 0
        for b in range(arrays["flags"].shape[1]):
            eps = TN.episodes_of(arrays["flags"][:n, b])
            starts = np.zeros(n, dtype=bool)
            starts[[k0 for k0, _ in eps]] = True
            assert (cut["ep_i"][~starts, b] == -1).all() and np.isnan(cut["ep_d"][~starts, b]).all()
            for k0, k1 in eps:
                assert cut["ep_i"][k0, b, 0] == k1 - k0 + 1
                if arrays["flags"][k1, b] & (TN.GOAL | TN.AGE):
                    assert cut["ep_i"][k0, b].tobytes() == whole["ep_i"][k0, b].tobytes() and cut["ep_d"][k0, b].tobytes() == whole["ep_d"][k0, b].tobytes(), (n, b, k0)
                    checked += 1
        assert checked >= min(n, 3)


def test_sub_batches_and_single_egos_are_bit_identical(pkg, eng, arrays):
    """One launch of 65 egos (the cases, repeated) against launches of its egos in reverse order in sub-batches of 65, 3 and 1, and
    the ten cases one launch per ego against their one launch."""
    n_cases = arrays["rec"].shape[1]
    egos = np.arange(65) % n_cases
    for n in (KC.N, 65):
        one = launch(pkg, eng, arrays, n=n, egos=egos)
        for size in (65, 3, 1):
            for lo in range(0, 65, size * (1 if size > 1 else 13)):    # (single egos: every 13th)
                rows = np.arange(lo, min(lo + size, 65))[::-1]
                part = launch(pkg, eng, arrays, n=n, egos=egos[rows])
                same_bits(part, {k: one[k][:, rows] for k in KEYS}, (n, size, lo))
    whole = launch(pkg, eng, arrays)
    for b in range(n_cases):
        same_bits(launch(pkg, eng, arrays, egos=[b]), {k: whole[k][:, [b]] for k in KEYS}, b)


# ---- live recorders ----
T = 13


def shifted(route, d):
    """A route moved d metres to the left of its own heading."""
    out = route.copy()
    out[:, 0] -= d * np.sin(route[:, 2])
    out[:, 1] += d * np.cos(route[:, 2])
    return out


def test_scenario_loop_and_its_fork(pkg, W, iroutes):
    B, n, m, at = 3, 70, 40, 20
    batch = W.ego_batch(iroutes, B, T, rank=2)
    src = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T), W.OBSTACLE_SPECS, max_age=25, record=n)
    src.run(n)
    res = check_recorder(pkg, src.recorder, n, "ScenarioLoop, 3 egos, 70 ticks")
    assert (res["ep_i"][0, :, 0] >= 1).all() and (res["ep_i"][0, :, 0] <= 26).all()    # max_age 25 ends the first episode
    assert src.recorder._tracking_table is not None
    same_bits(src.recorder.tracking(), res, "the kept table")
    # the same loop tick by tick: the same records, the same projection, bit for bit
    ticked = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T), W.OBSTACLE_SPECS, max_age=25, record=n)
    for _ in range(n):
        ticked.tick()
    same_bits(ticked.recorder.tracking(), res, "70 x tick()")
    # a fork onto routes 0.4 m to the left: against the source's routes it strays by about that much, against its own it does not
    eng = src.loop.eng
    pid = eng.path_id.cpu().numpy()
    fork = src.fork(np.arange(B), at, paths=[shifted(eng.paths[p], 0.4) for p in pid], path_id=np.arange(B), record=m)
    fork.run(m)
    on_source = check_recorder(pkg, fork.recorder, m, "the fork against the source's routes", paths=eng.paths, path_id=pid)
    on_own = check_recorder(pkg, fork.recorder, m, "the fork against its own routes")
    assert not np.array_equal(on_source["d"], on_own["d"]) and abs(float(np.median(on_source["d"] - on_own["d"])) - 0.4) < 0.05
    same_bits(src.recorder.tracking(), res, "the source after the fork")       # the context's tables are not read
    for kw in (dict(path_id=[0, 1]), dict(path_id=len(eng.paths)), dict(paths=eng.paths), dict(paths=[np.zeros((0, 3))], path_id=0)):
        with pytest.raises(ValueError):
            src.recorder.tracking(**kw)


def test_interacting_loop_of_two_egos(pkg, W, iroutes):
    n = 40
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 2, T, rank=2), T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[2], hist_cap=n, max_age=30, frame_window=20, record=n)
    il.run(n)
    res = check_recorder(pkg, il.recorder, n, "InteractingLoop, one group of 2, 40 ticks")
    one = check_recorder(pkg, il.recorder, n, "both egos against ego 0's route", paths=[eng.paths[int(eng.path_id[0])]])
    assert np.array_equal(one["d"][:, 0], res["d"][:, 0]) and not one["path_id"].any()


def test_a_closed_loop_without_glue(pkg, W, iroutes):
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, T, rank=1), T)
    loop = pkg.ClosedLoop(eng, x0, hist_cap=4, max_age=40, record=4)
    loop.run(2)
    res = check_recorder(pkg, loop.recorder, 2, "ClosedLoop, 2 ticks")
    assert res["ep_i"][0, :, 0].tolist() == [2, 2, 2] and (res["ep_i"][1] == -1).all()


def test_refusals_with_a_context(pkg, eng, arrays):
    who = "jsim_loop_eval_tracking: "
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_pts=-1), "n_pts=-1"), (dict(n_paths=-1), "n_paths=-1"), (dict(n_paths=0), "n_paths=0 with B=10"),
                    *[({k: None}, "null pointer " + k) for k in ("rec", "flags", "path_id", "px", "py", "pyaw", "path_off", "arc", *KEYS)]):
        err = launch(pkg, eng, arrays, rc_want=-22, **kw)
        assert err.startswith(who) and msg in err, (kw, err)
    # nothing to do: returns 0 and writes nothing
    launch(pkg, eng, arrays, n=0)
    launch(pkg, eng, arrays, B=0)
    # a path_id outside the table and a path_off beyond it: clamped, nothing is read outside and nothing but -1 / NaN comes out
    A = dict(arrays, path_id=np.array([8, -1] + [0] * 8, dtype=np.int32))
    out = launch(pkg, eng, A, n=65)
    assert (out["idx"][:, :2] == -1).all() and (out["seg"][:, :2] == -1).all() and np.isnan(out["d"][:, :2]).all() and np.isnan(out["ep_d"][:, :2]).all()
    assert (out["ep_i"][0, :2] == [65, -1]).all() and (out["idx"][:, 2:] == 0).all()
    few = launch(pkg, eng, arrays, n=65, n_pts=4)                      # the table ends after path 2's first point
    ref = KC.restate(arrays, n=65)
    assert np.array_equal(few["idx"][:, :2], ref["idx"][:, :2]) and (few["idx"][:, 2] == 0).all() and (few["idx"][:, 3:] == -1).all()
