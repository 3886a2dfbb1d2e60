"""Every recorded vehicle projected onto the ego's path on the device (jsim_loop_eval_headway, Recorder.headway, DESIGN.md section
25): all cases as one launch against the restatement and against the reference-made fixture; a launch cut to each tick count against
the long launch; sub-batches in reverse order and one launch per ego against one launch; the launch without the per-place outputs;
two mates that see each other antisymmetrically; a ScenarioLoop, a fork of it and an InteractingLoop against the restatement on the
recorder's own arrays; the refusals that need a context; and, in every launch, output buffers poisoned first with a row of guard
slots on either side.

Bars: lead, ttc_who and ep_i exact; inf and NaN exactly where the restatement has them; every double within BARS of the
restatement, relative to max(1, |value|) -- ttc, thw and the episode columns made of them relative to the value itself.  The bars
are four times the largest error seen on the first run on an MI355X (15 cases x 200 ticks and the live recorders of this file),
none above 1e-12; the largest errors seen (DESIGN.md section 25 has them too):
    gap 7.11e-15, lat 3.67e-15, rate 1.59e-15, lead_gap 5.11e-15, thw 2.47e-16, ttc 1.01e-15, u_ego 2.22e-16,
    ep_d: gap_min 0, thw_min 0, ttc_min 0 (each is one tick's value, and those ticks' values were exact), thw_mean 2.39e-16
(the device's sincos and cos against libm's: a last bit in a circle centre or a speed along the path, carried through a dozen
correctly rounded operations that are the same on both sides).  Against the fixture's reference-made centres and indices: gap 0,
lat 1.89e-15, held to the same bars."""
import numpy as np
import pytest
import torch

import headway_cases as HC
import headway_numpy as HN
from gpu_helpers import W, check_guarded, guarded_outputs, iroutes, loop_engine  # noqa: F401
from recorder_checks import HEADWAY_BARS as BARS, HEADWAY_INTS as INTS, HEADWAY_KEYS as KEYS, HEADWAY_PLACES as PLACES, HEADWAY_TICKS as TICKS
from recorder_checks import headway_check_recorder as check_recorder, headway_errors as errors, headway_same_bits as same_bits

pytestmark = pytest.mark.gpu
WIDTH = {"ep_i": HN.NI, "ep_d": HN.ND, "gap": 8, "lat": 8, "rate": 8}
POISON_I, POISON_D = -85, -8.5e85                                      # values no output can take
SPEC = [(k, np.int32 if k in INTS else np.float64, (WIDTH[k],) if k in WIDTH else (), POISON_I if k in INTS else POISON_D) for k in KEYS]
FREE = [b for b, c in enumerate(HC.cases()) if c["group"] is None]      # the cases that are nobody's mate: any sub-batch of them stands alone


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch or its paths."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return HC.recorder_arrays(HC.cases())


@pytest.fixture(scope="module")
def restated(arrays):
    return HC.restate(arrays)


@pytest.fixture(scope="module")
def whole(pkg, eng, arrays):
    """The launch of every case over all ticks, made once."""
    return launch(pkg, eng, arrays)


def launch(pkg, eng, A, n=HC.N, egos=None, rc_want=0, places=True, margin=HC.LAUNCH_MARGIN, **over):
    """jsim_loop_eval_headway on the first n ticks of recorder arrays (egos: a subset of the cases that are nobody's mate, in that
    order), on guarded outputs (gpu_helpers.guarded_outputs; places=False: without the per-place ones).  Returns numpy outputs."""
    e = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    mate = A["mate_range"] if egos is None else np.zeros((len(e), 2), dtype=np.int32)
    assert egos is None or all(A["mate_range"][b, 0] == A["mate_range"][b, 1] for b in e)
    B, dev = len(e), eng.device
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    m = max(n, 1)
    t = pkg.history.path_table(A["paths"])
    spec = [s for s in SPEC if places or s[0] not in PLACES]
    dv = dict(rec=up(A["rec"][:m, e]), flags=up(A["flags"][:m, e], np.int32), obs_rec=up(A["obs"][:m]), x_first=up(A["x_first"][e]),
              x_spawn=up(A["x_spawn"][e]), veh_range=up(A["veh_range"][e], np.int32), mate_range=up(mate, np.int32),
              path_id=up(A["path_id"][e], np.int32), px=up(t["x"]), py=up(t["y"]), pyaw=up(t["yaw"]), path_off=up(t["off"], np.int64),
              arc=up(t["arc_flat"]))
    views, buf = guarded_outputs(spec, n, B, dev)
    shapes = np.ascontiguousarray(A["shapes"], dtype=np.float64)
    ego = np.array(HC.CAR, dtype=np.float64)
    a = dict(B=B, n=n, n_obs=A["obs"].shape[1], n_pts=len(t["x"]), n_paths=len(A["paths"]), margin=margin, shapes=shapes.ctypes.data,
             ego_shape=ego.ctypes.data, **dv, **views, **{k: None for k in PLACES if not places})
    a.update(over)
    p = lambda x: x.data_ptr() if isinstance(x, torch.Tensor) else x
    rc = eng.lib.jsim_loop_eval_headway(eng._ctx, a["B"], a["n"], p(a["rec"]), p(a["flags"]), a["n_obs"], p(a["obs_rec"]), p(a["x_first"]),
                                        p(a["x_spawn"]), p(a["veh_range"]), p(a["mate_range"]), a["shapes"], a["ego_shape"], p(a["path_id"]),
                                        a["n_pts"], p(a["px"]), p(a["py"]), p(a["pyaw"]), a["n_paths"], p(a["path_off"]), p(a["arc"]),
                                        a["margin"], *[p(a[k]) for k in KEYS], None)
    return check_guarded(pkg, eng, "jsim_loop_eval_headway", spec, buf, n, rc, rc_want, nothing=a["n"] == 0 or a["B"] == 0)


def test_all_cases_in_one_launch(pkg, eng, arrays, restated, whole):
    cs = HC.cases()
    errors(whole, restated, f"{len(cs)} cases x {HC.N} ticks")
    launch(pkg, eng, arrays, n=0)                                         # returns 0 and writes nothing
    # the reference-made pieces: the fixture's circle centres and nearest indices give this gap and this lat
    g, paths = HC.fixture(), HC.paths()
    assert np.array_equal(restated["idx"], np.moveaxis(g["idx"], 0, 1))
    worst, checked = {"gap": 0.0, "lat": 0.0}, 0
    for b, c in enumerate(cs):
        path, arc = paths[c["path"]], HN.TN.arc_lengths(paths[c["path"]])
        kinds = c["kinds"] if c["group"] is None else next(d for d in cs if d["group"] == c["group"])["kinds"]   # (a group's vehicles are its first ego's)
        for j, k in enumerate(range(0, HC.N, HC.CENTRE_STRIDE)):
            for i in range(8):
                cen, idx = g["centres"][b, j, [0, 1 + i]], g["idx"][b, k, [0, 1 + i]]
                if np.isnan(cen).any():
                    assert np.isnan(whole["gap"][k, b, i]) and np.isnan(whole["lat"][k, b, i])
                    continue
                r_i = HC.SHAPES[kinds[i]][2] if i < len(kinds) else HC.CAR[2]                                       # (a mate has the ego's shape)
                gap, lat = HN.gap_lat_from(cen, idx, path, arc, HC.CAR[2], r_i)
                for key, want in (("gap", gap), ("lat", lat)):
                    got = float(whole[key][k, b, i])
                    worst[key] = max(worst[key], abs(got - want) / max(1.0, abs(want)))
                checked += 1
    print(f"against the fixture's centres and indices: {checked} places, largest relative error {worst}")
    assert checked > 1000 and worst["gap"] <= BARS["gap"] and worst["lat"] <= BARS["lat"]


def test_a_cut_launch_leaves_finished_episodes_as_they_are(pkg, eng, arrays, whole):
    """The per-tick and per-place outputs of a launch cut to n ticks are the long launch's; so is the row of every episode that
    ended before the cut, bit for bit; the cut closes the running one."""
    for n in HC.TICK_COUNTS:
        if n == 0:
            launch(pkg, eng, arrays, n=0)
            continue
        cut = whole if n == HC.N else launch(pkg, eng, arrays, n=n)
        for k in ("lead", "ttc_who") + TICKS + PLACES:
            assert cut[k].tobytes() == whole[k][:n].tobytes(), (n, k)
        checked = 0
        for b in range(arrays["flags"].shape[1]):
            eps = HN.TN.episodes_of(arrays["flags"][:n, b])
            starts = np.zeros(n, dtype=bool)
            starts[[k0 for k0, _ in eps]] = True
            assert (cut["ep_i"][~starts, b] == -1).all() and np.isnan(cut["ep_d"][~starts, b]).all()
            for k0, k1 in eps:
                assert cut["ep_i"][k0, b, 0] == k1 - k0 + 1
                if arrays["flags"][k1, b] & (HC.GOAL | HC.AGE):
                    assert cut["ep_i"][k0, b].tobytes() == whole["ep_i"][k0, b].tobytes() and cut["ep_d"][k0, b].tobytes() == whole["ep_d"][k0, b].tobytes(), (n, b, k0)
                    checked += 1
        assert checked >= (0 if n < 64 else 1)


def test_sub_batches_and_single_egos_are_bit_identical(pkg, eng, arrays, whole):
    """One launch of 33 egos (the cases that are nobody's mate, repeated) against launches of its egos in reverse order in sub-batches
    of 33, 3 and 1, and those cases one launch per ego against the launch of all."""
    egos = np.array(FREE)[np.arange(33) % len(FREE)]
    for n in (HC.N, 65):
        one = launch(pkg, eng, arrays, n=n, egos=egos)
        for size in (33, 3, 1):
            for lo in range(0, 33, size * (1 if size > 1 else 8)):       # (single egos: every 8th)
                rows = np.arange(lo, min(lo + size, 33))[::-1]
                same_bits(launch(pkg, eng, arrays, n=n, egos=egos[rows]), {k: one[k][:, rows] for k in KEYS}, (n, size, lo))
    for b in FREE:
        same_bits(launch(pkg, eng, arrays, egos=[b]), {k: whole[k][:, [b]] for k in KEYS}, b)


def test_without_the_per_place_outputs(pkg, eng, arrays, whole):
    for n in (HC.N, 65):
        bare = launch(pkg, eng, arrays, n=n, places=False)
        assert not any(k in bare for k in PLACES)
        keys = [k for k in KEYS if k not in PLACES]
        cut = whole if n == HC.N else launch(pkg, eng, arrays, n=n)
        same_bits(bare, cut, n, keys=keys)


def test_two_mates_see_each_other_antisymmetrically(arrays, whole):
    """Cases 6 and 7: one path, one shape, each the other's only place.  The follower's gap to the leader is minus the leader's gap
    to the follower, so are the rates, and the lateral offsets (+0.25 and -0.25) have one size: the arithmetic is mirror-symmetric,
    so no tolerance."""
    a, b = (j for j, c in enumerate(HC.cases()) if c["group"] == "pair")
    assert arrays["mate_range"][a].tolist() == [a, b + 1] == arrays["mate_range"][b].tolist()
    assert np.isfinite(whole["gap"][:, [a, b], 0]).all() and np.isnan(whole["gap"][:, [a, b], 1:]).all()
    assert np.array_equal(whole["gap"][:, a, 0], -whole["gap"][:, b, 0]) and (whole["gap"][:, a, 0] > 0).any() and (whole["gap"][:, a, 0] == 0).any()
    assert np.array_equal(whole["rate"][:, a, 0], -whole["rate"][:, b, 0]) and (whole["rate"][:, a, 0] == -0.5).all()
    assert np.array_equal(np.abs(whole["lat"][:, a, 0]), np.abs(whole["lat"][:, b, 0])) and (whole["lat"][:, a, 0] == -0.25).all()
    assert (whole["lead"][whole["gap"][:, a, 0] > 0, b] == -1).all()      # the leader has nobody in front of it


# ---- live recorders ----
T = 13


def test_scenario_loop_its_fork_and_an_interacting_loop(pkg, W, iroutes):
    B, n, m, at = 4, 70, 40, 20
    worst = {}
    batch = W.ego_batch(iroutes, B, T, rank=2)
    src = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T), W.OBSTACLE_SPECS, max_age=25, record=n)
    src.run(n)
    r = src.recorder
    res = check_recorder(pkg, r, n, "ScenarioLoop, 4 egos, four vehicles, 70 ticks", worst)
    assert res["veh_range"].tolist() == [[0, 4]] * B and not res["mate_range"].any() and np.isnan(res["gap"][:, :, 4:]).all()
    assert np.isfinite(res["gap"][:, :, :4]).all() and np.isfinite(res["u_ego"]).all()
    check_recorder(pkg, r, n, "the same with a margin of 1.5 m", worst, margin=1.5)
    eng = src.loop.eng
    pid = eng.path_id.cpu().numpy()
    fork = src.fork(np.arange(B), at, record=m)
    fork.run(m)
    check_recorder(pkg, fork.recorder, m, "the fork projected onto the source's routes", worst, paths=eng.paths, path_id=pid)
    # the Python surface's refusals
    for kw in (dict(margin=-0.5), dict(margin=float("nan")), dict(margin=float("inf")), dict(path_id=[0, 1]), dict(path_id=len(eng.paths)),
               dict(paths=eng.paths), dict(paths=[np.zeros((0, 3))], path_id=0), dict(shapes=np.ones((2, 4))),
               dict(mates=np.array([[0, 7]] * B)), dict(mates=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            r.headway(**kw)
    e2, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, 2, T, rank=2), T)
    il = pkg.InteractingLoop(e2, x0, group_sizes=[2], hist_cap=m, max_age=30, frame_window=20, record=m)
    il.run(m)
    one = [e2.paths[int(e2.path_id[0])]]
    res = check_recorder(pkg, il.recorder, m, "InteractingLoop, one group of 2, both on ego 0's route", worst, paths=one)
    assert res["mate_range"].tolist() == [[0, 2]] * 2 and not res["veh_range"].any() and np.isnan(res["gap"][:, :, 1:]).all()
    print(f"live recorders: largest relative error over all {worst}")


def test_refusals_with_a_context(pkg, eng, arrays):
    who = "jsim_loop_eval_headway: "
    bad_shapes = np.ascontiguousarray(arrays["shapes"], dtype=np.float64).copy()
    bad_shapes[2, 2] = -1.0
    odd_shapes = bad_shapes.copy()
    odd_shapes[2, 2], odd_shapes[3, 1] = 1.0, np.inf
    flat_ego, nan_ego = np.array([1.0, 0.0, 0.0]), np.array([np.nan, 0.0, 1.0])      # (kept alive: the calls take their addresses)
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_obs=-1), "n_obs=-1"), (dict(n_pts=-1), "n_pts=-1"), (dict(n_paths=-1), "n_paths=-1"),
                    (dict(n_paths=0), "n_paths=0 with B=15"), (dict(obs_rec=None), "null obs_rec with n_obs="),
                    (dict(margin=-1.0), "margin"), (dict(margin=float("nan")), "margin"), (dict(margin=float("inf")), "margin"),
                    (dict(gap=None), "given in part"), (dict(lat=None, rate=None), "given in part"),
                    (dict(ego_shape=flat_ego.ctypes.data), "radius"), (dict(ego_shape=nan_ego.ctypes.data), "circle offset"),
                    (dict(shapes=bad_shapes.ctypes.data), "shapes row 2"), (dict(shapes=odd_shapes.ctypes.data), "shapes row 3"),
                    *[({k: None}, "null pointer " + k) for k in ("rec", "flags", "x_first", "x_spawn", "veh_range", "mate_range", "ego_shape", "path_id",
                                                                  "px", "py", "pyaw", "path_off", "arc", "lead", "lead_gap", "thw", "ttc", "ttc_who",
                                                                  "u_ego", "ep_i", "ep_d")]):
        err = launch(pkg, eng, arrays, rc_want=-22, **kw)
        assert err.startswith(who) and msg in err, (kw, err)
    launch(pkg, eng, arrays, n=0)                                         # nothing to do: returns 0 and writes nothing
    launch(pkg, eng, arrays, B=0)
    # what needs a device read to detect is clamped: nothing is read outside the tables, nothing but -1 / NaN comes out
    B = arrays["rec"].shape[1]
    A = dict(arrays, path_id=np.array([len(arrays["paths"]), -1] + [0] * (B - 2), dtype=np.int32))
    out = launch(pkg, eng, A, n=60)
    assert (out["lead"][:, :2] == -1).all() and np.isnan(out["gap"][:, :2]).all() and np.isnan(out["u_ego"][:, :2]).all()
    assert (out["ep_i"][0, :2] == [60, 0, -1, -1, -1, -1, -1]).all() and np.isnan(out["ep_d"][:, :2]).all()
    wild = dict(arrays, veh_range=np.tile(np.array([-5, 1000], dtype=np.int32), (B, 1)), mate_range=np.tile(np.array([-3, 500], dtype=np.int32), (B, 1)))
    out = launch(pkg, eng, wild, n=60)                                    # every list clamped to the first eight recorded vehicles
    assert np.isfinite(out["gap"][:, 0]).all() and (out["ep_i"][0, :, 0] == 60).all()
    few = launch(pkg, eng, arrays, n=65, n_pts=4)                         # the table ends after path 2's first point
    assert np.isnan(few["u_ego"][:, [0, 1, 2, 3, 4, 5]]).all() and np.isfinite(few["u_ego"][:, [11, 12, 13]]).all()
