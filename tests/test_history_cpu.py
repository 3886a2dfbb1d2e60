"""The host half of the History recorder (history.py, pure numpy) on synthetic record / flag arrays, and the argument checks of
jsim_loop_set_recorder that run before anything touches a device."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import PKG_NAME

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    return importlib.import_module(PKG_NAME + ".history")


def _synthetic(n, B, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, B, 7)), np.zeros((n, B), dtype=np.int32)


def test_episodes_split_at_goal_and_age(H):
    rec, fl = _synthetic(10, 3)
    fl[2, 0] = H.GOAL
    fl[6, 0] = H.AGE
    fl[9, 1] = H.GOAL | H.AGE
    fl[4, 2] = H.FAILED                     # a failed solve ends nothing
    ep = H.episodes(fl)
    assert ep["count"].tolist() == [3, 2, 1]
    assert ep["ticks"][0].tolist() == [3, 4, 3] and ep["end"][0].tolist() == [H.END_GOAL, H.END_AGE, H.END_RUNNING]
    assert ep["ticks"][1].tolist() == [10, 0] and ep["end"][1].tolist() == [H.END_GOAL, H.END_RUNNING]
    assert ep["ticks"][2].tolist() == [10] and ep["end"][2].tolist() == [H.END_RUNNING]


def test_restated_episodes_agree_with_episode_bounds(H):
    """recorder_numpy.episodes_of (the restatements' rule) and history.episode_bounds (the package's) are two texts of one rule:
    on every flag series of the four case families, cut to every tick count the families are evaluated at, they give the same
    episodes, and episode_bounds adds only the running episode without a tick."""
    import conflict_cases as TC
    import episode_cases as EC
    import reason_ticks_cases as RC
    import recorder_numpy as RN
    import static_cases as SC
    families = ((TC.recorder_arrays(TC.cases())["flags"], TC.TICK_COUNTS), (SC.recorder_arrays(SC.cases())["flags"], SC.TICK_COUNTS),
                (RC.recorder_arrays(RC.cases())["flags"], RC.TICK_COUNTS), (EC.recorder_arrays()["flags"], EC.TICK_COUNTS))
    series = ends = 0
    for flags, counts in families:
        for n in counts:
            for b in range(flags.shape[1]):
                f = flags[:n, b]
                bounds, mine = H.episode_bounds(f), RN.episodes_of(f)
                assert [(k0, k1 - 1) for k0, k1, _ in bounds if k1 > k0] == mine, (n, b)
                assert all(k1 > k0 for k0, k1, _ in bounds[:-1]) and bounds[-1][2] == H.END_RUNNING and bounds[-1][1] == n, (n, b)
                assert [e for _, _, e in bounds[:-1]] == [H.END_GOAL if f[k1] & H.GOAL else H.END_AGE for _, k1 in mine[:len(bounds) - 1]]
                assert np.array_equal(np.flatnonzero(RN.is_end(f)), [k1 - 1 for _, k1, _ in bounds[:-1]]), (n, b)
                series, ends = series + 1, ends + len(bounds) - 1
    assert series == (28 + 29 + 27) * 9 + 87 * 10 and ends > 1000       # (the families are all there, and they do end episodes)


def test_histories_spawn_entries_fields_and_time(H):
    rec, fl = _synthetic(7, 2, seed=1)
    fl[3, 1] = H.GOAL
    dt = 0.2
    x0_first = np.array([1.0, 2.0, 3.0, 0.5])      # MPC order x, y, v, yaw
    spawn = np.array([-1.0, -2.0, 0.0, 1.5])
    hs = H.ego_histories(rec[:, 1], fl[:, 1], dt, x0_first, spawn)
    assert len(hs) == 2 and [len(h) for h in hs] == [5, 4]
    h0, h1 = hs
    assert (h0.x[0], h0.y[0], h0.yaw[0], h0.v[0]) == (1.0, 2.0, 0.5, 3.0)
    assert (h1.x[0], h1.y[0], h1.yaw[0], h1.v[0]) == (-1.0, -2.0, 1.5, 0.0)
    for h in hs:
        assert h.a[0] == h.delta[0] == h.xref_deviation[0] == 0.0
    for h, rows in ((h0, rec[0:4, 1]), (h1, rec[4:7, 1])):
        for j, name in enumerate(H.FIELDS):
            assert getattr(h, name)[1:] == rows[:, j].tolist(), name
        assert all(type(v) is float for name in H.FIELDS + ("t",) for v in getattr(h, name))
    for h in hs:                            # t: repeated + dt from 0, as History.store accumulates it
        t, ref = 0.0, []
        for _ in range(len(h)):
            t = t + dt
            ref.append(t)
        assert h.t == ref


def test_open_last_episode_and_nan_deviation(H):
    rec, fl = _synthetic(5, 1, seed=2)
    rec[2, 0, 6] = np.nan
    fl[2, 0] = H.FAILED
    hs = H.ego_histories(rec[:, 0], fl[:, 0], 0.1, np.zeros(4), np.zeros(4))
    assert len(hs) == 1 and len(hs[0]) == 6 and np.isnan(hs[0].xref_deviation[3])
    assert H.episodes(fl)["end"][0].tolist() == [H.END_RUNNING]


def test_overflow_beyond_cap(H):
    assert H.recorded_ticks(5, 8) == (5, False)
    assert H.recorded_ticks(8, 8) == (8, False)
    assert H.recorded_ticks(11, 8) == (8, True)


def test_obstacle_positions_like_the_scripts(H):
    obs = np.arange(3 * 2 * 6, dtype=np.float64).reshape(3, 2, 6)
    pos = H.obstacle_positions(obs)
    assert len(pos) == 2 and [i for i, _ in pos[1]] == [0, 1, 2]
    assert pos[1][2] == (2, tuple(obs[2, 1].tolist()))
    assert H.obstacle_positions(None) == []


def test_set_recorder_argument_errors_without_gpu(pkg):
    """jsim_loop_set_recorder checks its arguments before it looks at the context: sizes and missing buffers are refused (-22)
    with a message, and so is a null context."""
    lib = pkg._cabi.load()
    rec = np.zeros((4, 2, 7))
    fl = np.zeros((4, 2), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    assert lib.jsim_loop_set_recorder(None, -1, 4, p(rec), p(fl), 0, None) == -22
    assert b"B=-1" in lib.jsim_last_error(None)
    assert lib.jsim_loop_set_recorder(None, 2, -3, p(rec), p(fl), 0, None) == -22
    assert lib.jsim_loop_set_recorder(None, 2, 4, p(rec), p(fl), -1, None) == -22
    assert lib.jsim_loop_set_recorder(None, 2, 4, None, p(fl), 0, None) == -22
    assert b"rec and flags" in lib.jsim_last_error(None)
    assert lib.jsim_loop_set_recorder(None, 2, 4, p(rec), None, 0, None) == -22
    assert lib.jsim_loop_set_recorder(None, 2, 4, p(rec), p(fl), 0, None) == -22
    assert b"null ctx" in lib.jsim_last_error(None)
    assert lib.jsim_loop_set_recorder(None, 2, 0, None, None, 0, None) == -22


def test_set_recorder_is_declared_exported_and_documented(pkg):
    assert len(pkg._header.header().functions["jsim_loop_set_recorder"].params) == 7
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_set_recorder.argtypes) == 7 and lib.jsim_loop_set_recorder.restype is ctypes.c_int
    assert "`jsim_loop_set_recorder`" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_record_is_a_keyword_of_every_loop(pkg):
    import inspect
    for cls in (pkg.ClosedLoop, pkg.ScenarioLoop, pkg.InteractingLoop):
        assert inspect.signature(cls.__init__).parameters["record"].default == 0
