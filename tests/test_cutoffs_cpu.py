"""The collision cut-off of every recorded tick (jsim_loop_eval_cutoffs) without a GPU: the numpy restatement
(tests/cutoffs_numpy.py) on the reference's own loops -- tests/golden/loop_real_T13.npz and loop_interact_T13.npz turned into
recordings -- history.cutoff_episodes on hand-made series, and the C entry point's declaration, binding and the -22 refusals that
need no context.  (The refusals that read the context's tables need a context, so a device: tests/test_gpu_cutoffs.py.)"""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

GOAL, AGE = 2, 4
NAMES = ("rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "frame_window", "margin", "n_steps", "speed_cutoff", "interacting",
         "chunk_ticks", "first_tick", "carry", "status", "idx", "cut", "hit", "first", "col_xy")


@pytest.fixture(scope="module")
def CN(oracle):
    import cutoffs_numpy
    return cutoffs_numpy


def real_recording(g):
    """loop_real_T13.npz as a one-ego recording: tick k's record is the state tick k + 1 starts from (the last one: `final`), its
    applied controls, and the GOAL flag on the last tick (the reference's loop breaks on is_goal there)."""
    t = g["ticks"]
    K = len(t)
    after = np.concatenate([t[1:, :4], g["final"][None, :4]])             # x, y, yaw, v
    rec = np.zeros((K, 1, 7))
    rec[:, 0, :4], rec[:, 0, 4], rec[:, 0, 5] = after, t[:, 12], t[:, 13]
    flags = np.zeros((K, 1), dtype=np.int32)
    flags[-1, 0] = GOAL
    x_first = t[0, [0, 1, 3, 2]][None]
    return rec, flags, t[:, 15:].reshape(K, -1, 6), x_first, x_first.copy()


def interact_recording(g):
    """loop_interact_T13.npz as a recording of two egos: the recording respawns at the start of a tick (column 14), the recorder at
    the end of the one before -- that record carries the end flag, and the tick behind it starts from x_spawn."""
    t = g["ticks"]
    K, n = t.shape[:2]
    after = np.concatenate([t[1:, :, :4], g["final"][None, :, :4]])
    rec = np.zeros((K, n, 7))
    rec[..., :4], rec[..., 4], rec[..., 5] = after, t[..., 12], t[..., 13]
    flags = np.zeros((K, n), dtype=np.int32)
    flags[:-1][t[1:, :, 14] != 0] = GOAL
    x_first = t[0][:, [0, 1, 3, 2]]
    return rec, flags, x_first, x_first.copy()


def test_restatement_reproduces_the_reference_loop(CN):
    g = load_golden("loop_real_T13.npz")
    t = g["ticks"]
    rec, flags, obs, x_first, x_spawn = real_recording(g)
    out = CN.replay(rec, flags, obs, x_first, x_spawn, [g["trajectory_smoothed"]], [0], float(g["dl"]))
    assert len(t) == 91 and not out["status"].any()
    assert np.array_equal(out["idx"][:, 0], t[:, 6].astype(np.int64))
    assert np.array_equal(out["cut"][:, 0], t[:, 7].astype(np.int64))
    assert np.array_equal(out["hit"][:, 0], t[:, 8] != 0) and int(out["hit"].sum()) == 35
    assert np.array_equal(np.isnan(out["col_xy"][:, 0, 0]), t[:, 8] == 0)
    # the carried values are the recording's own: idx_in and prev_len of every tick
    assert np.array_equal(np.concatenate([[0], out["idx"][:-1, 0]]), t[:, 4].astype(np.int64))
    assert np.array_equal(np.concatenate([[-1], out["cut"][:-1, 0]]), t[:, 5].astype(np.int64))
    assert out["carry"].tolist() == [[0, -1, int(t[-1, 7])]]              # the last record ended the episode
    # in pieces, cut between any two ticks
    for k in (1, 23, 57, 90):
        a = CN.replay(rec, flags, obs, x_first, x_spawn, [g["trajectory_smoothed"]], [0], float(g["dl"]), n_ticks=k)
        b = CN.replay(rec, flags, obs, x_first, x_spawn, [g["trajectory_smoothed"]], [0], float(g["dl"]), first_tick=k, carry=a["carry"])
        for key in ("status", "idx", "cut", "hit"):
            assert np.array_equal(np.concatenate([a[key], b[key]]), out[key]), (k, key)
        assert np.array_equal(b["carry"], out["carry"])


def test_restatement_reproduces_the_interacting_reference_loop(CN):
    g = load_golden("loop_interact_T13.npz")
    t = g["ticks"]
    K, n = t.shape[:2]
    rec, flags, x_first, x_spawn = interact_recording(g)
    assert (K, n) == (150, 2) and int((flags != 0).sum()) >= 1
    for k, j in zip(*np.nonzero(flags)):                                   # a respawned ego starts from its spawn state
        assert np.array_equal(t[k + 1, j, [0, 1, 3, 2]], x_spawn[j])
    out = CN.replay(rec, flags, None, x_first, x_spawn, [g["smoothed0"], g["smoothed1"]], [0, 1], float(g["dl"]),
                    frame_window=int(g["frame_window"]), groups=np.array([0, n]))
    assert not out["status"].any()
    assert np.array_equal(out["idx"], t[:, :, 6].astype(np.int64))
    assert np.array_equal(out["cut"], t[:, :, 7].astype(np.int64))
    assert np.array_equal(out["hit"], t[:, :, 8] != 0) and int(out["hit"].sum()) >= 10


def test_cutoff_episodes(pkg):
    H = pkg.history
    n = 12
    flags = np.zeros((n, 3), dtype=np.int32)
    hit = np.zeros((n, 3), dtype=bool)
    # ego 0: episodes [0, 5), [5, 6) (one tick), [6, 12) running; a cut-off run over ticks 3..7 crosses both ends
    flags[4, 0], flags[5, 0] = GOAL, AGE
    hit[3:8, 0] = True
    hit[10, 0] = True
    # ego 1: one running episode, two runs (2 and 3 ticks)
    hit[1:3, 1] = True
    hit[6:9, 1] = True
    # ego 2: its last record ends the episode: a running one without a tick follows; never cut off
    flags[n - 1, 2] = GOAL
    res = {"status": np.zeros((n, 3), np.int32), "idx": np.arange(n * 3).reshape(n, 3), "cut": np.full((n, 3), 100), "hit": hit,
           "first": np.where(hit, 7, -1), "col_xy": np.repeat(np.where(hit, 1.5, np.nan)[..., None], 2, axis=2)}
    eps = H.cutoff_episodes(res, flags)
    assert [len(e) for e in eps] == [3, 1, 2]
    got = [[(e["first_cut_tick"], e["n_cut"], e["longest_cut"]) for e in ego] for ego in eps]
    assert got[0] == [(3, 2, 2), (5, 1, 1), (6, 3, 2)]                     # the run 3..7 is three runs, one per episode
    assert got[1] == [(1, 5, 3)]
    assert got[2] == [(-1, 0, 0), (-1, 0, 0)]
    assert eps[0][1]["idx"].tolist() == [15] and eps[0][1]["col_xy"].shape == (1, 2) and eps[2][1]["hit"].shape == (0,)
    assert eps[0][2]["first"].tolist() == [7, 7, -1, -1, 7, -1]
    # against plain loops on random series
    rng = np.random.default_rng(3)
    flags = np.where(rng.random((60, 5)) < 0.1, GOAL, 0).astype(np.int32)
    hit = rng.random((60, 5)) < 0.5
    res = {k: np.zeros((60, 5)) for k in ("status", "idx", "cut", "first")}
    res.update(hit=hit.astype(np.int32), col_xy=np.zeros((60, 5, 2)))
    for b, ego in enumerate(H.cutoff_episodes(res, flags)):
        for e, (k0, k1, _) in zip(ego, H.episode_bounds(flags[:, b])):
            run = best = 0
            first = -1
            for k in range(k0, k1):
                run = run + 1 if hit[k, b] else 0
                best = max(best, run)
                if hit[k, b] and first < 0:
                    first = k
            assert (e["first_cut_tick"], e["n_cut"], e["longest_cut"]) == (first, int(hit[k0:k1, b].sum()), best)


def test_entry_point_is_declared_and_bound(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    args = [a for _, a in pkg._header.header().functions["jsim_loop_eval_cutoffs"].params]
    assert len(args) == 24 and args == ["ctx", "B", "n_ticks", *NAMES, "stream"]
    for cite in ("main/scenarios/mpc_intersection.py:104-143", "overtaking_cyclist_bidirectional_road.py:111-169"):
        assert cite in hdr
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_eval_cutoffs.argtypes) == 24
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert re.search(r"^\| `jsim_loop_eval_cutoffs` \|", doc, flags=re.M)
    assert callable(pkg.closed_loop.Recorder.cutoffs) and callable(pkg.history.cutoff_episodes)
    src = open(os.path.join(REPO, "av-simulation-at-intersections_amd", "csrc", "jsim_mpc.hip")).read()
    tail = src[src.index('#include "cutoff_ticks.inc"'):]                  # inside the block the kernel translation units leave out:
    assert tail.count("#if") == 0 and tail.count("#endif") == 1 and tail.rstrip().endswith("#endif /* !JSIM_KERNEL_TU */")


def test_argument_errors_without_gpu(pkg):
    """The header's -22 list as far as it needs no context: from the host, before any device call."""
    lib = pkg._cabi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                    # a non-null address; no refused call reads it

    def call(B=2, n=3, ctx=None, **over):
        a = {k: p for k in NAMES}
        a.update(n_obs=2, frame_window=10, margin=16, n_steps=35, speed_cutoff=0, interacting=0, chunk_ticks=0, first_tick=0)
        a.update(over)
        rc = lib.jsim_loop_eval_cutoffs(ctx, B, n, *[a[k] for k in NAMES], None)
        return rc, lib.jsim_last_error(None).decode()

    who = "jsim_loop_eval_cutoffs: "
    bad = [(dict(B=-1), "B=-1"), (dict(n=-1), "n_ticks=-1"), (dict(n_obs=-1), "n_obs=-1"), (dict(margin=-1), "margin=-1"),
           (dict(chunk_ticks=-1), "chunk_ticks=-1"), (dict(first_tick=-1), "first_tick=-1 outside [0, n_ticks=3]"),
           (dict(first_tick=4), "first_tick=4 outside [0, n_ticks=3]"), (dict(obs_rec=None), "null obs_rec with n_obs=2"),
           (dict(n_steps=0), "n_steps=0 outside [1, 64]"), (dict(n_steps=65), "n_steps=65 outside [1, 64]"),
           (dict(frame_window=-1), "frame_window=-1 outside [0, 32]"), (dict(frame_window=33), "frame_window=33 outside [0, 32]"),
           (dict(speed_cutoff=2), "speed_cutoff=2"), (dict(interacting=-1), "interacting=-1"),
           (dict(speed_cutoff=1, interacting=1), "truncate glue only")]
    for kw, msg in bad:
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in ("rec", "flags", "x_first", "x_spawn", "status", "idx", "cut", "hit", "first", "col_xy"):
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null device pointer", (k, rc, err)
        rc, err = call(n=0, **{k: None})                                   # also with nothing to do
        assert rc == -22, k
    rc, err = call()                                                       # every argument good: the missing context is what is left
    assert rc == -22 and err == who + "null ctx"
    good = [dict(carry=None), dict(n_obs=0, obs_rec=None), dict(n=0), dict(B=0), dict(first_tick=3), dict(speed_cutoff=1),
            dict(interacting=1), dict(frame_window=0), dict(frame_window=32), dict(n_steps=1), dict(n_steps=64), dict(chunk_ticks=7)]
    for kw in good:
        rc, err = call(**kw)                                               # none of these is an error of its own
        assert rc == -22 and err == who + "null ctx", (kw, err)
    assert not buf.any()
