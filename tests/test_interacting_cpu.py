"""Interacting egos (InteractingLoop, jsim_loop_run_interacting) without a GPU: the reference's interactive_mpc loop recorded by
tests/golden/make_golden_loop_interact.py replayed by the numpy glue oracle, the new C-ABI exports against the header, and
the host-side refusal of bad group layouts."""
import ctypes
import os
import types

import numpy as np
import pytest

from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("jsim_loop_set_groups", "jsim_loop_predict_egos", "jsim_loop_run_interacting")


@pytest.fixture(scope="module")
def LO(oracle):
    import loop_oracle
    return loop_oracle


def mate_tuples(g):
    """[tick][ego] (x, y, v, yaw, a = 0, delta applied last tick) -- how every ego is predicted at the start of each tick."""
    t = g["ticks"]
    out = np.zeros(t.shape[:2] + (6,))
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = t[..., 0], t[..., 1], t[..., 3], t[..., 2]
    out[1:, :, 5] = t[:-1, :, 12]
    out[..., 5] *= 1.0 - t[..., 14]          # 0 after a respawn
    return out


def test_interacting_reference_loop_replayed_by_the_oracle_glue(LO):
    """Every tick, every ego: the oracle's glue with the other egos as obstacles reproduces the recorded progress index, path
    length and collision flag exactly, and the predictions the others saw to 1e-12."""
    g = load_golden("loop_interact_T13.npz")
    ticks, preds = g["ticks"], g["preds"]
    full = [g["smoothed0"], g["smoothed1"]]
    dl = float(g["dl"])
    assert LO.extra_cutoff_margin(dl) == int(g["margin"]) and int(g["frame_window"]) == 20
    tup = mate_tuples(g)
    n_ticks, n = ticks.shape[:2]
    n_cut, worst = 0, 0.0
    for i in range(n_ticks):
        for k in range(n):
            p = LO.predict_obstacle(*tup[i, k], dt=0.2)
            worst = max(worst, float(np.abs(p - preds[i, k]).max()))
        for j in range(n):
            x, y, yaw, v, idx_in, prev_len, idx_out, plen, hit = ticks[i, j, :9]
            obst = [tup[i, k] for k in range(n) if k != j]
            st, idx, path_len, col = LO.loop_pre_tick((x, y, yaw, v), int(idx_in), None if prev_len < 0 else int(prev_len),
                                                      full[j], obst, dl, frame_window=20)
            assert st == 0 and idx == int(idx_out) and path_len == int(plen) and (col is not None) == bool(hit), (i, j)
            n_cut += bool(hit)
    assert worst <= 1e-12, worst
    assert n_cut >= 10 and n_cut == int(ticks[:, :, 8].sum())
    assert ticks[:, :, 14].sum() >= 1          # the respawn rule was exercised


def test_interacting_exports_declared_in_the_header(pkg):
    hdr = pkg._header.header().functions
    for name in NEW_EXPORTS:
        assert hdr[name].ret == "int", name
    so = ctypes.CDLL(pkg.build.build())
    for name in NEW_EXPORTS:
        assert hasattr(so, name), name
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_run_interacting.argtypes) == len(hdr["jsim_loop_run_interacting"].params) == len(lib.jsim_loop_run_scenario.argtypes)
    assert len(lib.jsim_loop_set_groups.argtypes) == 4 and len(lib.jsim_loop_predict_egos.argtypes) == 7
    assert lib.jsim_loop_set_groups(None, 4, 1, None) == -22      # null ctx: refused before anything else
    assert lib.jsim_loop_predict_egos(None, 4, None, None, 35, None, None) == -22


@pytest.mark.parametrize("kw", [
    dict(),                                                   # neither
    dict(group_off=[0, 4], group_sizes=[4]),                  # both
    dict(group_off=[0, 3]),                                   # does not reach B
    dict(group_off=[1, 4]),                                   # does not start at 0
    dict(group_off=[0, 2, 2, 4]),                             # an empty group
    dict(group_sizes=[9, -5]),                                # a group of 9, then a negative one
    dict(group_sizes=[]),
    dict(group_off=[0.0, 4.0]),                               # not integers
])
def test_interacting_loop_rejects_bad_group_layouts_before_device_work(pkg, kw):
    """The layout is checked before the engine is touched: an object with nothing but B stands in for the engine."""
    eng = types.SimpleNamespace(B=4)
    with pytest.raises(ValueError):
        pkg.InteractingLoop(eng, None, **kw)


def test_interacting_loop_rejects_too_many_obstacles_per_ego(pkg):
    eng = types.SimpleNamespace(B=8)
    specs = [dict(direction=1, speed=5.0)] * 2
    with pytest.raises(ValueError, match="largest group"):
        pkg.InteractingLoop(eng, None, group_sizes=[8], obstacle_specs=specs)


def test_group_offsets(pkg):
    CL = pkg.closed_loop
    assert CL.group_offsets(10, group_sizes=[4, 4, 2]).tolist() == [0, 4, 8, 10]
    assert CL.group_offsets(3, group_off=np.array([0, 1, 3])).dtype == np.int32
