"""The path-yaw trig table (jsim_mpc_set_paths -> path_trig_kernel -> KP::ptrig) against the register kernels' own evaluation
(JSIM_PATH_TRIG=0 leaves the table out): S3 of the one-wave kernels (T = 13, 20: eight egos take the instantiations with helper
wavefronts) and of the four-wave kernel (T = 40) must build the same QP and return the same solution bit for bit, whatever the yaw."""
import dataclasses
import importlib
import math

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
from gpu_helpers import debug_bufs

pytestmark = pytest.mark.gpu

DL_ = 1.0
N_PTS = 44
# the yaws that matter to sincos: both zeros, the quadrant boundaries (where yaw + pi/2 lands on another), beyond one turn, a
# subnormal, and two arguments of its large-argument reduction
SPECIAL = (0.0, -0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 3 * math.pi, 7.5, -9.0, 1e-310, 1e5, 1e22)
AT = (1, 15, 29)         # the specials sit at path points AT[k] + 0 .. 11: behind the start, in the middle, towards the end


def _path():
    """One straight path along x, a point per metre, whose yaw column is what the test is about."""
    p = np.zeros((N_PTS, 3))
    p[:, 0] = DL_ * np.arange(N_PTS)
    p[:, 2] = 0.05 * np.sin(0.4 * np.arange(N_PTS))
    for a in AT:
        p[a:a + len(SPECIAL), 2] = SPECIAL
    return p


def _egos(T):
    """Eight egos: at the start and in the middle at several speeds (a metre per step at 5 m/s: lane t's reference point is
    t + 1 points ahead), off the path with a warm start, and one ON the last point -- every lane of it has `rend`."""
    B = 8
    at = np.array([0, 0, 14, 20, 27, N_PTS - 1, 5, 30])
    x0 = np.zeros((B, 4))
    x0[:, 0] = DL_ * at
    x0[:, 2] = [5.0, 2.5, 5.0, 5.0, 5.0, 1.0, 4.0, 1.0]
    x0[6, 1], x0[6, 3] = 0.4, 0.1
    oa, od = np.zeros((B, T)), np.zeros((B, T))
    oa[6], od[6] = 0.5, np.linspace(0.05, -0.05, T)
    return x0, at.astype(np.int64), oa, od


def _config(yaw_weight):
    """The stock weights; without the yaw terms the jumps of the yaw column cost nothing and every solve succeeds (with them the yaw
    errors of up to 1e22 rad leave most of the QPs without a solution the active-set method finds: status 1, zeroed outputs)."""
    c = importlib.import_module(PKG_NAME + ".config").MPCConfig.from_json()
    return c if yaw_weight else dataclasses.replace(c, Q_v_yaw=[c.Q_v_yaw[0], 0.0], Qf=list(c.Qf[:3]) + [0.0])


def _solve(pkg, T, yaw_weight):
    x0, tind, oa, od = _egos(T)
    B = len(x0)
    eng = pkg.BatchedMPC([_path()], np.zeros(B, dtype=np.int32), dl=DL_, T=T, speed=30 / 3.6, config=_config(yaw_weight),
                         device="cuda:0", smooth=False)
    eng.load_state(tind, oa, od, np.full(B, N_PTS, dtype=np.int32))
    dbg = debug_bufs(eng)
    eng.solve(torch.from_numpy(x0).to(eng.device), debug=dbg)
    torch.cuda.synchronize()
    out = {"H": dbg["H"], "g": dbg["g"], "oa": eng.oa, "od": eng.od, "status": eng.status, "active_mask": eng.active_mask}
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    ridx = dbg["ref_idx"].cpu().numpy().copy()
    eng.close()
    return out, ridx


@pytest.mark.parametrize("yaw_weight", (True, False), ids=("stock", "no-yaw-weight"))
@pytest.mark.parametrize("T", (13, 20, 40))
def test_path_trig_table_changes_nothing(pkg, monkeypatch, T, yaw_weight):
    monkeypatch.delenv("JSIM_PATH_TRIG", raising=False)
    with_table, ridx = _solve(pkg, T, yaw_weight)
    monkeypatch.setenv("JSIM_PATH_TRIG", "0")
    without, ridx0 = _solve(pkg, T, yaw_weight)
    # the inputs do what they are there for: every special yaw is some lane's reference point short of the path's end (the lanes
    # that evaluate the trig), and the ego on the last point has the end in every lane
    assert np.array_equal(ridx, ridx0)
    inner = ridx[ridx < N_PTS - 1]
    assert all(any(a + k in inner for a in AT) for k in range(len(SPECIAL)))
    assert np.all(ridx[5] == N_PTS - 1)
    print(f"T={T} yaw_weight={yaw_weight}: status {with_table['status']}")
    if not yaw_weight:
        assert np.all(with_table["status"] == 0) and np.abs(with_table["od"]).max() > 0   # (as the CPU oracle solves them)
    for k in with_table:                                   # bytes, not values: NaN and the sign of a zero count
        assert with_table[k].tobytes() == without[k].tobytes(), k
