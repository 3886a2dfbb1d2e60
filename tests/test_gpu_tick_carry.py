"""What the fused closed loop carries from tick to tick in registers -- the plant step's sin / cos from the rollout, tan of the warm
start's steer from the outputs to the next rollout -- must not depend on where a launch ends: 12 ticks as one launch, as three of
four and as twelve of one give the same history, records, final state, index, warm start and status bit for bit.  T = 13 and 20 on the
kernels with helper wavefronts (eight egos) and without (the same eight in front of a batch larger than the CU count, the way
test_helper_wavefronts_change_nothing switches), T = 40 on the four-wave kernel."""
import math

import numpy as np
import pytest
import torch

from gpu_helpers import cu_count

pytestmark = pytest.mark.gpu

DL_ = 1.0
K = 12
MAX_AGE = 25
SPLITS = ((12,), (4, 4, 4), (1,) * 12)
FAILED, GOAL, AGE = 1, 2, 4          # JSIM_REC_* (include/jsim_mpc.h)
E_RESPAWN, E_ANOMALY, E_NEGZERO, E_WARM, E_FAST = 0, 1, 2, 3, 4


def paths():
    """Three paths, a point per metre: (0) east along y = 0, then back west 0.6 m beside itself -- an ego on the first leg comes to
    where the points of the second are among its three nearest and the nearest-index search raises; (1) a gentle left arc; (2) the
    x axis."""
    s = np.arange(31.0)
    out = np.column_stack([s, np.zeros(31), np.zeros(31)])
    back = np.column_stack([np.arange(30.0, 17.0, -1.0), np.full(13, 0.6), np.full(13, math.pi)])
    p0 = np.vstack([out, [[30.4, 0.3, math.pi / 2]], back])
    R = 60.0
    s = np.arange(80.0)
    p1 = np.column_stack([R * np.sin(s / R), R * (1 - np.cos(s / R)), s / R])
    s = np.arange(60.0)
    p2 = np.column_stack([s, np.zeros(60), np.zeros(60)])
    return [p0, p1, p2]


def scenario(T):
    """Eight egos (x0 = x, y, v, yaw) and what the loop starts them with.  Ego E_RESPAWN is four ticks short of MAX_AGE; E_ANOMALY
    drives into the place where path 0 runs beside itself and fails there, mid-run; E_NEGZERO starts with y = yaw = -0.0; E_WARM
    with a warm start; E_FAST above its speed limit (the first tick fails and brakes, steering with the di it is given)."""
    P = paths()
    on = lambda p, i, lat=0.0, dyaw=0.0: (P[p][i, 0] - lat * math.sin(P[p][i, 2]), P[p][i, 1] + lat * math.cos(P[p][i, 2]), P[p][i, 2] + dyaw)
    rows = [(1, 5, 5.0, 0.0, 0.0), (0, 13, 5.0, 0.0, 0.0), (2, 3, 4.0, 0.0, 0.0), (1, 20, 5.0, 0.3, 0.05), (1, 30, 9.5, 0.0, 0.0),
            (1, 70, 3.0, -0.2, 0.0), (2, 10, 6.0, 0.5, 0.2), (0, 2, 5.0, 0.1, -0.05)]
    B = len(rows)
    x0 = np.zeros((B, 4))
    for b, (p, i, v, lat, dyaw) in enumerate(rows):
        x, y, yaw = on(p, i, lat, dyaw)
        x0[b] = (x, y, v, yaw)
    x0[E_NEGZERO, 1] = x0[E_NEGZERO, 3] = -0.0
    path_id = np.array([r[0] for r in rows], dtype=np.int32)
    oa, od = np.zeros((B, T)), np.zeros((B, T))
    oa[E_WARM], od[E_WARM] = 0.5, np.linspace(0.08, -0.04, T)
    age = np.zeros(B, dtype=np.int32)
    age[E_RESPAWN] = MAX_AGE - 4
    di_ai = np.zeros((B, 2))
    di_ai[E_FAST, 0] = 0.1
    return dict(x0=x0, path_id=path_id, path_len=np.array([len(P[p]) for p in path_id], dtype=np.int32),
                target_ind=np.array([r[1] for r in rows], dtype=np.int64), oa=oa, od=od, age=age, di_ai=di_ai)


def _run(pkg, T, sc, reps, split):
    """The scenario's egos, `reps` times over, through K ticks in launches of `split` ticks: what the loop leaves, rows of the
    first copy."""
    B = len(sc["x0"])
    rep = lambda a: np.concatenate([a] * reps)
    eng = pkg.BatchedMPC(paths(), rep(sc["path_id"]), dl=DL_, T=T, speed=30 / 3.6, device="cuda:0", smooth=False)
    eng.load_state(rep(sc["target_ind"]), rep(sc["oa"]), rep(sc["od"]), rep(sc["path_len"]))
    eng.di_ai.copy_(torch.from_numpy(rep(sc["di_ai"])))
    loop = pkg.ClosedLoop(eng, torch.from_numpy(rep(sc["x0"])).to(eng.device), hist_cap=K, max_age=MAX_AGE, record=K)
    loop.age.copy_(torch.from_numpy(rep(sc["age"])))
    for n in split:
        loop.run(n)
    torch.cuda.synchronize()
    out = dict(hist=loop.hist[:, :B], rec=loop.recorder.rec[:, :B], flags=loop.recorder.flags[:, :B], x0=loop.x0[:B], age=loop.age[:B],
               target_ind=eng.target_ind[:B], oa=eng.oa[:B], od=eng.od[:B], status=eng.status[:B], di_ai=eng.di_ai[:B])
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    eng.close()
    return out


@pytest.mark.parametrize("T,helpers", [(13, True), (13, False), (20, True), (20, False), (40, None)])
def test_launch_boundaries_change_nothing(pkg, T, helpers):
    sc = scenario(T)
    B = len(sc["x0"])
    reps = 1 if helpers is not False else cu_count() // B + 2          # helpers off: more egos than CUs
    assert (reps * B > cu_count()) == (helpers is False)
    runs = [_run(pkg, T, sc, reps, split) for split in SPLITS]
    fl = runs[0]["flags"]
    print(f"T={T} helpers={helpers}: failed ticks per ego {[(fl[:, b] & FAILED).nonzero()[0].tolist() for b in range(B)]}, "
          f"respawns {[(fl[:, b] & (GOAL | AGE)).nonzero()[0].tolist() for b in range(B)]}")
    # the scenario does what it is there for
    assert fl[3, E_RESPAWN] & AGE and not (fl[:, E_RESPAWN] & FAILED).any()
    bad = (fl[:, E_ANOMALY] & FAILED).nonzero()[0]
    assert len(bad) and bad[0] > 0                                       # fails mid-run
    assert fl[0, E_FAST] & FAILED and not (fl[-1, E_FAST] & FAILED)      # fails at once, recovers
    assert runs[0]["hist"][0, E_FAST, 0] == 0.1                          # .. steering with the di it was given
    assert not (fl[:, [E_NEGZERO, E_WARM]] & FAILED).any()
    for other, split in zip(runs[1:], SPLITS[1:]):
        for k in runs[0]:                                                # bytes, not values: NaN and the sign of a zero count
            assert runs[0][k].tobytes() == other[k].tobytes(), (k, split)
