"""The cases of tests/golden/reason_ticks.npz: synthetic position series for the per-tick stakeholder reasons,
chosen for the kernel's structure -- 64 ticks per chunk, two timers and one tracker bit carried from chunk to chunk, a reset at an
episode's first tick.  No RNG: an ego closes in on a slower cyclist, sits behind it, moves left across the centreline, passes it
and leaves its range, with the gap between the two given tick by tick as a piecewise-linear function whose knots put every event
on the tick a case is about.  Used by the fixture generator (tests/golden/make_golden_reason_ticks.py), which runs the reference on
them, by the CPU test, which rebuilds them and compares, and by the GPU test, which lays them out as recorder arrays."""
import os

import numpy as np

import reason_ticks_numpy as TN
import recorder_numpy as RN
from recorder_numpy import AGE, GOAL

N = 200                                              # ticks per case
TICK_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)  # every case is also evaluated cut to these lengths
SPLITS = (64, 37)                                    # the two-call splits of a run (restatement-made)
X_RIGHT, X_LEFT, X_CYC = 2.0, -2.0, 2.3              # the ego's lane positions and the cyclist's
V_CYC = 5.0 / 3.6
FAR = 1.0e3                                          # a timer threshold that is never reached


def par_row(**over):
    names = ("dt", "max_accel", "max_speed", "centerline", "width", "ref_d", "buf_d", "thr_d", "ref_c", "buf_c", "thr_c", "wheelbase")
    p = dict(zip(names, TN.DEFAULT_PAR.tolist()))
    p.update(over)
    return np.array([p[k] for k in names], dtype=np.float64)


def pw(knots, n=N):
    """Piecewise-linear through (tick, value) knots (ticks may be fractional: a knot at k - 0.5 puts a crossing between two ticks)."""
    k, v = zip(*knots)
    assert all(b > a for a, b in zip(k, k[1:])), knots
    return np.interp(np.arange(n, dtype=np.float64), k, v)


def accumulate(t, dt, count):
    for _ in range(count):
        t = t + dt
    return t


def _case(label, gap, x, par=None, threshold=0.7, carry=(0.0, 0.0, 0.0), flags=(), restated=False, veh=0):
    """gap [N] = cyclist's y minus the ego's at the start of each tick, x [N] = the ego's x; flags = ((tick, bit), ...)."""
    par = par_row() if par is None else par
    dt = par[0]
    cy = -20.0 + V_CYC * dt * np.arange(N)
    pos = np.stack([np.asarray(x, dtype=np.float64), cy - gap], axis=1)
    fl = np.zeros(N, dtype=np.int32)
    for k, bit in flags:
        fl[k] |= bit
    return {"label": label, "pos": pos, "cyc": np.stack([np.full(N, X_CYC), cy], axis=1), "flags": fl, "par": par,
            "threshold": float(threshold), "carry": np.array(carry, dtype=np.float64), "restated": bool(restated), "veh": int(veh)}


def _approach(par, enter_d, enter_c, hold, follow, tail=None):
    """Knots of a gap that crosses the driver's range between ticks enter_d - 1 and enter_d, the cyclist's between enter_c - 1 and
    enter_c, and reaches `follow` at tick `hold`; dx = X_CYC - X_RIGHT is part of the distance."""
    dx = X_CYC - X_RIGHT
    g_d, g_c = np.sqrt((par[5] + par[6]) ** 2 - dx * dx), np.sqrt((par[8] + par[9]) ** 2 - dx * dx)
    slope = (g_d - g_c) / (enter_c - enter_d)
    k = [(0, g_d + slope * (enter_d - 0.5)), (enter_d - 0.5, g_d), (enter_c - 0.5, g_c), (hold, follow)]
    return k + (tail if tail is not None else [(N, follow)])


def cases():
    out = []
    right = np.full(N, X_RIGHT)
    p0 = par_row()
    # 0: the whole manoeuvre at the reference's parameters: approach, follow at 9 m, left over ticks 100-115, pass, leave both ranges
    gap = pw(_approach(p0, 20, 30, 40, 9.0, [(115, 9.0), (150, -8.6), (151, -9.4), (170, -11.3), (171, -12.1), (N, -20.0)]))
    x = pw([(0, X_RIGHT), (100, X_RIGHT), (115, X_LEFT), (N, X_LEFT)])
    out.append(_case("the manoeuvre, reference parameters", gap, x))
    # 1-6: both timers first at their thresholds on tick X = 63, 64, 65, DT 0.1 and 0.2, carry-in not zero; the thresholds sit half
    # a step below the value the additions reach on tick X
    for X in (63, 64, 65):
        for dt, car in ((0.1, (1.3, 0.7, 0.0)), (0.2, (0.4, 2.6, 1.0))):
            e_d, e_c = 30, 41
            thr_d = accumulate(car[0], dt, X - e_d + 1) - dt / 2
            thr_c = accumulate(car[1], dt, X - e_c + 1) - dt / 2
            p = par_row(dt=dt, thr_d=thr_d, thr_c=thr_c)
            out.append(_case(f"timers at their thresholds on tick {X}, DT {dt}", pw(_approach(p, e_d, e_c, 50, 9.0)), right, par=p, carry=car))
    # 7-8: thresholds that are decimal multiples of DT: the additions land on them or one ulp beside them
    for dt, thr_d, thr_c in ((0.1, 0.8, 0.3), (0.2, 6.6, 1.4)):
        p = par_row(dt=dt, thr_d=thr_d, thr_c=thr_c)
        out.append(_case(f"thresholds on the grid of the additions, DT {dt}", pw(_approach(p, 57, 61, 70, 9.0)), right, par=p))
    # 9-12: entering a range between ticks 63 -> 64 and 64 -> 65; leaving one there (timers far from their thresholds)
    pf = par_row(thr_d=FAR, thr_c=FAR)
    out.append(_case("enter the driver's range on 64, the cyclist's on 65", pw(_approach(pf, 64, 65, 80, 9.0)), right, par=pf))
    out.append(_case("enter the driver's range on 65, the cyclist's on 66", pw(_approach(pf, 65, 66, 80, 9.0)), right, par=pf))
    for k in (64, 65):   # last tick inside the cyclist's range k - 1, inside the driver's k
        gap = pw([(0, 9.0), (k - 2, 9.0), (k - 0.5, 10.0 - 0.0045), (k + 0.5, 12.0 - 0.00375), (k + 2, 13.0), (N, 20.0)])
        out.append(_case(f"leave the cyclist's range on {k}, the driver's on {k + 1}", gap, right, par=pf, carry=(3.3, 2.1, 0.0)))
    # 13: chunks with exactly one in-range tick (70 and 130), none elsewhere
    gap = pw([(0, 14.0), (69, 14.0), (70, 9.5), (71, 14.0), (129, 14.0), (130, 9.5), (131, 14.0), (N, 14.0)])
    out.append(_case("one in-range tick per chunk", gap, right, par=par_row(thr_d=0.15, thr_c=0.15)))
    # 14-16: `below` at the chunk edge, from the cyclist's comfort alone (gap 7.9: 0.66, gap 8.6: 0.76)
    dip = lambda a, b: [(a - 1, 8.6), (a, 7.9), (b, 7.9), (b + 1, 8.6)]
    out.append(_case("below on 62-66: one trigger, on 62", pw([(0, 8.6)] + dip(62, 66) + [(N, 8.6)]), right, par=pf))
    out.append(_case("below first on 64: the tracker crosses the chunk", pw([(0, 8.6)] + dip(64, 70) + [(N, 8.6)]), right, par=pf))
    out.append(_case("below on 60-63, not on 64, again on 100-105", pw([(0, 8.6)] + dip(60, 63) + dip(100, 105) + [(N, 8.6)]), right, par=pf))
    # 17-20: respawn flags on tick 0 and on the last tick, on 62, 63 and 64: the next tick starts at the spawn state with timers of 0 and no
    # tracker; the ego is in range and below all the time, so every episode triggers on its first tick
    near = pw([(0, 7.9), (N, 7.9)])
    p = par_row(thr_d=2.0, thr_c=1.0)
    out.append(_case("respawn after tick 0 and after the last", near, right, par=p, carry=(1.9, 0.9, 1.0), flags=((0, GOAL), (N - 1, AGE))))
    for k, bit in ((62, AGE), (63, GOAL), (64, GOAL | AGE)):
        out.append(_case(f"respawn after tick {k}", near, right, par=p, carry=(0.5, 0.2, 0.0), flags=((k, bit),)))
    # 21-22: every entry of the row another one, two different rows, in the launch that holds the reference's rows
    for q, p in enumerate((par_row(dt=0.2, centerline=-0.5, width=1.8, ref_d=9.0, buf_d=1.5, thr_d=3.0, ref_c=6.5, buf_c=1.0, thr_c=2.0),
                           par_row(dt=0.05, centerline=0.4, width=2.4, ref_d=7.0, buf_d=4.5, thr_d=1.5, ref_c=5.0, buf_c=3.5, thr_c=1.0))):
        gap = pw(_approach(p, 25, 45, 60, 6.5, [(110, 6.5), (160, -9.0), (N, -14.0)]))
        x = pw([(0, X_RIGHT), (90, X_RIGHT), (109, X_LEFT), (N, X_LEFT)])   # (over 20 ticks the ego's edge would sit on a centreline)
        out.append(_case(f"another parameter row ({q})", gap, x, par=p))
    # 23-24: threshold 0.95
    out.append(_case("threshold 0.95, the manoeuvre", out[0]["cyc"][:, 1] - out[0]["pos"][:, 1], out[0]["pos"][:, 0], threshold=0.95))
    out.append(_case("threshold 0.95, below on 64-70 at 9.2 m", pw([(0, 9.9), (63, 9.9), (64, 9.2), (70, 9.2), (71, 9.9), (N, 9.9)]), right, par=pf, threshold=0.95))
    # restatement-made: no cyclist; the cyclist of another case (the GPU test's vehicle table puts it second or later)
    out.append(_case("no cyclist (restated)", out[0]["cyc"][:, 1] - out[0]["pos"][:, 1], out[0]["pos"][:, 0], restated=True, veh=-1))
    c = _case("the ego of case 0 with the cyclist of case 21 (restated)", out[0]["cyc"][:, 1] - out[0]["pos"][:, 1], out[0]["pos"][:, 0], restated=True)
    c["cyc"] = out[21]["cyc"].copy()
    out.append(c)
    return out


# ---- a case as recorder arrays ----
DECOY = 5.0e4                                        # where a record that must not be read puts the ego / a vehicle nobody follows


def recorder_arrays(cs):
    """rec [N][B][7], flags [N][B], obs [N][B + 1][6], x_first [B][4], x_spawn [B][4], veh_of [B], par, threshold, carry for a launch
    with one ego per case.  rec[k] is the start position of tick k + 1, except where flags[k] ends the episode: there rec[k] is a far
    away state (as the goal state would be) and tick k + 1 starts at x_spawn.  Vehicle 0 is a decoy; case b's cyclist is vehicle
    B - b (the order reversed), so that no ego's index is its own."""
    B = len(cs)
    heading = np.full((N, 1), np.pi / 2)
    A = RN.ego_arrays([np.hstack([c["pos"], heading]) for c in cs], [c["flags"] for c in cs], DECOY, labels=[c["label"] for c in cs])
    A["rec"][:, :, 2] = np.pi / 2                         # (a far away state keeps its heading here)
    obs = np.zeros((N, B + 1, 6))
    obs[:, 0, :2] = DECOY
    veh = np.zeros(B, dtype=np.int32)
    for b, c in enumerate(cs):
        veh[b] = B - b if c["veh"] >= 0 else -1
        obs[:, B - b, :2] = c["cyc"]
        obs[:, B - b, 2], obs[:, B - b, 3] = V_CYC, np.pi / 2
    return {**A, "obs": obs, "veh_of": veh, "par": np.stack([c["par"] for c in cs]),
            "threshold": np.array([c["threshold"] for c in cs]), "carry": np.stack([c["carry"] for c in cs])}


def restate(A, n=N, carry=None, k0=0):
    """The restatement on ticks k0 .. k0 + n - 1 of recorder_arrays' output (a piece that does not start at 0 starts from the state
    the piece before it left: x_first is the start position of tick k0)."""
    x_first = A["x_first"]
    if k0 > 0:
        x_first = A["x_first"].copy()
        x_first[:, :2] = TN.start_positions(A["rec"][:k0 + 1], A["flags"][:k0 + 1], A["x_first"], A["x_spawn"])[k0]
    return TN.eval_ticks(A["rec"][k0:k0 + n], A["flags"][k0:k0 + n], A["obs"][k0:k0 + n], x_first, A["x_spawn"], A["veh_of"], A["par"],
                         A["threshold"], A["carry"] if carry is None else carry)


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reason_ticks.npz"), allow_pickle=False)
    return _FIX
