"""The cases of tests/golden/predictions.npz: recorder buffers of 200 ticks, no RNG, every series piecewise
linear in its controls -- eight recorded vehicles and five egos, as jsim_loop_score_predictions reads them -- and what the fixture
stores of them.  The fixture holds expected outputs only; the inputs are regenerated here and pinned by a digest.

Every series is integrated tick by tick from controls that are constant or ramp linearly.  Where the heading is exactly 0 and the
reported tuple is the one that drives the vehicle, a prediction equals the recorded future bit for bit on any libm (cos(0) = 1,
sin(0) = 0, tan(0) = 0): error 0.  Everywhere else the vehicle is driven by something its tuple does not report (a steering ramp, a
speed drift, a jump in speed), so that the error grows with the look-ahead and the largest error of a tick is well apart from the
next: the integer outputs do not hang on the last bit of a cosine.

Vehicles (rows 0..7): 0 straight at constant speed; 1 parked until tick 20, then off at once; 2 straight, then from tick 180 a steering
ramp under a speed drift; 3 accelerating (a = 0.5), braking (a = -1) from tick 185; 4 a cyclist (wheelbase 1.0)
on a steering ramp from tick 180; 5 reported parked but moving 2.5 m a tick (the tolerance exceeded at sample 0); 6 moving 1 / 32 m a
tick more than reported (exceeded first at sample 63); 7 parked.
Egos (rows 8..12): 0 braking to a stop; 1, 2, 3 at constant speed with episodes ending on ticks 62 / 127, 63 / 128 and 64 / 129 (GOAL, then
AGE), the spawn pose far away; 4 straight to an AGE end on tick 170, then from a spawn pose of another heading on a steering ramp under
acceleration.  (The transitions stand late in the record: a (tick, row) with an error costs the fixture 144 incompressible bytes,
and every tick within 64 of a vehicle's transition has one.)"""
import hashlib
import math
import os

import numpy as np

import predictions_numpy as PN

N, DT, L_CAR, L_BIKE = 200, 0.2, 2.86, 1.0
TOL = 1.99
TICK_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
STEPS = (1, 35, 63, 64)
N_OBS, B = 8, 5
L_OBS = np.array([L_CAR] * 4 + [L_BIKE] + [L_CAR] * 3)
FAILED, GOAL, AGE = 1, 2, 4
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predictions.npz")


def ramp(k, k0, k1, v0, v1):
    """v0 up to tick k0, v1 from tick k1 on, linear between."""
    return v0 if k <= k0 else v1 if k >= k1 else v0 + (v1 - v0) * (k - k0) / (k1 - k0)


def vehicle_series(x, y, v, yaw, L, reported, actual):
    """[N][6] get() tuples.  reported(k, v) -> (v, a, steer) as the tuple of tick k shows them; actual(k, v) -> (v, a, steer) that
    move the vehicle from tick k to k + 1, by MovingObstaclesPrediction's own step."""
    out = np.zeros((N, 6))
    for k in range(N):
        rv, ra, rs = reported(k, v)
        out[k] = (x, y, rv, yaw, ra, rs)
        v, a, s = actual(k, v)
        x += v * math.cos(yaw) * DT
        y += v * math.sin(yaw) * DT
        v += a * DT
        yaw += (v / L) * math.tan(s) * DT
    return out


def vehicles():
    same = lambda f: (f, f)
    rows = []
    rows.append(vehicle_series(-30.0, -3.0, 2.5, 0.0, L_CAR, *same(lambda k, v: (2.5, 0.0, 0.0))))
    rows.append(vehicle_series(-20.0, -3.0, 0.0, 0.0, L_CAR, *same(lambda k, v: (0.0 if k < 20 else 2.5, 0.0, 0.0))))
    rows.append(vehicle_series(-80.0, 3.0, 5.0, 0.0, L_CAR, lambda k, v: (v, 0.0, ramp(k, 180, 195, 0.0, 0.3)),
                               lambda k, v: (v, 0.0 if k < 180 else 0.05, ramp(k, 180, 195, 0.0, 0.3))))

    def accel(k, v):
        a = 0.5 if k < 185 else -1.0
        if a < 0.0 and v + a * DT <= 1e-9:
            return 0.0, 0.0, 0.0
        return v, a, 0.0
    rows.append(vehicle_series(-40.0, 6.0, 1.0, 0.0, L_CAR, *same(accel)))
    rows.append(vehicle_series(-25.0, -6.0, 2.5, 0.0, L_BIKE, lambda k, v: (v, 0.0, ramp(k, 180, 195, 0.0, 0.1)),
                               lambda k, v: (v, 0.0 if k < 180 else 0.02, ramp(k, 180, 195, 0.0, 0.1))))
    rows.append(vehicle_series(-60.0, 9.0, 12.5, 0.0, L_CAR, lambda k, v: (0.0, 0.0, 0.0), lambda k, v: (12.5, 0.0, 0.0)))
    rows.append(vehicle_series(-50.0, 12.0, 2.65625, 0.0, L_CAR, lambda k, v: (2.5, 0.0, 0.0), lambda k, v: (2.65625, 0.0, 0.0)))
    rows.append(vehicle_series(5.0, 15.0, 0.0, 0.0, L_CAR, *same(lambda k, v: (0.0, 0.0, 0.0))))
    return np.stack(rows, axis=1)                                      # [N][N_OBS][6]


def ego_series(first, spawn, ends, control):
    """rec [N][7] and flags [N] of one ego: the plant's own step (lib/simulation.py:35-47) from `first` = (x, y, v, yaw) under
    control(k, v) -> (a, delta); ends: {tick: flag}; behind an end the ego stands at `spawn`."""
    rec, flags = np.zeros((N, 7)), np.zeros(N, dtype=np.int32)
    x, y, v, yaw = first
    for k in range(N):
        a, d = control(k, v)
        x += v * math.cos(yaw) * DT
        y += v * math.sin(yaw) * DT
        yaw += (v / L_CAR) * math.tan(d) * DT
        v += a * DT
        rec[k] = (x, y, yaw, v, d, a, 0.0)
        if k in ends:
            flags[k] = ends[k]
            x, y, v, yaw = spawn
    return rec, flags


def egos():
    def brake(k, v):
        if k < 20:
            return 0.0, 0.0
        return (-v / DT, 0.0) if v - 1.0 * DT <= 1e-9 else (-1.0, 0.0)
    rows = [((-10.0, 0.0, 5.0, 0.0), (-10.0, 0.0, 5.0, 0.0), {}, brake)]
    for i, ends in enumerate(({62: GOAL, 127: AGE}, {63: GOAL, 128: AGE}, {64: GOAL, 129: AGE})):
        rows.append(((-5.0, 20.0 + 3.0 * i, 2.5, 0.0), (-400.0, 50.0 + 3.0 * i, 2.5, 0.0), ends, lambda k, v: (0.0, 0.0)))
    rows.append(((0.0, -20.0, 2.5, 0.0), (30.0, -40.0, 1.0, 0.3), {170: AGE},
                 lambda k, v: (0.0, 0.0) if k <= 170 else (0.05, ramp(k, 171, 190, 0.1, 0.2))))
    out = [ego_series(*r) for r in rows]
    return (np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1),
            np.array([r[0] for r in rows]), np.array([r[1] for r in rows]))


def recorder_arrays():
    rec, flags, x_first, x_spawn = egos()
    shapes = np.array([[L / 2 + 0.5, L / 2 - 0.5, 1.5, L] for L in L_OBS])       # (cc_front, cc_rear, radius, wheelbase): only L is read
    return {"rec": rec, "flags": flags, "obs": vehicles(), "x_first": x_first, "x_spawn": x_spawn, "L_obs": L_OBS.copy(), "shapes": shapes}


def digest(A):
    return hashlib.sha256(b"".join(np.ascontiguousarray(A[k]).tobytes() for k in ("rec", "flags", "obs", "x_first", "x_spawn", "L_obs"))).hexdigest()


def cached(predictor):
    """predictor(tup, L, dt, n_steps) called once per (tuple, L, n_steps)."""
    memo = {}

    def call(tup, L, dt, n_steps):
        key = (np.asarray(tup, dtype=np.float64).tobytes(), float(L), int(n_steps))
        if key not in memo:
            memo[key] = predictor(tup, L, dt, n_steps)
        return memo[key]
    return call


def prefix_predictor():
    """The restatement's predictor, each tuple rolled out once to 64 samples: a shorter prediction is its first samples."""
    full = cached(lambda tup, L, dt, n_steps: PN.predict(tup, L, dt, 64))
    return lambda tup, L, dt, n_steps: full(tup, L, dt, 64)[:n_steps]


def restate(A, n, n_steps, predictor=None, tol=TOL):
    """All 13 rows (the vehicles, then the egos) on the first n ticks."""
    return PN.eval_predictions(A["rec"], A["flags"], A["obs"], A["x_first"], A["x_spawn"], True, n_steps, tol, DT, A["L_obs"], L_CAR, n=n,
                               predictor=predictor or prefix_predictor())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8) if a.size else a, b.view(np.uint8) if b.size else b)


def pack(results):
    """What the fixture stores of results {(n, n_steps): eval_predictions' dict}: per n_steps the outputs of the longest cut in full;
    of the shorter cuts step_cnt (one after the other, n_steps-major) and of pt_i / pt_d only the slots (n_steps, cut, tick, row)
    that differ from the longest cut's -- the ticks whose horizon the cut shortens."""
    out = {}
    top = max(TICK_COUNTS)
    where, cut_i, cut_d, cut_cnt = [], [], [], []
    for S in STEPS:
        full = results[top, S]
        for k in ("pt_i", "pt_d", "step_sum", "step_cnt"):
            out[f"s{S}_{k}"] = full[k].astype(np.int8) if k == "pt_i" else full[k].astype(np.int16) if k == "step_cnt" else full[k]
        for n in TICK_COUNTS[:-1]:
            r = results[n, S]
            for k in range(n):
                for v in range(r["pt_i"].shape[1]):
                    if not (same_bits(r["pt_i"][k, v], full["pt_i"][k, v]) and same_bits(r["pt_d"][k, v], full["pt_d"][k, v])):
                        where.append((S, n, k, v)); cut_i.append(r["pt_i"][k, v]); cut_d.append(r["pt_d"][k, v])
            cut_cnt.append(r["step_cnt"].reshape(-1))
    out["cut_where"] = np.array(where, dtype=np.int16).reshape(-1, 4)
    out["cut_pt_i"], out["cut_pt_d"] = np.array(cut_i, dtype=np.int8).reshape(-1, 3), np.array(cut_d).reshape(-1, 6)
    out["cut_step_cnt"] = np.concatenate(cut_cnt).astype(np.int16)
    return out


def fixture():
    g = np.load(FIXTURE)
    assert str(g["digest"]) == digest(recorder_arrays()), "tests/prediction_cases.py no longer makes the inputs of predictions.npz"
    return g


def expected(g, n, S):
    """pt_i [n][13][3], pt_d [n][13][6], step_cnt [13][S] (and, of the longest cut, step_sum) of the cut to n ticks at n_steps = S, from
    the fixture."""
    top, V = max(TICK_COUNTS), N_OBS + B
    pt_i, pt_d = g[f"s{S}_pt_i"][:n].astype(np.int32), g[f"s{S}_pt_d"][:n].copy()
    if n == top:
        return {"pt_i": pt_i, "pt_d": pt_d, "step_sum": g[f"s{S}_step_sum"], "step_cnt": g[f"s{S}_step_cnt"].astype(np.int32)}
    w = g["cut_where"].astype(np.int64)
    mine = (w[:, 0] == S) & (w[:, 1] == n)
    pt_i[w[mine, 2], w[mine, 3]] = g["cut_pt_i"][mine]
    pt_d[w[mine, 2], w[mine, 3]] = g["cut_pt_d"][mine]
    at = 0
    for s in STEPS:
        for m in TICK_COUNTS[:-1]:
            if (s, m) == (S, n):
                return {"pt_i": pt_i, "pt_d": pt_d, "step_cnt": g["cut_step_cnt"][at:at + V * s].reshape(V, s).astype(np.int32)}
            at += V * s
    raise KeyError((n, S))
