"""The cases of tests/golden/plan_predictions.npz: recorder buffers and plan records of 200 ticks, no RNG, as
jsim_loop_score_plan_predictions reads them -- one group of ego rows per horizon T = 13, 20, 40 -- and what the fixture stores of
them.  The fixture holds expected outputs only; the inputs are regenerated here and pinned by a digest.

Every ego's records are integrated tick by tick by the plant's step (lib/simulation.py:35-47; the generator checks every record
against the reference's own Simulation.step, bit for bit) from controls that differ from the plans stored beside them, so that the
error grows with the look-ahead and a tick's largest error is well apart from the next.  Where the heading is exactly 0 a prediction
that is right equals the recorded future bit for bit on any libm (cos(0) = 1, sin(0) = 0, tan(0) = 0): error 0.  A standing ego
(v = 0 under an all-zero plan) is predicted exactly at any heading.  A (tick, row) with an error costs the fixture some 200
incompressible bytes, so the rows that turn stand still through a first episode that ends with AGE on tick 169 and do what they are
there for on ticks 170..199, from a spawn state of their own.

T = 13 (rows 0..9): 0 a plan followed exactly (accelerating, then constant speed: error 0, hold = m); 1 a plan that brakes to a stand
while the ego drives on; 2, 3, 4 at constant speed with episodes ending on ticks 62 / 127, 63 / 128 and 64 / 129 (GOAL, then AGE), the spawn
pose far away, the plan all zeros (also behind each respawn) but for ticks 118..123, where it accelerates and the ego does not;
5 steering beyond +-MAX_STEER, also in the held tail; 6 accelerating into MAX_SPEED; 7 reversing into MIN_SPEED; 8 failed solves
(status 1) over a non-zero plan, the ego on a steering ramp; 9 failed solves (status 2) with the last steering beyond MAX_STEER.
T = 20 (rows 0, 1): a plan followed exactly; a smooth plan against a steering ramp.  T = 40 (rows 0, 1): the same with a plan longer
than a prediction of 35 steps."""
import hashlib
import math
import os

import numpy as np

import plan_predictions_numpy as PPN

N, DT, L_CAR = 200, 0.2, 2.86
MAX_STEER, MAX_SPEED, MIN_SPEED = float(np.deg2rad(45.0)), 30.0 / 3.6, -5.0      # main/lib/simulation.py:23-25
TOL = 1.99
TICK_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
STEPS = (1, 35, 63, 64)
HORIZONS = (13, 20, 40)
FAILED, GOAL, AGE = 1, 2, 4
WAKE = 170                                                             # the first tick of the late rows' second episode
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_predictions.npz")


def ramp(k, k0, k1, v0, v1):
    """v0 up to tick k0, v1 from tick k1 on, linear between."""
    return v0 if k <= k0 else v1 if k >= k1 else v0 + (v1 - v0) * (k - k0) / (k1 - k0)


def plant_step(x, y, v, yaw, a, delta):
    """Simulation.step (main/lib/simulation.py:35-47 with Bicycle.step, main/bicycle/main.py:28-41)."""
    d = max(min(delta, MAX_STEER), -MAX_STEER)
    xd, yd, td = v * math.cos(yaw), v * math.sin(yaw), (v / L_CAR) * math.tan(d)
    x += xd * DT
    y += yd * DT
    yaw += td * DT
    v += a * DT
    v = max(min(v, MAX_SPEED), MIN_SPEED)
    return x, y, v, yaw


def ego_series(T, first, spawn, ends, control, plan):
    """One ego: rec [N][7], flags [N], plan_oa / plan_od [N][T], plan_status [N].  control(k, v) -> (a, delta) drives tick k; plan(k)
    -> (oa [T], od [T], status) is what the controller holds at the start of tick k; ends: {tick: flag}; behind an end the ego stands
    at `spawn`."""
    rec, flags = np.zeros((N, 7)), np.zeros(N, dtype=np.int32)
    oa, od, st = np.zeros((N, T)), np.zeros((N, T)), np.zeros(N, dtype=np.int32)
    x, y, v, yaw = first
    for k in range(N):
        oa[k], od[k], st[k] = plan(k)
        a, d = control(k, v)
        x, y, v, yaw = plant_step(x, y, v, yaw, a, d)
        rec[k] = (x, y, yaw, v, d, a, 0.0)
        if st[k] != 0:
            flags[k] |= FAILED
        if k in ends:
            flags[k] |= ends[k]
            x, y, v, yaw = spawn
    return rec, flags, oa, od, st


def followed(T, accel_ticks=10):
    """A plan followed exactly at heading 0: a = 0.5 on the first ticks, then constant speed; element j of tick k's plan is the input
    of tick k + j - 1."""
    u = lambda k: (0.5 if 0 <= k < accel_ticks else 0.0, 0.0)
    plan = lambda k: (np.array([u(k + j - 1)[0] for j in range(T)]), np.zeros(T), 0)
    return ((-90.0, -12.0, 2.0, 0.0), (-90.0, -12.0, 2.0, 0.0), {}, lambda k, v: u(k), plan)


def late(T, spawn, control, plan, status=0):
    """A row that stands still under an all-zero plan until its AGE end on tick WAKE - 1 and then drives from `spawn`."""
    first = (40.0 + spawn[0], -60.0 + spawn[1], 0.0, spawn[3])
    idle = (np.zeros(T), np.zeros(T), status)
    return (first, spawn, {WAKE - 1: AGE}, lambda k, v: control(k, v) if k >= WAKE else (0.0, 0.0), lambda k: plan(k) if k >= WAKE else idle)


def smooth(T, k, a_scale, d_scale):
    """A plan as a solve leaves it: slowly varying, and another one on every tick."""
    j = np.arange(T)
    return a_scale * np.sin(0.37 * j + 0.11 * k), d_scale * np.sin(0.21 * j + 0.07 * k + 1.0)


def rows(T):
    """The group of horizon T as ego_series arguments."""
    out = [followed(T)]
    turning = late(T, (3.0, 4.0, 4.0, 0.4), lambda k, v: (0.1, ramp(k, WAKE, WAKE + 25, -0.1, 0.25)), lambda k: (*smooth(T, k, 1.2, 0.3), 0))
    if T != 13:
        return out + [turning]

    def braking(k):                                                     # v = 5: five steps of -5 * 0.2 and it stands
        oa = np.zeros(T)
        oa[1:6] = -5.0
        return oa, np.zeros(T), 0
    out.append(((-10.0, 0.0, 5.0, 0.0), (-10.0, 0.0, 5.0, 0.0), {}, lambda k, v: (0.0, 0.0), braking))
    for i, ends in enumerate(({62: GOAL, 127: AGE}, {63: GOAL, 128: AGE}, {64: GOAL, 129: AGE})):
        burst = lambda k: (np.full(T, 0.3) if 118 <= k < 124 else np.zeros(T), np.zeros(T), 0)
        out.append(((-5.0, 20.0 + 3.0 * i, 2.5, 0.0), (-400.0, 50.0 + 3.0 * i, 2.5, 0.0), ends, lambda k, v: (0.0, 0.0), burst))
    od = np.array([0.2, 1.2, -1.1, 0.9, -0.95, 0.3, 0.79, -0.79, 2.0, -2.0, 0.1, 0.5, 1.0])
    out.append(late(T, (0.0, 0.0, 3.5, 0.7), lambda k, v: (0.0, 0.1), lambda k: (0.3 * smooth(T, k, 1.0, 0.0)[0], np.roll(od, k % 3), 0)))
    out.append(late(T, (5.0, 5.0, 7.5, 0.2), lambda k, v: (0.0, 0.05), lambda k: (np.full(T, 2.0), smooth(T, k, 0.0, 0.2)[1], 0)))
    out.append(late(T, (5.0, -5.0, -4.3, 3.3), lambda k, v: (0.0, -0.05), lambda k: (np.full(T, -3.0), smooth(T, k, 0.0, 0.2)[1], 0)))
    out.append(late(T, (-8.0, 2.0, 4.5, -0.6), lambda k, v: (0.05, ramp(k, WAKE, WAKE + 25, 0.05, 0.4)), lambda k: (*smooth(T, k, 1.5, 0.3), 1), status=1))
    out.append(late(T, (9.0, -9.0, 2.5, 1.9), lambda k, v: (0.05, 1.3), lambda k: (*smooth(T, k, 1.5, 0.3), 2), status=2))
    return out


def recorder_arrays(T):
    """The group of horizon T: rec [N][B][7], flags [N][B], x_first, x_spawn [B][4], plan_oa, plan_od [N][B][T], plan_status [N][B]."""
    R = rows(T)
    S = [ego_series(T, *r) for r in R]
    stack = lambda i: np.ascontiguousarray(np.stack([s[i] for s in S], axis=1))
    return {"rec": stack(0), "flags": stack(1), "plan_oa": stack(2), "plan_od": stack(3), "plan_status": stack(4),
            "x_first": np.array([r[0] for r in R]), "x_spawn": np.array([r[1] for r in R])}


KEYS = ("rec", "flags", "x_first", "x_spawn", "plan_oa", "plan_od", "plan_status")


def digest(groups):
    """groups: {T: recorder_arrays(T)}."""
    return hashlib.sha256(b"".join(np.ascontiguousarray(groups[T][k]).tobytes() for T in HORIZONS for k in KEYS)).hexdigest()


def all_groups():
    return {T: recorder_arrays(T) for T in HORIZONS}


def cached(predictor):
    """predictor(state, oa, od, status, delta_last, n_steps, dt, L) rolled out once per input to 64 samples: a shorter prediction is
    its first samples."""
    memo = {}

    def call(state, oa, od, status, delta_last, n_steps, dt, L):
        key = b"".join(np.asarray(a, dtype=np.float64).tobytes() for a in (state, oa, od, [status, delta_last]))
        if key not in memo:
            memo[key] = predictor(state, oa, od, status, delta_last, 64, dt, L)
        return memo[key][:n_steps]
    return call


def restate(A, n, n_steps, predictor=None, tol=TOL):
    """One group's rows on the first n ticks."""
    return PPN.eval_plan_predictions(A["rec"], A["flags"], A["x_first"], A["x_spawn"], A["plan_oa"], A["plan_od"], A["plan_status"], n_steps,
                                     tol, DT, L_CAR, n=n, predictor=predictor or cached(PPN.predict))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8) if a.size else a, b.view(np.uint8) if b.size else b)


def pack(results):
    """What the fixture stores of results {(T, n, n_steps): eval_plan_predictions' dict}: per T and n_steps the outputs of the longest
    cut in full; of the shorter cuts step_cnt (one after the other, T-major, then n_steps, then the cut) and of pt_i / pt_d only the
    slots (T, n_steps, cut, tick, row) that differ from the longest cut's -- the ticks whose horizon the cut shortens."""
    out = {}
    top = max(TICK_COUNTS)
    where, cut_i, cut_d, cut_cnt = [], [], [], []
    for T in HORIZONS:
        for S in STEPS:
            full = results[T, top, S]
            for k in ("pt_i", "pt_d", "step_sum", "step_cnt"):
                out[f"T{T}_s{S}_{k}"] = full[k].astype(np.int8) if k == "pt_i" else full[k].astype(np.int16) if k == "step_cnt" else full[k]
            for n in TICK_COUNTS[:-1]:
                r = results[T, n, S]
                for k in range(n):
                    for v in range(r["pt_i"].shape[1]):
                        if not (same_bits(r["pt_i"][k, v], full["pt_i"][k, v]) and same_bits(r["pt_d"][k, v], full["pt_d"][k, v])):
                            where.append((T, S, n, k, v)); cut_i.append(r["pt_i"][k, v]); cut_d.append(r["pt_d"][k, v])
                cut_cnt.append(r["step_cnt"].reshape(-1))
    out["cut_where"] = np.array(where, dtype=np.int16).reshape(-1, 5)
    out["cut_pt_i"], out["cut_pt_d"] = np.array(cut_i, dtype=np.int8).reshape(-1, 3), np.array(cut_d).reshape(-1, 6)
    out["cut_step_cnt"] = np.concatenate(cut_cnt).astype(np.int16)
    return out


def fixture():
    g = np.load(FIXTURE)
    assert str(g["digest"]) == digest(all_groups()), "tests/plan_prediction_cases.py no longer makes the inputs of plan_predictions.npz"
    return g


def expected(g, T, n, S):
    """pt_i [n][B][3], pt_d [n][B][6], step_cnt [B][S] (and, of the longest cut, step_sum) of group T cut to n ticks at n_steps = S, from
    the fixture."""
    top = max(TICK_COUNTS)
    pt_i, pt_d = g[f"T{T}_s{S}_pt_i"][:n].astype(np.int32), g[f"T{T}_s{S}_pt_d"][:n].copy()
    if n == top:
        return {"pt_i": pt_i, "pt_d": pt_d, "step_sum": g[f"T{T}_s{S}_step_sum"], "step_cnt": g[f"T{T}_s{S}_step_cnt"].astype(np.int32)}
    w = g["cut_where"].astype(np.int64)
    mine = (w[:, 0] == T) & (w[:, 1] == S) & (w[:, 2] == n)
    pt_i[w[mine, 3], w[mine, 4]] = g["cut_pt_i"][mine]
    pt_d[w[mine, 3], w[mine, 4]] = g["cut_pt_d"][mine]
    at = 0
    for t in HORIZONS:
        B = g[f"T{t}_s{STEPS[0]}_pt_i"].shape[1]
        for s in STEPS:
            for m in TICK_COUNTS[:-1]:
                if (t, s, m) == (T, S, n):
                    return {"pt_i": pt_i, "pt_d": pt_d, "step_cnt": g["cut_step_cnt"][at:at + B * s].reshape(B, s).astype(np.int32)}
                at += B * s
    raise KeyError((T, n, S))
