"""jsim_loop_score_predictions (include/jsim_mpc.h) restated in numpy / math, in the rule's order: the
prediction of every recorded tick -- MovingObstaclesPrediction's recurrence (main/lib/moving_obstacles_prediction.py:21-47) from the
tuple the loop predicted from -- against the recorded poses of the ticks that followed.  Rows: the recorded vehicles, then (egos) the
egos under the constant rule.  Python floats and math's cos / sin / tan: the libm the reference itself calls."""
import math

import numpy as np

GOAL, AGE = 2, 4
PS_INT, PS_DOUBLE = ("n", "hold", "max_at"), ("ade", "fde", "max", "lon", "lat", "yaw")
PI = 3.141592653589793


def predict(tup, L, dt, n_steps):
    """The samples (x, y, yaw) [n_steps][3] of the prediction from tup = (x, y, v, yaw, a, steer)."""
    x, y, v, yaw, a, steer = (float(t) for t in tup)
    tn = math.tan(steer)
    out = np.empty((n_steps, 3))
    for j in range(n_steps):
        x += v * math.cos(yaw) * dt
        y += v * math.sin(yaw) * dt
        v += a * dt
        yaw += (v / L) * tn * dt
        out[j] = (x, y, yaw)
    return out


def ego_inputs(rec, flags, x_first, x_spawn):
    """[n][B][6]: every ego's tuple (x, y, v, yaw, 0, steer) at the start of every tick -- x_first on tick 0, x_spawn behind a record
    that ended an episode, else the record before; steer = that record's delta, 0 on tick 0 and behind an end."""
    n, B = flags.shape
    out = np.zeros((n, B, 6))
    for k in range(n):
        for b in range(B):
            if k == 0:
                out[k, b, :4] = x_first[b]
            elif flags[k - 1, b] & (GOAL | AGE):
                out[k, b, :4] = x_spawn[b]
            else:
                r = rec[k - 1, b]
                out[k, b] = (r[0], r[1], r[3], r[2], 0.0, r[4])
    return out


def ego_horizon(flags_b, k):
    """ke(k): the first tick >= k whose record ends an episode, or the last tick."""
    n = len(flags_b)
    for t in range(k, n):
        if flags_b[t] & (GOAL | AGE):
            return t
    return n - 1


def score(samples, truth, m, tol):
    """One tick of one row: samples [n_steps][3] (x, y, yaw) against truth [>= m][3] -> (pt_i row, pt_d row, e [n_steps])."""
    S = len(samples)
    e = np.full(S, np.nan)
    if m == 0:
        return (0, 0, -1), (np.nan,) * 6, e
    dxs, dys = samples[:m, 0] - truth[:m, 0], samples[:m, 1] - truth[:m, 1]
    e[:m] = np.sqrt(dxs * dxs + dys * dys)
    total = float(np.cumsum(e[:m])[-1])                              # e_0 + e_1 + ... in step order
    over = np.flatnonzero(~(e[:m] <= tol))
    hold = int(over[0]) if over.size else m
    max_at = int(np.argmax(e[:m]))                                   # the first of the largest
    mx, dx, dy = float(e[max_at]), float(dxs[m - 1]), float(dys[m - 1])
    psi = float(truth[m - 1, 2])
    lon = dx * math.cos(psi) + dy * math.sin(psi)
    lat = -dx * math.sin(psi) + dy * math.cos(psi)
    yaw = ((float(samples[m - 1, 2]) - psi) + PI) % 6.283185307179586 - PI      # Python's float %, as the device's jpl_pymod
    return (m, hold, max_at), (total / m, e[m - 1], mx, lon, lat, yaw), e


def eval_predictions(rec, flags, obs, x_first, x_spawn, egos, n_steps, tol, dt, L_obs, L_ego, n=None, predictor=predict):
    """The entry point on the first n ticks.  obs [N][n_obs][6] or None; L_obs [n_obs]: each vehicle's wheelbase; predictor(tup, L,
    dt, n_steps) -> samples [n_steps][3].  Returns pt_i [n][V][3] int32, pt_d [n][V][6], step_sum [V][n_steps], step_cnt int32, err
    [n][V][n_steps]."""
    n = flags.shape[0] if n is None else n
    B = flags.shape[1]
    n_obs = 0 if obs is None else obs.shape[1]
    V = n_obs + (B if egos else 0)
    rec, flags = rec[:n], flags[:n]
    pt_i, pt_d = np.zeros((n, V, 3), dtype=np.int32), np.full((n, V, 6), np.nan)
    err = np.full((n, V, n_steps), np.nan)
    inputs = ego_inputs(rec, flags, x_first, x_spawn) if egos and n else None
    for r in range(V):
        for k in range(n):
            if r < n_obs:
                tup, L = obs[k, r], L_obs[r]
                m = min(n_steps, n - 1 - k)
                truth = obs[k + 1:k + 1 + m, r][:, [0, 1, 3]]
            else:
                b = r - n_obs
                tup, L = inputs[k, b], L_ego
                m = min(n_steps, ego_horizon(flags[:, b], k) - k + 1)
                truth = rec[k:k + m, b, :3]
            pt_i[k, r], pt_d[k, r], err[k, r] = score(predictor(tup, L, dt, n_steps), truth, m, tol)
    scored = ~np.isnan(err)
    step_cnt = scored.sum(axis=0).astype(np.int32)
    step_sum = np.cumsum(np.where(scored, err, 0.0), axis=0)[-1] if n else np.zeros((V, n_steps))   # (cumsum adds in tick order)
    return {"pt_i": pt_i, "pt_d": pt_d, "step_sum": step_sum, "step_cnt": step_cnt, "err": err}
