"""Numpy restatement of the stakeholder-reasons scoring of candidate trajectories, written from the
contract and used by the tests as the CPU side of jsim_score_trajectories: resample each candidate by the ego's reachable
speed, time it, predict the cyclist for that long, score every sample for the policymaker, the driver and the cyclist, average,
and weigh the averages per weight row.  Sequential quantities (cumulative sums, the completion time, the two in-range timers)
are accumulated in index order; the means are numpy's."""
import numpy as np

# order of a situation's parameter row (JSIM_REASON_* of include/jsim_mpc.h)
PAR_NAMES = ("dt", "max_accel", "max_speed", "centerline", "width", "ref_d", "buf_d", "thr_d", "ref_c", "buf_c", "thr_c", "wheelbase")
DEFAULT_PAR = np.array([0.1, 2.0, 30.0 / 3.6, 0.0, 2.0, 10.0, 2.0, 8.0, 8.0, 2.0, 5.0, 1.0])
MAX_RES = 320
MAX_CAND = 8
MAX_STEPS = 65536
IDEAL = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)


def resample_step(n, mode, v, par):
    """dl per raw point (mode 0 below MAX_SPEED) or one number."""
    dt, a, vmax = par[0], par[1], par[2]
    if mode == 1:
        return dt * v
    if v < vmax:
        return dt * np.minimum(np.cumsum(np.full(n, a)) + v, vmax)
    return dt * vmax


def resample_curve(P, dl):
    """Keep the points at which floor(arc length / dl) steps up, the first and the last."""
    P = np.asarray(P, dtype=np.float64)
    d = P[1:, :2] - P[:-1, :2]
    cum = np.cumsum(np.append(0.0, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])))
    k = np.floor(cum / dl)
    keep = np.append(True, (k[1:] - k[:-1]) >= 1.0)
    keep[-1] = True
    return P[keep].copy()


def completion_time(R, v, par):
    vel, ct = v, 0.0
    for k in range(1, len(R)):
        vel = min(vel + par[1], par[2])
        dx, dy = R[k, 0] - R[k - 1, 0], R[k, 1] - R[k - 1, 1]
        ct += np.sqrt(dx * dx + dy * dy) / vel
    return ct


def predict_cyclist(cyc, nb, dt, wheelbase):
    """Rows 0 .. nb - 1 of explicit Euler; row i = the state after i + 1 steps."""
    x, y, v, yaw, a, steer = (float(c) for c in cyc)
    out = np.empty((nb, 2))
    for i in range(nb):
        x += v * np.cos(yaw) * dt
        y += v * np.sin(yaw) * dt
        v += a * dt
        yaw += (v / wheelbase) * np.tan(steer) * dt
        out[i] = x, y
    return out


def _nan_candidate(status, m=0, ct=np.nan, R=None):
    return {"status": status, "n_samples": m, "ct": ct, "avg": np.full(4, np.nan), "resampled": R, "detail": None}


def resample_candidate(pts, mode, ego, par):
    """(status, R): status 2 for the inputs the reference has no defined behaviour for, 4 past the kernel's table."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    v = ego[3]
    if len(pts) < 2 or (mode == 1 and not v > 0.0):
        return 2, None
    dl = resample_step(len(pts), mode, v, par)
    if not np.all(np.asarray(dl) > 0.0):
        return 2, None
    R = resample_curve(pts, dl)
    if len(R) > MAX_RES:
        return 4, R
    if len(R) < 3:
        return 2, R
    return 0, R


def score_samples(R, ct, cyc, now, par):
    """Steps 4-7 for one resampled candidate and the completion time it is scored with."""
    dt, centre, width = par[0], par[3], par[4]
    rng_d, thr_d, rng_c, thr_c = par[5] + par[6], par[7], par[8] + par[9], par[10]
    m = len(R)
    if not np.isfinite(ct):
        return _nan_candidate(2, m, ct, R)
    nb = int(np.ceil(ct / dt))
    if nb < 2:
        return _nan_candidate(2, m, ct, R)
    if nb > MAX_STEPS:
        return _nan_candidate(4, m, ct, R)
    rows = predict_cyclist(cyc, nb - 1, dt, par[11])
    step = (nb - 2) / (m - 1)
    idx = np.floor(np.arange(m) * step).astype(np.int64)
    idx[-1] = nb - 2
    dx, dy = rows[idx, 0] - R[:, 0], rows[idx, 1] - R[:, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    d = R[:, 0] - width / 2 - centre
    pol = np.where(d >= 0.0, 1.0, np.exp(0.2 * np.minimum(d, 0.0)))
    in_d, in_c = dist < rng_d, dist < rng_c
    comfort = np.where(in_c, np.exp(0.2 * (dist - rng_c)), 1.0)
    drv, cyt = np.ones(m), np.ones(m)
    t_d, t_c = now[3], now[4]
    for j in range(m):
        if in_d[j]:
            t_d += dt
            if t_d >= thr_d:
                drv[j] = 1.0 / np.exp(0.2 * (t_d - thr_d))
        if in_c[j]:
            t_c += dt
            if t_c >= thr_c:
                cyt[j] = 1.0 / np.exp(0.2 * (t_c - thr_c))
    comb = comfort * cyt
    p, dr, cb = pol[:-1].copy(), drv[:-1].copy(), comb[:-1].copy()
    p[0], dr[0], cb[0] = now[0], now[1], now[2]
    avg = np.array([np.mean(p[:-1]), np.mean(p), np.mean(dr), np.mean(cb)])
    return {"status": 0, "n_samples": m, "ct": ct, "avg": avg, "resampled": R, "nb": nb, "cyc_idx": idx, "in_d": in_d, "in_c": in_c,
            "dist": dist, "detail": {"policymaker": p, "driver": dr, "cyclist_comfort": comfort, "cyclist_time": cyt, "cyclist_combined": cb}}


def balance_function(weights, ideal=None):
    n = len(weights)
    ideal = [1.0 / n] * n if ideal is None else list(ideal)
    ratio = min(w / i for w, i in zip(weights, ideal))
    ssd = 0.0
    for w, i in zip(weights, ideal):
        ssd = ssd + (w - i) * (w - i)
    si = 0.0
    for i in ideal:
        si = si + i * i
    return (1.0 - np.sqrt(ssd / n) / np.sqrt(si)) * ratio


def weigh(avg, status, w, form, ideal=IDEAL):
    """scores [C] and the first best candidate of one weight row; candidates with a status never win."""
    w_p, w_d, w_c = (float(x) for x in w)
    bal = balance_function([w_c, w_d, w_p], ideal)
    scores = np.full(len(avg), np.nan)
    best, top = -1, -np.inf
    for c in range(len(avg)):
        if status[c] != 0:
            continue
        s = bal * ((w_p * avg[c][1 if form else 0] + w_d * avg[c][2]) + w_c * avg[c][3])
        if form:
            s = max(0.0, min(s, 1.0))
        scores[c] = s
        if s > top:
            best, top = c, s
    return scores, best


def score_situation(cands, modes, time_from, ego, cyc, now, par=DEFAULT_PAR, weights=((1 / 9, 4 / 9, 4 / 9),), forms=(0,), ideal=IDEAL):
    """One situation: per candidate results (list of dicts), scores [W][C] and best [W]."""
    C = len(cands)
    pre = [resample_candidate(cands[c], modes[c], ego, par) for c in range(C)]
    cts = [completion_time(R, ego[3], par) if st == 0 else np.nan for st, R in pre]
    res = []
    for c in range(C):
        st, R = pre[c]
        donor = time_from[c]
        if st != 0:
            res.append(_nan_candidate(st, 0 if R is None else len(R), cts[c], R))
        elif pre[donor][0] != 0:
            res.append(_nan_candidate(2, len(R), np.nan, R))
        else:
            res.append(score_samples(R, cts[donor], cyc, now, par))
    status = [r["status"] for r in res]
    avg = [r["avg"] for r in res]
    scores = np.empty((len(weights), C))
    best = np.empty(len(weights), dtype=np.int32)
    for k, (w, f) in enumerate(zip(weights, forms)):
        scores[k], best[k] = weigh(avg, status, w, f, ideal)
    return res, scores, best


def default_layout(C):
    """The reference's list: planned candidates, the following one last with the time of the one before it."""
    if C == 0:
        return [], []
    modes = [0] * (C - 1) + [1]
    time_from = list(range(C - 1)) + [C - 2 if C > 1 else 0]
    return modes, time_from


def weight_triples(weight_step):
    """Every (policy, driver, cyclist) on the grid that sums to one, rounded as the reference rounds; sorted."""
    precision = max(int(-np.log10(weight_step)) + 2, 6)
    values = np.arange(0, 1.0 + weight_step / 2, weight_step)
    out = set()
    for p in values:
        for d in values:
            c = round(1.0 - p - d, precision)
            if 0 <= c <= 1.0 + 1e-9:
                out.add((round(round(p, precision), precision), round(round(d, precision), precision), round(c, precision)))
    return sorted(t for t in out if abs(t[0] + t[1] + t[2] - 1.0) <= 1e-6), precision


def table_rows(triples, scores, precision):
    """(policy_data, driver_data, cyclist_data) from the scores [W][C] of the form-1 rows."""
    groups = ([], [], [])
    for (p, d, c), row in zip(triples, scores):
        s = [0.0 if x < 0 else float(x) for x in row]
        top = max(s)
        if top > 1.0:
            s = [x / top for x in s]
            top = max(s)
        hit = [i for i, x in enumerate(s) if abs(x - top) < 0.000001]
        names = [f"Traj {i}" for i in hit[:4]]
        if len(names) == 1:
            label = names[0]
        elif len(names) == 2:
            label = f"{names[0]} and {names[1]}"
        else:
            label = ", ".join(names[:-1]) + f", and {names[-1]}"
        line = [p, d, c] + [s[i] if i < len(s) else 0.0 for i in range(4)] + [label]
        big = max(p, d, c)
        groups[0 if (big == p or (p == d and p == c)) else 1 if big == d else 2].append(line)
    key = ((0, 1), (1, 0), (2, 0))
    return tuple(sorted(g, key=lambda x, k=k: (round(x[k[0]], precision), round(x[k[1]], precision))) for g, k in zip(groups, key))
