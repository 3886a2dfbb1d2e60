"""jsim_loop_eval_tracking restated with plain numpy and Python, operation for operation: the same unfused
sums in the same order, the same comparisons.  The sums of the episode means use math.fsum.  Besides the outputs it returns, for
every tick, the margin of each discrete choice: margin_idx = the gap between the two smallest squared distances (inf on a path of
one point), margin_seg = |q_a - q_b| relative to their larger value (0 when both are 0, inf with one candidate segment).  -1 / NaN
margins where the pose has no projection."""
import math

import numpy as np

GOAL, AGE = 2, 4
TWO_PI = 6.283185307179586
PI = 3.141592653589793
NI, ND = 2, 5                                          # JSIM_TRK_NI, JSIM_TRK_ND


def arc_lengths(path):
    """arc[i + 1] = arc[i] + sqrt(dx * dx + dy * dy), one after the other."""
    arc = [0.0]
    for i in range(len(path) - 1):
        dx, dy = float(path[i + 1][0]) - float(path[i][0]), float(path[i + 1][1]) - float(path[i][1])
        arc.append(arc[-1] + math.sqrt(dx * dx + dy * dy))
    return np.array(arc)


def episodes_of(flags_b):
    """(first tick, last tick) of every episode with a tick: an end flag closes one, the last record closes the running one."""
    out, k0, n = [], 0, len(flags_b)
    for k in range(n):
        if (int(flags_b[k]) & (GOAL | AGE)) or k == n - 1:
            out.append((k0, k))
            k0 = k + 1
    return out


def pymod(a, b):
    r = math.fmod(a, b)
    if r != 0.0 and r < 0.0:
        r += b
    return r


def foot(ax, ay, bx, by, x, y):
    ux, uy = bx - ax, by - ay
    L2 = ux * ux + uy * uy
    t = 0.0
    if L2 != 0.0:
        t = ((x - ax) * ux + (y - ay) * uy) / L2
        t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
    rx, ry = x - (ax + t * ux), y - (ay + t * uy)
    return t, rx * rx + ry * ry, ux, uy


def project(x, y, yaw, path, arc):
    """One pose on one path: (idx, seg, s, d, e_yaw, margin_idx, margin_seg)."""
    n = len(path)
    if n < 1 or not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
        return -1, -1, math.nan, math.nan, math.nan, math.nan, math.nan
    dx, dy = path[:, 0] - x, path[:, 1] - y
    d2 = dx * dx + dy * dy
    idx = int(np.argmin(d2))                           # the first occurrence of the minimum
    two = np.partition(d2, 1)[:2] if n > 1 else d2
    m_idx = float(two[1] - two[0]) if n > 1 else math.inf
    px, py = path[:, 0].tolist(), path[:, 1].tolist()
    if n == 1:
        rx, ry = x - px[0], y - py[0]
        seg, t, q, cross, m_seg = 0, 0.0, rx * rx + ry * ry, 0.0, math.inf
        s, ref = 0.0, float(path[0, 2])
    else:
        cand = [j for j in (idx - 1, idx) if 0 <= j <= n - 2]
        feet = [foot(px[j], py[j], px[j + 1], py[j + 1], x, y) for j in cand]
        pick = 0
        m_seg = math.inf
        if len(cand) == 2:
            qa, qb = feet[0][1], feet[1][1]
            pick = 1 if qb < qa else 0                 # the lower segment on a tie
            m_seg = abs(qa - qb) / max(qa, qb) if max(qa, qb) > 0.0 else 0.0
        seg = cand[pick]
        t, q, ux, uy = feet[pick]
        cross = ux * (y - py[seg]) - uy * (x - px[seg])
        a0, y0 = float(arc[seg]), float(path[seg, 2])
        s = a0 + t * (float(arc[seg + 1]) - a0)
        ref = y0 + t * (float(path[seg + 1, 2]) - y0)
    root = math.sqrt(q)
    d = root if cross >= 0.0 else -root
    e_yaw = pymod((yaw - ref) + PI, TWO_PI) - PI
    return idx, seg, s, d, e_yaw, m_idx, m_seg


def eval_tracking(rec, flags, path_id, paths):
    """rec [n][B][>= 3] (x, y, yaw of tick k in the first three columns), flags [n][B], path_id [B], paths: a list of (M, >= 3)
    arrays.  Returns idx, seg (int32), s, d, e_yaw [n][B], ep_i [n][B][2] (int32), ep_d [n][B][5], arc (a list), margin_idx,
    margin_seg [n][B]."""
    rec, flags = np.asarray(rec, dtype=np.float64), np.asarray(flags)
    n, B = flags.shape
    paths = [np.asarray(p, dtype=np.float64) for p in paths]
    arcs = [arc_lengths(p) for p in paths]
    idx, seg = np.full((n, B), -1, dtype=np.int32), np.full((n, B), -1, dtype=np.int32)
    s, d, e_yaw, m_idx, m_seg = (np.full((n, B), np.nan) for _ in range(5))
    ep_i, ep_d = np.full((n, B, NI), -1, dtype=np.int32), np.full((n, B, ND), np.nan)
    for b in range(B):
        p = int(path_id[b])
        have = 0 <= p < len(paths)
        path, arc = (paths[p], arcs[p]) if have else (np.zeros((0, 3)), np.zeros(0))
        for k in range(n):
            x, y, yaw = rec[k, b, :3].tolist()
            idx[k, b], seg[k, b], s[k, b], d[k, b], e_yaw[k, b], m_idx[k, b], m_seg[k, b] = project(x, y, yaw, path, arc)
        for k0, k1 in episodes_of(flags[:, b]):
            dmax, tick, ymax, sq = math.nan, -1, math.nan, []
            for k in range(k0, k1 + 1):
                dk, yk = float(d[k, b]), float(e_yaw[k, b])
                if dk == dk:
                    sq.append(dk * dk)
                    if dmax != dmax or abs(dk) > dmax:  # strictly: the first occurrence stays
                        dmax, tick = abs(dk), k
                if yk == yk and (ymax != ymax or abs(yk) > ymax):
                    ymax = abs(yk)
            ep_i[k0, b] = (k1 - k0 + 1, tick)
            ep_d[k0, b] = (dmax, math.fsum(sq) / len(sq) if sq else math.nan, ymax, s[k0, b], s[k1, b])
    return {"idx": idx, "seg": seg, "s": s, "d": d, "e_yaw": e_yaw, "ep_i": ep_i, "ep_d": ep_d, "arc": arcs,
            "margin_idx": m_idx, "margin_seg": m_seg}
