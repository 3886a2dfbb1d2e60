"""jsim_loop_eval_headway restated with plain numpy and Python, one ego and tick at a time, operation for
operation: the same unfused sums in the same order, the same comparisons.  The projection of a circle centre is
tracking_numpy.project's (idx, seg, s, d) with the path's yaw interpolated at the same foot; the vehicle list is
conflicts_numpy.vehicle_list's; the sum of the episode mean uses math.fsum.  Besides the outputs it returns what the cases'
condition() needs: per tick and place the circle centres (`centres` [n][B][9][2][2]: the ego in row 0, place i in row 1 + i; front,
rear; x, y), their nearest indices (`idx` [n][B][9][2]) and the margin of every discrete choice --
  m_idx, m_seg [n][B][9]: the smaller of the two centres' tracking_numpy margins;
  m_gap [n][B][8]: min(|V.lo - E.hi|, |V.hi - E.lo|), how far the place is from changing between ahead, alongside and behind;
  m_on [n][B][8]: | |lat| - (thr + margin) |;
  m_lead, m_ttc [n][B]: the difference between the smallest and the second smallest candidate of the tick's leader / of its
    time to collision (inf with fewer than two candidates, 0 on an exact tie; two +inf tie);
-- NaN where there is nothing to choose."""
import math

import numpy as np

import tracking_numpy as TN
from conflicts_numpy import MAX_OBS, vehicle_list
from recorder_numpy import episode_starts

NI, ND = 7, 4                                          # JSIM_HW_NI, JSIM_HW_ND
INF, NAN = math.inf, math.nan


def start_states(rec, flags, x_first, x_spawn):
    """[n][B][4]: every ego's (x, y, yaw, v) at the start of every tick: x_first at tick 0, x_spawn behind a record that ended an
    episode, else the record before (x_first / x_spawn are x, y, v, yaw; a record is x, y, yaw, v, ...)."""
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    st = np.empty((n, B, 4))
    if n:
        st[0] = np.asarray(x_first, dtype=np.float64).reshape(B, 4)[:, [0, 1, 3, 2]]
        st[1:] = rec[:-1, :, :4]
        s = episode_starts(np.asarray(flags).reshape(n, B))
        st[s] = np.broadcast_to(np.asarray(x_spawn, dtype=np.float64).reshape(B, 4)[:, [0, 1, 3, 2]], (n, B, 4))[s]
    return st


def centre(x, y, yaw, cc):
    return x + math.cos(yaw) * cc, y + math.sin(yaw) * cc


def project(cx, cy, path, arc):
    """(idx, s, d, ref, margin_idx, margin_seg) of one centre on one path of at least one point."""
    idx, seg, s, d, _, m_idx, m_seg = TN.project(cx, cy, 0.0, path, arc)
    if len(path) == 1:
        return idx, s, d, float(path[0, 2]), m_idx, m_seg
    t = TN.foot(float(path[seg, 0]), float(path[seg, 1]), float(path[seg + 1, 0]), float(path[seg + 1, 1]), cx, cy)[0]
    y0 = float(path[seg, 2])
    return idx, s, d, y0 + t * (float(path[seg + 1, 2]) - y0), m_idx, m_seg


def project_at(idx, cx, cy, path, arc):
    """(s, d) of one centre from a nearest index that is given (the fixture's: the reference's own calc_nearest_index): the segment
    rule restated -- of the segments idx - 1 and idx the one with the smaller residual, the lower on a tie."""
    n = len(path)
    px, py = path[:, 0].tolist(), path[:, 1].tolist()
    if n == 1:
        rx, ry = cx - px[0], cy - py[0]
        return 0.0, math.sqrt(rx * rx + ry * ry)
    cand = [j for j in (idx - 1, idx) if 0 <= j <= n - 2]
    feet = [TN.foot(px[j], py[j], px[j + 1], py[j + 1], cx, cy) for j in cand]
    pick = 1 if len(cand) == 2 and feet[1][1] < feet[0][1] else 0
    seg = cand[pick]
    t, q, ux, uy = feet[pick]
    cross = ux * (cy - py[seg]) - uy * (cx - px[seg])
    a0 = float(arc[seg])
    root = math.sqrt(q)
    return a0 + t * (float(arc[seg + 1]) - a0), root if cross >= 0.0 else -root


def gap_lat_from(centres, idx, path, arc, r_e, r_i):
    """(gap, lat) of one place from the circle centres [2][2][2] (ego, vehicle; front, rear; x, y) and their nearest indices [2][2]."""
    (esf, _), (esr, _) = (project_at(int(idx[0][c]), float(centres[0][c][0]), float(centres[0][c][1]), path, arc) for c in (0, 1))
    (vsf, df), (vsr, dr) = (project_at(int(idx[1][c]), float(centres[1][c][0]), float(centres[1][c][1]), path, arc) for c in (0, 1))
    e_lo, e_hi = min(esf, esr) - r_e, max(esf, esr) + r_e
    v_lo, v_hi = min(vsf, vsr) - r_i, max(vsf, vsr) + r_i
    ahead, behind = v_lo - e_hi, v_hi - e_lo
    return (ahead if ahead > 0.0 else (behind if behind < 0.0 else 0.0)), (dr if abs(dr) < abs(df) else df)


def _two_smallest(vals):
    """The difference between the smallest and the second smallest of a list (inf with fewer than two; two +inf: 0)."""
    v = sorted(vals)
    if len(v) < 2:
        return INF
    return 0.0 if v[0] == v[1] else v[1] - v[0]


def _minimum(series):
    """(value, first index) of the smallest entry that is not NaN, strictly: the first occurrence stays; (NaN, -1) without one."""
    best, at = NAN, -1
    for j, v in enumerate(series):
        if v == v and (best != best or v < best):
            best, at = v, j
    return best, at


def eval_headway(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, path_id, paths, margin=0.0):
    """rec [n][B][7], flags [n][B], obs [n][n_obs][6] or None, x_first / x_spawn [B][4], veh_range / mate_range [B][2], shapes
    [n_obs][>= 3] (cc_front, cc_rear, radius) or None (the ego's shape), ego_shape (cc_front, cc_rear, radius), path_id [B], paths: a
    list of (M, >= 3) arrays.  Returns the outputs of jsim_loop_eval_headway under their names and the margins of the module's
    docstring."""
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    n_obs = 0 if obs is None else np.shape(obs)[1]
    obs = None if obs is None else np.asarray(obs, dtype=np.float64)
    ego_shape = tuple(float(v) for v in ego_shape)
    rows = None if shapes is None else np.asarray(shapes, dtype=np.float64).reshape(n_obs, -1)[:, :3]
    paths = [np.asarray(p, dtype=np.float64) for p in paths]
    arcs = [TN.arc_lengths(p) for p in paths]
    st = start_states(rec, flags, x_first, x_spawn)
    margin = float(margin)
    cc_f, cc_r, r_e = ego_shape

    out = {"lead": np.full((n, B), -1, dtype=np.int32), "ttc_who": np.full((n, B), -1, dtype=np.int32),
           "ep_i": np.full((n, B, NI), -1, dtype=np.int32), "ep_d": np.full((n, B, ND), NAN),
           "centres": np.full((n, B, 1 + MAX_OBS, 2, 2), NAN), "idx": np.full((n, B, 1 + MAX_OBS, 2), -1, dtype=np.int32),
           "m_idx": np.full((n, B, 1 + MAX_OBS), NAN), "m_seg": np.full((n, B, 1 + MAX_OBS), NAN)}
    for k in ("lead_gap", "thw", "ttc", "u_ego", "m_lead", "m_ttc"):
        out[k] = np.full((n, B), NAN)
    for k in ("gap", "lat", "rate", "ttc_i", "m_gap", "m_on"):
        out[k] = np.full((n, B, MAX_OBS), NAN)

    def both(x, y, yaw, shape, path, arc, slot):
        """Front and rear centre of a pose projected: (s_front, s_rear, d_front, d_rear, ref_front); notes centres, idx, margins."""
        res = []
        for c, cc in enumerate(shape[:2]):
            cx, cy = centre(x, y, yaw, cc)
            res.append(project(cx, cy, path, arc))
            out["centres"][slot + (c,)] = (cx, cy)
            out["idx"][slot + (c,)] = res[-1][0]
        out["m_idx"][slot] = min(res[0][4], res[1][4])
        out["m_seg"][slot] = min(res[0][5], res[1][5])
        return res[0][1], res[1][1], res[0][2], res[1][2], res[0][3]

    for b in range(B):
        p = int(path_id[b])
        path, arc = (paths[p], arcs[p]) if 0 <= p < len(paths) else (np.zeros((0, 3)), np.zeros(0))
        lst = vehicle_list(b, B, n_obs, np.asarray(veh_range).reshape(B, 2), np.asarray(mate_range).reshape(B, 2))
        if not lst or len(path) == 0:
            lst = []
        for k in range(n):
            ex, ey, eyaw, ev = st[k, b].tolist()
            if not lst or not all(math.isfinite(v) for v in (ex, ey, eyaw, ev)):
                continue
            sf, sr, _, _, ref = both(ex, ey, eyaw, ego_shape, path, arc, (k, b, 0))
            e_lo, e_hi = min(sf, sr) - r_e, max(sf, sr) + r_e
            u_e = ev * math.cos(eyaw - ref)
            out["u_ego"][k, b] = u_e
            lead, lead_gap, ttc, ttc_who = -1, NAN, NAN, -1
            lead_c, ttc_c = [], []
            for i, (kind, j) in enumerate(lst):
                if kind == "veh":
                    x, y, v, yaw = obs[k, j, :4].tolist()
                    shape = ego_shape if rows is None else tuple(rows[j].tolist())
                else:
                    x, y, yaw, v = st[k, j].tolist()
                    shape = ego_shape
                if not all(math.isfinite(w) for w in (x, y, yaw, v)):
                    continue
                sf, sr, df, dr, ref = both(x, y, yaw, shape, path, arc, (k, b, 1 + i))
                r_i = shape[2]
                v_lo, v_hi = min(sf, sr) - r_i, max(sf, sr) + r_i
                ahead, behind = v_lo - e_hi, v_hi - e_lo
                gap = ahead if ahead > 0.0 else (behind if behind < 0.0 else 0.0)
                lat = dr if abs(dr) < abs(df) else df
                rate = v * math.cos(yaw - ref) - u_e
                thr = r_e + r_i
                on = abs(lat) <= thr + margin
                t = NAN
                if on:
                    if gap == 0.0:
                        t = 0.0
                    elif gap > 0.0:
                        t = gap / -rate if rate < 0.0 else INF
                    else:
                        t = -gap / rate if rate > 0.0 else INF
                out["gap"][k, b, i], out["lat"][k, b, i], out["rate"][k, b, i], out["ttc_i"][k, b, i] = gap, lat, rate, t
                out["m_gap"][k, b, i], out["m_on"][k, b, i] = min(abs(ahead), abs(behind)), abs(abs(lat) - (thr + margin))
                if on and gap >= 0.0:
                    lead_c.append(gap)
                    if lead < 0 or gap < lead_gap:
                        lead, lead_gap = i, gap
                if t == t:
                    ttc_c.append(t)
                    if ttc_who < 0 or t < ttc:
                        ttc_who, ttc = i, t
            out["lead"][k, b], out["lead_gap"][k, b], out["ttc"][k, b], out["ttc_who"][k, b] = lead, lead_gap, ttc, ttc_who
            out["m_lead"][k, b], out["m_ttc"][k, b] = _two_smallest(lead_c), _two_smallest(ttc_c)
            if lead >= 0:
                out["thw"][k, b] = 0.0 if lead_gap == 0.0 else (lead_gap / u_e if u_e > 0.0 else INF)
        for k0, k1 in TN.episodes_of(flags[:, b]):
            ticks = range(k0, k1 + 1)
            g, g_at = _minimum([float(out["lead_gap"][k, b]) for k in ticks])
            h, h_at = _minimum([float(out["thw"][k, b]) for k in ticks])
            t, t_at = _minimum([float(out["ttc"][k, b]) for k in ticks])
            fin = [float(out["thw"][k, b]) for k in ticks if math.isfinite(out["thw"][k, b])]
            at = lambda j: k0 + j if j >= 0 else -1
            out["ep_i"][k0, b] = (k1 - k0 + 1, int(sum(out["lead"][k, b] >= 0 for k in ticks)), at(g_at),
                                  out["lead"][k0 + g_at, b] if g_at >= 0 else -1, at(h_at), at(t_at),
                                  out["ttc_who"][k0 + t_at, b] if t_at >= 0 else -1)
            out["ep_d"][k0, b] = (g, h, t, math.fsum(fin) / len(fin) if fin else NAN)
    return out
