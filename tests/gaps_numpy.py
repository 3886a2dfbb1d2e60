"""Numpy restatement of the time gap per recorded tick, written from the contract and used by the tests as
the CPU side of jsim_loop_eval_gaps: from a History recorder's arrays, every ego's pose at the start of every tick, its vehicles'
and group mates' poses (conflicts_numpy's list and circle centres), and for every (ego, tick k, vehicle i) the offset `off` of
smallest |off| <= window at which one of the four circle pairs of (ego at tick k, vehicle at tick k - off) touches, -o in front of
+o; from that `gap`, `who` per tick and `ep_gap`, `ep_tick`, `ep_who`, `ep_off` per episode.  within = 0 ("episode"): only vehicle
ticks of the ego's own episode count; within = 1 ("record"): every recorded tick does.  eval_gaps tries every offset of every tick
at once, eval_gaps_loops states the same with one Python loop per index and is what the first is checked against."""
import math

import numpy as np

from conflicts_numpy import circle_centres, vehicle_list
from recorder_numpy import episodes_of, start_poses

NONE = -128                                          # JSIM_GAP_NONE
MAX_WINDOW = 63                                      # JSIM_GAP_MAX_WINDOW
PLACES = 8                                           # JSIM_MAX_OBS
WITHIN = {"episode": 0, "record": 1}


def scan_order(window):
    """The offsets in the order they are tried: 0, -1, +1, -2, +2, ..."""
    return np.array([0] + [s * o for o in range(1, window + 1) for s in (-1, 1)], dtype=np.int64)


def _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, window, within):
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    n_obs = 0 if obs is None else np.shape(obs)[1]
    obs = None if obs is None else np.asarray(obs, dtype=np.float64)
    if int(window) != window or not 0 <= int(window) <= MAX_WINDOW:
        raise ValueError("window outside [0, 63]")
    if within not in (0, 1):
        raise ValueError("within is neither 0 nor 1")
    ego_shape = tuple(float(v) for v in ego_shape)
    rows = None if shapes is None else np.asarray(shapes, dtype=np.float64).reshape(n_obs, -1)[:, :3]
    pose = start_poses(rec, flags, x_first, x_spawn)
    lists = []
    for b in range(B):
        lst = []
        for kind, j in vehicle_list(b, B, n_obs, np.asarray(veh_range).reshape(B, 2), np.asarray(mate_range).reshape(B, 2)):
            if kind == "veh":
                lst.append((obs[:, j][:, [0, 1, 3]], ego_shape if rows is None else tuple(rows[j].tolist())))
            else:
                lst.append((pose[:, j], ego_shape))
        lists.append(lst)
    return n, B, flags, pose, lists, ego_shape, int(window)


def _empty(n, B):
    full = lambda v: np.full((n, B), v, dtype=np.int32)
    return {"off": np.full((n, B, PLACES), NONE, dtype=np.int8), "gap": full(-1), "who": full(-1), "ep_gap": full(-1), "ep_tick": full(-1),
            "ep_who": full(-1), "ep_off": full(NONE)}


def _finish(out, flags):
    """gap, who per tick and the four episode outputs from `off`."""
    off = out["off"].astype(np.int64)
    n, B = off.shape[:2]
    mag = np.where(off == NONE, 1 << 20, np.abs(off))
    who = np.argmin(mag, axis=2)                                                  # the lowest place on ties
    gap = np.take_along_axis(mag, who[:, :, None], axis=2)[:, :, 0]
    has = gap < (1 << 20)
    out["gap"][:] = np.where(has, gap, -1)
    out["who"][:] = np.where(has, who, -1)
    for b in range(B):
        for k0, k1 in episodes_of(flags[:, b]):
            g = np.where(has[k0:k1 + 1, b], gap[k0:k1 + 1, b], 1 << 20)
            if g.min() < (1 << 20):
                k = k0 + int(np.argmin(g))                                        # the first tick that has the smallest
                out["ep_gap"][k0, b], out["ep_tick"][k0, b], out["ep_who"][k0, b] = gap[k, b], k, who[k, b]
                out["ep_off"][k0, b] = off[k, b, who[k, b]]
    return out


def eval_gaps(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, window=20, within=0, stats=None):
    """rec [n][B][7], flags [n][B], obs [n][n_obs][6] or None, x_first / x_spawn [B][4], veh_range / mate_range [B][2], shapes
    [n_obs][>= 3] (cc_front, cc_rear, radius) or None (the ego's shape), ego_shape (cc_front, cc_rear, radius).
    Returns off [n][B][8] int8, gap, who, ep_gap, ep_tick, ep_who, ep_off [n][B] int32.  stats: a dict that receives `margin`, the
    smallest |dist - threshold| of any comparison the rule admits."""
    n, B, flags, pose, lists, ego_shape, W = _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, window, within)
    out = _empty(n, B)
    offs = scan_order(W)
    k = np.arange(n)
    kv = k[:, None] - offs[None, :]                                               # [n][2W + 1] the vehicle's tick
    for b in range(B):
        if not lists[b]:
            continue
        lo, hi = np.zeros(n, dtype=np.int64), np.full(n, n - 1, dtype=np.int64)
        if within == 0:
            for k0, k1 in episodes_of(flags[:, b]):
                lo[k0:k1 + 1], hi[k0:k1 + 1] = k0, k1
        ok = (kv >= lo[:, None]) & (kv <= hi[:, None])
        kvc = np.clip(kv, 0, n - 1)
        A = [circle_centres(pose[:, b], cc) for cc in ego_shape[:2]]             # [a][n][2]
        for i, (tr, sh) in enumerate(lists[b]):
            thr = ego_shape[2] + sh[2]                                            # the unfused sum
            touch = np.zeros(kv.shape, dtype=bool)
            for c in range(2):
                V = circle_centres(tr, sh[c])[kvc]                                # [n][2W + 1][2]
                for a in range(2):
                    dx, dy = A[a][:, None, 0] - V[..., 0], A[a][:, None, 1] - V[..., 1]
                    dist = np.sqrt(dx * dx + dy * dy)
                    if stats is not None and ok.any():
                        stats["margin"] = min(stats.get("margin", np.inf), float(np.min(np.abs(dist[ok] - thr))))
                    touch |= dist <= thr
            touch &= ok
            out["off"][:, b, i] = np.where(touch.any(axis=1), offs[np.argmax(touch, axis=1)], NONE)
    return _finish(out, flags)


def eval_gaps_loops(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, window=20, within=0):
    """eval_gaps with one loop per index of the contract."""
    n, B, flags, pose, lists, ego_shape, W = _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, window, within)
    out = _empty(n, B)
    for b in range(B):
        E = [circle_centres(pose[:, b], cc).tolist() for cc in ego_shape[:2]]            # [a][n] (x, y) as Python floats
        Vs = [[circle_centres(tr, sh[c]).tolist() for c in range(2)] for tr, sh in lists[b]]
        for k0, k1 in episodes_of(flags[:, b]):
            lo, hi = (k0, k1) if within == 0 else (0, n - 1)
            for k in range(k0, k1 + 1):
                for i, (tr, sh) in enumerate(lists[b]):
                    thr = ego_shape[2] + sh[2]
                    for o in range(W + 1):
                        found = None
                        for off in ((0,) if o == 0 else (-o, o)):
                            g = k - off
                            if found is None and lo <= g <= hi:
                                for a in range(2):
                                    for c in range(2):
                                        dx, dy = E[a][k][0] - Vs[i][c][g][0], E[a][k][1] - Vs[i][c][g][1]
                                        if math.sqrt(dx * dx + dy * dy) <= thr:
                                            found = off
                        if found is not None:
                            out["off"][k, b, i] = found
                            break
    return _finish(out, flags)
