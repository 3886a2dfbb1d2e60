"""The collision cut-off of every recorded tick (jsim_loop_eval_cutoffs) in numpy: a recording -- the History
recorder's rec / flags / obs, x_first and x_spawn -- walked tick by tick through oracle/loop_oracle.py:loop_pre_tick with the loops'
carry rules.  Test infrastructure; one obstacle shape for all vehicles (the fixtures need no more)."""
import numpy as np

import loop_oracle as LO

GOAL, AGE = 2, 4          # JSIM_REC_GOAL, JSIM_REC_AGE


def state_at(rec, flags, x_first, x_spawn, k, b):
    """(x, y, v, yaw) of ego b at the start of tick k, and whether the tick starts an episode (tick 0 or behind an end flag)."""
    if k == 0:
        return np.asarray(x_first[b], dtype=np.float64), True
    if flags[k - 1, b] & (GOAL | AGE):
        return np.asarray(x_spawn[b], dtype=np.float64), True
    r = rec[k - 1, b]
    return np.array([r[0], r[1], r[3], r[2]]), False


def mate_tuple(rec, flags, x_first, x_spawn, k, b):
    """How ego b is predicted by its group mates at the start of tick k: (x, y, v, yaw, a = 0, the delta of its record before), the
    delta 0 on tick 0 and behind a respawn."""
    s, fresh = state_at(rec, flags, x_first, x_spawn, k, b)
    return (s[0], s[1], s[2], s[3], 0.0, 0.0 if fresh else float(rec[k - 1, b, 4]))


def initial_carry(fulls, path_id):
    """The loops' own start: progress index 0, no previous path, the whole path."""
    return np.array([[0, -1, len(fulls[p])] for p in path_id], dtype=np.int32)


def replay(rec, flags, obs, x_first, x_spawn, fulls, path_id, dl, frame_window=10, speed_cutoff=False, groups=None, veh_range=None,
           obst_dims=None, margin_factor=4, carry=None, first_tick=0, n_ticks=None, L=2.86, dt=0.2):
    """rec [n][B][7], flags [n][B], obs [n][n_obs][6] or None; fulls: the paths (arrays [M][3]), path_id [B]; groups: offsets
    [n_groups + 1] of interacting egos or None; veh_range [B][2]: each ego's vehicles among obs (default: all).  Evaluates the ticks
    [first_tick, n_ticks).  Returns status, idx, cut, hit [m][B], col_xy [m][B][2] and carry [B][3]."""
    rec, flags = np.asarray(rec, dtype=np.float64), np.asarray(flags)
    n, B = flags.shape
    n = n if n_ticks is None else n_ticks
    m = n - first_tick
    n_obs = 0 if obs is None else obs.shape[1]
    car = initial_carry(fulls, path_id) if carry is None else np.array(carry, dtype=np.int32)
    out = {"status": np.zeros((m, B), np.int32), "idx": np.zeros((m, B), np.int32), "cut": np.zeros((m, B), np.int32),
           "hit": np.zeros((m, B), bool), "col_xy": np.full((m, B, 2), np.nan)}
    group_of = None if groups is None else np.repeat(np.arange(len(groups) - 1), np.diff(groups))
    for k in range(first_tick, n):
        tup = [mate_tuple(rec, flags, x_first, x_spawn, k, b) for b in range(B)] if groups is not None else None
        for b in range(B):
            s, _ = state_at(rec, flags, x_first, x_spawn, k, b)
            full = fulls[path_id[b]]
            lo, hi = (0, n_obs) if veh_range is None else veh_range[b]
            obst = [tuple(obs[k, o]) for o in range(lo, hi)]
            if groups is not None:
                g = group_of[b]
                obst += [tup[j] for j in range(groups[g], groups[g + 1]) if j != b]
            idx, prev, cur = (int(v) for v in car[b])
            st, i2, plen, col = LO.loop_pre_tick((s[0], s[1], s[3], s[2]), idx, None if prev < 0 else prev, full, obst, dl, L=L, dt=dt,
                                                 obst_dims=obst_dims, margin_factor=margin_factor, frame_window=frame_window)
            if st == 0:                              # a refused tick leaves the index and the cut-off as they were
                idx, cur = i2, plen
            r = k - first_tick
            out["status"][r, b], out["idx"][r, b], out["cut"][r, b] = st, idx, cur
            if st == 0 and col is not None:
                out["hit"][r, b], out["col_xy"][r, b] = True, col
            prev = len(full) if speed_cutoff else cur
            if flags[k, b] & (GOAL | AGE):           # the ego respawns behind this record: the glue starts over
                idx, prev = 0, -1
            car[b] = (idx, prev, cur)
    out["carry"] = car
    return out
