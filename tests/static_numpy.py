"""Numpy restatement of the static-obstacle evaluation, written from the contract and used by the tests as
the CPU side of jsim_loop_eval_static and by tools/bench_static.py as its baseline: from a History recorder's arrays every ego's
pose at the start of every tick (recorder_numpy.start_poses), its two circle centres, and against the rows of
its obstacle set `clear`, `who`, `hit` per tick and `off_tick` per episode.  eval_static is vectorised over ticks and over the egos
that share a set; eval_static_loops states the same with one Python loop per index and is what the vectorised form is checked
against."""
import numpy as np

import conflicts_numpy as CN
import recorder_numpy as RN

ROW = 32                                             # JSIM_STATIC_ROW


def halfplane_values(hp, x, y):
    """(a * x + b * y) + c of every half-plane [n_hp][3] at points x, y [...]: the unfused sum, in that order -> [n_hp][...]."""
    hp = np.asarray(hp, dtype=np.float64)
    shape = (-1,) + (1,) * np.ndim(x)
    a, b, c = (hp[:, j].reshape(shape) for j in range(3))
    return (a * x + b * y) + c


def distance(row, x, y):
    """BoxObstacle / CircleObstacle.distance_to_point of one row at points x, y [...]."""
    g0, g1, g2, g3 = row[3:7]
    if row[0] != 0:
        dx, dy = g0 - x, g1 - y
        return np.maximum(0.0, np.sqrt(dx * dx + dy * dy) - g2)
    dx = np.maximum(np.maximum(g0 - x, 0.0), x - g2)
    dy = np.maximum(np.maximum(g1 - y, 0.0), y - g3)
    return np.sqrt(dx * dx + dy * dy)


def _inputs(rec, flags, x_first, x_spawn, set_of, set_off, rows, ego_shape):
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    set_off = np.asarray(set_off, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    set_of = np.broadcast_to(np.asarray(set_of, dtype=np.int64), (B,))
    cc_f, cc_r, radius = (float(v) for v in ego_shape)
    pose = RN.start_poses(rec, flags, x_first, x_spawn)
    return n, B, flags, set_of, set_off, rows, pose, CN.circle_centres(pose, cc_f), CN.circle_centres(pose, cc_r), radius


def _empty(n, B):
    return {"clear": np.full((n, B), np.nan), "who": np.full((n, B), -1, dtype=np.int32), "hit": np.full((n, B), -1, dtype=np.int32),
            "off_tick": np.full((n, B), -1, dtype=np.int32)}


def _off_ticks(out, flags):
    n, B = flags.shape
    for b in range(B):
        for k0, k1 in RN.episodes_of(flags[:, b]):
            t = np.flatnonzero(out["hit"][k0:k1 + 1, b] >= 0)
            if t.size:
                out["off_tick"][k0, b] = k0 + int(t[0])


def eval_static(rec, flags, x_first, x_spawn, set_of, set_off, rows, ego_shape, include_hidden=False, stats=None):
    """rec [n][B][7], flags [n][B], x_first / x_spawn [B][4], set_of [B] (or one index), set_off [n_sets + 1], rows [n_rows][32],
    ego_shape (cc_front, cc_rear, radius).  A set_of outside [0, n_sets) is an empty set.  Returns clear [n][B], who, hit, off_tick
    [n][B] int32.  stats: a dict that receives per ego `hp_margin [B]` -- the smallest amount by which a half-plane value would
    have to move to change whether a (centre, obstacle) pair touches -- and `who_margin [B]`, the smallest difference between the
    two smallest clearances of a tick (inf with fewer than two obstacles)."""
    n, B, flags, set_of, set_off, rows, pose, F, R, radius = _inputs(rec, flags, x_first, x_spawn, set_of, set_off, rows, ego_shape)
    out = _empty(n, B)
    if stats is not None:
        stats["hp_margin"], stats["who_margin"] = np.full(B, np.inf), np.full(B, np.inf)
    n_sets = len(set_off) - 1
    for s in np.unique(set_of):
        egos = np.flatnonzero(set_of == s)
        if not 0 <= s < n_sets or n == 0:
            continue
        X = np.stack([F[:, egos, 0], R[:, egos, 0]])                   # [circle][n][egos]
        Y = np.stack([F[:, egos, 1], R[:, egos, 1]])
        clear, who, hit = np.full(X.shape[1:], np.nan), np.full(X.shape[1:], -1), np.full(X.shape[1:], -1)
        for i, row in enumerate(rows[set_off[s]:set_off[s + 1]]):
            if row[1] != 0 and not include_hidden:
                continue
            cl = distance(row, X, Y).min(axis=0) - radius
            v = halfplane_values(row[8:8 + 3 * int(row[2])].reshape(-1, 3), X, Y)       # [n_hp][circle][n][egos]
            inside = (v <= 0.0).all(axis=0)
            touch = inside.any(axis=0)
            if stats is not None:
                m = np.where(inside, np.abs(v).min(axis=0), np.where(v > 0.0, v, -np.inf).max(axis=0))
                np.minimum.at(stats["hp_margin"], egos, m.min(axis=(0, 1)))
            better = (who < 0) | (cl < clear)
            clear, who = np.where(better, cl, clear), np.where(better, i, who)
            hit = np.where((hit < 0) & touch, i, hit)
        out["clear"][:, egos], out["who"][:, egos], out["hit"][:, egos] = clear, who, hit
        if stats is not None:
            stats["who_margin"][egos] = who_margins(rows[set_off[s]:set_off[s + 1]], X, Y, radius, include_hidden)
    _off_ticks(out, flags)
    return out


def who_margins(rows, X, Y, radius, include_hidden):
    """Per ego the smallest difference between the two smallest per-obstacle clearances of any tick (inf: fewer than two)."""
    cls = [distance(row, X, Y).min(axis=0) - radius for row in rows if include_hidden or row[1] == 0]
    if len(cls) < 2:
        return np.full(X.shape[2], np.inf)
    two = np.sort(np.stack(cls), axis=0)[:2]
    return (two[1] - two[0]).min(axis=0)


def eval_static_loops(rec, flags, x_first, x_spawn, set_of, set_off, rows, ego_shape, include_hidden=False):
    """eval_static with one loop per index of the contract."""
    n, B, flags, set_of, set_off, rows, pose, F, R, radius = _inputs(rec, flags, x_first, x_spawn, set_of, set_off, rows, ego_shape)
    out = _empty(n, B)
    for b in range(B):
        s = int(set_of[b])
        mine = rows[set_off[s]:set_off[s + 1]] if 0 <= s < len(set_off) - 1 else rows[:0]
        for k in range(n):
            best = None
            for i, row in enumerate(mine):
                if row[1] != 0 and not include_hidden:
                    continue
                touched = False
                for x, y in (F[k, b], R[k, b]):
                    d = float(distance(row, x, y)) - radius
                    if best is None or d < best[0]:
                        best = (d, i)
                    if all((row[8 + 3 * h] * x + row[9 + 3 * h] * y) + row[10 + 3 * h] <= 0.0 for h in range(int(row[2]))):
                        touched = True
                if touched and out["hit"][k, b] < 0:
                    out["hit"][k, b] = i
            if best is not None:
                out["clear"][k, b], out["who"][k, b] = best
    for b in range(B):
        k0 = 0
        for k in range(n):
            if out["hit"][k, b] >= 0 and out["off_tick"][k0, b] < 0:
                out["off_tick"][k0, b] = k
            if RN.is_end(flags[k, b]):
                k0 = k + 1
    return out
