"""Numpy restatement of the clearance and first-contact evaluation, written from the contract and used by
the tests as the CPU side of jsim_loop_eval_conflicts: from a History recorder's arrays, every ego's pose at the start of every
tick, its vehicles' and group mates' poses, and per episode the reference's pair table -- ego circle a, vehicle i, frame offset
off, vehicle circle c, the vehicle taken at the episode's frame clamp(f - off, 0, N - 1) -- from which come `clear`, `who`, `row`
per tick and `hit_tick`, `hit_frame`, `hit_xy` per episode.  eval_conflicts is vectorised over an episode's frames and rows;
eval_conflicts_loops states the same with one Python loop per index and is what the vectorised form is checked against."""
import numpy as np

from recorder_numpy import episodes_of, start_poses   # (the tests and the fixture generator reach them as CN.*)

MAX_OBS = 8                                          # JSIM_MAX_OBS
MAX_WINDOW = 20


def circle_centres(pose, cc):
    """[..., 2] the centre of the circle at body offset cc of poses [..., 3]."""
    return np.stack([pose[..., 0] + np.cos(pose[..., 2]) * cc, pose[..., 1] + np.sin(pose[..., 2]) * cc], axis=-1)


def vehicle_list(b, B, n_obs, veh_range, mate_range):
    """The vehicles of ego b in the contract's order: ("veh", o) for o in [lo, hi), then ("mate", m) for m in [mlo, mhi), m != b."""
    lo, hi = (int(v) for v in veh_range[b])
    mlo, mhi = (int(v) for v in mate_range[b])
    if not (0 <= lo <= n_obs and 0 <= hi <= n_obs and 0 <= mlo <= B and 0 <= mhi <= B):
        raise ValueError(f"ego {b}: a range outside its table")
    out = [("veh", o) for o in range(lo, hi)] + [("mate", m) for m in range(mlo, mhi) if m != b]
    if len(out) > MAX_OBS:
        raise ValueError(f"ego {b}: {len(out)} vehicles (at most {MAX_OBS})")
    return out


def _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, w):
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    n_obs = 0 if obs is None else np.shape(obs)[1]
    obs = None if obs is None else np.asarray(obs, dtype=np.float64)
    if not 0 <= int(w) <= MAX_WINDOW:
        raise ValueError("frame_window outside [0, 20]")
    ego_shape = tuple(float(v) for v in ego_shape)
    rows = None if shapes is None else np.asarray(shapes, dtype=np.float64).reshape(n_obs, -1)[:, :3]
    pose = start_poses(rec, flags, x_first, x_spawn)
    lists = []
    for b in range(B):
        lst = []
        for kind, j in vehicle_list(b, B, n_obs, np.asarray(veh_range).reshape(B, 2), np.asarray(mate_range).reshape(B, 2)):
            if kind == "veh":
                shape = ego_shape if rows is None else tuple(rows[j].tolist())
                lst.append((obs[:, j][:, [0, 1, 3]], shape))
            else:
                lst.append((pose[:, j], ego_shape))
        lists.append(lst)
    return n, B, flags, pose, lists, ego_shape, int(w)


def _empty(n, B):
    return {"clear": np.full((n, B), np.nan), "who": np.full((n, B), -1, dtype=np.int32), "row": np.full((n, B), -1, dtype=np.int32),
            "hit_tick": np.full((n, B), -1, dtype=np.int32), "hit_frame": np.full((n, B), -1, dtype=np.int32),
            "hit_xy": np.full((n, B, 2), np.nan)}


def _note(stats, dist, thr):
    """Keeps the smallest |dist - threshold| met (the fixture generator's condition)."""
    if stats is not None and dist.size:
        stats["margin"] = min(stats.get("margin", np.inf), float(np.min(np.abs(dist - thr))))


def _first_contact(out, b, k0, N, ego, ego_cc, first_f, pos, thr, stats=None):
    """The episode outputs from the first touching row's vehicle circle position: front ++ rear, the first hit modulo N."""
    traj = np.concatenate([circle_centres(ego, ego_cc[0]), circle_centres(ego, ego_cc[1])])
    dx, dy = pos[0] - traj[:, 0], pos[1] - traj[:, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    _note(stats, dist, thr)
    mask = dist <= thr
    frame = int(np.argmax(mask)) % N
    out["hit_tick"][k0, b] = k0 + first_f
    out["hit_frame"][k0, b] = frame
    out["hit_xy"][k0, b] = ego[frame, :2]


def eval_conflicts(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, w=0, stats=None):
    """rec [n][B][7], flags [n][B], obs [n][n_obs][6] or None, x_first / x_spawn [B][4], veh_range / mate_range [B][2], shapes
    [n_obs][>= 3] (cc_front, cc_rear, radius) or None (the ego's shape), ego_shape (cc_front, cc_rear, radius), w = frame_window.
    Returns clear [n][B], who, row, hit_tick, hit_frame [n][B] int32, hit_xy [n][B][2].  stats: a dict that receives `margin`, the
    smallest |dist - threshold| of any comparison made."""
    n, B, flags, pose, lists, ego_shape, w = _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, w)
    out = _empty(n, B)
    offs = np.arange(-w, w + 1)
    for b in range(B):
        nv = len(lists[b])
        if nv == 0:
            continue
        thr = np.array([ego_shape[2] + sh[2] for _, sh in lists[b]])                      # the unfused sum, per vehicle
        for k0, k1 in episodes_of(flags[:, b]):
            N = k1 - k0 + 1
            ego = pose[k0:k1 + 1, b]
            A = np.stack([circle_centres(ego, ego_shape[0]), circle_centres(ego, ego_shape[1])])            # [a][N][2]
            idx = np.clip(np.arange(N)[:, None] - offs[None, :], 0, N - 1)                                # [N][2w + 1]
            V = np.stack([np.stack([circle_centres(tr[k0:k1 + 1], sh[0]), circle_centres(tr[k0:k1 + 1], sh[1])])
                          for tr, sh in lists[b]])                                                            # [i][c][N][2]
            Vo = np.moveaxis(V[:, :, idx], 1, 3)                                                            # [i][N][off][c][2]
            d = A[:, None, :, None, None, :] - Vo[None]                                                     # [a][i][N][off][c][2]
            dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
            dist = np.moveaxis(dist, 2, 0)                                                                  # [N][a][i][off][c]
            _note(stats, dist, thr[None, None, :, None, None])
            touch = (dist <= thr[None, None, :, None, None]).reshape(N, -1)
            gap = (dist[:, :, :, w, :] - thr[None, None, :, None]).reshape(N, -1)                           # rows (a, i, c)
            j = np.argmin(gap, axis=1)                                                                      # the lowest row on ties
            out["clear"][k0:k1 + 1, b] = gap[np.arange(N), j]
            out["who"][k0:k1 + 1, b] = (j // 2) % nv
            any_f = touch.any(axis=1)
            out["row"][k0:k1 + 1, b] = np.where(any_f, np.argmax(touch, axis=1), -1)
            if any_f.any():
                f = int(np.argmax(any_f))
                r = int(out["row"][k0 + f, b])
                c, o, i = r % 2, (r // 2) % (2 * w + 1), (r // (2 * (2 * w + 1))) % nv
                _first_contact(out, b, k0, N, ego, ego_shape[:2], f, V[i, c, idx[f, o]], thr[i], stats)
    return out


def eval_conflicts_loops(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, w=0):
    """eval_conflicts with one loop per index of the contract (the circle centres come from the same circle_centres)."""
    n, B, flags, pose, lists, ego_shape, w = _inputs(rec, flags, obs, x_first, x_spawn, veh_range, mate_range, shapes, ego_shape, w)
    out = _empty(n, B)
    for b in range(B):
        nv = len(lists[b])
        if nv == 0:
            continue
        for k0, k1 in episodes_of(flags[:, b]):
            N = k1 - k0 + 1
            ego = pose[k0:k1 + 1, b]
            A = [circle_centres(ego, ego_shape[0]), circle_centres(ego, ego_shape[1])]
            V = [[circle_centres(tr[k0:k1 + 1], sh[0]), circle_centres(tr[k0:k1 + 1], sh[1])] for tr, sh in lists[b]]
            first = None
            for f in range(N):
                best, row = None, -1
                for a in range(2):
                    for i in range(nv):
                        thr = ego_shape[2] + lists[b][i][1][2]
                        for off in range(-w, w + 1):
                            g = min(max(f - off, 0), N - 1)
                            for c in range(2):
                                r = ((a * nv + i) * (2 * w + 1) + (off + w)) * 2 + c
                                dx, dy = A[a][f, 0] - V[i][c][g, 0], A[a][f, 1] - V[i][c][g, 1]
                                dist = np.sqrt(dx * dx + dy * dy)
                                if dist <= thr and row < 0:
                                    row = r
                                    if first is None:
                                        first = (f, V[i][c][g], thr)
                                if off == 0 and (best is None or dist - thr < best[0]):
                                    best = (dist - thr, i)
                out["clear"][k0 + f, b], out["who"][k0 + f, b], out["row"][k0 + f, b] = best[0], best[1], row
            if first is not None:
                _first_contact(out, b, k0, N, ego, ego_shape[:2], *first)
    return out
