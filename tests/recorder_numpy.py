"""How the tests' restatements read a History recorder's arrays, stated once in numpy and independent of the
package: which record ends an episode, which tick starts one, where an ego stands at the start of a tick, and an ego's episodes.
conflicts_numpy, static_numpy, reason_ticks_numpy, episodes_numpy and the four *_cases modules take these from here; ego_arrays is
the part of the cases' recorder_arrays that lays pose series out as a recorder would have written them."""
import numpy as np

FAILED, GOAL, AGE = 1, 2, 4                          # JSIM_REC_FAILED, JSIM_REC_GOAL, JSIM_REC_AGE


def is_end(flags):
    """A record with this flag ends an episode (the ego respawns behind it); elementwise."""
    return (np.asarray(flags) & (GOAL | AGE)) != 0


def episode_starts(flags):
    """[n][B] bool: tick k is the first of an episode because record k - 1 ended one (never tick 0: the reasons' carry decides there,
    and the episode outputs count tick 0 as a start by themselves)."""
    f = np.asarray(flags).reshape(np.shape(flags)[0], -1)
    s = np.zeros(f.shape, dtype=bool)
    s[1:] = is_end(f[:-1])
    return s


def start_poses(rec, flags, x_first, x_spawn):
    """[n][B][3]: every ego's (x, y, yaw) at the start of every tick: x_first at tick 0, x_spawn behind a record that ended an
    episode, else the record before (x_first / x_spawn are in the MPC's order x, y, v, yaw; a record is x, y, yaw, ...)."""
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    pose = np.empty((n, B, 3))
    if n:
        pose[0] = np.asarray(x_first, dtype=np.float64).reshape(B, 4)[:, [0, 1, 3]]
        pose[1:] = rec[:-1, :, :3]
        s = episode_starts(np.asarray(flags).reshape(n, B))
        pose[s] = np.broadcast_to(np.asarray(x_spawn, dtype=np.float64).reshape(B, 4)[:, [0, 1, 3]], (n, B, 3))[s]
    return pose


def episodes_of(flags_b):
    """(k0, k1) inclusive of every episode of one ego that has a tick: from a start to the tick whose flag ends it, or to n - 1."""
    f = np.asarray(flags_b).reshape(-1)
    out, k0 = [], 0
    for k in np.flatnonzero(is_end(f)):
        out.append((k0, int(k)))
        k0 = int(k) + 1
    if k0 < f.size:
        out.append((k0, f.size - 1))
    return out


def ego_arrays(egos, flags, decoy, hold_last=False, labels=None):
    """rec [N][B][7], flags [N][B], x_first, x_spawn [B][4] for one ego per pose series (egos[b] [N][3] = x, y, yaw at the start of
    every tick; flags[b] [N]), v = 3.0 throughout.  rec[k] is the pose at the start of tick k + 1, except where flags[k] ends the
    episode: there rec[k] is a far away state (`decoy`) and tick k + 1 starts at x_spawn, of which an ego has one.  The last record
    continues the last step, or repeats the last pose (hold_last).  An ego that never respawns keeps x_spawn = -decoy."""
    B, N = len(egos), len(egos[0])
    rec, fl_out = np.zeros((N, B, 7)), np.zeros((N, B), dtype=np.int32)
    x_first, x_spawn = np.zeros((B, 4)), np.full((B, 4), -float(decoy))
    for b, (ego, fl) in enumerate(zip(egos, flags)):
        x_first[b] = ego[0, 0], ego[0, 1], 3.0, ego[0, 2]
        rec[:-1, b, :3] = ego[1:]
        rec[-1, b, :3] = ego[-1] if hold_last else ego[-1] + (ego[-1] - ego[-2])
        rec[:, b, 3] = 3.0
        for k in np.flatnonzero(is_end(fl)):
            if k + 1 < N:
                spawn = (ego[k + 1, 0], ego[k + 1, 1], 3.0, ego[k + 1, 2])
                assert x_spawn[b, 0] == -decoy or tuple(x_spawn[b]) == spawn, b if labels is None else labels[b]
                x_spawn[b] = spawn
            rec[k, b, :3] = decoy
        fl_out[:, b] = fl
    return {"rec": rec, "flags": fl_out, "x_first": x_first, "x_spawn": x_spawn}
