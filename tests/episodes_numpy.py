"""Restatement of the per-episode table (jsim_loop_summarise_episodes), written from the contract with plain
loops over history.episode_bounds and used by the tests as the CPU side of the call: from a History recorder's arrays and the
per-tick series of the three evaluations (any of them None), one row per episode.  Sums by math.fsum; minima and maxima tick by
tick in order, a NaN passed over, the first tick that holds the value kept."""
import math

import numpy as np

from recorder_numpy import FAILED, start_poses

EP_INT = ("ego", "k0", "n", "end", "failed", "dev_tick", "veh_tick", "veh_who", "veh_hit_tick", "veh_hit_frame", "st_tick", "st_who",
          "st_off_tick", "st_obstacle", "st_ticks_off", "replan_tick")
EP_DOUBLE = ("length", "v_mean", "v_max", "a_min", "a_max", "delta_absmax", "dev_max", "dev_mean", "veh_clear", "veh_hit_x",
             "veh_hit_y", "st_clear", "pm_min", "driver_min", "cyclist_min", "dist_min")
SUMS = ("length", "v_mean", "dev_mean")                # the columns with a tolerance; every other one is exact
NAN = float("nan")


def extreme(values, k0, lowest):
    """(value, tick) of the smallest / largest entry that is not NaN, the first tick that holds it; (NaN, -1) without one."""
    best, tick = NAN, -1
    for i, v in enumerate(values):
        v = float(v)
        if v != v:
            continue
        if tick < 0 or (v < best if lowest else v > best):
            best, tick = v, k0 + i
    return best, tick


def summarise(H, rec, flags, x_first, x_spawn, veh=None, st=None, rs=None):
    """H: the package's history module (episode_bounds).  rec [n][B][7], flags [n][B], x_first / x_spawn [B][4] (x, y, v, yaw);
    veh: dict clear, who, hit_tick, hit_frame [n][B], hit_xy [n][B][2] or None; st: dict clear, who, hit, off_tick [n][B] or None;
    rs: dict val [n][B][4], trig [n][B] or None.  Returns ep_off [B + 1] and one array per column."""
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    pose = start_poses(rec, flags, x_first, x_spawn)
    rows = []
    off = [0]
    for b in range(B):
        for k0, k1, end in H.episode_bounds(flags[:, b]):
            r = {k: -1 for k in EP_INT}
            r.update({k: NAN for k in EP_DOUBLE})
            r.update(ego=b, k0=k0, n=k1 - k0, end=int(end), failed=0, st_ticks_off=0)
            if k1 > k0:
                steps = []
                for k in range(k0, k1):
                    dx, dy = rec[k, b, 0] - pose[k, b, 0], rec[k, b, 1] - pose[k, b, 1]
                    steps.append(math.sqrt(dx * dx + dy * dy))
                v, delta, a, dev = (rec[k0:k1, b, j].tolist() for j in (3, 4, 5, 6))
                r["failed"] = sum(1 for k in range(k0, k1) if flags[k, b] & FAILED)
                r["length"] = math.fsum(steps)
                r["v_mean"] = math.fsum(v) / (k1 - k0)
                r["v_max"] = extreme(v, k0, False)[0]
                r["a_min"], r["a_max"] = extreme(a, k0, True)[0], extreme(a, k0, False)[0]
                r["delta_absmax"] = extreme([abs(x) for x in delta], k0, False)[0]
                r["dev_max"], r["dev_tick"] = extreme(dev, k0, False)
                have = [x for x in dev if x == x]
                r["dev_mean"] = math.fsum(have) / len(have) if have else NAN
                if veh is not None:
                    r["veh_clear"], r["veh_tick"] = extreme(veh["clear"][k0:k1, b], k0, True)
                    r["veh_who"] = int(veh["who"][r["veh_tick"], b]) if r["veh_tick"] >= 0 else -1
                    r["veh_hit_tick"], r["veh_hit_frame"] = int(veh["hit_tick"][k0, b]), int(veh["hit_frame"][k0, b])
                    r["veh_hit_x"], r["veh_hit_y"] = (float(x) for x in veh["hit_xy"][k0, b])
                if st is not None:
                    r["st_clear"], r["st_tick"] = extreme(st["clear"][k0:k1, b], k0, True)
                    r["st_who"] = int(st["who"][r["st_tick"], b]) if r["st_tick"] >= 0 else -1
                    r["st_off_tick"] = int(st["off_tick"][k0, b])
                    r["st_obstacle"] = int(st["hit"][r["st_off_tick"], b]) if 0 <= r["st_off_tick"] < n else -1
                    r["st_ticks_off"] = sum(1 for k in range(k0, k1) if st["hit"][k, b] >= 0)
                if rs is not None:
                    for j, key in enumerate(("pm_min", "driver_min", "cyclist_min", "dist_min")):
                        r[key] = extreme(rs["val"][k0:k1, b, j], k0, True)[0]
                    r["replan_tick"] = next((k for k in range(k0, k1) if rs["trig"][k, b] & 1), -1)
            rows.append(r)
        off.append(len(rows))
    out = {"ep_off": np.array(off, dtype=np.int64)}
    out.update({k: np.array([r[k] for r in rows], dtype=np.int32) for k in EP_INT})
    out.update({k: np.array([r[k] for r in rows], dtype=np.float64) for k in EP_DOUBLE})
    return out


def compare(got, ref, bar=1e-12):
    """Every column of `got` against `ref`: exact but for the three sums, which are within bar * max(1, |value|).  Returns the largest
    error of a sum (relative to max(1, |value|))."""
    assert np.array_equal(got["ep_off"], ref["ep_off"]), (got["ep_off"][-5:], ref["ep_off"][-5:])
    worst = 0.0
    for k in EP_INT + EP_DOUBLE:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k in SUMS:
            assert np.array_equal(np.isnan(g), np.isnan(r)), k
            ok = ~np.isnan(r)
            if ok.any():
                err = float(np.max(np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))))
                assert err <= bar, (k, err)
                worst = max(worst, err)
        else:
            assert np.array_equal(g, r, equal_nan=k in EP_DOUBLE), (k, np.flatnonzero(~((g == r) | ((g != g) & (r != r))))[:5].tolist())
    return worst
