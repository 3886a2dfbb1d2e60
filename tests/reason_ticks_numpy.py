"""Numpy restatement of the per-tick stakeholder reasons and the replan trigger, written from the contract
and used by the tests as the CPU side of jsim_loop_eval_reasons: from a History recorder's arrays, the ego's position at the start
of every tick, the distance to its cyclist, the policymaker / driver / cyclist values, the two in-range timers and the trigger.
The lane-parallel part is vectorised over ticks and egos; the timers and the tracker go tick by tick in order (vectorised over
egos only), with the additions the reference makes."""
import numpy as np

from recorder_numpy import episode_starts, is_end, start_poses

# columns of a parameter row (JSIM_REASON_* of include/jsim_mpc.h) that the evaluation reads
DT, CENTRE, WIDTH, REF_D, BUF_D, THR_D, REF_C, BUF_C, THR_C = 0, 3, 4, 5, 6, 7, 8, 9, 10
DEFAULT_PAR = np.array([0.1, 2.0, 30.0 / 3.6, 0.0, 2.0, 10.0, 2.0, 8.0, 8.0, 2.0, 5.0, 1.0])
THRESHOLD = 0.7                                      # ReasonParameters.REASONS_THRESHOLD


def start_positions(rec, flags, x_first, x_spawn):
    """[n][B][2]: the ego's (x, y) at the start of every tick."""
    return start_poses(rec, flags, x_first, x_spawn)[:, :, :2]


def eval_ticks(rec, flags, obs, x_first, x_spawn, veh_of, par, threshold, carry=None):
    """rec [n][B][7], flags [n][B], obs [n][n_obs][6] or None, x_first / x_spawn [B][4] (x, y, v, yaw), veh_of [B] (-1: no
    cyclist), par [B][12], threshold [B], carry [B][3] or None (zeros).  Returns val [n][B][4] (policymaker, driver, cyclist,
    distance), timers [n][B][2], trig [n][B] (bit 0 needed, bits 1-3 policymaker / driver / cyclist below), first [B], carry [B][3]."""
    rec = np.asarray(rec, dtype=np.float64)
    n, B = rec.shape[:2]
    flags = np.asarray(flags).reshape(n, B)
    par = np.asarray(par, dtype=np.float64).reshape(B, -1)
    thr = np.asarray(threshold, dtype=np.float64).reshape(B)
    veh = np.asarray(veh_of).reshape(B) if obs is not None else np.full(B, -1)
    has = veh >= 0
    carry = np.zeros((B, 3)) if carry is None else np.array(carry, dtype=np.float64).reshape(B, 3)
    pos = start_positions(rec, flags, x_first, x_spawn)
    dist = np.full((n, B), np.nan)
    if obs is not None and has.any() and n:
        c = np.asarray(obs, dtype=np.float64)[:, veh[has], :2]
        dx, dy = c[:, :, 0] - pos[:, has, 0], c[:, :, 1] - pos[:, has, 1]
        dist[:, has] = np.sqrt(dx * dx + dy * dy)
    rng_d, rng_c = par[:, REF_D] + par[:, BUF_D], par[:, REF_C] + par[:, BUF_C]
    with np.errstate(invalid="ignore"):
        in_d, in_c = dist < rng_d, dist < rng_c              # NaN (no cyclist) is in no range
    dc = (pos[:, :, 0] - par[:, WIDTH] / 2) - par[:, CENTRE]
    pol = np.where(dc >= 0.0, 1.0, np.exp(0.2 * np.minimum(dc, 0.0)))
    comfort = np.where(in_c, np.exp(0.2 * np.where(in_c, dist - rng_c, 0.0)), 1.0)
    start = episode_starts(flags)
    dt = par[:, DT]
    timers = np.empty((n, B, 2))
    t_d, t_c = carry[:, 0].copy(), carry[:, 1].copy()
    for k in range(n):
        t_d = np.where(start[k], 0.0, t_d)
        t_c = np.where(start[k], 0.0, t_c)
        t_d = np.where(in_d[k], t_d + dt, t_d)
        t_c = np.where(in_c[k], t_c + dt, t_c)
        timers[k, :, 0], timers[k, :, 1] = t_d, t_c
    on_d, on_c = in_d & (timers[:, :, 0] >= par[:, THR_D]), in_c & (timers[:, :, 1] >= par[:, THR_C])
    drv = np.where(on_d, 1.0 / np.exp(0.2 * np.where(on_d, timers[:, :, 0] - par[:, THR_D], 0.0)), 1.0)
    cyt = np.where(on_c, 1.0 / np.exp(0.2 * np.where(on_c, timers[:, :, 1] - par[:, THR_C], 0.0)), 1.0)
    cyc = cyt * comfort
    drv[:, ~has] = np.nan
    cyc[:, ~has] = np.nan
    with np.errstate(invalid="ignore"):
        lo = np.stack([pol < thr, drv < thr, cyc < thr], axis=2)
    below = lo.any(axis=2)
    trig = np.zeros((n, B), dtype=np.int32)
    first = np.full(B, -1, dtype=np.int32)
    tracker = carry[:, 2] != 0.0
    for k in range(n):
        tracker = tracker & ~start[k]
        need = below[k] & ~tracker
        tracker = below[k]
        trig[k] = need
        first[need & (first < 0)] = k
    trig |= (lo[:, :, 0] * 2 + lo[:, :, 1] * 4 + lo[:, :, 2] * 8).astype(np.int32)
    out_carry = np.stack([t_d, t_c, tracker.astype(np.float64)], axis=1) if n else carry.copy()
    if n:
        out_carry[is_end(flags[n - 1])] = 0.0   # the next tick starts an episode
    return {"val": np.stack([pol, drv, cyc, dist], axis=2), "timers": timers, "trig": trig, "first": first, "carry": out_carry}
