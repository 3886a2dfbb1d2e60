"""Inputs that drive the active-set iteration down the paths the stock inputs barely reach, shared by tests/test_active_set_cpu.py
(the premises, on the oracle alone) and tests/test_gpu_active_set.py (every kernel against the oracle).  Seeded builders only: the
same arguments give the same arrays, no state is kept here.

Three families:

  off-path tight   every ego 3 m to the left of where the draw put it and turned 0.8 rad away from its path, zero warm start,
                   MAX_ACCEL = 0.05, MAX_DECEL = -0.05, MAX_DSTEER = 0.4 deg/s.  All solvable; most of the 8T rows want into the
                   working set, so a solve makes dozens of adds and drops, meets entering rows that depend on the working set (a
                   pure dual step and a forced drop) and fills the working set up to 2T - 1 rows.
  infeasible A     v0 = speed - 0.01 and MAX_DECEL = +0.5: the row a_0 >= MAX_DECEL wants a_0 >= 0.5, the row v_1 <= speed, with
                   v_1 = v0 + dt * a_0, wants a_0 <= (speed - v0) / dt = 0.05.
  infeasible B     v0 = 0.5, MAX_DECEL = -10 and MAX_ACCEL = -3.0 (T < 25) or -1.5: every a_t <= MAX_ACCEL gives
                   v_T = v0 + dt * sum a_t <= v0 + dt * T * MAX_ACCEL (-7.3 at T = 13, -7.0 at T = 25), below MIN_SPEED = -5.

v0 of A and B lies inside [MIN_SPEED, speed], so the constant rows hold and the exits before the iteration are not taken: the
solver finds the contradiction only inside the loop, after adds and drops, as "no step length" (an entering row that depends on the
working set while no multiplier can decrease).  `contradiction` states the failure by arithmetic on v0, speed, dt, T and the limits
alone -- no solver, no oracle.

mixed_case builds one batch with all of it through the per-ego table: most egos off-path tight, every eighth one an A or a B row
between solvable neighbours, and the v0-above-limit ego of the per-ego table tests (gpu_helpers.PLANT_FAIL, braking with -3.7),
so that both kinds of failure sit in one launch.

Two branches of the iteration are taken by no input here and by none of the suite's other families: a working set of all 2T
variables at the start of an iteration (2T - 1 is reached), and the clamp of a negative primal step length to 0.  The oracle's
trace shows the first; the second was counted in a scratch copy of the oracle (0 times in 2.4 million iterations of these inputs).
Neither is chased.
"""
from dataclasses import replace

import numpy as np

from gpu_helpers import PLANT_DECEL, PLANT_FAIL

LATERAL, DYAW = 3.0, 0.8                      # off-path: metres to the left, radians turned away
TIGHT = dict(MAX_ACCEL=0.05, MAX_DECEL=-0.05, MAX_DSTEER=0.4)
EVERY = 8                                     # every eighth ego is planted ...
FIRST = 7                                     # ... from ego 7 on: A at 7, 23, 39, .., B at 15, 31, 47, ..
A_MARGIN, A_DECEL = 0.01, 0.5
B_V0 = 0.5
V0_ABOVE = 9.5                                # PLANT_FAIL's speed, as gpu_helpers.plant_ego_states plants it
ROW_TIGHT, ROW_A, ROW_B, ROW_V0 = 0, 1, 2, 3  # `which` of the mixed batch
# the draw of the egos per horizon.  Changed only on the oracle's evidence (tests/test_active_set_cpu.py), never on a device's.
SEEDS = {20: 15}                              # (T = 20 with draw 5: a planted ego at B = 96, 256 and 1025 reaches the exit without a drop)
DEFAULT_SEED = 5


def seed_of(T):
    return SEEDS.get(T, DEFAULT_SEED)


def b_accel(T):
    """Family B's MAX_ACCEL at horizon T."""
    return -3.0 if T < 25 else -1.5


def tight_config(base, T):
    return replace(base, T=T, **TIGHT)


def a_config(base, T):
    return replace(base, T=T, MAX_DECEL=A_DECEL)


def b_config(base, T):
    return replace(base, T=T, MAX_ACCEL=b_accel(T), MAX_DECEL=-10.0)


def off_path_batch(synth, routes, B, T, seed=None):
    """The off-path tight family's egos: a draw on untruncated paths away from their ends, then every ego moved LATERAL to its
    left and turned DYAW further to the left, warm starts zero."""
    batch = synth.make_ego_batch(routes, B, T, seed=seed_of(T) if seed is None else seed, truncate=False, near_end_frac=0.0)
    yaw = batch.x0[:, 3].copy()
    batch.x0[:, 0] -= LATERAL * np.sin(yaw)
    batch.x0[:, 1] += LATERAL * np.cos(yaw)
    batch.x0[:, 3] += DYAW
    batch.oa[:] = 0.0
    batch.od[:] = 0.0
    return batch


def planted(B):
    """(A egos, B egos) of a mixed batch of B egos."""
    egos = np.arange(FIRST, B, EVERY)
    return egos[0::2], egos[1::2]


def family_case(synth, routes, base, B, T, family, seed=None):
    """(batch, cfg) of one family alone under one configuration: "tight", "A" or "B"."""
    batch = off_path_batch(synth, routes, B, T, seed)
    if family == "tight":
        return batch, tight_config(base, T)
    if family == "A":
        batch.x0[:, 2] = batch.speed - A_MARGIN
        return batch, a_config(base, T)
    assert family == "B"
    batch.x0[:, 2] = B_V0
    return batch, b_config(base, T)


def mixed_case(synth, routes, base, B, T, seed=None, plant=True):
    """(batch, cfgs, which) of the mixed batch: ego b solves with cfgs[b], egos with equal which[b] share a configuration.
    plant=False: the same states, but every planted A / B row replaced by the stock row `base` (under which those egos solve) --
    the run that the neighbours of a planted ego must not be able to tell from the planted one."""
    assert B > max(PLANT_FAIL, FIRST + EVERY)
    batch = off_path_batch(synth, routes, B, T, seed)
    rows = {ROW_TIGHT: tight_config(base, T), ROW_A: a_config(base, T), ROW_B: b_config(base, T),
            ROW_V0: replace(base, T=T, MAX_DECEL=PLANT_DECEL)}
    which = np.full(B, ROW_TIGHT, dtype=np.int64)
    ea, eb = planted(B)
    assert PLANT_FAIL not in ea and PLANT_FAIL not in eb
    batch.x0[ea, 2] = batch.speed[ea] - A_MARGIN
    batch.x0[eb, 2] = B_V0
    batch.x0[PLANT_FAIL, 2] = V0_ABOVE
    which[ea], which[eb], which[PLANT_FAIL] = ROW_A, ROW_B, ROW_V0
    if not plant:
        rows[ROW_A] = rows[ROW_B] = replace(base, T=T)
    return batch, [rows[k] for k in which], which


def contradiction(v0, speed, dt, T, cfg):
    """Why ego (v0, speed) cannot have a feasible QP under cfg's limits, or None.  The model's speed is v_t = v0 + dt * (a_0 + ..
    + a_{t-1}) exactly (the linearisation's speed row is the plant's), and MAX_DECEL <= a_s <= MAX_ACCEL, so
    v0 + dt * t * MAX_DECEL <= v_t <= v0 + dt * t * MAX_ACCEL; the QP asks MIN_SPEED <= v_t <= speed for t = 0 .. T.
    1e-8: the violation of a constant row that the reference's solver still accepts (mpc_oracle.c, orc_build_qp)."""
    lo, hi, vmin = float(cfg.MAX_DECEL), float(cfg.MAX_ACCEL), float(cfg.MIN_SPEED)
    if v0 - speed > 1e-8:
        return "v0 > speed"
    if vmin - v0 > 1e-8:
        return "v0 < MIN_SPEED"
    if lo > hi:
        return "MAX_DECEL > MAX_ACCEL"
    for t in range(1, T + 1):
        if v0 + dt * t * lo > speed:
            return f"v_{t} >= v0 + dt * {t} * MAX_DECEL > speed"
        if v0 + dt * t * hi < vmin:
            return f"v_{t} <= v0 + dt * {t} * MAX_ACCEL < MIN_SPEED"
    return None


def contradictory(batch, cfgs, dt):
    """bool [B]: the egos of a batch whose QP `contradiction` proves infeasible."""
    return np.array([contradiction(float(batch.x0[b, 2]), float(batch.speed[b]), dt, c.T, c) is not None for b, c in enumerate(cfgs)])


def trace_totals(oracle, trace):
    """The batch totals of a traced oracle run that the tests and the reports use."""
    t = oracle.TRACE
    return dict(adds=int(trace[:, t["adds"]].sum()), drops=int(trace[:, t["drops"]].sum()),
                dependent=int(trace[:, t["dependent"]].sum()), drops_first=int(trace[:, t["drops_first"]].sum()),
                drops_last=int(trace[:, t["drops_last"]].sum()), max_q=int(trace[:, t["max_q"]].max()),
                in_loop=int((trace[:, t["end"]] == oracle.END_INFEASIBLE_IN_LOOP).sum()),
                max_iters=int((trace[:, t["end"]] == oracle.END_MAX_ITERS).sum()),
                before_loop=int((trace[:, t["end"]] == oracle.END_BEFORE_LOOP).sum()))
