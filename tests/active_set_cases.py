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

A fourth family, the full-set family (full_set_case; tests/test_full_set_cpu.py, tests/test_gpu_full_set.py), brings the working
set to all 2T variables, which the three above cannot: with the stock weights the last acceleration moves only v_T, which costs
nothing, so one variable always stays free and 2T - 1 is where they end.  The off-path egos at v0 = 0.1 .. 0.35 under the tight
acceleration limits and a weight on the speed (Q_v_yaw[0] = 1, Qf[2] = 1, R = [0.01, 1e-4]) reach, on nine egos in ten:
  * the add at position 2T - 1 (the last column of R, a Householder reflection on a trailing block of one element) and the full set
    at termination (2T active bits) -- form "adds", MAX_DSTEER = 3000: by 2T adds and nothing else on most egos;
  * an entering row at q = 2T -- form "drops", MAX_DSTEER = 0.4: with every variable bound a further violated row depends on the
    working set by necessity, so the iteration is a pure dual step and a forced drop; the oracle's trace counts the iterations that
    begin there (full_entering): 900 .. 2600 per batch of 64, not zero as a first probe of this family had it;
  * the full set carried over the ticks of a closed loop (the later ticks start from the tick before);
  * form "mixed": full-set rows and stock rows alternate through the per-ego table, solves of 60 .. 180 iterations beside solves of 40.
Still taken by no input of the suite: the clamp of a negative primal step length to 0.  In exact arithmetic it cannot fire --
viol > 0 at selection, zn > 0, and a partial step of length t1 < t2 leaves viol - t1 zn > 0 --, so it is a rounding guard, not a
path; a scratch copy of the oracle counted it 0 times in 2.4 million iterations of the three families above.  It is not in the trace.
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


# ------------------------------------------------------------------------------------------------
# The full-set family: a working set of all 2T variables.
# ------------------------------------------------------------------------------------------------
# With the stock weights Q_v_yaw[0] = 0 and Qf[2] = 0 the last acceleration a_{T-1} moves only v_T, which costs nothing: R and Rd
# alone hold it strictly inside its box, and one of the 2T variables stays free (2T - 1 above).  A weight on the speed sends it to
# its bound like the others.
FULL_WEIGHTS = dict(Q_v_yaw=[1.0, 0.5], Qf=[1.0, 1.0, 1.0, 0.5], R=[0.01, 1e-4])
FULL_LIMITS = dict(MAX_ACCEL=0.05, MAX_DECEL=-0.05)
FULL_DSTEER = dict(drops=0.4, adds=3000.0)    # "drops": TIGHT's steering rate -- drops and dependent rows on the way; "adds": the
#                                               rate rows out of reach, the full set by 2T adds and nothing else
# the start speed per horizon, and the draw.  Chosen on the oracle's evidence alone (tests/test_full_set_cpu.py prints the counts).
FULL_V0 = {25: 0.35, 40: 0.1}                 # (at 0.25: 0 .. 4 egos of a batch reach the full set at T = 25; at T = 40 a sixth
#                                               of a batch misses the margin of the mask comparison)
FULL_V0_DEFAULT = 0.25
FULL_SEED = 5
FULL_B = dict(drops=64, adds=48, mixed=96)    # the family's egos per form; a GPU case tiles them up to its kernel's dispatch size
FULL_MARGIN = 1000.0                          # a compared ego's multipliers exceed this many activity thresholds
FULL_LEFT_OUT = 0.10                          # .. and at most this share of a batch is left out of the mask comparison


def full_v0(T):
    return FULL_V0.get(T, FULL_V0_DEFAULT)


def full_config(base, T, form="drops"):
    """The full-set row: tight acceleration limits, a weight on the speed, and the form's steering-rate limit."""
    return replace(base, T=T, MAX_DSTEER=FULL_DSTEER[form], **FULL_LIMITS,
                   **{k: list(v) for k, v in FULL_WEIGHTS.items()})


def full_set_case(synth, routes, base, B, T, form="drops", seed=FULL_SEED, v0=None):
    """(batch, cfgs, which) of the full-set family: the off-path tight family's egos at speed v0 (default: full_v0(T)) under
    full_config.  form "drops" / "adds": every ego a full-set row (which = 0).  form "mixed": the even egos full-set rows of the
    "drops" form, the odd egos the stock row `base` (which = 1) -- one launch then holds solves that end at q = 2T after a hundred
    iterations beside solves that have long finished."""
    batch = off_path_batch(synth, routes, B, T, seed)
    batch.x0[:, 2] = full_v0(T) if v0 is None else v0
    rows = (full_config(base, T, "drops" if form == "mixed" else form), replace(base, T=T))
    which = np.zeros(B, dtype=np.int64)
    if form == "mixed":
        which[1::2] = 1
    return batch, [rows[k] for k in which], which


def full_set_stock_case(synth, routes, base, B, T, seed=FULL_SEED):
    """The mixed batch's states with every full-set row replaced by the stock row: what a stock-row neighbour must not be able to
    tell from the mixed batch."""
    batch, _, which = full_set_case(synth, routes, base, B, T, "mixed", seed)
    return batch, [replace(base, T=T)] * B, which


def tile(batch, cfgs, which, B):
    """The family's egos repeated cyclically up to B egos (B >= len(cfgs)): (batch, cfgs, which, first) with first[b] the ego that b
    copies."""
    first = np.arange(B) % len(cfgs)
    fields = {k: np.ascontiguousarray(v[first]) for k, v in vars(batch).items()}
    return type(batch)(**fields), [cfgs[k] for k in first], which[first], first


def oracle_steps(oracle, routes, batch, cfgs, which):
    """The oracle's traced step of every ego of a family batch, one ego at a time with its condensed QP: the arrays of
    oracle.mpc_step_batch_per_config(trace=True) and beside them H [B, n, n], g [B, n], lam [B, 8T] and u [B, n] (a_0, delta_0, ..;
    under the acceleration-state variant the free acc_0 last, recovered from the predicted speeds)."""
    from gpu_helpers import oracle_params_list
    ps = oracle_params_list(oracle, cfgs, which)
    rows = []
    for b in range(len(cfgs)):
        p = ps[which[b]]
        r, x0 = routes[int(batch.path_id[b])][:int(batch.path_len[b])], batch.x0[b]
        res = oracle.mpc_step(p, (x0[0], x0[1], x0[3], x0[2]), r[:, 0], r[:, 1], r[:, 2], int(batch.target_ind[b]), float(batch.speed[b]),
                              oa=batch.oa[b], od=batch.od[b], want_qp=True, trace=True)
        res["u"] = np.stack([res["oa"], res["od"]], axis=1).reshape(-1)
        if p.nx == 5:
            res["u"] = np.concatenate([res["u"], [(res["ov"][1] - res["ov"][0]) / p.dt - res["oa"][0]]])
        rows.append(res)
    keys = ("oa", "od", "ox", "oy", "ov", "oyaw", "lam", "active_mask", "H", "g", "trace", "u", "status", "n_iter", "target_ind")
    return {k: np.array([r[k] for r in rows]) for k in keys}


def full_reached(oracle, ref, n):
    """bool [B] from a traced oracle run: the egos whose working set reached all n variables and whose final active mask has n bits."""
    bits = np.unpackbits(np.ascontiguousarray(ref["active_mask"]).view(np.uint8), axis=1).sum(axis=1)
    return (ref["trace"][:, oracle.TRACE["max_q"]] == n) & (bits == n) & (ref["status"] == 0)


def margin_ok(lam, g):
    """The rule that admits an ego to the bit-exact mask comparison, on the oracle's multipliers alone: every multiplier of the
    final working set that is positive exceeds FULL_MARGIN activity thresholds 1e-9 max(1, |g|_inf), so that no kernel's rounding
    can move one across the threshold."""
    thr = 1e-9 * max(1.0, float(np.abs(g).max()))
    lam = np.asarray(lam)
    return bool(np.all(lam[lam > 0.0] > FULL_MARGIN * thr))


def compared(ref):
    """bool [B] of an oracle_steps result: the egos that solve and pass margin_ok."""
    return np.array([ref["status"][b] == 0 and margin_ok(ref["lam"][b], ref["g"][b]) for b in range(len(ref["status"]))])


def active_rows(mask_row, m):
    """The row ids of an active mask's set bits."""
    words = np.ascontiguousarray(mask_row).view(np.uint32)
    return [i for i in range(m) if (int(words[i >> 5]) >> (i & 31)) & 1]


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
