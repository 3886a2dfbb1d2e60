"""The cases of tests/test_conditioning_cpu.py and tests/test_gpu_conditioning.py: the cost weights of the reference's sensitivity
study (main/scenarios/mpc_sensitivity_analysis_comulative.py:103-128 -- one weight at a time around its reset_config defaults,
zeros included) and four rows beyond them, each at three states.  No RNG; every case carries its expected class, written here.

  rows    SWEEP_ROWS: the script's 30 rows.  EXTREME_ROWS: both steering weights zero, both R entries zero, both acceleration
          weights zero (the last acceleration column of H is then exactly zero), and that row with R[0] = 1e-8 instead.
  states  a  the script's start (:187): the route's first point, v = 0, cold warm start, the controller's default speed limit;
          b  v = 1e-3, 0.3 m / 0.05 rad off route 0 at point 40, speed limit 5;
          c  as b with v = 3.
  class   "pd": cond(H) <= 1e13 and the KKT system on the optimal active set is regular.  "singular": everything else -- state a
          with a zero steering weight R[1] (at a standstill a constant steering angle costs nothing) and, at every state, the
          row whose acceleration weights R[0] and Rd[0] are both zero; under the acceleration-state variant (NX = 5) also the
          standstill without w_para (SINGULAR_JERK).  tests/test_conditioning_cpu.py proves the classes from the oracle's H.
The kernels get the weights as they are: nothing floors a zero."""
from dataclasses import dataclass, replace

import numpy as np

# reset_config of the script (:32-50): what every sweep row starts from
DEFAULTS = dict(w_perp=20.0, w_para=1.0, R=[0.1, 0.01], Rd=[10.0, 1.0], Q_v_yaw=[0.0, 0.5], Qf=[1.0, 1.0, 0.0, 0.5],
                MAX_DSTEER=30.0, MAX_ACCEL=2.0, MAX_DECEL=-10.0, MAX_ITER=1)
SWEEP_ROWS = tuple(
    [(f"w_perp={v}", dict(w_perp=float(v))) for v in (0, 1, 10, 20, 50)] +
    [(f"w_para={v}", dict(w_para=float(v))) for v in (0, 0.1, 1, 5, 10)] +
    [(f"R_acc={v}", dict(R=[float(v), 0.01])) for v in (0, 0.01, 0.1, 1, 10)] +
    [(f"R_steer={v}", dict(R=[0.1, float(v)])) for v in (0, 0.01, 0.1, 1, 10)] +
    [(f"Rd_acc={v}", dict(Rd=[float(v), 1.0])) for v in (0, 1, 5, 10, 20)] +
    [(f"Rd_steer={v}", dict(Rd=[10.0, float(v)])) for v in (0, 0.01, 0.1, 1, 10)])
EXTREME_ROWS = (("steer_free", dict(R=[0.1, 0.0], Rd=[10.0, 0.0])), ("R_zero", dict(R=[0.0, 0.0])),
                ("acc_free", dict(R=[0.0, 0.01], Rd=[0.0, 1.0])), ("acc_1e-8", dict(R=[1e-8, 0.01], Rd=[0.0, 1.0])))
ROWS = SWEEP_ROWS + EXTREME_ROWS
STATES = ("a", "b", "c")
ROUTE, POINT, LATERAL, DYAW, SPEED_LIMIT_BC, SPEED_LIMIT_A = 0, 40, 0.3, 0.05, 5.0, 30 / 3.6
V0 = dict(a=0.0, b=1e-3, c=3.0)
# the singular class, by name
SINGULAR = frozenset([("R_steer=0", "a"), ("steer_free", "a"), ("R_zero", "a"), ("acc_free", "a"), ("acc_free", "b"), ("acc_free", "c")])
# the acceleration-state variant (NX = 5) has one more: at the standstill without w_para its free acc_0 costs nothing
SINGULAR_JERK = SINGULAR | frozenset([("w_para=0", "a")])


def cls_of(case, kind="stock"):
    """The class of a case under the stock model (Case.cls) or the acceleration-state variant (kind "jerk")."""
    return "singular" if (case.row, case.state) in (SINGULAR_JERK if kind == "jerk" else SINGULAR) else "pd"


@dataclass(frozen=True)
class Case:
    row: str
    state: str
    weights: dict          # the row's overrides of DEFAULTS
    cls: str               # "pd" | "singular"

    @property
    def name(self):
        return f"{self.row}@{self.state}"


CASES = tuple(Case(name, s, w, "singular" if (name, s) in SINGULAR else "pd") for name, w in ROWS for s in STATES)
SWEEP_CASES_A = tuple(c for c in CASES if c.state == "a" and c.row in dict(SWEEP_ROWS))
assert len(SWEEP_ROWS) == 30 and len(CASES) == 102 and len(SINGULAR) == sum(c.cls == "singular" for c in CASES) == 6


def config_of(case, base, T):
    """The MPCConfig of a case: `base` (what the table does not carry: NX, JERK_WEIGHT, ...) with the script's defaults and the
    row's weights."""
    kw = dict(DEFAULTS)
    kw.update(case.weights)
    return replace(base, T=T, **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})


def state_of(case, routes):
    """(x0 [x, y, v, yaw], target_ind, speed limit) of a case on the yaw-smoothed route table."""
    r = routes[ROUTE]
    if case.state == "a":
        return np.array([r[0, 0], r[0, 1], 0.0, r[0, 2]]), 0, SPEED_LIMIT_A
    s = POINT
    yaw = r[s, 2]
    return (np.array([r[s, 0] - LATERAL * np.sin(yaw), r[s, 1] + LATERAL * np.cos(yaw), V0[case.state], yaw + DYAW]), s,
            SPEED_LIMIT_BC)


def box_widths(cfg, T, max_steer, jerk=None):
    """D of qp_exact.certificate: how far two feasible points can lie apart in each variable, from the box rows -- the
    acceleration rows AU / AL and the steering rows S; for the free acc_0 of the acceleration-state variant (jerk = (speed limit,
    MIN_SPEED, dt)) from the t = 1 speed rows, v_1 = v_0 + dt (acc_0 + u_0)."""
    D = np.empty(2 * T + (1 if jerk else 0))
    D[0:2 * T:2] = cfg.MAX_ACCEL - cfg.MAX_DECEL
    D[1:2 * T:2] = 2 * max_steer
    if jerk:
        speed, vmin, dt = jerk
        D[2 * T] = (speed - vmin) / dt + (cfg.MAX_ACCEL - cfg.MAX_DECEL)
    return D


# What "the certificate passes" means for the oracle: the tolerances of the solver the reference calls (ECOS: feastol = abstol =
# reltol = 1e-8).  The kernels are held to 16 x the oracle's own figures instead (bar()).
FEAS_TOL = GAP_TOL = 1e-8


def certificate_passes(ce):
    return ce["primal"] <= FEAS_TOL and ce["lam_min"] >= 0.0 and ce["gap"] <= GAP_TOL * max(1.0, abs(ce["f"]))


def bar(oracle_figure, value=0.0):
    """The bar of a kernel figure next to the oracle's figure for the same case: 16 x -- another summation order and fast_rsqrt's
    <= 1 ulp -- with a floor of 1e-13 max(1, |value|)."""
    return max(16.0 * oracle_figure, 1e-13 * max(1.0, abs(value)))


def measure(QX, H, g, G, h, u, lam, active, D, exact=True):
    """The figures of one answer (u, lam, active set) to the QP (H, g, G, h): qp_exact.certificate's, and -- exact -- its distance
    from qp_exact.solve_on on its own active set: err_u, err_lam (on the active rows), u_max / lam_max of the exact solution and
    `infeasible`, by how much that solution violates a row outside the set.  `singular`: solve_on refused."""
    out = dict(QX.certificate(H, g, G, h, u, lam, D))
    if exact:
        try:
            ue, le, _ = QX.solve_on(H, g, G, h, active)
        except QX.SingularKKT:
            out["singular"] = True
            return out
        out.update(singular=False, err_u=float(np.abs(u - ue).max()), u_max=float(np.abs(ue).max()),
                   err_lam=float(np.abs(np.asarray(lam)[active] - le).max(initial=0.0)), lam_max=float(np.abs(le).max(initial=0.0)),
                   infeasible=float(np.max(G @ ue - h)))
    return out


def with_acc0(u, oa0, ov, dt):
    """The acceleration-state variant's full decision vector (u0_0, delta_0, ..., acc_0) from a step's outputs: the step does
    not return its free acc_0, but its predicted speeds do, v_1 = v_0 + dt (acc_0 + u0_0) -- to a few ulp of v / dt."""
    return np.concatenate([u, [(ov[1] - ov[0]) / dt - oa0]])


def oracle_step(oracle, p, routes, batch, b):
    """oracle.mpc_step of ego b of `batch` with parameters p, the condensed QP included; "u" = (a_0, delta_0, a_1, ...), with the
    recovered acc_0 behind it under the acceleration-state variant."""
    r, x0 = routes[int(batch.path_id[b])][:int(batch.path_len[b])], batch.x0[b]
    res = oracle.mpc_step(p, (x0[0], x0[1], x0[3], x0[2]), r[:, 0], r[:, 1], r[:, 2], int(batch.target_ind[b]), float(batch.speed[b]),
                          oa=batch.oa[b], od=batch.od[b], want_qp=True)
    res["u"] = np.stack([res["oa"], res["od"]], axis=1).reshape(-1)
    if p.nx == 5 and res["status"] == 0:
        res["u"] = with_acc0(res["u"], res["oa"][0], res["ov"], p.dt)
    return res


def make_batch(synth, routes, T, B, base, cases=CASES):
    """(batch, cfgs, which, cases): B egos, ego b the case cases[b % len(cases)] (the list tiled cyclically), full paths, cold warm
    starts; cfgs[b] its MPCConfig, which[b] = b % len(cases) (egos with equal which share a configuration)."""
    n = len(cases)
    which = np.arange(B, dtype=np.int64) % n
    st = [state_of(c, routes) for c in cases]
    pool = [config_of(c, base, T) for c in cases]
    batch = synth.EgoBatch(x0=np.array([st[k][0] for k in which]), path_id=np.full(B, ROUTE, dtype=np.int32),
                           path_len=np.full(B, len(routes[ROUTE]), dtype=np.int32),
                           target_ind=np.array([st[k][1] for k in which], dtype=np.int64),
                           speed=np.array([st[k][2] for k in which]), oa=np.zeros((B, T)), od=np.zeros((B, T)))
    return batch, [pool[k] for k in which], which, cases
