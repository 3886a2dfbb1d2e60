"""jsim_loop_score_plan_predictions (include/jsim_mpc.h) restated in numpy: the plan-rule prediction of every
recorded tick of every ego -- tests/mate_plan_numpy.py's predict_plan from the tick-start state, the recorded plan and the steering
of the record before -- against the ego's records of the ticks that followed, by tests/predictions_numpy.py's error arithmetic.  TEST
INFRASTRUCTURE ONLY.  Rows are the egos."""
import numpy as np

import mate_plan_numpy as MP
import predictions_numpy as PN


def predict(state, oa, od, status, delta_last, n_steps, dt, L):
    """The samples (x, y, yaw) [n_steps][3] of the plan rule from state = (x, y, v, yaw)."""
    x, y, v, yaw = (float(t) for t in state)
    return MP.predict_plan(x, y, v, yaw, oa, od, int(status), float(delta_last), n_steps, dt=dt, L=L)


def eval_plan_predictions(rec, flags, x_first, x_spawn, plan_oa, plan_od, plan_status, n_steps, tol, dt, L, n=None, predictor=predict):
    """The entry point on the first n ticks.  plan_oa, plan_od [N][B][T], plan_status [N][B] (0 = JSIM_OK); predictor(state, oa, od,
    status, delta_last, n_steps, dt, L) -> samples [n_steps][3].  Returns pt_i [n][B][3] int32, pt_d [n][B][6], step_sum [B][n_steps],
    step_cnt int32, err [n][B][n_steps]."""
    n = flags.shape[0] if n is None else n
    B = flags.shape[1]
    rec, flags = rec[:n], flags[:n]
    pt_i, pt_d = np.zeros((n, B, 3), dtype=np.int32), np.full((n, B, 6), np.nan)
    err = np.full((n, B, n_steps), np.nan)
    inputs = PN.ego_inputs(rec, flags, x_first, x_spawn) if n else None          # (x, y, v, yaw, 0, delta_last)
    for b in range(B):
        for k in range(n):
            tup = inputs[k, b]
            m = min(n_steps, PN.ego_horizon(flags[:, b], k) - k + 1)
            samples = predictor(tup[:4], plan_oa[k, b], plan_od[k, b], plan_status[k, b], tup[5], n_steps, dt, L)
            pt_i[k, b], pt_d[k, b], err[k, b] = PN.score(samples, rec[k:k + m, b, :3], m, tol)
    scored = ~np.isnan(err)
    step_cnt = scored.sum(axis=0).astype(np.int32)
    step_sum = np.cumsum(np.where(scored, err, 0.0), axis=0)[-1] if n else np.zeros((B, n_steps))   # (cumsum adds in tick order)
    return {"pt_i": pt_i, "pt_d": pt_d, "step_sum": step_sum, "step_cnt": step_cnt, "err": err}
