"""numpy restatement of the plan rule of interacting egos (JSIM_MATE_PLAN, include/jsim_mpc.h): an ego as
its group mates predict it when the egos share their MPC plans, and the loop glue of one ego against such predictions.  TEST
INFRASTRUCTURE ONLY.  Pinned by tests/golden/mate_plan.npz, which the reference's own Simulation.step wrote
(tests/golden/make_golden_mate_plan.py): the same libm calls in the same order, so the two agree to rounding of the last bit."""
import os

import numpy as np

import loop_oracle as LO
import oracle_py as O

MAX_STEER = np.deg2rad(45.0)      # main/lib/simulation.py:23-25
MAX_SPEED = 30.0 / 3.6
MIN_SPEED = -5.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def plan_cases():
    """The cases of tests/golden/mate_plan.npz as dicts (padding removed)."""
    g = np.load(os.path.join(GOLDEN, "mate_plan.npz"), allow_pickle=False)
    out = []
    for k, name in enumerate(g["names"]):
        T, n = int(g["T"][k]), int(g["n_steps"][k])
        out.append(dict(name=str(name), x0=g["x0"][k], oa=g["oa"][k, :T], od=g["od"][k, :T], status=int(g["status"][k]),
                        delta_last=float(g["delta_last"][k]), T=T, n_steps=n, pred=g["pred"][k, :n], cc=g["cc"][k, :n]))
        assert np.isnan(g["oa"][k, T:]).all() and np.isnan(g["pred"][k, n:]).all()
    return out


def plan_inputs(oa, od, status, delta_last, n_steps):
    """(a [n_steps], delta [n_steps]): the input of every prediction step.  oa, od [T]: the controls of the ego's last solve as the
    engine holds them at the start of the tick (element 0 = the input applied last tick); status: that solve's (0 = JSIM_OK);
    delta_last: the steering applied last tick."""
    T = len(oa)
    a, d = np.zeros(n_steps), np.zeros(n_steps)
    for i in range(n_steps):
        j = i + 1
        if status == 0:
            a[i], d[i] = (oa[j], od[j]) if j <= T - 1 else (0.0, od[T - 1])
        else:
            a[i], d[i] = 0.0, delta_last
    return a, d


def predict_plan(x, y, v, yaw, oa, od, status, delta_last, n_steps, dt=LO.DT, L=2.86, max_steer=MAX_STEER, max_speed=MAX_SPEED,
                 min_speed=MIN_SPEED):
    """[n_steps][3] (x, y, yaw): sample i is the pose after step i of Simulation.step (main/lib/simulation.py:35-47 with
    Bicycle.step, main/bicycle/main.py:28-41) under plan_inputs."""
    a, d = plan_inputs(oa, od, status, delta_last, n_steps)
    out = np.zeros((n_steps, 3))
    for i in range(n_steps):
        delta = max(min(d[i], max_steer), -max_steer)
        xc_dot = v * np.cos(yaw)
        yc_dot = v * np.sin(yaw)
        theta_dot = (v / L) * np.tan(delta)
        x += xc_dot * dt
        y += yc_dot * dt
        yaw += theta_dot * dt
        v += a[i] * dt
        v = max(min(v, max_speed), min_speed)
        out[i] = (x, y, yaw)
    return out


def predict_constant(x, y, v, yaw, delta_last, n_steps, dt=LO.DT, L=2.86):
    """The constant rule (jsim_loop_predict_egos): MovingObstaclesPrediction(x, y, v, yaw, a = 0, steering = delta_last)."""
    return LO.predict_obstacle(x, y, v, yaw, 0.0, delta_last, dt=dt, L=L, horizon=n_steps * dt - 0.5 * dt)


def circle_centres(pred, L=2.86):
    """[n_steps][2 circles][2]: the circle centres of a predicted trajectory, front circle first."""
    _, offs = LO.car_circles(L)
    return np.stack([LO.circle_centres(pred, xo) for xo in offs], axis=1)


def pre_tick(state_xyyawv, traj_agent_idx, prev_path_len, full, preds, dl, L=2.86, dt=LO.DT, frame_window=20):
    """LO.loop_pre_tick for one ego whose obstacles come as predicted trajectories `preds` (each [n_steps][3]) instead of get()
    tuples -- the same building blocks in the same order: (status, traj_agent_idx, path_len, collision_xy or None)."""
    x, y, yaw, v = state_xyyawv
    M = len(full)
    if prev_path_len is None or traj_agent_idx != prev_path_len - 1:
        st, idx = O.nearest_index_in_direction(x, y, full[:, 0], full[:, 1], traj_agent_idx, True)
        if st != 0:
            return st, traj_agent_idx, prev_path_len if prev_path_len is not None else M, None
        traj_agent_idx = idx
    detailed = full[traj_agent_idx:]
    res = detailed[LO.resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), v, dt))]
    col = LO.first_collision_fast(res, detailed, preds, L=L, frame_window=frame_window)
    if col is None:
        return 0, traj_agent_idx, M, None
    c = LO.cutoff_index(full, col[0], col[1])
    assert c is not None
    return 0, traj_agent_idx, max(traj_agent_idx + 1, c - LO.extra_cutoff_margin(dl, L)), (col[0], col[1])


def min_clearance_margin(res, preds, L=2.86, frame_window=20):
    """How far the closest circle pair of first_collision_fast's table is from the threshold (|distance - 2 radius|, metres): a
    decision with a margin near 0 is a near-tie that rounding could flip."""
    radius, offs = LO.car_circles(L)
    thr = 2 * radius
    P = len(preds[0])
    F = max(len(res), P)
    fa, fo = np.minimum(np.arange(F), len(res) - 1), np.minimum(np.arange(F), P - 1)
    j = np.clip(fo[:, None] - np.arange(-frame_window, frame_window + 1)[None, :], 0, P - 1)
    ego = np.stack([LO.circle_centres(res, xo)[fa] for xo in offs], axis=1)
    obs = np.stack([np.stack([LO.circle_centres(p, xo)[j] for xo in offs], axis=2) for p in preds], axis=1)
    d = ego[:, :, None, None, None, :] - obs[:, None, :, :, :, :]
    return float(np.abs(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) - thr).min())
