#!/usr/bin/env python3
"""Interacting egos that share their MPC plans: tests/golden/loop_interact_plan_T13.npz -- the loop of
tests/golden/make_golden_loop_interact.py (main/scenarios/interactive_mpc.py run by the reference's own code, with the corrections
stated there, the same egos, the same stored columns, and beside them the plans the predictions were made from: plan_oa, plan_od
[tick][ego][T] and plan_ok [tick][ego], 0 after a failed solve), where an ego is predicted for the other one by the plan rule (include/jsim_mpc.h,
DESIGN.md section 27) instead of MovingObstaclesPrediction: the controls its controller holds at the start of the tick --
mpc[k].oa, mpc[k].odelta of its last solve, element 0 the input applied last tick -- from element 1 on, then the last steering
held at constant speed, rolled through the reference's own lib.simulation.Simulation.step from the tick-start state.  A
controller that has not solved yet (a new run, a respawn) holds an all-zero plan, as the device's cleared arrays do; after a failed
solve (oa, odelta = None) the input is (0, the steering applied last tick) throughout.  Build machine only (needs the reference
tree).

Asserted here: at least 10 ego-ticks cut by the other ego, at least 10 ticks on which a stored prediction lies more than 0.1 m from
the constant rule's, at least one respawn, no failed solve, and no collision decision within 1e-6 m of its threshold (a near-tie
that rounding could flip on another machine).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_golden_loop_interact import COLS, EGOS  # noqa: E402

N_TICKS = 112     # the second ego reaches its goal and respawns at tick 107; with the plans stored, the first ego's respawn at
                  # tick 119 would take the file beyond loop_interact_T13.npz's size


def main():
    import make_golden_refqp as RQ
    refmpc, rec = RQ.import_reference(13)
    from make_golden_planner import reference_primitives
    import mate_plan_numpy as MP
    from envs.intersection import intersection
    from lib.car_dimensions import BicycleModelDimensions
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    from lib.mp_search_ww_generic import MotionPrimitiveSearch
    from lib.simulation import HistorySimulation, Simulation, State
    from lib.trajectories import calc_nearest_index_in_direction, resample_curve
    MPC, MAX_ACCEL, T = refmpc.MPC, refmpc.MAX_ACCEL, refmpc.T

    DT = 0.2
    car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    mps = reference_primitives(car)
    n = len(EGOS)
    scenarios = [intersection(sp, tn) for sp, tn in EGOS]           # positional, as lib/ego_instance.py:16
    paths = []
    for sc in scenarios:
        _, _, trajectory_full = MotionPrimitiveSearch(sc, car, mps, margin=car.radius).run(debug=False)
        paths.append(trajectory_full)
    planned = [p.copy() for p in paths]                             # before MPC.__init__ unwraps the yaw column in place
    dl = np.linalg.norm(paths[0][0, :2] - paths[0][1, :2])
    TIME_HORIZON, FRAME_WINDOW = 7., 20
    N_STEPS = len(np.arange(0, TIME_HORIZON, DT))                   # the samples MovingObstaclesPrediction.state_prediction makes
    EXTRA_CUTOFF_MARGIN = 4 * int(math.ceil(car.radius / dl))

    def fresh(j):
        mpc = MPC(cx=paths[j][:, 0], cy=paths[j][:, 1], cyaw=paths[j][:, 2], dl=dl, dt=DT, car_dimensions=car)
        st = State(x=paths[j][0, 0], y=paths[j][0, 1], yaw=paths[j][0, 2], v=0.0)
        return mpc, st, HistorySimulation(car_dimensions=car, sample_time=DT, initial_state=st)

    def plan_held(k):
        """(oa [T], od [T], solved) of ego k's controller at the start of the tick."""
        if not solved[k]:
            return np.zeros(T), np.zeros(T), True                     # the controller has not solved yet
        if mpc[k].odelta is None:
            return np.zeros(T), np.zeros(T), False
        return np.array(mpc[k].oa, dtype=np.float64), np.array(mpc[k].odelta, dtype=np.float64), True

    def plan_prediction(k):
        """Ego k as the others see it: the rule's inputs through the reference's Simulation.step."""
        sim = Simulation(car_dimensions=car, sample_time=DT,
                         initial_state=State(x=state[k].x, y=state[k].y, yaw=state[k].yaw, v=state[k].v))
        oa, od, ok = plan_held(k)
        out = []
        for i in range(N_STEPS):
            j = i + 1
            if ok:
                a, d = (oa[j], od[j]) if j <= T - 1 else (0.0, od[T - 1])
            else:
                a, d = 0.0, delta[k]
            s = sim.step(a=a, delta=d)
            out.append((s.x, s.y, s.yaw))
        return np.array(out)

    mpc, state, simulation = [None] * n, [None] * n, [None] * n
    for j in range(n):
        mpc[j], state[j], simulation[j] = fresh(j)
    traj_agent_idx, tmp_trajectory, delta, solved = [0] * n, [None] * n, [0.0] * n, [False] * n
    ticks = np.zeros((N_TICKS, n, len(COLS)))
    preds = np.zeros((N_TICKS, n, N_STEPS, 3))
    plan_oa, plan_od, plan_ok = np.zeros((N_TICKS, n, T)), np.zeros((N_TICKS, n, T)), np.zeros((N_TICKS, n), dtype=np.int64)
    mate_cuts, differ, tightest = 0, 0, np.inf
    for i in range(N_TICKS):
        respawned = [False] * n
        for j in range(n):
            if mpc[j].is_goal(state[j]):                             # :121 -> respawn
                mpc[j], state[j], simulation[j] = fresh(j)
                traj_agent_idx[j], tmp_trajectory[j], delta[j], solved[j] = 0, None, 0.0, False
                respawned[j] = True
        # every ego as the others see it, from the tick-start states and the plans held at the start of the tick
        trajs = [plan_prediction(k) for k in range(n)]
        for k in range(n):
            plan_oa[i, k], plan_od[i, k], plan_ok[i, k] = plan_held(k)
        const = [np.vstack(MovingObstaclesPrediction(state[k].x, state[k].y, state[k].v, state[k].yaw, 0.0, delta[k],
                                                     sample_time=DT, car_dimensions=car).state_prediction(TIME_HORIZON)).T[:, :3]
                 for k in range(n)]
        differ += any(np.abs(trajs[k][:, :2] - const[k][:, :2]).max() > 0.1 for k in range(n))
        step_out = []
        for j in range(n):
            prev_len = -1 if tmp_trajectory[j] is None else len(tmp_trajectory[j])
            idx_in = traj_agent_idx[j]
            if tmp_trajectory[j] is None or np.any(tmp_trajectory[j][traj_agent_idx[j], :] != tmp_trajectory[j][-1, :]):
                traj_agent_idx[j] = calc_nearest_index_in_direction(state[j], paths[j][:, 0], paths[j][:, 1],
                                                                    start_index=traj_agent_idx[j], forward=True)
            trajectory_res = trajectory = paths[j][traj_agent_idx[j]:]
            if state[j].v < Simulation.MAX_SPEED:
                resample_dl = np.zeros((trajectory_res.shape[0],)) + MAX_ACCEL
                resample_dl = np.cumsum(resample_dl) + state[j].v
                resample_dl = DT * np.minimum(resample_dl, Simulation.MAX_SPEED)
                trajectory_res = resample_curve(trajectory_res, dl=resample_dl)
            else:
                trajectory_res = resample_curve(trajectory_res, dl=DT * Simulation.MAX_SPEED)
            others = [trajs[k] for k in range(n) if k != j]          # ego_vehicles[:j] + ego_vehicles[j+1:]
            tightest = min(tightest, MP.min_clearance_margin(trajectory_res, others, frame_window=FRAME_WINDOW))
            collision_xy = check_collision_moving_cars(car, trajectory_res, trajectory, others, frame_window=FRAME_WINDOW)
            if collision_xy is not None:
                cutoff_idx = get_cutoff_curve_by_position_idx(paths[j], collision_xy[0], collision_xy[1]) - EXTRA_CUTOFF_MARGIN
                cutoff_idx = max(traj_agent_idx[j] + 1, cutoff_idx)
                tmp_trajectory[j] = paths[j][:cutoff_idx]
                mate_cuts += 1
            else:
                tmp_trajectory[j] = paths[j]
            mpc[j].set_trajectory_fromarray(tmp_trajectory[j])
            tind_in = mpc[j].target_ind
            del rec.RECORDS[:]
            d, a = mpc[j].step(state[j])
            status = 0 if mpc[j].odelta is not None else 1
            dev = mpc[j].get_current_xref_deviation() if status == 0 else None
            ticks[i, j] = (state[j].x, state[j].y, state[j].yaw, state[j].v, idx_in, prev_len, traj_agent_idx[j],
                           len(tmp_trajectory[j]), 0.0 if collision_xy is None else 1.0, tind_in, mpc[j].target_ind, status,
                           d, a, float(respawned[j]))
            preds[i, j] = trajs[j]
            step_out.append((d, a, dev))
        for j in range(n):                                           # :188-190, after every ego has solved
            d, a, dev = step_out[j]
            delta[j], solved[j] = d, True
            state[j] = simulation[j].step(a=a, delta=d, xref_deviation=dev)
    assert mate_cuts >= 10, mate_cuts
    assert differ >= 10, differ
    assert ticks[:, :, 14].sum() >= 1
    assert ticks[:, :, 11].sum() == 0
    assert tightest > 1e-6, tightest
    final = np.array([[s.x, s.y, s.yaw, s.v] for s in state])
    np.savez_compressed(os.path.join(HERE, "loop_interact_plan_T13.npz"), ticks=ticks, preds=preds, final=final,
                        egos=np.array(EGOS, dtype=np.int64), planned0=planned[0], planned1=planned[1],
                        smoothed0=paths[0], smoothed1=paths[1], dl=np.float64(dl), margin=np.int64(EXTRA_CUTOFF_MARGIN),
                        frame_window=np.int64(FRAME_WINDOW), cols=np.array(COLS), plan_oa=plan_oa, plan_od=plan_od, plan_ok=plan_ok)
    print(f"plan-sharing egos {EGOS}: routes of {[len(p) for p in planned]} points (dl = {dl:.6f}), {N_TICKS} ticks, "
          f"ticks cut by the other ego: {mate_cuts}, ticks whose prediction differs from the constant rule's by > 0.1 m: {differ}, "
          f"respawns: {int(ticks[:, :, 14].sum())}, failed solves: {int(ticks[:, :, 11].sum())}, "
          f"tightest collision decision: {tightest:.3e} m from its threshold")


if __name__ == "__main__":
    main()
