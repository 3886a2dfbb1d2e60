#!/usr/bin/env python3
"""Interacting egos: tests/golden/loop_interact_T13.npz -- main/scenarios/interactive_mpc.py (two MPC egos at one intersection
that predict each other and cut their paths at the first predicted collision) as the reference's own code runs it, recorded
tick by tick.  Build machine only (needs the reference tree).

Everything on the path is the reference's own code, imported and executed unmodified:
    envs.intersection.intersection(...)                                  the scenarios, called as Ego_instance calls them
    lib.mp_search_ww_generic.MotionPrimitiveSearch(...).run()            the planner -> paths[j]                   (:60-63)
    lib.mpc.MPC(cx, cy, cyaw, dl, dt, car_dimensions)                    one controller per ego, stock T = 13      (:98-100)
    lib.moving_obstacles_prediction.MovingObstaclesPrediction            the prediction of the other egos
    lib.collision_avoidance.check_collision_moving_cars (FRAME_WINDOW = 20), get_cutoff_curve_by_position_idx with
    EXTRA_CUTOFF_MARGIN (:75-77), lib.trajectories.resample_curve / calc_nearest_index_in_direction, one
    lib.simulation.HistorySimulation per ego
The scenarios are built as lib/ego_instance.py:16 builds them: intersection(self.start_position, self.turn_indicator) passed
POSITIONALLY to intersection(turn_indicator, start_pos) (envs/intersection.py:10), so Ego_instance(1, 1) drives
intersection(turn_indicator=1, start_pos=1) and Ego_instance(3, 2) drives intersection(turn_indicator=3, start_pos=2).
The loop body is interactive_mpc.py:117-190 in its own order -- every ego's glue and MPC.step on the tick-start states, then
every ego's plant step (a Jacobi step) -- with these corrections, without which the script cannot run or records nothing:
  * prediction of the other egos: MovingObstaclesPrediction(x, y, v, yaw, a = 0, steering = the delta the ego applied last
    tick, 0 before its first step and after a respawn).  The script's OtherAgentsPrediction is called without the
    steering_angle its constructor requires (TypeError at :145) and its step doubles the speed every sample
    (lib/other_agents_prediction.py:26); its comment says constant speed, which a = 0 gives;
  * tmp_trajectory[j] starts as None: the list of [] at :86 fails on the first index;
  * the `break` on is_goal at :121 becomes the respawn rule of the device loop (the ego restarts from its spawn pose with a
    new controller, progress index 0 and no previous path), or the recording would stop at the first goal;
  * `simulation.step` at :190 becomes the ego's own simulation[j].step (with the xref deviation of a successful solve, as
    mpc_intersection.py:163), and `Simulation[j].MAX_SPEED` at :134-140 becomes Simulation.MAX_SPEED;
  * `for k, _ in other_agents` at :152 becomes the other egos' states, ego_vehicles[:j] + ego_vehicles[j+1:] in order.
The motion primitives are regenerated from the reference's recipe and `cvxpy` is the recording stand-in
tests/golden/cvxpy_recorder.py, exactly as in make_golden_loop_real.py.  The script's own pair of egos already conflicts on
enough ticks (asserted below: at least 10 ticks where an ego's path is cut by the other), so no ego is added.

Stored per tick and per ego: the state, progress index in / out, previous / new path length, collision flag, target_ind in /
out, solver status, (delta, a), a respawn flag, and the ego's predicted trajectory (x, y, yaw) that the others saw.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

EGOS = ((1, 1), (3, 2))      # Ego_instance(start_position, turn_indicator), interactive_mpc.py:47-50
N_TICKS = 150
# columns of `ticks` [N_TICKS][n_egos][COLS]
COLS = ("x", "y", "yaw", "v", "idx_in", "prev_len", "idx_out", "path_len", "hit", "tind_in", "tind_out", "status", "delta",
        "accel", "respawned")


def main():
    import make_golden_refqp as RQ
    refmpc, rec = RQ.import_reference(13)
    from make_golden_planner import reference_primitives
    from envs.intersection import intersection
    from lib.car_dimensions import BicycleModelDimensions
    from lib.collision_avoidance import check_collision_moving_cars, get_cutoff_curve_by_position_idx
    from lib.moving_obstacles_prediction import MovingObstaclesPrediction
    from lib.mp_search_ww_generic import MotionPrimitiveSearch
    from lib.simulation import HistorySimulation, Simulation, State
    from lib.trajectories import calc_nearest_index_in_direction, resample_curve
    MPC, MAX_ACCEL = refmpc.MPC, refmpc.MAX_ACCEL

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
    EXTRA_CUTOFF_MARGIN = 4 * int(math.ceil(car.radius / dl))

    def fresh(j):
        mpc = MPC(cx=paths[j][:, 0], cy=paths[j][:, 1], cyaw=paths[j][:, 2], dl=dl, dt=DT, car_dimensions=car)
        st = State(x=paths[j][0, 0], y=paths[j][0, 1], yaw=paths[j][0, 2], v=0.0)
        return mpc, st, HistorySimulation(car_dimensions=car, sample_time=DT, initial_state=st)

    mpc, state, simulation = [None] * n, [None] * n, [None] * n
    for j in range(n):
        mpc[j], state[j], simulation[j] = fresh(j)
    traj_agent_idx, tmp_trajectory, delta = [0] * n, [None] * n, [0.0] * n
    ticks = np.zeros((N_TICKS, n, len(COLS)))
    preds = None
    mate_cuts = 0
    for i in range(N_TICKS):
        respawned = [False] * n
        for j in range(n):
            if mpc[j].is_goal(state[j]):                             # :121 -> respawn
                mpc[j], state[j], simulation[j] = fresh(j)
                traj_agent_idx[j], tmp_trajectory[j], delta[j] = 0, None, 0.0
                respawned[j] = True
        # every ego as the others see it, from the tick-start states
        trajs = [np.vstack(MovingObstaclesPrediction(state[k].x, state[k].y, state[k].v, state[k].yaw, 0.0, delta[k],
                                                     sample_time=DT, car_dimensions=car).state_prediction(TIME_HORIZON)).T
                 for k in range(n)]
        if preds is None:
            preds = np.zeros((N_TICKS, n, len(trajs[0]), 3))
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
            preds[i, j] = trajs[j][:, :3]
            step_out.append((d, a, dev))
        for j in range(n):                                           # :188-190, after every ego has solved
            d, a, dev = step_out[j]
            delta[j] = d
            state[j] = simulation[j].step(a=a, delta=d, xref_deviation=dev)
    assert mate_cuts >= 10, mate_cuts
    final = np.array([[s.x, s.y, s.yaw, s.v] for s in state])
    np.savez_compressed(os.path.join(HERE, "loop_interact_T13.npz"), ticks=ticks, preds=preds, final=final,
                        egos=np.array(EGOS, dtype=np.int64), planned0=planned[0], planned1=planned[1],
                        smoothed0=paths[0], smoothed1=paths[1], dl=np.float64(dl), margin=np.int64(EXTRA_CUTOFF_MARGIN),
                        frame_window=np.int64(FRAME_WINDOW), cols=np.array(COLS))
    print(f"interacting egos {EGOS}: routes of {[len(p) for p in planned]} points (dl = {dl:.6f}), {N_TICKS} ticks, "
          f"ticks cut by the other ego: {mate_cuts}, respawns: {int(ticks[:, :, 14].sum())}, "
          f"failed solves: {int(ticks[:, :, 11].sum())}")


if __name__ == "__main__":
    main()
