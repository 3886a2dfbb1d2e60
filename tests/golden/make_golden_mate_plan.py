#!/usr/bin/env python3
"""The plan rule of interacting egos, open loop: tests/golden/mate_plan.npz -- an ego's state and the controls its controller
holds (oa, od of its last solve, that solve's status, the steering applied last tick) rolled out by the reference's own
lib.simulation.Simulation.step, the circle centres by lib.trajectories.car_trajectory_to_collision_point_trajectories.  Build
machine only (needs the reference tree).

The rule (include/jsim_mpc.h) decides only WHICH input every step gets: with j = i + 1, a solved plan gives
(oa[j], od[j]) while j <= T - 1 and then (0, od[T - 1]); any other status gives (0, delta_last) throughout.  Everything else --
the steering clamp, the bicycle step with the speed from before the update, the speed clamps -- is Simulation.step, executed
unmodified.  Sample i is the state after step i.

Cases (name: what it is there for):
    hold_tail      T = 13, n_steps = 35: the plan ends inside the prediction, its last steering is held at constant speed
    long_plan      T = 40, n_steps = 35: the plan is longer than the prediction
    one_step       n_steps = 1
    all_lanes      n_steps = 64, T = 13: every lane of the wavefront has a step
    all_lanes_T40  n_steps = 64, T = 40
    T20            T = 20, n_steps = 35
    steer_clamp    steering beyond +-MAX_STEER, both signs, also in the held tail
    hit_max_speed  accelerates into MAX_SPEED
    hit_min_speed  reverses into MIN_SPEED
    failed         status 1: the plan (non-zero here) is ignored, (0, delta_last) throughout
    failed_clamp   status 2 and delta_last beyond MAX_STEER
    zero_plan      an all-zero plan (before the first solve, after a respawn): straight at constant speed, delta_last ignored
    stopping       brakes to v = 0 in three steps and stays there
Stored per case, padded with NaN to T_MAX / N_MAX: x0 (x, y, v, yaw), oa, od, status, delta_last, T, n_steps, pred (x, y, yaw),
cc [step][circle][2].
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
T_MAX, N_MAX = 40, 64
DT = 0.2


def smooth_plan(rng, T, a_scale=1.5, d_scale=0.3):
    """A plan as a solve leaves it: slowly varying accelerations and steering angles."""
    t = np.arange(T)
    oa = a_scale * np.sin(0.37 * t + rng.uniform(0, 6)) + rng.normal(0, 0.1, T)
    od = d_scale * np.sin(0.21 * t + rng.uniform(0, 6)) + rng.normal(0, 0.02, T)
    return oa, od


def cases():
    rng = np.random.default_rng(27)
    out = []

    def add(name, x0, oa, od, status, delta_last, n_steps):
        out.append(dict(name=name, x0=np.array(x0, dtype=np.float64), oa=np.array(oa, dtype=np.float64),
                        od=np.array(od, dtype=np.float64), status=int(status), delta_last=float(delta_last), n_steps=int(n_steps)))

    add("hold_tail", (12.5, -3.25, 4.0, 0.4), *smooth_plan(rng, 13), 0, 0.11, 35)
    add("long_plan", (-20.0, 7.5, 5.5, 2.9), *smooth_plan(rng, 40), 0, -0.2, 35)
    add("one_step", (3.0, 4.0, 6.0, -1.2), *smooth_plan(rng, 13), 0, 0.05, 1)
    add("all_lanes", (-55.0, 41.0, 3.0, 5.5), *smooth_plan(rng, 13), 0, 0.3, 64)
    add("all_lanes_T40", (80.0, -60.0, 2.0, -3.0), *smooth_plan(rng, 40), 0, 0.0, 64)
    add("T20", (1.5, 2.5, 7.0, 1.0), *smooth_plan(rng, 20), 0, 0.0, 35)
    oa, od = smooth_plan(rng, 13)
    od = np.array([0.2, 1.2, -1.1, 0.9, -0.95, 0.3, 0.79, -0.79, 2.0, -2.0, 0.1, 0.5, 1.0])
    add("steer_clamp", (0.0, 0.0, 3.5, 0.7), oa * 0.3, od, 0, 0.0, 35)
    add("hit_max_speed", (5.0, 5.0, 7.5, 0.2), np.full(13, 2.0), smooth_plan(rng, 13)[1], 0, 0.0, 35)
    add("hit_min_speed", (5.0, -5.0, -4.3, 3.3), np.full(13, -3.0), smooth_plan(rng, 13)[1], 0, 0.0, 35)
    add("failed", (-8.0, 2.0, 4.5, -0.6), *smooth_plan(rng, 13), 1, 0.27, 35)
    add("failed_clamp", (9.0, -9.0, 2.5, 1.9), *smooth_plan(rng, 13), 2, -1.3, 35)
    add("zero_plan", (20.0, 10.0, 5.0, 2.2), np.zeros(13), np.zeros(13), 0, 0.4, 35)
    oa = np.zeros(13)
    oa[1:4] = -5.0                                              # v = 3: 3 - 3 * (5 * 0.2) = 0 after three steps
    add("stopping", (-3.0, -30.0, 3.0, np.pi / 2), oa, np.full(13, 0.05), 0, 0.05, 35)
    return out


def rollout(case, car):
    """The reference's Simulation stepped n_steps times under the rule's inputs; returns (pred [n][3], cc [n][2][2], speeds)."""
    from lib.simulation import Simulation, State
    from lib.trajectories import car_trajectory_to_collision_point_trajectories
    x, y, v, yaw = case["x0"]
    sim = Simulation(car_dimensions=car, sample_time=DT, initial_state=State(x=x, y=y, yaw=yaw, v=v))
    oa, od, T = case["oa"], case["od"], len(case["oa"])
    pred, speeds = [], []
    for i in range(case["n_steps"]):
        j = i + 1
        if case["status"] == 0:
            a, d = (oa[j], od[j]) if j <= T - 1 else (0.0, od[T - 1])
        else:
            a, d = 0.0, case["delta_last"]
        s = sim.step(a=a, delta=d)
        pred.append((s.x, s.y, s.yaw))
        speeds.append(s.v)
    pred = np.array(pred)
    cc = np.stack([t[:, :2] for t in car_trajectory_to_collision_point_trajectories(pred, car)], axis=1)
    return pred, cc, np.array(speeds)


def main():
    import make_golden_refqp as RQ
    if RQ.REF_MAIN not in sys.path:
        sys.path.insert(0, RQ.REF_MAIN)
    import matplotlib
    matplotlib.use("Agg")
    from lib.car_dimensions import BicycleModelDimensions
    from lib.simulation import Simulation
    car = BicycleModelDimensions(skip_back_circle_collision_checking=False)
    cs = cases()
    n = len(cs)
    x0, oa, od = np.zeros((n, 4)), np.full((n, T_MAX), np.nan), np.full((n, T_MAX), np.nan)
    pred, cc = np.full((n, N_MAX, 3), np.nan), np.full((n, N_MAX, 2, 2), np.nan)
    for k, c in enumerate(cs):
        p, q, v = rollout(c, car)
        T, ns = len(c["oa"]), c["n_steps"]
        x0[k], oa[k, :T], od[k, :T], pred[k, :ns], cc[k, :ns] = c["x0"], c["oa"], c["od"], p, q
        # every case does what it is there for
        if c["name"] == "steer_clamp":
            assert np.abs(c["od"][1:]).max() > Simulation.MAX_STEER and abs(c["od"][-1]) > Simulation.MAX_STEER
        if c["name"] == "hit_max_speed":
            assert v[0] < Simulation.MAX_SPEED and v[-1] == Simulation.MAX_SPEED
        if c["name"] == "hit_min_speed":
            assert v[0] > Simulation.MIN_SPEED and v[-1] == Simulation.MIN_SPEED
        if c["name"] == "stopping":
            assert v[1] > 0 and np.all(v[2:] == 0.0) and np.all(p[3:] == p[3])
        if c["name"] == "zero_plan":
            assert np.all(p[:, 2] == c["x0"][3])
        if c["name"] == "failed_clamp":
            assert abs(c["delta_last"]) > Simulation.MAX_STEER
        print(f"{c['name']:14s} T = {T:2d} n_steps = {ns:2d} status {c['status']}  end pose ({p[-1, 0]:+9.3f}, {p[-1, 1]:+9.3f}, "
              f"{p[-1, 2]:+7.3f})  end speed {v[-1]:+.3f}")
    np.savez_compressed(os.path.join(HERE, "mate_plan.npz"), names=np.array([c["name"] for c in cs]), x0=x0, oa=oa, od=od,
                        status=np.array([c["status"] for c in cs], dtype=np.int64),
                        delta_last=np.array([c["delta_last"] for c in cs]), T=np.array([len(c["oa"]) for c in cs], dtype=np.int64),
                        n_steps=np.array([c["n_steps"] for c in cs], dtype=np.int64), pred=pred, cc=cc, dt=np.float64(DT))


if __name__ == "__main__":
    main()
