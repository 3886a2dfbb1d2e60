"""Numpy restatement of the two calls a fork starts from, written from the contract and used by the tests as
the CPU side of jsim_loop_fork_state and jsim_loop_obstacles_at: the ego's state at the start of a recorded tick with the first tick
of that tick's episode, and the scripted vehicles of main/lib/moving_obstacles.py advanced tick by tick in the loops' two calls --
get() alone, then get() + step()."""
import math

import numpy as np

from recorder_numpy import is_end


def fork_state(rec, flags, x_first, x_spawn, ego, at):
    """rec [n][B][7] (x, y, yaw, v, ...), flags [n][B], x_first / x_spawn [B][4] (x, y, v, yaw); ego, at [R] with 0 <= at <= n.
    Returns x0 [R][4] (x, y, v, yaw) and k0 [R]."""
    rec, flags = np.asarray(rec, dtype=np.float64), np.asarray(flags)
    x0, k0 = np.empty((len(ego), 4)), np.zeros(len(ego), dtype=np.int32)
    for r, (e, k) in enumerate(zip(ego, at)):
        if k == 0:
            x0[r] = x_first[e]
        elif is_end(flags[k - 1, e]):
            x0[r] = x_spawn[e]
        else:
            x0[r] = rec[k - 1, e, [0, 1, 3, 2]]
        j = k - 1
        while j >= 0 and not is_end(flags[j, e]):          # the last end before `at`
            j -= 1
        k0[r] = j + 1
    return x0, k0


def start_states(specs):
    """(state0 [n][4] = xc, yc, theta, counter; param [n][8]) of ScriptedObstacles' spec dicts at dt = 0.2, from the reference classes'
    constructors."""
    kinds = {"t_intersection": 0.0, "roundabout": 1.0, "arterial": 2.0}
    st, pr = [], []
    for s in specs:
        kind = s.get("kind", "t_intersection")
        off = s.get("offset")
        off = float(off) if (off is not None and off > 0) else 0.0
        if kind == "arterial":
            st.append([s["x_init"], s["y_init"], math.pi / 2, 0.0])
            pr.append([1.0, 0.0, s["speed"], off, 0.0, 0.2, 2.0, s["initial_speed"]])
        elif s["direction"] >= 0:
            st.append([-30.0, -3.0, 0.0, 0.0])
            pr.append([1.0, float(bool(s["turning"])), s["speed"], off, -10.0, 0.2, kinds[kind], 0.0])
        else:
            st.append([30.0, 3.0, math.pi, 0.0])
            pr.append([-1.0, float(bool(s["turning"])), s["speed"], off, 12.0, 0.2, kinds[kind], 0.0])
    return np.array(st, dtype=np.float64).reshape(-1, 4), np.array(pr, dtype=np.float64).reshape(-1, 8)


def _one_call(s, p, L, step):
    """One evaluation of a vehicle's get() (step: followed by step()) on its state s, in place; returns the get() tuple."""
    xc, yc, th, cnt = s
    d, turning, speed, offs, x_turn, dt, kind, v0 = p
    th_get = th
    waited = not (offs > 0.0)
    if kind == 1.0:
        steer = 0.0
        if turning:
            A = math.atan((1.0 / 5.0) * 2.86)
            if d > 0:
                if -7.0 <= xc <= -4.0 and yc < 0.0: steer = -A
                if -3.0 < xc: steer = A
                if yc > 0.0 and -5.0 <= xc <= -3.0: steer = -A
                if xc <= -3.0 and yc > 0.0: th, steer = -math.pi, 0.0
            else:
                if 4.0 <= xc <= 7.0 and yc > 0.0: steer = -A
                if xc < 3.0: steer = A
                if yc < 0.0 and 3.0 <= xc <= 5.0: steer = -A
                if 3.0 <= xc and yc < 0.0: th, steer = 0.0, 0.0
        v = speed if (waited or cnt > offs / 0.2) else 0.0
    elif kind == 2.0:
        steer = 0.0
        v = speed if (waited or cnt > offs / dt) else v0
    else:
        steer = 0.0
        if turning:
            if d > 0:
                steer = -0.38 if (xc >= x_turn and th > -math.pi / 2) else 0.0
            else:
                steer = 0.19 if (xc <= x_turn and th < 3 * math.pi / 2) else 0.0
        v = speed if (waited or cnt > offs / dt) else 0.0
    get = (xc, yc, v, th_get, 0.0, steer)
    if step:
        xd, yd, thd = v * math.cos(th), v * math.sin(th), (v / L) * math.tan(steer)
        xc, yc, th, cnt = xc + xd * dt, yc + yd * dt, th + thd * dt, cnt + 1.0
    s[:] = xc, yc, th, cnt
    return get


def obstacles_at(state0, param, wheelbase, ticks, L=2.86, trace=False):
    """state [n][4] after ticks[o] ticks from state0 (wheelbase [n] or None: L for all).  trace: also the get() tuples of every tick's
    first call, a list per vehicle."""
    state = np.array(state0, dtype=np.float64).reshape(-1, 4)
    gets = []
    for o in range(len(state)):
        Lo = L if wheelbase is None else float(wheelbase[o])
        row = []
        for _ in range(int(ticks[o])):
            row.append(_one_call(state[o], param[o], Lo, False))
            _one_call(state[o], param[o], Lo, True)
        gets.append(row)
    return (state, gets) if trace else state
