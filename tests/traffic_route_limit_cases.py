"""Route tables at their limits, shared by tests/test_traffic_route_limits_cpu.py and
tests/test_gpu_traffic_route_limits.py: tables of 64, 65 and 129 routes -- one, two and three 64-thread blocks of route_arclen_kernel,
the last block full, holding one route, holding one route more than the table's -- whose lengths cycle through 0, 1, 2, 5, 64, 65
and 300 points, a table whose last route is empty (its points would start one past the allocation), a table without any point, and
a route of 2049 points (a bisection 11 steps deep) that is driven at 37 segments a tick.  Everything is a closed form of the route
index: no RNG, no planner, no device."""
import numpy as np

import traffic_route_numpy as TR

DT, K = 0.2, 45                                   # the tick of the param rows, the ticks every test runs
LENGTHS = (0, 1, 2, 5, 64, 65, 300)               # route r has LENGTHS[(r + 4) % 7] points: routes 0, 63, 64, 128 have 64, 64, 65, 300
SPACING = 0.3                                     # metres between the points of those routes
LONG_N, LONG_SPACING = 2049, 0.098                # the long route: 2048 segments of 0.098 m, 200.7 m
FAR = (0, 63, 64, 128)                            # the routes at the blocks' edges whose vehicles must never be taken for one another


def n_points(r):
    return LENGTHS[(r + 4) % 7]


def arc(n, radius, spacing, left):
    """n points on a circle of `radius`, `spacing` apart along it, from the origin heading +x; yaw = the tangent's, continuous."""
    a = np.arange(n) * (spacing / radius) * (1.0 if left else -1.0)
    return np.column_stack([radius * np.sin(np.abs(a)), (1.0 if left else -1.0) * radius * (1.0 - np.cos(a)), a])


def lane(n, spacing, amp, wave):
    """n points of the lane y = amp sin(x / wave), `spacing` apart in x, with the tangent's yaw."""
    x = np.arange(n) * spacing
    return np.column_stack([x, amp * np.sin(x / wave), np.arctan((amp / wave) * np.cos(x / wave))])


def route(r):
    """Route r, [n_points(r), 3]: an arc (even r) or a sine-shaped lane (odd r), shifted by r metres to the left and r
    metres up.  A 300-point arc of radius 7 .. 11 m turns through 8 .. 13 rad, so its yaw runs past pi; a one-point route has yaw
    0.1 + 0.01 r."""
    n = n_points(r)
    if n == 0:
        return np.zeros((0, 3))
    p = arc(n, 7.0 + r % 5, SPACING, r % 4 == 0) if r % 2 == 0 else lane(n, SPACING, 1.0 + 0.25 * (r % 3), 4.0 + r % 5)
    if n == 1:
        p[0, 2] = 0.1 + 0.01 * r
    return p + [-float(r), float(r), 0.0]


def long_route(shift=0.0):
    """The 2049-point route: an arc of radius 40 m through 5.02 rad (past pi), shifted by `shift` metres."""
    return arc(LONG_N, 40.0, LONG_SPACING, True) + [-50.0 + shift, 20.0 + shift, 0.0]


def vehicle(r):
    """The vehicle of route r: end, start delay, s0, speed and period cycle with r at periods 2, 3, 4, 6 and 5.  At 0.5 .. 1.5 m/s
    a vehicle covers at most 13.5 m in 45 ticks: it stays on a route of >= 64 points (>= 18.9 m, s0 <= 0.9) and reaches the end of
    one of 2 or 5 points (0.3 and 1.2 m)."""
    return dict(route=r, end=r % 2, speed=0.5 + 0.2 * (r % 6), offset=(0.0, 0.3, 1.0)[r % 3], s0=0.3 * (r % 4), dt=DT,
                period=(0, 0, 11, 0, 23)[r % 5])


def long_vehicles(r, S_end):
    """name -> the vehicles of the long route (index r, length S_end): `fast` passes 18 * 0.2 / 0.098 = 36.7 vertices a tick and
    wraps every 9 ticks, `slow` needs 1.6 ticks for a segment, `still` stands on a curved segment for ever (v = 0, steer != 0), the
    two `last_*` start on the last segment and reach the end on their third moving tick."""
    base = dict(route=r, end=0, offset=0.0, s0=0.0, dt=DT, period=0)
    return {"fast": dict(base, speed=18.0, period=9),
            "slow": dict(base, speed=0.3, s0=1.0, offset=0.5),
            "still": dict(base, speed=0.0, s0=77.7),
            "last_stop": dict(base, speed=0.1, s0=S_end - 0.05, end=1),
            "last_leave": dict(base, speed=0.1, s0=S_end - 0.05, end=0)}


def tables():
    """name -> (routes, vehicle dicts): `r64`, `r65`, `r129` with one vehicle per route; `last_empty`: r65 with its last route
    emptied; `all_empty`: 65 routes without a point; `long`: r129 and the 2049-point route, 130 routes with 134 vehicles."""
    out = {}
    for n in (64, 65, 129):
        out[f"r{n}"] = ([route(r) for r in range(n)], [vehicle(r) for r in range(n)])
    out["last_empty"] = ([route(r) for r in range(64)] + [np.zeros((0, 3))], [vehicle(r) for r in range(65)])
    out["all_empty"] = ([np.zeros((0, 3)) for _ in range(65)], [vehicle(r) for r in range(65)])
    lr = long_route()
    out["long"] = ([route(r) for r in range(129)] + [lr],
                   [vehicle(r) for r in range(129)] + list(long_vehicles(129, TR.arc_length(lr)[-1]).values()))
    return out


def pack(routes):
    """(x, y, yaw [points], off [n + 1] int32) of a table as jsim_loop_set_traffic_routes takes it; a table without a point gives
    arrays of one unused element, so that their pointers are not null."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in routes])]).astype(np.int32)
    cat = np.concatenate([np.zeros((0, 3))] + [np.asarray(r, dtype=np.float64).reshape(-1, 3) for r in routes], axis=0)
    if cat.shape[0] == 0:
        cat = np.zeros((1, 3))
    return tuple(np.ascontiguousarray(cat[:, i]) for i in range(3)) + (off,)


def restated(routes, vehicles, L, n_ticks=K):
    """TR.run on a table's vehicles with wheelbase L: (get_all [n_ticks][n][6], the final state [n][4], the param rows [n][8])."""
    param = TR.case_rows(vehicles)
    get, state = TR.run(routes, np.zeros((len(vehicles), 4)), param, np.full(len(vehicles), float(L)), n_ticks)
    return get, state, param


def branch(routes, k, c):
    """Which branch of items 5 - 7 vehicle k takes at counter c: "moving", "waiting" (item 5 with v = speed / v = 0 before its
    start tick), "stop", "leave" (item 6), "one_point", "empty" (item 7)."""
    p = routes[k["route"]]
    if len(p) < 2:
        return "one_point" if len(p) == 1 else "empty"
    cc, n0, s = TR.arc_at(c, k["speed"], k["offset"], k["s0"], k["dt"], k["period"])
    if s < TR.arc_length(p)[-1]:
        return "moving" if cc >= n0 else "waiting"
    return "stop" if k["end"] == 1 else "leave"


# ---- the ScenarioLoop of the rollout test: 17 sets of 8 route vehicles on 136 distinct routes, none of them empty (a spec's
# route has a point: route_array refuses one without)
N_SETS, PER_SET = 17, 8


def loop_specs():
    """(sets [17][8] of kind="route" specs, the flat vehicle dicts): the first 131 routes that have a point with their vehicles,
    and the five vehicles of the long route on a copy of it each, a metre apart -- 136 vehicles on 136 distinct routes, three
    blocks of route_arclen_kernel and of obstacle_rollout_kernel."""
    idx = [r for r in range(200) if n_points(r) > 0][:N_SETS * PER_SET - 5]
    flat = [(route(r), vehicle(r)) for r in idx]
    for i, name in enumerate(("fast", "slow", "still", "last_stop", "last_leave")):
        lr = long_route(float(i))
        flat.append((lr, long_vehicles(0, TR.arc_length(lr)[-1])[name]))
    specs = [dict(kind="route", route=p, speed=k["speed"], offset=k["offset"] or None, s0=k["s0"], end=("leave", "stop")[k["end"]],
                  period=k["period"] * DT if k["period"] else None) for p, k in flat]
    return [specs[lo:lo + PER_SET] for lo in range(0, len(specs), PER_SET)], [k for _, k in flat]
