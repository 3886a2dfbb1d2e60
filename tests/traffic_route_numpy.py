"""numpy restatement of the route vehicle's rule (kind 3 of the scripted obstacle tables; include/jsim_mpc.h states it above
jsim_loop_set_traffic_routes, the item numbers below are its): the arc length of a route, the pose at a counter in closed form, and
the get() / step() calls of jsim_loop_obstacles on (state, param) rows.  Independent of the package: plain numpy, fp64, the
header's order of operations."""
import math

import numpy as np

PARK = 1.0e6          # JSIM_ROUTE_PARK
SNAP = 1e-9


def arc_length(route):
    """S [N] of a route [N, >= 2]: S[0] = 0, S[j] = S[j-1] + sqrt(dx^2 + dy^2), summed in index order."""
    r = np.asarray(route, dtype=np.float64)
    S = np.zeros(r.shape[0])
    for j in range(1, r.shape[0]):
        dx, dy = r[j, 0] - r[j - 1, 0], r[j, 1] - r[j - 1, 1]
        S[j] = S[j - 1] + np.sqrt(dx * dx + dy * dy)
    return S


def start_tick(offset, dt):
    """n0 of item 2: the first counter at which the vehicle moves."""
    return int(math.floor(offset / dt)) + 1 if offset > 0 else 0


def arc_at(c, speed, offset, s0, dt, period):
    """(c', n0, s) of items 1-4 at counter c."""
    c = int(c)
    if period >= 1:
        c = c % int(period)
    n0 = start_tick(offset, dt)
    m = max(0, c - n0)
    return c, n0, s0 + float(m) * (speed * dt)


def segment(S, s):
    """Item 5's index by bisection, with the snap: (j, whether the snap moved it)."""
    n = len(S)
    j = min(int(np.searchsorted(S, s, side="right")) - 1, n - 2)      # the largest j with S[j] <= s, j <= n - 2
    j = max(j, 0)
    if j + 1 <= n - 2 and S[j + 1] - s <= SNAP:
        return j + 1, True
    return j, False


def pose(route, S, c, end, speed, offset, s0, dt, period, L):
    """(x, y, v, yaw, 0, steer): the get() tuple at counter c.  route [N, 3] with a continuous yaw, S = arc_length(route)."""
    route = np.asarray(route, dtype=np.float64).reshape(-1, 3)
    n = route.shape[0]
    c, n0, s = arc_at(c, speed, offset, s0, dt, period)
    if n < 2:                                                           # 7
        p = route[0] if n == 1 else np.zeros(3)
        return np.array([p[0], p[1], 0.0, p[2], 0.0, 0.0])
    if s < S[-1]:                                                       # 5
        j, _ = segment(S, s)
        a, q = route[j], route[j + 1]
        ds = S[j + 1] - S[j]
        f = (s - S[j]) / ds if ds > 0 else 0.0
        x, y, yaw = a[0] + f * (q[0] - a[0]), a[1] + f * (q[1] - a[1]), a[2] + f * (q[2] - a[2])
        v = speed if c >= n0 else 0.0
        steer = math.atan((L * (q[2] - a[2])) / ds) if ds > 0 else 0.0
        return np.array([x, y, v, yaw, 0.0, steer])
    if int(end) == 1:                                                   # 6
        return np.array([route[-1, 0], route[-1, 1], 0.0, route[-1, 2], 0.0, 0.0])
    return np.array([PARK, PARK, 0.0, 0.0, 0.0, 0.0])


def param_row(route_index, end, speed, offset, s0, dt, period_ticks):
    return [float(route_index), float(end), float(speed), float(offset) if offset and offset > 0 else 0.0, float(s0), float(dt), 3.0,
            float(period_ticks)]


def call(routes, lengths, state, param, wheelbase, step):
    """One jsim_loop_obstacles call on the kind-3 rows of (state [n][4], param [n][8]), in place: returns get [n][6] (rows of other
    kinds: NaN).  routes: the table's arrays, lengths: their arc_length; wheelbase [n]."""
    get = np.full((len(state), 6), np.nan)
    for o, (st, pr) in enumerate(zip(state, param)):
        if int(pr[6]) != 3:
            continue
        r = min(max(int(pr[0]), 0), len(routes) - 1)                    # 8
        args = (routes[r], lengths[r])
        rest = (pr[1], pr[2], pr[3], pr[4], pr[5], pr[7], wheelbase[o])
        g = pose(*args, st[3], *rest)
        get[o] = g
        if step:
            st[3] += 1.0
            g = pose(*args, st[3], *rest)
        st[0], st[1], st[2] = g[0], g[1], g[3]
    return get


def run(routes, state, param, wheelbase, n_ticks):
    """n_ticks ticks of the loops' two calls -- get(), then get() + step(): (get_all [n_ticks][n][6], the final state)."""
    lengths = [arc_length(r) for r in routes]
    state = np.array(state, dtype=np.float64).reshape(-1, 4)
    out = []
    for _ in range(n_ticks):
        call(routes, lengths, state, param, wheelbase, False)
        out.append(call(routes, lengths, state, param, wheelbase, True))
    return np.array(out).reshape(n_ticks, len(state), 6), state


def stepped(route, n_ticks, end, speed, offset, s0, dt, period, L):
    """The get() tuples of counters 0 .. n_ticks - 1 by stepping ONE counter at a time from a carried arc length, without the closed
    form in the counter: s advances by speed * dt on every moving tick and returns to s0 on a wrap.  (Sums instead of one product:
    equal to `pose` to rounding, not to the bit.)"""
    route = np.asarray(route, dtype=np.float64).reshape(-1, 3)
    S = arc_length(route)
    n0 = start_tick(offset, dt)
    out, c, s = [], 0, s0
    for _ in range(n_ticks):
        moving = c >= n0
        if route.shape[0] < 2:
            p = route[0] if route.shape[0] == 1 else np.zeros(3)           # 7 (an empty route: at the origin)
            g = [p[0], p[1], 0.0, p[2], 0.0, 0.0]
        elif s < S[-1]:
            j = 0
            while j + 1 <= len(S) - 2 and S[j + 1] <= s:
                j += 1
            if j + 1 <= len(S) - 2 and S[j + 1] - s <= SNAP:
                j += 1
            ds = S[j + 1] - S[j]
            f = (s - S[j]) / ds if ds > 0 else 0.0
            p = route[j] + f * (route[j + 1] - route[j])
            g = [p[0], p[1], speed if moving else 0.0, p[2], 0.0, math.atan(L * (route[j + 1, 2] - route[j, 2]) / ds) if ds > 0 else 0.0]
        elif int(end) == 1:
            g = [route[-1, 0], route[-1, 1], 0.0, route[-1, 2], 0.0, 0.0]
        else:
            g = [PARK, PARK, 0.0, 0.0, 0.0, 0.0]
        out.append(g)
        c += 1
        if period >= 1 and c == int(period):
            c, s = 0, s0
        elif c > n0:
            s = s + speed * dt
    return np.array(out)


# ---- the table and the vehicles that the CPU and the device tests share
def case_routes():
    """Routes of 2, 3, 1, 64, 65 (with a zero-length segment: point 30 twice) and 129 points, [N, 3] with a continuous yaw."""
    def arc(n, radius, x0, y0, sweep):
        a = np.linspace(0.0, sweep, n)
        return np.column_stack([x0 + radius * np.sin(a), y0 + radius * (1.0 - np.cos(a)), a])
    r2 = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    r3 = np.array([[-5.0, 2.0, 0.0], [1.0, 2.0, 0.3], [4.0, 6.0, 0.9]])
    r1 = np.array([[7.0, -3.0, 0.5]])
    r64 = arc(64, 12.0, -20.0, -3.0, 1.7)
    r65 = np.insert(arc(64, 9.0, 5.0, 5.0, -2.9), 30, arc(64, 9.0, 5.0, 5.0, -2.9)[30], axis=0)
    r129 = np.column_stack([np.linspace(-30.0, 30.0, 129), 3.0 + 0.5 * np.sin(np.linspace(0.0, 7.0, 129)),
                            np.arctan(0.5 * np.cos(np.linspace(0.0, 7.0, 129)) * 7.0 / 60.0)])
    return [r2, r3, r1, r64, r65, r129]


def edge_cases():
    """name -> dict(route index into case_routes(), end, speed, offset, s0, dt, period ticks): item 3 of the issue's CPU tests."""
    routes = case_routes()
    S65, S129 = arc_length(routes[4]), arc_length(routes[5])
    below = np.nextafter(10.0, 0.0)
    c = {}
    c["offset_integer_ticks"] = dict(route=0, end=1, speed=2.0, offset=1.0, s0=0.0, dt=0.25, period=0)       # 1.0 / 0.25 = 4 exactly
    c["offset_fraction"] = dict(route=5, end=0, speed=5.5, offset=0.7, s0=0.0, dt=0.2, period=0)
    c["period_wraps"] = dict(route=5, end=0, speed=6.3, offset=0.0, s0=2.0, dt=0.2, period=7)
    c["period_with_offset"] = dict(route=3, end=1, speed=3.1, offset=0.5, s0=0.0, dt=0.2, period=12)
    c["period_after_leaving"] = dict(route=0, end=0, speed=7.0, offset=0.0, s0=0.0, dt=0.2, period=20)       # leaves at tick 8, back at 20
    for e in (0, 1):
        # speed * dt = 1 and a 10 m route: s is S_end exactly at m = 10; from s0 = 1 - 2^-49 it is one ulp below S_end at m = 9
        c[f"arrives_exactly_end{e}"] = dict(route=0, end=e, speed=4.0, offset=0.0, s0=0.0, dt=0.25, period=0)
        c[f"arrives_ulp_below_end{e}"] = dict(route=0, end=e, speed=4.0, offset=0.0, s0=below - 9.0, dt=0.25, period=0)
        c[f"stands_at_end{e}"] = dict(route=5, end=e, speed=0.0, offset=0.0, s0=S129[-1], dt=0.2, period=0)
        c[f"stands_ulp_below_end{e}"] = dict(route=5, end=e, speed=0.0, offset=0.0, s0=np.nextafter(S129[-1], 0.0), dt=0.2, period=0)
        c[f"s0_beyond_end{e}"] = dict(route=4, end=e, speed=3.0, offset=0.0, s0=S65[-1] + 1.0, dt=0.2, period=0)
        c[f"one_point_end{e}"] = dict(route=2, end=e, speed=5.0, offset=0.4, s0=0.0, dt=0.2, period=0)
    c["zero_length_segment_crossed"] = dict(route=4, end=0, speed=4.7, offset=0.0, s0=0.0, dt=0.2, period=0)
    c["zero_length_segment_stood_on"] = dict(route=4, end=1, speed=0.0, offset=0.0, s0=S65[30], dt=0.2, period=0)
    c["s0_positive"] = dict(route=3, end=1, speed=4.2, offset=0.0, s0=3.3, dt=0.2, period=0)
    c["three_points"] = dict(route=1, end=1, speed=1.3, offset=0.3, s0=0.0, dt=0.2, period=0)
    return c


def case_rows(cases):
    """param [n][8] of a list of case dicts."""
    return np.array([param_row(k["route"], k["end"], k["speed"], k["offset"], k["s0"], k["dt"], k["period"]) for k in cases], dtype=np.float64)


def golden_vehicles(g, dt=0.2):
    """(route [N, 3], speed, offset, get [140][6]) of the four T-intersection vehicles of tests/golden/obstacles_scripted.npz (g, loaded):
    the route is the vehicle's own recorded (x, y, yaw) from its first moving tick n0 on."""
    out = []
    for i in range(g["get"].shape[1]):
        off = float(g["offset"][i]) if g["offset"][i] > 0 else 0.0
        n0 = start_tick(off, dt)
        out.append((np.ascontiguousarray(g["get"][n0:, i][:, [0, 1, 3]]), float(g["speed"][i]), off, g["get"][:, i]))
    return out
