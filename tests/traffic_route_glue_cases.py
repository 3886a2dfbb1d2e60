"""The workload of tests/test_gpu_traffic_route_glue.py: 40 egos on the planned intersection routes, each
with a traffic set of its own in which route vehicles (kind="route") drive where the ego drives -- a slower leader on the ego's own
route that stops inside the run, vehicles on a route that crosses the ego's in the junction (one waiting on a curved segment, one
that enters again at a period, one that leaves a short route and is parked at 10^6 m), eight vehicles of kinds 0 and 3 alternating
in both list orders, a vehicle that is parked from the first tick, and no vehicle at all.  Built from the routes and a seeded ego
pool alone: no device."""
import dataclasses

import numpy as np

K = 60                                            # ticks
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
N_LEAD, N_CROSS, N_MIXED, N_GONE = 8, 8, 4, 4     # base egos per group; leaders, mixed and gone are used twice
GROUPS = ("leader_car",) * N_LEAD + ("leader_cyclist",) * N_LEAD + ("crossing",) * N_CROSS + ("mixed",) * N_MIXED + \
         ("mixed_reversed",) * N_MIXED + ("gone",) * N_GONE + ("empty",) * N_GONE
B = len(GROUPS)
LEAD_AHEAD, LEAD_RUN, LEAD_SPEED = 12.0, 10.0, 2.5      # the leader starts 12 m ahead, drives 10 m at 2.5 m/s (20 ticks) and stops
PERIOD_S = 4.0


def T_INT(d, turn, kmh, off, **kw):
    return dict(direction=d, turning=turn, speed=kmh / 3.6, offset=off, **kw)


def arc(route):
    return np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(route[:, 0]), np.diff(route[:, 1])))])


def crossings(routes, p, i0):
    """The routes that cross route p ahead of its point i0 at an angle, from another approach: [(q, i on p, j on q)]."""
    P = routes[p]
    out = []
    for q, Q in enumerate(routes):
        if q == p or np.hypot(*(Q[0, :2] - P[0, :2])) < 5.0:
            continue
        d = np.hypot(P[i0:, None, 0] - Q[None, :, 0], P[i0:, None, 1] - Q[None, :, 1])
        i, j = np.unravel_index(int(d.argmin()), d.shape)
        turn = abs((P[i0 + i, 2] - Q[j, 2] + np.pi) % (2 * np.pi) - np.pi)
        if d[i, j] < 0.1 and 0.5 < turn < np.pi - 0.5 and j >= 2:
            out.append((q, i0 + int(i), int(j)))
    return out


def leader(full, S, i0, **kw):
    """On the ego's own route, LEAD_AHEAD m ahead of its start, on the prefix that ends LEAD_RUN m further: it stops there."""
    s0 = float(S[i0]) + LEAD_AHEAD
    n = int(np.searchsorted(S, s0 + LEAD_RUN)) + 1
    return dict(kind="route", route=full[:n], speed=LEAD_SPEED, s0=s0, end="stop", **kw)


def crossing_vehicles(routes, S_ego, i0, cands):
    """(waiting, periodic, leaving) for an ego at point i0 of its route (arc lengths S_ego) and its crossings `cands`."""
    curve = []
    for q, i, j in cands:                             # the most curved segment ahead of a crossing: the waiting vehicle stands on it
        Q, Sq = routes[q], arc(routes[q])
        ds = np.diff(Sq[:j + 1])
        c = np.where(ds > 0, np.abs(np.diff(Q[:j + 1, 2])) / np.where(ds > 0, ds, 1.0), 0.0)
        curve.append((float(c.max()), q, int(c.argmax())))
    _, qa, seg = max(curve)
    Sa = arc(routes[qa])
    waiting = dict(kind="route", route=routes[qa], speed=5.0, offset=3.0, s0=float(0.5 * (Sa[seg] + Sa[seg + 1])))
    q, i, j = cands[0]
    Sq = arc(routes[q])
    t_ego = (S_ego[i] - S_ego[i0]) / 6.0 + 1.0        # about when the ego is there
    periodic = dict(kind="route", route=routes[q], speed=6.0, s0=max(0.0, float(Sq[j]) - 6.0 * t_ego), period=PERIOD_S)
    q, i, j = cands[-1]
    Sq = arc(routes[q])
    leaving = dict(kind="route", route=routes[q][:j + 40], speed=3.0, s0=max(0.0, float(Sq[j]) - 10.0), end="leave")
    return waiting, periodic, leaving


def workload(W, routes, T):
    """(batch of B egos, their B traffic sets, GROUPS): ego b meets set b.  The base egos are the first of a seeded pool that have
    30 m of route ahead and a crossing 6 .. 35 m ahead; a group that is used twice holds the same egos twice."""
    pool = W.ego_batch(routes, 400, T, rank=3)
    S = [arc(r) for r in routes]
    base = []
    for e in range(len(pool.path_id)):
        p = int(pool.path_id[e])
        i0 = int(np.hypot(routes[p][:, 0] - pool.x0[e, 0], routes[p][:, 1] - pool.x0[e, 1]).argmin())
        if S[p][-1] - S[p][i0] < 30.0:
            continue
        cands = [c for c in crossings(routes, p, i0) if 6.0 <= S[p][c[1]] - S[p][i0] <= 35.0]
        if cands:
            base.append((e, p, i0, cands))
        if len(base) == N_LEAD + N_CROSS + N_MIXED + N_GONE:
            break
    assert len(base) == N_LEAD + N_CROSS + N_MIXED + N_GONE, len(base)
    lead, cross = base[:N_LEAD], base[N_LEAD:N_LEAD + N_CROSS]
    mixed, gone = base[N_LEAD + N_CROSS:N_LEAD + N_CROSS + N_MIXED], base[N_LEAD + N_CROSS + N_MIXED:]
    egos, sets = [], []
    for dims in (None, CYCLIST):
        for e, p, i0, _ in lead:
            egos.append(e)
            sets.append([leader(routes[p], S[p], i0, **({"dims": dims} if dims else {}))])
    for e, p, i0, cands in cross:
        egos.append(e)
        sets.append(list(crossing_vehicles(routes, S[p], i0, cands)))
    both = []
    for e, p, i0, cands in mixed:
        w, per, lv = crossing_vehicles(routes, S[p], i0, cands)
        both.append([T_INT(1, False, 25, 2.0), leader(routes[p], S[p], i0), T_INT(-1, True, 20, 4.0, dims=CYCLIST), dict(per, dims=CYCLIST),
                     T_INT(-1, False, 30, 1.0), lv, T_INT(1, True, 22, 0.5, dims=CYCLIST), w])
    for rev in (False, True):
        for (e, _, _, _), st in zip(mixed, both):
            egos.append(e)
            sets.append(st[::-1] if rev else st)
    for parked in (True, False):
        for e, p, i0, cands in gone:
            egos.append(e)
            sets.append([dict(kind="route", route=routes[cands[0][0]][:60], speed=5.0, s0=50.0, end="leave")] if parked else [])
    idx = np.array(egos)
    batch = dataclasses.replace(pool, **{f.name: getattr(pool, f.name)[idx] for f in dataclasses.fields(pool)})
    assert len(sets) == B
    return batch, sets, GROUPS
