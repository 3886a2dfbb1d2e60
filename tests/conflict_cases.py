"""The cases of tests/golden/conflicts.npz: synthetic pose series for the clearance and first-contact
evaluation, chosen for the kernel's structure -- 64 ticks per chunk, an offset that reaches up to 20 ticks across a chunk edge and
is clamped to the episode's own first and last tick, a second sweep that carries one vehicle circle through an episode.  No RNG:
every pose series is piecewise linear over 200 ticks (a series may jump: a knot per tick), with the knots putting each event on the
tick the case is about.  Used by the fixture generator (tests/golden/make_golden_conflicts.py), which hands every episode to the
reference's own check_collision_moving_cars / check_collision_moving_bicycle, by the CPU test, which rebuilds the cases and
compares, and by the GPU test, which lays them out as recorder arrays: one ego per case, every case's vehicles in one table."""
import os

import numpy as np

import conflicts_numpy as CN
import recorder_numpy as RN
from recorder_numpy import AGE, GOAL

N = 200                                              # ticks per case
TICK_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)  # every case is also evaluated cut to these lengths
WINDOWS = (0, 1, 3, 20)


def shape_of(L, width, extra_length=0.64):
    """(cc_front, cc_rear, radius) as lib/car_dimensions.py computes them (the generator compares with the reference's classes)."""
    length = L + extra_length
    offset = length / 2 - width / 2
    return (L / 2 + offset, L / 2 - offset, width / (2 ** .5))


CAR, BIKE = shape_of(2.86, 2.0), shape_of(1.0, 0.45)   # BicycleModelDimensions, BicycleRealDimensions
SHAPES = {"car": CAR, "bike": BIKE}
FAR = (61.7, 58.3, 0.3)                              # where a vehicle waits that is to be met on chosen ticks only


def pw(knots, n=N):
    """Piecewise-linear through (tick, value) knots."""
    k, v = zip(*knots)
    assert all(b > a for a, b in zip(k, k[1:])), knots
    return np.interp(np.arange(n, dtype=np.float64), k, v)


def line(p0, p1, n=N):
    """A pose series from pose p0 at tick 0 to pose p1 at tick n - 1."""
    return np.stack([pw([(0, a), (n - 1, b)], n) for a, b in zip(p0, p1)], axis=1)


def still(p, n=N):
    return np.tile(np.asarray(p, dtype=np.float64), (n, 1))


def blip(base, pose, ticks):
    """`base` with `pose` on the given ticks only."""
    out = np.array(base, dtype=np.float64)
    out[list(ticks)] = pose
    return out


def respawning(spawn, step, ends, n=N):
    """An ego that starts every episode at `spawn` and moves by `step` per tick; ends = the ticks whose record ends an episode.
    Returns (poses [n][3], flags [n])."""
    poses, flags = np.empty((n, 3)), np.zeros(n, dtype=np.int32)
    k0 = 0
    for j, k in enumerate(list(ends) + [n - 1]):
        t = np.arange(k - k0 + 1, dtype=np.float64)[:, None]
        poses[k0:k + 1] = np.asarray(spawn)[None, :] + t * np.asarray(step)[None, :]
        if k in ends:
            flags[k] = (GOAL, AGE, GOAL | AGE)[j % 3]
        k0 = k + 1
    return poses, flags


def _case(label, ego, vehicles=(), kind="car", flags=None, restated=False, group=None):
    """vehicles: pose series [N][3]; kind: one name for all of them or one per vehicle; group: the label egos that are each
    other's mates share (consecutive cases)."""
    kinds = [kind] * len(vehicles) if isinstance(kind, str) else list(kind)
    assert len(kinds) == len(vehicles)
    return {"label": label, "ego": np.asarray(ego, dtype=np.float64), "vehicles": [np.asarray(v, dtype=np.float64) for v in vehicles],
            "kinds": kinds, "flags": np.zeros(N, dtype=np.int32) if flags is None else np.asarray(flags, dtype=np.int32),
            "restated": bool(restated), "group": group}


def cases():
    out = []
    h = np.pi / 2
    # 0: a crossing at an intersection: the ego eastbound, a car northbound through its lane, meeting around tick 100
    ego_east = line((-20.0, 0.13, 0.02), (19.8, 0.13, 0.02))
    out.append(_case("crossing at an intersection", ego_east, [line((3.1, -30.3, h - 0.01), (3.1, 29.4, h - 0.01))]))
    # 1-2: passing a 5 km/h cyclist, both northbound, the lateral gap just above and just below car radius + bicycle radius
    thr_cb = CAR[2] + BIKE[2]
    ego_north = line((0.0, -10.0, h), (0.0, -10.0 + 0.5 * (N - 1), h))
    cyc = lambda x: line((x, 20.0, h), (x, 20.0 + 5 / 3.6 * 0.1 * (N - 1), h))
    out.append(_case("cyclist passed with a gap just above the threshold", ego_north, [cyc(thr_cb + 0.02)], kind="bike"))
    out.append(_case("cyclist passed with a gap just below the threshold", ego_north, [cyc(thr_cb - 0.05)], kind="bike"))
    # 3: a contact that lasts a single frame
    creep = line((5.3, -2.7, 0.4), (7.3, -1.9, 0.45))
    out.append(_case("contact on a single frame (100)", creep, [blip(still(FAR), (8.9, -0.2, 2.1), [100])]))
    # 4: found only through an offset: on tick 100 the vehicle is where the ego is on ticks 99 and 101, and the ego is elsewhere
    out.append(_case("contact only through an offset (ticks 99 and 101)", blip(still((5.3, -2.7, 0.4)), (-50.0, -50.0, 0.4), [100]),
                     [blip(still(FAR), (8.9, -0.2, 2.1), [100])]))
    # 5: a westbound car stops behind the standing ego: its rear circle touches the ego's rear circle, the ego's front circle never
    # reaches that position -- the first hit of front ++ rear lies in the rear half, and modulo the length it is frame 0
    behind = np.stack([pw([(0, -12.0), (120, -1.32), (N, -1.32)]), np.full(N, 0.05), np.full(N, np.pi)], axis=1)
    out.append(_case("only the rear circle touches the hit position", still((0.0, 0.0, 0.0)), [behind]))
    # 6: a cyclist comes down onto the standing ego's front circle: the ego was within reach of that position from frame 0 on
    down = np.stack([np.full(N, 2.3), pw([(0, 40.0), (150, 1.2), (N, 1.2)]), np.full(N, -h)], axis=1)
    out.append(_case("hit_frame earlier than hit_tick", still((0.0, 0.0, 0.1)), [down], kind="bike"))
    # 7-12: contact on ticks 0, 62, 63, 64, 65 and on the last tick, nowhere else
    for j, k in enumerate((0, 62, 63, 64, 65, N - 1)):
        near = (creep[k, 0] + 2.4 + 0.1 * j, creep[k, 1] + 1.7 - 0.2 * j, 1.9 + 0.3 * j)
        out.append(_case(f"contact on tick {k} only", creep, [blip(still(FAR), near, [k])], kind="car" if j % 2 == 0 else "bike"))
    # 13-15: an episode ending on 62, 63, 64 while a car passes the spawn point (the contact spans the end)
    passing = line((-24.7, 2.1, 0.05), (27.1, 2.3, 0.05))
    for k in (62, 63, 64):
        ego, fl = respawning((-9.0, 0.0, 0.03), (0.011, 0.002, 0.0), [k])
        out.append(_case(f"episode ending on tick {k}", ego, [passing], flags=fl))
    # 16: an episode of length 1 (tick 101) inside a long contact
    ego, fl = respawning((0.9, 0.0, 0.03), (0.004, 0.0, 0.0002), [100, 101])
    out.append(_case("episode of length 1", ego, [passing], flags=fl))
    # 17: episodes of 5, 2, 1 and 3 ticks: every offset clamped at both ends, w = 20 on an episode of 5 ticks
    ego, fl = respawning((-22.6, 0.0, 0.03), (0.05, 0.01, 0.0), [4, 6, 7, 10])
    out.append(_case("episodes shorter than the window", ego, [line((-26.9, 2.2, 0.05), (52.0, 2.2, 0.05))], flags=fl))
    # 18-21: 0, 2 and 8 vehicles (1 is everywhere above); the eight as cyclists in a row and as cars on a ring
    out.append(_case("no vehicles", ego_east))
    out.append(_case("two cars", ego_east, [line((3.1, 29.4, -h), (3.1, -30.3, -h)), line((-6.2, -30.3, h + 0.02), (-6.2, 29.4, h + 0.02))]))
    row = [line((thr_cb + 0.4 - 0.15 * j, 4.0 + 9.0 * j, h), (thr_cb + 0.4 - 0.15 * j, 4.0 + 9.0 * j + 5 / 3.6 * 0.1 * (N - 1), h)) for j in range(8)]
    out.append(_case("eight cyclists in a row", ego_north, row, kind="bike"))
    ring = [line((9.0 * np.cos(0.7 * j) + 0.3 * j, 9.0 * np.sin(0.7 * j), 0.7 * j + h),
                 (1.5 * np.cos(0.7 * j + 1.0) + 0.3 * j, 1.5 * np.sin(0.7 * j + 1.0), 0.7 * j + h + 1.0)) for j in range(8)]
    out.append(_case("eight cars closing in", still((0.0, 0.0, 0.3)), ring))
    # restatement-made (no reference function takes a mixed list or a list of egos): a car and a cyclist in one list; two egos that
    # are each other's only vehicle, one of them respawning; a group of three with a scripted cyclist
    out.append(_case("a car and a cyclist in one list (restated)", ego_east,
                     [line((3.1, -30.3, h - 0.01), (3.1, 29.4, h - 0.01)), line((-4.0, thr_cb + 0.3, 0.0), (-1.2, thr_cb - 0.5, 0.0))],
                     kind=["car", "bike"], restated=True))
    ego, fl = respawning((2.9, -34.0, h + 0.01), (0.0, 0.3, 0.0), [149])
    out.append(_case("mates: eastbound (restated)", ego_east, restated=True, group="pair"))
    out.append(_case("mates: northbound, respawning after tick 149 (restated)", ego, flags=fl, restated=True, group="pair"))
    lane = [line((-20.0 + 7.5 * j, -0.1 * j, 0.01 * j), (-20.0 + 7.5 * j + (0.2 - 0.036 * j) * (N - 1), -0.1 * j, 0.01 * j)) for j in range(3)]
    rider = line((-30.0, thr_cb + 0.1, 0.0), (21.0, thr_cb - 0.3, 0.0))
    for j in range(3):
        out.append(_case(f"mates: three in a lane with a cyclist beside them, ego {j} (restated)", lane[j], [rider] if j == 0 else [], kind="bike",
                         restated=True, group="lane"))
    return out


# ---- the cases as recorder arrays ----
DECOY = 5.0e4                                        # where a record that must not be read puts the ego / a vehicle nobody meets


def recorder_arrays(cs):
    """rec [N][B][7], flags [N][B], obs [N][n_obs][6], x_first, x_spawn [B][4], veh_range, mate_range [B][2], shapes [n_obs][4] for
    a launch with one ego per case.  rec[k] is the pose at the start of tick k + 1, except where flags[k] ends the episode: there
    rec[k] is a far away state and tick k + 1 starts at x_spawn.  Vehicle 0 is a decoy; the cases' vehicles follow in case order
    (a group's scripted vehicles are its first ego's, and every ego of the group meets them)."""
    B = len(cs)
    n_obs = 1 + sum(len(c["vehicles"]) for c in cs)
    A = RN.ego_arrays([c["ego"] for c in cs], [c["flags"] for c in cs], DECOY, labels=[c["label"] for c in cs])
    obs, shapes = np.zeros((N, n_obs, 6)), np.zeros((n_obs, 4))
    obs[:, 0, :2], shapes[0] = DECOY, (*CAR, 2.86)
    veh_range, mate_range = np.zeros((B, 2), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
    o = 1
    for b, c in enumerate(cs):
        veh_range[b] = o, o + len(c["vehicles"])
        for v, kind in zip(c["vehicles"], c["kinds"]):
            obs[:, o, 0], obs[:, o, 1], obs[:, o, 2], obs[:, o, 3] = v[:, 0], v[:, 1], 1.0, v[:, 2]
            shapes[o] = (*SHAPES[kind], 2.86 if kind == "car" else 1.0)
            o += 1
        if c["group"] is not None:
            members = [j for j, d in enumerate(cs) if d["group"] == c["group"]]
            assert members == list(range(members[0], members[-1] + 1))
            mate_range[b] = members[0], members[-1] + 1
            veh_range[b] = veh_range[members[0]] if b > members[0] else veh_range[b]
        else:
            mate_range[b] = b, b                                  # none
    return {**A, "obs": obs, "veh_range": veh_range, "mate_range": mate_range, "shapes": shapes}


def restate(A, w, n=N, loops=False, stats=None):
    """The restatement on the first n ticks of recorder_arrays' output."""
    args = (A["rec"][:n], A["flags"][:n], A["obs"][:n], A["x_first"], A["x_spawn"], A["veh_range"], A["mate_range"], A["shapes"], CAR, w)
    return CN.eval_conflicts_loops(*args) if loops else CN.eval_conflicts(*args, stats=stats)


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conflicts.npz"), allow_pickle=False)
    return _FIX


def expected(g, w, n):
    """The fixture's per-episode records of window w and tick count n as arrays over [n][B]: made (an episode starts here and the
    record is there), hit (the reference did not return None), hit_tick (w = 0 only, else -2), hit_frame, hit_xy."""
    B = int(g["n_cases"])
    made, hit = np.zeros((n, B), dtype=bool), np.zeros((n, B), dtype=bool)
    tick, frame, xy = np.full((n, B), -1, dtype=np.int64), np.full((n, B), -1, dtype=np.int64), np.full((n, B, 2), np.nan)
    r = g["records"]
    for q in r[(r[:, 0] == w) & (r[:, 1] == n)]:
        b, k0 = int(q[2]), int(q[3])
        made[k0, b] = True
        hit[k0, b] = q[4] != 0
        tick[k0, b], frame[k0, b], xy[k0, b] = int(q[5]), int(q[6]), q[7:9]
    return made, hit, tick, frame, xy
