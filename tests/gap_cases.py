"""The cases of tests/golden/gaps.npz: synthetic pose series for the time gap per recorded tick, in the style
of tests/conflict_cases.py (whose helpers and recorder layout they use) and chosen for the kernel's structure -- 64 ticks per chunk,
offsets that reach 63 ticks into either neighbouring chunk, vehicle ticks that count or do not count by the episode they lie in, a
tie between -o and +o, a wavefront minimum per episode.  No RNG: every pose series is piecewise linear over 200 ticks.  Used by the
fixture generator (tests/golden/make_golden_gaps.py), which hands every episode to the reference's own check_collision_moving_cars /
check_collision_moving_bicycle at every frame_window 0 .. 63 and stores the least one that hits, by the CPU test and by the GPU test,
which lays the cases out as recorder arrays: one ego per case, every case's vehicles in one table."""
import os

import numpy as np

import conflict_cases as TC
import gaps_numpy as GN
from conflict_cases import BIKE, CAR, FAR, N, blip, line, pw, respawning, still

TICK_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)  # every case is also evaluated cut to these lengths
WINDOWS = (0, 1, 20, 62, 63)
RULES = ("episode", "record")
H = np.pi / 2

# the crossing: the ego northbound through the origin at 1 m per tick, there on tick 100; a vehicle eastbound through the origin at
# `speed` m per tick, there on tick 100 + g.  g < 0: the vehicle goes first.
CROSS_G = (0, 6, 7, 10, 21, 40, 67, 68, 69)          # least offsets 0, 1, 2, 5, 16, 35, 62, 63 and 64 (none within the window)
CROSS_LEAST = (0, 1, 2, 5, 16, 35, 62, 63, -1)


def northbound(x=0.13, at=100, yaw=H - 0.01):
    return line((x, -float(at), yaw), (x, float(N - 1 - at), yaw))


def eastbound(g, speed=1.0, y=0.07, yaw=0.02, at=100):
    k = at + g
    return line((-speed * k, y, yaw), (speed * (N - 1 - k), y, yaw))


HOME = (5.3, -2.7, 0.4)                              # where an ego waits that is to be somewhere on chosen ticks only
AWAY, BESIDE = (-50.0, -50.0, 0.4), (-48.1, -49.2, 2.1)   # the ego's place on those ticks and a vehicle pose that touches it there


def _case(label, ego, vehicles=(), kind="car", flags=None, restated=False, group=None):
    return TC._case(label, ego, vehicles, kind=kind, flags=flags, restated=restated, group=group)


def cases():
    out = []
    ego = northbound()
    # 0-16: the crossing at every gap, the ego first (g > 0) and the vehicle first (g < 0)
    for g in CROSS_G:
        for s in ((1,) if g == 0 else (1, -1)):
            out.append(_case(f"crossing, the vehicle at the origin {s * g:+d} ticks after the ego", ego, [eastbound(s * g)]))
    # 17: nothing ever touches
    out.append(_case("a vehicle that is never near", ego, [still(FAR)]))
    # 18-19: the crossing with the vehicle at half the speed
    out.append(_case("crossing at half the speed, vehicle first", ego, [eastbound(-31, speed=0.5)]))
    out.append(_case("crossing at half the speed, ego first", ego, [eastbound(54, speed=0.5)]))
    # 20: a tie: the vehicle is beside the ego's place of tick 100 on ticks 91 and 109 and on no tick between
    out.append(_case("tie between -9 and +9 on tick 100", blip(still(HOME), AWAY, [100]), [blip(still(FAR), BESIDE, [91, 109])]))
    # 21-23: the ego's lane: a leader 12 m ahead, a follower 30 m behind, both
    lead, follow = northbound(at=88), northbound(at=130)
    out.append(_case("a leader 12 m ahead in the ego's lane", ego, [lead]))
    out.append(_case("a follower 30 m behind in the ego's lane", ego, [follow]))
    out.append(_case("a leader and a follower", ego, [lead, follow]))
    # 24-25: an oncoming pass 2.3 m to the side: within the car's threshold (2.83), outside the cyclist's (1.73)
    oncoming = line((0.13 + 2.3, 100.0, -H), (0.13 + 2.3, 100.0 - (N - 1), -H))
    out.append(_case("an oncoming car 2.3 m to the side", ego, [oncoming]))
    out.append(_case("an oncoming cyclist 2.3 m to the side", ego, [oncoming], kind="bike"))
    # 26-29: 0, 2 and 8 vehicles (1 is everywhere above), cars and cyclists
    out.append(_case("no vehicles", ego))
    out.append(_case("two cars", ego, [eastbound(-10), eastbound(21)]))
    out.append(_case("eight cyclists", ego, [eastbound(g, y=0.07 + 0.2 * j) for j, g in enumerate((-60, 33, -19, 4, 58, -2, 70, -41))], kind="bike"))
    out.append(_case("eight cars", ego, [eastbound(g, y=-0.3 + 0.1 * j) for j, g in enumerate((52, -67, 30, -30, 68, -69, 12, -8))]))
    # 30-34: chunk edges: the ego beside a place on chosen ticks only, the vehicle there on chosen ticks only
    there = lambda ticks: blip(still(FAR), BESIDE, ticks)
    out.append(_case("ego tick 64 against vehicle ticks 1 and 127", blip(still(HOME), AWAY, [64]), [there([1]), there([127])]))
    out.append(_case("ego ticks 63 and 64 against vehicle ticks 0, 127 and 128", blip(still(HOME), AWAY, [63, 64]), [there([0]), there([127]), there([128])]))
    out.append(_case("ego tick 0 against vehicle tick 63", blip(still(HOME), AWAY, [0]), [there([63])]))
    out.append(_case("ego tick 199 against vehicle tick 136", blip(still(HOME), AWAY, [N - 1]), [there([136])], kind="bike"))
    out.append(_case("ego tick 64 against vehicle ticks 0 and 128: one tick too far", blip(still(HOME), AWAY, [64]), [there([0, 128])]))
    # 35-37: an episode ending on 62, 63, 64: the ego is at the origin on tick 50 and again 51 ticks after the end, the car on tick 70
    # -- behind the first episode's end, so only the record rule counts it there
    for k in (62, 63, 64):
        e, fl = respawning((0.13, -50.0, H - 0.01), (0.0, 1.0, 0.0), [k])
        out.append(_case(f"episode ending on tick {k}, the car at the origin on tick 70", e, [eastbound(-30)], flags=fl))
    # 38: an episode of length 1 (tick 101) beside a slow car
    e, fl = respawning((0.13, -3.0, H - 0.01), (0.0, 0.05, 0.0), [100, 101])
    out.append(_case("episode of length 1", e, [eastbound(4, speed=0.3)], flags=fl))
    # 39: episodes of 5, 2, 1 and 3 ticks, then a long one
    e, fl = respawning((0.13, -4.0, H - 0.01), (0.0, 1.0, 0.0), [4, 6, 7, 10])
    out.append(_case("episodes shorter than the window", e, [eastbound(-92, speed=3.0)], flags=fl))
    # 40: the vehicle is beside the spawn point 3 ticks before the ego respawns there, and never else
    e, fl = respawning(AWAY, (0.011, 0.002, 0.0), [79])
    e[:80] = np.asarray(HOME) + np.arange(80)[:, None] * np.array([0.011, 0.002, 0.0])
    out.append(_case("a vehicle beside the spawn point 3 ticks before the respawn", e, [there([77])], flags=fl))
    # restatement-made (no reference function takes a mixed list or a list of egos)
    out.append(_case("a car and a cyclist in one list (restated)", ego, [eastbound(-10), eastbound(21, y=0.4)], kind=["car", "bike"], restated=True))
    out.append(_case("mates: northbound (restated)", ego, restated=True, group="pair"))
    out.append(_case("mates: eastbound, at the origin 10 ticks later (restated)", eastbound(10), restated=True, group="pair"))
    e, fl = respawning((0.13, -80.0, H - 0.01), (0.0, 1.0, 0.0), [99])
    lane = [northbound(at=88), e, northbound(at=130)]
    for j in range(3):
        out.append(_case(f"mates: three in a lane, the middle one respawning after tick 99, ego {j} (restated)", lane[j], [eastbound(45)] if j == 0 else [],
                         flags=fl if j == 1 else None, restated=True, group="lane"))
    return out


def recorder_arrays(cs):
    """conflict_cases' layout: one ego per case, vehicle 0 a decoy, the cases' vehicles in case order."""
    return TC.recorder_arrays(cs)


def restate(A, window, within, n=N, loops=False, stats=None):
    """The restatement on the first n ticks of recorder_arrays' output; within: 0 / 1 or a rule's name."""
    within = GN.WITHIN.get(within, within)
    args = (A["rec"][:n], A["flags"][:n], A["obs"][:n], A["x_first"], A["x_spawn"], A["veh_range"], A["mate_range"], A["shapes"], CAR, window, within)
    return GN.eval_gaps_loops(*args) if loops else GN.eval_gaps(*args, stats=stats)


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaps.npz"), allow_pickle=False)
    return _FIX


def expected(g, n):
    """The fixture's per-episode records of tick count n as arrays over [n][B]: made (an episode starts here) and least (the least
    frame_window 0 .. 63 at which the reference does not return None, -1: none; for the flagged cases the restatement's ep_gap)."""
    B = int(g["n_cases"])
    made, least = np.zeros((n, B), dtype=bool), np.full((n, B), -1, dtype=np.int64)
    r = g["records"]
    for q in r[r[:, 0] == n]:
        made[q[2], q[1]], least[q[2], q[1]] = True, q[3]
    return made, least
