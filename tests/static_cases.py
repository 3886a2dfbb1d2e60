"""The cases of tests/golden/static.npz: synthetic pose series for the static-obstacle evaluation, chosen
for the kernel's structure -- 64 ticks per chunk, a loop over the rows of the ego's own obstacle set, a touch test on half-planes
beside a clearance from true distances, an episode's first touching tick from ballots.  No RNG: every pose series is piecewise
linear over 200 ticks (an arc is linear in its angle), with the knots putting each event on the tick the case is about.  Used by
the fixture generator (tests/golden/make_golden_static.py), which hands every tick to the reference's own check_collision and
distance_to_point, by the CPU test, which rebuilds the cases and compares, and by the GPU test, which lays them out as recorder
arrays: one ego per case, every set's rows in one table.

The three real sets (the reference's intersection, roundabout and T-intersection) exist only in the fixture, as the rows the
reference's objects made; the synthetic sets are written here as primitives ("box", xy_width, xy_center, hidden) / ("circle",
radius, xy_center, hidden), from which the generator builds the reference's objects and planner.static_obstacle_rows the rows."""
import os

import numpy as np

import conflict_cases as TC
import recorder_numpy as RN
import static_numpy as SN
from conflict_cases import CAR, GOAL, AGE, N, blip, line, pw, respawning, still   # noqa: F401

TICK_COUNTS = TC.TICK_COUNTS                          # 1, 2, 63, 64, 65, 127, 128, 129 and the whole 200
HIDDEN = (0, 1)                                       # include_hidden
R = CAR[2]                                            # the ego radius, and the margin of every row in the fixture
FAR = (61.7, 58.3, 0.3)                               # where an ego waits that is to touch on chosen ticks only
EVENT_TICKS = (0, 62, 63, 64, 65, N - 1)

# set index -> name; 0..2 are the reference's builders (called by the generator), the others the primitives below
SET_NAMES = ("intersection(1, 1)", "roundabout(1, 1, 'small')", "t_intersection(1, 1)", "empty", "one box 4 x 2", "all hidden",
             "two boxes at equal distance", "one circle", "one box 2 x 2")
SYNTHETIC = {
    3: [],
    4: [("box", (4.0, 2.0), (0.0, 0.0), False)],
    5: [("box", (4.0, 2.0), (0.0, 0.0), True), ("circle", 1.5, (6.0, 0.0), True)],
    6: [("box", (6.0, 2.0), (1.0, 3.0), False), ("box", (6.0, 2.0), (1.0, -3.0), False)],
    7: [("circle", 2.0, (0.0, 0.0), False)],
    8: [("box", (2.0, 2.0), (0.0, 0.0), False)],
}


def intersection_configs():
    """(number_of_lanes, start_pos, turn_indicator, start_lane, goal_lane) of every intersection whose rows the fixture pins by
    digest: the one-lane builder (number_of_lanes 0, as planner.intersection_query names it) and the two-lane one."""
    return ([(0, sp, tn, 1, 1) for sp in (1, 2, 3, 4) for tn in (1, 2, 3)] +
            [(2, sp, tn, sl, gl) for sp in (1, 2, 3, 4) for tn in (1, 2, 3) for sl in (1, 2) for gl in (1, 2)])


def arc(centre, radius, phi0, phi1, clockwise, n=N):
    """Poses on a circle around `centre`, the angle linear from phi0 to phi1, heading along the motion."""
    phi = pw([(0, phi0), (n - 1, phi1)], n)
    yaw = phi - np.pi / 2 if clockwise else phi + np.pi / 2
    return np.stack([centre[0] + radius * np.cos(phi), centre[1] + radius * np.sin(phi), yaw], axis=1)


def exact_edge_poses():
    """Against the right edge of set 8's box with yaw = 0 (cos = 1, sin = 0 exactly): the pose whose rear circle centre is exactly
    on the inflated edge, so that the right half-plane's value (1 * x + 0 * y) + c is exactly 0.0, and the pose 2 ulp further."""
    edge = 1.0 + R                                                    # -c of the right half-plane of to_convex(R)
    px = edge - CAR[1]
    for _ in range(8):
        if px + CAR[1] == edge:
            break
        px = np.nextafter(px, np.inf if px + CAR[1] < edge else -np.inf)
    assert px + CAR[1] == edge
    further = np.nextafter(np.nextafter(px, np.inf), np.inf)
    return (float(px), 0.0, 0.0), (float(further), 0.0, 0.0)


def _case(label, ego, set_index, flags=None, exact=False):
    return {"label": label, "ego": np.asarray(ego, dtype=np.float64), "set": int(set_index), "exact": bool(exact),
            "flags": np.zeros(N, dtype=np.int32) if flags is None else np.asarray(flags, dtype=np.int32)}


def cases():
    out = []
    h = np.pi / 2
    # 0-3: up the start lane of the intersection beside the pavement (obstacle 13, x from 5): touched from x = 4.0 on; at x = 3.0 the
    # median (obstacle 0) and the pavement are equally far, exactly (cos(pi/2) * cc is below half an ulp of 3.0): who = 0; the drive
    # ends before the corner island's octagon (obstacle 11) is reached
    for x in (3.0, 3.5, 4.0, 4.5):
        out.append(_case(f"start lane at x = {x}", line((x, -40.0, h), (x, -24.0, h)), 0, exact=(x == 3.0)))
    # 4-5: a drift towards the pavement that touches with the rear circle only, and one with the front circle only
    out.append(_case("drift, rear circle only", line((3.2, -30.0, h + 0.3), (4.1, -20.0, h + 0.3)), 0))
    out.append(_case("drift, front circle only", line((2.7, -30.0, h - 0.3), (3.3, -20.0, h - 0.3)), 0))
    # 6: a right turn around the south-east corner island (obstacle 11: centre (12, -12), r = 7) at radius 8.8: outside the axis planes
    # (8.41) at both ends, inside the diagonal plane (9.0) in between -- touching while 0.4 m clear
    out.append(_case("right turn past a corner island", arc((12.0, -12.0), 8.8, np.pi, h, clockwise=True), 0))
    # 7: down the oncoming lane of the south arm: inside a hidden box (obstacle 22) and nothing else
    out.append(_case("inside a hidden box only", line((-2.9, -16.0, -h), (-2.9, -30.0, -h)), 0))
    # 8-9: the other two real sets: into the roundabout past its centre island; a left turn through the T-intersection
    out.append(_case("into the roundabout", line((3.1, -30.0, 1.5), (5.2, -2.0, 1.2)), 1))
    out.append(_case("left turn through the T-intersection", arc((-12.0, -12.0), 14.8, 0.0, h, clockwise=False), 2))
    # 10: no obstacles
    out.append(_case("empty set", line((-3.0, -0.5, 0.1), (3.0, 0.5, 0.1)), 3))
    # 11-16: one box, touched on ticks 0, 62, 63, 64, 65 and 199 only
    for j, k in enumerate(EVENT_TICKS):
        out.append(_case(f"one box, touched on tick {k} only", blip(still(FAR), (1.2 + 0.3 * j, 0.4 - 0.1 * j, 0.2 * j), [k]), 4))
    # 17: the box-corner quirk: the rear centre 0.9 r beyond the corner in x and y touches the square-cornered inflated box with
    # clear = +0.386; two ticks with it 1.1 r beyond (no touch)
    corner = (2.0 + 0.9 * R - CAR[1], 1.0 + 0.9 * R, 0.0)
    out.append(_case("box corner: touching while clear", blip(still(corner), (2.0 + 1.1 * R - CAR[1], 1.0 + 1.1 * R, 0.0), [63, 64]), 4))
    # 18: a centre inside the obstacle: clear = -radius
    out.append(_case("a centre inside the box", line((-2.18 + 0.5, 0.2, 0.0), (-2.18 + 1.5, -0.2, 0.0)), 4))
    # 19-24: one box, the ego approaching from its spawn state (touching from the 27th tick of an episode on), episodes ending on
    # 62, 63, 64, on 0 and on 199; and leaving it (touching on an episode's first two ticks) with episodes of length 1
    for ends in ([62], [63], [64], [0], [N - 1]):
        ego, fl = respawning((3.0, 0.3, 0.0), (-0.01, 0.0, 0.0), ends)
        out.append(_case(f"one box, approaching, episodes ending on {ends}", ego, 4, flags=fl))
    ego, fl = respawning((3.4 - CAR[1], 0.3, 0.0), (0.01, 0.0, 0.0), [100, 101, 102])
    out.append(_case("one box, leaving, episodes of length 1", ego, 4, flags=fl))
    # 25: a set that is all hidden: nothing without the hidden ones, a touch with them
    out.append(_case("all hidden", line((-4.0, 0.3, 0.0), (4.0, -0.3, 0.0)), 5))
    # 26: two boxes at equal distance, exactly (yaw = 0: both centres have y = 0.0): who = 0
    out.append(_case("two boxes at equal distance", line((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)), 6, exact=True))
    # 27: the octagon quirk: the rear centre at 45 degrees, 3.9 from the centre of a circle of r = 2 (diagonal plane at 4.0, true
    # contact at 3.41), and at 22.5 degrees, 3.6 from it (axis plane at 3.41 / cos 22.5 = 3.70); then both just outside
    at = lambda deg, d: (d * np.cos(np.radians(deg)) - CAR[1], d * np.sin(np.radians(deg)), 0.0)
    ego = still(at(45.0, 3.9))
    ego[50:100], ego[100:150], ego[150:] = at(22.5, 3.6), at(45.0, 4.1), at(22.5, 3.8)
    out.append(_case("octagon at 45 and 22.5 degrees", ego, 7))
    # 28: exactly on the inflated right edge (even ticks: value 0.0, touches) and 2 ulp further (odd ticks: +4.4e-16, does not)
    on, off = exact_edge_poses()
    ego = still(on)
    ego[1::2] = off
    out.append(_case("exactly on the edge / 2 ulp further", ego, 8, exact=True))
    return out


# ---- the cases as recorder arrays ----
DECOY = TC.DECOY


def recorder_arrays(cs):
    """rec [N][B][7], flags [N][B], x_first, x_spawn [B][4], set_of [B] for a launch with one ego per case.  rec[k] is the pose at the
    start of tick k + 1, except where flags[k] ends the episode: there rec[k] is a far away state and tick k + 1 starts at x_spawn."""
    A = RN.ego_arrays([c["ego"] for c in cs], [c["flags"] for c in cs], DECOY, hold_last=True, labels=[c["label"] for c in cs])
    return {**A, "set_of": np.array([c["set"] for c in cs], dtype=np.int32)}


def restate(A, g, hidden, n=N, loops=False, stats=None, egos=None):
    """The restatement on the first n ticks of recorder_arrays' output against the fixture's tables."""
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    args = (A["rec"][:n, idx], A["flags"][:n, idx], A["x_first"][idx], A["x_spawn"][idx], A["set_of"][idx], g["set_off"], g["rows"], CAR, bool(hidden))
    return SN.eval_static_loops(*args) if loops else SN.eval_static(*args, stats=stats)


def expected_off_tick(hit, flags):
    """off_tick [n][B] from a `hit` [n][B] by plain loops: per episode its first tick with hit >= 0, at the episode's first slot."""
    n, B = hit.shape
    out = np.full((n, B), -1, dtype=np.int32)
    for b in range(B):
        for k0, k1 in RN.episodes_of(flags[:n, b]):
            for k in range(k0, k1 + 1):
                if hit[k, b] >= 0:
                    out[k0, b] = k
                    break
    return out


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "static.npz"), allow_pickle=False)
    return _FIX
