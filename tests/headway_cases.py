"""The cases of tests/golden/headway.npz: paths, ego and vehicle series for the projection of every recorded
vehicle onto the ego's path, chosen for the kernel's structure -- a search that serves the ego's two circle centres in one pass and
the vehicles' in groups of 4, 2 and 1 places, four points to a step and then the rest one by one, the at most three points a lane
gathers around each index, a segmented reduction over 64-tick chunks with a carry.  No RNG.  Every exact tie is exact by
construction (small dyadic coordinates on a straight path, headings of exactly 0: cos = 1, sin = 0); apart from those every discrete
choice of every case has a margin >= 1e-9 and every |rate| is exactly 0 or >= 0.05 (asserted by condition(), which the CPU test and
the fixture generator call): a last-bit difference between device and host cannot flip an integer or turn a finite TTC into inf.
Used by the fixture generator (tests/golden/make_golden_headway.py), which hands every pose to the reference's own
car_trajectory_to_collision_point_trajectories and every circle centre to its calc_nearest_index, by the CPU test and by the GPU
test, which lays the cases out as recorder arrays: one ego per case, all paths in one table, every case's vehicles in one table."""
import os

import numpy as np

import headway_numpy as HN
import recorder_numpy as RN
import tracking_cases as KC
from conflict_cases import BIKE, CAR, N, respawning
from recorder_numpy import AGE, GOAL

TICK_COUNTS = (0, 1, 63, 64, 65, 129, 200)           # every case is also evaluated cut to these lengths
MARGIN = 1e-9
RATE_MIN = 0.05
LAUNCH_MARGIN = 0.25                                 # the call's `margin`: dyadic, so thr + margin is one rounded sum on both sides
DT = 0.125
EPS = 2.0 ** -20
SHAPES = {"car": CAR, "bike": BIKE}
THR_CC = (CAR[2] + CAR[2]) + LAUNCH_MARGIN           # a car's threshold against a car ego, with the margin: in [2, 4)
DECOY = 5.0e4
CENTRE_STRIDE = 5                                    # the fixture stores the reference's circle centres of every fifth tick


def straight(n, dx):
    """n points along +x from the origin at y = 0, a point every dx (dyadic), yaw exactly 0."""
    return np.stack([dx * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)


def paths():
    """1, 2, 3, 63, 64, 65 and 700 points (tracking_cases' own), then straight paths of 4, 5, 8 and 9 points."""
    return KC.paths()[:7] + [straight(4, 8.0), straight(5, 8.0), straight(8, 4.0), straight(9, 4.0)]


P1, P2, P3, P63, P64, P65, P700, S4, S5, S8, S9 = range(11)


def cruise(x0, y0, yaw, v, speed=None, n=N):
    """[n][4] x, y, yaw, v: from (x0, y0) along heading yaw at v metres per second (DT a tick); `speed`: the v that is recorded."""
    k = np.arange(n, dtype=np.float64)
    return np.stack([x0 + (v * DT * np.cos(yaw)) * k, y0 + (v * DT * np.sin(yaw)) * k, np.full(n, yaw), np.full(n, v if speed is None else speed)], axis=1)


def beside(path, u, off, dyaw, v):
    """[n][4]: KC._along's poses beside a path with the recorded speed v."""
    return np.concatenate([KC._along(path, u, off, dyaw), np.full((len(u), 1), float(v))], axis=1)


def _case(label, path, ego, v_ego, vehicles=(), kinds="car", flags=None, group=None, ties=()):
    """ego [N][3] poses at the start of every tick, v_ego its constant speed; vehicles: [N][4] series; kinds: one name or one per
    vehicle; group: the label egos that are each other's mates share (consecutive cases; a group's scripted vehicles are its first
    ego's); ties: the (tick, place) pairs whose |lat| is exactly thr + margin."""
    kinds = [kinds] * len(vehicles) if isinstance(kinds, str) else list(kinds)
    assert len(kinds) == len(vehicles)
    ego = np.asarray(ego, dtype=np.float64)
    assert ego.shape == (N, 3)
    return {"label": label, "path": int(path), "ego": ego, "v_ego": float(v_ego), "vehicles": [np.asarray(v, dtype=np.float64) for v in vehicles],
            "kinds": kinds, "flags": np.zeros(N, dtype=np.int32) if flags is None else np.asarray(flags, dtype=np.int32), "group": group,
            "ties": tuple(ties)}


def cases():
    P = paths()
    k = np.arange(N, dtype=np.float64)
    out = []
    # 0: one car ahead at a quarter of the ego's speed: ahead, alongside (gap == 0.0 from tick 61 on) and behind (from tick 154 on)
    out.append(_case("9 points: a slower car ahead, then alongside, then behind", S9, cruise(2.0, 0.0, 0.0, 1.0)[:, :3], 1.0,
                     [cruise(12.03, 0.25, 0.0, 0.25)]))
    # 1: episodes that end on a chunk's last tick and on its first, twice; a standing car ahead, an oncoming cyclist in the other lane
    # (off the path) and an oncoming car on it; two shapes in one list
    ego, fl = respawning((2.0, 0.0, 0.0), (0.125, 0.0, 0.0), [63, 64, 127, 128])
    out.append(_case("8 points: episodes ending on ticks 63, 64, 127, 128; a standing car, an oncoming cyclist beside the path, an oncoming car on it",
                     S8, ego, 1.0, [cruise(20.07, 0.3, 0.0, 0.0), cruise(26.0, 3.5, np.pi, 1.5), cruise(27.9, 0.2, np.pi, 0.5)],
                     kinds=["car", "bike", "car"], flags=fl))
    # 2: equal speeds on a heading of exactly 0: rate == 0.0, TTC inf, thw = gap; two cars at the same gap: the lower place leads
    out.append(_case("5 points: two cars at the same gap and at the ego's speed", S5, cruise(2.0, 0.0, 0.0, 1.0)[:, :3], 1.0,
                     [cruise(12.0, 0.25, 0.0, 1.0), cruise(12.0, -0.25, 0.0, 1.0)]))
    # 3: a standing ego (u_e == 0: thw inf) and an oncoming cyclist that closes, passes and leaves
    out.append(_case("4 points: a standing ego, an oncoming cyclist", S4, cruise(3.0, 0.0, 0.0, 0.0)[:, :3], 0.0, [cruise(13.04, 0.5, np.pi, 0.5)], kinds="bike"))
    # 4: three standing cars side by side ahead, headings exactly 0: |lat| = thr + margin + 2^-20 (off), exactly thr + margin (on)
    # and 2^-20 less (on); the two on the path are at the same gap: place 1 leads
    ys = [KC.C + THR_CC + EPS, KC.C + THR_CC, KC.C + THR_CC - EPS]
    assert all(y - KC.C == t for y, t in zip(ys, (THR_CC + EPS, THR_CC, THR_CC - EPS)))          # exact sums
    out.append(_case("63 points: |lat| exactly at the threshold and 2^-20 either side", P63, cruise(-1.0, KC.C, 0.0, 0.25)[:, :3], 0.25,
                     [cruise(9.0, y, 0.0, 0.0) for y in ys], ties=[(t, 1) for t in range(N)]))
    # 5: eight vehicles along the route, cars and cyclists in turn, the last ones beyond the path's end; a pose of NaN in the middle
    # of the run (place 3, ticks 90 .. 95), a speed of NaN (place 5, tick 100), a pose of inf (place 0, tick 129)
    veh = [beside(P[P700], 0.8 * k + 45.37 + 80.0 * j, 0.7 + 0.1 * j + (1.5 if j >= 6 else 0.0), 0.02 * j, 1.2 - 0.05 * j) for j in range(8)]
    veh[3][90:96, 0] = np.nan
    veh[5][100, 3] = np.nan
    veh[0][129, 1] = np.inf
    flags = np.zeros(N, dtype=np.int32)
    flags[130] = GOAL
    out.append(_case("700 points: eight vehicles, two shapes, poses that are not finite, vehicles beyond the path's end", P700,
                     KC._along(P[P700], 3.0 * k + 5.45, 0.2 * np.sin(k / 9) + 0.8, 0.1 * np.sin(k / 11)), 3.0, veh,
                     kinds=["car", "bike"] * 4, flags=flags))
    # 6-7: two mates on one path with one shape: each is the other's only place
    out.append(_case("mates: the follower", S9, cruise(2.0, 0.25, 0.0, 1.0)[:, :3], 1.0, group="pair"))
    out.append(_case("mates: the leader, at half the speed", S9, cruise(14.0, -0.25, 0.0, 0.5)[:, :3], 0.5, group="pair"))
    # 8-9: two mates and a scripted cyclist on the arc: vehicles and mates in one list
    out.append(_case("64 points, an arc: a mate ahead and a cyclist between, ego 0", P64, KC._along(P[P64], 0.2 * k + 2.0, 0.5, 0.02), 2.0,
                     [beside(P[P64], 0.1 * k + 30.3, 0.4, 0.05, 1.0)], kinds="bike", group="duo"))
    out.append(_case("64 points, an arc: ego 1", P64, KC._along(P[P64], 0.2 * k + 14.1, 0.7, -0.03), 1.5, group="duo"))
    # 10: no vehicles: -1 / NaN throughout
    out.append(_case("three points: no vehicles", P3, KC.cases()[2]["ego"], 1.0))
    # 11-13: the shortest paths
    out.append(_case("a path of one point: everything alongside", P1, np.stack([-3.0 + 0.04 * k, -2.0 + 0.015 * k, np.full(N, 0.3)], axis=1), 1.0,
                     [cruise(0.5, -1.75, 0.7, 0.4)], kinds="bike"))
    out.append(_case("two points: clamped at both ends", P2, np.stack([-3.0 + 0.03 * k, np.full(N, 0.2), np.full(N, 0.05)], axis=1), 0.8,
                     [cruise(3.5, -0.3, 0.1, 0.0)]))
    out.append(_case("three points: round the bend behind a cyclist", P3, np.stack([-1.0 + 0.022 * k, 0.3 + 0.002 * k, np.full(N, 0.1)], axis=1), 0.6,
                     [np.stack([np.full(N, 3.8), 0.5 + 0.017 * k, np.full(N, 1.5), np.full(N, 0.3)], axis=1)], kinds="bike"))
    # 14: the spiral
    out.append(_case("65 points, a spiral: a slower car ahead", P65, KC._along(P[P65], 0.1 * k + 1.2, 0.6, 0.0), 1.5,
                     [beside(P[P65], 0.05 * k + 8.1, 0.9, 0.05, 0.7)]))
    return out


def recorder_arrays(cs):
    """rec [N][B][7], flags [N][B], obs [N][n_obs][6] (x, y, v, yaw, then values no output may show), x_first, x_spawn [B][4],
    veh_range, mate_range [B][2], shapes [n_obs][4], path_id [B], paths, for a launch with one ego per case: the egos as
    recorder_numpy.ego_arrays lays them out, with each case's own speed.  Vehicle 0 is a decoy nobody meets."""
    B = len(cs)
    n_obs = 1 + sum(len(c["vehicles"]) for c in cs)
    A = RN.ego_arrays([c["ego"] for c in cs], [c["flags"] for c in cs], DECOY, labels=[c["label"] for c in cs])
    for b, c in enumerate(cs):
        A["rec"][:, b, 3], A["x_first"][b, 2], A["x_spawn"][b, 2] = c["v_ego"], c["v_ego"], c["v_ego"]
    obs, shapes = np.full((N, n_obs, 6), 7.0e4), np.zeros((n_obs, 4))
    obs[:, 0, :4], shapes[0] = (DECOY, DECOY, 1.0, 0.0), (*CAR, 2.86)
    veh_range, mate_range = np.zeros((B, 2), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
    o = 1
    for b, c in enumerate(cs):
        veh_range[b] = o, o + len(c["vehicles"])
        for v, kind in zip(c["vehicles"], c["kinds"]):
            obs[:, o, 0], obs[:, o, 1], obs[:, o, 2], obs[:, o, 3] = v[:, 0], v[:, 1], v[:, 3], v[:, 2]
            shapes[o] = (*SHAPES[kind], 2.86 if kind == "car" else 1.0)
            o += 1
        if c["group"] is not None:
            members = [j for j, d in enumerate(cs) if d["group"] == c["group"]]
            assert members == list(range(members[0], members[-1] + 1))
            mate_range[b] = members[0], members[-1] + 1
            veh_range[b] = veh_range[members[0]] if b > members[0] else veh_range[b]
        else:
            mate_range[b] = b, b
    return {**A, "obs": obs, "veh_range": veh_range, "mate_range": mate_range, "shapes": shapes,
            "path_id": np.array([c["path"] for c in cs], dtype=np.int32), "paths": paths()}


def restate(A, n=N, egos=None, margin=LAUNCH_MARGIN):
    """The restatement on the first n ticks of recorder_arrays' output (egos: a subset, in that order, whose mate ranges must then
    be empty or inside it -- the tests cut whole groups only)."""
    if egos is None:
        return HN.eval_headway(A["rec"][:n], A["flags"][:n], A["obs"][:n], A["x_first"], A["x_spawn"], A["veh_range"], A["mate_range"],
                               A["shapes"], CAR, A["path_id"], A["paths"], margin)
    e = list(egos)
    assert all(A["mate_range"][b, 0] == A["mate_range"][b, 1] for b in e)
    return HN.eval_headway(A["rec"][:n, e], A["flags"][:n, e], A["obs"][:n], A["x_first"][e], A["x_spawn"][e], A["veh_range"][e],
                           np.zeros((len(e), 2), dtype=np.int32), A["shapes"], CAR, A["path_id"][e], A["paths"], margin)


def _series_margin(v):
    """How far the first minimum of a series (NaN passed over) is from every other value that is not equal to it; inf without two."""
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size < 2:
        return np.inf
    rest = v[v != v.min()]
    return float(rest.min() - v.min()) if rest.size else np.inf


def condition(cs, ref):
    """Every discrete choice has a margin >= MARGIN, apart from the exact ties: the constructed ones at the threshold (`ties`), equal
    candidates of a leader or a time to collision (identical operands: case 2's two cars, case 4's two on the path; 0.0 and inf), and
    equal values of a series over an episode's ticks (the first tick stays).  Every |rate| is 0.0 or >= RATE_MIN.  `ref`: the
    restatement of all N ticks.  Returns the smallest margin apart from the ties."""
    least = np.inf
    for b, c in enumerate(cs):
        what = c["label"]
        for key in ("m_idx", "m_seg", "m_gap"):
            m = ref[key][:, b]
            m = m[~np.isnan(m)]
            assert (m >= MARGIN).all(), (what, key, float(m.min()))
            least = min(least, float(m.min(initial=np.inf)))
        on = ref["m_on"][:, b].copy()
        for tick, place in c["ties"]:
            assert on[tick, place] == 0.0, (what, tick, place, on[tick, place])
            on[tick, place] = np.nan
        on = on[~np.isnan(on)]
        assert (on >= MARGIN).all(), (what, "m_on", float(on.min()))
        least = min(least, float(on.min(initial=np.inf)))
        for key in ("m_lead", "m_ttc"):
            m = ref[key][:, b]
            m = m[~np.isnan(m) & (m != 0.0)]
            assert (m >= MARGIN).all(), (what, key, float(m.min()))
            least = min(least, float(m.min(initial=np.inf)))
        rate = ref["rate"][:, b]
        rate = np.abs(rate[~np.isnan(rate)])
        assert ((rate == 0.0) | (rate >= RATE_MIN)).all(), (what, "rate", float(rate[rate > 0].min()))
        for k0, k1 in HN.TN.episodes_of(c["flags"]):
            for key in ("lead_gap", "thw", "ttc"):
                m = _series_margin(ref[key][k0:k1 + 1, b])
                assert m >= MARGIN, (what, key, k0, m)
                least = min(least, m)
    return least


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headway.npz"), allow_pickle=False)
    return _FIX
