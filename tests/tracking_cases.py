"""The cases of tests/golden/tracking.npz: paths and pose series for the projection of every recorded pose onto
a path, chosen for the kernel's structure -- a search that takes four points to a step and then the rest one by one, the at most
three points a lane gathers around its own index, ties that the lower index and the lower segment win, a segmented reduction over
64-tick chunks with a carry.  No RNG.  Every exact tie is exact by construction: its coordinates are small dyadic numbers, so every
product and sum is exact; `ties` names the ticks that hold one.  Apart from those every discrete choice of every case has a margin
>= 1e-9 (asserted by condition(), which the CPU test and the fixture generator call): a last-bit difference between device and host
cannot flip an integer.  Used by the fixture generator (tests/golden/make_golden_tracking.py), which hands every pose and its path
to the reference's own calc_nearest_index, by the CPU test and by the GPU test, which lays the cases out as recorder arrays: one
ego per case, all paths in one table."""
import os

import numpy as np

import tracking_numpy as TN
from conflict_cases import N, blip, line, pw

TICK_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)   # every case is also evaluated cut to these lengths
GOAL, AGE = TN.GOAL, TN.AGE
MARGIN = 1e-9
C, X0, DX = 0.5, -2.0, 0.25                          # the straight path: along x at y = C from x = X0, a point every DX
R, DTH = 20.0, 1.0 / 64                              # the circular arc: radius, angle between two points; centre (0, R)
EPS = 2.0 ** -20


def _spiral(n=65, turn=7.5):
    th = turn * np.arange(n) / (n - 1)
    r = 10.0 + 0.5 * th
    x, y = r * np.cos(th), r * np.sin(th)
    yaw = th + np.arctan2(r, 0.5)                    # the tangent's angle, unwrapped: runs from 1.52 to 9.05, beyond 2 pi
    return np.stack([x, y, yaw], axis=1)


def _route(n=700, dl=0.1, r=8.0):
    """A planned route's shape: 250 points straight along +x, a quarter circle to the left, straight along +y; a point every dl."""
    pts, n_arc = [], int(round(r * np.pi / 2 / dl))
    for i in range(n):
        if i < 250:
            pts.append((dl * i, 0.0, 0.0))
        elif i < 250 + n_arc:
            a = (i - 249) * dl / r
            pts.append((dl * 249 + r * np.sin(a), r - r * np.cos(a), a))
        else:
            a = n_arc * dl / r
            j = i - (249 + n_arc)
            pts.append((dl * 249 + r * np.sin(a) + dl * j * np.cos(a), r - r * np.cos(a) + dl * j * np.sin(a), a))
    return np.array(pts)


def paths():
    th = DTH * np.arange(64)
    return [np.array([[1.5, -2.25, 0.5]]),                                               # 0: one point
            np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0]]),                                # 1: two
            np.array([[0.0, 0.0, 0.0], [4.0, 0.0, np.pi / 4], [4.0, 4.0, np.pi / 2]]),   # 2: three, a right-angled bend to the left
            np.stack([X0 + DX * np.arange(63), np.full(63, C), np.zeros(63)], axis=1),   # 3: 63, straight
            np.stack([R * np.sin(th), R - R * np.cos(th), th], axis=1),                  # 4: 64, a circular arc to the left
            _spiral(),                                                                   # 5: 65, the yaw beyond 2 pi
            _route(),                                                                    # 6: 700
            np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.5], [4.0, 2.0, 1.5]])]   # 7: identical points, twice


def _case(label, path, ego, flags=(), ties=()):
    """flags: {tick: flag}; ties: the ticks with a constructed exact tie, or "any": identical path points tie on every tick that
    is nearest to them, so a margin is 0 or >= MARGIN."""
    f = np.zeros(N, dtype=np.int32)
    for k, v in dict(flags).items():
        f[k] = v
    ego = np.asarray(ego, dtype=np.float64)
    assert ego.shape == (N, 3)
    return {"label": label, "path": int(path), "ego": ego, "flags": f, "ties": ties if ties == "any" else tuple(sorted(ties))}


def _along(path, u, off, dyaw, wrap=False):
    """Poses beside a path: at the (fractional) point index u[k], `off` to the left of it, heading the path's yaw + dyaw."""
    i = np.clip(np.floor(u).astype(int), 0, len(path) - 2)
    f = u - i
    p = path[i] + f[:, None] * (path[i + 1] - path[i])
    x, y, yaw = p[:, 0] - off * np.sin(p[:, 2]), p[:, 1] + off * np.cos(p[:, 2]), p[:, 2] + dyaw
    if wrap:
        yaw = (yaw + np.pi) % (2 * np.pi) - np.pi
    return np.stack([x, y, yaw], axis=1)


def cases():
    P = paths()
    k = np.arange(N, dtype=np.float64)
    out = []
    # 0: one point: seg 0, t 0, s 0, d = + the distance
    out.append(_case("a path of one point", 0, line((-3.0, -2.0, 0.3), (5.0, 1.0, 0.9))))
    # 1: two points: before the first and beyond the last (t clamped), left then right of the path; tick 100 exactly equidistant
    # from both points (the lower idx wins); ticks 50 and 150 on the segment's extension (zero cross product: +); ticks 120 and 121
    # not finite
    ego = line((-3.0, 1.25, 0.1), (7.0, -1.5, -0.2))
    ego = blip(blip(blip(ego, (2.0, 0.75, 0.0), [100]), (-1.5, 0.0, 0.0), [50]), (6.0, 0.0, 0.0), [150])
    ego = blip(blip(ego, (np.nan, 0.5, 0.0), [120]), (1.0, 0.5, np.inf), [121])
    out.append(_case("two points: clamped at both ends, an idx tie, the extension, two poses that are not finite", 1, ego, ties=[100]))
    # 2: the bend: a sweep round its inside; tick 40 exactly on the middle vertex, 41 on the bisector inside the bend, 42 outside the
    # corner (all three: a tie of the two segments, the lower wins); 43 and 44 inside the bend where the two segments disagree
    ego = np.stack([pw([(0, -1.0), (90, 3.3), (199, 3.4)]), pw([(0, 0.61), (90, 0.8), (199, 5.0)]), pw([(0, 0.0), (90, 0.7), (199, 1.6)])], axis=1)
    for tick, pose in ((40, (4.0, 0.0, 0.5)), (41, (3.0, 1.0, 0.5)), (42, (5.0, -1.0, 0.5)), (43, (3.0, 1.5, 0.5)), (44, (2.5, 1.0, 0.5))):
        ego = blip(ego, pose, [tick])
    out.append(_case("three points: on the vertex, on the bisector, outside the corner, inside the bend", 2, ego, ties=[40, 41, 42]))
    # 3: the straight path, every coordinate dyadic and no tie: d = y - C and s = x - X0 exactly.  Episodes end on 62, 63 and 64.
    # Heading errors just inside +-pi, across the wrap and exactly +-pi on ticks 10-15; tick 20 exactly on a vertex (the lower
    # segment), tick 21 exactly between two vertices (the lower idx)
    ego = np.stack([X0 + 1 / 32 + k / 16, C + (k - 100) / 64, (k - 100) / 256], axis=1)
    for tick, yaw in zip(range(10, 16), (np.pi - EPS, -np.pi + EPS, np.pi + EPS, -np.pi - EPS, np.pi, -np.pi)):
        ego[tick, 2] = yaw
    ego = blip(blip(ego, (0.0, 1.0, 0.25), [20]), (0.125, 0.25, 0.25), [21])
    out.append(_case("63 points, straight: exact; episodes ending on 62, 63, 64; the wrap", 3, ego, flags={62: GOAL, 63: AGE, 64: GOAL | AGE}, ties=[20, 21]))
    # 4: the same path: the same largest |d| = 2 on ticks 30 (+) and 130 (-) of one episode that covers three chunks (0 .. 150)
    d = np.where(k < 151, 1.0 + np.abs(((k + 3) % 16) - 8) / 16, 0.25)
    d[30], d[130] = 2.0, -2.0
    ego = np.stack([X0 + 3 / 32 + k / 16, C + d, np.full(N, -0.125)], axis=1)
    out.append(_case("63 points, straight: the largest |d| twice in an episode over three chunks", 3, ego, flags={150: AGE}))
    # 5: the arc, from before its first point to beyond its last, from inside to outside; every tick ends an episode
    phi, rho = -0.02 + 1.04 * k / (N - 1), 19.0 + 2.5 * k / (N - 1)
    ego = np.stack([rho * np.sin(phi), R - rho * np.cos(phi), phi + 0.05], axis=1)
    out.append(_case("64 points, an arc: every tick ends an episode", 4, ego, flags={int(t): (GOAL, AGE)[int(t) % 2] for t in k}))
    # 6: the spiral: beside it, the pose's yaw wrapped to [-pi, pi) while the path's runs beyond 2 pi; no episode ends
    out.append(_case("65 points, a spiral whose yaw runs beyond 2 pi", 5, _along(P[5], 63.3 * k / (N - 1) + 0.2, 0.3 * np.sin(k / 7) + 0.35, 0.1 * np.cos(k / 5), wrap=True)))
    # 7-8: two egos on the route; the first one's last record ends its episode
    out.append(_case("700 points: along the route, the last record ends the episode", 6, _along(P[6], 3.4712345 * k + 0.6, 0.2 * np.sin(k / 9) + 0.25, 0.2 * np.sin(k / 11)),
                     flags={130: GOAL, N - 1: AGE}))
    out.append(_case("700 points: the second ego on the same route, backwards", 6, _along(P[6], 697.3 - 3.3154321 * k, 0.7 - 0.2 * np.cos(k / 6), np.pi - 0.3), flags={5: AGE, 6: GOAL, 127: AGE}))
    # 9: identical consecutive points: an idx tie on every tick nearest to them; at the path's start the segment between them is
    # the only candidate (L2 = 0: t = 0)
    out.append(_case("two identical consecutive points", 7, line((-1.0, 0.5, 0.2), (5.0, 1.5, 0.9)), ties="any"))
    return out


def recorder_arrays(cs):
    """rec [N][B][7], flags [N][B], path_id [B] for a launch with one ego per case: rec[k] holds the pose of tick k in its first
    three columns and values no output may show in the others."""
    rec = np.full((N, len(cs), 7), 7.0e4)
    for b, c in enumerate(cs):
        rec[:, b, :3] = c["ego"]
    return {"rec": rec, "flags": np.stack([c["flags"] for c in cs], axis=1), "path_id": np.array([c["path"] for c in cs], dtype=np.int32),
            "paths": paths()}


def restate(A, n=N, egos=None):
    """The restatement on the first n ticks of recorder_arrays' output (egos: a subset, in that order)."""
    e = slice(None) if egos is None else list(egos)
    return TN.eval_tracking(A["rec"][:n, e], A["flags"][:n, e], A["path_id"][e], A["paths"])


def condition(cs, ref):
    """Apart from the constructed exact ties every discrete choice has a margin >= MARGIN; the constructed ones are exact.  `ref`:
    the restatement of all N ticks.  Returns the smallest margin apart from the ties."""
    least = np.inf
    for b, c in enumerate(cs):
        m = np.fmin(ref["margin_idx"][:, b], ref["margin_seg"][:, b])
        has = ref["idx"][:, b] >= 0
        assert not np.isnan(m[has]).any(), c["label"]
        if c["ties"] == "any":
            assert (m[has] == 0.0).any(), c["label"]
            free = has & (m != 0.0)
        else:
            tied = np.zeros(N, dtype=bool)
            tied[list(c["ties"])] = True
            assert (m[tied] == 0.0).all(), (c["label"], m[tied])
            free = has & ~tied
        assert (m[free] >= MARGIN).all(), (c["label"], np.flatnonzero(free & ~(m >= MARGIN)), m[free].min())
        least = min(least, float(m[free].min()))
    return least


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking.npz"), allow_pickle=False)
    return _FIX
