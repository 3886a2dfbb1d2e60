#!/usr/bin/env python3
"""Writes tests/golden/planner_shapes.npz: the route planner on GENERAL shapes and at its table limits, solved by
oracle/planner_oracle.py (the numpy restatement that reproduces the reference's planner bit for bit on its stored routes,
tests/test_planner.py; it has no pruning circle, no tables, no passes).  These are the ORACLE's outputs.

1. Collision probes: one route query each, ONE primitive ("straight"), one obstacle under test, the goal box around the primitive's
   end pose.  The car's foremost collision point (the "tip", 7.16 m ahead of the start) ends PROBE_EPS = 0.05 m inside row i of
   the obstacle at the middle of that edge (every row satisfied: blocked, status 1 after one expansion) or 0.05 m outside it
   (row i is the ONLY row that rejects the point: free, status 0 with one primitive) -- every row of every obstacle decides two
   outcomes.  Families: "poly" (3 ... 12 rows, rotated, rows scaled, centres off the origin; each probe also with the world moved
   so that the start is the origin: create_2d_transform_mtx's 2 x 2 branch), "unb" (one half-plane, a wedge, a strip, no row at
   all), "red" (a 16-gon with every row four times -- repeated and tiled -- and a 12-gon with 20 rows that bind nowhere; the
   de-duplicated polygons beside them), "pos" (the probed 12-gon as obstacle 1, 33 and 64 of 64 with 512 rows in all, the others
   next to the car's path: in reach of the pruning circle, touching nothing).
2. Whole searches with other primitive sets (1, 3, 16 primitives; 31 points), circle sets (1, 3, 4 circles; 10 ... 256
   (primitive, collision point) pairs) on asymmetric random fields of such polygons, and for each an obstacle whose removal
   changes the route.

usage: make_golden_planner_shapes.py      (~3 min on 4 cores; seeds are fixed, a dropped seed is printed with its reason)"""
import math
import os
import struct
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import planner_oracle as PO     # noqa: E402

L, WIDTH, EXTRA = 2.86, 2.0, 0.64
RADIUS = WIDTH / (2 ** .5)
_len = L + EXTRA
CENTRES = np.array([[L / 2 + (_len / 2 - WIDTH / 2), 0.0], [L / 2 - (_len / 2 - WIDTH / 2), 0.0]])
PROBE_EPS = 0.05
POLY_ROWS = (3, 5, 6, 7, 9, 10, 11, 12)
BUDGET = 1500            # oracle expansions per search (~1 ms each)


def primitives(steer, L=L, v=8.3, n_steps=60, dt=0.01):
    """PO.make_motion_primitives' recipe (Bicycle.step from the origin, the state recorded before every step) for any list of
    steering angles; v may be one speed per primitive."""
    out = []
    for k, delta in enumerate(steer):
        vk = v[k] if np.ndim(v) else v
        x = y = th = 0.0
        pts = []
        for _ in range(n_steps + 1):
            pts.append((x, y, th))
            xd = vk * np.cos(th); yd = vk * np.sin(th); thd = (vk / L) * np.tan(delta)
            x += xd * dt; y += yd * dt; th += thd * dt
        pts = np.array(pts, dtype=np.float64)
        out.append((f"s{delta:+.2f}", pts, float(np.linalg.norm(pts[:-1, :2] - pts[1:, :2], axis=1).sum())))
    return out


STRAIGHT = primitives([0.0])
assert np.array_equal(STRAIGHT[0][1], PO.make_motion_primitives()[0][1])
_cc = PO.collision_points(STRAIGHT[0][1], CENTRES, RADIUS)
assert len(_cc) == 10 and np.all(_cc[:, 1] == 0.0)
TIP = float(_cc[:, 0].max())                       # the foremost collision point, on the car's axis
END = STRAIGHT[0][1][-1]


# ------------------------------------------------------------------------------------------------ obstacles
def polygon(rng, n, centre, radius, jitter=0.2, scale=True, shuffle=True):
    """(rows [n, 3], edge midpoints [n, 2]): a convex polygon inscribed in a circle, its corners at jittered angles (so no two
    edges alike, no normal at a multiple of 45 degrees), rows a x + b y + c <= 0 with the outward normal scaled by a random
    positive factor each, listed in random order."""
    ang = rng.uniform(0, 2 * np.pi) + (np.arange(n) + rng.uniform(-jitter, jitter, n)) * 2 * np.pi / n
    v = np.asarray(centre) + radius * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    rows, mids = [], []
    for k in range(n):
        p, q = v[k], v[(k + 1) % n]
        nrm = np.array([q[1] - p[1], -(q[0] - p[0])])
        nrm /= np.hypot(*nrm)
        s = rng.uniform(0.2, 5.0) if scale else 1.0
        rows.append([s * nrm[0], s * nrm[1], -s * float(nrm @ p)])
        mids.append((p + q) / 2)
    rows, mids = np.array(rows), np.array(mids)
    if shuffle:
        perm = rng.permutation(n)
        rows, mids = rows[perm], mids[perm]
    return rows, mids


def signed(rows, pts):
    """[rows, points] signed distances (normalised rows)."""
    pts = np.atleast_2d(pts)
    return (rows[:, :2] @ pts.T + rows[:, 2:3]) / np.hypot(rows[:, 0], rows[:, 1])[:, None]


def moved(rows, alpha, t):
    """The rows of the set turned by alpha about the origin, then shifted by t."""
    R = np.array([[np.cos(alpha), -np.sin(alpha)], [np.sin(alpha), np.cos(alpha)]])
    nrm = rows[:, :2] @ R.T
    return np.column_stack([nrm, rows[:, 2] - nrm @ np.asarray(t)])


def probe_start(rows, i, anchor, inside):
    """The start pose from which the straight primitive's tip ends PROBE_EPS inside (outside) row i at `anchor` (a point on its
    boundary), heading against the row's normal -- every other collision point is further out along that normal."""
    nrm = rows[i, :2] / np.hypot(*rows[i, :2])
    tip = np.asarray(anchor) + (-PROBE_EPS if inside else PROBE_EPS) * nrm
    th = PO.normalize_angle(float(np.arctan2(-nrm[1], -nrm[0])))
    s = tip - TIP * np.array([np.cos(th), np.sin(th)])
    return (float(s[0]), float(s[1]), th)


def probe_query(start, obstacles):
    x, y, th = start
    ex, ey = x + END[0] * np.cos(th), y + END[0] * np.sin(th)
    return dict(start=start, goal=(float(ex), float(ey), th), goal_box=(float(ex - 0.5), float(ey - 0.5), float(ex + 0.5), float(ey + 0.5)),
                tol=0.5, obstacles=obstacles)


def shifted_to_origin(q):
    """The same query in a world whose origin is the start's position."""
    sx, sy, th = q["start"]
    obst = [np.column_stack([o[:, :2], o[:, 2] + o[:, 0] * sx + o[:, 1] * sy]) if len(o) else o for o in q["obstacles"]]
    gx, gy, gth = q["goal"]
    b = q["goal_box"]
    return dict(start=(0.0, 0.0, th), goal=(gx - sx, gy - sy, gth), goal_box=(b[0] - sx, b[1] - sy, b[2] - sx, b[3] - sy), tol=q["tol"], obstacles=obst)


def solve_probe(q):
    orc = PO.PlannerOracle(q["start"], q["goal"], q["goal_box"], q["tol"], q["obstacles"], STRAIGHT, CENTRES, RADIUS)
    try:
        cost, path, _ = orc.run()
        assert orc.prim_sequence(path) == [0]
        return 0, orc.n_expanded
    except Exception as e:
        assert str(e) == "No solution found."
        return 1, orc.n_expanded


def check_decisive(q, rows, i, inside):
    """The construction's promise, on the geometry alone: the tip is PROBE_EPS from row i and at least 0.04 m from every other
    row's boundary, on its inner side; every other collision point is at least 0.04 m outside the obstacle."""
    x, y, th = q["start"]
    c = np.array([np.cos(th), np.sin(th)])
    pts = np.array([x, y]) + _cc[:, :1] * c
    tip = pts[np.argmax(_cc[:, 0])]
    d = signed(rows, tip)[:, 0]
    same = np.all(np.abs(rows / np.hypot(rows[:, 0], rows[:, 1])[:, None] - rows[i] / np.hypot(*rows[i, :2])) < 1e-12, axis=1)
    assert abs(d[i] - (-PROBE_EPS if inside else PROBE_EPS)) < 1e-9 and np.all(d[~same] <= -0.04), (i, inside, d)
    rest = np.delete(pts, np.argmax(_cc[:, 0]), axis=0)
    assert np.all(signed(rows, rest).max(axis=0) >= 0.04)


class Probes:
    """One family: its obstacles once, and per probe the start, the obstacle list (indices into the family's), the probed obstacle,
    the row, inside / outside, a variant number and the oracle's outcome."""

    def __init__(self, name):
        self.name, self.obst, self.rows = name, [], []

    def obstacle(self, rows):
        self.obst.append(np.asarray(rows, dtype=np.float64).reshape(-1, 3))
        return len(self.obst) - 1

    def add(self, q, ids, target, row, inside, variant, expect=None):
        status, ne = solve_probe(q)
        if expect is not None:
            assert status == expect, (self.name, target, row, inside, variant, status)
        assert (status, ne) in ((1, 1), (0, 2))
        self.rows.append(dict(start=q["start"], goal=q["goal"], goal_box=q["goal_box"], tol=q["tol"], ids=list(ids), target=target, row=row,
                              inside=int(inside), variant=variant, status=status, n_expanded=ne))

    def arrays(self):
        p = f"p_{self.name}_"
        off = np.cumsum([0] + [len(o) for o in self.obst]).astype(np.int32)
        ids_off = np.cumsum([0] + [len(r["ids"]) for r in self.rows]).astype(np.int32)
        return {p + "hp": np.concatenate(self.obst, axis=0), p + "hp_off": off,
                p + "start": np.array([r["start"] for r in self.rows]), p + "goal": np.array([r["goal"] for r in self.rows]),
                p + "goal_box": np.array([r["goal_box"] for r in self.rows]), p + "tol": np.array([r["tol"] for r in self.rows]),
                p + "ids": np.concatenate([r["ids"] for r in self.rows]).astype(np.int32), p + "ids_off": ids_off,
                p + "meta": np.array([[r["target"], r["row"], r["inside"], r["variant"]] for r in self.rows], dtype=np.int32),
                p + "status": np.array([r["status"] for r in self.rows], dtype=np.int32),
                p + "n_expanded": np.array([r["n_expanded"] for r in self.rows], dtype=np.int32)}


def family_poly():
    """variant 0: as built (the start wherever the probe puts it), 1: the world moved so that the start is the origin."""
    rng = np.random.default_rng(4201)
    F = Probes("poly")
    for n in POLY_ROWS:
        rows, mids = polygon(rng, n, rng.uniform(-25, 25, 2) + np.array([40.0, -15.0]), float(rng.uniform(2.5, 6.0)))
        o = F.obstacle(rows)
        for i in range(n):
            for inside in (True, False):
                q = probe_query(probe_start(rows, i, mids[i], inside), [rows])
                check_decisive(q, rows, i, inside)
                assert q["start"][0] != 0.0 and q["start"][1] != 0.0
                F.add(q, [o], o, i, inside, 0, expect=1 if inside else 0)
                q0 = shifted_to_origin(q)
                F.obst.append(q0["obstacles"][0])              # (the moved polygon is an obstacle of its own)
                F.add(q0, [len(F.obst) - 1], o, i, inside, 1, expect=1 if inside else 0)
    return F


def family_unbounded():
    """One half-plane; a wedge of two (70 degrees between the normals); a strip 2 m wide; an obstacle without a row, for which the
    reference's np.all over nothing says "inside" whatever the point: pinned as the oracle has it.  Both variants as in "poly"."""
    rng = np.random.default_rng(4202)
    F = Probes("unb")
    a0 = rng.uniform(0, 2 * np.pi)
    n0 = np.array([np.cos(a0), np.sin(a0)])
    p0 = np.array([12.0, -7.0])
    half = np.array([[2.5 * n0[0], 2.5 * n0[1], -2.5 * float(n0 @ p0)]])
    a1 = a0 + np.deg2rad(70.0)
    n1 = np.array([np.cos(a1), np.sin(a1)])
    apex = np.array([-9.0, 14.0])
    wedge = np.array([[0.4 * n0[0], 0.4 * n0[1], -0.4 * float(n0 @ apex)], [3.0 * n1[0], 3.0 * n1[1], -3.0 * float(n1 @ apex)]])
    strip = np.array([[1.7 * n1[0], 1.7 * n1[1], -1.7 * float(n1 @ p0)], [-0.6 * n1[0], -0.6 * n1[1], 0.6 * (float(n1 @ p0) - 2.0)]])
    # anchors: on row i's boundary, 3 m from the wedge's apex on the side the other row accepts
    t0, t1 = np.array([-n0[1], n0[0]]), np.array([-n1[1], n1[0]])
    w0 = apex + 3.0 * t0 * (1 if n1 @ t0 < 0 else -1)
    w1 = apex + 3.0 * t1 * (1 if n0 @ t1 < 0 else -1)
    for rows, anchors in ((half, [p0]), (wedge, [w0, w1]), (strip, [p0, p0 - 2.0 * n1])):
        o = F.obstacle(rows)
        for i, anchor in enumerate(anchors):
            for inside in (True, False):
                q = probe_query(probe_start(rows, i, anchor, inside), [rows])
                check_decisive(q, rows, i, inside)
                F.add(q, [o], o, i, inside, 0, expect=1 if inside else 0)
                q0 = shifted_to_origin(q)
                F.obst.append(q0["obstacles"][0])
                F.add(q0, [len(F.obst) - 1], o, i, inside, 1, expect=1 if inside else 0)
    o = F.obstacle(np.zeros((0, 3)))
    for variant, start in ((0, (3.0, -4.0, 0.7)), (1, (0.0, 0.0, -2.1))):
        F.add(probe_query(start, [np.zeros((0, 3))]), [o], o, -1, 1, variant)           # whatever the oracle says: status 1
    assert all(r["status"] == 1 for r in F.rows[-2:])
    return F


def regular_polygon(n, centre, circumradius):
    ang = np.arange(n) * 2 * np.pi / n
    v = np.asarray(centre) + circumradius * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    rows, mids = [], []
    for k in range(n):
        p, q = v[k], v[(k + 1) % n]
        nrm = np.array([q[1] - p[1], -(q[0] - p[0])])
        nrm /= np.hypot(*nrm)
        rows.append([nrm[0], nrm[1], -float(nrm @ p)])
        mids.append((p + q) / 2)
    return np.array(rows), np.array(mids)


def family_redundant():
    """Rows that add nothing to the set: target = the de-duplicated polygon's obstacle id, variant 0: that polygon itself, 1: every
    row four times in a row (np.repeat), 2: the list four times over (np.tile), 3: 20 more rows that bind nowhere.  Every edge of
    the polygon is probed (16 and 12 directions around it)."""
    rng = np.random.default_rng(4203)
    F = Probes("red")
    gon16, mid16 = regular_polygon(16, (10.0, 0.0), 3.06)
    gon12, mid12 = polygon(rng, 12, (-14.0, 9.0), 3.5)
    far = []
    for _ in range(20):                                          # tangent to circles 0.5 ... 2 m outside the 12-gon's
        a, s, d = rng.uniform(0, 2 * np.pi), rng.uniform(0.2, 5.0), 3.5 + rng.uniform(0.5, 2.0)
        far.append([s * np.cos(a), s * np.sin(a), -s * (np.cos(a) * -14.0 + np.sin(a) * 9.0 + d)])
    plus20 = np.concatenate([gon12, np.array(far)], axis=0)[rng.permutation(32)]
    for base, mids, forms in ((gon16, mid16, ((1, np.repeat(gon16, 4, axis=0)), (2, np.tile(gon16, (4, 1))))), (gon12, mid12, ((3, plus20),))):
        o = F.obstacle(base)
        ids = [(0, o, base)] + [(v, F.obstacle(rows), rows) for v, rows in forms]
        for i in range(len(base)):
            for inside in (True, False):
                start = probe_start(base, i, mids[i], inside)
                check_decisive(probe_query(start, [base]), base, i, inside)
                for v, oid, rows in ids:
                    F.add(probe_query(start, [rows]), [oid], o, i, inside, v, expect=1 if inside else 0)
    return F


def family_position():
    """The probed obstacle (a 12-gon, moved for every probe so that the start stays where it is) as number 1, 33 and 64 of the
    route's 64 obstacles (variant 0, 32, 63: its index), 12 + 59 x 8 + 4 x 7 = 512 rows.  The 63 others stand beside the car's
    path -- 1.5 and 3 m to either side, within 6.8 m of the start, corners 0.4 m out: inside the pruning radius, so that all 64 are
    walked, and clear of every collision point."""
    rng = np.random.default_rng(4204)
    F = Probes("pos")
    S = (6.0, -3.5, 0.9)
    c, s = np.cos(S[2]), np.sin(S[2])
    spots = [(a, l) for l in (1.5, -1.5, 3.0, -3.0) for a in np.linspace(-3.0, 6.0, 16)][:63]
    others = []
    for k, (a, l) in enumerate(spots):
        centre = (S[0] + a * c - l * s, S[1] + a * s + l * c)
        others.append(F.obstacle(polygon(rng, 7 if k % 16 == 5 else 8, centre, 0.4)[0]))
    assert sum(len(F.obst[k]) for k in others) == 500
    base, mids = polygon(rng, 12, (0.0, 0.0), 4.0)
    for i in range(12):
        for inside in (True, False):
            sx, sy, sth = probe_start(base, i, mids[i], inside)
            alpha = S[2] - sth                                  # the polygon's frame -> the world in which the start is S
            R = np.array([[np.cos(alpha), -np.sin(alpha)], [np.sin(alpha), np.cos(alpha)]])
            rows = moved(base, alpha, np.array(S[:2]) - R @ np.array([sx, sy]))
            check_decisive(probe_query(S, [rows]), rows, i, inside)
            o = F.obstacle(rows)
            for at in (0, 32, 63):
                ids = others[:at] + [o] + others[at:]
                assert len(ids) == 64 and sum(len(F.obst[k]) for k in ids) == 512
                F.add(probe_query(S, [F.obst[k] for k in ids]), ids, o, i, inside, at, expect=1 if inside else 0)
    return F


# ------------------------------------------------------------------------------------------------ searches
STEER16 = [s * m for m in (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4) for s in (1, -1)]
_c1 = np.array([[L / 2, 0.0]])
_c3 = np.array([[0.4, 0.0], [L / 2, 0.0], [2.46, 0.0]])
_c4 = np.array([[0.3, 0.0], [1.1, 0.0], [1.9, 0.0], [2.7, 0.0]])
# name: steering angles, (n_steps, dt), (radius, circle centres), seeds tried in this order until `keep` are kept
CONFIGS = {
    "p1":     dict(steer=[0.0], steps=(60, 0.01), circles=(RADIUS, CENTRES), seeds=range(0, 2), keep=2),              # 10 pairs
    "p3":     dict(steer=[0.0, 0.3, -0.2], steps=(60, 0.01), circles=(RADIUS, CENTRES), seeds=list(range(10, 30)) + list(range(300, 330)), keep=3),  # 30
    "p3n31":  dict(steer=[0.0, 0.2, -0.35], steps=(30, 0.02), circles=(1.6, _c1), seeds=list(range(30, 50)) + list(range(330, 360)), keep=2),       # 3 x 5 = 15
    "p9n31":  dict(steer=list(PO.MP_STEER), steps=(30, 0.02), circles=(1.3, _c3), seeds=range(50, 70), keep=3),        # 9 x 15 = 135
    "p16c1":  dict(steer=STEER16, steps=(60, 0.01), circles=(1.0, _c1), seeds=range(70, 130), keep=3),                  # 16 x 6 = 96
    "p16c2":  dict(steer=STEER16, steps=(60, 0.01), circles=(RADIUS, CENTRES), seeds=range(130, 190), keep=3),          # 16 x 10 = 160
    "p16c4":  dict(steer=STEER16, steps=(60, 0.01), circles=(1.8, _c4), seeds=range(190, 250), keep=3),                # 16 x 16 = 256
}


def config_primitives(cfg):
    return primitives(cfg["steer"], n_steps=cfg["steps"][0], dt=cfg["steps"][1])


def field(seed, n_prim):
    """An asymmetric field of general polygons (the margin is the largest car circle's radius, added to the circumradius) inside
    a fence; start off the origin for odd seeds.  One primitive: the goal four primitives straight ahead, and for odd seeds a
    polygon across the third."""
    rng = np.random.default_rng(7000 + seed)
    start = (0.0, 0.0, float(rng.uniform(-np.pi, np.pi))) if seed % 2 == 0 else (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5)), float(rng.uniform(-np.pi, np.pi)))
    obs = []
    for _ in range(int(rng.integers(6, 15))):
        c = rng.uniform(-28, 28, 2)
        r = float(rng.uniform(1.0, 4.5)) + RADIUS
        n = int(rng.choice(POLY_ROWS))
        if np.hypot(c[0] - start[0], c[1] - start[1]) < r + 7.5:      # keep the start clear
            continue
        obs.append(polygon(rng, n, c, r)[0])
    for cx, cy, w, h in ((0, 36, 80, 4), (0, -36, 80, 4), (36, 0, 4, 80), (-36, 0, 4, 80)):
        obs.append(PO.box_halfplanes((w, h), (cx, cy), RADIUS))
    if n_prim == 1:
        d = np.array([np.cos(start[2]), np.sin(start[2])])
        obs = [o for o in obs[:-4] if np.all(signed(o, np.array(start[:2]) + np.linspace(0, 30, 121)[:, None] * d).max(axis=0) > 0.5)]
        if seed % 2:
            obs.insert(len(obs) // 2, polygon(rng, 7, np.array(start[:2]) + 16.0 * d, 1.5)[0])
        g = np.array(start[:2]) + 4 * END[0] * d
        return dict(start=start, goal=(float(g[0]), float(g[1]), start[2]), goal_box=(float(g[0] - 1), float(g[1] - 1), float(g[0] + 1), float(g[1] + 1)),
                    tol=0.3, obstacles=obs)
    # (sixteen primitives: the open list grows sixteen-fold per level -- nearer goals keep the oracle's search within its budget)
    ang, dist = float(rng.uniform(-np.pi, np.pi)), float(rng.uniform(10, 24) if n_prim < 16 else rng.uniform(14, 20))
    gx, gy = start[0] + dist * np.cos(ang), start[1] + dist * np.sin(ang)
    gth = float(rng.uniform(-np.pi, np.pi))
    half = float(rng.uniform(2.0, 4.0))
    tol = float(rng.choice([np.pi / 4, np.pi / 6, np.pi / 8]))
    if n_prim >= 16:      # ... and in the open space such a goal leaves, a polygon on the way to it, a little to one side
        half, tol = max(half, 3.0), float(np.pi / 4)
        side = float(rng.uniform(0.5, 1.5)) * (1 if rng.random() < 0.5 else -1)
        mid = np.array([start[0] + 0.5 * dist * np.cos(ang) - side * np.sin(ang), start[1] + 0.5 * dist * np.sin(ang) + side * np.cos(ang)])
        obs.insert(len(obs) // 2, polygon(rng, int(rng.choice(POLY_ROWS)), mid, float(rng.uniform(2.0, 3.0)))[0])
    return dict(start=start, goal=(gx, gy, gth), goal_box=(gx - half, gy - half, gx + half, gy + half), tol=tol, obstacles=obs)


def run_oracle(q, mps, circles, obstacles=None, budget=BUDGET):
    """-> dict(status, cost, path, prims, n_expanded) or the reason the search is not kept."""
    orc = PO.PlannerOracle(q["start"], q["goal"], q["goal_box"], q["tol"], q["obstacles"] if obstacles is None else obstacles, mps,
                           circles[1], circles[0])
    try:
        cost, path, _ = orc.run(max_expansions=budget)
        return dict(status=0, cost=cost, path=np.array(path), prims=np.array(orc.prim_sequence(path), dtype=np.int32), n_expanded=orc.n_expanded)
    except RuntimeError:
        return f"more than {budget} expansions"
    except Exception as e:
        assert str(e) == "No solution found."
        return dict(status=1, cost=np.nan, path=np.zeros((0, 3)), prims=np.zeros(0, dtype=np.int32), n_expanded=orc.n_expanded)


class ExplicitOrder(PO.PlannerOracle):
    """The same planner with the pose transform written out operation by operation (x' = px cos + py (-sin), then + x) instead of
    numpy's matmul: equal in exact arithmetic, different in the last bit now and then.  A search whose expansion count depends on
    that bit (exact ties in g + h decided by the poses, nodes reached twice that are one dict entry or two) cannot be pinned to
    max(1, n // 50) expansions on any other implementation, the HIP kernel included; such seeds are not kept."""

    def neighbors(self, node):
        return self._neighbors(node, math.cos(node[2]), math.sin(node[2]))

    def _neighbors(self, node, cs, sn):
        x0, y0, th0 = node
        rot = (x0 == 0 and y0 == 0)
        for k, (name, pts, total) in enumerate(self.mps):
            c = self.cc[k]
            wx, wy = c[:, 0] * cs + c[:, 1] * (-sn), c[:, 0] * sn + c[:, 1] * cs
            if not rot:
                wx, wy = wx + x0, wy + y0
            if any(bool(np.any(np.all(((o[:, 0:1] * wx + o[:, 1:2] * wy) + o[:, 2:3]) <= 0, axis=0))) for o in self.hp):
                continue
            ex, ey = pts[-1, 0] * cs + pts[-1, 1] * (-sn), pts[-1, 0] * sn + pts[-1, 1] * cs
            if not rot:
                ex, ey = ex + x0, ey + y0
            nb = (float(ex), float(ey), PO.normalize_angle(float(pts[-1, 2] + th0)))
            self.edge_mp[(node, nb)] = k
            yield self.wc_dist * total + self.wc_steer * self.steering_change(node, nb), nb     # (wh_obstacle = wc_center = 0 here)


class OneUlp(ExplicitOrder):
    """... and with the cosine and the sine of about half the headings one ulp off, up or down, picked by a hash of the heading
    and `mode`: another libm."""
    mode = 0

    def neighbors(self, node):
        h = (struct.unpack("Q", struct.pack("d", node[2]))[0] * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        cs, sn = math.cos(node[2]), math.sin(node[2])
        b = (h >> (40 + 2 * self.mode)) & 3
        if b & 1:
            cs = math.nextafter(cs, 2.0 if (h >> 50) & 1 else -2.0)
        if b & 2:
            sn = math.nextafter(sn, 2.0 if (h >> 51) & 1 else -2.0)
        return self._neighbors(node, cs, sn)


def last_bit_sensitive(q, mps, circles, out):
    """None, or why the search is not kept: what ExplicitOrder and three OneUlp modes make of it against the oracle's `out`
    (expansions within half the bar of the tests, max(1, n // 100); the same route)."""
    ne = out["n_expanded"]
    for mode in (None, 0, 1, 2):
        orc = (ExplicitOrder if mode is None else OneUlp)(q["start"], q["goal"], q["goal_box"], q["tol"], q["obstacles"], mps, circles[1], circles[0])
        orc.mode = mode
        what = "the pose transform in explicit order" + ("" if mode is None else f" and cos / sin one ulp off (mode {mode})")
        try:
            cost, path, _ = orc.run(max_expansions=4 * BUDGET)
            prims = orc.prim_sequence(path)
        except RuntimeError:
            return f"with {what} the search outgrows its budget"
        except Exception as e:
            assert str(e) == "No solution found."
            prims = []
        if prims != list(out["prims"]):
            return f"another route with {what} (a tie in g + h)"
        if abs(orc.n_expanded - ne) > max(1, ne // 100):
            return f"{orc.n_expanded} expansions instead of {ne} with {what} (ties in g + h; half the bar is {max(1, ne // 100)})"
    return None


# seeds whose route the HIP planner finds with the SAME cost (to 1e-9) but another primitive sequence or expansion count: an exact tie in g + h between
# two open nodes, decided by the last ulp of the pose transform (tests/test_planner.py) -- replaced, the assertion stays
# (p3 seed 10, with the set (0, +0.3, -0.3) the configuration had first: 240 expansions on the MI355X against the oracle's 230, the
# same route and cost to the last bit -- ExplicitOrder gives 240 as well.  Mirror-image primitives make such ties the rule: the
# three-primitive sets are asymmetric since, and last_bit_sensitive() drops what still depends on the last bit)
TIED_SEEDS = {"p3": (10,)}


def solve_search(args):
    name, seed = args
    cfg = CONFIGS[name]
    mps = config_primitives(cfg)
    q = field(seed, len(mps))
    if seed in TIED_SEEDS.get(name, ()):
        return name, seed, "ties in g + h seen on the GPU (equal costs, another route or expansion count)"
    out = run_oracle(q, mps, cfg["circles"])
    if isinstance(out, str):
        return name, seed, out
    if out["status"] == 1 and len(mps) > 1:
        return name, seed, "no route"
    if out["status"] == 0 and len(out["prims"]) < 2:
        return name, seed, "a route of one primitive"
    why = last_bit_sensitive(q, mps, cfg["circles"], out)
    if why:
        return name, seed, why
    # an obstacle without which the route is another one (the fence is not tried; the ones nearest to the route first)
    key = -1
    n_try = len(q["obstacles"]) - (4 if len(mps) > 1 else 0)
    near = out["path"][:, :2] if out["status"] == 0 else np.array([q["start"][:2]])
    for k in sorted(range(n_try), key=lambda k: float(signed(q["obstacles"][k], near).max(axis=0).min()))[:3]:
        alt = run_oracle(q, mps, cfg["circles"], obstacles=q["obstacles"][:k] + q["obstacles"][k + 1:])
        if not isinstance(alt, str) and list(alt["prims"]) != list(out["prims"]):
            key = k
            break
    if key < 0 and not (len(mps) == 1 and out["status"] == 0):
        return name, seed, "none of the three obstacles nearest to the route decides it"
    out.update(seed=seed, key_obstacle=key, start=np.array(q["start"]), goal=np.array(q["goal"]), goal_box=np.array(q["goal_box"]), tol=q["tol"],
               hp=np.concatenate(q["obstacles"], axis=0), hp_off=np.cumsum([0] + [len(o) for o in q["obstacles"]]).astype(np.int32))
    return name, seed, out


if __name__ == "__main__":
    arrays = {"radius": RADIUS, "circle_centers": CENTRES, "probe_eps": PROBE_EPS, "tip": TIP}
    for fam in (family_poly(), family_unbounded(), family_redundant(), family_position()):
        a = fam.arrays()
        arrays.update(a)
        st = a[f"p_{fam.name}_status"]
        print(f"probes {fam.name}: {len(st)} routes, {int((st == 1).sum())} blocked, {int((st == 0).sum())} free, {len(fam.obst)} obstacles")
    arrays["families"] = np.array(["poly", "unb", "red", "pos"])
    kept = {name: [] for name in CONFIGS}
    with ProcessPoolExecutor(max_workers=4) as ex:
        for name, cfg in CONFIGS.items():
            seeds = list(cfg["seeds"])
            while seeds and len(kept[name]) < cfg["keep"]:
                now, seeds = seeds[:4], seeds[4:]
                for _, seed, out in ex.map(solve_search, [(name, s) for s in now]):
                    if isinstance(out, str):
                        print(f"search {name} seed {seed}: dropped -- {out}", flush=True)
                    elif len(kept[name]) >= cfg["keep"]:
                        print(f"search {name} seed {seed}: not needed ({cfg['keep']} kept)", flush=True)
                    else:
                        print(f"search {name} seed {seed}: status {out['status']}, {out['n_expanded']} expansions, {len(out['prims'])} primitives, "
                              f"obstacle {out['key_obstacle']} of {len(out['hp_off']) - 1} decides", flush=True)
                        kept[name].append(out)
    for name, cfg in CONFIGS.items():
        assert len(kept[name]) == cfg["keep"], (name, len(kept[name]))
        mps = config_primitives(cfg)
        mpset = f"{len(mps)}x{cfg['steps'][0] + 1}"              # (the three sixteen-primitive configurations share one set)
        arrays[f"c_{name}_mpset"] = np.array(mpset)
        pts = np.stack([p for _, p, _ in mps])
        assert f"mp_{mpset}_points" not in arrays or np.array_equal(arrays[f"mp_{mpset}_points"], pts)
        arrays[f"mp_{mpset}_points"] = pts
        arrays[f"mp_{mpset}_length"] = np.array([t for _, _, t in mps])
        arrays[f"c_{name}_radius"] = float(cfg["circles"][0])
        arrays[f"c_{name}_centres"] = np.asarray(cfg["circles"][1], dtype=np.float64)
        arrays[f"c_{name}_n"] = len(kept[name])
        for j, out in enumerate(kept[name]):
            for k, v in out.items():
                arrays[f"c_{name}_r{j}_{k}"] = v
    arrays["configs"] = np.array(list(CONFIGS))
    # a two-primitive set whose second primitive is faster and so longer: 16 and 17 collision points with one circle of 0.34 m
    two = primitives([0.0, 0.1], v=[8.3, 8.9])
    arrays["cc17_mp_points"] = np.stack([p for _, p, _ in two])
    arrays["cc17_mp_length"] = np.array([t for _, _, t in two])
    arrays["cc17_radius"] = 0.34
    arrays["cc17_centres"] = _c1
    assert [len(PO.collision_points(p, _c1, 0.34)) for _, p, _ in two] == [16, 17]
    path = os.path.join(HERE, "planner_shapes.npz")
    np.savez_compressed(path, **arrays)
    print(os.path.getsize(path), "bytes")
