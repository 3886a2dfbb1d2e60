"""The route planner on general shapes and at its table limits, CPU half: tests/golden/planner_shapes.npz is the oracle's
(every probe and the cheap searches solved again, bit for bit), and the fixture covers what it claims -- on the oracle and the
geometry alone, no device: every row of every probed obstacle decides a blocked and a free outcome, the padded walks, all four
collision passes, the table limits and both transform branches occur.  tests/test_gpu_planner_shapes.py runs the same cases on the
HIP planner."""
import numpy as np
import pytest

import planner_oracle as PO
import planner_shapes_cases as SC

POLY_ROWS = {3, 5, 6, 7, 9, 10, 11, 12}


@pytest.fixture(scope="module")
def car():
    g = SC.golden()
    return g["circle_centers"], float(g["radius"])


def _tip(r):
    g = SC.golden()
    return np.array(r.start[:2]) + float(g["tip"]) * np.array([np.cos(r.start[2]), np.sin(r.start[2])])


def _distances(rows, p):
    return (rows[:, :2] @ p + rows[:, 2]) / np.hypot(rows[:, 0], rows[:, 1])


def _vertices(q, cap=None):
    """The corners of a half-plane set as the planner's host code finds them: pairwise intersections of the boundaries that
    satisfy every row, in its order; cap: stop after so many (it used to, after 128)."""
    v = []
    for i in range(len(q)):
        for j in range(i + 1, len(q)):
            if cap is not None and len(v) >= cap:
                break
            det = q[i, 0] * q[j, 1] - q[j, 0] * q[i, 1]
            if abs(det) <= 1e-12 * (abs(q[i, 0]) + abs(q[i, 1])) * (abs(q[j, 0]) + abs(q[j, 1])):
                continue
            p = np.array([(q[i, 1] * q[j, 2] - q[j, 1] * q[i, 2]) / det, (q[j, 0] * q[i, 2] - q[i, 0] * q[j, 2]) / det])
            if np.all(q[:, :2] @ p + q[:, 2] <= 1e-9 * (1.0 + np.abs(q[:, 2]) + (np.abs(q[:, 0]) + np.abs(q[:, 1])) * np.abs(p).sum())):
                v.append(p)
    return np.array(v)


@pytest.mark.parametrize("fam", SC.FAMILIES)
def test_every_probe_is_the_oracles(pkg, car, fam):
    rad, cen = pkg.planner.car_circles()
    assert rad == car[1] and np.array_equal(cen, car[0])
    mps = SC.straight(PO)
    _, routes = SC.probes(fam)
    for i, r in enumerate(routes):
        status, _, _, prims, ne = SC.solve(PO, r, mps, *car)
        assert (status, ne) == (r.status, r.n_expanded), (fam, i)
        assert (status, ne, prims) in ((1, 1, []), (0, 2, [0])), (fam, i)      # blocked at the start / one primitive, nothing else


@pytest.mark.parametrize("fam", SC.FAMILIES)
def test_every_row_of_every_probed_obstacle_decides_both_outcomes(fam):
    """For every (obstacle, row, variant): one probe blocked and one free; and on the geometry: the tip is 0.05 m from row i, the
    blocked tip is accepted by every row, the free tip is rejected by row i (and its copies) ALONE -- a walk that skipped or
    repeated a row, or read a pad slot as a row, changes one of the two."""
    g = SC.golden()
    eps = float(g["probe_eps"])
    obst, routes = SC.probes(fam)
    seen = {}
    for r in routes:
        if r.row < 0:
            continue
        # (pos: one 12-gon, moved for every probe)
        seen.setdefault((-1 if fam == "pos" else r.target, r.row, r.variant), set()).add((r.inside, r.status))
        rows = r.obstacles[r.ids.index(r.target)] if fam == "pos" else r.obstacles[0]
        base = obst[r.target] if fam == "red" else rows
        d = _distances(rows, _tip(r))
        own = _distances(base, _tip(r))[r.row]
        assert abs(own - (-eps if r.inside else eps)) < 1e-9
        if r.inside:
            assert np.all(d <= -0.04)
        else:
            assert np.all((d <= -0.04) | (np.abs(d - eps) < 1e-9)) and np.any(np.abs(d - eps) < 1e-9)
    for key, outcomes in seen.items():
        assert outcomes == {(1, 1), (0, 0)}, (fam, key, outcomes)
    n_rows = lambda k: 12 if k < 0 else len(obst[k])
    targets = sorted({t for t, _, _ in seen})
    for t in targets:                                        # every row index of the obstacle, in every variant
        for v in {v for tt, _, v in seen if tt == t}:
            assert {row for tt, row, vv in seen if tt == t and vv == v} == set(range(n_rows(t))), (fam, t, v)
    if fam == "poly":
        assert {n_rows(t) for t in targets} == POLY_ROWS       # the pad slots of both walks: 3; 5, 6, 7; 9, 10, 11 (and 12: none)
        for r in routes:                                     # variant 1: the 2 x 2 transform (start at the origin), 0: the 3 x 3
            assert (r.start[0] == 0.0 and r.start[1] == 0.0) == (r.variant == 1)
        for t in targets:                                    # rotated, unnormalised, away from the origin
            rows = obst[t]
            nrm = np.hypot(rows[:, 0], rows[:, 1])
            assert nrm.max() / nrm.min() > 1.5
            ang = np.degrees(np.arctan2(rows[:, 1], rows[:, 0])) % 45.0
            assert np.all(np.minimum(ang, 45.0 - ang) > 1e-3)
    if fam == "unb":
        assert sorted(n_rows(t) for t in targets) == [1, 2, 2]
        empty = [r for r in routes if r.row < 0]
        assert len(empty) == 2 and all(len(r.obstacles[0]) == 0 and r.status == 1 and r.n_expanded == 1 for r in empty)
        assert {r.start[:2] == (0.0, 0.0) for r in empty} == {True, False}
        strip = [obst[t] for t in targets if n_rows(t) == 2]
        cross = sorted(abs(float(s[0, 0] * s[1, 1] - s[0, 1] * s[1, 0])) / float(np.prod(np.hypot(s[:, 0], s[:, 1]))) for s in strip)
        assert cross[0] < 1e-12 and cross[1] > 0.5           # a strip of two parallel rows, a wedge
    if fam == "red":
        assert {(r.variant, len(r.obstacles[0])) for r in routes} == {(0, 16), (0, 12), (1, 64), (2, 64), (3, 32)}
        by = {}
        for r in routes:
            by.setdefault((r.target, r.row, r.inside), {})[r.variant] = (r.status, r.n_expanded)
        for key, out in by.items():                          # outcomes equal those of the de-duplicated polygon
            assert len(out) in (2, 3) and all(o == out[0] for o in out.values()), key
        gon16 = [t for t in targets if n_rows(t) == 16][0]
        assert len({r.row for r in routes if r.target == gon16}) == 16      # probed from 16 directions (and the 12-gon from 12)
        rep = [r for r in routes if r.variant == 1][0].obstacles[0]
        til = [r for r in routes if r.variant == 2][0].obstacles[0]
        assert np.array_equal(rep, np.repeat(obst[gon16], 4, axis=0)) and np.array_equal(til, np.tile(obst[gon16], (4, 1)))
    if fam == "pos":
        assert {r.variant for r in routes} == {0, 32, 63}
        for r in routes:
            assert len(r.obstacles) == 64 and sum(len(o) for o in r.obstacles) == 512 and r.ids.index(r.target) == r.variant
            # the 63 others: in reach of the pruning circle (within the tip's reach of the start), so the walk passes them
            for k, o in zip(r.ids, r.obstacles):
                if k != r.target:
                    assert float(np.hypot(*(_vertices(o).mean(axis=0) - np.array(r.start[:2])))) < float(g["tip"])


def test_the_wrong_pruning_circle_of_repeated_rows():
    """The host's vertex search as it was (it stopped after 128 vertices) on the 16-gon with every row four times: a circle that
    does not contain the polygon -- which is why the "red" probes exist; without the stop, it does."""
    obst, routes = SC.probes("red")
    gon = [o for o in obst if len(o) == 16][0]
    rows = np.repeat(gon, 4, axis=0)

    def circle(q, cap):
        v = _vertices(q, cap)
        c = v.mean(axis=0)
        return c, float(np.hypot(*(v - c).T).max())

    corners = np.array([10.0, 0.0]) + 3.06 * np.stack([np.cos(np.arange(16) * np.pi / 8), np.sin(np.arange(16) * np.pi / 8)], axis=1)
    c, r = circle(rows, 128)
    assert np.hypot(*(corners - c).T).max() > r + 1.0                          # (centre (10.57, 1.88), r = 3.30)
    c, r = circle(rows, None)
    assert np.hypot(*(corners - c).T).max() <= r + 1e-9


def test_cheap_searches_are_the_oracles_and_hang_on_their_obstacles(pkg):
    """Every stored search of at most 250 expansions again, bit for bit; and without its key obstacle the route is another one
    (the primitive sequence is compared: expansion counts barely move when a polygon loses a row)."""
    PL = pkg.planner
    n_cheap = n_key = 0
    for name in SC.CONFIGS:
        cfg = SC.config(name)
        mps = SC.oracle_mps(cfg.points, cfg.length)
        for j, r in enumerate(cfg.routes):
            assert r.n_expanded <= 1500
            if r.n_expanded > 250:
                continue
            status, cost, path, prims, ne = SC.solve(PO, r, mps, cfg.centres, cfg.radius)
            assert (status, prims, ne) == (r.status, r.prims, r.n_expanded), (name, j)
            if status == 0:
                assert cost == r.cost and np.array_equal(path, r.path), (name, j)
            n_cheap += 1
            if r.key_obstacle >= 0:
                rest = r.obstacles[:r.key_obstacle] + r.obstacles[r.key_obstacle + 1:]
                assert SC.solve(PO, r, mps, cfg.centres, cfg.radius, obstacles=rest, max_expansions=1500)[3] != r.prims, (name, j)
                n_key += 1
    assert n_cheap >= 10 and n_key >= 9


def test_search_configurations_cover_the_passes_and_the_sets(pkg):
    """(primitive, collision point) pairs in every bucket of the kernel's four passes of 64 lanes, a primitive with exactly
    JPL_MAX_CC = 16 points, 1 / 3 / 9 / 16 primitives, 31 and 61 points, 1 ... 4 circles -- counted with the PRODUCT's collision
    points, which are the oracle's."""
    PL = pkg.planner
    buckets, sets = set(), set()
    for name in SC.CONFIGS:
        cfg = SC.config(name)
        for p in cfg.points:
            assert np.array_equal(PL.collision_points(p, cfg.centres, cfg.radius), PO.collision_points(p, cfg.centres, cfg.radius)[:, :2])
        pairs, most = SC.pair_count(PL, cfg)
        assert most <= PL.MAX_COLLISION_POINTS and len(cfg.points) <= PL.MAX_PRIMITIVES
        buckets.add(((pairs - 1) // 64, most == 16))
        sets.add((cfg.points.shape[0], cfg.points.shape[1], len(cfg.centres)))
        for r in cfg.routes:                                 # general polygons, asymmetric fields
            assert {len(o) for o in r.obstacles} - {4} and len(r.obstacles) <= 64 and sum(len(o) for o in r.obstacles) <= 512
    assert {b for b, _ in buckets} == {0, 1, 2, 3} and (3, True) in buckets
    assert {s[0] for s in sets} == {1, 3, 9, 16} and {s[1] for s in sets} == {31, 61} and {s[2] for s in sets} == {1, 2, 3, 4}


def test_table_limit_cases_are_what_they_claim(pkg):
    PL = pkg.planner
    g = SC.golden()
    r = SC.config("p9n31").routes[0]
    assert len(SC.too_many_obstacles(r).obstacles) == PL.MAX_OBSTACLES + 1
    assert sum(len(o) for o in SC.too_many_rows(r).obstacles) == PL.MAX_HALFPLANES + 1 and len(SC.too_many_rows(r).obstacles) <= PL.MAX_OBSTACLES
    n = [len(PL.collision_points(p, g["cc17_centres"], float(g["cc17_radius"]))) for p in g["cc17_mp_points"]]
    assert n == [PL.MAX_COLLISION_POINTS, PL.MAX_COLLISION_POINTS + 1]
    # the reference's cyclist (L = 1.0, width = 0.45, extra_length = 0.64) on the stock primitives: 34 collision points each
    rad, cen = PL.car_circles(L=1.0, width=0.45, extra_length=0.64)
    pts, _ = PL.make_motion_primitives()
    assert {len(PL.collision_points(p, cen, rad)) for p in pts} == {34}
    assert len(PO.collision_points(pts[0], cen, rad)) == 34


def test_open_space_and_start_in_goal_on_the_oracle():
    """The route-level cases the GPU test solves with the oracle on the spot stay cheap; and what the oracle says of a start that
    passes the goal test: popped, found -- one expansion, cost 0, the path is the start alone (its trajectory() cannot join zero
    segments: the search is stepped up to the goal test only)."""
    for name in SC.CONFIGS:
        cfg = SC.config(name)
        mps = SC.oracle_mps(cfg.points, cfg.length)
        r = cfg.routes[0]
        status, cost, path, prims, ne = SC.solve(PO, SC.open_space(r), mps, cfg.centres, cfg.radius, max_expansions=400)
        assert status == 0 and len(prims) >= 1
        s = SC.start_in_goal(r)
        orc = PO.PlannerOracle(s.start, s.goal, s.goal_box, s.tol, s.obstacles, mps, cfg.centres, cfg.radius)
        assert orc.is_goal(s.start)


def test_status_messages_tell_which_limit(pkg):
    PL = pkg.planner
    route = lambda status: PL.PlannedRoute(status=status, cost=0.0, prims=np.zeros(0, np.int32), nodes=np.zeros((0, 3)), trajectory=np.zeros((0, 3)), n_expanded=0)
    with pytest.raises(RuntimeError, match="status 5") as e:
        PL._raise_unless_found(route(5), 32)
    msg = str(e.value)
    assert "64 obstacles" in msg and "512 half-planes" in msg and "16 primitives" in msg and "16 collision points" in msg
    assert "longer than max_path" not in msg
    with pytest.raises(RuntimeError, match="6: path longer than max_path = 7"):
        PL._raise_unless_found(route(6), 7)
    with pytest.raises(RuntimeError, match="node_cap"):
        PL._raise_unless_found(route(4), 7)
    with pytest.raises(Exception, match="No solution found"):
        PL._raise_unless_found(route(1), 7)
    PL._raise_unless_found(route(0), 7)
