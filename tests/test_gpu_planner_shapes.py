"""The HIP route planner on general shapes and at its table limits, against oracle/planner_oracle.py (its outcomes stored in
tests/golden/planner_shapes.npz; tests/test_planner_shapes_cpu.py shows on the CPU what the cases cover).  Collision probes: one
launch per family, hundreds of routes of one expansion each, status and expansion count exact.  Searches: the bars of
tests/test_planner.py (identical primitive sequence, cost <= 1e-9 max(1, |cost|), nodes / trajectory <= 1e-9, expansions within
max(1, n // 50)).

What the cases are after: the "red" probes run into a 16-gon with every row listed four times in a row, for which the host's
vertex search used to stop at 128 of 256 vertex hits and draw the pruning circle around one side of the polygon only
(tests/test_planner_shapes_cpu.py restates that circle: it misses the far corners by more than a metre), so that probes from the
other side skipped the obstacle's collision test and came out free."""
import numpy as np
import pytest

import planner_oracle as PO
import planner_shapes_cases as SC

pytestmark = pytest.mark.gpu


def _straight(PL):
    pts, length = PL.make_motion_primitives()
    return pts[:1], length[:1]


@pytest.mark.parametrize("fam", SC.FAMILIES)
def test_collision_probes(pkg, fam):
    """Every probe of the family in ONE launch: blocked -> status 1 after one expansion, free -> status 0 with the one primitive."""
    PL = pkg.planner
    _, routes = SC.probes(fam)
    res = PL.plan_routes([SC.query(PL, r) for r in routes], primitives=_straight(PL), max_path=4, node_cap=64, retry_node_cap=0)
    wrong = [(i, r.target, r.row, r.inside, r.variant, (o.status, o.n_expanded), (r.status, r.n_expanded))
             for i, (r, o) in enumerate(zip(routes, res)) if (o.status, o.n_expanded) != (r.status, r.n_expanded)]
    print(f"{fam}: {len(routes)} probes, {len(wrong)} wrong (index, obstacle, row, inside, variant, got, oracle): {wrong}")
    assert not wrong
    for r, o in zip(routes, res):
        if r.status == 0:
            assert list(o.prims) == [0] and o.nodes.shape == (2, 3) and o.trajectory.shape == (60, 3)
            assert np.array_equal(o.nodes[0], np.array(r.start))
            np.testing.assert_allclose(o.nodes[1], np.array(r.goal), rtol=0, atol=1e-9)
        else:
            assert len(o.prims) == 0 and len(o.trajectory) == 0
    if fam == "red":                                             # rows that add nothing change nothing
        by = {}
        for r, o in zip(routes, res):
            by.setdefault((r.target, r.row, r.inside), {})[r.variant] = (o.status, o.n_expanded)
        assert all(v == out[0] for out in by.values() for v in out.values())


@pytest.mark.parametrize("name", SC.CONFIGS)
def test_searches_with_other_primitive_and_circle_sets(pkg, name):
    """One launch per configuration: its stored searches, and behind them routes at the table limits, which end with status 5 and
    leave the others as they are; a route without an obstacle; a start that already passes the goal test."""
    PL = pkg.planner
    cfg = SC.config(name)
    mps = SC.oracle_mps(cfg.points, cfg.length)
    kw = dict(primitives=(cfg.points, cfg.length), circles=(cfg.radius, cfg.centres), max_path=24)
    r0 = cfg.routes[0]
    extra = [SC.open_space(r0), SC.too_many_obstacles(r0), SC.too_many_rows(r0), SC.start_in_goal(r0)]
    pairs, most = SC.pair_count(PL, cfg)
    print(f"{name}: {len(cfg.points)} primitives x {cfg.points.shape[1]} points, {len(cfg.centres)} circles, {pairs} pairs (at most {most} per primitive)")
    res = PL.plan_routes([SC.query(PL, r) for r in cfg.routes + extra], **kw)
    n = len(cfg.routes)
    for j, r in enumerate(cfg.routes):
        SC.assert_route(PO, res[j], r, cfg.points, f"{name} route {j} (seed {r.seed})")
    # no obstacle at all: the oracle on the spot (tests/test_planner_shapes_cpu.py keeps it below 400 expansions)
    status, cost, path, prims, ne = SC.solve(PO, extra[0], mps, cfg.centres, cfg.radius, max_expansions=400)
    want = SC.NS(status=status, cost=cost, path=path, prims=prims, n_expanded=ne)
    SC.assert_route(PO, res[n], want, cfg.points, f"{name} without obstacles")
    for k in (1, 2):                                             # 65 obstacles; 513 half-planes
        assert res[n + k].status == 5 and res[n + k].n_expanded == 0 and len(res[n + k].prims) == 0 and len(res[n + k].trajectory) == 0
    s = res[n + 3]                                               # found before anything is expanded
    assert s.status == 0 and len(s.prims) == 0 and s.cost == 0.0 and s.n_expanded == 1 and len(s.trajectory) == 0
    assert s.nodes.shape == (1, 3) and np.array_equal(s.nodes[0], np.array(extra[3].start))
    # the same searches alone: bit for bit what they were beside the routes that were turned away
    alone = PL.plan_routes([SC.query(PL, r) for r in cfg.routes], **kw)
    for a, b in zip(alone, res[:n]):
        assert (a.status, a.n_expanded, a.cost) == (b.status, b.n_expanded, b.cost) or (a.status == b.status == 1 and a.n_expanded == b.n_expanded)
        assert np.array_equal(a.prims, b.prims) and np.array_equal(a.nodes, b.nodes) and np.array_equal(a.trajectory, b.trajectory)


def test_a_launch_without_any_obstacle(pkg):
    """n_obs_total = 0, the half-plane array empty: three routes of the nine-primitive set through open space."""
    PL = pkg.planner
    cfg = SC.config("p9n31")
    mps = SC.oracle_mps(cfg.points, cfg.length)
    qs = [SC.open_space(r) for r in cfg.routes]
    res = PL.plan_routes([SC.query(PL, q) for q in qs], primitives=(cfg.points, cfg.length), circles=(cfg.radius, cfg.centres))
    for j, (q, o) in enumerate(zip(qs, res)):
        status, cost, path, prims, ne = SC.solve(PO, q, mps, cfg.centres, cfg.radius, max_expansions=1500)
        SC.assert_route(PO, o, SC.NS(status=status, cost=cost, path=path, prims=prims, n_expanded=ne), cfg.points, f"open space {j}")


def test_collision_point_and_primitive_limits(pkg):
    """JPL_MAX_CC = 16: a primitive with 17 collision points (the other has 16), and the reference's cyclist -- 34 per primitive --
    end every route of the launch with status 5, which the class surface reports as what it is; 17 primitives are refused."""
    from types import SimpleNamespace as NS
    PL = pkg.planner
    g = SC.golden()
    cfg = SC.config("p9n31")
    qs = [SC.query(PL, r) for r in cfg.routes]
    res = PL.plan_routes(qs, primitives=(g["cc17_mp_points"], g["cc17_mp_length"]), circles=(float(g["cc17_radius"]), g["cc17_centres"]))
    assert [(r.status, r.n_expanded, len(r.prims)) for r in res] == [(5, 0, 0)] * len(qs)
    cyclist = PL.car_circles(L=1.0, width=0.45, extra_length=0.64)
    res = PL.plan_routes(qs, circles=cyclist)
    assert [(r.status, r.n_expanded, len(r.prims)) for r in res] == [(5, 0, 0)] * len(qs)
    pts, length = PL.make_motion_primitives()
    mps = {n: NS(points=pts[k], total_length=float(length[k])) for k, n in enumerate(PL.MP_NAMES)}
    r = cfg.routes[0]
    scen = NS(start=r.start, goal_point=r.goal, goal_area=NS(xy1=r.goal_box[:2], xy2=r.goal_box[2:]), allowed_goal_theta_difference=r.tol,
              obstacles=[NS(to_convex=(lambda margin, o=o: o)) for o in r.obstacles])
    with pytest.raises(RuntimeError, match="16 collision points per primitive") as e:
        PL.MotionPrimitiveSearch(scen, NS(radius=cyclist[0], circle_centers=cyclist[1]), mps, margin=0.0).run()
    assert "status 5" in str(e.value) and "longer than max_path" not in str(e.value)
    p16 = SC.config("p16c2")
    p17 = (np.concatenate([p16.points, p16.points[:1]]), np.concatenate([p16.length, p16.length[:1]]))
    with pytest.raises(pkg._cabi.JsimError, match="primitives 17"):
        PL.plan_routes(qs[:1], primitives=p17)


def test_max_path_at_the_path_length_and_one_below(pkg):
    PL = pkg.planner
    cfg = SC.config("p9n31")
    r = cfg.routes[0]
    n = len(r.prims)
    assert n >= 3
    kw = dict(primitives=(cfg.points, cfg.length), circles=(cfg.radius, cfg.centres))
    fits = PL.plan_routes([SC.query(PL, r)], max_path=n, **kw)[0]
    SC.assert_route(PO, fits, r, cfg.points, f"max_path = {n}")
    short = PL.plan_routes([SC.query(PL, r)], max_path=n - 1, **kw)[0]
    assert short.status == 6 and len(short.prims) == 0 and len(short.trajectory) == 0
    assert abs(short.n_expanded - r.n_expanded) <= max(1, r.n_expanded // 50)
