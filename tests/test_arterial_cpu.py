"""The arterial road of the overtaking study (planner.arterial_obstacles / arterial_query) without a GPU: every
scene of tests/golden/arterial.npz -- the reference's ArterialMultiLanes.create_scenario for several (num_lanes, goal_lane) pairs and
three replan situations, stored as data -- against the geometry written here, and the oracle's routes on the stored scenes against
the stored routes of the reference's planner."""
import numpy as np
import pytest

from conftest import load_golden


def scene_kwargs(g, i):
    nl, gl = (int(v) for v in g[f"s{i}_lanes"])
    replan = None
    if int(g[f"s{i}_replan"]):
        replan = dict(trajectory=g[f"s{i}_trajectory"], spawn=tuple(g[f"s{i}_spawn"]), av=tuple(g[f"s{i}_av"]))
    return dict(num_lanes=nl, goal_lane=gl, replan=replan)


def stored_primitives(g, i):
    return [("box", (w, h), (cx, cy), bool(hid)) for w, h, cx, cy, hid in g[f"s{i}_obs"]]


def test_scenes_equal_the_references(pkg):
    PL = pkg.planner
    g = load_golden("arterial.npz")
    n = int(g["n_scenes"])
    rad, cen = PL.car_circles()
    assert rad == float(g["radius"]) and np.array_equal(cen, g["circle_centers"])
    assert n >= 8 and sum(int(g[f"s{i}_replan"]) for i in range(n)) == 3 and len({tuple(g[f"s{i}_lanes"]) for i in range(n)}) >= 5
    for i in range(n):
        label, kw = str(g["labels"][i]), scene_kwargs(g, i)
        q = PL.arterial_query(rad, **kw)
        assert q.start == tuple(g[f"s{i}_start"]) and q.goal == tuple(g[f"s{i}_goal"]), label          # exactly equal
        assert q.goal_box == tuple(g[f"s{i}_goal_box"]) and q.tol == float(g[f"s{i}_tol"]), label
        prims = PL.arterial_obstacles(**kw)
        assert len(prims) == len(g[f"s{i}_obs"]) == 3 and not any(p[3] for p in prims), label
        for margin in (0.0, rad):
            assert np.array_equal(PL.static_obstacle_rows(prims, margin), PL.static_obstacle_rows(stored_primitives(g, i), margin)), label
        r = int(g[f"s{i}_route"])
        if r >= 0:            # the half-planes the reference's own to_convex(margin = radius) gave its planner
            off = g[f"r{r}_hp_off"]
            assert len(q.obstacles) == len(off) - 1
            for k, hp in enumerate(q.obstacles):
                assert np.array_equal(hp, g[f"r{r}_hp"][off[k]:off[k + 1]]), (label, k)
    # the plain road: two pavements and the closed left road; the replan form opens the left road and boxes the cyclist's prediction
    plain = PL.arterial_obstacles()
    assert plain[0][2][0] == -plain[1][2][0] == -5.5 and plain[2] == ("box", (4.0, 44.0), (-2.0, 0), False)
    traj = np.array([[2.0, 1.0 + 0.5 * k] for k in range(20)])
    box = PL.arterial_obstacles(replan=dict(trajectory=traj, spawn=(2.0, 1.0), av=(2.0, -9.0)))[2]
    assert box == ("box", (1.64, 9.5), (2.0, 1.0 + 9.5 / 2), False)
    assert PL.arterial_query(rad, replan=dict(trajectory=traj, spawn=(2.0, 1.0), av=(1.9, -9.0))).start == (1.9, -9.0, np.pi / 2)
    # the constants are keywords
    wide = PL.arterial_query(rad, width_road=3.5, length=60.0, y_goal=30.0)
    assert wide.start == (1.75, -30.0, np.pi / 2) and wide.goal == (2.0, 30.0, np.pi / 2)
    assert PL.arterial_obstacles(width_road=3.5, length=60.0)[2] == ("box", (3.5, 60.0), (-1.75, 0), False)
    for kw, msg in ((dict(num_lanes=0), "at least one lane"), (dict(num_lanes=2, goal_lane=3), "goal lane 3 of 2")):
        with pytest.raises(ValueError, match=msg):
            PL.arterial_query(rad, **kw)
    with pytest.raises(ValueError, match="predicted trajectory"):
        PL.arterial_obstacles(replan=dict(trajectory=[1.0, 2.0], spawn=(0, 0), av=(0, 0)))


def test_planner_oracle_on_the_arterial_road(pkg):
    """As tests/test_planner.py checks planner_envs.npz: the oracle's route on each stored scene is the reference's, bit for bit -- all
    four of them (the longest search, 4085 expansions, takes the numpy oracle about 3 s)."""
    import planner_oracle as PO
    PL = pkg.planner
    g = load_golden("arterial.npz")
    mps = PO.make_motion_primitives()
    rad = float(g["radius"])
    checked = 0
    for r in range(int(g["n_routes"])):
        i = int(g[f"r{r}_scene"])
        assert int(g[f"s{i}_route"]) == r
        q = PL.arterial_query(rad, **scene_kwargs(g, i))
        orc = PO.PlannerOracle(q.start, q.goal, q.goal_box, q.tol, q.obstacles, mps, g["circle_centers"], rad)
        cost, path, traj = orc.run()
        assert cost == float(g[f"r{r}_cost"]) and np.array_equal(np.array(path), g[f"r{r}_path"]) and np.array_equal(traj, g[f"r{r}_traj"])
        assert orc.prim_sequence(path) == list(g[f"r{r}_prims"]) and orc.n_expanded == int(g[f"r{r}_n_expanded"])
        checked += 1
    assert checked == 4
    # the plain two-lane road: cost 44.82, 10 nodes, a 540-point straight line
    assert round(float(g["r0_cost"]), 2) == 44.82 and g["r0_path"].shape == (10, 3) and g["r0_traj"].shape == (540, 3)
    assert np.ptp(g["r0_traj"][:, 0]) <= 1e-12                                        # (cos(pi / 2) is 6e-17, not 0)
    assert all(float(g[f"r{r}_traj"][:, 0].min()) < 0.0 for r in range(1, 4))       # every replan route swerves over the centre line
