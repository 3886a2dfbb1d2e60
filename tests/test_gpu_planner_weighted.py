"""Per-route planner weights on the GPU (jsim_plan_routes_weighted): the multi-trajectory planner's searches (form 1) against
the reference-made fixture tests/golden/planner_multi.npz, all combinations of a scenario in one launch; mixed batches of both
forms; the launch-wide entry point as a wrapper; planner.MultiTrajectorySearch.run_all() through the shim name; the planner
sensitivity sweep as one batch.  Bars as in tests/test_planner.py: identical primitive sequence, cost / nodes / trajectory <= 1e-9,
expansion count within max(1, n / 50)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
import planner_multi_cases as MC

pytestmark = pytest.mark.gpu


def _check_against_fixture(g, i, j, cost, nodes, traj, prims, n_expanded):
    k = f"s{i}_c{j}_"
    ne = int(g[k + "n_expanded"])
    print(f"scenario {i} combination {j} wh {g[k + 'wh']}: expansions {n_expanded} (fixture {ne}), |cost - fixture| {abs(cost - float(g[k + 'cost'])):.3e}")
    assert list(prims) == list(g[k + "prims"]), (i, j)
    assert abs(cost - float(g[k + "cost"])) <= 1e-9, (i, j)
    np.testing.assert_allclose(np.asarray(nodes), g[k + "path"], rtol=0, atol=1e-9)
    assert np.asarray(traj).shape == g[k + "traj"].shape
    np.testing.assert_allclose(traj, g[k + "traj"], rtol=0, atol=1e-9)
    if n_expanded is not None:
        assert abs(n_expanded - ne) <= max(1, ne // 50), (i, j, n_expanded, ne)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_hip_form1_against_the_reference_fixture_one_launch_per_scenario(pkg, i):
    PL = pkg.planner
    g = MC.golden()
    q = MC.stored_query(PL, g, i)
    combos = MC.combos(g, i)
    wh = np.array([[e, p, o, 0.0, 0.0] for e, p, o in combos])
    res = PL.plan_routes([q] * len(combos), wh=wh, wc=g[f"s{i}_wc"], form=PL.FORM_MULTI)       # ONE launch
    for j, r in enumerate(res):
        assert r.status == 0, (i, j, r.status)
        _check_against_fixture(g, i, j, r.cost, r.nodes, r.trajectory, r.prims, r.n_expanded)
    assert len({tuple(r.prims) for r in res}) >= 3                              # the weights are not ignored


def test_mixed_batch_of_both_forms_equals_each_route_alone(pkg):
    """Form 0 and form 1 routes with distinct weight rows, on different scenarios, in one launch: each route bit for bit what the
    same route gives launched alone, whatever its place in the batch."""
    PL = pkg.planner
    g = MC.golden()
    rad = PL.car_circles()[0]
    q0, q1, q2 = (MC.stored_query(PL, g, i) for i in (0, 1, 2))
    q3 = PL.intersection_query(2, 3, rad)
    cases = [(q0, (1.0, 2.7, 15.0, 0.0, 0.0), (1.0, 5.0, 0.1, 0.0), 1), (q2, (1.0, 2.7, 15.0, 0.0, 0.0), (1.0, 5.0, 0.1, 0.0), 0),
             (q2, (1.0, 2.7, 15.0, 0.0, 0.0), (1.0, 5.0, 0.1, 0.0), 1), (q1, (10.0, 2.7, 15.0, 0.0, 0.0), (1.0, 5.0, 0.1, 0.0), 1),
             (q1, (1.0, 2.7, 15.0, 0.0, 0.0), (0.0, 10.0, 0.1, 0.0), 0), (q3, (1.1, 2.0, 12.0, 0.7, 0.05), (0.9, 4.0, 0.3, 0.02), 0),
             (q3, (3.0, 0.5, 2.0, 9.0, 9.0), (0.9, 4.0, 0.0, 0.02), 1), (q0, (1.5, 2.7, 15.0, 0.0, 0.0), (1.0, 5.0, 0.0, 0.0), 1)]
    alone = [PL.plan_routes([q], wh=wh, wc=wc, form=f)[0] for q, wh, wc, f in cases]
    assert all(r.status == 0 for r in alone)
    assert alone[1].cost != alone[2].cost                                       # same scenario and weights, the other form: another search
    # wh[3], wh[4] are not read by form 1
    MC.assert_same_route(alone[6], PL.plan_routes([q3], wh=(3.0, 0.5, 2.0, 0.0, 0.0), wc=cases[6][2], form=1)[0])
    for order in (list(range(8)), [7, 2, 5, 0, 3, 6, 1, 4]):
        batch = PL.plan_routes([cases[k][0] for k in order], wh=np.array([cases[k][1] for k in order]),
                               wc=np.array([cases[k][2] for k in order]), form=np.array([cases[k][3] for k in order]))
        for r, k in zip(batch, order):
            MC.assert_same_route(r, alone[k])


def test_launch_wide_entry_point_equals_broadcast_weights_form0(pkg):
    """jsim_plan_routes == jsim_plan_routes_weighted with its row repeated and form 0, bit for bit, on the 18 reference routes of
    planner.npz (which the launch-wide call must still reproduce)."""
    PL = pkg.planner
    g = load_golden("planner.npz")
    rad = PL.car_circles()[0]
    qs = []
    for i in range(int(g["n_routes"])):
        kind, sp, tn, sl, gl = (int(v) for v in g[f"r{i}_meta"])
        qs.append(PL.intersection_query(sp, tn, rad, sl or 1, gl or 1, number_of_lanes=2 if kind else 0))
    assert len(qs) == 18
    rc_a, a = MC.call_entry(pkg, "jsim_plan_routes", qs, PL.WH_DEFAULT, PL.WC_DEFAULT)
    wh, wc, form = PL.weight_tables(18)
    rc_b, b = MC.call_entry(pkg, "jsim_plan_routes_weighted", qs, wh, wc, form)
    assert rc_a == 0 and rc_b == 0 and np.all(a["status"] == 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for i in range(18):
        n = int(a["n_prims"][i])
        assert list(a["prims"][i, :n]) == list(g[f"r{i}_prims"])
        assert abs(a["cost"][i] - float(g[f"r{i}_cost"])) <= 1e-9
        np.testing.assert_allclose(a["traj"][i, :n * 60], g[f"r{i}_traj"], rtol=0, atol=1e-9)


def test_multi_trajectory_search_run_all_through_the_shim_in_one_launch(pkg, monkeypatch):
    spec = importlib.util.spec_from_file_location("shim_multi_trajectory_generator", os.path.join(REPO, "shim", "lib", "multi_trajectory_generator.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    PL = pkg.planner
    g = MC.golden()
    lib = pkg._cabi.load()
    calls = []
    for name in ("jsim_plan_routes_weighted", "jsim_plan_routes"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (calls.append((_n, a[1])), _fn(*a))[1])
    for i in (0, 2):
        q = MC.stored_query(PL, g, i)
        scen, car, mps = MC.objects(PL, q, g)
        wc = g[f"s{i}_wc"]
        lists = dict(wh_ego=[float(v) for v in g[f"s{i}_wh_ego"]], wh_policy=[float(v) for v in g[f"s{i}_wh_policy"]],
                     wh_other=[float(v) for v in g[f"s{i}_wh_other"]])
        s = shim.MotionPrimitiveSearch(scen, car, mps, margin=car.radius, wc_dist=wc[0], wc_steering=wc[1], wc_obstacle=wc[2], wc_center=wc[3], **lists)
        del calls[:]
        sols = s.run_all()
        assert calls == [("jsim_plan_routes_weighted", int(g[f"s{i}_n_comb"]))]                 # ONE launch, every combination in it
        assert [tuple(sol[3:]) for sol in sols] == MC.combos(g, i)                               # the reference's order
        for j, (cost, path, traj, e, p, o) in enumerate(sols):
            assert isinstance(path, list) and isinstance(path[0], tuple)
            _check_against_fixture(g, i, j, cost, path, traj, s.last[j].prims, s.last[j].n_expanded)
            assert [s._points_to_mp_names[a, b] for a, b in zip(path[:-1], path[1:])] == [PL.MP_NAMES[k] for k in g[f"s{i}_c{j}_prims"]]
    # run(): the sums of the lists (here 1.0 + 0.5 = 1.5, 2.7, 15 = combination 1 of scenario 0)
    q = MC.stored_query(PL, g, 0)
    scen, car, mps = MC.objects(PL, q, g)
    s = shim.MotionPrimitiveSearch(scen, car, mps, margin=car.radius, wh_ego=[1.0, 0.5], wh_policy=[2.7], wh_other=[10, 5])
    cost, path, traj = s.run()
    _check_against_fixture(g, 0, 1, cost, path, traj, s.last[0].prims, s.last[0].n_expanded)
    # a combination whose open list runs empty: the reference's loop raises on reaching it
    from types import SimpleNamespace as NS
    walled = NS(start=(0.0, 0.0, 0.0), goal_point=(60.0, 0.0, 0.0), goal_area=NS(xy1=(59.0, -1.0), xy2=(61.0, 1.0)), allowed_goal_theta_difference=np.pi / 16,
                obstacles=[NS(to_convex=lambda margin: PL.box_halfplanes((49.0, 100.0), (25.5, 0.0), margin))])
    with pytest.raises(Exception, match="No solution found"):
        shim.MotionPrimitiveSearch(walled, car, mps, margin=0.0, wh_ego=[1.0, 2.0], wh_policy=[2.7], wh_other=[15]).run_all()


def test_planner_sensitivity_sweep_as_one_batch(pkg):
    """main/planner/Planner_Sensitivity_TrueCost.py:38-45: wc_dist in {0, 1} x wc_steering in {0, 10} on the two-lane scenario
    (start 1, turn 1, lane 1 -> 1), one MotionPrimitiveSearch per combination there -- here one batch of four, each route bit for
    bit the single run's.  (All four combinations finish in the capped CPU screening -- 45, 35, 145 and 324 expansions -- none is
    dropped.)"""
    from itertools import product
    PL = pkg.planner
    g = MC.golden()
    q = MC.stored_query(PL, g, 1)
    scen, car, mps = MC.objects(PL, q, g)
    combos = list(product([0, 1], [0, 10]))
    wc = np.array([[d, s, 0.1, 0.0] for d, s in combos], dtype=np.float64)
    batch = PL.plan_routes([q] * 4, wc=wc)
    assert len({tuple(r.prims) for r in batch}) == 4
    for r, (d, s) in zip(batch, combos):
        one = PL.MotionPrimitiveSearch(scen, car, mps, margin=car.radius, wc_dist=d, wc_steering=s)
        cost, path, traj = one.run()
        MC.assert_same_route(r, one.last)
        assert cost == r.cost and np.array_equal(traj, r.trajectory) and np.array_equal(np.array(path), r.nodes)
