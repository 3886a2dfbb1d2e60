"""Route vehicles (kind="route", jsim_loop_set_traffic_routes) without a GPU: the numpy restatement of the rule
(tests/traffic_route_numpy.py) against the reference's own vehicles played back along their recorded poses
(tests/golden/obstacles_scripted.npz), against stepping one counter at a time, and on the rule's edge cases; the entry point's
declaration, binding and documentation, and every refusal of the Python layer, none of which needs a device."""
import ctypes
import os
import types

import numpy as np
import pytest

import traffic_route_numpy as TR
from conftest import REPO, load_golden

L_CAR, DT = 2.86, 0.2
NO_ENGINE = types.SimpleNamespace(dt=0.2, B=1)      # all that a loop may read of its engine before it refuses a spec


def test_reference_vehicles_are_a_special_case():
    """Bicycle.step is explicit Euler, so a T-intersection vehicle played along its own poses at its own speed gives its get() tuples
    back: all six fields, ticks 0 .. 138, to 1e-9 (<= 140 additions of magnitude <= 60: about 1e-12; measured 3.2e-13)."""
    vehicles = TR.golden_vehicles(load_golden("obstacles_scripted.npz"))
    assert len(vehicles) == 4 and sorted(o for _, _, o, _ in vehicles) == [0.0, 0.0, 2.0, 4.0]
    worst, turned = 0.0, 0
    for route, speed, off, want in vehicles:
        S = TR.arc_length(route)
        got = np.array([TR.pose(route, S, c, 0, speed, off, 0.0, DT, 0, L_CAR) for c in range(139)])
        worst = max(worst, float(np.abs(got - want[:139]).max()))
        np.testing.assert_allclose(got, want[:139], rtol=0, atol=1e-9)
        turned += bool((want[:139, 5] != 0).any())
        # the snap decision is never in doubt: no s lies between 1e-11 and 1e-7 of a vertex
        for c in range(139):
            d = np.abs(S - TR.arc_at(c, speed, off, 0.0, DT, 0)[2]).min()
            assert d <= 1e-11 or d >= 1e-7, (c, d)
    print(f"max |restatement - reference get()| = {worst:.3e}")
    assert turned == 2                                                           # two of the four turn: the steering angle is compared


def irregular_route(seed, n):
    rng = np.random.default_rng(seed)
    xy = np.cumsum(rng.uniform(0.3, 1.7, (n, 2)) * [1.0, 0.4], axis=0)
    d = np.diff(xy, axis=0)
    yaw = np.arctan2(d[:, 1], d[:, 0])
    return np.column_stack([xy, np.append(yaw, yaw[-1])])


@pytest.mark.parametrize("end, offset, s0, period", [(0, 0.0, 0.0, 0), (1, 0.5, 1.7, 0), (0, 0.3, 0.4, 23), (1, 0.0, 0.0, 9)])
def test_closed_form_equals_stepping(end, offset, s0, period):
    route = irregular_route(5, 40)
    S = TR.arc_length(route)
    speed, n = 3.7, 90                                                           # (reaches the end at about tick 60 without a period)
    for c in range(n):                                                           # no arc length within the reach of a sum's rounding of a vertex
        assert np.abs(S - TR.arc_at(c, speed, offset, s0, DT, period)[2]).min() > 1e-7 or TR.arc_at(c, speed, offset, s0, DT, period)[2] == s0
    closed = np.array([TR.pose(route, S, c, end, speed, offset, s0, DT, period, L_CAR) for c in range(n)])
    np.testing.assert_allclose(closed, TR.stepped(route, n, end, speed, offset, s0, DT, period, L_CAR), rtol=0, atol=1e-9)
    # and the two calls per tick of jsim_loop_obstacles on a (state, param) row give the closed form's tuples and leave the pose of
    # the counter they end at
    get, state = TR.run([route], np.zeros((1, 4)), TR.case_rows([dict(route=0, end=end, speed=speed, offset=offset, s0=s0, dt=DT, period=period)]),
                        [L_CAR], n)
    assert np.array_equal(get[:, 0], closed)
    last = TR.pose(route, S, n, end, speed, offset, s0, DT, period, L_CAR)
    assert state[0, 3] == n and np.array_equal(state[0, :3], last[[0, 1, 3]])


def case_poses(name, n=70, L=L_CAR):
    k = TR.edge_cases()[name]
    route = TR.case_routes()[k["route"]]
    S = TR.arc_length(route)
    return k, route, S, np.array([TR.pose(route, S, c, k["end"], k["speed"], k["offset"], k["s0"], k["dt"], k["period"], L) for c in range(n)])


PARKED = [TR.PARK, TR.PARK, 0.0, 0.0, 0.0, 0.0]


def test_edge_cases_spelt_out():
    # offset / dt an exact integer: the vehicle moves at n0 = 5, not before
    k, route, S, g = case_poses("offset_integer_ticks")
    assert k["offset"] / k["dt"] == 4.0 and TR.start_tick(k["offset"], k["dt"]) == 5
    assert (g[:5, 2] == 0).all() and (g[:6, 0] == 0).all() and g[5, 2] == 2.0 and g[6, 0] == 0.5 and g[7, 0] == 1.0
    # a period of 7 ticks: ticks 6, 7, 8 are counters 6, 0, 1
    k, route, S, g = case_poses("period_wraps")
    assert np.array_equal(g[7], g[0]) and np.array_equal(g[8], g[1]) and np.array_equal(g[13], g[6]) and g[6, 0] > g[5, 0] > g[7, 0]
    assert g[0, 2] == 6.3 and np.array_equal(g[0, :2], TR.pose(route, S, 0, 0, 0.0, 0.0, 2.0, 0.2, 0, L_CAR)[:2])
    k, route, S, g = case_poses("period_with_offset")                           # the start delay holds again after every wrap
    assert (g[[0, 1, 2, 12, 13, 14, 24], 2] == 0).all() and (g[[3, 11, 15, 23], 2] == 3.1).all() and np.array_equal(g[12:24], g[:12])
    k, route, S, g = case_poses("period_after_leaving")                         # 1.4 m per tick on 10 m: gone from tick 8, back at 20
    assert g[7, 0] < 10.0 and g[7, 2] == 7.0 and g[8:20].tolist() == [PARKED] * 12 and np.array_equal(g[20:28], g[:8])
    # the end, both ways: s exactly S_end, one ulp below it, beyond it
    for e, gone in ((0, PARKED), (1, [10.0, 0.0, 0.0, 0.0, 0.0, 0.0])):
        k, route, S, g = case_poses(f"arrives_exactly_end{e}")
        assert TR.arc_at(10, 4.0, 0.0, 0.0, 0.25, 0)[2] == S[-1] == 10.0
        assert g[9].tolist() == [9.0, 0.0, 4.0, 0.0, 0.0, 0.0] and g[10].tolist() == gone and g[11].tolist() == gone and g[69].tolist() == gone
        k, route, S, g = case_poses(f"arrives_ulp_below_end{e}")
        assert TR.arc_at(9, 4.0, 0.0, k["s0"], 0.25, 0)[2] == np.nextafter(10.0, 0.0)
        assert g[9, 2] == 4.0 and abs(g[9, 0] - 10.0) < 1e-14 and g[9, 0] < 10.0 and g[10].tolist() == gone
        k, route, S, g = case_poses(f"stands_at_end{e}")
        last = [route[-1, 0], route[-1, 1], 0.0, route[-1, 2], 0.0, 0.0]
        assert (g == (gone if e == 0 else last)).all()
        k, route, S, g = case_poses(f"stands_ulp_below_end{e}")                 # still on the route: the last segment's pose and curvature
        assert (g[:, 2] == 0.0).all() and np.abs(g[0, [0, 1, 3]] - route[-1]).max() < 1e-12 and g[0, 5] != 0 and (g == g[0]).all()
        k, route, S, g = case_poses(f"s0_beyond_end{e}")
        assert (g == (PARKED if e == 0 else [route[-1, 0], route[-1, 1], 0.0, route[-1, 2], 0.0, 0.0])).all()
        k, route, S, g = case_poses(f"one_point_end{e}")                        # a route of one point: "stop" at it, whatever `end`
        assert (g == [7.0, -3.0, 0.0, 0.5, 0.0, 0.0]).all()
    # a zero-length segment: crossed without a division by zero, stood on with the segment ahead's curvature
    k, route, S, g = case_poses("zero_length_segment_crossed")
    assert S[30] == S[31] and np.isfinite(g).all() and (np.diff(g[:27, 0]) != 0).all() and g[69].tolist() == PARKED
    k, route, S, g = case_poses("zero_length_segment_stood_on")
    assert np.array_equal(g[0, [0, 1, 3]], route[31]) and g[0, 5] == np.arctan(L_CAR * (route[32, 2] - route[31, 2]) / (S[32] - S[31]))
    # s0 > 0: the vehicle starts there and needs that much less to the end
    k, route, S, g = case_poses("s0_positive")
    j = int(np.searchsorted(S, 3.3, side="right")) - 1
    f = (3.3 - S[j]) / (S[j + 1] - S[j])
    assert np.array_equal(g[0, :2], route[j, :2] + f * (route[j + 1, :2] - route[j, :2])) and g[0, 2] == 4.2
    first_gone = int(np.argmax(g[:, 2] == 0))
    assert first_gone == int(np.ceil((S[-1] - 3.3) / (4.2 * 0.2))) and np.array_equal(g[first_gone, [0, 1, 3]], route[-1])
    # a cyclist's wheelbase changes the steering angle and nothing else
    car, bike = case_poses("three_points")[3], case_poses("three_points", L=1.0)[3]
    assert np.array_equal(car[:, :5], bike[:, :5]) and (car[:, 5] != bike[:, 5]).any()


def test_every_edge_case_agrees_with_stepping():
    for name, k in TR.edge_cases().items():
        if "ulp" in name or "exactly" in name:
            continue                                                             # (a carried sum has its own last bit)
        route = TR.case_routes()[k["route"]]
        got = case_poses(name)[3]
        want = TR.stepped(route, 70, k["end"], k["speed"], k["offset"], k["s0"], k["dt"], k["period"], L_CAR)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9, err_msg=name)


def test_entry_point_is_declared_bound_and_documented(pkg):
    decl = pkg._header.header().functions["jsim_loop_set_traffic_routes"]
    assert [n for _, n in decl.params] == ["ctx", "n_routes", "x", "y", "yaw", "off"]
    assert pkg._header.constant("JSIM_ROUTE_PARK") == TR.PARK == pkg.closed_loop.ROUTE_PARK and pkg._header.constant("JSIM_ABI_VERSION") == 2
    assert hasattr(ctypes.CDLL(pkg.build.build()), "jsim_loop_set_traffic_routes")
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_set_traffic_routes.argtypes) == 6
    assert lib.jsim_loop_set_traffic_routes(None, 0, None, None, None, None) == -22     # null ctx: refused before anything else
    assert b"null ctx" in lib.jsim_last_error(None)
    assert "jsim_loop_set_traffic_routes" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert pkg.ScriptedObstacles.KINDS["route"] == 3.0
    inc = open(os.path.join(REPO, pkg.__name__, "csrc", "loop_pre_tick.inc")).read()
    assert "route_pt" in inc[inc.index("struct ObsStepP"):].split("};")[0].split("shape;")[1]      # the table: trailing members


def test_python_refusals_need_no_device(pkg):
    CL = pkg.closed_loop
    ok = dict(kind="route", route=np.array([[0.0, 0.0], [5.0, 0.0], [5.0, 5.0]]), speed=3.0)
    routes, rows = CL.route_table([ok, dict(direction=1, speed=3.0), dict(ok, route=ok["route"].copy(), end="stop", s0=1.0, period=2.4)], 0.2)
    assert len(routes) == 1 and rows[1] is None and rows[0] == [0.0, 0.0, 3.0, 0.0, 0.0, 0.2, 3.0, 0.0]
    assert rows[2] == [0.0, 1.0, 3.0, 0.0, 1.0, 0.2, 3.0, 12.0]
    # two columns: the yaw of the segment ahead, the last point the last segment's
    assert np.array_equal(routes[0][:, 2], [0.0, np.pi / 2, np.pi / 2]) and np.array_equal(routes[0][:, :2], ok["route"])
    wrapped = CL.route_array(np.array([[0.0, 0.0, 3.1], [1.0, 0.0, -3.1], [2.0, 0.0, -3.0]]))       # made continuous, the input left alone
    assert np.allclose(wrapped[:, 2], [3.1, 2 * np.pi - 3.1, 2 * np.pi - 3.0])
    for bad, msg in ((dict(ok, end="park"), "end must be"), (dict(ok, route=np.array([[0.0, 0.0], [np.nan, 1.0]])), "not finite"),
                     (dict(ok, route=np.array([[0.0, 0.0, 0.0], [1.0, 1.0, np.inf]])), "not finite"), (dict(ok, s0=-0.1), "s0="),
                     (dict(ok, speed=-1.0), "speed="), (dict(ok, period=0.3), "period="), (dict(ok, period=0.0), "period="),
                     (dict(ok, period=-0.2), "period="), (dict(ok, route=np.zeros((0, 3))), "a route is"), (dict(ok, route=np.zeros(4)), "a route is")):
        with pytest.raises(ValueError, match=msg):
            CL.route_table([bad], 0.2)
        # a loop and the vehicle table refuse before they touch their engine: there is none here
        with pytest.raises(ValueError, match=msg):
            pkg.ScenarioLoop(NO_ENGINE, None, [bad])
        with pytest.raises(ValueError, match=msg):
            pkg.ScriptedObstacles(None, [bad], dt=0.2)
    with pytest.raises(ValueError, match="unknown obstacle kind"):
        pkg.ScenarioLoop(NO_ENGINE, None, [dict(kind="rout", route=ok["route"], speed=1.0)])
    # a stream of arrivals: n specs per route, headway_s apart, further keys passed on
    specs = pkg.traffic_on_routes([ok["route"], ok["route"] + 1.0], 4.0, 2.5, 3, end="stop", period=30.0)
    assert len(specs) == 6 and [s["offset"] for s in specs] == [None, 2.5, 5.0] * 2 and all(s["kind"] == "route" and s["end"] == "stop" for s in specs)
    assert specs[0]["route"] is specs[2]["route"] and specs[3]["route"] is not specs[0]["route"]
    routes, rows = CL.route_table(specs, 0.1)
    assert len(routes) == 2 and [r[0] for r in rows] == [0.0] * 3 + [1.0] * 3 and all(r[7] == 300.0 for r in rows)
