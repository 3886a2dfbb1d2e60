"""The premises of tests/test_gpu_traffic_route_limits.py, without a GPU: what the tables of tests/traffic_route_limit_cases.py hold
and what the restatement (tests/traffic_route_numpy.py) makes of them, so that the device test cannot pass on nothing."""
import numpy as np
import pytest

import traffic_route_limit_cases as LC
import traffic_route_numpy as TR

L_CAR = 2.86


@pytest.fixture(scope="module")
def tables():
    return LC.tables()


@pytest.fixture(scope="module")
def runs(tables):
    return {name: LC.restated(routes, vehicles, L_CAR) for name, (routes, vehicles) in tables.items()}


def test_the_tables_are_what_the_device_test_needs(tables):
    assert {name: len(r) for name, (r, _) in tables.items()} == dict(r64=64, r65=65, r129=129, last_empty=65, all_empty=65, long=130)
    routes = tables["r129"][0]
    assert [len(routes[r]) for r in LC.FAR] == [64, 64, 65, 300]
    assert {len(r) for r in routes} == set(LC.LENGTHS) and [len(r) for r in routes[:7]] == [64, 65, 300, 0, 1, 2, 5]
    assert len(tables["last_empty"][0][-1]) == 0 and len(tables["last_empty"][0][-2]) == 64
    assert all(len(r) == 0 for r in tables["all_empty"][0]) and LC.pack(tables["all_empty"][0])[3].tolist() == [0] * 66
    x, y, yaw, off = LC.pack(tables["last_empty"][0])
    assert off[-1] == off[-2] == len(x) and off.dtype == np.int32                 # the last route starts one past the points
    long = tables["long"][0][-1]
    assert long.shape == (LC.LONG_N, 3) and int(np.ceil(np.log2(LC.LONG_N - 1))) == 11
    assert np.abs(np.diff(TR.arc_length(long)) - LC.LONG_SPACING).max() < 1e-4
    # route r lies r metres to the left of and r metres above route 0: their first points do
    first = {r: routes[r][0, :2] for r in range(129) if len(routes[r])}
    assert all(np.array_equal(p, [-r, r]) for r, p in first.items())
    # a yaw beyond [-pi, pi] in the tables
    assert max(np.abs(r[:, 2]).max() for r in routes if len(r)) > np.pi and long[-1, 2] > np.pi
    # every route's yaw is continuous as route_array would leave it (steps below pi / 2)
    assert max(np.abs(np.diff(r[:, 2])).max() for r in routes + [long] if len(r) > 1) < 0.5


def test_vehicles_of_empty_routes_stand_at_the_origin(tables, runs):
    n_seen = 0
    for name, (routes, vehicles) in tables.items():
        get, state, _ = runs[name]
        for i, k in enumerate(vehicles):
            if len(routes[k["route"]]) == 0:
                assert not get[:, i].any() and not state[i, :3].any() and state[i, 3] == LC.K, (name, i)
                n_seen += 1
    assert n_seen >= 65 + 1 + 4 * 9
    assert not runs["all_empty"][0].any()


def test_vehicles_at_the_blocks_edges_are_far_apart(tables, runs):
    get = runs["long"][0]
    assert [tables["long"][1][r]["route"] for r in LC.FAR] == list(LC.FAR)
    for i, a in enumerate(LC.FAR):
        for b in LC.FAR[i + 1:]:
            d = np.hypot(get[:, a, 0] - get[:, b, 0], get[:, a, 1] - get[:, b, 1])
            assert d.min() > 1.0, (a, b, d.min())
    assert (np.abs(get[:, list(LC.FAR), 0]) < 1000).all() and (get[-1, list(LC.FAR), 2] > 0).all()    # none parked, all moving


def test_the_fast_vehicle_strides_and_wraps(tables, runs):
    routes, vehicles = tables["long"]
    S = TR.arc_length(routes[-1])
    names = list(LC.long_vehicles(129, S[-1]))
    fast, slow, still = (vehicles[129 + names.index(n)] for n in ("fast", "slow", "still"))
    seg = [TR.segment(S, TR.arc_at(c, fast["speed"], fast["offset"], fast["s0"], LC.DT, fast["period"])[2])[0] for c in range(LC.K + 1)]
    step = np.diff(seg)
    assert (step[step > 0] > 30).all() and (step > 0).sum() == 40 and (step < 0).sum() == 5        # 8 strides, then a wrap: five times
    assert [c for c in range(1, LC.K + 1) if c % fast["period"] == 0] == [9, 18, 27, 36, 45]
    assert 0 < slow["speed"] * LC.DT < LC.LONG_SPACING
    g = runs["long"][0][:, 129 + names.index("still")]
    assert (g[:, 2] == 0).all() and (g[:, 5] != 0).all() and (g == g[0]).all()
    for n, parked in (("last_stop", False), ("last_leave", True)):
        k, g = vehicles[129 + names.index(n)], runs["long"][0][:, 129 + names.index(n)]
        assert TR.segment(S, k["s0"])[0] == LC.LONG_N - 2 and g[0, 2] > 0 and g[-1, 2] == 0
        assert (g[-1, 0] == TR.PARK) == parked and (parked or np.array_equal(g[-1, [0, 1, 3]], routes[-1][-1]))


def test_the_walk_agrees_with_the_closed_form(tables):
    worst = 0.0
    for name, (routes, vehicles) in tables.items():
        for k in vehicles:
            p = routes[k["route"]]
            rest = (k["end"], k["speed"], k["offset"], k["s0"], k["dt"], k["period"], L_CAR)
            S = TR.arc_length(p)
            closed = np.array([TR.pose(p, S, c, *rest) for c in range(LC.K)])
            walked = TR.stepped(p, LC.K, *rest)
            worst = max(worst, float(np.abs(closed - walked).max()))
            np.testing.assert_allclose(walked, closed, rtol=0, atol=1e-9, err_msg=f"{name} {k}")
    print(f"max |walk - closed form| = {worst:.3e}")


def test_every_branch_of_items_5_to_7_occurs(tables, runs):
    for name in ("r64", "r65", "r129", "last_empty", "long"):
        routes, vehicles = tables[name]
        seen = {LC.branch(routes, k, c) for k in vehicles for c in range(LC.K)}
        assert seen == {"moving", "waiting", "stop", "leave", "one_point", "empty"}, (name, seen)
    routes, vehicles = tables["all_empty"]
    assert {LC.branch(routes, k, c) for k in vehicles for c in (0, 7)} == {"empty"}
    # the recorded tuples say the same: parked, standing at an end, waiting with a steering angle, a yaw beyond pi
    get = runs["long"][0]
    assert (get[..., 0] == TR.PARK).any() and ((get[..., 2] == 0) & (get[..., 5] != 0)).any()
    assert (np.abs(get[..., 3]) > np.pi).any()
    # a period wrap moves a vehicle back: some vehicle's arc length decreases between two ticks
    fast = get[:, 129]
    assert (np.hypot(*(fast[9, :2] - fast[8, :2])) > 20.0)


def test_the_loop_of_the_rollout_test(tables):
    sets, flat = LC.loop_specs()
    assert len(sets) == LC.N_SETS and all(len(s) == LC.PER_SET for s in sets) and len(flat) == 136
    arrays = [sp["route"] for st in sets for sp in st]
    assert len({(a.shape[0], a.tobytes()) for a in arrays}) == 136 and min(len(a) for a in arrays) == 1
    assert sum(len(a) == LC.LONG_N for a in arrays) == 5 and {len(a) for a in arrays} == set(LC.LENGTHS[1:]) | {LC.LONG_N}
