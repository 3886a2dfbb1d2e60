"""Route tables at their limits on the device (the tables and vehicles of tests/traffic_route_limit_cases.py,
whose premises tests/test_traffic_route_limits_cpu.py holds): 64, 65, 129 and 130 routes -- the second and the third block of
route_arclen_kernel, its guard, a vehicle on a route of a later block --, empty routes at the table's end and everywhere, a route of
2049 points driven at 37 segments a tick, and a table replaced by a larger and by a smaller one.  Doubles against the numpy
restatement (tests/traffic_route_numpy.py) to 1e-9, the three ways to run a loop against each other bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import traffic_route_cases as RC
import traffic_route_limit_cases as LC
import traffic_route_numpy as TR
from gpu_helpers import W, iroutes, loop_engine  # noqa: F401
from test_gpu_traffic_route import ATOL, bare_engine, device_ticks

pytestmark = pytest.mark.gpu

T = 13


@pytest.fixture(scope="module")
def tables():
    return LC.tables()


def register(eng, routes):
    """jsim_loop_set_traffic_routes through the C-ABI (route_array refuses a route without a point on purpose): the return code."""
    arrays = LC.pack(routes)
    return eng.lib.jsim_loop_set_traffic_routes(eng._ctx, len(routes), *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays))


def poses(eng, param, n_ticks=LC.K):
    """(get_all [n_ticks][n][6], gets of the get-only calls, the final state [n][4]) of the param rows, eight vehicles a call."""
    got, first, state = [], [], []
    for lo in range(0, len(param), 8):
        st = torch.full((len(param[lo:lo + 8]), 4), 123.0, dtype=torch.float64, device=eng.device)   # the pose slots are outputs ..
        st[:, 3] = 0.0                                                                               # .. only the counter is read
        g, f = device_ticks(eng, st, torch.from_numpy(np.ascontiguousarray(param[lo:lo + 8])).to(eng.device), n_ticks)
        got.append(g)
        first.append(f)
        state.append(st.cpu().numpy())
    return np.concatenate(got, axis=1), np.concatenate(first, axis=1), np.concatenate(state, axis=0)


def check_table(eng, routes, vehicles, name):
    """Every vehicle's 45 ticks through jsim_loop_obstacles against TR.run: the worst difference."""
    want, end, param = LC.restated(routes, vehicles, eng.L)
    got, first, state = poses(eng, param)
    assert np.array_equal(got, first), name                                  # get() alone moves nothing
    err = np.abs(got - want).max(axis=(0, 2))
    assert err.max() <= ATOL, (name, int(err.argmax()), vehicles[int(err.argmax())], err.max())
    assert np.array_equal(state[:, 3], np.full(len(vehicles), float(LC.K))) and np.abs(state - end).max() <= ATOL, name
    return float(err.max())


# ---- 1. jsim_loop_obstacles: every pose by bisection ----
def test_every_table_through_the_obstacle_call(pkg, routes, tables):
    """Every table of the case module, one vehicle per route (and five on the 2049-point route), 45 ticks of get() and get() +
    step() on one engine, the tables registered one after another.  After the table without a point a vehicle stands at the
    origin: it is not stepped as a kind-0 car, which is what a kind-3 row does without a table."""
    eng = bare_engine(pkg, routes)
    worst = {}
    for name, (table, vehicles) in tables.items():
        assert register(eng, table) == 0, eng.lib.jsim_last_error(eng._ctx)
        worst[name] = check_table(eng, table, vehicles, name)
        if name == "all_empty":
            got, _, state = poses(eng, TR.case_rows(vehicles[:8]), 12)
            assert not got.any() and not state[:, :3].any() and (state[:, 3] == 12).all()
    print("max |device - restatement| per table: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    # the vehicles at the blocks' edges are where the restatement has them, a metre and more from one another
    want, _, param = LC.restated(*tables["long"], eng.L)
    assert register(eng, tables["long"][0]) == 0
    got, _, _ = poses(eng, param[list(LC.FAR)])
    assert np.abs(got - want[:, list(LC.FAR)]).max() <= ATOL
    assert register(eng, []) == 0                                               # (n_routes = 0 clears the table)


# ---- 2. the rollout kernel: every pose by the hinted walk ----
def limits_loop(pkg, iroutes, W, **kw):
    sets, _ = LC.loop_specs()
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, LC.N_SETS, T, rank=3), T)
    return pkg.ScenarioLoop(eng, x0, sets, max_age=RC.MAX_AGE, frame_window=20, traffic_of=np.arange(LC.N_SETS), record=LC.K, **kw)


def test_the_rollout_walks_every_route(pkg, W, iroutes):
    """17 egos with a traffic set of 8 route vehicles each, 136 vehicles on 136 distinct routes (three blocks of both kernels),
    the five vehicles of the 2049-point route among them: run(45), fused chunks of 7 ticks (the fast vehicle's 9-tick period wraps
    in the ticks 8, 17, 26, 35 and 44: at five phases of a chunk, its first tick among them, and two chunks hold no wrap), chunks
    of 10 ticks (a wrap inside every chunk) and 45 x tick() leave the same recorded tuples, states and last get() bit for bit, and those are the restatement's."""
    loops = {"run": limits_loop(pkg, iroutes, W), "chunks of 7": limits_loop(pkg, iroutes, W, chunk_ticks=7),
             "chunks of 10": limits_loop(pkg, iroutes, W, chunk_ticks=10), "ticks": limits_loop(pkg, iroutes, W)}
    for name in ("run", "chunks of 7", "chunks of 10"):
        loops[name].run(LC.K)
    for _ in range(LC.K):
        loops["ticks"].tick()
    torch.cuda.synchronize()
    a = loops["run"]
    assert a.obst.n == 136 and len(a.obst.routes) == len(a.loop.eng.traffic_routes) == 136
    assert sum(len(r) == LC.LONG_N for r in a.obst.routes) == 5
    for name in ("chunks of 7", "chunks of 10", "ticks"):
        b = loops[name]
        assert torch.equal(a.recorder.obs[:LC.K], b.recorder.obs[:LC.K]), name
        assert torch.equal(a.obst.state, b.obst.state) and torch.equal(a.obst.get_buf, b.obst.get_buf), name
    want, end = RC.restated(TR, a, LC.K)
    got = a.recorder.obs[:LC.K].cpu().numpy()
    err = np.abs(got - want).max(axis=(0, 2))
    print(f"136 vehicles x {LC.K} ticks: max |rollout - restatement| = {err.max():.3e} (vehicle {int(err.argmax())}); "
          f"on the 2049-point routes {err[-5:].max():.3e}")
    assert not np.isnan(want).any() and err.max() <= ATOL
    st = a.obst.state.cpu().numpy()
    assert (st[:, 3] == LC.K).all() and np.abs(st - end).max() <= ATOL
    assert np.abs(a.obst.get_buf.cpu().numpy() - want[-1]).max() <= ATOL
    # the routes as registered are the case module's (smooth_yaw changes no continuous yaw), so the premises of the CPU test hold here
    sets, flat = LC.loop_specs()
    assert all(np.array_equal(r, sp["route"]) for r, sp in zip(a.obst.routes, [sp for st in sets for sp in st]))
    assert np.array_equal(a.obst.param.cpu().numpy()[:, [1, 2, 3, 4, 7]],
                          np.array([[k["end"], k["speed"], k["offset"], k["s0"], k["period"]] for k in flat]))
    fast = got[:, 131]
    assert np.hypot(*(fast[9, :2] - fast[8, :2])) > 20.0 and (got[..., 0] == TR.PARK).any() and (np.abs(got[..., 3]) > np.pi).any()


# ---- 3. a table replaced by a larger and by a smaller one ----
def test_a_table_is_replaced_by_a_larger_and_a_smaller_one(pkg, routes, tables):
    CL = pkg.closed_loop
    eng = bare_engine(pkg, routes)
    lib, ctx = eng.lib, eng._ctx
    six = TR.case_routes()
    edge = TR.edge_cases()
    small = [edge[k] for k in ("s0_positive", "period_wraps", "zero_length_segment_crossed", "three_points")]
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                           # noqa: E731

    def held(table, vehicles, what):
        want, _, param = LC.restated(table, vehicles, eng.L)
        got, _, _ = poses(eng, param)
        assert np.abs(got - want).max() <= ATOL, what
        assert eng.traffic_routes is not None and len(eng.traffic_routes) == len(table) and all(
            np.array_equal(a, b) for a, b in zip(eng.traffic_routes, table)), what

    def refused(table, vehicles, what):
        x, y, yaw, off = LC.pack(table)
        bad, down = x.copy(), off.copy()
        bad[len(x) // 2], down[len(off) // 2] = np.nan, -1
        assert lib.jsim_loop_set_traffic_routes(ctx, len(table), dp(bad), dp(y), dp(yaw), dp(off)) == -22, what
        assert lib.jsim_loop_set_traffic_routes(ctx, len(table), dp(x), dp(y), dp(yaw), dp(down)) == -22, what
        held(table, vehicles, what + ", after refusals")

    CL._register_routes(eng, six)
    held(six, small, "6 routes")
    assert lib.jsim_loop_set_traffic_routes(ctx, 129, *(dp(a) for a in LC.pack(tables["r129"][0]))) == 0
    CL._register_routes(eng, tables["r129"][0])                                 # (the Python layer's call: the engine's list follows)
    held(*tables["r129"], "129 routes after 6")
    refused(*tables["r129"], "129 routes")
    assert lib.jsim_loop_set_traffic_routes(ctx, 65, *(dp(a) for a in LC.pack(tables["r65"][0]))) == 0
    CL._register_routes(eng, tables["r65"][0])
    held(*tables["r65"], "65 routes after 129")
    refused(*tables["r65"], "65 routes")
    # the smaller table's vehicles read nothing of the larger one that the allocation may still hold: route 64 is the last, and an
    # index beyond it is clamped onto it
    row = TR.case_rows([dict(LC.vehicle(64), route=64), dict(LC.vehicle(64), route=128)])
    got, _, _ = poses(eng, row)
    assert np.array_equal(got[:, 0], got[:, 1])
    CL._register_routes(eng, [])
    assert eng.traffic_routes is None
