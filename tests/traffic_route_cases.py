"""The loops of tests/test_gpu_traffic_route.py, built in one place so that the child process of the .npz test
(tests/traffic_route_child.py) builds the very loop its parent saved: T = 13 with 8 egos over two traffic sets, one of which holds
route vehicles -- on the egos' own planned routes, so they cross the junction the egos cross -- beside a T-intersection car."""
import importlib

import numpy as np

T, B, N, EVERY = 13, 8, 60, 20
MAX_AGE = 30
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
TRAFFIC_OF = np.array([0, 1, 0, 1, 0, 0, 1, 0])
GOAL, AGE = 2, 4


def routes_of(pkg):
    return pkg.workloads.route_table(False)[0]


def sets(routes):
    """Set 0: a T-intersection car, a route vehicle that enters again every 8 s, one that leaves a short route within the run, and a
    cyclist that starts 5 m along its route and stops at its end.  Set 1: vehicles of the other kinds only."""
    return [[dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0),
             dict(kind="route", route=routes[4], speed=6.0, offset=1.0, period=8.0),
             dict(kind="route", route=routes[9][:150, :2], speed=7.0),
             dict(kind="route", route=routes[7], speed=4.0, s0=5.0, end="stop", dims=CYCLIST)],
            [dict(direction=-1, turning=False, speed=25 / 3.6, offset=None),
             dict(kind="arterial", x_init=1.5, y_init=-30.0, speed=25 / 3.6, initial_speed=5 / 3.6, offset=3.0)]]


def scenario_loop(pkg, routes, T=T, record=N, **kw):
    """The base ScenarioLoop; kw: checkpoint_every, ..."""
    Wl = pkg.workloads
    eng, x0 = Wl.make_engine(routes, Wl.ego_batch(routes, B, T, rank=3), T, "cuda:0")
    return pkg.ScenarioLoop(eng, x0, sets(routes), max_age=MAX_AGE, frame_window=20, traffic_of=TRAFFIC_OF, record=record, **kw)


def restated(TR, loop, n_ticks, state0=None):
    """tests/traffic_route_numpy.run on a loop's own tables: (get_all [n_ticks][n][6] with NaN rows for the other kinds, state)."""
    obst = loop.obst
    L = np.full(obst.n, float(loop.loop.eng.L)) if loop.shapes is None else loop.shapes[:, 3]
    state0 = obst._state0.cpu().numpy() if state0 is None else state0
    return TR.run(obst.routes, state0, obst.param.cpu().numpy(), L, n_ticks)


def package():
    import conftest
    return importlib.import_module(conftest.PKG_NAME)
