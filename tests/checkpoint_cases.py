"""The loops of tests/test_gpu_checkpoint.py, built in one place so that the child process of the .npz test (tests/checkpoint_child.py)
builds the very loop its parent saved: T = 13 with 6 egos -- small, but with respawns and vehicles -- over the four traffic sets of
tests/test_gpu_fork.py (T-intersection cars, a turning roundabout car, an arterial car with a start delay beside a cyclist with
dims, an empty set)."""
import importlib

import numpy as np

T, B, N, EVERY = 13, 6, 100, 25
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
SETS = [[dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(direction=-1, turning=True, speed=25 / 3.6, offset=None)],
        [dict(kind="roundabout", direction=1, turning=True, speed=20 / 3.6, offset=1.0)],
        [dict(kind="arterial", x_init=1.5, y_init=-30.0, speed=25 / 3.6, initial_speed=5 / 3.6, offset=3.0),
         dict(kind="arterial", x_init=2.0, y_init=-12.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)],
        []]
TRAFFIC_OF = np.array([0, 1, 2, 3, 0, 2])
MAX_AGE = 30
GOAL, AGE = 2, 4


def routes_of(pkg):
    return pkg.workloads.route_table(False)[0]


def scenario_loop(pkg, routes, mode="truncate", T=T, B=B, record=N, traffic=True, **kw):
    """The base ScenarioLoop; kw: checkpoint_every, checkpoint_slots, ..."""
    Wl = pkg.workloads
    eng, x0 = Wl.make_engine(routes, Wl.ego_batch(routes, B, T, rank=3), T, "cuda:0", mode=mode)
    if traffic:
        return pkg.ScenarioLoop(eng, x0, SETS, max_age=MAX_AGE, frame_window=20, mode=mode, traffic_of=TRAFFIC_OF[:B], record=record, **kw)
    return pkg.ScenarioLoop(eng, x0, SETS[0] + SETS[2], max_age=MAX_AGE, frame_window=20, mode=mode, record=record, **kw)


def package():
    import conftest
    return importlib.import_module(conftest.PKG_NAME)
