"""Shared by tests/test_planner_shapes_cpu.py and tests/test_gpu_planner_shapes.py: tests/golden/planner_shapes.npz (the oracle's
outcomes, written by tests/golden/make_golden_planner_shapes.py) as collision probes and searches, and the route-level cases at
the kernel's table limits."""
from types import SimpleNamespace as NS

import numpy as np

from conftest import load_golden

FAMILIES = ("poly", "unb", "red", "pos")
CONFIGS = ("p1", "p3", "p3n31", "p9n31", "p16c1", "p16c2", "p16c4")
_G = None


def golden():
    global _G
    if _G is None:
        g = load_golden("planner_shapes.npz")
        _G = {k: g[k] for k in g.files}          # read once, shared; nobody writes to it
        for v in _G.values():
            v.setflags(write=False)
    return _G


def probes(fam):
    """(obstacles, routes) of a probe family: routes are namespaces with start, goal, goal_box, tol, obstacles (arrays), ids,
    target (the obstacle under test, before it was moved or padded), row, inside, variant, status, n_expanded."""
    g, p = golden(), f"p_{fam}_"
    off, ioff = g[p + "hp_off"], g[p + "ids_off"]
    obst = [g[p + "hp"][off[k]:off[k + 1]] for k in range(len(off) - 1)]
    routes = []
    for i in range(len(g[p + "status"])):
        ids = [int(k) for k in g[p + "ids"][ioff[i]:ioff[i + 1]]]
        target, row, inside, variant = (int(v) for v in g[p + "meta"][i])
        routes.append(NS(start=tuple(float(v) for v in g[p + "start"][i]), goal=tuple(float(v) for v in g[p + "goal"][i]),
                         goal_box=tuple(float(v) for v in g[p + "goal_box"][i]), tol=float(g[p + "tol"][i]), ids=ids,
                         obstacles=[obst[k] for k in ids], target=target, row=row, inside=inside, variant=variant,
                         status=int(g[p + "status"][i]), n_expanded=int(g[p + "n_expanded"][i])))
    return obst, routes


def config(name):
    """A search configuration: points [P, n, 3], length [P], radius, centres [k, 2] and its routes (namespaces with the query and
    the oracle's status, cost, path, prims, n_expanded, key_obstacle)."""
    g, c = golden(), f"c_{name}_"
    mpset = str(g[c + "mpset"])
    routes = []
    for j in range(int(g[c + "n"])):
        r = f"{c}r{j}_"
        off = g[r + "hp_off"]
        routes.append(NS(start=tuple(float(v) for v in g[r + "start"]), goal=tuple(float(v) for v in g[r + "goal"]),
                         goal_box=tuple(float(v) for v in g[r + "goal_box"]), tol=float(g[r + "tol"]),
                         obstacles=[g[r + "hp"][off[k]:off[k + 1]] for k in range(len(off) - 1)], status=int(g[r + "status"]),
                         cost=float(g[r + "cost"]), path=g[r + "path"], prims=[int(k) for k in g[r + "prims"]],
                         n_expanded=int(g[r + "n_expanded"]), key_obstacle=int(g[r + "key_obstacle"]), seed=int(g[r + "seed"])))
    return NS(name=name, points=g[f"mp_{mpset}_points"], length=g[f"mp_{mpset}_length"], radius=float(g[c + "radius"]), centres=g[c + "centres"],
              routes=routes)


def oracle_mps(points, length):
    return [(f"p{k}", np.array(points[k]), float(length[k])) for k in range(len(points))]


def straight(PO):
    """The probes' one-primitive set."""
    return PO.make_motion_primitives()[:1]


def query(PL, r, obstacles=None):
    return PL.RouteQuery(start=r.start, goal=r.goal, goal_box=r.goal_box, tol=r.tol, obstacles=r.obstacles if obstacles is None else obstacles)


def solve(PO, r, mps, centres, radius, obstacles=None, max_expansions=200000):
    """The oracle on a route -> (status, cost, path, prims, n_expanded, oracle)."""
    orc = PO.PlannerOracle(r.start, r.goal, r.goal_box, r.tol, r.obstacles if obstacles is None else obstacles, mps, centres, radius)
    try:
        cost, path, _ = orc.run(max_expansions=max_expansions)
        return 0, cost, np.array(path), orc.prim_sequence(path), orc.n_expanded
    except RuntimeError:
        raise
    except Exception as e:
        assert str(e) == "No solution found."
        return 1, float("nan"), np.zeros((0, 3)), [], orc.n_expanded


def trajectory(PO, path, prims, points):
    """path_to_full_trajectory from a stored path: segment s = primitive prims[s] placed at node s, all points but the last."""
    segs = [PO.transform_pts(a[2], PO.transform_mtx(*a), np.array(points[k]))[:-1] for a, k in zip(path[:-1], prims)]
    return np.concatenate(segs, axis=0) if segs else np.zeros((0, 3))


def pair_count(PL, cfg):
    """((primitive, collision point) pairs, the largest count of one primitive) as the product lays them out."""
    n = [len(PL.collision_points(p, cfg.centres, cfg.radius)) for p in cfg.points]
    return sum(n), max(n)


# ------------------------------------------------------------------------------------------------ route-level cases
def open_space(r):
    """The route's start without any obstacle, the goal two primitives down the stored route (a box of 2 m around that node):
    near enough for the oracle to solve on the spot with any primitive set."""
    gx, gy, gth = (float(v) for v in r.path[min(2, len(r.path) - 1)])
    return NS(start=r.start, goal=(gx, gy, gth), goal_box=(gx - 1.0, gy - 1.0, gx + 1.0, gy + 1.0), tol=r.tol, obstacles=[])


def _far_box(k):
    x = 500.0 + 3.0 * k
    return np.array([[1.3, 0.0, -1.3 * (x + 1.0)], [-0.7, 0.0, 0.7 * (x - 1.0)], [0.0, 2.0, -2.0 * 901.0], [0.0, -1.0, 899.0]])


def too_many_obstacles(r):
    """65 obstacles: the route's own and boxes far away (JPL_MAX_OBS = 64)."""
    obst = list(r.obstacles)
    assert len(obst) < 65
    return NS(start=r.start, goal=r.goal, goal_box=r.goal_box, tol=r.tol, obstacles=obst + [_far_box(k) for k in range(65 - len(obst))])


def too_many_rows(r):
    """513 half-planes in 9 obstacles far away: eight boxes with every row sixteen times, and one row more (JPL_MAX_HP = 512)."""
    obst = [np.tile(_far_box(k), (16, 1)) for k in range(8)] + [_far_box(9)[:1]]
    assert sum(len(o) for o in obst) == 513
    return NS(start=r.start, goal=r.goal, goal_box=r.goal_box, tol=r.tol, obstacles=obst)


def start_in_goal(r):
    """A start that already passes the goal test (the middle of the goal box, the goal's heading), the route's obstacles kept."""
    b = r.goal_box
    s = (0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3]), r.goal[2])
    return NS(start=s, goal=r.goal, goal_box=r.goal_box, tol=r.tol, obstacles=r.obstacles)


def assert_route(PO, res, r, points, what):
    """A planned route against the oracle's (the bars of tests/test_planner.py): the same primitive at every step, cost within
    1e-9 max(1, |cost|), nodes and trajectory within 1e-9, expansions within max(1, n // 50).  Every figure is printed first."""
    ne = r.n_expanded
    dc = abs(res.cost - r.cost) if r.status == 0 and res.status == 0 else float("nan")
    print(f"{what}: status {res.status} (oracle {r.status}), expansions {res.n_expanded} (oracle {ne}), primitives {len(res.prims)} "
          f"(oracle {len(r.prims)}), |cost - oracle| {dc:.3e}")
    assert res.status == r.status, (what, res.status, r.status)
    assert abs(res.n_expanded - ne) <= max(1, ne // 50), (what, res.n_expanded, ne)
    if r.status != 0:
        assert len(res.prims) == 0 and len(res.trajectory) == 0, what
        return
    assert list(res.prims) == list(r.prims), (what, list(res.prims), list(r.prims), res.cost, r.cost)
    assert dc <= 1e-9 * max(1.0, abs(r.cost)), (what, res.cost, r.cost)
    np.testing.assert_allclose(res.nodes, r.path, rtol=0, atol=1e-9)
    traj = trajectory(PO, [tuple(p) for p in r.path], r.prims, points)
    assert res.trajectory.shape == traj.shape, what
    np.testing.assert_allclose(res.trajectory, traj, rtol=0, atol=1e-9)
