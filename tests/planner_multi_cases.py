"""Shared by the tests of the per-route planner weights: the stored scenarios of tests/golden/planner_multi.npz as route queries
and as the scenario / car / primitive OBJECTS the reference's constructors take, and a direct call of either C-ABI entry point."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np

from conftest import load_golden

_G = None


def golden():
    global _G
    if _G is None:
        g = load_golden("planner_multi.npz")
        _G = {k: g[k] for k in g.files}          # read once, shared; nobody writes to it
        for v in _G.values():
            v.setflags(write=False)
    return _G


def stored_query(PL, g, i):
    off = g[f"s{i}_hp_off"]
    return PL.RouteQuery(start=tuple(float(v) for v in g[f"s{i}_start"]), goal=tuple(float(v) for v in g[f"s{i}_goal"]),
                         goal_box=tuple(float(v) for v in g[f"s{i}_goal_box"]), tol=float(g[f"s{i}_tol"]),
                         obstacles=[g[f"s{i}_hp"][off[k]:off[k + 1]] for k in range(len(off) - 1)])


def combos(g, i):
    return [tuple(float(v) for v in g[f"s{i}_c{j}_wh"]) for j in range(int(g[f"s{i}_n_comb"]))]


def objects(PL, q, g):
    """(scenario, car_dimensions, mps) stand-ins with exactly the attributes the reference's constructors read; the stored
    half-planes already hold the margin."""
    mps = {n: NS(points=np.array(g["mp_points"][k]), total_length=float(g["mp_length"][k]), name=n) for k, n in enumerate(PL.MP_NAMES)}
    car = NS(radius=float(g["radius"]), circle_centers=np.array(g["circle_centers"]))
    scen = NS(start=q.start, goal_point=q.goal, goal_area=NS(xy1=q.goal_box[:2], xy2=q.goal_box[2:]),
              allowed_goal_theta_difference=q.tol, obstacles=[NS(to_convex=(lambda margin, o=o: o)) for o in q.obstacles])
    return scen, car, mps


def assert_same_route(a, b):
    """bit for bit"""
    assert a.status == b.status and a.n_expanded == b.n_expanded and a.cost == b.cost
    assert np.array_equal(a.prims, b.prims) and np.array_equal(a.nodes, b.nodes) and np.array_equal(a.trajectory, b.trajectory)


def call_entry(pkg, name, queries, wh, wc, form=None, max_path=32, node_cap=1 << 15, null=()):
    """Call jsim_plan_routes (wh (5,), wc (4,), form None) or jsim_plan_routes_weighted (tables) directly -> (rc, outputs);
    `null` names arguments passed as NULL."""
    PL = pkg.planner
    lib = pkg._cabi.load()
    pts, length = PL.make_motion_primitives()
    rad, cen = PL.car_circles()
    cc = [PL.collision_points(p, cen, rad) for p in pts]
    a = dict(cc=np.ascontiguousarray(np.concatenate(cc, axis=0)), cc_off=np.concatenate([[0], np.cumsum([len(c) for c in cc])]).astype(np.int32))
    hp_off, r_off, hps = [0], [0], []
    for q in queries:
        for o in q.obstacles:
            hps.append(np.asarray(o, dtype=np.float64).reshape(-1, 3)); hp_off.append(hp_off[-1] + len(hps[-1]))
        r_off.append(len(hp_off) - 1)
    R = len(queries)
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    a.update(hp=f64(np.concatenate(hps, axis=0)), hp_off=np.array(hp_off, np.int32), r_off=np.array(r_off, np.int32),
             start=f64([q.start for q in queries]), goal=f64([q.goal for q in queries]), box=f64([q.goal_box for q in queries]),
             tol=f64([q.tol for q in queries]), mp=f64(pts), ml=f64(length), wh=f64(wh), wc=f64(wc),
             form=None if form is None else np.ascontiguousarray(form, dtype=np.int32))
    out = dict(status=np.full(R, -7, np.int32), cost=np.zeros(R), n_prims=np.zeros(R, np.int32), prims=np.zeros((R, max_path), np.int32),
               nodes=np.zeros((R, max_path + 1, 3)), traj=np.zeros((R, max_path * 60, 3)), n_exp=np.zeros(R, np.int32))
    p = lambda k: None if (k in null or a.get(k, out.get(k)) is None) else C.c_void_p(a[k].ctypes.data if k in a else out[k].ctypes.data)
    args = [0, R, p("start"), p("goal"), p("box"), p("tol"), p("hp"), p("hp_off"), len(hp_off) - 1, p("r_off"), p("mp"), p("ml"), 9, 61,
            p("cc"), p("cc_off"), p("wh"), p("wc")]
    if name == "jsim_plan_routes_weighted":
        args.append(p("form"))
    args += [max_path, node_cap] + [p(k) for k in ("status", "cost", "n_prims", "prims", "nodes", "traj", "n_exp")]
    return getattr(lib, name)(*args), out
