"""Per-vehicle shapes (jsim_loop_set_vehicle_shapes) without a GPU: the numpy restatement with one shape per obstacle
(tests/shapes_numpy.py) pinned before any GPU test relies on it -- with every obstacle of one shape it IS the oracle's glue, on
the reference-made cases of loop_f1.npz (two cars) and loop_bicycle.npz (car and cyclist); on mixed cases its vectorised form
equals the plain nested loops.  The mixed case itself has no reference function behind it (the reference never mixes shapes).
Also: the Python layer's checks of `dims`, the export in header and binding, and that every PRE row of the variant table has a
uniform-table case in tests/test_gpu_vehicle_shapes.py."""
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

from conftest import PKG_NAME, REPO, load_golden

CFG = importlib.import_module(PKG_NAME + ".config")


@pytest.fixture(scope="module")
def SN(oracle):
    import shapes_numpy
    return shapes_numpy


@pytest.fixture(scope="module")
def LO(oracle):
    import loop_oracle
    return loop_oracle


def _case(LO, routes, g, k):
    full = routes[int(g["route"][k])]
    idx, v = int(g["idx"][k]), float(g["v"][k])
    detailed = full[idx:]
    res = detailed[LO.resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), v))]
    return full, idx, v, detailed, res


@pytest.mark.parametrize("fixture,dims,margin_factor", (("loop_f1.npz", None, 4), ("loop_bicycle.npz", (1.0, 0.45, 0.64), 2)))
def test_uniform_shapes_are_the_oracle_exactly(SN, LO, routes, fixture, dims, margin_factor):
    """Every reference-made case: first_collision_fast and loop_pre_tick of the helper with a table of one shape -- the ego's
    for loop_f1.npz, the cyclist's for loop_bicycle.npz -- return what the oracle returns with that obst_dims, and so (the
    oracle is pinned to them in tests/test_loop_oracle.py) what the reference's functions returned."""
    g = load_golden(fixture)
    shape = SN.shape_of(*(dims or SN.CAR))
    n_col = 0
    for k in range(len(g["route"])):
        full, idx, v, detailed, res = _case(LO, routes, g, k)
        preds = list(g["pred"][k])
        shapes = [shape] * len(preds)
        want = LO.first_collision_fast(res, detailed, preds, obst_dims=dims)
        got = SN.first_collision_fast(res, detailed, preds, shapes)
        assert (got is None) == (want is None) and (got is None or got[:3] == want), k
        flag, cx, cy, first = g["col"][k]
        assert (got is not None) == bool(flag) and (got is None or (got[0], got[1], got[2]) == (cx, cy, int(first))), k
        n_col += got is not None
        if k % 8 == 0:
            assert SN.first_collision(res, detailed, preds, shapes) == got, k
        for p, q in zip(SN.predict(g["obst"][k], shapes), preds):
            np.testing.assert_allclose(p, q, rtol=0, atol=1e-12)
        x, y, yaw = full[idx]
        want = LO.loop_pre_tick((x, y, yaw, v), idx, idx + 1, full, g["obst"][k], float(g["dl"]), obst_dims=dims,
                                margin_factor=margin_factor)
        got = SN.loop_pre_tick((x, y, yaw, v), idx, idx + 1, full, g["obst"][k], float(g["dl"]), shapes,
                               margin_factor=margin_factor)
        assert got[:4] == want and got[2] == int(g["cutoff"][k]), k
        # .. and through the nearest-index branch (no previous path)
        want = LO.loop_pre_tick((x, y, yaw, v), max(idx - 3, 0), None, full, g["obst"][k], float(g["dl"]), obst_dims=dims,
                                margin_factor=margin_factor)
        got = SN.loop_pre_tick((x, y, yaw, v), max(idx - 3, 0), None, full, g["obst"][k], float(g["dl"]), shapes,
                               margin_factor=margin_factor)
        assert got[:4] == want, k
    assert n_col >= 40


def test_mixed_shapes_vectorised_equals_nested_loops(SN, LO, routes):
    """Mixed cases (each obstacle a car or a cyclist, seeded; predictions with each one's wheelbase): the vectorised form
    equals the plain nested-loop form; the mix matters (it differs from both uniform tables on some cases, and hits both kinds)."""
    rng = np.random.default_rng(7)
    car, bike = SN.shape_of(*SN.CAR), SN.shape_of(*SN.BIKE)
    n = {"car": 0, "bike": 0, "not_car": 0, "not_bike": 0, "cases": 0}
    for name in ("loop_f1.npz", "loop_bicycle.npz"):
        g = load_golden(name)
        for k in range(0, len(g["route"]), 2):
            full, idx, v, detailed, res = _case(LO, routes, g, k)
            obst = g["obst"][k]
            kinds = rng.integers(0, 2, len(obst))
            if len(obst) >= 2:
                kinds[:2] = (0, 1) if k % 2 else (1, 0)
            shapes = [bike if c else car for c in kinds]
            preds = SN.predict(obst, shapes)
            fast = SN.first_collision_fast(res, detailed, preds, shapes)
            assert SN.first_collision(res, detailed, preds, shapes) == fast, (name, k)
            n["cases"] += 1
            if fast is not None:
                n["bike" if kinds[fast[3]] else "car"] += 1
            n["not_car"] += SN.first_collision_fast(res, detailed, preds, [car] * len(obst)) != fast
            n["not_bike"] += SN.first_collision_fast(res, detailed, preds, [bike] * len(obst)) != fast
    print(n)
    assert n["cases"] >= 100 and min(n["car"], n["bike"], n["not_car"], n["not_bike"]) >= 5, n


def test_shape_rows_and_dims_checks(pkg, LO):
    """vehicle_shape is car_circles' numbers in the C-ABI's row order; unknown keys and sizes that are not positive raise
    ValueError -- in the loops before anything reaches the device (an object with nothing but B and L stands in for the engine)."""
    CL = pkg.closed_loop
    for dims in (dict(L=1.0, width=0.45, extra_length=0.64), dict(L=2.86), dict()):
        r, (c0, c1) = LO.car_circles(dims.get("L", 2.86), dims.get("width", 2.0), dims.get("extra_length", 0.64))
        assert CL.vehicle_shape(dims) == (c0, c1, r, dims.get("L", 2.86))
    assert CL.vehicle_shape(L=2.5)[3] == 2.5
    spec = dict(direction=1, turning=False, speed=5.0, offset=None)
    assert CL.shape_table([spec, spec], CL.vehicle_shape()) is None
    tab = CL.shape_table([spec, dict(spec, dims=dict(L=1.0, width=0.45))], CL.vehicle_shape())
    assert tab.shape == (2, 4) and tuple(tab[0]) == CL.vehicle_shape() and tuple(tab[1]) == CL.vehicle_shape(dict(L=1.0, width=0.45))
    eng = types.SimpleNamespace(B=4, L=2.86)
    bad = (dict(l=1.0), dict(L=1.0, wheelbase=1.0), dict(L=0.0), dict(L=-1.0), dict(width=0.0), dict(L=1.0, width=-0.45),
           dict(extra_length=-0.1), dict(L=float("nan")), dict(width=float("inf")))
    for dims in bad:
        with pytest.raises(ValueError):
            CL.vehicle_shape(dims)
        with pytest.raises(ValueError):
            pkg.ScenarioLoop(eng, None, [dict(spec, dims=dims)])
        with pytest.raises(ValueError):
            pkg.ScenarioLoop(eng, None, [[spec], [dict(spec, dims=dims)]], traffic_of=[0, 1, 0, 1])
        with pytest.raises(ValueError):
            pkg.InteractingLoop(eng, None, group_sizes=[2, 2], obstacle_specs=[dict(spec, dims=dims)])
        with pytest.raises(ValueError):
            pkg.ScriptedObstacles(eng, [dict(spec, dims=dims)])


def test_sharded_gather_refuses_a_shape_table(pkg):
    eng = types.SimpleNamespace(B=4, vehicle_shapes=np.zeros((1, 4)), traffic_layout=None)
    with pytest.raises(ValueError, match="shape table"):
        pkg.sharding.CabiGather(eng, rank=0, world=2, unique_id=b"\0" * 128)


def test_vehicle_shapes_export_in_header_binding_and_library(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    decl = pkg._header.header().functions["jsim_loop_set_vehicle_shapes"]
    assert decl.ret == "int" and decl.params == (("jsim_ctx *", "ctx"), ("int32_t", "n"), ("const double *", "shapes"))
    assert "collision_avoidance.py:126-165" in hdr and "moving_obstacles_prediction.py:21-47" in hdr
    assert hasattr(ctypes.CDLL(pkg.build.build()), "jsim_loop_set_vehicle_shapes")
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_set_vehicle_shapes.argtypes) == 3
    assert lib.jsim_loop_set_vehicle_shapes(None, 1, None) == -22       # null ctx: refused before anything else
    assert "jsim_loop_set_vehicle_shapes" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_every_pre_row_has_a_uniform_table_case():
    """tests/test_gpu_vehicle_shapes.py runs the uniform-table comparison on every PRE row of config.REG_VARIANTS (its
    parameter list is plain data), and on a horizon without a register kernel (the LDS kernel, host ticks)."""
    gpu = importlib.import_module("test_gpu_vehicle_shapes")
    pre_rows = [row for row in CFG.REG_VARIANTS if row[2]]
    assert len(pre_rows) == 10 and sorted(gpu.UNIFORM_ROWS) == sorted(pre_rows)
    reg_T = {row[1] for row in CFG.REG_VARIANTS}
    assert gpu.LDS_T not in reg_T
    assert set(gpu.MIXED_T) == {13, 20, 24, 40}
