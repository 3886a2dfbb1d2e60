"""Per-vehicle shapes on the device (jsim_loop_set_vehicle_shapes; `dims=` in an obstacle spec, PreTick.predict(shapes=...)):
a uniform table changes no bit on any PRE register kernel, the LDS kernel, both glues, fused launches and host ticks; the
reference's cyclist cases through the table; a car and a cyclist in one traffic_of batch against the numpy restatement
(tests/shapes_numpy.py, pinned to the oracle by tests/test_vehicle_shapes_cpu.py); every ego of that batch against its plain
loop; interacting egos beside a cyclist; refusals and clearing."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, load_golden
from gpu_helpers import (REG_VARIANTS, W, assert_state_equal, cu_count, iroutes, loop_engine, loop_state,  # noqa: F401
                         obstacle_state, sub_batch, variant_batch, variant_id)

pytestmark = pytest.mark.gpu

BIKE = dict(L=1.0, width=0.45, extra_length=0.64)    # BicycleRealDimensions (lib/car_dimensions.py:92-100)
CAR = dict(L=2.86, width=2.0, extra_length=0.64)     # the egos' BicycleModelDimensions
T_INT = lambda d, turn, kmh, off, **kw: dict(direction=d, turning=turn, speed=kmh / 3.6, offset=off, **kw)     # noqa: E731
UNIFORM_ROWS = tuple(row for row in REG_VARIANTS if row[2])     # every PRE row (tests/test_vehicle_shapes_cpu.py checks the list)
LDS_T = 24                                                       # a horizon without a register kernel: host ticks
MIXED_T = (13, 20, 24, 40)
SPECS = [T_INT(1, False, 25, None), T_INT(-1, True, 20, 6.0), T_INT(1, True, 15, 12.0), T_INT(-1, False, 25, 3.0)]


def with_dims(specs, dims):
    return [dict(s, dims=dims) for s in specs]


@pytest.fixture(scope="module")
def SN(oracle):
    import shapes_numpy
    return shapes_numpy


def _global_geometry(sc, dims):
    """The parent's way to give ALL obstacles another shape: jsim_loop_set_obstacle_geometry on the loop's context."""
    eng = sc.loop.eng
    c0, c1, r, L = importlib.import_module(PKG_NAME + ".closed_loop").vehicle_shape(dims)
    assert eng.lib.jsim_loop_set_obstacle_geometry(eng._ctx, c0, c1, r, L) == 0


# ---------------------------------------------------------------------------------------------------------------- 1. uniform
def _uniform_runs(pkg, W, iroutes, T, B, K, mode):
    """The same egos and vehicles run five ways; returns {name: (state, obstacles)}."""
    batch = W.ego_batch(iroutes, B, T, rank=4)
    out = {}

    def run(name, specs, traffic=False, ticks=False, global_dims=None):
        eng, x0 = loop_engine(pkg, iroutes, batch, T, mode)
        kw = dict(traffic_of=np.zeros(B, dtype=np.int64)) if traffic else {}
        sc = pkg.ScenarioLoop(eng, x0, [specs] if traffic else specs, hist_cap=K, max_age=W.MAX_AGE, frame_window=20, mode=mode,
                              record=K, **kw)
        if global_dims is not None:
            _global_geometry(sc, global_dims)
        assert (sc.shapes is not None) == any("dims" in s for s in specs)
        assert (eng.vehicle_shapes is not None) == (sc.shapes is not None)
        if ticks:
            for _ in range(K):
                sc.tick()
        else:
            sc.run(K)
        torch.cuda.synchronize()
        assert int(sc.pre.status.abs().sum().item()) == 0
        out[name] = (loop_state(sc), obstacle_state(sc), int(sc.pre.col_flag.sum().item()), int(sc.loop.n_respawn.item()))

    run("none", SPECS)
    run("car_table", with_dims(SPECS, CAR))
    run("car_table_traffic", with_dims(SPECS, CAR), traffic=True)
    run("car_table_ticks", with_dims(SPECS, CAR), ticks=True)
    run("bike_global", SPECS, global_dims=BIKE)
    run("bike_table", with_dims(SPECS, BIKE))
    run("bike_table_traffic", with_dims(SPECS, BIKE), traffic=True)
    run("bike_table_ticks", with_dims(SPECS, BIKE), ticks=True)
    return out


def _check_uniform(out, what):
    for ref, names in (("none", ("car_table", "car_table_traffic", "car_table_ticks")),
                       ("bike_global", ("bike_table", "bike_table_traffic", "bike_table_ticks"))):
        for n in names:
            assert_state_equal(out[ref][0], out[n][0], (what, n))
            assert_state_equal(out[ref][1], out[n][1], (what, n))
            assert out[ref][2:] == out[n][2:], (what, n)
    print(what, "cut egos at the last tick / respawns: car", out["none"][2:], "cyclist", out["bike_global"][2:])


@pytest.mark.parametrize("mode", ("truncate", "speed_cutoff"))
@pytest.mark.parametrize("row", UNIFORM_ROWS, ids=variant_id)
def test_uniform_table_changes_no_bit_on_every_pre_kernel(pkg, W, iroutes, row, mode):
    """On the batch size at which the dispatch takes `row`: a table of the ego's shape equals no table, a table of the
    cyclist's shape equals the global obstacle geometry -- loop state, outputs, controls, History records and obstacle states, bit
    for bit; through a shared obstacle list, a one-set traffic layout, and host-side ticks (fused single-tick launches)."""
    _, T, _, _, _ = row
    B = variant_batch(row, cu_count())
    _check_uniform(_uniform_runs(pkg, W, iroutes, T, B, 24, mode), (variant_id(row), mode))


@pytest.mark.parametrize("mode", ("truncate", "speed_cutoff"))
@pytest.mark.parametrize("T,force", ((LDS_T, False), (20, True)))
def test_uniform_table_changes_no_bit_on_the_lds_kernel(pkg, W, iroutes, monkeypatch, T, force, mode):
    """The same on host ticks: a horizon without a register kernel, and T = 20 sent through the LDS kernel."""
    if force:
        monkeypatch.setenv("JSIM_FORCE_LDS_KERNEL", "1")
    _check_uniform(_uniform_runs(pkg, W, iroutes, T, 96, 24, mode), (T, force, mode))


def test_uniform_table_pre_tick_and_interacting(pkg, W, iroutes, routes):
    """PreTick: predict(shapes=) with the cyclist's rows equals obstacle_dims=, with the ego's rows equals neither argument --
    predictions, path_len, traj_idx, flag, point, first_idx.  InteractingLoop: a table of the ego's shape equals no table."""
    g = load_golden("loop_bicycle.npz")
    CL = pkg.closed_loop
    pres = []
    for od, dims in ((dict(BIKE), None), (None, BIKE), (None, None), (None, CAR)):
        eng = pkg.BatchedMPC(routes, np.zeros(1, dtype=np.int32), dl=float(g["dl"]), T=13, smooth=False)
        pres.append((pkg.PreTick(eng, obstacle_dims=od, margin_factor=2), dims))
    x0 = torch.zeros(1, 4, dtype=torch.float64, device="cuda:0")
    for k in range(0, len(g["route"]), 2):
        rid, idx, v = int(g["route"][k]), int(g["idx"][k]), float(g["v"][k])
        full = routes[rid]
        x0[0, 0], x0[0, 1], x0[0, 2], x0[0, 3] = full[idx, 0], full[idx, 1], v, full[idx, 2]
        res = []
        for pre, dims in pres:
            pre.eng.path_id.fill_(rid)
            pre.traj_idx.fill_(idx)
            pre.prev_len.fill_(idx + 1)
            obst = torch.from_numpy(np.ascontiguousarray(g["obst"][k])).to("cuda:0")
            sh = None if dims is None else np.array([CL.vehicle_shape(dims)] * len(obst))
            pred = pre.predict(obst, shapes=sh).clone()
            pre.run(x0)
            torch.cuda.synchronize()
            res.append((pred, pre.eng.path_len.clone(), pre.traj_idx.clone(), pre.col_flag.clone(), pre.first_idx.clone(),
                        pre.col_xy.clone() * pre.col_flag, pre.status.clone()))
        for a, b in ((0, 1), (2, 3)):
            for u, w_ in zip(res[a], res[b]):
                assert torch.equal(u, w_), (k, a, b)
    # interacting egos
    T, G, K = 13, 12, 30
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=13)
    runs = []
    for specs in (SPECS[:3], with_dims(SPECS[:3], CAR)):
        eng, xs = loop_engine(pkg, iroutes, batch, T)
        il = pkg.InteractingLoop(eng, xs, group_sizes=sizes, obstacle_specs=specs, hist_cap=K, max_age=W.MAX_AGE, record=K)
        il.run(K)
        torch.cuda.synchronize()
        runs.append((loop_state(il), obstacle_state(il), il.pred_egos().clone()))
    assert_state_equal(runs[0][0], runs[1][0], "interacting")
    assert_state_equal(runs[0][1], runs[1][1], "interacting")
    assert torch.equal(runs[0][2], runs[1][2])


# -------------------------------------------------------------------------------------------- 2. the reference's cyclist cases
def test_reference_cyclist_cases_through_the_table(pkg, routes):
    """loop_bicycle.npz -- what the reference's MovingObstaclesPrediction(car_dimensions=bicycle_dimensions) and
    check_collision_moving_bicycle returned -- with a shape table in place of obstacle_dims: the bars of
    test_pre_tick_bicycle_obstacles_vs_reference_golden (predictions <= 1e-12; flag, cut-off, first index, point exact)."""
    g = load_golden("loop_bicycle.npz")
    bike = pkg.closed_loop.vehicle_shape(BIKE)
    eng = pkg.BatchedMPC(routes, np.zeros(1, dtype=np.int32), dl=float(g["dl"]), T=13, smooth=False)
    pre = pkg.PreTick(eng, margin_factor=2)
    assert pre.margin == int(g["margin"])      # 2 * ceil(car radius / dl): the ego's radius, whatever the table holds
    assert pre.radius == float(g["car_radius"]) and bike[2] == float(g["bike_radius"])
    x0 = torch.zeros(1, 4, dtype=torch.float64, device=eng.device)
    n_col = 0
    for k in range(len(g["route"])):
        rid, idx, v = int(g["route"][k]), int(g["idx"][k]), float(g["v"][k])
        eng.path_id.fill_(rid)
        full = routes[rid]
        x0[0, 0], x0[0, 1], x0[0, 2], x0[0, 3] = full[idx, 0], full[idx, 1], v, full[idx, 2]
        pre.traj_idx.fill_(idx)
        pre.prev_len.fill_(idx + 1)
        obst = np.ascontiguousarray(g["obst"][k])
        pred = pre.predict(torch.from_numpy(obst).to(eng.device), shapes=np.array([bike] * len(obst)))
        assert eng.vehicle_shapes.shape == (len(obst), 4)
        pre.run(x0)
        torch.cuda.synchronize()
        assert int(pre.status.item()) == 0 and int(pre.traj_idx.item()) == idx
        np.testing.assert_allclose(pred.cpu().numpy(), g["pred"][k], rtol=0, atol=1e-12)
        flag, cx, cy, first = g["col"][k]
        assert int(pre.col_flag.item()) == int(flag)
        assert int(eng.path_len.item()) == int(g["cutoff"][k])
        if flag:
            n_col += 1
            assert int(pre.first_idx.item()) == int(first)
            assert tuple(pre.col_xy[0].cpu().numpy()) == (cx, cy)
    assert 40 <= n_col <= 110


# ------------------------------------------------------------------------------------- 3 / 4. a car and a cyclist in one batch
def _bike(spec):
    return dict(spec, dims=BIKE)


# a car and a cyclist in both list orders, all cars, all cyclists, a car with explicit dims beside plain ones, an empty set
MIXED_SETS = [[T_INT(1, False, 25, 2.0), _bike(T_INT(-1, True, 20, 4.0))],
              [_bike(T_INT(1, False, 18, 1.0)), T_INT(-1, False, 30, 1.0)],
              [T_INT(-1, False, 30, 1.0), T_INT(1, True, 22, 0.5), T_INT(1, False, 28, 3.0)],
              [_bike(T_INT(1, False, 15, None)), _bike(T_INT(-1, True, 20, 2.0)), _bike(T_INT(-1, False, 12, 0.5))],
              [_bike(T_INT(-1, False, 16, None)), T_INT(1, False, 25, 3.0), _bike(T_INT(1, True, 20, 1.5)), T_INT(-1, True, 24, 2.5)],
              []]
MIXED_B, MIXED_K, MIXED_SAMPLE = 96, 50, 48       # egos, ticks, compared egos (8 per set)


def _mixed_loop(pkg, W, iroutes, T, **kw):
    batch = W.ego_batch(iroutes, MIXED_B, T, rank=3)
    traffic_of = np.arange(MIXED_B) % len(MIXED_SETS)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    sc = pkg.ScenarioLoop(eng, x0, MIXED_SETS, hist_cap=MIXED_K, max_age=W.MAX_AGE, frame_window=20, traffic_of=traffic_of,
                          record=MIXED_K, **kw)
    return batch, traffic_of, eng, sc


# (T = 24 has no register kernel: its run calls are host ticks already)
MIXED_RUNS = tuple((T, how) for T in MIXED_T for how in ("fused", "host") if not (T == LDS_T and how == "fused"))


@pytest.mark.parametrize("T,how", MIXED_RUNS)
def test_mixed_traffic_against_the_restatement(pkg, W, iroutes, SN, monkeypatch, T, how):
    """Every tick, the sampled egos' glue equals tests/shapes_numpy.py on the device's own inputs (tick-start state, loop state,
    the tick's get() tuples), exactly:
      * progress index, path length and flag as the loop's own kernels (the fused register kernel, or the host-tick glue) left them;
      * first index and collision point of the loop's own kernels, which they do not store, through the cut-off they do store:
        where the cut-off is not clamped to idx + 1, path_len = idx + first - margin, so the exact path length IS the first
        index (the path's points are distinct) and the point is that path point -- counted per kind of vehicle hit;
      * first index and collision point as stored, from jsim_loop_pre_tick (loop_pre_tick_kernel, the same jsim_pre_tick_ego) run
        every tick on the same inputs with the set's table rows -- counted per kind, too.
    Obstacle states and predictions follow predict_obstacle at each vehicle's wheelbase (<= 1e-12).  The workload is only accepted
    when both kinds are hit first >= 50 times (and as often compared in both ways above) and the cut-off differs from what an
    all-car and an all-cyclist geometry give on >= 20 compared ego-ticks each (else a threshold mix-up would go unseen).  These
    counts are read off the device's run: the routes come from the GPU planner, so the workload cannot be replayed without one."""
    import loop_oracle as LO
    if how == "host" and T != LDS_T:
        monkeypatch.setenv("JSIM_FORCE_LDS_KERNEL", "1")
    batch, traffic_of, eng, sc = _mixed_loop(pkg, W, iroutes, T)
    CL = pkg.closed_loop
    set_of, obs_off = sc.traffic
    flat = [sp for st in MIXED_SETS for sp in st]
    shapes = [CL.vehicle_shape(sp.get("dims")) if "dims" in sp else CL.vehicle_shape(L=float(eng.L)) for sp in flat]
    assert np.array_equal(np.array(shapes), sc.shapes) and np.array_equal(eng.vehicle_shapes, sc.shapes)
    car, bike = SN.shape_of(*SN.CAR), SN.shape_of(*SN.BIKE)
    assert all(tuple(s) in (car, bike) for s in shapes)
    sample = [b for b in range(MIXED_B) if (b // len(MIXED_SETS)) % 2 == 0][:MIXED_SAMPLE]
    dl, dt = float(eng.dl), float(eng.dt)
    margin = sc.pre.margin
    assert margin == LO.extra_cutoff_margin(dl)
    # the single-tick glue of every non-empty set's sampled egos, on a context of its own with the set's rows of the table
    side = {}
    for s in range(len(MIXED_SETS)):
        if obs_off[s + 1] > obs_off[s]:
            egos = [b for b in sample if set_of[b] == s]
            e2, _ = loop_engine(pkg, iroutes, sub_batch(batch, np.array(egos)), T)
            side[s] = (egos, e2, pkg.PreTick(e2, frame_window=20))
    n = dict(car=0, bike=0, not_car=0, not_bike=0, ticks=0, own_car=0, own_bike=0, stored_car=0, stored_bike=0)
    worst = 0.0
    for k in range(MIXED_K):
        xs = sc.loop.x0.cpu().numpy().copy()
        idx_in = sc.pre.traj_idx.cpu().numpy().copy()
        prev = sc.pre.prev_len.cpu().numpy().copy()
        ostate = sc.obst.state.cpu().numpy().copy()
        sc.tick()
        torch.cuda.synchronize()
        get = sc.obst.get_buf[: sc.obst.n].cpu().numpy()           # t-intersection vehicles: both get() calls of a tick agree
        assert np.array_equal(get[:, :2], ostate[:, :2]) and np.array_equal(get[:, 3], ostate[:, 2])
        preds_all = SN.predict(get, shapes)
        if k % 10 == 0:   # the stepped states: Bicycle.step with each vehicle's own wheelbase
            after = sc.obst.state.cpu().numpy()
            for o, sh in enumerate(shapes):
                x, y, v, yaw, _, steer = get[o]
                want = (x + v * np.cos(yaw) * dt, y + v * np.sin(yaw) * dt, yaw + (v / sh[3]) * np.tan(steer) * dt)
                worst = max(worst, float(np.abs(np.array(want) - after[o, :3]).max()))
        plen, col = eng.path_len.cpu().numpy(), sc.pre.col_flag.cpu().numpy()
        idx_out, st, age = sc.pre.traj_idx.cpu().numpy(), sc.pre.status.cpu().numpy(), sc.loop.age.cpu().numpy()
        helper = {}
        for b in sample:
            s = set_of[b]
            lo, hi = obs_off[s], obs_off[s + 1]
            sh, pr = shapes[lo:hi], preds_all[lo:hi]
            full = iroutes[batch.path_id[b]]
            args = ((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]), None if prev[b] < 0 else int(prev[b]), full,
                    get[lo:hi], dl)
            r = helper[b] = SN.loop_pre_tick(*args, sh, frame_window=20, preds=pr)
            assert r[0] == 0 and st[b] == 0, (k, b)
            assert r[2] == int(plen[b]) and (r[3] is not None) == bool(col[b]), (k, b, r, plen[b], col[b])
            if age[b] != 0:
                assert r[1] == int(idx_out[b]), (k, b)
            n["ticks"] += 1
            if r[3] is not None:
                kind = "bike" if tuple(sh[r[5]]) == bike else "car"
                n[kind] += 1
                if int(plen[b]) > r[1] + 1:   # not clamped: the loop's own cut-off gives its first index and point
                    first = int(plen[b]) + margin - r[1]
                    assert first == r[4] and (full[r[1] + first, 0], full[r[1] + first, 1]) == r[3], (k, b)
                    n["own_" + kind] += 1
            if hi > lo:
                n["not_car"] += SN.loop_pre_tick(*args, [car] * (hi - lo), frame_window=20, preds=pr)[2] != r[2]
                n["not_bike"] += SN.loop_pre_tick(*args, [bike] * (hi - lo), frame_window=20, preds=pr)[2] != r[2]
        for s, (egos, e2, pre) in side.items():
            lo, hi = obs_off[s], obs_off[s + 1]
            pred = pre.predict(torch.from_numpy(np.ascontiguousarray(get[lo:hi])).to(e2.device), shapes=np.array(shapes[lo:hi]))
            pre.traj_idx.copy_(torch.from_numpy(idx_in[egos]))
            pre.prev_len.copy_(torch.from_numpy(prev[egos]))
            pre.run(torch.from_numpy(np.ascontiguousarray(xs[egos])).to(e2.device))
            torch.cuda.synchronize()
            if k % 10 == 0:
                for o in range(hi - lo):
                    want = LO.predict_obstacle(*get[lo + o], L=shapes[lo + o][3])
                    worst = max(worst, float(np.abs(pred[o].cpu().numpy() - want).max()))
            p_len, p_col = e2.path_len.cpu().numpy(), pre.col_flag.cpu().numpy()
            p_first, p_xy = pre.first_idx.cpu().numpy(), pre.col_xy.cpu().numpy()
            for i, b in enumerate(egos):
                r = helper[b]
                assert int(p_len[i]) == r[2] == int(plen[b]) and bool(p_col[i]) == (r[3] is not None), (k, s, b)
                if r[3] is not None:
                    assert int(p_first[i]) == r[4] and tuple(p_xy[i]) == r[3], (k, s, b)
                    n["stored_bike" if tuple(shapes[lo + r[5]]) == bike else "stored_car"] += 1
    print(f"T = {T}, {how}: {n}, worst prediction / state error {worst:.3g}")
    assert worst <= 1e-12, worst
    assert n["stored_car"] == n["car"] and n["stored_bike"] == n["bike"], n
    assert min(n["own_car"], n["own_bike"]) >= 50, n
    assert n["car"] >= 50 and n["bike"] >= 50 and n["not_car"] >= 20 and n["not_bike"] >= 20, n


@pytest.mark.parametrize("T", MIXED_T)
def test_each_ego_of_the_mixed_batch_equals_its_plain_loop(pkg, W, iroutes, T):
    """Ego e of the mixed batch equals, bit for bit, a single-set ScenarioLoop whose shared obstacles are set set_of[e] with the
    same table rows (the traffic sets' property); and the batch's one run(K) -- multi-tick fused launches, the
    vehicles rolled forward K ticks with their own wheelbases -- equals K single-tick calls, which anchors the fused path to the
    numpy restatement of test_mixed_traffic_against_the_restatement."""
    batch, traffic_of, eng, sc = _mixed_loop(pkg, W, iroutes, T)
    plain = []
    for s, specs in enumerate(MIXED_SETS):
        e, x = loop_engine(pkg, iroutes, sub_batch(batch, np.flatnonzero(traffic_of == s)), T)
        plain.append(pkg.ScenarioLoop(e, x, specs, hist_cap=MIXED_K, max_age=W.MAX_AGE, frame_window=20, record=MIXED_K))
    _, _, _, ticked = _mixed_loop(pkg, W, iroutes, T)
    sc.run(MIXED_K)
    for p in plain:
        p.run(MIXED_K)
    for _ in range(MIXED_K):
        ticked.tick()              # single-tick launches: what test_mixed_traffic_against_the_restatement compares with numpy
    torch.cuda.synchronize()
    assert_state_equal(loop_state(sc), loop_state(ticked), "run(K) against K ticks")
    assert_state_equal(obstacle_state(sc), obstacle_state(ticked), "run(K) against K ticks")
    _, obs_off = sc.traffic
    for s, p in enumerate(plain):
        idx = torch.from_numpy(np.flatnonzero(traffic_of == s)).to(eng.device)
        assert_state_equal(loop_state(sc, idx), loop_state(p), s)
        if p.obst.n:
            assert_state_equal(obstacle_state(sc, obs_off[s], obs_off[s + 1]), obstacle_state(p), s)
    assert int(sc.loop.n_respawn.item()) == sum(int(p.loop.n_respawn.item()) for p in plain)


# ------------------------------------------------------------------------------------------ 5. interacting egos beside a cyclist
@pytest.mark.parametrize("size", (2, 4))
def test_interacting_egos_beside_a_cyclist(pkg, W, iroutes, SN, size):
    """Groups of `size` egos with a cyclist-shaped scripted vehicle (and a car): every tick the device's glue equals the numpy
    glue fed the scripted vehicles with their own shapes, then the group mates with the ego's -- progress index, path length,
    flag, exact.  The mates' predictions are bit-equal through jsim_loop_predict_egos and jsim_loop_predict_obstacles."""
    T, G, K = 13, 24, 30
    batch4, _ = W.interacting_batch(iroutes, G, T, seed=17)
    keep = np.array([4 * g + k for g in range(G) for k in range(size)])
    batch = sub_batch(batch4, keep)
    specs = [_bike(T_INT(1, False, 15, None)), T_INT(-1, True, 20, 2.0)]
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[size] * G, obstacle_specs=specs, max_age=W.MAX_AGE)
    car, bike = SN.shape_of(*SN.CAR), SN.shape_of(*SN.BIKE)
    shapes = [bike, car]
    assert np.array_equal(eng.vehicle_shapes, np.array(shapes))
    B, dl = eng.B, float(eng.dl)
    n_cut = n_bike = 0
    for k in range(K):
        xs = il.loop.x0.cpu().numpy().copy()
        delta = eng.di_ai[:, 0].cpu().numpy().copy()
        idx_in = il.pre.traj_idx.cpu().numpy().copy()
        prev = il.pre.prev_len.cpu().numpy().copy()
        if k == 3:   # the mates' predictions through both entry points
            pe = il.pred_egos()
            tup = torch.from_numpy(np.stack([xs[:8, 0], xs[:8, 1], xs[:8, 2], xs[:8, 3], np.zeros(8), delta[:8]], axis=1)).to(eng.device)
            po = il.pre.predict(tup.contiguous(), shapes=np.array([car] * 8)).clone()
            assert torch.equal(pe[:8], po)
            il.pre.predict(torch.zeros(0, 6, dtype=torch.float64, device=eng.device))
            pkg.closed_loop._register_shapes(eng, np.array(shapes))
        il.tick()
        torch.cuda.synchronize()
        get = il.obst.get_buf[: il.obst.n].cpu().numpy()
        plen, col = eng.path_len.cpu().numpy(), il.pre.col_flag.cpu().numpy()
        idx_out, st, age = il.pre.traj_idx.cpu().numpy(), il.pre.status.cpu().numpy(), il.loop.age.cpu().numpy()
        tup = [(xs[b, 0], xs[b, 1], xs[b, 2], xs[b, 3], 0.0, delta[b]) for b in range(B)]
        for b in range(B):
            g0 = size * (b // size)
            obst = [tuple(r) for r in get] + [tup[m] for m in range(g0, g0 + size) if m != b]
            sh = shapes + [car] * (size - 1)
            r = SN.loop_pre_tick((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]), None if prev[b] < 0 else int(prev[b]),
                                 iroutes[batch.path_id[b]], obst, dl, sh, frame_window=20)
            assert r[0] == 0 and st[b] == 0, (k, b)
            assert r[2] == int(plen[b]) and (r[3] is not None) == bool(col[b]), (k, b)
            if age[b] != 0:
                assert r[1] == int(idx_out[b]), (k, b)
            n_cut += bool(col[b])
            n_bike += r[5] == 0
    print(f"groups of {size}: {n_cut} ego-ticks cut, {n_bike} of them first by the cyclist")
    assert n_cut > 0 and n_bike > 0


# ---------------------------------------------------------------------------------------------------- 6. refusals and clearing
def test_refusals_leave_the_context_alone_and_clearing_restores(pkg, W, iroutes):
    """Twin loops, one of which is sent every refused call first: -22 with a message for a radius / wheelbase that is not
    positive, another n_obs in the run, obstacle and prediction calls (no obstacle at all passes), speed_cutoff with interacting
    egos (its own message); the following run is bit-identical to the twin's.  n = 0 restores the no-table behaviour; without a
    table jsim_loop_run_interacting still refuses a global obstacle geometry."""
    T, K = 13, 12
    batch, sizes = W.interacting_batch(iroutes, 6, T, seed=5)
    mixed = [_bike(SPECS[0]), SPECS[1], _bike(SPECS[2])]
    P = importlib.import_module(PKG_NAME + ".batched")._ptr
    CL = pkg.closed_loop
    tab = np.array([CL.vehicle_shape(s.get("dims")) for s in mixed])
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def make(specs, cls=None, **kw):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        sc = (cls or pkg.ScenarioLoop)(eng, x0, obstacle_specs=specs, hist_cap=K, max_age=W.MAX_AGE, **kw)
        return eng, sc

    eng, sc = make(mixed)
    _, twin = make(mixed)
    lib, ctx = eng.lib, eng._ctx
    for bad, msg in ((tab * [1, 1, 0, 1], b"radius"), (tab * [1, 1, 1, -1], b"wheelbase"), (tab * [1, 1, -1, 1], b"radius")):
        assert lib.jsim_loop_set_vehicle_shapes(ctx, 3, dp(bad)) == -22 and msg in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_set_vehicle_shapes(ctx, 3, None) == -22 and lib.jsim_loop_set_vehicle_shapes(ctx, -1, dp(tab)) == -22
    assert lib.jsim_loop_run_scenario(ctx, eng.B, 3, *sc._run_args(n_obs=2)) == -22 and b"shape table" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_obstacles(ctx, 2, P(sc.obst.state), P(sc.obst.param), P(sc.obst.get_buf), 1, eng._stream()) == -22
    assert b"shape table" in lib.jsim_last_error(ctx)
    pred = torch.zeros(4, sc.pre.n_steps, 3, dtype=torch.float64, device=eng.device)
    assert lib.jsim_loop_predict_obstacles(ctx, 4, P(sc.obst.get_buf), sc.pre.n_steps, P(pred), eng._stream()) == -22
    assert b"shape table" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_predict_obstacles(ctx, 0, None, sc.pre.n_steps, None, eng._stream()) == 0     # no obstacle at all passes
    assert lib.jsim_loop_set_groups(ctx, eng.B, len(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32).ctypes.data_as(ctypes.c_void_p)) == 0
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 3, *sc._run_args(speed_cutoff=1)) == -22 and b"truncate glue" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 3, *sc._run_args(n_obs=2)) == -22 and b"shape table" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_set_groups(ctx, eng.B, 0, None) == 0
    sc.run(K)
    twin.run(K)
    torch.cuda.synchronize()
    assert_state_equal(loop_state(sc), loop_state(twin), "after refusals")
    assert_state_equal(obstacle_state(sc), obstacle_state(twin), "after refusals")
    # n = 0: the no-table behaviour again
    eng2, cleared = make(mixed)
    assert eng2.lib.jsim_loop_set_vehicle_shapes(eng2._ctx, 0, None) == 0
    _, plain = make([{k: v for k, v in s.items() if k != "dims"} for s in mixed])
    cleared.run(K)
    plain.run(K)
    torch.cuda.synchronize()
    assert_state_equal(loop_state(cleared), loop_state(plain), "cleared")
    assert_state_equal(obstacle_state(cleared), obstacle_state(plain), "cleared")
    # interacting egos: a global geometry without a table is still refused, with a table it runs
    eng3, il = make(SPECS[:2], cls=pkg.InteractingLoop, group_sizes=sizes)
    _global_geometry(il, BIKE)
    assert eng3.lib.jsim_loop_run_interacting(eng3._ctx, eng3.B, 3, *il._run_args()) == -22 and b"another shape" in eng3.lib.jsim_last_error(eng3._ctx)
    pkg.closed_loop._register_shapes(eng3, tab[:2])
    assert eng3.lib.jsim_loop_run_interacting(eng3._ctx, eng3.B, 3, *il._run_args()) == 0
    torch.cuda.synchronize()
    # the Python layer: ValueError before the device is touched
    for dims in (dict(L=1.0, wheelbase=2.0), dict(L=0.0), dict(width=-1.0)):
        before = loop_state(sc)
        with pytest.raises(ValueError):
            pkg.ScenarioLoop(eng, sc.loop.x0, [dict(SPECS[0], dims=dims)])
        assert_state_equal(before, loop_state(sc), dims)
    with pytest.raises(ValueError, match="shape table"):
        pkg.sharding.CabiGather(eng, rank=0, world=2, unique_id=b"\0" * 128)
