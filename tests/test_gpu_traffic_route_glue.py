"""What the loops' glue and the recorder's evaluators compute in route traffic (kind="route") against the
project's own restatements, on the workload of tests/traffic_route_glue_cases.py: route vehicles that drive where the egos drive.

The glue, tick by tick, exactly: progress index, path length (or speed cut-off) and flag of the loop's own kernels, the first index
and point through the unclamped cut-off, and jsim_loop_pre_tick on a side engine, all against tests/shapes_numpy.py on the device's
own tick-start inputs -- as test_mixed_traffic_against_the_restatement of tests/test_gpu_vehicle_shapes.py holds T-intersection cars.
The evaluators on that run's recording at the bars of their own GPU tests (tests/recorder_checks.py).  The workload is only accepted
when the floors of FLOORS hold on the device's run: the routes come from the GPU planner, so it cannot be replayed without one."""
import numpy as np
import pytest
import torch

import predictions_numpy as PN
import recorder_checks as RK
import traffic_route_glue_cases as GC
import traffic_route_numpy as TR
from gpu_helpers import W, assert_state_equal, iroutes, loop_engine, loop_state, sub_batch  # noqa: F401

pytestmark = pytest.mark.gpu

# (T, how, mode): the fused register kernel, the helper-wave kernel with glue, host ticks of the LDS kernel, the speed cut-off glue
FORMS = ((13, "fused", "truncate"), (20, "fused", "truncate"), (13, "host", "truncate"), (13, "fused", "speed_cutoff"))
# what the sampled ego-ticks of a run must hold, else the test has compared nothing (the issue's floors; `parked` is exact)
FLOORS = dict(route=50, route_cyclist=10, route_standing=10, own_route=20, not_car=10, not_bike=10)
_runs = {}


@pytest.fixture(scope="module")
def SN(oracle):
    import shapes_numpy
    return shapes_numpy


def glue_run(pkg, W, iroutes, SN, T, how, mode, monkeypatch=None):
    """K ticks of the workload's ScenarioLoop, every tick held to the restatement (see the module's docstring): (loop, counts, worst
    prediction error of a route vehicle, every ego's group), made once per form."""
    key = (T, how, mode)
    if key in _runs:
        return _runs[key]
    import loop_oracle as LO
    if how == "host":
        monkeypatch.setenv("JSIM_FORCE_LDS_KERNEL", "1")
    CL = pkg.closed_loop
    batch, sets, groups = GC.workload(W, iroutes, T)
    B, K = GC.B, GC.K
    eng, x0 = loop_engine(pkg, iroutes, batch, T, mode)
    sc = pkg.ScenarioLoop(eng, x0, sets, hist_cap=K, max_age=W.MAX_AGE, frame_window=20, mode=mode, traffic_of=np.arange(B), record=K)
    set_of, obs_off = sc.traffic
    flat = [sp for st in sets for sp in st]
    shapes = [CL.vehicle_shape(sp.get("dims")) if "dims" in sp else CL.vehicle_shape(L=float(eng.L)) for sp in flat]
    assert np.array_equal(np.array(shapes), sc.shapes) and np.array_equal(eng.vehicle_shapes, sc.shapes)
    car, bike = SN.shape_of(*SN.CAR), SN.shape_of(*SN.BIKE)
    assert all(tuple(s) in (car, bike) for s in shapes)
    is_route = np.array([sp.get("kind") == "route" for sp in flat])
    assert (sc.obst.param[:, 6].cpu().numpy() == 3.0).tolist() == is_route.tolist()
    dl = float(eng.dl)
    margin = sc.pre.margin
    assert margin == LO.extra_cutoff_margin(dl)
    want_get, _ = TR.run(sc.obst.routes, sc.obst._state0.cpu().numpy(), sc.obst.param.cpu().numpy(), sc.shapes[:, 3], K)
    # the single-tick glue of every ego that has vehicles, on a context of its own with its set's rows of the table
    side = {}
    for b in range(B):
        if obs_off[b + 1] > obs_off[b]:
            e2, _ = loop_engine(pkg, iroutes, sub_batch(batch, np.array([b])), T, mode)
            side[b] = (e2, pkg.PreTick(e2, frame_window=20, mode=mode))
    twin = {b: b + GC.N_MIXED for b in range(B) if groups[b] == "mixed"}
    n = dict(ticks=0, hit=0, route=0, route_cyclist=0, route_standing=0, own_route=0, stored_route=0, parked=0, not_car=0, not_bike=0,
             kind0=0, order_dependent=0, waiting_predicted=0, parked_predicted=0)
    worst = 0.0
    cut_of = lambda: (eng.path_len if mode == "truncate" else sc.pre.cut).cpu().numpy()     # noqa: E731
    for k in range(K):
        xs = sc.loop.x0.cpu().numpy().copy()
        idx_in = sc.pre.traj_idx.cpu().numpy().copy()
        prev = sc.pre.prev_len.cpu().numpy().copy()
        sc.tick()
        torch.cuda.synchronize()
        get = sc.obst.get_buf[: sc.obst.n].cpu().numpy()
        assert np.abs(get[is_route] - want_get[k][is_route]).max() <= 1e-9, k      # the tick's tuples are the rule's
        preds_all = SN.predict(get, shapes)
        plen, col = cut_of(), sc.pre.col_flag.cpu().numpy()
        idx_out, st, age = sc.pre.traj_idx.cpu().numpy(), sc.pre.status.cpu().numpy(), sc.loop.age.cpu().numpy()
        helper = {}
        for b in range(B):
            lo, hi = obs_off[b], obs_off[b + 1]
            sh, pr = shapes[lo:hi], preds_all[lo:hi]
            full = iroutes[batch.path_id[b]]
            args = ((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]), None if prev[b] < 0 else int(prev[b]), full, get[lo:hi], dl)
            r = helper[b] = SN.loop_pre_tick(*args, sh, frame_window=20, preds=pr)
            assert r[0] == 0 and st[b] == 0, (k, b)
            assert r[2] == int(plen[b]) and (r[3] is not None) == bool(col[b]), (k, b, groups[b], r, plen[b], col[b])
            if age[b] != 0:
                assert r[1] == int(idx_out[b]), (k, b)
            n["ticks"] += 1
            if r[3] is not None:
                o = lo + r[5]
                n["hit"] += 1
                n["parked"] += get[o, 0] == TR.PARK
                if is_route[o]:
                    n["route"] += 1
                    n["route_cyclist"] += tuple(shapes[o]) == bike
                    n["route_standing"] += get[o, 2] == 0.0
                else:
                    n["kind0"] += 1
                if int(plen[b]) > r[1] + 1:   # not clamped: the loop's own cut-off gives its first index and point
                    first = int(plen[b]) + margin - r[1]
                    assert first == r[4] and (full[r[1] + first, 0], full[r[1] + first, 1]) == r[3], (k, b)
                    n["own_route"] += bool(is_route[o])
            if hi > lo:
                n["not_car"] += SN.loop_pre_tick(*args, [car] * (hi - lo), frame_window=20, preds=pr)[2] != r[2]
                n["not_bike"] += SN.loop_pre_tick(*args, [bike] * (hi - lo), frame_window=20, preds=pr)[2] != r[2]
        for a, b in twin.items():             # the same vehicles in reverse list order: the same flag, and the same cut-off ..
            assert col[a] == col[b], (k, a, b)
            if helper[a][2] == helper[b][2]:  # .. unless the restatement itself says that the order decides (see the test's docstring)
                assert plen[a] == plen[b], (k, a, b)
            else:
                n["order_dependent"] += 1
        for b, (e2, pre) in side.items():
            lo, hi = obs_off[b], obs_off[b + 1]
            pred = pre.predict(torch.from_numpy(np.ascontiguousarray(get[lo:hi])).to(e2.device), shapes=np.array(shapes[lo:hi]))
            pre.traj_idx.copy_(torch.from_numpy(idx_in[[b]]))
            pre.prev_len.copy_(torch.from_numpy(prev[[b]]))
            pre.run(torch.from_numpy(np.ascontiguousarray(xs[[b]])).to(e2.device))
            torch.cuda.synchronize()
            if k % 10 == 0:
                for o in range(lo, hi):
                    if is_route[o]:
                        want = LO.predict_obstacle(*get[o], L=shapes[o][3])
                        worst = max(worst, float(np.abs(pred[o - lo].cpu().numpy() - want).max()))
                        n["parked_predicted"] += get[o, 0] == TR.PARK
                        n["waiting_predicted"] += get[o, 2] == 0.0 and get[o, 5] != 0.0
            p_len = int((e2.path_len if mode == "truncate" else pre.cut).item())
            r = helper[b]
            assert p_len == r[2] == int(plen[b]) and bool(pre.col_flag.item()) == (r[3] is not None), (k, b)
            if r[3] is not None:
                assert int(pre.first_idx.item()) == r[4] and tuple(pre.col_xy[0].cpu().numpy()) == r[3], (k, b)
                n["stored_route"] += bool(is_route[lo + r[5]])
    n = {k: int(v) for k, v in n.items()}
    print(f"T = {T}, {how}, {mode}: {n}, worst prediction error of a route vehicle {worst:.3g}, respawns {int(sc.loop.n_respawn.item())}")
    _runs[key] = (sc, n, worst, groups)
    return _runs[key]


@pytest.mark.parametrize("T,how,mode", FORMS)
def test_route_traffic_against_the_restatement(pkg, W, iroutes, SN, monkeypatch, T, how, mode):
    """Every tick of 60, every ego of 40 (see the module's docstring); the predictions of route vehicles every 10th tick within 1e-12
    of predict_obstacle at the vehicle's own wheelbase, a parked and a waiting vehicle (v = 0, steer != 0) among them; the egos whose
    only vehicle is parked from the first tick equal the same egos without a vehicle bit for bit.
    The eight vehicles in reverse list order: the flag is the same by the rule (a hit exists or not).  The cut-off is the first
    hit's obstacle circle in the order (frame, ego circle, vehicle in list order, ...) of first_collision in tests/shapes_numpy.py:
    where two vehicles touch at the same frame and ego circle, the list order decides which point cuts the path, by the reference's
    own rule.  So the twins' cut-offs are asserted equal only where the restatement gives both the same; elsewhere each equals the
    restatement (as every ego does), and the count of such ticks is printed.
    Counts of the first run on an MI355X: DESIGN.md section 32."""
    sc, n, worst, groups = glue_run(pkg, W, iroutes, SN, T, how, mode, monkeypatch)
    assert worst <= 1e-12, worst
    assert n["stored_route"] == n["route"] and n["parked"] == 0, n
    assert n["parked_predicted"] >= 1 and n["waiting_predicted"] >= 1, n
    assert all(n[k] >= v for k, v in FLOORS.items()), (n, FLOORS)
    gone = torch.from_numpy(np.flatnonzero(np.array(groups) == "gone")).to(sc.loop.eng.device)
    empty = torch.from_numpy(np.flatnonzero(np.array(groups) == "empty")).to(sc.loop.eng.device)
    assert len(gone) == len(empty) == GC.N_GONE
    assert_state_equal(loop_state(sc, gone), loop_state(sc, empty), "a vehicle parked 10^6 m away changes nothing")


# ---- the evaluators on the recording of the T = 13 fused run ----
@pytest.fixture(scope="module")
def recorded(pkg, W, iroutes, SN):
    sc, n, _, groups = glue_run(pkg, W, iroutes, SN, 13, "fused", "truncate")
    return sc, np.array(groups)


def test_conflicts_and_gaps_of_the_recording(pkg, recorded):
    sc, groups = recorded
    r = sc.recorder
    res = r.conflicts(frame_window=20)
    RK.conflicts_equal_restatement(res, RK.conflicts_restate_recorder(r, res), "route traffic, w = 20")
    found = RK.gaps_check_recorder(pkg, r, GC.K, "route traffic")
    g = r.gaps(window=63)
    lead = np.flatnonzero(np.char.startswith(groups, "leader"))
    print(f"episode gaps of the leader egos: {g['ep_gap'][:, lead].max(axis=0).tolist()}")
    assert (g["ep_gap"][:, lead] >= 0).any() and any(v >= 0 for v in found["episode", 63])


def test_headway_and_tracking_of_the_recording(pkg, recorded):
    sc, groups = recorded
    r = sc.recorder
    worst = {}
    res = RK.headway_check_recorder(pkg, r, GC.K, "route traffic", worst)
    RK.headway_check_recorder(pkg, r, GC.K, "route traffic, margin 1.5 m", worst, margin=1.5)
    RK.tracking_check_recorder(pkg, r, GC.K, "route traffic")
    lead = np.flatnonzero(np.char.startswith(groups, "leader"))
    led = (res["lead"][:, lead] >= 0) & np.isfinite(res["thw"][:, lead])
    print(f"leader egos: ticks with a lead vehicle and a finite thw {led.sum(axis=0).tolist()}, with a finite ttc "
          f"{np.isfinite(res['ttc'][:, lead]).sum(axis=0).tolist()}; largest relative error {worst}")
    assert led.sum() >= 20 and np.isfinite(res["ttc"][:, lead]).any()


def test_predictions_of_the_recording(pkg, recorded):
    """Every row against tests/predictions_numpy.py (integers exact, doubles to 1e-9: the bar of test_every_fixture_cut), and a tick
    whose horizon spans a period wrap: there the error is the length of the jump back, tens of metres, on both sides."""
    sc, groups = recorded
    r, eng = sc.recorder, sc.loop.eng
    res = r.predictions(steps=True)
    S, n = sc.pre.n_steps, GC.K
    ref = PN.eval_predictions(r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy(), r.obs[:n].cpu().numpy(), r.x0_first.cpu().numpy(),
                              r.loop.x0_spawn.cpu().numpy(), False, S, res["tol"], eng.dt, sc.shapes[:, 3], float(eng.L))
    pt_i = np.stack([res[k] for k in pkg.history.PS_INT], axis=2)
    pt_d = np.stack([res[k] for k in pkg.history.PS_DOUBLE], axis=2)
    assert np.array_equal(pt_i, ref["pt_i"]) and np.array_equal(res["step_cnt"], ref["step_cnt"])
    assert np.array_equal(np.isnan(pt_d), np.isnan(ref["pt_d"])) and np.array_equal(np.isnan(res["err"]), np.isnan(ref["err"]))
    obs = r.obs[:n].cpu().numpy()
    far = (np.abs(obs[:, :, 0]) >= 1e5)                                 # the vehicle is parked at this tick ..
    far = far | np.array([[far[k:k + S + 1, v].any() for v in range(obs.shape[1])] for k in range(n)])   # .. or within its horizon
    d = np.abs(pt_d - ref["pt_d"])
    e = np.abs(res["err"] - ref["err"])
    near_d, far_d = np.nanmax(d[~far], initial=0.0), np.nanmax(d[far], initial=0.0)
    print(f"|pt_d - restatement|: {near_d:.3g} on poses within the junction, {far_d:.3g} where a pose is parked at 10^6 m; "
          f"|err - restatement| {np.nanmax(e[~far], initial=0.0):.3g} and {np.nanmax(e[far], initial=0.0):.3g}")
    assert near_d <= 1e-9 and far_d <= 1e-9
    per = np.flatnonzero(sc.obst.param[:, 7].cpu().numpy() > 0)
    wrap = int(round(GC.PERIOD_S / eng.dt))
    jump = res["max"][wrap - 3, per]
    print(f"largest error of the predictions made 3 ticks ahead of a period wrap: {jump.tolist()}")
    assert len(per) >= GC.N_CROSS and (res["n"][wrap - 3, per] == S).all() and (jump > 10.0).any()
    assert np.abs(jump - ref["pt_d"][wrap - 3, per, pkg.history.PS_DOUBLE.index("max")]).max() <= 1e-9


def test_cutoffs_of_the_recording_replay_the_live_glue(pkg, W, iroutes, SN, recorded):
    """The replay of the recording against K x run(1) of a twin loop, as test_traffic_sets_and_vehicle_shapes of
    tests/test_gpu_cutoffs.py does; status 0 on every tick."""
    sc, _ = recorded
    batch, sets, _ = GC.workload(W, iroutes, 13)
    a = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, 13), sets, hist_cap=GC.K, max_age=W.MAX_AGE, frame_window=20,
                         traffic_of=np.arange(GC.B))
    live, resp = RK.run1_rows(a, GC.K)
    assert int((live["hit"] != 0).sum()) >= 50 and int((live["status"] != 0).sum()) == 0
    r7, r0 = sc.recorder._cutoffs_device(chunk_ticks=7), sc.recorder._cutoffs_device(chunk_ticks=0)
    for k in ("status", "idx", "cut", "hit", "first", "col_xy", "carry"):
        assert torch.equal(r7[k].nan_to_num(nan=-7.0), r0[k].nan_to_num(nan=-7.0)) if r7[k].is_floating_point() else torch.equal(r7[k], r0[k]), k
    RK.assert_replay_equals_run1(r7, live, resp, "route traffic")
    assert int((r7["status"] != 0).sum()) == 0
