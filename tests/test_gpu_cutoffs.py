"""The collision cut-off of every recorded tick on the device (Recorder.cutoffs / jsim_loop_eval_cutoffs): the
reference's own loops (tests/golden/loop_real_T13.npz, loop_interact_T13.npz) recorded and replayed; the replay of a fused run
against the live glue of host ticks, bit for bit, with both glues, with traffic sets and vehicle shapes, and with interacting
groups; a run evaluated in pieces; a recorder that overflowed; and the refusals that read the context."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_helpers import W, iroutes, loop_engine  # noqa: F401
from recorder_checks import assert_replay_equals_live, assert_replay_equals_run1, live_rows, run1_rows

pytestmark = pytest.mark.gpu

KEYS = ("status", "idx", "cut", "hit", "first", "col_xy")
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)


def test_reference_loop_recorded_and_replayed(pkg):
    """tests/golden/loop_real_T13.npz, the mpc_intersection loop run by the reference's own code: its 91 ticks as one fused run with a
    recorder, then the replay: idx_out, len(tmp_trajectory) and the collision flag of every tick."""
    g = load_golden("loop_real_T13.npz")
    t = g["ticks"]
    PL = pkg.planner
    rad, _ = PL.car_circles()
    full = PL.plan_routes([PL.intersection_query(1, 1, rad)], device=0)[0].trajectory.copy()
    specs = [dict(direction=int(d), offset=float(o), turning=bool(tn), speed=float(s)) for d, o, tn, s in g["obstacle_specs"]]
    eng = pkg.BatchedMPC([full.copy()], [0], dl=float(g["dl"]), T=13)
    x0 = torch.tensor([[full[0, 0], full[0, 1], 0.0, eng.paths[0][0, 2]]], dtype=torch.float64, device=eng.device)
    sc = pkg.ScenarioLoop(eng, x0, specs, max_age=0, record=92)
    sc.run(91)
    out = sc.recorder.cutoffs()
    assert out["status"].shape == (91, 1) and not out["status"].any()
    assert np.array_equal(out["idx"][:, 0], t[:, 6].astype(np.int64))
    assert np.array_equal(out["cut"][:, 0], t[:, 7].astype(np.int64))
    assert np.array_equal(out["hit"][:, 0], t[:, 8] != 0) and int(out["hit"].sum()) == 35
    assert np.array_equal(np.isnan(out["col_xy"]).any(axis=2), ~out["hit"]) and np.array_equal(out["first"] >= 0, out["hit"])
    assert out["carry"].tolist() == [[0, -1, int(t[-1, 7])]]              # the ego reached its goal on the last tick
    eps = pkg.history.cutoff_episodes(out, sc.recorder.flags[:91].cpu().numpy())[0]
    assert len(eps) == 2 and eps[0]["n_cut"] == 35 and eps[1]["n_cut"] == 0 and eps[0]["first_cut_tick"] == int(np.argmax(t[:, 8] != 0))


def test_interacting_reference_loop_recorded_and_replayed(pkg):
    """tests/golden/loop_interact_T13.npz, interactive_mpc.py's two egos run by the reference's own code: 150 ticks."""
    g = load_golden("loop_interact_T13.npz")
    t = g["ticks"]
    K, n = t.shape[:2]
    PL = pkg.planner
    rad, _ = PL.car_circles()
    full = [r.trajectory.copy() for r in PL.plan_routes([PL.intersection_query(int(tn), int(sp), rad) for sp, tn in g["egos"]], device=0)]
    eng = pkg.BatchedMPC([f.copy() for f in full], list(range(n)), dl=float(g["dl"]), T=13)
    x0 = torch.tensor([[f[0, 0], f[0, 1], 0.0, eng.paths[j][0, 2]] for j, f in enumerate(full)], dtype=torch.float64, device=eng.device)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[n], max_age=0, frame_window=int(g["frame_window"]), record=K)
    il.run(K)
    out = il.recorder.cutoffs()
    assert (K, n) == (150, 2) and out["status"].shape == (K, n) and not out["status"].any()
    assert np.array_equal(out["idx"], t[:, :, 6].astype(np.int64))
    assert np.array_equal(out["cut"], t[:, :, 7].astype(np.int64))
    assert np.array_equal(out["hit"], t[:, :, 8] != 0) and int(out["hit"].sum()) == int(t[:, :, 8].sum()) >= 10


def same(a, b):
    """torch.equal with NaN equal to NaN."""
    return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)


SCENARIO = {"truncate": 13, "speed_cutoff": 20}     # mode -> horizon
S_B, S_K = 64, 70
_scenario = {}


def scenario_case(pkg, W, iroutes, mode):
    """Loop a driven by host ticks, split as ScenarioLoop.tick() splits them so that the glue's outputs are read behind pre.run; loop
    b as one fused run with a recorder.  (live series, loop a, loop b), made once per mode."""
    if mode in _scenario:
        return _scenario[mode]
    T = SCENARIO[mode]
    batch = W.ego_batch(iroutes, S_B, T, rank=3)
    mk = lambda record: pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T, mode), W.OBSTACLE_SPECS, max_age=60, frame_window=20,  # noqa: E731
                                         mode=mode, record=record)
    a, b = mk(0), mk(S_K)
    eng, pre = a.loop.eng, a.pre
    rows = []
    for _ in range(S_K):
        pre.predict(a.obst.get(step=False))
        pre.run(a.loop.x0)
        rows.append({"status": pre.status.clone(), "idx": pre.traj_idx.clone(), "hit": pre.col_flag.clone(), "first": pre.first_idx.clone(),
                     "cut": (eng.path_len if mode == "truncate" else pre.cut).clone(), "col_xy": pre.col_xy.clone()})
        a.loop.tick()
        resp = a.loop.age == 0
        pre.traj_idx.masked_fill_(resp, 0)
        pre.prev_len.masked_fill_(resp, -1)
        a.obst.get(step=True)
    b.run(S_K)
    torch.cuda.synchronize()
    _scenario[mode] = (live_rows(rows), a, b)
    return _scenario[mode]


@pytest.mark.parametrize("mode", tuple(SCENARIO))
def test_replay_of_a_fused_run_equals_the_live_glue_of_host_ticks(pkg, W, iroutes, mode):
    live, a, b = scenario_case(pkg, W, iroutes, mode)
    n_hit, n_bad = int((live["hit"] != 0).sum()), int((live["status"] != 0).sum())
    print(f"{mode}: {S_B} egos x {S_K} ticks, {n_hit} ego-ticks cut off, {n_bad} refused by the glue, {int(a.loop.n_respawn.item())} respawns")
    assert n_hit >= 1 and int(a.loop.n_respawn.item()) >= 1                # asserted on the live series, not on the replay
    assert torch.equal(a.loop.x0, b.loop.x0) and torch.equal(a.pre.traj_idx, b.pre.traj_idx)
    rep = b.recorder._cutoffs_device(chunk_ticks=7)
    assert_replay_equals_live(rep, live, mode)
    # after the last tick the carry is the loop's own glue state
    car = rep["carry"]
    assert torch.equal(car[:, 0], b.pre.traj_idx.to(torch.int32)) and torch.equal(car[:, 1], b.pre.prev_len)
    assert torch.equal(car[:, 2], b.loop.eng.path_len if mode == "truncate" else b.pre.cut)


def test_pieces_and_a_null_carry(pkg, W, iroutes):
    """Ticks [0, 23) and then [23, K) from the returned carry equal one call; a NULL carry of the entry point is the loops' start."""
    _, _, b = scenario_case(pkg, W, iroutes, "truncate")
    rec = b.recorder
    one = rec._cutoffs_device()
    p1 = rec._cutoffs_device(chunk_ticks=5, n=23)
    p2 = rec._cutoffs_device(chunk_ticks=9, carry=p1["carry"].cpu().numpy(), first_tick=23)
    for k in KEYS:
        assert same(torch.cat([p1[k], p2[k]]), one[k]), k
    assert torch.equal(p2["carry"], one["carry"]) and not torch.equal(p1["carry"], one["carry"])
    eng, g = b.loop.eng, rec.glue
    outs = [torch.full_like(one[k], -9) for k in KEYS]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = eng.lib.jsim_loop_eval_cutoffs(eng._ctx, eng.B, S_K, ptr(rec.rec), ptr(rec.flags), rec.n_obs, ptr(rec.obs), ptr(rec.x0_first),
                                        ptr(b.loop.x0_spawn), g["frame_window"], g["margin"], g["n_steps"], 0, 0, 0, 0, None,
                                        *[ptr(t) for t in outs], eng._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, t in zip(KEYS, outs):
        assert same(t, one[k]), k


def test_overflowed_recorder_replays_what_it_holds(pkg, W, iroutes):
    """record = K // 2: the recorded ticks are evaluated, with the recorder's overflow warning."""
    _, _, b = scenario_case(pkg, W, iroutes, "truncate")
    full = b.recorder.cutoffs()
    batch = W.ego_batch(iroutes, S_B, 13, rank=3)
    c = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, 13), W.OBSTACLE_SPECS, max_age=60, frame_window=20, record=S_K // 2)
    c.run(S_K)
    with pytest.warns(RuntimeWarning, match="are not recorded"):
        half = c.recorder.cutoffs()
    for k in KEYS:
        assert half[k].shape[0] == S_K // 2 and np.array_equal(half[k], full[k][: S_K // 2], equal_nan=True), k
    assert np.array_equal(half["carry"], b.recorder._cutoffs_device(n=S_K // 2)["carry"].cpu().numpy())


def test_traffic_sets_and_vehicle_shapes(pkg, W, iroutes):
    """Every ego with its own set's vehicles, one of them a cyclist: the replay in chunks of 7 ticks and in one chunk against run(1) x
    K."""
    T, B, K = 13, 48, 30
    batch = W.ego_batch(iroutes, B, T, rank=2)
    sets, tof = W.traffic_batch(B, seed=5, n_sets=6)
    s = next(i for i, st in enumerate(sets) if st and i in set(tof.tolist()))
    sets[s][0] = dict(sets[s][0], dims=CYCLIST)
    mk = lambda record: pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T), sets, max_age=W.MAX_AGE, traffic_of=tof, record=record)  # noqa: E731
    a, b = mk(0), mk(K)
    live, resp = run1_rows(a, K)
    assert int((live["hit"] != 0).sum()) >= 1 and b.loop.eng.vehicle_shapes is not None
    b.run(K)
    r7, r0 = b.recorder._cutoffs_device(chunk_ticks=7), b.recorder._cutoffs_device(chunk_ticks=0)
    for k in KEYS + ("carry",):
        assert same(r7[k], r0[k]), k
    assert_replay_equals_run1(r7, live, resp, "traffic sets")
    # the context's tables are the call's: a vehicle count that is not the layout's total is refused, with its message
    rec = b.recorder
    rec.n_obs -= 1
    with pytest.raises(pkg._cabi.JsimError, match="but the traffic sets hold"):
        rec.cutoffs()
    rec.n_obs += 1


def test_interacting_groups(pkg, W, iroutes):
    """Groups of 1, 3, 4 and 8 egos, each with its own scripted vehicles (4, 2, 3, none: vehicles + mates <= 8): host ticks against
    run(K) and the replay, in one call and in pieces."""
    T, K = 13, 40
    batch, _ = W.interacting_batch(iroutes, 4, T, seed=9)
    sets = [W.OBSTACLE_SPECS, W.OBSTACLE_SPECS[:2], W.OBSTACLE_SPECS[1:], []]
    mk = lambda record: pkg.InteractingLoop(*loop_engine(pkg, iroutes, batch, T), group_sizes=[1, 3, 4, 8], obstacle_specs=sets,  # noqa: E731
                                            max_age=25, traffic_of=np.arange(4), record=record)
    a, b = mk(0), mk(K)
    live, resp = run1_rows(a, K)
    mates = (live["hit"][:, 8:] != 0).sum()                                 # the group of eight meets no scripted vehicle
    print(f"interacting: {int((live['hit'] != 0).sum())} ego-ticks cut off, {int(mates)} of them by group mates alone, {int(resp.sum())} respawns")
    assert int(mates) >= 1 and int(resp.sum()) >= 1
    b.run(K)
    torch.cuda.synchronize()
    assert torch.equal(a.loop.x0, b.loop.x0)
    one = b.recorder._cutoffs_device(chunk_ticks=7)
    assert_replay_equals_run1(one, live, resp, "interacting")
    p1 = b.recorder._cutoffs_device(n=23)
    p2 = b.recorder._cutoffs_device(carry=p1["carry"].cpu().numpy(), first_tick=23, chunk_ticks=4)
    for k in KEYS:
        assert same(torch.cat([p1[k], p2[k]]), one[k]), k
    assert torch.equal(p2["carry"], one["carry"])
    assert torch.equal(one["carry"][:, 0], b.pre.traj_idx.to(torch.int32)) and torch.equal(one["carry"][:, 1], b.pre.prev_len)
    # without groups on the context the interacting replay is refused
    eng = b.loop.eng
    assert eng.lib.jsim_loop_set_groups(eng._ctx, eng.B, 0, None) == 0
    with pytest.raises(pkg._cabi.JsimError, match="no groups set"):
        b.recorder.cutoffs()


def test_refusals_of_the_python_surface_and_the_context(pkg, W, iroutes):
    T, B = 13, 8
    batch = W.ego_batch(iroutes, B, T, rank=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    cl = pkg.closed_loop.ClosedLoop(eng, x0, record=4)
    cl.run(2)
    with pytest.raises(ValueError, match="no glue"):
        cl.recorder.cutoffs()
    sc = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS[:2], record=4)
    assert sc.recorder.cutoffs()["status"].shape == (0, B)                  # nothing recorded yet: nothing to do
    sc.run(3)
    rec = sc.recorder
    ok = rec.cutoffs()
    assert ok["status"].shape == (3, B)
    for bad in (dict(chunk_ticks=-1), dict(chunk_ticks=1.5), dict(carry=np.zeros((B, 2), dtype=np.int32)), dict(carry=np.zeros((B, 3)))):
        with pytest.raises(ValueError):
            rec.cutoffs(**bad)
    rec.glue = dict(rec.glue, mode="speed_cutoff")                          # the engine has no speed cut-off registered
    with pytest.raises(pkg._cabi.JsimError, match="without a registered speed cut-off"):
        rec.cutoffs()
    rec.glue = dict(rec.glue, mode="truncate", interacting=True)
    with pytest.raises(pkg._cabi.JsimError, match="no groups set"):
        rec.cutoffs()
    rec.glue = dict(rec.glue, interacting=False)
    sc2 = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS[:1], record=4)          # a later loop on the engine: its tables now
    with pytest.raises(ValueError, match="replaced this recorder"):
        rec.cutoffs()
    assert sc2.recorder.cutoffs()["status"].shape == (0, B)
