"""The device History recorder (ClosedLoop / ScenarioLoop / InteractingLoop record=, jsim_loop_set_recorder): against the
reference's own History on its loops (tests/golden/loop_real_T13.npz, loop_interact_T13.npz), fused launches against host ticks
record for record on every kind of kernel that records, the fields against independent sources, no change to any other output,
and graph replay."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_helpers import W, iroutes, loop_engine  # noqa: F401

pytestmark = pytest.mark.gpu


def _rec(r):
    return r.rec.clone(), r.flags.clone(), (r.obs.clone() if r.obs is not None else None)


def _assert_rec_equal(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "rec")
    assert torch.equal(a[1], b[1]), (what, "flags")
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or torch.equal(a[2], b[2])), (what, "obs")


def _fixture_history(g, dt):
    """The reference's HistorySimulation.history of the loop_real fixture: the initial state, the tick-start states of ticks
    1..K-1, then `final`; a / delta / xref_deviation from columns 13 / 12 / 14."""
    t = g["ticks"]
    states = np.vstack([t[:, :4], g["final"][None]])            # x, y, yaw, v
    a = np.concatenate([[0.0], t[:, 13]])
    d = np.concatenate([[0.0], t[:, 12]])
    dev = np.concatenate([[0.0], t[:, 14]])
    tt, cur = [], 0.0
    for _ in range(len(states)):
        cur = cur + dt
        tt.append(cur)
    return states, a, d, dev, tt


def test_history_of_the_reference_intersection_loop(pkg):
    g = load_golden("loop_real_T13.npz")
    PL = pkg.planner
    rad, _ = PL.car_circles()
    full = PL.plan_routes([PL.intersection_query(1, 1, rad)], device=0)[0].trajectory.copy()
    dl = float(np.linalg.norm(full[0, :2] - full[1, :2]))
    specs = [dict(direction=int(d), offset=float(o), turning=bool(t), speed=float(s)) for d, o, t, s in g["obstacle_specs"]]
    K = len(g["ticks"])

    def fresh():
        eng = pkg.BatchedMPC([full.copy()], [0], dl=dl, T=13)
        x0 = torch.tensor([[full[0, 0], full[0, 1], 0.0, eng.paths[0][0, 2]]], dtype=torch.float64, device=eng.device)
        return eng, pkg.ScenarioLoop(eng, x0, specs, hist_cap=K, max_age=0, record=K + 1)

    eng, sc = fresh()
    for _ in range(K):
        sc.tick()
    eng2, sc2 = fresh()
    sc2.run(K)
    torch.cuda.synchronize()
    _assert_rec_equal(_rec(sc.recorder), _rec(sc2.recorder), "host ticks vs run(K)")
    states, a, d, dev, tt = _fixture_history(g, eng.dt)
    for s in (sc, sc2):
        hs = s.recorder.histories(0)
        assert len(hs) == 2 and len(hs[0]) == K + 1
        h = hs[0]
        for name, ref in (("x", states[:, 0]), ("y", states[:, 1]), ("yaw", states[:, 2]), ("v", states[:, 3]), ("a", a),
                          ("delta", d), ("xref_deviation", dev)):
            np.testing.assert_allclose(getattr(h, name), ref, rtol=0, atol=1e-6, err_msg=name)
        assert h.t == tt
        assert all(isinstance(v, float) for v in h.x + h.t + h.xref_deviation)
        # the last tick reaches the goal: episode 1 starts at the spawn state
        h1 = hs[1]
        sp = s.loop.x0_spawn[0].cpu().numpy()
        assert len(h1) == 1 and [h1.x[0], h1.y[0], h1.yaw[0], h1.v[0]] == [sp[0], sp[1], sp[3], sp[2]]
        assert h1.a == h1.delta == h1.xref_deviation == [0.0]
        ep = s.recorder.episodes()
        assert ep["count"][0] == 2 and list(ep["ticks"][0]) == [K, 0] and list(ep["end"][0]) == [1, 0]
        pos = s.recorder.obstacle_positions()
        assert len(pos) == 2 and all(len(p) == K for p in pos)
        for o in range(2):
            assert [i for i, _ in pos[o]] == list(range(K))
            got = np.array([tup for _, tup in pos[o]])
            np.testing.assert_allclose(got, g["ticks"][:, 15 + 6 * o: 21 + 6 * o], rtol=0, atol=1e-10)


def _scenario(pkg, W, iroutes, T, B, K, mode="truncate", traffic=False, chunk=0):
    batch = W.ego_batch(iroutes, B, T, rank=2)
    eng, x0 = loop_engine(pkg, iroutes, batch, T, mode)
    if traffic:
        sets, tof = W.traffic_batch(B, seed=5, n_sets=6)
        return pkg.ScenarioLoop(eng, x0, sets, hist_cap=K, max_age=60, frame_window=20, mode=mode, traffic_of=tof,
                                chunk_ticks=chunk, record=K)
    return pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS, hist_cap=K, max_age=60, frame_window=20, mode=mode, record=K)


@pytest.mark.parametrize("T,B,mode", [(13, 64, "truncate"), (13, 320, "truncate"), (20, 64, "speed_cutoff"),
                                      (20, 320, "truncate"), (24, 32, "truncate"), (40, 32, "speed_cutoff")])
def test_scenario_run_equals_host_ticks_record_for_record(pkg, W, iroutes, T, B, mode):
    """Fused PRE kernels with HELP (B <= CU count) and without at T = 13 / 20, the LDS fallback (T = 24), the four-wave kernel
    (T = 40), both glues: run(K) records what K x tick() records, and the respawns show up as flags."""
    K = 70
    a = _scenario(pkg, W, iroutes, T, B, K, mode)
    for _ in range(K):
        a.tick()
    b = _scenario(pkg, W, iroutes, T, B, K, mode)
    b.run(K)
    torch.cuda.synchronize()
    _assert_rec_equal(_rec(a.recorder), _rec(b.recorder), (T, B, mode))
    fl = b.recorder.flags
    assert int(((fl & 6) != 0).sum().item()) == int(b.loop.n_respawn.item()) > 0


def test_traffic_chunks_record_for_record(pkg, W, iroutes):
    """Per-ego traffic sets, fused in chunks of 7 ticks, against host ticks: rec, flags and every vehicle's get() tuples."""
    T, B, K = 13, 48, 30
    a = _scenario(pkg, W, iroutes, T, B, K, traffic=True, chunk=7)
    a.run(K)
    b = _scenario(pkg, W, iroutes, T, B, K, traffic=True, chunk=1)
    for _ in range(K):
        b.run(1)
    torch.cuda.synchronize()
    _assert_rec_equal(_rec(a.recorder), _rec(b.recorder), "chunks")
    assert a.recorder.obs.shape[1] == a.obst.n and bool((a.recorder.obs[K - 1, :, 2] != 0).any())


def _closed(pkg, W, iroutes, T, B, K, record=0, max_age=40):
    batch = W.ego_batch(iroutes, B, T, rank=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    return pkg.ClosedLoop(eng, x0, hist_cap=K, max_age=max_age, record=record)


@pytest.mark.parametrize("T,B", [(13, 64), (13, 512), (20, 1100)])
def test_closed_loop_run_equals_ticks_on_the_wpe2_kernels(pkg, W, iroutes, T, B):
    """ClosedLoop.run(K) against K x tick(): HELP at 64 egos, the two-waves-per-SIMD kernels above the thresholds."""
    K = 50
    a = _closed(pkg, W, iroutes, T, B, K, record=K)
    for _ in range(K):
        a.tick()
    b = _closed(pkg, W, iroutes, T, B, K, record=K)
    b.run(K)
    torch.cuda.synchronize()
    _assert_rec_equal(_rec(a.recorder), _rec(b.recorder), (T, B))
    assert torch.equal(a.x0, b.x0)


def test_fields_from_independent_sources(pkg, W, iroutes):
    """Host ticks: the deviation equals xref_deviation_and_goal between solve and advance bit for bit (NaN where the solve
    failed), (delta, a) equals hist, the state equals x0 after the advance where no respawn happened, flag counts equal
    n_respawn.  Failures are forced (egos 0..7 above the speed limit at tick 5: the v_0 row cannot hold) and max_age is small."""
    T, B, K = 13, 64, 40
    loop = _closed(pkg, W, iroutes, T, B, K, record=K, max_age=15)
    eng = loop.eng
    devs = []
    for k in range(K):
        if k == 5:
            loop.x0[:8, 2] = 40.0
        eng.solve(loop.x0)
        dev, _ = eng.xref_deviation_and_goal(loop.x0)
        devs.append(torch.where(eng.status == 0, dev, torch.full_like(dev, float("nan"))))
        pkg._cabi.check(eng.lib.jsim_loop_advance(eng._ctx, eng.B, *loop._advance_args()), eng._ctx, "jsim_loop_advance")
        respawned = (loop.recorder.flags[k] & 6) != 0
        assert torch.equal(loop.recorder.rec[k][~respawned][:, [0, 1, 3, 2]], loop.x0[~respawned]), k
    torch.cuda.synchronize()
    r = loop.recorder
    dev_rec = r.rec[:, :, 6]
    ref = torch.stack(devs)
    assert torch.equal(torch.isnan(dev_rec), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert torch.equal(dev_rec[ok], ref[ok])
    assert torch.equal(r.rec[:, :, 4:6], loop.hist[:K])
    failed = (r.flags & 1) != 0
    assert int(failed.sum().item()) >= 8 and torch.equal(failed, torch.isnan(dev_rec))
    assert int(((r.flags & 6) != 0).sum().item()) == int(loop.n_respawn.item()) > 0
    assert int(((r.flags & 4) != 0).sum().item()) > 0


@pytest.mark.parametrize("kind", ("closed", "scenario"))
def test_recording_changes_nothing(pkg, W, iroutes, kind):
    T, B, K = 20, 64, 60
    outs = []
    for record in (0, K):
        if kind == "closed":
            loop = _closed(pkg, W, iroutes, T, B, K, record=record)
            loop.run(K)
            bufs = {}
        else:
            sc = _scenario(pkg, W, iroutes, T, B, K)
            if not record:
                sc = pkg.ScenarioLoop(sc.loop.eng, sc.loop.x0_spawn.clone(), W.OBSTACLE_SPECS, hist_cap=K, max_age=60,
                                      frame_window=20)
            sc.run(K)
            loop = sc.loop
            bufs = dict(traj_idx=sc.pre.traj_idx, prev_len=sc.pre.prev_len, col_flag=sc.pre.col_flag, pre=sc.pre.status,
                        path_len=loop.eng.path_len)
        eng = loop.eng
        torch.cuda.synchronize()
        d = dict(x0=loop.x0, hist=loop.hist, oa=eng.oa, od=eng.od, target_ind=eng.target_ind, **bufs)
        outs.append({k: v.clone() for k, v in d.items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_interacting_reference_loop_episodes(pkg):
    g = load_golden("loop_interact_T13.npz")
    ticks = g["ticks"]
    K, n = ticks.shape[:2]
    PL = pkg.planner
    rad, _ = PL.car_circles()
    res = PL.plan_routes([PL.intersection_query(int(tn), int(sp), rad) for sp, tn in g["egos"]], device=0)
    full = [r.trajectory.copy() for r in res]
    eng = pkg.BatchedMPC([f.copy() for f in full], list(range(n)), dl=float(g["dl"]), T=13)
    x0 = torch.tensor([[f[0, 0], f[0, 1], 0.0, eng.paths[j][0, 2]] for j, f in enumerate(full)], dtype=torch.float64,
                      device=eng.device)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[n], hist_cap=K, max_age=0, frame_window=int(g["frame_window"]), record=K)
    il.run(K)
    torch.cuda.synchronize()
    assert int(ticks[1:, :, 14].sum()) == 4
    age = il.loop.age.cpu().numpy()
    for j in range(n):
        hs = il.recorder.histories(j)
        # a respawn marked at the start of tick k + 1 ends the episode with tick k's record; a respawn at the end of the last tick
        # (age 0 after the run) ends one with the last record
        ends = [k for k in range(K - 1) if ticks[k + 1, j, 14]] + ([K - 1] if age[j] == 0 else [])
        assert len(hs) == len(ends) + 1, (j, len(hs), ends)
        starts = [0] + [k + 1 for k in ends]
        stops = [k + 1 for k in ends] + [K]
        for e, (h, k0, k1) in enumerate(zip(hs, starts, stops)):
            assert len(h) == k1 - k0 + 1, (j, e)
            # entry i >= 1 is the state after tick k0 + i - 1: the start state of tick k0 + i, except an ended episode's last
            # entry (the goal state; the next tick starts at the spawn state)
            last = k1 - 1 if e < len(ends) else k1
            upto = min(last, K - 1)
            if upto > k0:
                got = np.c_[h.x[1:upto - k0 + 1], h.y[1:upto - k0 + 1], h.yaw[1:upto - k0 + 1], h.v[1:upto - k0 + 1]]
                np.testing.assert_allclose(got, ticks[k0 + 1: upto + 1, j, :4], rtol=0, atol=1e-6, err_msg=f"{j} {e}")
            np.testing.assert_allclose(h.a[1:], ticks[k0:k1, j, 13], rtol=0, atol=1e-6)
            np.testing.assert_allclose(h.delta[1:], ticks[k0:k1, j, 12], rtol=0, atol=1e-6)
    assert sum(len(h) - 1 for j in range(n) for h in il.recorder.histories(j)) == n * K


def test_traffic_host_ticks_record_the_vehicles(pkg, W, iroutes):
    """Traffic sets on host ticks (T = 24, no register kernel: the gridded get() + step() launch records the tuples) against
    the fused gridded rollout at T = 13: the vehicles do not depend on the egos, so every tuple is the same; and run(K) equals
    K x run(1) record for record at T = 24."""
    B, K = 24, 25
    fused = _scenario(pkg, W, iroutes, 13, B, K, traffic=True)
    fused.run(K)
    host = _scenario(pkg, W, iroutes, 24, B, K, traffic=True)
    host.run(K)
    ticks = _scenario(pkg, W, iroutes, 24, B, K, traffic=True)
    for _ in range(K):
        ticks.run(1)
    torch.cuda.synchronize()
    assert host.recorder.obs.shape[1] == fused.recorder.obs.shape[1] > 0
    assert torch.equal(host.recorder.obs, fused.recorder.obs)
    _assert_rec_equal(_rec(host.recorder), _rec(ticks.recorder), "T = 24 traffic")


def test_a_later_loop_supersedes_the_recorder(pkg, W, iroutes):
    first = _closed(pkg, W, iroutes, 13, 16, 8, record=8)
    first.run(3)
    later = pkg.ClosedLoop(first.eng, first.x0.clone(), hist_cap=8, max_age=40)
    later.run(2)
    torch.cuda.synchronize()
    assert first.recorder.superseded and later.recorder is None
    with pytest.warns(RuntimeWarning, match="replaced this recorder"):
        first.recorder.episodes()
    assert int((first.recorder.flags[3:] != 0).sum().item()) == 0 and bool((first.recorder.rec[3:] == 0).all())


def test_graph_replay_and_overflow(pkg, W, iroutes):
    T, B, K = 13, 64, 12
    eager = _closed(pkg, W, iroutes, T, B, 3 * K, record=2 * K)
    for _ in range(3 * K):
        eager.tick()
    torch.cuda.synchronize()
    g = _closed(pkg, W, iroutes, T, B, 3 * K, record=2 * K)
    g.capture(K)          # one warm-up tick outside the capture, then K captured
    for _ in range(2):
        g.replay()
    for _ in range(K - 1):
        g.tick()
    torch.cuda.synchronize()
    _assert_rec_equal(_rec(eager.recorder), _rec(g.recorder), "graph")
    assert eager.recorder.overflow and g.recorder.ticks_run == 3 * K
    with pytest.warns(RuntimeWarning):
        hs = eager.recorder.histories(0)
    assert sum(len(h) - 1 for h in hs) == 2 * K


def test_no_tick_recorded_yet_evaluates_to_nothing(pkg, W, iroutes):
    """A recorder that holds no tick yet: every evaluator still hands its entry point valid pointers (an empty tensor has none),
    the call returns and the result has no rows, of the trailing shapes of history.EVALUATORS."""
    B = 3
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, 13, rank=2), 13)
    r = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS[:2], record=4).recorder
    res = {"reasons": r._reasons_device(), "conflicts": r.conflicts(), "gaps": r.gaps(), "tracking": r.tracking(), "headway": r.headway(),
           "static": r.static_conflicts(pkg.planner.intersection_obstacles(1, 1)), "cutoffs": r.cutoffs()}
    assert set(res) == set(pkg.history.EVALUATORS)
    for name, out in res.items():
        for k, _, shape in pkg.history.EVALUATORS[name].outputs:
            assert tuple(out[k].shape) == (0, B, *shape), (name, k)
    assert r.reasons()["first_replan"].tolist() == [-1] * B and r.gaps()["gap"].shape == (0, B)
