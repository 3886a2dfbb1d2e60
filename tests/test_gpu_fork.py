"""Forking a recorded run on the device (Recorder.fork_state / jsim_loop_fork_state, jsim_loop_obstacles_at, ScenarioLoop.fork,
DESIGN.md section 22): the fork state and the vehicles' fast-forward against snapshots of the live loop, bit for bit; an episode
replayed from its first tick in both glue modes; a mid-episode fork against a loop built by hand; the chain of the overtaking study
-- trigger, situation, candidates on the arterial road, scoring, fork onto the best one; the planner on the arterial road against the
reference's routes; and the refusals."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import reason_ticks_numpy as TN
from conftest import load_golden
from gpu_helpers import W, iroutes, loop_engine  # noqa: F401

pytestmark = pytest.mark.gpu

T = 13
CYCLIST = dict(L=1.0, width=0.45, extra_length=0.64)
GOAL, AGE = 2, 4


def same(a, b):
    """torch.equal with NaN equal to NaN (a failed solve records no xref deviation)."""
    return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def obstacles_at(pkg, eng, state0, param, wheel, ticks):
    """jsim_loop_obstacles_at on an engine's context: device tensors in, the states out."""
    ticks = np.ascontiguousarray(ticks, dtype=np.int32)
    out = torch.full_like(state0, -7.0)
    rc = eng.lib.jsim_loop_obstacles_at(eng._ctx, len(ticks), ptr(state0), ptr(param), ptr(wheel), ticks.ctypes.data_as(ctypes.c_void_p), ptr(out),
                                        eng._stream())
    pkg._cabi.check(rc, eng._ctx, "jsim_loop_obstacles_at")
    return out


# ---- 1. the state is the live state ----
def test_fork_state_and_vehicles_equal_the_live_loop(pkg, W, iroutes):
    B, n = 6, 140
    sets = [[dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(direction=-1, turning=True, speed=25 / 3.6, offset=None)],
            [dict(kind="roundabout", direction=1, turning=True, speed=20 / 3.6, offset=1.0)],
            [dict(kind="arterial", x_init=1.5, y_init=-30.0, speed=25 / 3.6, initial_speed=5 / 3.6, offset=3.0),
             dict(kind="arterial", x_init=2.0, y_init=-12.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)],
            []]
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T)
    loop = pkg.ScenarioLoop(eng, x0, sets, max_age=20, frame_window=20, traffic_of=np.array([0, 1, 2, 3, 0, 2]), record=n + 10)
    snaps = []
    for _ in range(n):
        snaps.append((loop.loop.x0.clone(), loop.loop.age.clone(), loop.obst.state.clone()))
        loop.tick()
    snaps.append((loop.loop.x0.clone(), loop.loop.age.clone(), loop.obst.state.clone()))
    live_x0, live_age, live_obs = (torch.stack([s[j] for s in snaps]) for j in range(3))           # [n + 1][...]
    rec = loop.recorder
    assert rec.ticks_run == n and int(loop.loop.n_respawn.item()) >= 3 * B
    # every ego at every tick 0 .. n: more than 64 rows, ticks on both sides of 64, behind every end
    ego, at = np.tile(np.arange(B), n + 1), np.repeat(np.arange(n + 1), B)
    x0f, k0, age = rec.fork_state(ego, at)
    assert torch.equal(x0f.reshape(n + 1, B, 4), live_x0)
    assert np.array_equal(age.reshape(n + 1, B), live_age.cpu().numpy()) and np.array_equal(k0, at - age)
    flags = rec.flags[:n].cpu().numpy()
    ep = pkg.history.episodes(flags)
    for b in range(B):
        starts = np.concatenate([[0], np.cumsum(ep["ticks"][b])])[:-1]                             # the first tick of every episode
        assert ep["count"][b] >= 4
        want = starts[np.searchsorted(starts, np.arange(n + 1), side="right") - 1]
        assert np.array_equal(k0.reshape(n + 1, B)[:, b], want), b
    second = [int(ep["ticks"][b][0]) for b in range(B)]                                            # the second episode's first / last tick
    for b in range(B):
        for k in (0, 1, 63, 64, 65, second[b], second[b] + int(ep["ticks"][b][1]) - 1, n):
            x, kk, a = rec.fork_state(b, k)
            assert torch.equal(x[0], live_x0[k, b]) and int(a[0]) == int(live_age[k, b]) and int(kk[0]) == k - int(live_age[k, b])
    assert int(rec.fork_state(0, second[0])[2][0]) == 0 and torch.equal(rec.fork_state(0, second[0])[0][0], loop.loop.x0_spawn[0])
    # the vehicles at every tick, each (vehicle, tick) pair a vehicle of one call: more than 64
    nv = loop.obst.n
    assert nv == 5 and loop.shapes is not None
    wheel = torch.from_numpy(np.ascontiguousarray(loop.shapes[:, 3])).to(eng.device)
    got = obstacles_at(pkg, eng, loop.obst._state0.repeat(n + 1, 1), loop.obst.param.repeat(n + 1, 1), wheel.repeat(n + 1),
                       np.repeat(np.arange(n + 1), nv))
    assert torch.equal(got.reshape(n + 1, nv, 4), live_obs)
    # (xc, yc, theta) = the recorded get()'s (x, y, yaw) -- but the record is the tuple of the tick's second call, so on a tick whose
    # first call rewrote the roundabout car's heading (xc <= -3 and yc > 0: theta = -pi) it holds the rewritten heading already
    st, ob = got.reshape(n + 1, nv, 4)[:n], rec.obs[:n]
    assert torch.equal(st[:, :, :2], ob[:, :, :2])
    rewritten = torch.zeros(n, nv, dtype=torch.bool, device=eng.device)
    rewritten[:, 2] = (st[:, 2, 0] <= -3.0) & (st[:, 2, 1] > 0.0)                                   # vehicle 2: the roundabout car, direction +1
    assert torch.equal(st[:, :, 2][~rewritten], ob[:, :, 3][~rewritten]) and bool((ob[:, :, 3][rewritten] == -np.pi).all())
    print(f"ticks on which the roundabout rule rewrites the heading: {int(rewritten.sum())}, of them with another heading before: "
          f"{int((st[:, :, 2][rewritten] != -np.pi).sum())}")
    assert torch.equal(obstacles_at(pkg, eng, loop.obst._state0, loop.obst.param, wheel, np.zeros(nv)), loop.obst._state0)
    # the source is left as it was
    assert not rec.superseded and torch.equal(loop.obst.state, live_obs[n])


# ---- 2. an episode replays from its first tick ----
@pytest.mark.parametrize("mode", ("truncate", "speed_cutoff"))
def test_an_episode_replays_from_its_first_tick(pkg, W, iroutes, mode):
    B, K = 8, 100
    batch = W.ego_batch(iroutes, B, T, rank=3)
    src = pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T, mode), W.OBSTACLE_SPECS, max_age=30, frame_window=20, mode=mode, record=K)
    src.run(K)
    refused = int((src.recorder.cutoffs()["status"] != 0).sum())
    flags = src.recorder.flags[:K].cpu().numpy()
    ep = pkg.history.episodes(flags)
    print(f"{mode}: {B} egos x {K} ticks, {int(src.loop.n_respawn.item())} respawns, {refused} ticks refused by the glue, "
          f"episodes per ego {ep['count'].tolist()}")
    assert refused == 0                                                    # the premise: every tick's glue wrote its cut-off
    assert (ep["count"] >= 3).all()                                        # a second episode that ends, and later respawns
    at = np.array([int(t[0]) for t in ep["ticks"]])
    keep = src.recorder.rec[:K].clone(), src.recorder.flags[:K].clone(), src.loop.x0.clone()
    m = K - int(at.min())
    fork = src.fork(np.arange(B), at, record=m)
    assert torch.equal(fork.loop.x0, src.loop.x0_spawn) and not fork.loop.age.any() and fork.pre.mode == mode
    fork.run(m)
    for b in range(B):
        k = K - int(at[b])
        assert same(fork.recorder.rec[:k, b], src.recorder.rec[at[b]:K, b]), (mode, b)
        assert torch.equal(fork.recorder.flags[:k, b], src.recorder.flags[at[b]:K, b]), (mode, b)
        assert int((flags[at[b]:, b] & (GOAL | AGE) != 0).sum()) >= 1      # later respawns are part of it
    assert same(src.recorder.rec[:K], keep[0]) and torch.equal(src.recorder.flags[:K], keep[1]) and torch.equal(src.loop.x0, keep[2])
    assert not src.recorder.superseded


# ---- 3. a mid-episode fork equals a loop built by hand ----
def shifted(route, d):
    """A route moved d metres to the left of its own heading."""
    out = route.copy()
    out[:, 0] -= d * np.sin(route[:, 2])
    out[:, 1] += d * np.cos(route[:, 2])
    return out


def test_a_mid_episode_fork_equals_a_loop_built_by_hand(pkg, W, iroutes):
    B, m, ticks = 4, 30, (12, 37)
    specs = [dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(kind="roundabout", direction=-1, turning=True, speed=25 / 3.6, offset=1.0),
             dict(kind="arterial", x_init=2.0, y_init=-12.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)]
    batch = W.ego_batch(iroutes, B, T, rank=5)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    src = pkg.ScenarioLoop(eng, x0, specs, max_age=25, frame_window=20, record=64)
    live = {}
    for k in range(max(ticks) + 1):
        if k in ticks:
            live[k] = (src.loop.x0.clone(), src.loop.age.clone(), src.obst.state.clone())
        if k < max(ticks):
            src.tick()                                                     # host ticks
    pid = batch.path_id
    new_paths = [shifted(iroutes[p], 0.4) for p in pid]

    def by_hand(k, paths, rows):
        """A new engine on `paths` for the source egos `rows`, started from the live clones of tick k."""
        e2 = pkg.BatchedMPC([p.copy() for p in paths], np.arange(len(rows)), dl=eng.dl, T=T, speed=batch.speed[rows])
        x, age, obs = live[k]
        lp = pkg.ScenarioLoop(e2, x[rows].clone(), specs, max_age=25, frame_window=20, record=m)
        lp.loop.age.copy_(age[rows])
        lp.obst.state.copy_(obs)
        lp.run(m)
        return lp

    rows = np.arange(B)
    k = ticks[1]
    hand = by_hand(k, new_paths, rows)
    fork = src.fork(rows, k, paths=[p.copy() for p in new_paths], path_id=rows, record=m)
    assert torch.equal(fork.loop.x0, live[k][0]) and torch.equal(fork.loop.age, live[k][1]) and torch.equal(fork.obst.state, live[k][2])
    assert fork.traffic is None                                            # one tick, one shared list: a loop like the source
    fork.run(m)
    assert same(fork.recorder.rec[:m], hand.recorder.rec[:m]) and torch.equal(fork.recorder.flags[:m], hand.recorder.flags[:m])
    assert torch.equal(fork.recorder.obs[:m], hand.recorder.obs[:m])
    assert not same(fork.recorder.rec[:m], src.recorder.rec[:m])           # (the new paths are driven, not the old ones)
    fork.obst.reset()
    assert torch.equal(fork.obst.state, live[k][2])                        # reset() returns to the fork tick
    # rows with ticks of their own in one fork, each against the hand-built loop of its tick
    at = np.array([ticks[0], ticks[1], ticks[0], ticks[1]])
    mixed = src.fork(rows, at, paths=[p.copy() for p in new_paths], path_id=rows, record=m)
    assert mixed.traffic is not None and mixed.obst.n == 2 * len(specs)
    mixed.run(m)
    hands = {ticks[0]: by_hand(ticks[0], new_paths, rows), ticks[1]: hand}
    for r in range(B):
        h = hands[int(at[r])]
        assert same(mixed.recorder.rec[:m, r], h.recorder.rec[:m, r]) and torch.equal(mixed.recorder.flags[:m, r], h.recorder.flags[:m, r]), r
        s = int(mixed.traffic[0][r])
        lo, hi = int(mixed.traffic[1][s]), int(mixed.traffic[1][s + 1])
        assert torch.equal(mixed.recorder.obs[:m, lo:hi], h.recorder.obs[:m]), r
    # one ego onto three paths: three rows with one first state and three different records
    three = src.fork([1, 1, 1], k, paths=[shifted(iroutes[pid[1]], d) for d in (-0.4, 0.0, 0.4)], path_id=[0, 1, 2], record=m)
    assert torch.equal(three.loop.x0, live[k][0][1].expand(3, 4)) and three.traffic is None
    three.run(m)
    r3 = three.recorder.rec[:m]
    assert not same(r3[:, 0], r3[:, 1]) and not same(r3[:, 1], r3[:, 2]) and not same(r3[:, 0], r3[:, 2])
    assert same(r3[:, 2], fork.recorder.rec[:m, 1])                        # the row on the + 0.4 m path is the first fork's ego 1


# ---- 4. the chain of the overtaking study ----
def plant_step(cfg, dt, L, s, delta, a):
    """Simulation.step on (x, y, v, yaw)."""
    x, y, v, th = s
    d = min(max(delta, -cfg.MAX_STEER_RAD), cfg.MAX_STEER_RAD)
    v2 = min(max(v + a * dt, cfg.MIN_SPEED), cfg.MAX_SPEED)
    return np.array([x + v * np.cos(th) * dt, y + v * np.sin(th) * dt, v2, th + (v / L) * np.tan(d) * dt])


def test_the_chain_trigger_candidates_scoring_fork(pkg):
    PL, R, H = pkg.planner, pkg.reasons, pkg.history
    rad, cen = PL.car_circles()
    K, M, speed = 70, 60, 30 / 3.6                                         # MPCParameters.MAX_SPEED_FREEWAY
    road = PL.plan_routes([PL.arterial_query(rad)], device=0)[0]
    assert road.status == 0 and road.trajectory.shape == (540, 3)
    eng = pkg.BatchedMPC([road.trajectory.copy()], [0, 0, 0], dl=0.083, T=T)
    x0 = torch.tensor([[2.0, -22.0, v, np.pi / 2] for v in (0.0, 2.0, 4.0)], dtype=torch.float64, device=eng.device)
    # (the cyclist starts beyond the driver's 12 m range, so the egos enter it -- and run out of patience -- on ticks of their own)
    cyclist = dict(kind="arterial", x_init=2.0, y_init=-22.0 + 13.5, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST)
    src = pkg.ScenarioLoop(eng, x0, [cyclist], max_age=0, frame_window=20, record=K)
    src.run(K)
    par = R.par_row(dt=eng.dt, thr_d=4.0)                                  # (a driver of little patience: the trigger fires while the road
    res = src.recorder.reasons(par=par)                                    # ahead still has room for the cyclist's box and the way back)
    first = res["first_replan"]
    egos = np.flatnonzero(first >= 0)
    print(f"first_replan {first.tolist()}, ends in the source {int(res['ends'].sum())}")
    assert len(egos) >= 2 and len(set(first[egos].tolist())) >= 2 and not res["ends"].any()   # ticks of their own: a fork with sets
    at = first[egos]
    # the candidates of every triggered ego: the arterial road from where it stands, the cyclist's prediction boxed
    pts, length = PL.make_motion_primitives()
    mps = {n: NS(points=pts[j], total_length=float(length[j]), name=n) for j, n in enumerate(PL.MP_NAMES)}
    car = NS(radius=rad, circle_centers=cen)
    n_pred = src.pre.n_steps
    sits, cands = [], []
    for b, k in zip(egos, at):
        sit = R.situation_at(src.recorder, int(b), int(k), [], reasons=res)
        cx, cy, cv, cyaw = sit["cyclist"][:4]
        pred = np.array([[cx + cv * np.cos(cyaw) * eng.dt * j, cy + cv * np.sin(cyaw) * eng.dt * j] for j in range(n_pred)])
        q = PL.arterial_query(rad, replan=dict(trajectory=pred, spawn=(cx, cy), av=sit["ego"][:2]))
        scen = NS(start=q.start, goal_point=q.goal, goal_area=NS(xy1=q.goal_box[:2], xy2=q.goal_box[2:]), allowed_goal_theta_difference=q.tol,
                  obstacles=[NS(to_convex=(lambda margin, o=o: o)) for o in q.obstacles])
        found = PL.MultiTrajectorySearch(scen, car, mps, margin=rad, wh_ego=[1.0], wh_policy=[2.7, 1.0], wh_other=[15, 5]).run_all()
        cands.append([t for _, _, t, _, _, _ in found])
        sit["candidates"], sit["modes"], sit["time_from"] = cands[-1], [0] * len(found), list(range(len(found)))
        sits.append(sit)
    out = R.score_situations(sits, [(1 / 9, 4 / 9, 4 / 9)], [0])
    best = [cands[s][int(out["best"][0, s])] for s in range(len(sits))]
    print(f"triggered egos {egos.tolist()} at {at.tolist()}, candidate statuses {out['status'].tolist()}, best {out['best'][0].tolist()}, "
          f"their leftmost x {[round(float(c[:, 0].min()), 2) for c in best]}")
    assert not out["status"].any()
    fork = src.fork(egos, at, paths=[c.copy() for c in best], path_id=np.arange(len(egos)), speed=speed, record=M)
    x0f, k0, age = src.recorder.fork_state(egos, at)
    start = x0f.cpu().numpy()
    assert not k0.any() and np.array_equal(age, at) and torch.equal(fork.loop.x0, x0f) and bool((fork.loop.eng.speed == speed).all())
    fork.run(M)
    frec, fflags, fobs = fork.recorder.rec[:M].cpu().numpy(), fork.recorder.flags[:M].cpu().numpy(), fork.recorder.obs[:M].cpu().numpy()
    srec, sflags, sobs = src.recorder.rec[:K].cpu().numpy(), src.recorder.flags[:K].cpu().numpy(), src.recorder.obs[:K].cpu().numpy()
    cfg = fork.loop.eng.config
    carry = H.reasons_carry_at(res, egos, at)
    fres = fork.recorder.reasons(par=par, carry=carry)
    veh = fork.recorder.default_cyclist()
    for r, (b, k) in enumerate(zip(egos.tolist(), at.tolist())):
        # the first record is one plant step from the fork state (libm's cos / sin / tan within a few ulp on values below 25:
        # 1e-12 leaves about 100 x)
        want = plant_step(cfg, eng.dt, eng.L, start[r], frec[0, r, 4], frec[0, r, 5])
        np.testing.assert_allclose(frec[0, r, [0, 1, 3, 2]], want, rtol=0, atol=1e-12)
        # the joined History: the source episode up to the start of tick k, then the fork
        whole = src.recorder.histories(b)[0]
        head = H.History(eng.dt)
        for i in range(k + 1):
            head.store(whole.x[i], whole.y[i], whole.yaw[i], whole.v[i], whole.a[i], whole.delta[i], whole.xref_deviation[i])
        tail = fork.recorder.histories(r)[0]
        j = H.join(head, tail)
        assert len(j) == len(head) + len(tail) - 1 and (j.x[k], j.y[k], j.v[k], j.yaw[k]) == tuple(start[r])
        assert np.allclose(np.diff(j.t), eng.dt, rtol=0, atol=1e-9) and j.t[k] == head.t[k]
        step = np.hypot(np.diff(j.x), np.diff(j.y))
        assert np.all(step <= np.abs(j.v[:-1]) * eng.dt + 1e-9)              # continuous in pose: no entry further than its speed allows
        assert (j.x[k + 1], j.y[k + 1]) == (frec[0, r, 0], frec[0, r, 1])
        # the three series go on across the fork: the restatement over the joined recording, cut at tick k
        n1 = len(tail) - 1                                                   # the fork's first episode (it may reach the goal)
        jrec, jflags = np.concatenate([srec[:k, b], frec[:n1, r]])[:, None], np.concatenate([sflags[:k, b], fflags[:n1, r]])[:, None]
        jobs = np.concatenate([sobs[:k, :1], fobs[:n1, veh[r]:veh[r] + 1]])
        ref = TN.eval_ticks(jrec, jflags, jobs, src.recorder.x0_first[b:b + 1].cpu().numpy(), start[r:r + 1], [0], res["par"][b:b + 1],
                            res["threshold"][b:b + 1])
        val = np.stack([fres["policymaker"], fres["driver"], fres["cyclist"], fres["distance"]], axis=2)[:n1, r]
        np.testing.assert_allclose(val, ref["val"][k:, 0], rtol=1e-12, atol=0)
        assert np.array_equal(fres["timers"][:n1, r], ref["timers"][k:, 0])
        assert np.array_equal(fres["below"][:n1, r], ((ref["trig"][k:, 0, None] >> np.arange(1, 4)) & 1) != 0)
        assert np.array_equal(fres["replan"][:n1, r], (ref["trig"][k:, 0] & 1) != 0)
        # the fork's first tick is the trigger tick again, from the same state and beside the same cyclist: the same values, and with
        # the carried tracker the trigger fires on it as it did in the source
        for key in ("policymaker", "driver", "cyclist", "distance", "replan"):
            assert fres[key][0, r] == res[key][k, b], key
        assert np.array_equal(fres["timers"][0, r], res["timers"][k, b]) and fres["replan"][0, r]
        # the forked ego leaves x = 2 towards its candidate's lane
        side = best[r][:, 0].min() - 2.0
        assert side < -0.5 and frec[:n1, r, 0].min() - 2.0 < -0.5


# ---- 5. the planner on the arterial road ----
def test_hip_planner_on_the_arterial_road(pkg):
    PL = pkg.planner
    g = load_golden("arterial.npz")
    rad = float(g["radius"])
    scenes = [int(g[f"r{r}_scene"]) for r in range(int(g["n_routes"]))]
    qs = []
    for i in scenes:
        nl, gl = (int(v) for v in g[f"s{i}_lanes"])
        rp = dict(trajectory=g[f"s{i}_trajectory"], spawn=tuple(g[f"s{i}_spawn"]), av=tuple(g[f"s{i}_av"])) if int(g[f"s{i}_replan"]) else None
        qs.append(PL.arterial_query(rad, num_lanes=nl, goal_lane=gl, replan=rp))
    res = PL.plan_routes(qs, device=0)
    assert len(res) == 4
    for r, out in enumerate(res):
        label = str(g["labels"][scenes[r]])
        ne = int(g[f"r{r}_n_expanded"])
        assert out.status == 0 and abs(out.n_expanded - ne) <= max(1, ne // 50), (label, out.status, out.n_expanded, ne)
        assert list(out.prims) == list(g[f"r{r}_prims"]), label
        assert abs(out.cost - float(g[f"r{r}_cost"])) <= 1e-9 * max(1.0, abs(float(g[f"r{r}_cost"]))), label
        np.testing.assert_allclose(out.nodes, g[f"r{r}_path"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(out.trajectory, g[f"r{r}_traj"], rtol=0, atol=1e-9)


# ---- 6. refusals ----
def test_refusals(pkg, W, iroutes):
    B = 3
    batch = W.ego_batch(iroutes, B, T, rank=2)
    mk = lambda **kw: pkg.ScenarioLoop(*loop_engine(pkg, iroutes, batch, T), W.OBSTACLE_SPECS, max_age=30, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="recording"):
        mk().fork(0, 0)
    loop = mk(record=8)
    loop.run(5)
    rec, eng = loop.recorder, loop.loop.eng
    for ego, at, msg in (([3], [0], r"ego 3 outside \[0, 3\)"), ([0], [6], r"tick 6 outside \[0, 5\]"), ([0, 1], [1, 2, 3], "rows"), ([0.5], [1], "integers")):
        with pytest.raises(ValueError, match=msg):
            rec.fork_state(ego, at)
        with pytest.raises(ValueError, match=msg):
            loop.fork(ego, at)
    with pytest.raises(ValueError, match="path_id"):
        loop.fork(0, 2, paths=[iroutes[0].copy()])
    with pytest.raises(ValueError, match="one route per row"):
        loop.fork([0, 1], 2, path_id=[0])
    with pytest.raises(ValueError, match="at least one row"):
        loop.fork([], [])
    assert rec.fork_state([], [])[0].shape == (0, 4)
    # the C calls with a context: the message goes to the context
    x = torch.zeros(2, 4, dtype=torch.float64, device=eng.device)
    k = torch.zeros(2, dtype=torch.int32, device=eng.device)
    bufs = [ptr(t) for t in (rec.rec, rec.flags, rec.x0_first, loop.loop.x0_spawn)]
    rows = lambda *v: np.array(v, dtype=np.int32)                          # noqa: E731
    for ego, at, msg in ((rows(0, 3), rows(0, 0), "row 1: ego=3 outside [0, B=3)"), (rows(0, 1), rows(0, 6), "row 1: at=6 outside [0, n_ticks=5]")):
        rc = eng.lib.jsim_loop_fork_state(eng._ctx, B, 5, *bufs, 2, ego.ctypes.data, at.ctypes.data, ptr(x), ptr(k), None)
        assert rc == -22 and msg in eng.lib.jsim_last_error(eng._ctx).decode()
    st = loop.obst._state0
    rc = eng.lib.jsim_loop_obstacles_at(eng._ctx, 4, ptr(st), ptr(loop.obst.param), None, rows(0, 1, -2, 3).ctypes.data, ptr(torch.empty_like(st)), None)
    assert rc == -22 and "vehicle 2: ticks=-2" in eng.lib.jsim_last_error(eng._ctx).decode()
    assert torch.equal(obstacles_at(pkg, eng, st, loop.obst.param, None, [0, 0, 0, 0]), st)         # NULL wheelbase: the context's
    # a superseded recorder
    later = pkg.ScenarioLoop(eng, loop.loop.x0, W.OBSTACLE_SPECS, max_age=30, record=4)
    assert rec.superseded and not later.recorder.superseded
    with pytest.raises(ValueError, match="replaced this recorder"):
        rec.fork_state(0, 0)
    with pytest.raises(ValueError, match="replaced this recorder"):
        loop.fork(0, 0)
    # interacting groups
    ib, sizes = W.interacting_batch(iroutes, 1, T)
    il = pkg.InteractingLoop(*loop_engine(pkg, iroutes, ib, T), group_sizes=sizes, max_age=30, record=4)
    il.run(2)
    with pytest.raises(ValueError, match="warm starts .* are not recorded"):
        il.fork(0, 1)
    assert il.recorder.fork_state(0, 1)[0].shape == (1, 4)                 # the state itself is there; the mates' controllers are not
