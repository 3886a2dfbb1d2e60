"""Route vehicles on the device (kind="route", jsim_loop_set_traffic_routes) against the numpy restatement of
the rule (tests/traffic_route_numpy.py, held to the reference's own vehicles by tests/test_traffic_route_cpu.py): doubles to 1e-9,
integers exact; and wherever the feature only has to leave things as they are or to continue them -- the other kinds beside a route
table, host ticks against the fused run, forks, restores, another process -- bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import traffic_route_cases as RC
import traffic_route_numpy as TR
from conftest import REPO, load_golden
from gpu_helpers import W, iroutes, loop_engine, loop_state, obstacle_state, sub_batch  # noqa: F401
from traffic_route_cases import B, EVERY, N, T

pytestmark = pytest.mark.gpu

ATOL = 1e-9


def same(a, b):
    """torch.equal with NaN equal to NaN (a failed solve records no xref deviation)."""
    return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert same(a[k], b[k]), (what, k)


def records(loop, k0=0, k1=None):
    r = loop.recorder
    return {k: v[k0:k1].clone() for k, v in dict(rec=r.rec, flags=r.flags, obs=r.obs).items()}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bare_engine(pkg, routes):
    return pkg.BatchedMPC(routes, np.zeros(1, dtype=np.int32), dl=pkg.synth.DL, L=2.86, T=T, smooth=False)


def device_ticks(eng, state, param, n_ticks):
    """n_ticks x (get(), then get() + step()) of jsim_loop_obstacles on device tensors, at most eight vehicles a call:
    (get_all [n_ticks][n][6], gets of the first calls [n_ticks][n][6])."""
    n = state.shape[0]
    assert n <= 8
    first, second = [], []
    get = torch.full((n, 6), -7.0, dtype=torch.float64, device=state.device)
    for _ in range(n_ticks):
        for step, keep in ((0, first), (1, second)):
            rc = eng.lib.jsim_loop_obstacles(eng._ctx, n, ptr(state), ptr(param), ptr(get), step, eng._stream())
            assert rc == 0, eng.lib.jsim_last_error(eng._ctx)
            keep.append(get.clone())
    return torch.stack(second).cpu().numpy(), torch.stack(first).cpu().numpy()


# ---- 1. the table's shapes and the rule's edge cases ----
def test_edge_cases_against_the_restatement(pkg, routes):
    """Routes of 2, 3, 1, 64, 65 (a zero-length segment) and 129 points; every edge case of tests/test_traffic_route_cpu.py through
    jsim_loop_obstacles for 70 ticks, get only and get + step; vehicles on the first and on the last route of the table."""
    CL = pkg.closed_loop
    eng = bare_engine(pkg, routes)
    table = TR.case_routes()
    assert [len(r) for r in table] == [2, 3, 1, 64, 65, 129]
    CL._register_routes(eng, table)
    cases = TR.edge_cases()
    names = list(cases)
    assert {cases[k]["route"] for k in names} >= {0, len(table) - 1}
    worst = 0.0
    for lo in range(0, len(names), 8):
        chunk = [cases[k] for k in names[lo:lo + 8]]
        param = TR.case_rows(chunk)
        state = torch.full((len(chunk), 4), 123.0, dtype=torch.float64, device=eng.device)      # the pose slots are outputs ..
        state[:, 3] = 0.0                                                                       # .. only the counter is read
        d_param = torch.from_numpy(param).to(eng.device)
        got, first = device_ticks(eng, state, d_param, 70)
        want, end = TR.run(table, np.zeros((len(chunk), 4)), param, np.full(len(chunk), float(eng.L)), 70)
        assert np.array_equal(got, first)                                                       # get() alone moves nothing
        for i, name in enumerate(names[lo:lo + 8]):
            err = np.abs(got[:, i] - want[:, i]).max()
            worst = max(worst, err)
            assert err <= ATOL, (name, err, int(np.abs(got[:, i] - want[:, i]).max(axis=1).argmax()))
        st = state.cpu().numpy()
        assert np.array_equal(st[:, 3], np.full(len(chunk), 70.0)) and np.abs(st - end).max() <= ATOL
    print(f"{len(names)} cases x 70 ticks: max |device - restatement| = {worst:.3e}")
    # a route index outside the table is clamped into it (the Python layer refuses one; the C-ABI does not fault on one)
    k = dict(cases["s0_positive"])
    rows = TR.case_rows([dict(k, route=-3), dict(k, route=0), dict(k, route=99), dict(k, route=len(table) - 1)])
    state = torch.zeros(4, 4, dtype=torch.float64, device=eng.device)
    got, _ = device_ticks(eng, state, torch.from_numpy(rows).to(eng.device), 5)
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 2], got[:, 3]) and not np.array_equal(got[:, 0], got[:, 2])


def test_a_cyclists_wheelbase_changes_the_steering_angle_only(pkg, routes):
    CL = pkg.closed_loop
    eng = bare_engine(pkg, routes)
    pre = pkg.PreTick(eng)                                                   # (the shape table needs the egos' geometry)
    table = TR.case_routes()
    CL._register_routes(eng, table)
    k = TR.edge_cases()["three_points"]
    param = TR.case_rows([k, k])
    shapes = np.array([pre.default_shape, CL.vehicle_shape(RC.CYCLIST)])
    CL._register_shapes(eng, shapes)
    state = torch.zeros(2, 4, dtype=torch.float64, device=eng.device)
    got, _ = device_ticks(eng, state, torch.from_numpy(param).to(eng.device), 70)
    want, _ = TR.run(table, np.zeros((2, 4)), param, shapes[:, 3], 70)
    assert np.abs(got - want).max() <= ATOL and shapes[0, 3] != shapes[1, 3] == 1.0
    assert np.array_equal(got[:, 0, :5], got[:, 1, :5]) and (got[:, 0, 5] != got[:, 1, 5]).any()


# ---- 2. the reference's own vehicles ----
def test_reference_vehicles_played_along_their_own_poses(pkg, routes):
    g = load_golden("obstacles_scripted.npz")
    vehicles = TR.golden_vehicles(g)
    eng = bare_engine(pkg, routes)
    specs = [dict(kind="route", route=r, speed=v, offset=off or None) for r, v, off, _ in vehicles]
    obst = pkg.ScriptedObstacles(eng, specs, dt=0.2)
    assert len(obst.routes) == 4 and len(eng.traffic_routes) == 4
    got = []
    for _ in range(139):
        obst.get(step=False)
        got.append(obst.get(step=True).clone())
    got = torch.stack(got).cpu().numpy()
    want = np.stack([w[:139] for _, _, _, w in vehicles], axis=1)
    err = np.abs(got - want).max()
    print(f"max |device - reference get()| over 139 ticks of 4 vehicles = {err:.3e}")
    assert err <= ATOL
    assert (want[:, :, 5] != 0).any(axis=0).sum() == 2 and eng.L == 2.86     # the steering angle of the two turning ones included


# ---- 3. the other kinds beside a route table ----
def mixed_sets(routes, with_routes):
    """Nine sets of 8, 8, ..., 6 vehicles = 70 (past one 64-thread block), kinds 0, 1, 2, 3 interleaved; with_routes=False: a
    T-intersection car in every kind-3 row."""
    kinds = [lambda i: dict(direction=1 if i % 8 < 4 else -1, turning=i % 3 == 0, speed=(15 + i % 7) / 3.6, offset=float(i % 5) or None),
             lambda i: dict(kind="roundabout", direction=-1 if i % 8 < 4 else 1, turning=i % 5 != 0, speed=(12 + i % 6) / 3.6, offset=float(i % 3) or None),
             lambda i: dict(kind="arterial", x_init=1.5, y_init=-30.0 + i, speed=(20 + i % 4) / 3.6, initial_speed=(i % 3) / 3.6, offset=float(i % 4) or None),
             lambda i: dict(kind="route", route=routes[i % len(routes)][:60 + 40 * (i % 5)], speed=3.0 + 0.25 * (i % 9), offset=0.4 * (i % 4) or None,
                            s0=float(i % 6), end=("leave", "stop")[(i // 4) % 2], period=None if i % 3 else 4.0) if with_routes else kinds[0](i)]
    flat = [kinds[i % 4](i) for i in range(70)]
    return [flat[lo:lo + 8] for lo in range(0, 70, 8)]


def test_seventy_vehicles_of_all_kinds(pkg, W, iroutes):
    K, Bm = 30, 9
    batch = W.ego_batch(iroutes, Bm, T, rank=3)
    runs = {}
    for with_routes in (True, False):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        loop = pkg.ScenarioLoop(eng, x0, mixed_sets(iroutes, with_routes), max_age=RC.MAX_AGE, frame_window=20, traffic_of=np.arange(Bm), record=K)
        assert loop.obst.n == 70 and (eng.traffic_routes is not None) == with_routes
        loop.run(K)
        torch.cuda.synchronize()
        runs[with_routes] = loop
    a, b = runs[True], runs[False]
    kind3 = np.arange(70) % 4 == 3
    other = torch.from_numpy(np.flatnonzero(~kind3)).to(a.obst.state.device)
    # kinds 0 - 2: the rows of the run without a table, bit for bit -- states, last get() and every recorded tuple
    assert torch.equal(a.obst.state[other], b.obst.state[other]) and torch.equal(a.obst.get_buf[other], b.obst.get_buf[other])
    assert torch.equal(a.recorder.obs[:K, other], b.recorder.obs[:K, other])
    assert (a.obst.param[:, 6].cpu().numpy() == np.arange(70) % 4).all()
    # kind 3: the restatement
    want, end = RC.restated(TR, a, K)
    got = a.recorder.obs[:K].cpu().numpy()
    assert np.isnan(want[:, ~kind3]).all() and np.abs(got[:, kind3] - want[:, kind3]).max() <= ATOL
    st = a.obst.state.cpu().numpy()
    assert np.abs(st[kind3] - end[kind3]).max() <= ATOL and (st[:, 3] == K).all()
    assert (want[:, kind3, 0] == TR.PARK).any() and (want[:, kind3, 2] > 0).any()


# ---- 4. host ticks against the fused run ----
@pytest.mark.parametrize("horizon", (13, 14))
def test_host_ticks_equal_the_fused_run(pkg, iroutes, horizon):
    """T = 13: a register kernel (one rollout of K ticks against K rollouts of one); T = 14: the LDS kernel, host-driven launches."""
    K = 40
    fused, ticked = RC.scenario_loop(pkg, iroutes, T=horizon, record=K), RC.scenario_loop(pkg, iroutes, T=horizon, record=K)
    fused.run(K)
    for _ in range(K):
        ticked.tick()
    torch.cuda.synchronize()
    assert_same(loop_state(fused), loop_state(ticked), horizon)
    assert_same(obstacle_state(fused), obstacle_state(ticked), horizon)
    want, _ = RC.restated(TR, fused, K)
    route = ~np.isnan(want[0, :, 0])
    assert route.sum() == 3 and np.abs(fused.recorder.obs[:K].cpu().numpy()[:, route] - want[:, route]).max() <= ATOL
    print(f"T = {horizon}: cut egos at the last tick {int(fused.pre.col_flag.sum().item())}, respawns {int(fused.loop.n_respawn.item())}")


# ---- 5. the recorder ----
def test_recorder_on_a_run_with_a_parked_vehicle(pkg, iroutes):
    loop = RC.scenario_loop(pkg, iroutes)
    loop.run(N)
    rec = loop.recorder
    want, _ = RC.restated(TR, loop, N)
    route = np.flatnonzero(~np.isnan(want[0, :, 0]))
    pos = rec.obstacle_positions()
    assert len(pos) == loop.obst.n == 6 and route.tolist() == [1, 2, 3]
    for o in route:
        assert [i for i, _ in pos[o]] == list(range(N))
        assert np.abs(np.array([g for _, g in pos[o]]) - want[:, o]).max() <= ATOL
    parked = want[:, 2, 0] == TR.PARK                                        # vehicle 2 leaves its short route within the run
    assert 0 < parked.sum() < N and not parked[0] and parked[-1]
    egos = np.flatnonzero(RC.TRAFFIC_OF == 0)                                # the egos that meet it: place 2 of their list
    c = rec.conflicts(frame_window=20)
    assert np.isfinite(c["clear"][:N][:, egos]).all() and (c["who"][:N][:, egos] >= 0).all()
    h = rec.headway()
    for k in ("gap", "lat", "rate"):
        assert np.isfinite(h[k][:N][parked][:, egos, 2]).all(), k
    assert np.isfinite(h["u_ego"][:N][:, egos]).all()
    p = rec.predictions()
    scored = p["n"][:N, 2] > 0
    assert scored[parked].any()
    for k in ("ade", "fde", "max", "lon", "lat", "yaw"):
        assert np.isfinite(p[k][:N, 2][scored]).all(), k
    assert np.isfinite(p["step_sum"]).all()


# ---- 6. forks and checkpoints ----
@pytest.fixture(scope="module")
def base(pkg, iroutes):
    """The base loop after run(N) with checkpoints: the source of the forks; nothing below changes it."""
    loop = RC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY)
    loop.run(N)
    return loop


def test_a_cold_fork_replays_an_episode_and_places_the_vehicles(pkg, iroutes, base):
    flags = base.recorder.flags[:N].cpu().numpy()
    ep = pkg.history.episodes(flags)
    assert (ep["count"] >= 2).all()
    at = np.array([int(t[0]) for t in ep["ticks"]])                          # the first tick of every ego's second episode
    assert int((base.recorder.cutoffs()["status"] != 0).sum()) == 0          # the premise: every tick's glue wrote its cut-off
    m = N - int(at.min())
    fork = base.fork(np.arange(B), at, record=m)
    assert len(fork.loop.eng.traffic_routes) == 3                            # the specs carried their arrays to the new engine
    # every fork set's vehicles stand where the restatement has them at the set's tick
    all_ticks, _ = RC.restated(TR, base, N)
    for r in range(B):
        s, s0 = int(fork.traffic[0][r]), int(base.traffic[0][r])
        lo, lo0, hi0 = int(fork.traffic[1][s]), int(base.traffic[1][s0]), int(base.traffic[1][s0 + 1])
        st = fork.obst.state[lo:lo + hi0 - lo0].cpu().numpy()
        assert (st[:, 3] == at[r]).all()
        for j in range(hi0 - lo0):
            if not np.isnan(all_ticks[0, lo0 + j, 0]):
                assert np.abs(st[j, :3] - all_ticks[at[r], lo0 + j][[0, 1, 3]]).max() <= ATOL, (r, j)
    fork.run(m)
    for b in range(B):
        k = N - int(at[b])
        assert same(fork.recorder.rec[:k, b], base.recorder.rec[at[b]:N, b]), b
        assert torch.equal(fork.recorder.flags[:k, b], base.recorder.flags[at[b]:N, b]), b
        s, s0 = int(fork.traffic[0][b]), int(base.traffic[0][b])
        lo, hi, lo0, hi0 = int(fork.traffic[1][s]), int(fork.traffic[1][s + 1]), int(base.traffic[1][s0]), int(base.traffic[1][s0 + 1])
        assert torch.equal(fork.recorder.obs[:k, lo:hi], base.recorder.obs[at[b]:N, lo0:hi0]), b
    assert not base.recorder.superseded


def test_restore_and_warm_fork_continue_bit_for_bit(pkg, iroutes, base):
    keep = records(base, 0, N)
    loop = RC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY)
    loop.run(N)
    end = loop.obst.state.clone()
    assert_same(records(loop, 0, N), keep, "the same run")
    loop.restore(1)
    assert int(loop.loop.tick_counter.item()) == EVERY
    loop.recorder.rec[EVERY:].fill_(-1.0)
    loop.recorder.flags[EVERY:].fill_(-1)
    loop.recorder.obs[EVERY:].fill_(-1.0)
    loop.run(N - EVERY)
    assert_same(records(loop, 0, N), keep, "restored")
    assert torch.equal(loop.obst.state, end)
    at, m = 2 * EVERY, N - 2 * EVERY
    fork = base.fork(np.arange(B), at, warm=True, record=m)
    assert len(fork.loop.eng.traffic_routes) == 3
    fork.run(m)
    for r in range(B):
        assert same(fork.recorder.rec[:m, r], base.recorder.rec[at:N, r]) and torch.equal(fork.recorder.flags[:m, r], base.recorder.flags[at:N, r]), r
        s, s0 = int(fork.traffic[0][r]), int(base.traffic[0][r])
        lo, hi, lo0, hi0 = int(fork.traffic[1][s]), int(fork.traffic[1][s + 1]), int(base.traffic[1][s0]), int(base.traffic[1][s0 + 1])
        assert torch.equal(fork.recorder.obs[:m, lo:hi], base.recorder.obs[at:N, lo0:hi0]), r
    assert_same(records(base, 0, N), keep, "the source is left as it was")


def test_checkpoints_continue_in_a_fresh_process(pkg, base, tmp_path):
    path, out = str(tmp_path / "ck.npz"), str(tmp_path / "out.npz")
    base.save_checkpoints(path)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "traffic_route_child.py"), path, "2", str(N - 2 * EVERY), out], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.load(out)
    r = base.recorder
    nan = lambda a: np.nan_to_num(a, nan=-7.0)                               # noqa: E731
    assert int(got["k0"]) == 2 * EVERY and int(got["ticks_run"]) == N
    assert np.array_equal(nan(got["rec"]), nan(r.rec[2 * EVERY:N].cpu().numpy())) and np.array_equal(got["flags"], r.flags[2 * EVERY:N].cpu().numpy())
    assert np.array_equal(got["obs"], r.obs[2 * EVERY:N].cpu().numpy()) and np.array_equal(got["x0"], base.loop.x0.cpu().numpy())
    assert np.array_equal(got["obs_state"], base.obst.state.cpu().numpy())


# ---- 7. interacting groups ----
def test_an_interacting_group_beside_a_route_vehicle(pkg, W, iroutes):
    K = 30
    batch8, _ = W.interacting_batch(iroutes, 2, T, seed=0)
    specs = [dict(kind="route", route=iroutes[4], speed=5.0, offset=0.6, period=5.0)]

    def make():
        eng, x0 = loop_engine(pkg, iroutes, sub_batch(batch8, np.array([0, 1, 2])), T)
        return pkg.InteractingLoop(eng, x0, group_sizes=[3], obstacle_specs=specs, max_age=RC.MAX_AGE, record=K)
    fused, ticked = make(), make()
    fused.run(K)
    for _ in range(K):
        ticked.tick()
    torch.cuda.synchronize()
    assert_same(loop_state(fused), loop_state(ticked), "interacting")
    assert_same(obstacle_state(fused), obstacle_state(ticked), "interacting")
    want, _ = RC.restated(TR, fused, K)
    assert np.abs(fused.recorder.obs[:K].cpu().numpy() - want).max() <= ATOL and (want[25, 0] == want[0, 0]).all()


# ---- 8. clearing and refusals ----
def test_a_later_loop_without_routes_runs_as_on_a_fresh_engine(pkg, W, iroutes):
    K = 20
    batch = W.ego_batch(iroutes, B, T, rank=3)
    plain = [dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0), dict(direction=-1, turning=False, speed=25 / 3.6, offset=None)]
    # a kind-3 row the C-ABI meets without a table is stepped as kind 0: (route 1 = direction +1, end 1 = turning, s0 = x_turn)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    first = pkg.ScenarioLoop(eng, x0, [dict(kind="route", route=iroutes[2], speed=5.0)] + plain, max_age=RC.MAX_AGE, frame_window=20)
    first.run(K)
    assert eng.traffic_routes is not None
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    eng.di_ai.zero_()
    eng.status.zero_()
    again = pkg.ScenarioLoop(eng, torch.from_numpy(batch.x0).to(eng.device), plain, max_age=RC.MAX_AGE, frame_window=20, record=K)
    assert eng.traffic_routes is None
    eng2, x02 = loop_engine(pkg, iroutes, batch, T)
    fresh = pkg.ScenarioLoop(eng2, x02, plain, max_age=RC.MAX_AGE, frame_window=20, record=K)
    again.run(K)
    fresh.run(K)
    assert_same(records(again, 0, K), records(fresh, 0, K), "after clearing")
    assert_same(obstacle_state(again), obstacle_state(fresh), "after clearing")
    # without a table a kind-3 row falls through to kind 0
    param = torch.tensor([[1.0, 1.0, 5.0, 0.0, -10.0, 0.2, 3.0, 0.0], [1.0, 1.0, 5.0, 0.0, -10.0, 0.2, 0.0, 0.0]], dtype=torch.float64, device=eng.device)
    state = torch.tensor([[-30.0, -3.0, 0.0, 0.0]] * 2, dtype=torch.float64, device=eng.device)
    got, _ = device_ticks(eng, state, param, 30)
    assert np.array_equal(got[:, 0], got[:, 1]) and got[29, 0, 0] > -30.0


def test_refusals_keep_the_table(pkg, routes):
    eng = bare_engine(pkg, routes)
    lib, ctx = eng.lib, eng._ctx
    table = TR.case_routes()
    pkg.closed_loop._register_routes(eng, table)
    param = torch.from_numpy(TR.case_rows([TR.edge_cases()["s0_positive"]])).to(eng.device)

    def poses():
        state = torch.zeros(1, 4, dtype=torch.float64, device=eng.device)
        return device_ticks(eng, state, param, 6)[0]
    keep = poses()
    x, y, yaw, off = pkg.synth.pack_paths(table)
    off = off.astype(np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    bad_x, bad_yaw = x.copy(), yaw.copy()
    bad_x[5], bad_yaw[70] = np.nan, np.inf
    down, late = off.copy(), off.copy()
    down[3], late[0] = down[2] - 1, 1
    for args, msg in (((-1, x, y, yaw, off), "n_routes=-1"), ((6, None, y, yaw, off), "null array"), ((6, x, y, yaw, None), "null array"),
                      ((6, bad_x, y, yaw, off), "point 5 is not finite"), ((6, x, y, bad_yaw, off), "point 70 is not finite"),
                      ((6, x, y, yaw, down), "offsets decrease at route 2"), ((6, x, y, yaw, late), "off[0]=1")):
        rc = lib.jsim_loop_set_traffic_routes(ctx, args[0], *(dp(a) for a in args[1:]))
        assert rc == -22 and msg in lib.jsim_last_error(ctx).decode(), (msg, lib.jsim_last_error(ctx))
        assert np.array_equal(poses(), keep), msg                                       # the previous table is kept
    assert lib.jsim_loop_set_traffic_routes(None, 6, dp(x), dp(y), dp(yaw), dp(off)) == -22
    # a spec's bad route never reaches the device: the engine's table stays
    with pytest.raises(ValueError, match="not finite"):
        pkg.ScriptedObstacles(eng, [dict(kind="route", route=np.array([[0.0, 0.0], [np.nan, 1.0]]), speed=1.0)])
    assert np.array_equal(poses(), keep)
    assert lib.jsim_loop_set_traffic_routes(ctx, 0, None, None, None, None) == 0
