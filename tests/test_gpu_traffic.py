"""Traffic sets on the device (ScenarioLoop / InteractingLoop traffic_of, jsim_loop_set_traffic): every ego of a batch with
its own scripted vehicles equals that ego run in a plain loop whose shared obstacles are its set, bit for bit -- on the fused
one-wave (T = 13, 20) and four-wave (T = 40) kernels and on host ticks (T = 24), with both glues; the shared-traffic special
case, chunked fused launches, run(K) against K ticks, per-group sets of interacting egos, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_helpers import W, assert_state_equal, iroutes, loop_engine, loop_state, obstacle_state, sub_batch  # noqa: F401

pytestmark = pytest.mark.gpu

T_INT = lambda d, turn, kmh, off: dict(direction=d, turning=turn, speed=kmh / 3.6, offset=off)     # noqa: E731
ROUND = lambda d, off: dict(kind="roundabout", direction=d, turning=True, speed=25 / 3.6, offset=off)   # noqa: E731
# two t-intersection sets (mpc_intersection.py's offsets 2 / 4, mpc_intersection_new_ref.py's 1), a roundabout set
# (mpc_roundabout.py:49-50), a set of 8 and an empty set
SETS = [[T_INT(1, False, 25, 2.0), T_INT(-1, True, 20, 4.0)],
        [T_INT(-1, False, 30, 1.0), T_INT(1, True, 22, 0.5), T_INT(1, False, 28, 3.0)],
        [ROUND(1, 1.0), ROUND(-1, 4.0)],
        [T_INT(1, False, 25, None), T_INT(-1, True, 20, 6.0), T_INT(1, True, 15, 12.0), T_INT(-1, False, 25, 3.0),
         T_INT(1, False, 30, 1.5), T_INT(-1, True, 24, 2.5), T_INT(-1, False, 21, 0.5), T_INT(1, True, 27, 4.5)],
        []]


@pytest.mark.parametrize("mode", ("truncate", "speed_cutoff"))
@pytest.mark.parametrize("T", (13, 20, 24, 40))
def test_per_ego_sets_equal_plain_loops_per_set(pkg, W, iroutes, T, mode):
    """64 egos over the intersection routes, five sets (two t-intersection, roundabout, eight vehicles, empty), 60 ticks: each
    set's egos equal a plain ScenarioLoop of just those egos with that set shared, bit for bit -- every loop buffer, the history
    and the obstacle states; the respawn counts add up; every non-empty set cuts some ego-ticks."""
    B, K = 64, 60
    batch = W.ego_batch(iroutes, B, T, rank=3)
    traffic_of = np.arange(B) % len(SETS)
    eng, x0 = loop_engine(pkg, iroutes, batch, T, mode)
    sc = pkg.ScenarioLoop(eng, x0, SETS, hist_cap=K, max_age=W.MAX_AGE, frame_window=20, mode=mode, traffic_of=traffic_of)
    plain = []
    for s, specs in enumerate(SETS):
        sub = sub_batch(batch, np.flatnonzero(traffic_of == s))
        e, x = loop_engine(pkg, iroutes, sub, T, mode)
        plain.append(pkg.ScenarioLoop(e, x, specs, hist_cap=K, max_age=W.MAX_AGE, frame_window=20, mode=mode))
    cuts = np.zeros(len(SETS), dtype=np.int64)
    tof = torch.from_numpy(traffic_of).to(eng.device)
    for _ in range(K):
        sc.tick()
        for p in plain:
            p.run(1)                  # the same launches as sc.tick() with a layout: fused, or host ticks at T = 24
        col = sc.pre.col_flag
        for s in range(len(SETS)):
            cuts[s] += int(col[tof == s].sum().item())
    torch.cuda.synchronize()
    _, obs_off = sc.traffic
    for s, p in enumerate(plain):
        idx = torch.from_numpy(np.flatnonzero(traffic_of == s)).to(eng.device)
        assert_state_equal(loop_state(sc, idx), loop_state(p), s)
        assert_state_equal(obstacle_state(sc, obs_off[s], obs_off[s + 1]), obstacle_state(p), s)
    assert int(sc.loop.n_respawn.item()) == sum(int(p.loop.n_respawn.item()) for p in plain)
    print(f"T = {T}, {mode}: cut ego-ticks per set {cuts.tolist()}, respawns {int(sc.loop.n_respawn.item())}")
    assert cuts[-1] == 0 and (cuts[:-1] > 0).all(), cuts


@pytest.mark.parametrize("T", (13, 24))
def test_one_set_for_everyone_equals_shared_obstacles(pkg, W, iroutes, T):
    """A layout with one set holding config 3's four vehicles equals today's shared-obstacle call bit for bit."""
    B, K = 48, 40
    batch = W.ego_batch(iroutes, B, T, rank=1)
    runs = []
    for traffic in (False, True):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        kw = dict(traffic_of=np.zeros(B, dtype=np.int64)) if traffic else {}
        sc = pkg.ScenarioLoop(eng, x0, [W.OBSTACLE_SPECS] if traffic else W.OBSTACLE_SPECS, hist_cap=K, max_age=W.MAX_AGE, **kw)
        sc.run(K)
        torch.cuda.synchronize()
        runs.append((loop_state(sc), obstacle_state(sc), int(sc.loop.n_respawn.item())))
    assert_state_equal(runs[0][0], runs[1][0], "shared")
    assert_state_equal(runs[0][1], runs[1][1], "shared")
    assert runs[0][2] == runs[1][2]


def test_chunked_equals_unchunked_and_run_equals_ticks(pkg, W, iroutes):
    """T = 30 (config 3's horizon) over traffic_batch sets: chunk_ticks = 7 equals the automatic chunk over 50 ticks, and
    run(50) equals 50 x tick(), bit for bit."""
    T, B, K = 30, 96, 50
    batch = W.ego_batch(iroutes, B, T, rank=2)
    sets, tof = W.traffic_batch(B, seed=5, n_sets=12)
    runs = []
    for how in ("auto", "chunk7", "ticks"):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        sc = pkg.ScenarioLoop(eng, x0, sets, hist_cap=K, max_age=W.MAX_AGE, traffic_of=tof, chunk_ticks=7 if how == "chunk7" else 0)
        if how == "ticks":
            for _ in range(K):
                sc.tick()
        else:
            sc.run(K)
        torch.cuda.synchronize()
        runs.append((loop_state(sc), obstacle_state(sc), int(sc.loop.n_respawn.item())))
    for r in runs[1:]:
        assert_state_equal(runs[0][0], r[0], "chunks")
        assert_state_equal(runs[0][1], r[1], "chunks")
        assert runs[0][2] == r[2]


def test_per_group_sets_equal_groups_run_alone(pkg, W, iroutes):
    """Interacting egos, groups of four (workloads.interacting_batch) with per-group sets: each group equals that group run alone
    as an InteractingLoop with its set shared, bit for bit."""
    T, G, K = 13, 10, 30
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=13)
    sets = [s[:4] for s in SETS] + [[T_INT(1, True, 26, 1.0)]]       # + 3 group mates <= 8
    tog = np.arange(G) % len(sets)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=sets, hist_cap=K, max_age=W.MAX_AGE, traffic_of=tog)
    il.run(K)
    torch.cuda.synchronize()
    n_cut = 0
    for g in range(G):
        idx = np.arange(4 * g, 4 * g + 4)
        e, x = loop_engine(pkg, iroutes, sub_batch(batch, idx), T)
        alone = pkg.InteractingLoop(e, x, group_sizes=[4], obstacle_specs=sets[tog[g]], hist_cap=K, max_age=W.MAX_AGE)
        alone.run(K)
        torch.cuda.synchronize()
        assert_state_equal(loop_state(il, torch.from_numpy(idx).to(eng.device)), loop_state(alone), g)
        o0, o1 = il.traffic[1][tog[g]], il.traffic[1][tog[g] + 1]
        assert torch.equal(il.obst.state[o0:o1], alone.obst.state[: alone.obst.n]), g
        n_cut += int(alone.pre.col_flag.sum().item())
    print(f"{G} groups with their own traffic: {n_cut} egos cut at the last tick")


def test_interacting_glue_with_per_group_sets_against_the_oracle(pkg, W, iroutes, oracle):
    """256 egos in groups of four, each group with its own traffic_batch set of t-intersection vehicles, 12 ticks: every tick
    the device's glue equals oracle/loop_oracle.py fed the tick-start states, the group's scripted vehicles (their get()
    tuples of the tick, left in obs_get) and then the group mates."""
    import loop_oracle as LO
    G, T, K = 64, 13, 12
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=17)
    sets, tog = W.traffic_batch(G, seed=3, vehicles=2, roundabout=0.0)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=sets, max_age=W.MAX_AGE, traffic_of=tog)
    set_of, obs_off = il.traffic
    B, dl = eng.B, float(eng.dl)
    n_cut = n_scripted = 0
    for k in range(K):
        xs = il.loop.x0.cpu().numpy().copy()
        delta = eng.di_ai[:, 0].cpu().numpy().copy()
        idx_in = il.pre.traj_idx.cpu().numpy().copy()
        prev = il.pre.prev_len.cpu().numpy().copy()
        il.tick()
        get = il.obst.get_buf[: il.obst.n].cpu().numpy()       # this tick's get() (t-intersection vehicles: both calls agree)
        plen, col = eng.path_len.cpu().numpy(), il.pre.col_flag.cpu().numpy()
        idx_out, st, age = il.pre.traj_idx.cpu().numpy(), il.pre.status.cpu().numpy(), il.loop.age.cpu().numpy()
        tup = [(xs[b, 0], xs[b, 1], xs[b, 2], xs[b, 3], 0.0, delta[b]) for b in range(B)]
        for b in range(B):
            g0 = 4 * (b // 4)
            s = set_of[b]
            scripted = [tuple(r) for r in get[obs_off[s]:obs_off[s + 1]]]
            obst = scripted + [tup[m] for m in range(g0, g0 + 4) if m != b]
            r = LO.loop_pre_tick((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]), None if prev[b] < 0 else int(prev[b]),
                                 iroutes[batch.path_id[b]], obst, dl, frame_window=20)
            assert r[0] == 0 and st[b] == 0, (k, b)
            assert r[2] == int(plen[b]) and (r[3] is not None) == bool(col[b]), (k, b)
            if age[b] != 0:
                assert r[1] == int(idx_out[b]), (k, b)
            n_cut += bool(col[b])
            n_scripted += len(scripted)
    print(f"{B} interacting egos with per-group traffic x {K} ticks: {n_cut} ego-ticks cut")
    assert n_cut > 0 and n_scripted > 0


def test_traffic_refusals_leave_the_buffers_alone(pkg, W, iroutes):
    """-22 with a message for every bad layout (set_of out of range, obs_off not from 0 / decreasing, a set of 9), a run with
    another B or total, and interacting groups with mixed sets or too many vehicles per group -- and nothing on the device
    changes: the registered layout stays, the loop buffers and obstacle states keep their values."""
    T = 13
    batch, sizes = W.interacting_batch(iroutes, 2, T, seed=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    B = eng.B
    sets = [SETS[0], SETS[2]]
    sc = pkg.ScenarioLoop(eng, x0, sets, hist_cap=4, traffic_of=np.array([0, 1] * (B // 2)))
    lib, ctx = eng.lib, eng._ctx
    p = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    torch.cuda.synchronize()
    before = (loop_state(sc), obstacle_state(sc))

    def unchanged():
        torch.cuda.synchronize()
        assert_state_equal(before[0], loop_state(sc), "refusal")
        assert_state_equal(before[1], obstacle_state(sc), "refusal")

    good_of, good_off = np.zeros(B), [0, 2, 4]
    for of, off, msg in (([0] * (B - 1) + [2], good_off, b"set_of"), ([0] * (B - 1) + [-1], good_off, b"set_of"),
                         (good_of, [1, 2, 4], b"start at 0"), (good_of, [0, 3, 2], b"decreases"),
                         (good_of, [0, 2, 11], b"9 vehicles")):
        assert lib.jsim_loop_set_traffic(ctx, B, len(off) - 1, p(of), p(off), 0) == -22, msg
        assert msg in lib.jsim_last_error(ctx), lib.jsim_last_error(ctx)
    assert lib.jsim_loop_set_traffic(ctx, B, 2, None, p(good_off), 0) == -22
    assert lib.jsim_loop_set_traffic(ctx, B, 2, p(good_of), p(good_off), -1) == -22
    # the registered layout is still the good one: a run with the right total works after all these
    assert lib.jsim_loop_run_scenario(ctx, B, 3, *sc._run_args(n_obs=3)) == -22        # wrong total
    assert b"4 vehicles" in lib.jsim_last_error(ctx)
    unchanged()
    assert lib.jsim_loop_run_scenario(ctx, B - 4, 3, *sc._run_args()) == -22 and b"B=" in lib.jsim_last_error(ctx)   # wrong B
    unchanged()
    # interacting: a group mixing sets; a set of 6 + 3 group mates
    assert lib.jsim_loop_set_groups(ctx, B, 2, p([0, 4, 8])) == 0
    assert lib.jsim_loop_run_interacting(ctx, B, 3, *sc._run_args()) == -22
    assert b"mixes traffic sets" in lib.jsim_last_error(ctx)
    unchanged()
    big = [[T_INT(1, False, 25, 1.0 + i) for i in range(6)], []]
    assert lib.jsim_loop_set_traffic(ctx, B, 2, p([0] * 4 + [1] * 4), p([0, 6, 6]), 0) == 0
    args = list(sc._run_args(n_obs=6))
    obs6 = pkg.ScriptedObstacles(eng, big[0])
    args[-6], args[-5], args[-4] = (t.data_ptr() for t in (obs6.state, obs6.param, obs6.get_buf))
    assert lib.jsim_loop_run_interacting(ctx, B, 3, *args) == -22
    assert b"group mates" in lib.jsim_last_error(ctx)
    unchanged()
    assert lib.jsim_loop_set_traffic(ctx, B, 2, p([1] * 4 + [0] * 4), p([0, 2, 4]), 0) == 0   # per-group sets: accepted
    assert lib.jsim_loop_run_interacting(ctx, B, 3, *sc._run_args()) == 0
    assert lib.jsim_loop_set_traffic(ctx, B, 0, None, None, 0) == 0                   # cleared: n_obs <= 8 again
    assert lib.jsim_loop_set_groups(ctx, B, 0, None) == 0
    torch.cuda.synchronize()
