"""Interacting egos on the device (InteractingLoop / jsim_loop_run_interacting, jsim_loop_predict_egos): the reference's
interactive_mpc loop replayed tick by tick, singleton groups against ScenarioLoop, isolation of groups, the ego predictor
against the obstacle predictor, the glue at scale against the numpy oracle, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_helpers import W, assert_state_equal, iroutes, iter_totals, loop_engine, loop_state  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def LO(oracle):
    import loop_oracle
    return loop_oracle


def test_interacting_reference_loop_planned_and_driven_on_the_device(pkg):
    """tests/golden/loop_interact_T13.npz: interactive_mpc.py's two egos run by the reference's own code (planner, MPC under
    the recording cvxpy stand-in, prediction, collision check, plant; tests/golden/make_golden_loop_interact.py).  The routes
    are planned by jsim_plan_routes, then InteractingLoop is driven tick by tick: every recorded state, progress index, path
    length, collision flag, target_ind and status, and the controls to 1e-6.  Then the same ticks as one run(K) call."""
    g = load_golden("loop_interact_T13.npz")
    ticks = g["ticks"]
    K, n = ticks.shape[:2]
    PL = pkg.planner
    rad, _ = PL.car_circles()
    # Ego_instance(start_position, turn_indicator) -> intersection(turn_indicator=start_position, start_pos=turn_indicator)
    qs = [PL.intersection_query(int(tn), int(sp), rad) for sp, tn in g["egos"]]
    res = PL.plan_routes(qs, device=0)
    full = []
    for j, r in enumerate(res):
        assert r.status == 0 and r.trajectory.shape == g[f"planned{j}"].shape
        np.testing.assert_allclose(r.trajectory, g[f"planned{j}"], rtol=0, atol=1e-9)
        full.append(r.trajectory.copy())
    dl = float(g["dl"])

    def fresh():
        eng = pkg.BatchedMPC([f.copy() for f in full], list(range(n)), dl=dl, T=13)
        for j in range(n):
            np.testing.assert_allclose(eng.paths[j][:, 2], g[f"smoothed{j}"][:, 2], rtol=0, atol=1e-9)
        x0 = torch.tensor([[f[0, 0], f[0, 1], 0.0, eng.paths[j][0, 2]] for j, f in enumerate(full)], dtype=torch.float64,
                          device=eng.device)
        return eng, pkg.InteractingLoop(eng, x0, group_sizes=[n], hist_cap=K, max_age=0, frame_window=int(g["frame_window"]))

    eng, il = fresh()
    worst_pred = 0.0
    for k in range(K):
        np.testing.assert_allclose(il.loop.x0.cpu().numpy(), ticks[k][:, [0, 1, 3, 2]], rtol=0, atol=1e-6)
        worst_pred = max(worst_pred, float(np.abs(il.pred_egos().cpu().numpy() - g["preds"][k]).max()))
        il.tick()
        age = il.loop.age.cpu().numpy()
        for j in range(n):
            row = ticks[k, j]
            assert int(eng.path_len[j].item()) == int(row[7]) and int(eng.status[j].item()) == int(row[11]) == 0, (k, j)
            assert int(il.pre.col_flag[j].item()) == int(row[8]) and int(il.pre.status[j].item()) == 0, (k, j)
            if k + 1 < K:     # the device respawns at the end of the tick, the recording at the start of the next one
                assert (age[j] == 0) == bool(ticks[k + 1, j, 14]), (k, j)
            if age[j] != 0:
                assert int(eng.target_ind[j].item()) == int(row[10]) and int(il.pre.traj_idx[j].item()) == int(row[6]), (k, j)
    hist = il.loop.hist[:K].cpu().numpy()
    d_ctrl = max(np.abs(hist[..., 0] - ticks[..., 12]).max(), np.abs(hist[..., 1] - ticks[..., 13]).max())
    assert d_ctrl <= 1e-6, d_ctrl
    assert worst_pred <= 1e-6, worst_pred
    # respawns recorded at the start of ticks 1..K-1, plus those at the end of the last tick
    assert int(il.loop.n_respawn.item()) == int(ticks[1:, :, 14].sum()) + int((il.loop.age == 0).sum().item())
    eng2, il2 = fresh()
    il2.run(K)
    torch.cuda.synchronize()
    assert torch.equal(il2.loop.hist[:K], il.loop.hist[:K]) and torch.equal(il2.loop.x0, il.loop.x0)
    assert torch.equal(il2.pre.traj_idx, il.pre.traj_idx) and torch.equal(eng2.path_len, eng.path_len)
    print(f"interactive_mpc on the reference's routes: {K} ticks x {n} egos, {int(ticks[:, :, 8].sum())} cut by the other ego, "
          f"max control difference {d_ctrl:.2e}, max prediction difference {worst_pred:.2e}")


@pytest.mark.parametrize("with_obstacles", (False, True))
@pytest.mark.parametrize("T", (13, 20))
def test_singleton_groups_equal_the_scenario_loop(pkg, W, iroutes, T, with_obstacles):
    """Groups of one ego: bit-identical to ScenarioLoop.tick(), without scripted obstacles and with config 3's four."""
    batch, _ = W.interacting_batch(iroutes, 8, T, seed=3)
    specs = W.OBSTACLE_SPECS if with_obstacles else []
    K = 40
    eng_a, x0a = loop_engine(pkg, iroutes, batch, T)
    sc = pkg.ScenarioLoop(eng_a, x0a, specs, hist_cap=K, max_age=W.MAX_AGE, frame_window=20)
    eng_b, x0b = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng_b, x0b, group_sizes=[1] * eng_b.B, obstacle_specs=specs, hist_cap=K, max_age=W.MAX_AGE)
    n_cut = 0
    for _ in range(K):
        sc.tick()
        il.tick()
        assert_state_equal(loop_state(sc), loop_state(il), "singleton groups")
        n_cut += int(il.pre.col_flag.sum().item())
    assert torch.equal(sc.obst.state, il.obst.state)
    assert with_obstacles or n_cut == 0                         # a group of one has nothing to meet but scripted vehicles
    print(f"singleton groups, T = {T}, {len(specs)} scripted obstacles: {n_cut} ego-ticks with a cut-off")


def test_interacting_run_counts_every_tick_into_the_iteration_totals(pkg, W, iroutes):
    """jsim_loop_run_interacting runs separate launches per tick; jsim_mpc_iter_totals after run(K) is the per-tick n_iter of
    K x tick() added up, and both loops end bit-identical."""
    T, K = 13, 20
    batch, sizes = W.interacting_batch(iroutes, 6, T, seed=7)
    loops = []
    for _ in range(2):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        loops.append((eng, pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=W.OBSTACLE_SPECS[:2], hist_cap=K,
                                               max_age=W.MAX_AGE)))
    (e1, l1), (e2, l2) = loops
    iters = torch.zeros(e1.B, dtype=torch.int64, device=e1.device)
    for _ in range(K):
        l1.tick()
        iters += e1.n_iter
    l2.run(K)
    torch.cuda.synchronize()
    assert_state_equal(loop_state(l1), loop_state(l2), "run(K) against K ticks")
    assert np.array_equal(iter_totals(e2), iters.cpu().numpy()) and int(iters.sum()) > 0


def test_groups_are_isolated(pkg, W, iroutes):
    """Perturbing the spawn states of group 1 changes nothing in groups 0 and 2, bit for bit (and does change group 1)."""
    T, K = 13, 30
    batch, sizes = W.interacting_batch(iroutes, 3, T, seed=5)
    runs = []
    for perturb in (False, True):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        if perturb:
            x0[4:8, 2] += 0.5
            x0[4:8, 0] += 0.05
        il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, hist_cap=K, max_age=W.MAX_AGE)
        il.run(K)
        torch.cuda.synchronize()
        runs.append(loop_state(il))
    a, b = runs
    keep = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11], device=a["x0"].device)
    for key in a:
        dim = 1 if key == "hist" else 0
        assert torch.equal(a[key].index_select(dim, keep), b[key].index_select(dim, keep)), key
    assert not torch.equal(a["x0"][4:8], b["x0"][4:8])


def test_ego_prediction_equals_the_obstacle_prediction(pkg, W, iroutes):
    """jsim_loop_predict_egos on (x0, di_ai) == jsim_loop_predict_obstacles on the tuples (x, y, v, yaw, 0, delta), bit for bit."""
    batch, sizes = W.interacting_batch(iroutes, 6, 13, seed=7)
    eng, x0 = loop_engine(pkg, iroutes, batch, 13)
    il = pkg.InteractingLoop(eng, x0, group_sizes=sizes)
    rng = np.random.default_rng(2)
    eng.di_ai[:, 0] = torch.from_numpy(rng.uniform(-0.6, 0.6, eng.B)).to(eng.device)
    eng.di_ai[:, 1] = torch.from_numpy(rng.uniform(-3.0, 2.0, eng.B)).to(eng.device)   # ignored: a = 0
    x0[:, 2] = torch.from_numpy(rng.uniform(-1.0, 9.0, eng.B)).to(eng.device)
    x0[:, 3] += torch.from_numpy(rng.uniform(-4.0, 4.0, eng.B)).to(eng.device)
    pe = il.pred_egos()
    tup = torch.stack([x0[:, 0], x0[:, 1], x0[:, 2], x0[:, 3], torch.zeros_like(x0[:, 0]), eng.di_ai[:, 0]], dim=1).contiguous()
    for s in range(0, eng.B, 8):
        po = il.pre.predict(tup[s:s + 8].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(po, pe[s:s + 8]), s
    assert pe.shape == (eng.B, il.pre.n_steps, 3) and torch.isfinite(pe).all()


def test_interacting_glue_at_scale_against_the_oracle(pkg, W, iroutes, LO):
    """64 groups x 4 egos of the shared workload for 20 ticks: every tick, the device's tick-start states and steering fed to
    the numpy glue give the same path length, collision flag and progress index; most cuts come from group mates."""
    G, T, K = 64, 13, 20
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=11)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, max_age=W.MAX_AGE)
    B = eng.B
    dl = float(eng.dl)
    n_cut = 0
    for k in range(K):
        xs = il.loop.x0.cpu().numpy().copy()
        delta = eng.di_ai[:, 0].cpu().numpy().copy()
        idx_in = il.pre.traj_idx.cpu().numpy().copy()
        prev = il.pre.prev_len.cpu().numpy().copy()
        il.tick()
        plen, col = eng.path_len.cpu().numpy(), il.pre.col_flag.cpu().numpy()
        idx_out, st, age = il.pre.traj_idx.cpu().numpy(), il.pre.status.cpu().numpy(), il.loop.age.cpu().numpy()
        tup = [(xs[b, 0], xs[b, 1], xs[b, 2], xs[b, 3], 0.0, delta[b]) for b in range(B)]
        for b in range(B):
            g0 = 4 * (b // 4)
            obst = [tup[m] for m in range(g0, g0 + 4) if m != b]
            s, idx, path_len, c = LO.loop_pre_tick((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]),
                                                   None if prev[b] < 0 else int(prev[b]), iroutes[batch.path_id[b]], obst, dl,
                                                   frame_window=20)
            assert s == 0 and st[b] == 0, (k, b)
            assert path_len == int(plen[b]) and (c is not None) == bool(col[b]), (k, b)
            if age[b] != 0:
                assert idx == int(idx_out[b]), (k, b)
            n_cut += bool(col[b])
    print(f"{B} interacting egos x {K} ticks: {n_cut} ego-ticks cut by a group mate")
    assert n_cut >= B * K // 4


def test_interacting_refusals(pkg, W, iroutes):
    """-22 with a message: too many obstacles per ego, bad group_off, no groups for this B, speed_cutoff, obstacle geometry."""
    batch, sizes = W.interacting_batch(iroutes, 2, 13, seed=1)
    eng, x0 = loop_engine(pkg, iroutes, batch, 13)
    il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=W.OBSTACLE_SPECS[:2])
    lib, ctx = eng.lib, eng._ctx
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args()) == 0
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args(speed_cutoff=1)) == -22
    assert b"truncate" in lib.jsim_last_error(ctx)

    def groups(off):
        a = np.asarray(off, dtype=np.int32)
        return lib.jsim_loop_set_groups(ctx, eng.B, len(a) - 1, a.ctypes.data_as(ctypes.c_void_p))

    for bad in ([0, 9, 8], [0, 0, 8], [0, 4, 7], [1, 4, 8]):
        assert groups(bad) == -22, bad
    assert groups([0, 8]) == 0                                  # two obstacles + a group of 8: 2 + 7 > 8
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args()) == -22
    assert b"largest group" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_set_groups(ctx, eng.B, 0, None) == 0   # cleared
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args()) == -22
    assert groups([0, 4, 8]) == 0
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args()) == 0
    assert lib.jsim_loop_set_obstacle_geometry(ctx, 1.0, 0.0, 0.3, 1.0) == 0
    assert lib.jsim_loop_run_interacting(ctx, eng.B, 1, *il._run_args()) == -22
    assert b"obstacle" in lib.jsim_last_error(ctx)
    torch.cuda.synchronize()
