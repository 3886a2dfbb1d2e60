"""Interacting egos that share their MPC plans on the device (InteractingLoop(mate_prediction="plan"),
jsim_loop_set_mate_prediction, jsim_loop_predict_egos_plan): the predictor against the reference's rollouts and
the numpy restatement of the rule, the reference's interactive loop under the rule replayed tick by tick, the glue at scale against
the restatement and the oracle's glue, the constant mode and everything built on it unmoved, and the refusals."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_helpers import W, assert_state_equal, iroutes, loop_engine, loop_state  # noqa: F401
import mate_plan_numpy as MP
from mate_plan_numpy import plan_cases

pytestmark = pytest.mark.gpu

ATOL = 1e-9     # the project's bound for trajectories: 35-64 steps of a few ulp at |coordinate| <= 100 m stay near 1e-11


def _ptr(t):
    return None if t is None else t.data_ptr()


def predict_plan_device(eng, x0, oa, od, status, di_ai, n_steps, B=None):
    """jsim_loop_predict_egos_plan on host arrays: [B][n_steps][3]."""
    dev = eng.device
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev) for a, dt in
         ((x0, np.float64), (oa, np.float64), (od, np.float64), (status, np.int32), (di_ai, np.float64))]
    B = len(x0) if B is None else B
    pred = torch.full((B + 1, n_steps, 3), 777.0, dtype=torch.float64, device=dev)      # one guard row behind
    rc = eng.lib.jsim_loop_predict_egos_plan(eng._ctx, B, *map(_ptr, d), n_steps, _ptr(pred), eng._stream())
    assert rc == 0, eng.lib.jsim_last_error(eng._ctx)
    torch.cuda.synchronize()
    out = pred.cpu().numpy()
    assert np.all(out[B] == 777.0)
    return out[:B]


def restate(eng, x0, oa, od, status, di_ai, n_steps):
    """The restatement for every row, with the engine's plant constants."""
    c = eng.config
    return np.stack([MP.predict_plan(x0[b, 0], x0[b, 1], x0[b, 2], x0[b, 3], oa[b], od[b], int(status[b]), di_ai[b, 0], n_steps,
                                     dt=eng.dt, L=eng.L, max_steer=c.MAX_STEER_RAD, max_speed=c.MAX_SPEED, min_speed=c.MIN_SPEED)
                     for b in range(len(x0))])


def plan_loop(pkg, W, iroutes, G, T, seed, mode="plan", **kw):
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=seed)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    kw.setdefault("max_age", W.MAX_AGE)
    return batch, eng, pkg.InteractingLoop(eng, x0, group_sizes=kw.pop("group_sizes", sizes), mate_prediction=mode, **kw)


@pytest.mark.parametrize("T", (13, 20, 40))
def test_plan_predictor_on_the_reference_cases(pkg, W, iroutes, T):
    """Every case of tests/golden/mate_plan.npz with this horizon, stacked into one batch and predicted at every n_steps the fixture
    has (1, 35, 64): all rows against the restatement, and the rows whose own n_steps it is against the reference's rollout."""
    cs = [c for c in plan_cases() if c["T"] == T]
    assert cs
    _, eng, il = plan_loop(pkg, W, iroutes, 1, T, seed=1)          # (the loop registers the egos' geometry)
    x0 = np.stack([c["x0"] for c in cs])
    oa, od = np.stack([c["oa"] for c in cs]), np.stack([c["od"] for c in cs])
    status = np.array([c["status"] for c in cs])
    di_ai = np.stack([[c["delta_last"], -1.5] for c in cs])
    worst = 0.0
    for n in sorted({c["n_steps"] for c in plan_cases()}):
        got = predict_plan_device(eng, x0, oa, od, status, di_ai, n)
        want = restate(eng, x0, oa, od, status, di_ai, n)
        np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
        for k, c in enumerate(cs):
            if c["n_steps"] == n:
                np.testing.assert_allclose(got[k], c["pred"], rtol=0, atol=ATOL, err_msg=c["name"])
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"T = {T}: {len(cs)} reference cases, max difference to the restatement {worst:.2e}")


def test_plan_predictor_on_random_egos(pkg, W, iroutes):
    """130 egos with states and last steering drawn as test_ego_prediction_equals_the_obstacle_prediction draws them, plans with
    steering beyond +-MAX_STEER and accelerations that reach both speed clamps, a quarter of them with a failed status; through
    pred_egos() (the loop's own buffers) and through the entry point."""
    batch, eng, il = plan_loop(pkg, W, iroutes, 33, 13, seed=7)
    B = 130
    rng = np.random.default_rng(2)
    x0 = il.loop.x0
    eng.di_ai[:, 0] = torch.from_numpy(rng.uniform(-0.6, 0.6, eng.B)).to(eng.device)
    eng.di_ai[:, 1] = torch.from_numpy(rng.uniform(-3.0, 2.0, eng.B)).to(eng.device)
    x0[:, 2] = torch.from_numpy(rng.uniform(-1.0, 9.0, eng.B)).to(eng.device)
    x0[:, 3] += torch.from_numpy(rng.uniform(-4.0, 4.0, eng.B)).to(eng.device)
    eng.oa.copy_(torch.from_numpy(rng.uniform(-3.0, 2.0, (eng.B, 13))))
    eng.od.copy_(torch.from_numpy(rng.uniform(-1.0, 1.0, (eng.B, 13))))
    eng.status.copy_(torch.from_numpy(rng.choice([0, 0, 0, 1, 2, 4], eng.B).astype(np.int32)))
    h = [t.cpu().numpy().copy() for t in (x0, eng.oa, eng.od, eng.status, eng.di_ai)]
    assert (h[3] != 0).sum() >= 20 and (np.abs(h[2]) > eng.config.MAX_STEER_RAD).any()
    n = il.pre.n_steps
    want = restate(eng, *h, n)
    pe = il.pred_egos()
    torch.cuda.synchronize()
    assert pe.shape == (eng.B, n, 3)
    np.testing.assert_allclose(pe.cpu().numpy(), want, rtol=0, atol=ATOL)
    got = predict_plan_device(eng, *h, n, B=B)
    np.testing.assert_allclose(got, want[:B], rtol=0, atol=ATOL)
    assert np.array_equal(got, pe.cpu().numpy()[:B])                 # the same kernel on the same rows
    print(f"{B} random egos: max difference to the restatement {np.abs(got - want[:B]).max():.2e}")


def test_plan_sharing_reference_loop_planned_and_driven_on_the_device(pkg):
    """tests/golden/loop_interact_plan_T13.npz: interactive_mpc.py's two egos run by the reference's own code with each ego predicted
    from its controller's plan (tests/golden/make_golden_loop_interact_plan.py).  What
    test_interacting_reference_loop_planned_and_driven_on_the_device asserts, under mate_prediction="plan": routes planned by
    jsim_plan_routes, every recorded state, progress index, path length, collision flag, target_ind and status, the controls and
    pred_egos() to 1e-6; then the same ticks as one run(K) call, bit-identical."""
    g = load_golden("loop_interact_plan_T13.npz")
    ticks = g["ticks"]
    K, n = ticks.shape[:2]
    PL = pkg.planner
    rad, _ = PL.car_circles()
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
        return eng, pkg.InteractingLoop(eng, x0, group_sizes=[n], hist_cap=K, max_age=0, frame_window=int(g["frame_window"]),
                                        mate_prediction="plan")

    eng, il = fresh()
    worst_pred = worst_plan = 0.0
    for k in range(K):
        np.testing.assert_allclose(il.loop.x0.cpu().numpy(), ticks[k][:, [0, 1, 3, 2]], rtol=0, atol=1e-6)
        worst_pred = max(worst_pred, float(np.abs(il.pred_egos().cpu().numpy() - g["preds"][k]).max()))
        worst_plan = max(worst_plan, float(np.abs(eng.oa.cpu().numpy() - g["plan_oa"][k]).max()),
                         float(np.abs(eng.od.cpu().numpy() - g["plan_od"][k]).max()))
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
    assert int(il.loop.n_respawn.item()) == int(ticks[1:, :, 14].sum()) + int((il.loop.age == 0).sum().item())
    eng2, il2 = fresh()
    il2.run(K)
    torch.cuda.synchronize()
    assert torch.equal(il2.loop.hist[:K], il.loop.hist[:K]) and torch.equal(il2.loop.x0, il.loop.x0)
    assert torch.equal(il2.pre.traj_idx, il.pre.traj_idx) and torch.equal(eng2.path_len, eng.path_len)
    assert_state_equal(loop_state(il), loop_state(il2), "run(K) against K ticks")
    print(f"interactive_mpc under the plan rule: {K} ticks x {n} egos, {int(ticks[:, :, 8].sum())} cut by the other ego, "
          f"max control difference {d_ctrl:.2e}, max prediction difference {worst_pred:.2e}, max plan difference {worst_plan:.2e}")


def test_plan_glue_at_scale_against_the_restatement_and_the_oracle(pkg, W, iroutes):
    """16 groups x 4 egos, T = 13, 20 ticks, egos re-entering after 8 ticks from staggered ages: every tick the device's tick-start
    x0, oa, od, status, di_ai go through the restatement and the oracle's glue, which must give the device's path length,
    collision flag and progress index.  The same batch under "constant" cuts at least one ego-tick elsewhere."""
    G, T, K, MAX_AGE = 16, 13, 20, 8
    ages = np.random.default_rng(5).integers(0, MAX_AGE - 1, 4 * G).astype(np.int32)
    plens = {}
    for mode in ("plan", "constant"):
        batch, eng, il = plan_loop(pkg, W, iroutes, G, T, seed=11, mode=mode, max_age=MAX_AGE)
        il.loop.age.copy_(torch.from_numpy(ages))
        B, dl = eng.B, float(eng.dl)
        n_cut, rows = 0, []
        for k in range(K):
            xs, oa, od, st_in, di_ai = (t.cpu().numpy().copy() for t in (il.loop.x0, eng.oa, eng.od, eng.status, eng.di_ai))
            idx_in = il.pre.traj_idx.cpu().numpy().copy()
            prev = il.pre.prev_len.cpu().numpy().copy()
            il.tick()
            plen, col = eng.path_len.cpu().numpy().copy(), il.pre.col_flag.cpu().numpy()
            rows.append(plen)
            n_cut += int(col.sum())
            if mode != "plan":
                continue
            idx_out, st, age = il.pre.traj_idx.cpu().numpy(), il.pre.status.cpu().numpy(), il.loop.age.cpu().numpy()
            preds = restate(eng, xs, oa, od, st_in, di_ai, il.pre.n_steps)
            for b in range(B):
                g0 = 4 * (b // 4)
                s, idx, path_len, c = MP.pre_tick((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]),
                                                  None if prev[b] < 0 else int(prev[b]), iroutes[batch.path_id[b]],
                                                  [preds[m] for m in range(g0, g0 + 4) if m != b], dl, L=eng.L, dt=eng.dt,
                                                  frame_window=20)
                assert s == 0 and st[b] == 0, (k, b)
                assert path_len == int(plen[b]) and (c is not None) == bool(col[b]), (k, b)
                if age[b] != 0:
                    assert idx == int(idx_out[b]), (k, b)
        plens[mode] = np.stack(rows)
        n_resp = int(il.loop.n_respawn.item())
        assert n_resp >= B, n_resp                                  # every ego re-entered at least once
        print(f"{mode}: {B} egos x {K} ticks, {n_cut} ego-ticks cut by a group mate, {n_resp} respawns")
        assert n_cut > 0
    n_diff = int((plens["plan"] != plens["constant"]).sum())
    assert n_diff >= 1
    print(f"ego-ticks whose path length differs between the two modes: {n_diff}")


def test_constant_mode_is_the_default_and_survives_a_plan_loop(pkg, W, iroutes):
    """mate_prediction="constant" equals the default bit for bit (loop_state after 30 ticks), and so does a constant loop built
    on an engine that a plan loop has run on."""
    T, K = 13, 30
    batch, sizes = W.interacting_batch(iroutes, 6, T, seed=7)

    def run(eng, x0, **kw):
        il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=W.OBSTACLE_SPECS[:2], hist_cap=K, max_age=W.MAX_AGE, **kw)
        il.run(K)
        torch.cuda.synchronize()
        return il

    eng_a, x0_a = loop_engine(pkg, iroutes, batch, T)
    default = loop_state(run(eng_a, x0_a))
    eng_b, x0_b = loop_engine(pkg, iroutes, batch, T)
    assert_state_equal(default, loop_state(run(eng_b, x0_b, mate_prediction="constant")), "constant against the default")
    eng_c, x0_c = loop_engine(pkg, iroutes, batch, T)
    plan = loop_state(run(eng_c, x0_c.clone(), mate_prediction="plan"))
    assert not torch.equal(plan["hist"], default["hist"])            # (the plan loop did run as one)
    # the engine back to its start, then a constant loop on it
    eng_c.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    for t in (eng_c.status, eng_c.di_ai, eng_c.ox, eng_c.oy, eng_c.ov, eng_c.oyaw):
        t.zero_()
    assert_state_equal(default, loop_state(run(eng_c, x0_c.clone())), "a constant loop after a plan loop on one engine")


def test_singleton_groups_in_plan_mode_equal_the_scenario_loop(pkg, W, iroutes):
    """A group of one has no mates: bit-identical to ScenarioLoop.tick(), with config 3's scripted obstacles."""
    T, K = 13, 25
    batch, _ = W.interacting_batch(iroutes, 8, T, seed=3)
    eng_a, x0a = loop_engine(pkg, iroutes, batch, T)
    sc = pkg.ScenarioLoop(eng_a, x0a, W.OBSTACLE_SPECS, hist_cap=K, max_age=W.MAX_AGE, frame_window=20)
    eng_b, x0b = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng_b, x0b, group_sizes=[1] * eng_b.B, obstacle_specs=W.OBSTACLE_SPECS, hist_cap=K, max_age=W.MAX_AGE,
                             mate_prediction="plan")
    for _ in range(K):
        sc.tick()
        il.tick()
        assert_state_equal(loop_state(sc), loop_state(il), "singleton groups, plan mode")
    assert torch.equal(sc.obst.state, il.obst.state)


def test_groups_are_isolated_in_plan_mode(pkg, W, iroutes):
    """test_groups_are_isolated's scheme: perturbing the spawn states of group 1 changes nothing in groups 0 and 2, bit for bit
    (and does change group 1)."""
    T, K = 13, 30
    batch, sizes = W.interacting_batch(iroutes, 3, T, seed=5)
    runs = []
    for perturb in (False, True):
        eng, x0 = loop_engine(pkg, iroutes, batch, T)
        if perturb:
            x0[4:8, 2] += 0.5
            x0[4:8, 0] += 0.05
        il = pkg.InteractingLoop(eng, x0, group_sizes=sizes, hist_cap=K, max_age=W.MAX_AGE, mate_prediction="plan")
        il.run(K)
        torch.cuda.synchronize()
        runs.append(loop_state(il))
    a, b = runs
    keep = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11], device=a["x0"].device)
    for key in a:
        dim = 1 if key == "hist" else 0
        assert torch.equal(a[key].index_select(dim, keep), b[key].index_select(dim, keep)), key
    assert not torch.equal(a["x0"][4:8], b["x0"][4:8])


def test_mate_prediction_refusals(pkg, W, iroutes):
    """-22 with a message: a mode other than 0 / 1 (the mode stays: the loop goes on as a plan loop), n_steps outside 1..64, a
    negative B, a null pointer; Recorder.cutoffs() refuses a plan-mode recording and serves a constant one."""
    K = 10
    loops = [plan_loop(pkg, W, iroutes, 4, 13, seed=9, record=K) for _ in range(2)]
    (_, eng, il), (_, eng2, il2) = loops
    lib, ctx = eng.lib, eng._ctx
    for bad in (2, -1, 7):
        assert lib.jsim_loop_set_mate_prediction(ctx, bad) == -22
        assert f"mode={bad}".encode() in lib.jsim_last_error(ctx)
    il.run(K)
    il2.run(K)
    torch.cuda.synchronize()
    assert_state_equal(loop_state(il), loop_state(il2), "a refused mode leaves the plan mode in place")
    _, eng3, il3 = plan_loop(pkg, W, iroutes, 4, 13, seed=9, mode="constant", record=K)
    il3.run(K)
    torch.cuda.synchronize()
    assert not torch.equal(il3.loop.x0, il.loop.x0)
    # the predictor's checks
    args = [_ptr(t) for t in (il.loop.x0, eng.oa, eng.od, eng.status, eng.di_ai)]
    for n_steps in (0, -3, 65, 1000):
        assert lib.jsim_loop_predict_egos_plan(ctx, eng.B, *args, n_steps, None, eng._stream()) == -22
        assert f"n_steps={n_steps}".encode() in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_predict_egos_plan(ctx, -1, *args, 35, None, eng._stream()) == -22
    for hole in range(5):
        holed = [None if i == hole else a for i, a in enumerate(args)]
        assert lib.jsim_loop_predict_egos_plan(ctx, eng.B, *holed, 35, None, eng._stream()) == -22
        assert b"null device pointer" in lib.jsim_last_error(ctx)
    assert lib.jsim_loop_predict_egos_plan(ctx, 0, *([None] * 5), 35, None, eng._stream()) == 0       # nothing to do
    for n_steps in (1, 64):
        assert lib.jsim_loop_predict_egos_plan(ctx, eng.B, *args, n_steps, None, eng._stream()) == 0  # pred may be NULL
    torch.cuda.synchronize()
    # the cut-off replay
    assert il.recorder.glue["mate_prediction"] == "plan" and il3.recorder.glue["mate_prediction"] == "constant"
    with pytest.raises(ValueError, match="plan"):
        il.recorder.cutoffs()
    out = il3.recorder.cutoffs()
    assert out["cut"].shape == (K, eng3.B)
