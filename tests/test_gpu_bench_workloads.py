"""Parity ON THE BENCHMARK'S OWN WORKLOADS: the egos, routes and loop objects come from the same
`workloads.py` functions bench.py times -- GPU-planned routes (12 intersection / 48 two-lane), `ego_batch(..., rank=0)` = seed 1,
whole routes, config 3's four scripted obstacle vehicles -- not from the synthetic arcs the other GPU tests use.

  config 2 (256 x T=20)   every ego against the oracle, first step and 30 closed-loop ticks with the oracle fed the device's inputs
  config 5 (1024 x T=40)  every ego against the oracle on the 48 planned two-lane routes, first step and 8 inputs-fed ticks
  config 4 (4096 x T=20)  KKT on all 4096, a 512-ego slice against the oracle; 10 inputs-fed ticks on the slice
  config 3 (4096 x T=30)  the scenario loop for 12 ticks: every tick the loop glue (progress index, cut-off, collision flag)
                          against oracle/loop_oracle.py for a 384-ego slice and bit-exact; the MPC step of ALL egos against
                          the oracle on the device's inputs (cut-off paths included); then fused == tick by tick
  bench.py's JSON fields  straggler / iters_source / other_respawn_rule / kernel name, from a short real run
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from gpu_helpers import debug_bufs, kkt_check

pytestmark = pytest.mark.gpu
U_TOL = 1e-4


@pytest.fixture(scope="module")
def planned(pkg):
    WL = pkg.workloads
    return {ml: WL.route_table(ml, source="planner", device_index=0)[0] for ml in (False, True)}


def _oracle_step(oracle, pkg, routes, T, x0, path_id, path_len, speed, tind, oa, od, n_threads=16):
    p = oracle.make_params(T=T)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    return oracle.mpc_step_batch(p, np.ascontiguousarray(x0), path_id, path_len, speed, cx, cy, cyaw, off, tind, oa, od,
                                 n_threads=n_threads)


def _compare(eng, ref, sl=slice(None), tol=1e-7):
    st = eng.status.cpu().numpy()[sl]
    assert np.array_equal(st, ref["status"])
    use = ref["status"] != 2
    assert np.array_equal(eng.target_ind.cpu().numpy()[sl][use], ref["target_ind"][use])
    ok = st == 0
    np.testing.assert_array_equal(eng.xref.cpu().numpy()[sl][ok], ref["xref"][ok])
    err = max(np.abs(eng.oa.cpu().numpy()[sl] - ref["oa"])[ok].max(initial=0.0), np.abs(eng.od.cpu().numpy()[sl] - ref["od"])[ok].max(initial=0.0))
    assert err <= tol, err
    assert np.array_equal(eng.active_mask.cpu().numpy().view(np.uint32)[sl][ok], ref["active_mask"][ok])
    return err


def _inputs_fed_ticks(oracle, pkg, routes, eng, loop, batch, T, K, sl=slice(None), tol=1e-7):
    """K closed-loop ticks driven one by one; before every tick the device's inputs (state, remembered index, warm start, path
    length) are read back and given to the oracle, after the solve the outputs are compared.  Returns the worst |du|."""
    worst = 0.0
    for _ in range(K):
        x0 = loop.x0.cpu().numpy()[sl].copy()
        tind = eng.target_ind.cpu().numpy()[sl].copy(); oa = eng.oa.cpu().numpy()[sl].copy(); od = eng.od.cpu().numpy()[sl].copy()
        plen = eng.path_len.cpu().numpy()[sl].copy()
        ref = _oracle_step(oracle, pkg, routes, T, x0, batch.path_id[sl], plen, batch.speed[sl], tind, oa, od)
        eng.solve(loop.x0)                       # loop.tick() = this solve + the advance below
        torch.cuda.synchronize()
        worst = max(worst, _compare(eng, ref, sl, tol))
        pkg._cabi.check(eng.lib.jsim_loop_advance(eng._ctx, eng.B, *loop._advance_args()), eng._ctx, "jsim_loop_advance")
    return worst


def test_config2_headline_workload_every_ego_vs_oracle(pkg, oracle, planned):
    WL = pkg.workloads
    c = WL.CONFIGS[2]
    B, T = c["batch"], c["horizon"]
    routes = planned[False]
    assert len(routes) == 12
    batch = WL.ego_batch(routes, B, T, rank=0)
    eng, x0 = WL.make_engine(routes, batch, T, "cuda:0")
    dbg = debug_bufs(eng)
    eng.solve(x0, debug=dbg)
    torch.cuda.synchronize()
    kkt_check(eng, batch, dbg)
    ref = _oracle_step(oracle, pkg, routes, T, batch.x0, batch.path_id, batch.path_len, batch.speed, batch.target_ind, batch.oa, batch.od)
    e0 = _compare(eng, ref)
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    sc, loop = WL.make_loop(2, eng, x0, hist_cap=64, routes=routes, batch=batch)
    e1 = _inputs_fed_ticks(oracle, pkg, routes, eng, loop, batch, T, 30)
    print(f"config 2 on the bench's planned routes: first step max|du|={e0:.2e}; 30 inputs-fed closed-loop ticks max|du|={e1:.2e}, "
          f"respawns {int(loop.n_respawn.item())}")


def test_config5_share_on_planned_two_lane_routes_every_ego_vs_oracle(pkg, oracle, planned):
    WL = pkg.workloads
    c = WL.CONFIGS[5]
    B, T = c["batch"], c["horizon"]
    routes = planned[True]
    assert len(routes) == 48
    batch = WL.ego_batch(routes, B, T, rank=0)
    assert len(np.unique(batch.path_id)) >= 40
    eng, x0 = WL.make_engine(routes, batch, T, "cuda:0")
    dbg = debug_bufs(eng)
    eng.solve(x0, debug=dbg)
    torch.cuda.synchronize()
    kkt_check(eng, batch, dbg)
    ref = _oracle_step(oracle, pkg, routes, T, batch.x0, batch.path_id, batch.path_len, batch.speed, batch.target_ind, batch.oa, batch.od)
    e0 = _compare(eng, ref, tol=1e-6)
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    sc, loop = WL.make_loop(5, eng, x0, hist_cap=16, routes=routes, batch=batch)
    e1 = _inputs_fed_ticks(oracle, pkg, routes, eng, loop, batch, T, 8, tol=1e-6)
    print(f"config 5 share on the 48 planned two-lane routes: first step max|du|={e0:.2e}; 8 inputs-fed ticks max|du|={e1:.2e}")


def test_config4_share_on_planned_routes(pkg, oracle, planned):
    WL = pkg.workloads
    c = WL.CONFIGS[4]
    B, T = c["batch"], c["horizon"]
    routes = planned[False]
    batch = WL.ego_batch(routes, B, T, rank=0)
    eng, x0 = WL.make_engine(routes, batch, T, "cuda:0")
    dbg = debug_bufs(eng)
    eng.solve(x0, debug=dbg)
    torch.cuda.synchronize()
    assert int((eng.status == 0).sum()) >= B - 4
    kkt_check(eng, batch, dbg)
    sl = slice(2048, 2560)
    ref = _oracle_step(oracle, pkg, routes, T, batch.x0[sl], batch.path_id[sl], batch.path_len[sl], batch.speed[sl],
                       batch.target_ind[sl], batch.oa[sl], batch.od[sl])
    e0 = _compare(eng, ref, sl)
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    sc, loop = WL.make_loop(4, eng, x0, hist_cap=16, routes=routes, batch=batch)
    e1 = _inputs_fed_ticks(oracle, pkg, routes, eng, loop, batch, T, 10, sl)
    print(f"config 4 share on the planned routes: KKT on 4096; 512-ego slice first step max|du|={e0:.2e}, 10 inputs-fed ticks {e1:.2e}")


def test_config3_scenario_loop_4096x30_glue_and_step_vs_oracles(pkg, oracle, planned):
    """soak_scenario.py as a test, at config 3's own size and set-up."""
    import loop_oracle as LO
    WL = pkg.workloads
    c = WL.CONFIGS[3]
    B, T, K = c["batch"], c["horizon"], 12
    routes = planned[False]
    batch = WL.ego_batch(routes, B, T, rank=0)
    S = pkg.synth

    def fresh():
        eng, x0 = WL.make_engine(routes, batch, T, "cuda:0")
        sc, loop = WL.make_loop(3, eng, x0, hist_cap=K + 4, routes=routes, batch=batch)
        return eng, sc, loop

    eng, sc, loop = fresh()
    glue_slice = np.arange(0, B, B // 384)[:384]
    n_glue = n_col = n_cut = 0
    worst = 0.0
    iters_by_tick = torch.zeros(B, dtype=torch.int64, device="cuda:0")
    for k in range(K):
        g = sc.obst.get(step=False)
        obst = g.cpu().numpy().copy()
        x0 = loop.x0.cpu().numpy().copy()
        tidx = sc.pre.traj_idx.cpu().numpy().copy(); prev = sc.pre.prev_len.cpu().numpy().copy()
        plen_before = eng.path_len.cpu().numpy().copy()
        sc.pre.predict(g)
        sc.pre.run(loop.x0)
        torch.cuda.synchronize()
        d_idx = sc.pre.traj_idx.cpu().numpy(); d_len = eng.path_len.cpu().numpy().copy()
        d_col = sc.pre.col_flag.cpu().numpy(); d_st = sc.pre.status.cpu().numpy()
        for b in glue_slice:
            full = routes[batch.path_id[b]]
            st, idx, plen, col = LO.loop_pre_tick((x0[b, 0], x0[b, 1], x0[b, 3], x0[b, 2]), int(tidx[b]),
                                                  None if prev[b] < 0 else int(prev[b]), full, obst, S.DL)
            if st != 0:
                ok = d_st[b] == st and d_len[b] == plen_before[b] and d_idx[b] == tidx[b]
            else:
                ok = d_st[b] == 0 and d_idx[b] == idx and d_len[b] == plen and bool(d_col[b]) == (col is not None)
            n_glue += not ok
            n_col += col is not None
        n_cut += int((d_len < batch.path_len).sum())
        tind = eng.target_ind.cpu().numpy().copy(); oa = eng.oa.cpu().numpy().copy(); od = eng.od.cpu().numpy().copy()
        ref = _oracle_step(oracle, pkg, routes, T, x0, batch.path_id, d_len, batch.speed, tind, oa, od)
        eng.solve(loop.x0)
        torch.cuda.synchronize()
        worst = max(worst, _compare(eng, ref, tol=1e-6))
        iters_by_tick += eng.n_iter.to(torch.int64)
        pkg._cabi.check(eng.lib.jsim_loop_advance(eng._ctx, eng.B, *loop._advance_args()), eng._ctx, "jsim_loop_advance")
        resp = loop.age == 0
        sc.pre.traj_idx.masked_fill_(resp, 0); sc.pre.prev_len.masked_fill_(resp, -1)
        sc.obst.get(step=True)
    assert n_glue == 0, n_glue
    assert n_col > 0 and n_cut > 0          # the obstacle vehicles did cut paths: the glue had work
    # the same K ticks as ONE fused scenario launch on a fresh copy: bit-identical history and end state
    eng2, sc2, loop2 = fresh()
    sc2.run(K)
    torch.cuda.synchronize()
    assert torch.equal(loop2.hist[:K], loop.hist[:K]) and torch.equal(loop2.x0, loop.x0)
    assert torch.equal(eng2.path_len, eng.path_len) and torch.equal(eng2.target_ind, eng.target_ind)
    # the per-ego iteration totals bench.py reads from the timed launches == the per-tick counts added up
    tot = np.zeros(B, dtype=np.uint64)
    pkg._cabi.check(eng2.lib.jsim_mpc_iter_totals(eng2._ctx, B, tot.ctypes.data, 1), eng2._ctx, "jsim_mpc_iter_totals")
    assert np.array_equal(tot.astype(np.int64), iters_by_tick.cpu().numpy())
    pkg._cabi.check(eng2.lib.jsim_mpc_iter_totals(eng2._ctx, B, tot.ctypes.data, 0), eng2._ctx, "jsim_mpc_iter_totals")
    assert not tot.any()                                       # reset
    print(f"config 3 at 4096 x 30, {K} ticks: glue of {len(glue_slice)} egos bit-exact every tick ({n_col} collision findings), "
          f"{n_cut} truncated-path steps, MPC step of all egos vs oracle max|du|={worst:.2e}; fused launch == tick by tick; "
          f"mean iterations per step {float(iters_by_tick.sum()) / (B * K):.2f}")


def test_bench_line_fields():
    """The headline workload with few ticks, as a real `python bench.py` run: the fields VERDICT round 2 (item 7) asked for."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "20", "--warmup", "3", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][0])
    cfg = j["config"]
    assert "jsim_mpc_iter_totals" in cfg["iters_source"] and 3.0 < cfg["mean_active_set_iters"] < 30.0
    s = cfg["straggler"]
    assert s["max_ego_iters_per_tick"] >= cfg["mean_active_set_iters"] and s["slowest_over_mean"] >= 1.0
    o = j["other_respawn_rule"]
    assert o["respawn"] == "start" and o["value"] > 0 and o["straggler"]["slowest_over_mean"] >= 1.0
    assert j["roofline"]["kernel"] == "mpc_step_reg_kernel<20, false, 1, true>"
    # the flops of the roofline come from the timed launches' own iteration count (SURVEY 8d's formula)
    flops = (16 * 20 ** 3 + 8 * 20 ** 3 / 3 + 40 * 400 * cfg["mean_active_set_iters"] + 32 * 400 + 1200) * 256 * 20
    assert abs(j["roofline"]["algorithmic_flops_per_launch"] / flops - 1.0) < 2e-3 and j["roofline"]["ticks_per_launch"] == 20
    spec_src = open(os.path.join(REPO, "bench.py")).read()
    assert 'mpc_step_reg4_kernel<{T}, {pre}>' in spec_src and "reg2" not in spec_src


def test_bench_on_a_horizon_without_a_register_kernel():
    """`python bench.py --horizon 24`: no register kernel, so the fused mode's closed loop runs as separate launches per tick
    inside jsim_mpc_run_ticks -- which count into jsim_mpc_iter_totals like the fused launches do, so the line has its
    iteration figures and names the LDS-resident kernel."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--horizon", "24", "--steps", "5", "--warmup", "2",
                          "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][0])
    cfg = j["config"]
    assert cfg["horizon"] == 24 and "jsim_mpc_iter_totals" in cfg["iters_source"] and cfg["mean_active_set_iters"] > 0
    s = cfg["straggler"]
    assert s["max_ego_iters_per_tick"] >= cfg["mean_active_set_iters"] and s["slowest_over_mean"] >= 1.0
    assert j["roofline"]["kernel"] == "mpc_step_kernel"


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """`python bench.py --dump-outputs DIR`: the last timed tick's controls, state, solution, status, index and path of every
    ego as float64 .npy files; two runs with the same arguments write identical arrays."""
    runs = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "20", "--warmup", "3", "--no-cpu-baseline",
                              "--no-respawn-start", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][0])
        assert j["steps"] == 20 and j["ms_per_step"] > 0
        runs.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = runs
    B, T = j["config"]["egos_per_gpu"], j["config"]["horizon"]
    shapes = {"controls": (B, 2), "state": (B, 4), "oa": (B, T), "od": (B, T), "status": (B,), "target_ind": (B,), "path_len": (B,)}
    assert {k: v.shape for k, v in a.items()} == shapes and all(v.dtype == np.float64 for v in a.values())
    assert all(np.isfinite(v).all() for v in a.values()) and np.abs(a["controls"]).max() > 0
    for k in shapes:
        assert np.array_equal(a[k], b[k]), k
