"""The per-ego table (BatchedMPC.set_ego_configs / jsim_mpc_set_ego_config: ego b solves with row b of a device array of weights
and limits instead of the context's jsim_cfg) on every kernel that reads it and in every loop.  Run with -m gpu on an MI355X.

The table is read by the one-wave register kernels (into their register copy of the launch constants, every wave of a block with
helpers), by the four-wave kernels (lane 0 into the LDS copy), by the LDS kernel and by the plant kernels of the host-ticked loops
(a failed ego brakes with its own MAX_DECEL); the fused kernels take that from their own copy.  The cases:

  1. one step of every single-step register kernel at every dispatch boundary, the LDS kernel and the acceleration-state variant
     against the oracle run per configuration (oracle_py.mpc_step_batch_per_config), the condensed QP of a dozen egos included;
  2. a table whose every row is the context's configuration changes nothing, bit for bit;
  3. row b means ego b: an engine whose context is row b, without a table, gives ego b the same bits;
  4. fused loops equal host-ticked loops with the table set (ClosedLoop, ScenarioLoop in both glue modes, InteractingLoop), the
     failed ego braking with its own row's MAX_DECEL on both sides; MAX_ITER = 3 and the path-speed reference against the oracle;
  5. launch ordering (the kernels index the table with order[blockIdx.x]) changes nothing;
  6. the states a closed loop visits, every ego and tick against the oracle;
  7. the surface: refusals, replacing a table, sharding.

Inputs: gpu_helpers.ego_config_case -- a pool of 12 drawn configurations (so that the oracle can group egos) and, at fixed ego
indices next to each other, planted rows: twins with one state and very different rows, an ego that fails and brakes with -3.7, a
row with tight limits beside a loose one.  Bars are those of test_step_vs_oracle and test_per_ego_weights_one_batch.  Controls
are compared where the ORACLE's status is 0; at most 1/16 of a case's egos may be left out that way (EXCLUDED_MAX), which
tests/test_ego_config_cpu.py proves for every shape used here from the oracle alone."""
import ctypes as C
import importlib
from dataclasses import replace

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
from gpu_helpers import (PLANT_DECEL, PLANT_EGOS, PLANT_FAIL, PLANT_LOOSE, PLANT_TIGHT, PLANT_TWINS, cu_count, debug_bufs,
                         ego_config_case, ego_config_pool, ego_config_rows, ego_config_table, engine, iter_totals, kkt_check, n_active,
                         oracle_batch_per_config, oracle_params_list, variant_batches, variant_id)

pytestmark = pytest.mark.gpu
CFG = importlib.import_module(PKG_NAME + ".config")
NON_PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if not r[2])
PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if r[2])
# the speed-cut-off glue on one row of each kernel family: one wave, one wave with helpers, four waves
SPEED_CUTOFF_ROWS = ((1, 20, True, 1, False), (1, 13, True, 1, True), (4, 40, True, 1, False))
SCENARIO_SPECS = [dict(direction=1, turning=False, speed=25 / 3.6, offset=None), dict(direction=-1, turning=True, speed=20 / 3.6, offset=1.0),
                  dict(kind="roundabout", direction=1, turning=True, speed=15 / 3.6, offset=2.0)]
NAMES = ("oa", "od", "ox", "oy", "ov", "oyaw", "xref", "target_ind", "status", "n_iter", "active_mask", "di_ai")
EXCLUDED_MAX = 16          # at most B // 16 egos of a case may have an oracle status != 0 (and so no compared controls)


def _rows(rows, every_batch=False, kind="stock"):
    """pytest params (T, size, kind) of rows: size = (row, k), k indexing variant_batches(row, cu) (every boundary size with
    every_batch, else the first)."""
    return [pytest.param(r[1], (r, k), kind, id=variant_id(r) + (f"-b{k}" if k else ""))
            for r in rows for k in range(len(variant_batches(r, 256)) if every_batch else 1)]


# beside the register kernels: the LDS kernel (no register kernel at T = 24) and the acceleration-state variant (NX = 5, LDS kernel)
OTHER_KERNELS = [pytest.param(24, 48, "stock", id="lds-T24"), pytest.param(13, 48, "jerk", id="jerk-T13")]
STEP_CASES = _rows(NON_PRE_ROWS, every_batch=True) + OTHER_KERNELS                     # case 1
SAME_CASES = _rows(CFG.REG_VARIANTS) + OTHER_KERNELS                                   # case 2
ROW_CASES = _rows(NON_PRE_ROWS) + OTHER_KERNELS                                        # case 3
CLOSED_LOOP_CASES = _rows(NON_PRE_ROWS) + OTHER_KERNELS                                # case 4, ClosedLoop
SCENARIO_CASES = (_rows(PRE_ROWS, kind="truncate") +                                   # case 4, ScenarioLoop
                  [pytest.param(r[1], (r, 0), "speed_cutoff", id=variant_id(r) + "-speed-cutoff") for r in SPEED_CUTOFF_ROWS])
VISITED_ROWS = ((1, 20, False, 1, True), (1, 20, False, 1, False), (4, 40, False, 1, False))   # case 6: B = CU count, + 1, 97
VISITED_CASES = _rows(VISITED_ROWS)
VISITED_K, VISITED_BATCH = 12, dict(truncate=False, near_end_frac=0.1)


def _batch(size, cu=None):
    """The batch size of a case: the fixed size, or variant_batches(row, this device's CU count)[k]."""
    if isinstance(size, int):
        return size
    row, k = size
    return variant_batches(row, cu_count() if cu is None else cu)[k]


def oracle_compared_shapes(cu):
    """The (T, B, kind, batch keywords, ticks) of the cases that compare controls with the oracle where its status is 0 -- cases 1
    (ticks = 0: one step) and 6 -- on a device of `cu` CUs, for tests/test_ego_config_cpu.py."""
    one = {(p.values[0], _batch(p.values[1], cu), p.values[2], (), 0) for p in STEP_CASES}
    loop = {(p.values[0], _batch(p.values[1], cu), p.values[2], tuple(sorted(VISITED_BATCH.items())), VISITED_K) for p in VISITED_CASES}
    return sorted(one) + sorted(loop)


def _base(pkg, kind, T):
    """The context's configuration of a case: the stock JSON, or the acceleration-state variant's / the path-speed variant's."""
    src = {"stock": pkg.MPCConfig.from_json, "jerk": lambda: pkg.mpc_jerk.config, "with_speed": lambda: pkg.mpc_with_speed.config}
    return replace(src[kind](), T=T)


def _snap(eng, **more):
    out = {k: getattr(eng, k).clone() for k in NAMES}
    out.update({k: v.clone() for k, v in more.items()})
    return out


def _eq(a, b):
    """torch.equal bit for bit: a failed ego's History record holds NaN for the deviation (and its predicted states may), which
    must be the same NaN on both sides."""
    if a.is_floating_point() and a.shape == b.shape and a.dtype == b.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def _same(a, b, where=""):
    assert a.keys() == b.keys()
    for k in a:
        assert _eq(a[k], b[k]), (k, where)


@pytest.mark.parametrize("T,size,kind", STEP_CASES)
def test_step_against_oracle_with_table(pkg, oracle, routes, T, size, kind):
    """Case 1.  One step with the table set, on every single-step register kernel at every batch size where the dispatch takes it,
    on the LDS kernel and on the acceleration-state variant, every ego against the oracle with that ego's configuration: status,
    target_ind and xref bit-exact, u* within 1e-7, active sets bit-exact, the condensed (H, g) of a dozen egos -- the planted ones
    first -- against the oracle's dense build with that ego's parameters (1e-9 relative: this pins the weights, not only the
    limits), the KKT conditions with per-ego limits.  The twins' solutions differ by more than 1e-2; slot 15 of the rows
    (`reserved`) holding NaN instead of 0 changes no bit."""
    B, base = _batch(size), _base(pkg, kind, T)
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, base=base)
    n = 2 * T + (1 if kind == "jerk" else 0)
    x0 = torch.from_numpy(batch.x0).cuda()
    runs = []
    for table in (cfgs, ego_config_rows(cfgs, reserved=np.nan)):           # the list form (reserved = 0.0), the array form
        eng = engine(pkg, routes, batch, T, config=base)
        eng.set_ego_configs(table)
        dbg = debug_bufs(eng, n)
        eng.solve(x0, debug=dbg)
        torch.cuda.synchronize()
        runs.append((eng, dbg))
    (eng, dbg), (eng_nan, dbg_nan) = runs
    _same(_snap(eng, **dbg), _snap(eng_nan, **dbg_nan), "reserved = NaN")
    ps, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which)
    st = eng.status.cpu().numpy()
    ok = ref["status"] == 0
    print(f"T={T} B={B} {kind}: oracle status != 0 for {(~ok).sum()} egos (cap {B // EXCLUDED_MAX}), "
          f"non-empty active sets {(n_active(ref['active_mask'])[ok] > 0).sum()}")
    assert (~ok).sum() <= B // EXCLUDED_MAX
    assert np.array_equal(st, ref["status"]) and st[PLANT_FAIL] == 1
    assert np.array_equal(eng.target_ind.cpu().numpy(), ref["target_ind"])
    np.testing.assert_array_equal(eng.xref.cpu().numpy(), ref["xref"])
    oa, od = eng.oa.cpu().numpy(), eng.od.cpu().numpy()
    err = max(np.abs(oa - ref["oa"])[ok].max(), np.abs(od - ref["od"])[ok].max())
    print(f"T={T} B={B} {kind}: max|du|={err:.2e}")
    assert err <= 1e-7, err
    assert np.array_equal(eng.active_mask.cpu().numpy().view(np.uint32), ref["active_mask"])
    lo = np.array([c.MAX_DECEL for c in cfgs])[:, None]
    hi = np.array([c.MAX_ACCEL for c in cfgs])[:, None]
    if kind != "jerk":                                  # (there oa is the jerk input u0, not the bounded acceleration)
        assert np.all(oa[ok] <= hi[ok] + 1e-9) and np.all(oa[ok] >= lo[ok] - 1e-9)
    a, b = PLANT_TWINS
    assert ok[a] and ok[b] and max(np.abs(oa[a] - oa[b]).max(), np.abs(od[a] - od[b]).max()) > 1e-2
    assert ok[PLANT_TIGHT] and ok[PLANT_LOOSE]
    assert n_active(ref["active_mask"])[PLANT_TIGHT] > n_active(ref["active_mask"])[PLANT_LOOSE]   # working sets differ between neighbours
    # the condensed QP with each ego's own weights
    H, g = dbg["H"].cpu().numpy(), dbg["g"].cpu().numpy()
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    egos = [e for e in PLANT_EGOS if ok[e]] + [e for e in np.flatnonzero(ok) if e not in PLANT_EGOS]
    for e in egos[:12]:
        o, m = off[batch.path_id[e]], batch.path_len[e]
        r = oracle.mpc_step(ps[which[e]], (batch.x0[e, 0], batch.x0[e, 1], batch.x0[e, 3], batch.x0[e, 2]), cx[o:o + m], cy[o:o + m],
                            cyaw[o:o + m], int(batch.target_ind[e]), batch.speed[e], oa=batch.oa[e], od=batch.od[e], want_qp=True)
        He = H[e]
        if kind == "jerk":                              # that kernel writes the lower triangle
            He = np.tril(He) + np.tril(He, -1).T
        assert np.abs(He - r["H"]).max() <= 1e-9 * np.abs(r["H"]).max(), e
        assert np.abs(g[e] - r["g"]).max() <= 1e-9 * max(1.0, np.abs(r["g"]).max()), e
    if kind != "jerk":                                  # kkt_check states the 2T-variable QP
        kkt_check(eng, batch, dbg, cfgs=cfgs)


def _run_loop(pkg, eng, x0, pre, K, **kw):
    """K fused ticks of the closed loop (pre: of the scenario loop, whose kernels carry the glue): (loop, snapshot)."""
    if pre:
        sc = pkg.ScenarioLoop(eng, x0.clone(), SCENARIO_SPECS, hist_cap=K, **kw)
        loop, run = sc.loop, sc.run
    else:
        loop = pkg.ClosedLoop(eng, x0.clone(), hist_cap=K, **kw)
        run = loop.run
    run(K)
    torch.cuda.synchronize()
    return loop, _snap(eng, x0=loop.x0, hist=loop.hist, age=loop.age, n_respawn=loop.n_respawn, path_len=eng.path_len)


@pytest.mark.parametrize("T,size,kind", SAME_CASES)
def test_table_of_context_rows_changes_nothing(pkg, routes, T, size, kind):
    """Case 2.  A table whose every row is the context's configuration (a drawn one, not the stock values) against no table:
    one step and K fused ticks -- ClosedLoop.run, on the rows with the glue ScenarioLoop.run -- equal bit for bit on every
    register kernel, the LDS kernel and the acceleration-state variant.  Qf * T and MAX_DSTEER_rad * dt are formed from the same
    doubles on both paths, so a unit or scaling slip shows without any tolerance.  set_ego_configs(None) restores the plain results."""
    B, K = _batch(size), 8
    pre = not isinstance(size, int) and size[0][2]
    base = _base(pkg, kind, T)
    ctx = ego_config_pool(T, base=base)[3]
    batch, _, _ = ego_config_case(pkg.synth, routes, T, B, base=base, truncate=not pre)
    x0 = torch.from_numpy(batch.x0).cuda()
    steps, loops = [], []
    for table in (None, [ctx] * B):
        eng = engine(pkg, routes, batch, T, config=ctx)
        eng.set_ego_configs(table)
        eng.solve(x0)
        torch.cuda.synchronize()
        steps.append(_snap(eng))
        eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
        loops.append(_run_loop(pkg, eng, x0, pre, K, max_age=5)[1])
    _same(steps[0], steps[1], "one step")
    _same(loops[0], loops[1], "fused ticks")
    assert int(steps[0]["status"][PLANT_FAIL]) == 1 and int((steps[0]["status"] == 0).sum()) >= B - B // EXCLUDED_MAX
    assert int(loops[0]["n_respawn"]) >= B
    eng.set_ego_configs(ego_config_table(ego_config_pool(T, base=base), B)[0])       # another table in between ...
    eng.set_ego_configs(None)                                                        # ... and off again
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    eng.solve(x0)
    torch.cuda.synchronize()
    again = _snap(eng)
    solved = again["status"] == 0                       # (a failed ego's predicted states are not written: they are the loop's last)
    for k in ("oa", "od", "ox", "oy", "ov", "oyaw", "active_mask", "n_iter", "status"):
        rows = solved if k in ("ox", "oy", "ov", "oyaw") else slice(None)
        assert _eq(again[k][rows], steps[0][k][rows]), k


@pytest.mark.parametrize("T,size,kind", ROW_CASES)
def test_row_b_means_ego_b(pkg, routes, T, size, kind):
    """Case 3.  For the planted egos and three drawn ones: an engine of the same batch and size whose CONTEXT is that ego's
    configuration, without a table, gives that ego what the table run gives it, bit for bit (the same kernel row on both sides)."""
    B, base = _batch(size), _base(pkg, kind, T)
    batch, cfgs, _ = ego_config_case(pkg.synth, routes, T, B, base=base)
    x0 = torch.from_numpy(batch.x0).cuda()
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    eng.solve(x0)
    torch.cuda.synchronize()
    tab = _snap(eng)
    others = np.setdiff1d(np.arange(B), PLANT_EGOS)
    egos = list(PLANT_EGOS) + [int(e) for e in np.random.default_rng(T).choice(others, 3, replace=False)]
    n_diff = 0
    for e in egos:
        one = engine(pkg, routes, batch, T, config=cfgs[e])
        one.solve(x0)
        torch.cuda.synchronize()
        got = _snap(one)
        for k in NAMES:
            assert _eq(got[k][e], tab[k][e]), (k, e)
        n_diff += int(not _eq(got["oa"], tab["oa"]))
    assert n_diff == len(egos)                          # each context differs from the table somewhere else: rows are per ego


def _loop_state(eng, loop, **more):
    rec = loop.recorder
    return _snap(eng, x0=loop.x0, hist=loop.hist, age=loop.age, n_respawn=loop.n_respawn, tick=loop.tick_counter, rec=rec.rec,
                 flags=rec.flags, path_len=eng.path_len, **more)


def _brakes_with_its_own_row(state, where, n_min=2):
    """The planted ego fails at tick 0 (and after every respawn: n_min times at least) and brakes with ITS row's MAX_DECEL: applied
    acceleration -3.7 in the History record, not the context's -10 or -5 and not a neighbour's."""
    a = state["rec"][:, PLANT_FAIL, 5].cpu().numpy()
    assert a[0] == PLANT_DECEL and (a == PLANT_DECEL).sum() >= n_min, (where, a)
    assert state["hist"][0, PLANT_FAIL, 1].item() == PLANT_DECEL, where


@pytest.mark.parametrize("T,size,kind", CLOSED_LOOP_CASES)
def test_fused_ticks_equal_single_ticks_with_table(pkg, routes, T, size, kind):
    """Case 4, ClosedLoop.  jsim_mpc_run_ticks (the fused kernels: the failure path brakes with the kernel's own copy of the row)
    against K x (jsim_mpc_step + jsim_loop_advance) (the plant kernel reads the table itself) with the table set, on every
    single-step register kernel, the LDS kernel and the acceleration-state variant: history, History records and flags, final
    state, ages, respawn count (max_age forces respawns) and iteration totals bit for bit; the failed planted ego brakes with -3.7
    on both sides."""
    B, K = _batch(size), 16
    base = _base(pkg, kind, T)
    batch, cfgs, _ = ego_config_case(pkg.synth, routes, T, B, base=base, truncate=False, near_end_frac=0.5)
    def make():
        eng = engine(pkg, routes, batch, T, config=base)
        eng.set_ego_configs(cfgs)
        return eng, pkg.ClosedLoop(eng, torch.from_numpy(batch.x0).cuda(), hist_cap=K, max_age=5, record=K)
    e1, l1 = make()
    iters = torch.zeros(B, dtype=torch.int64, device=e1.device)
    for _ in range(K):
        l1.tick()
        iters += e1.n_iter
    e2, l2 = make()
    l2.run(K // 2 - 3); l2.run(K - (K // 2 - 3))
    torch.cuda.synchronize()
    s1, s2 = _loop_state(e1, l1), _loop_state(e2, l2)
    _same(s1, s2)
    assert int(s1["tick"]) == K and int(s1["n_respawn"]) >= 2 * B
    assert np.array_equal(iter_totals(e2), iters.cpu().numpy()) and int(iters.sum()) > 0
    _brakes_with_its_own_row(s1, "host ticks"); _brakes_with_its_own_row(s2, "fused")


@pytest.mark.parametrize("T,size,mode", SCENARIO_CASES)
def test_fused_scenario_loop_equals_tick_by_tick_with_table(pkg, routes, T, size, mode):
    """Case 4, ScenarioLoop.  jsim_loop_run_scenario against the same ticks driven from the host with the table set, on every kernel
    with the glue inside (truncating glue) and on one row of each kernel family with the speed-cut-off glue: every buffer and History
    record bit-identical, iteration totals equal, the failed planted ego braking with -3.7 on both sides."""
    B, K1, K2 = _batch(size), 7, 9
    kw, kind = {}, "stock"
    if mode == "speed_cutoff":
        kind = "with_speed"
        kw = dict(cv=[np.full(len(r), pkg.mpc_with_speed.MAX_SPEED) for r in routes])
    base = _base(pkg, kind, T)
    states, iters = [], []
    for fused in (False, True):
        batch, cfgs, _ = ego_config_case(pkg.synth, routes, T, B, base=base, seed=17, truncate=False, near_end_frac=0.1)
        eng = engine(pkg, routes, batch, T, config=base, **kw)
        eng.set_ego_configs(cfgs)
        sc = pkg.ScenarioLoop(eng, torch.from_numpy(batch.x0).cuda(), SCENARIO_SPECS, hist_cap=K1 + K2, max_age=5, mode=mode, record=K1 + K2)
        if fused:
            sc.run(K1); sc.run(K2)
            iters.append(iter_totals(eng))
        else:
            n = torch.zeros(B, dtype=torch.int64, device=eng.device)
            for _ in range(K1 + K2):
                sc.tick()
                n += eng.n_iter
            iters.append(n.cpu().numpy())
        torch.cuda.synchronize()
        cut = eng.path_len if mode == "truncate" else sc.pre.cut
        states.append(_loop_state(eng, sc.loop, cut=cut, traj_idx=sc.pre.traj_idx, prev_len=sc.pre.prev_len, col=sc.pre.col_flag,
                                  pst=sc.pre.status, obs=sc.obst.state, get=sc.obst.get_buf, rec_obs=sc.recorder.obs))
    _same(*states)
    a = states[0]
    assert np.array_equal(iters[0], iters[1]) and iters[0].sum() > 0
    assert int((a["col"] != 0).sum()) > 0 and int((a["cut"] < eng.full_len).sum()) > 0 and int((a["pst"] != 0).sum()) == 0
    assert int(((a["flags"] & 6) != 0).sum()) >= B          # every ego respawned
    for s, where in zip(states, ("host ticks", "fused")):
        _brakes_with_its_own_row(s, where)


def test_interacting_loop_with_table(pkg):
    """Case 4, InteractingLoop (jsim_loop_run_interacting): K ticks in one call against K calls of one tick with the table set --
    every buffer and History record bit-identical; the failed planted ego brakes with -3.7; and the table matters (the same loop
    without it ends elsewhere)."""
    W = importlib.import_module(PKG_NAME + ".workloads")
    iroutes = W.route_table(False)[0]
    T, G, K = 13, 8, 20
    base = _base(pkg, "stock", T)
    batch, sizes = W.interacting_batch(iroutes, G, T, seed=3)
    batch.x0[PLANT_FAIL, 2] = 9.5
    cfgs, _ = ego_config_table(ego_config_pool(T, base=base), batch.x0.shape[0])
    states = []
    for mode in ("ticks", "run", "no table"):
        eng = engine(pkg, iroutes, batch, T, config=base)
        eng.set_ego_configs(None if mode == "no table" else cfgs)
        il = pkg.InteractingLoop(eng, torch.from_numpy(batch.x0).cuda(), group_sizes=sizes, hist_cap=K, max_age=7, frame_window=20, record=K)
        if mode == "ticks":
            for _ in range(K):
                il.tick()
        else:
            il.run(K)
        torch.cuda.synchronize()
        states.append(_loop_state(eng, il.loop, traj_idx=il.pre.traj_idx, prev_len=il.pre.prev_len, col=il.pre.col_flag))
    _same(states[0], states[1])
    _brakes_with_its_own_row(states[0], "ticks"); _brakes_with_its_own_row(states[1], "run")
    assert not _eq(states[0]["hist"], states[2]["hist"])
    assert states[2]["rec"][0, PLANT_FAIL, 5].item() == base.MAX_DECEL


@pytest.mark.parametrize("T", (20, 40))
def test_max_iter_passes_with_table(pkg, oracle, routes, T):
    """Case 4.  MAX_ITER = 3 (one launch per linearisation pass, every pass reads the table again) against the oracle's three passes
    per configuration."""
    B = 96 if T <= 20 else 48
    base = replace(_base(pkg, "stock", T), MAX_ITER=3)
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, base=base)
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    eng.solve(torch.from_numpy(batch.x0).cuda())
    torch.cuda.synchronize()
    ps, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which)
    assert ps[which[0]].max_iter == 3
    _, ref1 = oracle_batch_per_config(oracle, pkg.synth, routes, batch, [replace(c, MAX_ITER=1) for c in cfgs], which)
    st = eng.status.cpu().numpy()
    ok = ref["status"] == 0
    assert (~ok).sum() <= B // EXCLUDED_MAX
    assert np.array_equal(st, ref["status"]) and st[PLANT_FAIL] == 1
    assert np.array_equal(eng.target_ind.cpu().numpy(), ref["target_ind"])
    np.testing.assert_array_equal(eng.xref.cpu().numpy()[ok], ref["xref"][ok])
    assert np.abs(eng.oa.cpu().numpy() - ref["oa"])[ok].max() <= 1e-7
    assert np.abs(eng.od.cpu().numpy() - ref["od"])[ok].max() <= 1e-7
    assert np.array_equal(eng.active_mask.cpu().numpy().view(np.uint32)[ok], ref["active_mask"][ok])
    assert np.abs(ref["oa"] - ref1["oa"])[ok].max() > 1e-3                     # the extra passes matter


def test_path_speed_reference_with_table(pkg, oracle, routes):
    """Case 4.  The mpc_with_speed variant (a per-point speed reference with a per-ego cut-off; its speed weight of 20 drawn over by
    the rows' 0 or 2) with the table set, against the oracle per configuration."""
    T, B = 13, 96
    m = pkg.mpc_with_speed
    base = _base(pkg, "with_speed", T)
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, base=base, seed=9, near_end_frac=0.3)
    cut = np.where(np.random.default_rng(3).random(B) < 0.6, np.random.default_rng(4).integers(0, 720, size=B), -1).astype(np.int32)
    cvs = [np.full(len(r), m.MAX_SPEED) for r in routes]
    eng = engine(pkg, routes, batch, T, config=base, cv=cvs)
    eng.set_speed_cutoff(cut)
    eng.set_ego_configs(cfgs)
    eng.solve(torch.from_numpy(batch.x0).cuda())
    torch.cuda.synchronize()
    _, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, cv=np.concatenate(cvs), cv_cut=cut)
    ok = ref["status"] == 0
    assert (~ok).sum() <= B // EXCLUDED_MAX
    assert np.array_equal(eng.status.cpu().numpy(), ref["status"])
    np.testing.assert_array_equal(eng.xref.cpu().numpy(), ref["xref"])
    assert float(np.abs(ref["xref"][:, 2]).max()) > 0 and (ref["xref"][:, 2] == 0).any()
    assert np.abs(eng.oa.cpu().numpy() - ref["oa"])[ok].max() <= 1e-7
    assert np.abs(eng.od.cpu().numpy() - ref["od"])[ok].max() <= 1e-7
    assert np.array_equal(eng.active_mask.cpu().numpy().view(np.uint32), ref["active_mask"])


@pytest.mark.parametrize("pre", (False, True), ids=("closed", "scenario"))
@pytest.mark.parametrize("B", (600, 1025))
@pytest.mark.parametrize("T", (20, 40))
def test_launch_order_with_table(pkg, routes, T, B, pre):
    """Case 5.  With 512 <= B <= 65536 the second fused launch hands workgroup w the ego order[w]; the kernels must index the table
    with that ego, not with the workgroup.  Half the pool has tight limits, so iteration counts differ strongly and the order of
    the second launch is far from the identity (asserted); two launches with ordering on equal the same with ordering off, bit
    for bit.  B = 1025 at T = 20 is the two-waves-per-SIMD row."""
    K = 4
    base = _base(pkg, "stock", T)
    pool = ego_config_pool(T, base=base)
    pool = pool[:6] + [replace(c, MAX_ACCEL=0.05, MAX_DSTEER=0.4) for c in pool[6:]]
    batch, _, _ = ego_config_case(pkg.synth, routes, T, B, base=base, truncate=False, near_end_frac=0.1)
    cfgs, _ = ego_config_table(pool, B)
    out = []
    for enabled in (False, True):
        eng = engine(pkg, routes, batch, T, config=base)
        eng.set_ego_configs(cfgs)
        pkg._cabi.check(eng.lib.jsim_mpc_set_launch_order(eng._ctx, 1 if enabled else 0), eng._ctx)
        x0 = torch.from_numpy(batch.x0).cuda()
        if pre:
            sc = pkg.ScenarioLoop(eng, x0, SCENARIO_SPECS[:2], hist_cap=2 * K, max_age=400, record=2 * K)
            loop, run = sc.loop, sc.run
        else:
            loop = pkg.ClosedLoop(eng, x0, hist_cap=2 * K, max_age=400, record=2 * K)
            run = loop.run
        run(K)
        work1 = None
        if enabled:
            work1 = np.zeros(B, dtype=np.uint32)
            pkg._cabi.check(eng.lib.jsim_mpc_get_launch_order(eng._ctx, B, None, work1.ctypes.data_as(C.c_void_p)), eng._ctx)
        run(K)
        torch.cuda.synchronize()
        out.append((eng, _loop_state(eng, loop), work1))
    (e0, s0, _), (e1, s1, work1) = out
    order = np.zeros(B, dtype=np.int32)
    pkg._cabi.check(e1.lib.jsim_mpc_get_launch_order(e1._ctx, B, order.ctypes.data_as(C.c_void_p), None), e1._ctx)
    assert np.array_equal(order, np.argsort(-work1.astype(np.int64), kind="stable"))
    print(f"T={T} B={B}: {(order != np.arange(B)).mean() * 100:.0f} % of the workgroups get another ego; iterations in launch 1: "
          f"median {int(np.median(work1))}, max {work1.max()}")
    assert not np.array_equal(order, np.arange(B))       # otherwise the case proves nothing
    _same(s0, s1)
    _brakes_with_its_own_row(s1, "ordered", n_min=1)        # (no respawns here)


@pytest.mark.parametrize("T,size,kind", VISITED_CASES)
def test_visited_states_against_oracle_with_table(pkg, oracle, routes, T, size, kind):
    """Case 6.  The states a closed loop with the table visits: before every tick the oracle gets the kernel's inputs (so no drift
    bar is needed) and solves every ego with its configuration; status, active sets and target_ind exact, controls within 1e-7,
    every ego and tick.  T = 20 at B = CU count (helpers) and one more, T = 40."""
    B, base = _batch(size), _base(pkg, kind, T)
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, base=base, **VISITED_BATCH)
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    loop = pkg.ClosedLoop(eng, torch.from_numpy(batch.x0).cuda(), max_age=70)
    ps = oracle_params_list(oracle, cfgs, which)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    worst = 0.0
    for k in range(VISITED_K):
        x0 = loop.x0.cpu().numpy().copy(); tind = eng.target_ind.cpu().numpy().copy()
        oa = eng.oa.cpu().numpy().copy(); od = eng.od.cpu().numpy().copy()
        loop.tick()
        torch.cuda.synchronize()
        # loop.tick() has advanced the plant; status / controls / masks / target_ind are still this tick's solve
        ref = oracle.mpc_step_batch_per_config(ps, which, x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off, tind, oa, od,
                                               n_threads=16)
        ok = ref["status"] == 0
        assert (~ok).sum() <= B // EXCLUDED_MAX, k
        assert np.array_equal(eng.status.cpu().numpy(), ref["status"]), k
        assert np.array_equal(eng.active_mask.cpu().numpy().view(np.uint32), ref["active_mask"]), k
        resp = loop.age.cpu().numpy() == 0                              # respawned egos had oa / od / target_ind reset by the advance
        keep = ok & ~resp
        worst = max(worst, float(np.abs(eng.oa.cpu().numpy() - ref["oa"])[keep].max()), float(np.abs(eng.od.cpu().numpy() - ref["od"])[keep].max()))
        assert np.array_equal(eng.target_ind.cpu().numpy()[~resp], ref["target_ind"][~resp]), k
        if not resp[PLANT_FAIL]:                                        # (a respawn clears the applied controls)
            assert (eng.di_ai[PLANT_FAIL, 1].item() == PLANT_DECEL) == (ref["status"][PLANT_FAIL] != 0), k
    print(f"T={T} B={B}: worst |du| over {VISITED_K} ticks {worst:.2e}")
    assert worst <= 1e-7, worst


def test_set_ego_configs_surface(pkg, routes):
    """Case 7.  set_ego_configs refuses a wrong shape and a configuration of another horizon; a new table replaces the old one for
    the next run of an existing ClosedLoop (the result is that of a fresh loop with the new table from the same state)."""
    T, B, K = 20, 64, 6
    base = _base(pkg, "stock", T)
    batch, cfgs, _ = ego_config_case(pkg.synth, routes, T, B, base=base, truncate=False)
    eng = engine(pkg, routes, batch, T, config=base)
    rows = ego_config_rows(cfgs)
    for bad in (rows[:-1], rows[:, :15], np.zeros((B, 17)), cfgs[:-1], torch.zeros(B + 1, 16, dtype=torch.float64)):
        with pytest.raises(ValueError):
            eng.set_ego_configs(bad)
    with pytest.raises(ValueError):
        eng.set_ego_configs(cfgs[:-1] + [replace(cfgs[-1], T=T + 1)])
    other = ego_config_table(ego_config_pool(T, seed=5, base=base), B, seed=6)[0]
    eng.set_ego_configs(cfgs)
    loop = pkg.ClosedLoop(eng, torch.from_numpy(batch.x0).cuda(), hist_cap=2 * K, max_age=400)
    loop.run(K)
    torch.cuda.synchronize()
    mid = dict(x0=loop.x0.clone(), tind=eng.target_ind.clone(), oa=eng.oa.clone(), od=eng.od.clone(), di_ai=eng.di_ai.clone(),
               age=loop.age.clone())
    eng.set_ego_configs(other)
    loop.run(K)
    torch.cuda.synchronize()
    e2 = engine(pkg, routes, batch, T, config=base)
    e2.load_state(mid["tind"], mid["oa"], mid["od"])
    e2.di_ai.copy_(mid["di_ai"])
    e2.set_ego_configs(other)
    l2 = pkg.ClosedLoop(e2, mid["x0"].clone(), hist_cap=K, max_age=400)
    l2.x0_spawn.copy_(loop.x0_spawn); l2.target_spawn.copy_(loop.target_spawn); l2.age.copy_(mid["age"])
    l2.run(K)
    torch.cuda.synchronize()
    assert _eq(l2.hist[:K], loop.hist[K:2 * K]) and _eq(l2.x0, loop.x0)
    e3 = engine(pkg, routes, batch, T, config=base)                   # ... and differs from going on with the old table
    e3.set_ego_configs(cfgs)
    l3 = pkg.ClosedLoop(e3, torch.from_numpy(batch.x0).cuda(), hist_cap=2 * K, max_age=400)
    l3.run(2 * K)
    torch.cuda.synchronize()
    assert _eq(l3.hist[:K], loop.hist[:K]) and not _eq(l3.hist[K:], loop.hist[K:])


def test_sharded_table(pkg, routes):
    """Case 7.  Sharding with a table: the table is per engine, so rank r's engine gets rows [lo:hi] of shard_range along with its
    egos; sharding.CabiGather takes no part in it and does not refuse it.  Rehearsed in one process like test_cabi_gather_single_rank
    (a communicator of one rank per engine): the shards' gathered results are the unsharded run's, bit for bit."""
    T, B, world = 20, 96, 2
    base = _base(pkg, "stock", T)
    batch, cfgs, _ = ego_config_case(pkg.synth, routes, T, B, base=base)
    whole = engine(pkg, routes, batch, T, config=base)
    whole.set_ego_configs(cfgs)
    whole.solve(torch.from_numpy(batch.x0).cuda())
    parts = []
    for rank in range(world):
        lo, hi = pkg.sharding.shard_range(B, rank, world)
        sub = pkg.synth.EgoBatch(**{k: getattr(batch, k)[lo:hi].copy() for k in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od")})
        eng = engine(pkg, routes, sub, T, config=base)
        eng.set_ego_configs(cfgs[lo:hi])
        eng.solve(torch.from_numpy(sub.x0).cuda())
        g = pkg.sharding.CabiGather(eng, rank=0, world=1)
        parts.append({k: g.gather_rows(getattr(eng, k), hi - lo) for k in ("oa", "od", "status", "active_mask")})
        torch.cuda.synchronize()
        g.close()
    for k in parts[0]:
        assert _eq(torch.cat([p[k] for p in parts]), getattr(whole, k)), k
    assert int(whole.status[PLANT_FAIL]) == 1 and float((whole.oa[PLANT_TWINS[0]] - whole.oa[PLANT_TWINS[1]]).abs().max()) > 1e-2
