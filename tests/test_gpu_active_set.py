"""The active-set iteration's own failure exit and its dependent entering rows on every kernel.  Run with -m gpu on an MI355X.

Every failing ego of the other GPU tests fails by v0 > speed or v0 < MIN_SPEED, an exit the owner takes before the QP is built.
Here egos fail INSIDE the loop -- `if (isinf(t1) && isinf(t2)) { failed = true; break; }` of csrc/mpc_step_reg.inc, its twins in
mpc_step_reg4.inc and in the LDS kernel of jsim_mpc.hip -- after dozens of adds and drops, with J's rows in registers, R in LDS
and the multipliers half updated; in the fused loops the same wave then goes on to the next tick.  Their neighbours are solvable
egos under tight limits that start off their path: large working sets (2T - 1 rows), hundreds of drops, and entering rows that
depend on the working set (`dependent = !(zn > JSIM_DEP_TOL * dd)`: a pure dual step and a forced drop), which the stock inputs
meet 1 to 4 times per 96 egos.  Inputs: tests/active_set_cases.py (mixed_case, through the per-ego table); that they do take these
paths is proved on the oracle alone, with its trace, by tests/test_active_set_cpu.py for every (T, B) used here.

  (a) test_step_mixed_batch_against_oracle      one step, every row without the glue at its first dispatch batch, and T = 24
  (b) test_closed_loop_mixed_batch / test_scenario_loop_mixed_batch
                                               K ticks: fused == tick by tick, the ticked run against the oracle's closed loop,
                                               the neighbours of a planted ego byte-identical to a run without the planted rows
  (c) test_max_iter_passes_mixed_batch          MAX_ITER = 3: a planted ego fails in the loop on the first pass

Parametrised by row of config.REG_VARIANTS: a new row is covered without a list to edit."""
import importlib
from dataclasses import replace

import numpy as np
import pytest
import torch

import active_set_cases as AC
from conftest import PKG_NAME
from gpu_helpers import (PLANT_DECEL, PLANT_FAIL, W, cu_count, debug_bufs, engine, iter_totals, kkt_check, oracle_batch_per_config,  # noqa: F401
                         oracle_params_list, variant_batch, variant_id)

pytestmark = pytest.mark.gpu
CFG = importlib.import_module(PKG_NAME + ".config")
NON_PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if not r[2])
PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if r[2])
LDS_T, LDS_B = 24, 48                      # no register kernel at T = 24: the LDS kernel
STEP_CASES = [pytest.param(r[1], r, id=variant_id(r)) for r in NON_PRE_ROWS] + [pytest.param(LDS_T, LDS_B, id="lds-T24")]
CLOSED_CASES = [pytest.param(r[1], r, id=variant_id(r)) for r in NON_PRE_ROWS] + [pytest.param(LDS_T, 64, id="lds-T24")]
SCENARIO_CASES = [pytest.param(r[1], r, id=variant_id(r)) for r in PRE_ROWS]
MAX_ITER_SHAPES = ((20, 96), (40, 48))     # (c): the shapes of test_max_iter_relinearisation_passes at these horizons
LOOP_B, LOOP_MAX_AGE, LOOP_DI = 64, 3, 0.05
N_ITER_SAME = 0.8                          # test_speed_rows_in_the_working_set's floor for horizons outside its baseline, all egos
N_ITER_SAME_SOLVABLE = 0.9                 # test_step_vs_oracle's floor, here on the egos that solve
NAMES = ("oa", "od", "ox", "oy", "ov", "oyaw", "xref", "target_ind", "status", "n_iter", "active_mask", "di_ai")


def max_iters(T):
    """The iteration cap of one solve, in the oracle and in every kernel: 50 n + 100 with n = 2T variables."""
    return 50 * 2 * T + 100


def loop_ticks(T):
    return 6 if T <= 25 else 4


def step_batch(size, cu):
    """(a): the fixed size, or the row's first dispatch batch on a device of cu CUs."""
    return size if isinstance(size, int) else variant_batch(size, cu)


def loop_batch(size, cu):
    """(b): 64 egos where the dispatch takes the row at that size -- the rows with helpers (B <= cu) and the four-wave rows (any B)
    -- else the row's own first dispatch batch."""
    if isinstance(size, int):
        return size
    W_, T, pre, wpe, help_ = size
    return LOOP_B if (help_ or W_ == 4) else variant_batch(size, cu)


def oracle_shapes(cu):
    """What tests/test_active_set_cpu.py proves the premises for: the (T, B) of the one-step cases (a) and (c) and the (T, B, K)
    of the closed loops against the oracle (b), on a device of cu CUs."""
    one = {(p.values[0], step_batch(p.values[1], cu)) for p in STEP_CASES} | set(MAX_ITER_SHAPES)
    loops = {(p.values[0], loop_batch(p.values[1], cu), loop_ticks(p.values[0])) for p in CLOSED_CASES}
    return sorted(one), sorted(loops)


def _base(pkg, T, **kw):
    return replace(pkg.MPCConfig.from_json(), T=T, **kw)


def _eq(a, b):
    """Bit for bit (a failed ego's History record holds NaN for the deviation: the same NaN on both sides)."""
    if a.is_floating_point() and a.shape == b.shape and a.dtype == b.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def _check_step(pkg, oracle, routes, eng, dbg, batch, cfgs, which, what, u_tol=1e-6):
    """One solved step of a mixed batch against the oracle; returns (reference, device n_iter, report line)."""
    T, B = eng.T, eng.B
    _, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, trace=True)
    must_fail = AC.contradictory(batch, cfgs, eng.dt)
    st = eng.status.cpu().numpy()
    assert np.array_equal(st, ref["status"]), np.flatnonzero(st != ref["status"])
    assert np.array_equal(st == 1, must_fail) and set(st) <= {0, 1}
    ok = st == 0
    oa, od = eng.oa.cpu().numpy(), eng.od.cpu().numpy()
    assert np.all(oa[~ok] == 0) and np.all(od[~ok] == 0)          # failure -> cold start next tick
    mask = eng.active_mask.cpu().numpy().view(np.uint32)
    assert np.array_equal(mask[ok], ref["active_mask"][ok])
    err = max(np.abs(oa - ref["oa"])[ok].max(), np.abs(od - ref["od"])[ok].max())
    errs = {k: float(np.abs(getattr(eng, k).cpu().numpy() - ref[k])[ok].max()) for k in ("ox", "oy", "ov", "oyaw")}
    n_iter = eng.n_iter.cpu().numpy()
    same = float((n_iter == ref["n_iter"]).mean())
    ea, eb = AC.planted(B)
    pl = np.concatenate([ea, eb])
    same_ok, same_pl = float((n_iter == ref["n_iter"])[ok].mean()), float((n_iter == ref["n_iter"])[pl].mean())
    line = (f"{what} T={T} B={B}: in-loop failures {int((st[pl] == 1).sum())} of {len(pl)} planted, longest solve {int(n_iter.max())} "
            f"(oracle {int(ref['n_iter'].max())}), n_iter identical {same:.3f} (solvable egos {same_ok:.3f}, planted {same_pl:.3f}), max|du| {err:.2e}, max|dx| {max(errs.values()):.2e}, "
            f"planted iterations {int(n_iter[pl].min())}..{int(n_iter[pl].max())}; oracle trace {AC.trace_totals(oracle, ref['trace'])}")
    print(line)
    assert err <= u_tol, err
    assert max(errs.values()) <= 1e-6, errs
    if dbg is not None:
        kkt_check(eng, batch, dbg, cfgs)
    # the device's own counters: a planted ego completed an iteration before the one that found no step length -- and it was that
    # exit, not the iteration cap beside it, which counts max_iters + 1 --, the ego that fails on a constant row never entered the
    # loop, and the batch's longest solve is longer than 2T
    assert np.all(st[pl] == 1) and np.all(n_iter[pl] >= 2) and np.all(n_iter[pl] <= max_iters(T)), n_iter[pl]
    assert st[PLANT_FAIL] == 1 and n_iter[PLANT_FAIL] == 0
    assert n_iter.max() > 2 * T
    assert same_ok >= N_ITER_SAME_SOLVABLE, same_ok
    return ref, n_iter, same


@pytest.mark.parametrize("T,size", STEP_CASES)
def test_step_mixed_batch_against_oracle(pkg, oracle, routes, T, size):
    """(a) One step of the mixed batch through the per-ego table against the oracle run per configuration: status identical for
    every ego and 1 exactly on the egos whose limits contradict each other by arithmetic (active_set_cases.contradiction); oa, od
    zero on failed egos; where the status is 0 the active sets bit-identical, u* within 1e-6 (the bar
    test_large_working_sets_on_the_long_horizon_kernels holds for these limits), the predicted states within 1e-6, and the KKT
    conditions of the kernel's own QP with per-ego limits.  From the device's n_iter: the planted egos iterated before failing
    and the longest solve exceeds 2T.  The share of egos with the oracle's iteration count is printed and held to 0.8, the floor
    of test_speed_rows_in_the_working_set for horizons outside its baseline: rows that tie to the last bits may enter in another
    order, a different pivoting rule would not pass.

    Measured on an MI355X: 0.875 .. 0.911 over all egos on every row -- and the egos that differ are the planted ones (an eighth
    of the batch), the solvable egos agree to 1.000.  That is the nature of the exit, not of a kernel: on an infeasible QP the
    entering row depends on the working set, and of r = R^-1 d1 the components that are zero in exact arithmetic carry rounding
    noise whose SIGN decides whether a position is "dropped" on the way to "no step length".  The oracle shows it alone: yaw
    changed in its last bits changes the iteration count of most planted egos (drops and dependent rows; the adds and the largest
    working set stay) and of no solvable ego -- tests/test_active_set_cpu.py, test_the_way_to_the_exit_is_decided_by_rounding.
    So the first differing decision of a planted ego is a drop at a noise-sized r_k; the status, which is what the reference
    defines, is identical.  The solvable egos are held to test_step_vs_oracle's 0.9 on their own."""
    B = step_batch(size, cu_count())
    base = _base(pkg, T)
    batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    dbg = debug_bufs(eng, 2 * T)
    eng.solve(torch.from_numpy(batch.x0).cuda(), debug=dbg)
    torch.cuda.synchronize()
    _, _, same = _check_step(pkg, oracle, routes, eng, dbg, batch, cfgs, which, "step")
    assert same >= N_ITER_SAME, same


def _snap(eng, loop, **more):
    rec = loop.recorder
    out = {k: getattr(eng, k).clone() for k in NAMES}
    out.update(x0=loop.x0.clone(), hist=loop.hist.clone(), age=loop.age.clone(), n_respawn=loop.n_respawn.clone(),
               tick=loop.tick_counter.clone(), rec=rec.rec.clone(), flags=rec.flags.clone(), path_len=eng.path_len.clone())
    out.update({k: v.clone() for k, v in more.items()})
    return out


BY_TICK = ("hist", "rec", "flags")            # [ticks, B, ..]; the other per-ego buffers are [B, ..]
WHOLE = ("n_respawn", "tick", "obs", "get", "rec_obs")


def _same(a, b, where, egos=None):
    """Two snapshots bit for bit; egos: only these egos' rows (and not the batch-wide counters)."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if egos is not None:
            if k in ("n_respawn",):
                continue
            if k not in WHOLE:
                x, y = (x.index_select(1, egos), y.index_select(1, egos)) if k in BY_TICK else (x.index_select(0, egos), y.index_select(0, egos))
        assert _eq(x, y), (k, where)


def _planted_brake(snap, cfgs, B, K, where):
    """From the History records: a planted ego fails on every tick, brakes with its own row's MAX_DECEL (+0.5 for an A row) and
    keeps its steering -- LOOP_DI until the age limit respawns it, 0 from then on."""
    ea, eb = AC.planted(B)
    rec, flags = snap["rec"][:K].cpu().numpy(), snap["flags"][:K].cpu().numpy()
    for e in np.concatenate([ea, eb]):
        assert np.all(flags[:, e] & 1), (where, e, flags[:, e])
        assert np.all(rec[:, e, 5] == cfgs[e].MAX_DECEL), (where, e, rec[:, e, 5])
        want_di = np.where(np.arange(K) < LOOP_MAX_AGE, LOOP_DI, 0.0)     # the respawn at the end of tick LOOP_MAX_AGE - 1 clears it
        assert np.array_equal(rec[:, e, 4], want_di), (where, e, rec[:, e, 4])
        assert np.array_equal(snap["hist"][:K, e].cpu().numpy(), rec[:, e, 4:6]), (where, e)
    assert rec[0, PLANT_FAIL, 5] == PLANT_DECEL and flags[0, PLANT_FAIL] & 1, where
    return int((flags & 1).sum())


def _loop(pkg, routes, batch, cfgs, base, K, specs=None):
    """A loop on the mixed batch with the table set and every ego's applied steering preset to LOOP_DI (what a failing ego keeps):
    ClosedLoop, or with specs the ScenarioLoop with those scripted vehicles."""
    eng = engine(pkg, routes, batch, base.T, config=base)
    eng.set_ego_configs(cfgs)
    eng.di_ai[:, 0] = LOOP_DI
    x0 = torch.from_numpy(batch.x0).cuda()
    if specs is None:
        loop = pkg.ClosedLoop(eng, x0, hist_cap=K, max_age=LOOP_MAX_AGE, record=K)
        return eng, loop, loop
    sc = pkg.ScenarioLoop(eng, x0, specs, hist_cap=K, max_age=LOOP_MAX_AGE, record=K)
    return eng, sc.loop, sc


@pytest.mark.parametrize("T,size", CLOSED_CASES)
def test_closed_loop_mixed_batch(pkg, oracle, routes, T, size):
    """(b) K ticks of ClosedLoop on the mixed batch, on every row without the glue and on the LDS kernel.
    Tick by tick against oracle.closed_loop_per_config, both free-running from the same start: the visited states and the applied
    controls of every ego within 1e-7 after every tick (the bar of test_closed_loop_visited_states_against_oracle), target_ind
    equal, and the device's count of failed ticks equal to the oracle's n_fail.  A planted ego fails on every tick, brakes with its
    own row's MAX_DECEL and keeps its steering.  jsim_mpc_run_ticks (fused) equals the ticked run byte for byte, iteration totals
    included; the planted egos' totals show they iterated on every tick.  The neighbours are unharmed: the same batch with every
    planted row replaced by the stock row, under which those egos solve, gives every other ego the same bytes."""
    B, K = loop_batch(size, cu_count()), loop_ticks(T)
    base = _base(pkg, T)
    batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
    ea, eb = AC.planted(B)
    pl = np.concatenate([ea, eb])
    # tick by tick, the oracle beside it
    e1, l1, _ = _loop(pkg, routes, batch, cfgs, base, K)
    ps = oracle_params_list(oracle, cfgs, which)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    state = oracle.loop_state_from_batch(batch, T)
    state["di_ai"][:, 0] = LOOP_DI
    iters = torch.zeros(B, dtype=torch.int64, device=e1.device)
    n_fail, worst_x, worst_u = 0, 0.0, 0.0
    for k in range(K):
        l1.tick()
        iters += e1.n_iter
        it = e1.n_iter.cpu().numpy()[pl]
        assert np.all(it >= 2) and np.all(it <= max_iters(T)), (k, it)              # iterated before failing, this tick too; not the cap
        r = oracle.closed_loop_per_config(ps, which, state, cx, cy, cyaw, off, 1, max_age=LOOP_MAX_AGE, n_threads=16)
        n_fail += r["n_fail"]
        worst_x = max(worst_x, float(np.abs(l1.x0.cpu().numpy() - state["x0"]).max()))
        worst_u = max(worst_u, float(np.abs(l1.hist[k].cpu().numpy() - r["hist"][0]).max()))
        assert np.array_equal(e1.target_ind.cpu().numpy(), state["target_ind"]), k
        assert np.array_equal(l1.age.cpu().numpy(), state["age"]), k
    torch.cuda.synchronize()
    s1 = _snap(e1, l1)
    failed = _planted_brake(s1, cfgs, B, K, "host ticks")
    print(f"loop T={T} B={B} K={K}: failed ticks {failed} (oracle {n_fail}, planted egos {len(pl)}), worst |dx| {worst_x:.2e}, "
          f"worst |d(di, ai)| {worst_u:.2e}, planted iteration totals {int(iters[pl].min())}..{int(iters[pl].max())}")
    assert worst_x <= 1e-7 and worst_u <= 1e-7, (worst_x, worst_u)
    assert failed == n_fail and failed >= K * len(pl) + 1
    # fused
    e2, l2, _ = _loop(pkg, routes, batch, cfgs, base, K)
    l2.run(2); l2.run(K - 2)
    torch.cuda.synchronize()
    s2 = _snap(e2, l2)
    _same(s1, s2, "fused")
    tot = iter_totals(e2)
    assert np.array_equal(tot, iters.cpu().numpy()) and np.all(tot[pl] >= 2 * K)
    # the neighbours
    batch3, cfgs3, _ = AC.mixed_case(pkg.synth, routes, base, B, T, plant=False)
    assert all(np.array_equal(getattr(batch, f), getattr(batch3, f)) for f in ("x0", "path_id", "target_ind", "oa", "od"))
    e3, l3, _ = _loop(pkg, routes, batch3, cfgs3, base, K)
    l3.run(2); l3.run(K - 2)
    torch.cuda.synchronize()
    s3 = _snap(e3, l3)
    others = torch.from_numpy(np.setdiff1d(np.arange(B), pl)).cuda()
    _same(s2, s3, "neighbours", egos=others)
    assert int((s3["flags"][:K, torch.from_numpy(pl).cuda()] & 1).sum()) == 0      # the replaced rows do solve


@pytest.mark.parametrize("T,size", SCENARIO_CASES)
def test_scenario_loop_mixed_batch(pkg, routes, W, T, size):
    """(b) on the rows with the glue inside: K ticks of ScenarioLoop with workloads.OBSTACLE_SPECS on the mixed batch.
    jsim_loop_run_scenario equals the same ticks driven from the host byte for byte -- every buffer, History record and the
    iteration totals; a planted ego fails on every tick, brakes with its own row's MAX_DECEL and keeps its steering; and the
    neighbours of the planted egos get the same bytes when the planted rows are replaced by the stock row."""
    B, K = loop_batch(size, cu_count()), loop_ticks(T)
    base = _base(pkg, T)
    ea, eb = AC.planted(B)
    pl = np.concatenate([ea, eb])
    snaps, iters = [], []
    for how in ("host ticks", "fused", "neighbours"):
        batch, cfgs, _ = AC.mixed_case(pkg.synth, routes, base, B, T, plant=how != "neighbours")
        eng, loop, sc = _loop(pkg, routes, batch, cfgs, base, K, specs=W.OBSTACLE_SPECS)
        if how == "host ticks":
            n = torch.zeros(B, dtype=torch.int64, device=eng.device)
            for _ in range(K):
                sc.tick()
                n += eng.n_iter
            iters.append(n.cpu().numpy())
        else:
            sc.run(2); sc.run(K - 2)
            iters.append(iter_totals(eng))
        torch.cuda.synchronize()
        snaps.append(_snap(eng, loop, traj_idx=sc.pre.traj_idx, prev_len=sc.pre.prev_len, col=sc.pre.col_flag, pst=sc.pre.status,
                           obs=sc.obst.state, get=sc.obst.get_buf, rec_obs=sc.recorder.obs))
        if how != "neighbours":
            failed = _planted_brake(snaps[-1], cfgs, B, K, how)
            assert failed >= K * len(pl) + 1
    _same(snaps[0], snaps[1], "fused")
    assert np.array_equal(iters[0], iters[1]) and np.all(iters[1][pl] > 0)
    print(f"scenario T={T} B={B} K={K}: failed ticks {failed}, planted iteration totals {int(iters[1][pl].min())}..{int(iters[1][pl].max())}, "
          f"largest total of an ego {int(iters[1].max())}")
    others = torch.from_numpy(np.setdiff1d(np.arange(B), pl)).cuda()
    _same(snaps[1], snaps[2], "neighbours", egos=others)
    assert np.array_equal(iters[1][others.cpu().numpy()], iters[2][others.cpu().numpy()])
    assert int((snaps[2]["flags"][:K, torch.from_numpy(pl).cuda()] & 1).sum()) == 0


@pytest.mark.parametrize("T,B", MAX_ITER_SHAPES)
def test_max_iter_passes_mixed_batch(pkg, oracle, routes, T, B):
    """(c) MAX_ITER = 3 on the mixed batch (the pattern of test_max_iter_relinearisation_passes, which plants only a v0 failure):
    a planted ego fails in the loop on the first pass and the failure stands through the later passes -- its n_iter is the first
    pass's alone, equal to what one pass of the same batch counts -- while its neighbours go through three passes against the
    oracle's three.  The bars of (a); u* within 1e-6 here too: every pass solves under the tight limits, around the pass before."""
    base = _base(pkg, T, MAX_ITER=3)
    batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
    outs = {}
    for passes in (3, 1):
        c = [replace(x, MAX_ITER=passes) for x in cfgs]
        eng = engine(pkg, routes, batch, T, config=replace(base, MAX_ITER=passes))
        eng.set_ego_configs(c)
        eng.solve(torch.from_numpy(batch.x0).cuda())
        torch.cuda.synchronize()
        ref, n_iter, same = _check_step(pkg, oracle, routes, eng, None, batch, c, which, f"MAX_ITER={passes}")
        assert same >= N_ITER_SAME, same
        outs[passes] = (ref, n_iter)
    pl = np.concatenate(AC.planted(B))
    assert np.array_equal(outs[3][1][pl], outs[1][1][pl]) and np.array_equal(outs[3][0]["trace"][pl], outs[1][0]["trace"][pl])
    ok = outs[3][0]["status"] == 0
    assert np.abs(outs[3][0]["oa"] - outs[1][0]["oa"])[ok].max() > 1e-3 and outs[3][1][ok].sum() > outs[1][1][ok].sum()   # the extra passes matter
