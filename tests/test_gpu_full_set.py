"""The active-set loop at a working set of all 2T variables, on every kernel.  Run with -m gpu on an MI355X.

The full set is the last index of every per-position structure of the solvers: the last column of R, the last working-set
position's multiplier and row id, the Householder reflection on a trailing block of one element, an active mask with 2T bits, and
in the four-wave kernels the last of 64 / 80 positions spread over waves and lane pairs.  The stock weights never bring a solve
there (the last acceleration moves only v_T, which costs nothing: 2T - 1 is where the off-path tight family ends); the full-set
family of tests/active_set_cases.py does, in three forms -- "drops" (hundreds of dependent rows and drops on the way, and hundreds
of iterations per batch that BEGIN at q = 2T: a violated row while every variable is bound, a pure dual step and a forced drop),
"adds" (2T adds and nothing else) and "mixed" (full-set rows and stock rows alternate through the per-ego table).  That the inputs
do this is proved on the oracle alone by tests/test_full_set_cpu.py, which also holds the oracle to an exact solve at the vertex.

The family has 48 .. 96 egos; a case tiles it cyclically up to the size at which the dispatch takes its kernel, and a tiled copy
must be the first copy bit for bit.

  (a) test_step_at_the_full_set          one step through the debug entry on every row without the glue at its first dispatch size
                                         (the one-wave row at T = 20 also below the two-waves-per-SIMD threshold), the LDS kernel
                                         at T = 24 and the acceleration-state variant (n = 2T + 1) at T = 13, against the oracle and
                                         against the exact vertex solve; plain run == debug run; a stock-row neighbour of the
                                         mixed batch gets the same bytes without the full-set rows
  (b) test_helper_form_equals_plain_form  with and without helper wavefronts, byte for byte (a child process)
  (c) test_closed_loop_at_the_full_set / test_scenario_loop_at_the_full_set
                                         six ticks: fused == tick by tick bit for bit, every host tick against the oracle on
                                         that tick's inputs

The mask and the iteration count are compared on the egos whose multipliers all lie a thousand activity thresholds above the
threshold (active_set_cases.margin_ok, evaluated on the oracle alone; at most a tenth of a batch is left out, asserted on the CPU)."""
import importlib
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import active_set_cases as AC
import conditioning_cases as CC
import full_set_child as CH
import qp_exact as QX
import test_gpu_active_set as GA
from conftest import PKG_NAME
from gpu_helpers import cu_count, debug_bufs, engine, kkt_check, n_active, qp_constraints, variant_batches, variant_id

pytestmark = pytest.mark.gpu
CFG = importlib.import_module(PKG_NAME + ".config")
NON_PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if not r[2])
PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if r[2])
FORMS = ("drops", "adds", "mixed")
LDS_T = 24
HELP_HORIZONS = CH.HORIZONS
K = 6
N_EXACT = 6


def _form_changes(row, k):
    """Whether a row's k-th dispatch boundary beyond the first is run: where the kernel of the sizes around it changes form -- the
    one-wave row of a horizon that also has the two-waves-per-SIMD form, just below that form's threshold."""
    return row[0] == 1 and row[3] == 1 and not row[4] and (1, row[1], row[2], 2, False) in CFG.REG_VARIANTS


# (T, row or fixed size, form, dispatch boundary, kind)
STEP_CASES = ([pytest.param(r[1], r, form, 0, "stock", id=f"{variant_id(r)}-{form}") for r in NON_PRE_ROWS for form in FORMS] +
              [pytest.param(r[1], r, "drops", k, "stock", id=f"{variant_id(r)}-b{k}-drops") for r in NON_PRE_ROWS
               for k in range(1, len(variant_batches(r, 256))) if _form_changes(r, k)] +
              [pytest.param(LDS_T, 0, form, 0, "stock", id=f"lds-T24-{form}") for form in FORMS] +
              [pytest.param(13, 0, "drops", 0, "jerk", id="jerk-T13-drops")])
CLOSED_CASES = [pytest.param(r[1], r, id=variant_id(r)) for r in NON_PRE_ROWS] + [pytest.param(LDS_T, 0, id="lds-T24")]
SCENARIO_CASES = [pytest.param(r[1], r, id=variant_id(r)) for r in PRE_ROWS] + [pytest.param(LDS_T, 0, id="lds-T24")]
STEP_KEYS = ("status", "target_ind", "n_iter", "active_mask", "oa", "od", "ox", "oy", "ov", "oyaw")
_REF = {}


def _base(pkg, T, kind="stock"):
    return replace(pkg.mpc_jerk.config if kind == "jerk" else pkg.MPCConfig.from_json(), T=T)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def reference(pkg, oracle, routes, T, form, kind="stock"):
    """(batch, cfgs, which, ref, exact) of the family at its own size (cached): the oracle's traced steps, and for the first N_EXACT
    full-set egos that keep the margin the oracle's figures against the exact vertex solve (conditioning_cases.measure)."""
    key = (T, form, kind)
    if key not in _REF:
        base = _base(pkg, T, kind)
        batch, cfgs, which = AC.full_set_case(pkg.synth, routes, base, AC.FULL_B[form], T, form)
        ref = AC.oracle_steps(oracle, routes, batch, cfgs, which)
        n = 2 * T + (1 if kind == "jerk" else 0)
        G, h = qp_constraints(T, pkg.synth.DT, batch.x0[:, 2], batch.speed, cfgs, base.MIN_SPEED, base.MAX_STEER_RAD, jerk=kind == "jerk")
        exact = {}
        for b in np.flatnonzero(AC.full_reached(oracle, ref, n) & AC.compared(ref))[:N_EXACT]:
            act = AC.active_rows(ref["active_mask"][b], 8 * T)
            exact[int(b)] = CC.measure(QX, QX.symmetric(ref["H"][b]), ref["g"][b], G, h[b], ref["u"][b], ref["lam"][b], act, _widths(batch, cfgs, b, T, base, kind))
        _REF[key] = (batch, cfgs, which, ref, exact)
    return _REF[key]


def _widths(batch, cfgs, b, T, base, kind):
    return CC.box_widths(cfgs[b], T, base.MAX_STEER_RAD, jerk=(batch.speed[b], base.MIN_SPEED, 0.2) if kind == "jerk" else None)


def _solve(pkg, routes, batch, cfgs, T, base, n, debug):
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    dbg = debug_bufs(eng, n) if debug else None
    eng.solve(torch.from_numpy(batch.x0).cuda(), debug=dbg)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy() for k in STEP_KEYS}
    if debug:
        out.update({k: v.cpu().numpy() for k, v in dbg.items()})
    return eng, dbg, out


def _against_oracle(out, ref, n, where, egos=slice(None)):
    """Status and target_ind identical; on the compared egos the mask bit for bit -- n bits where the oracle says so -- and the
    oracle's iteration count; u* within 1e-6 (the bar of tests/test_gpu_active_set.py for these limits).  Returns the figures."""
    keep = AC.compared(ref)
    st = out["status"][egos]
    assert np.array_equal(st, ref["status"]) and np.all(st == 0), (where, np.flatnonzero(st != ref["status"]))
    assert np.array_equal(out["target_ind"][egos], ref["target_ind"]), where
    mask = out["active_mask"][egos].view(np.uint32)
    assert np.array_equal(mask[keep], ref["active_mask"][keep]), (where, np.flatnonzero((mask != ref["active_mask"]).any(axis=1)))
    full = (n_active(ref["active_mask"]) == n) & keep
    assert np.all(n_active(mask)[full] == n), where
    same = out["n_iter"][egos] == ref["n_iter"]
    assert np.all(same[keep]), (where, np.flatnonzero(~same & keep), out["n_iter"][egos][~same], ref["n_iter"][~same])
    err = max(float(np.abs(out["oa"][egos] - ref["oa"]).max()), float(np.abs(out["od"][egos] - ref["od"]).max()))
    assert err <= 1e-6, (where, err)
    return dict(full=int(full.sum()), compared=int(keep.sum()), same_n_iter=float(same.mean()), err_u=err)


@pytest.mark.parametrize("T,size,form,k,kind", STEP_CASES)
def test_step_at_the_full_set(pkg, oracle, routes, T, size, form, k, kind):
    """(a), per kernel and form: status and target_ind identical to the oracle; active masks bit-exact on the compared egos, 2T bits
    where the oracle says so; n_iter the oracle's on every compared ego; u* within 1e-6; the KKT conditions of the kernel's own QP
    with per-ego limits; for six full-set egos u* and the multipliers of the kernel's own (H, g) against qp_exact's exact solve on
    the active set -- at the full set the solution of G_A u = h_A, whatever H and g -- within 16 x the oracle's own distance from
    it, floor 1e-13 max(1, |value|) ("Conditioning").  The plain run equals the debug run and a tiled copy the
    first copy bit for bit; in the mixed batch a stock-row ego gets the same bytes when the full-set rows are stock rows too."""
    base = _base(pkg, T, kind)
    n = 2 * T + (1 if kind == "jerk" else 0)
    fam, cfgs_f, which_f, ref, exact = reference(pkg, oracle, routes, T, form, kind)
    F = len(cfgs_f)
    B = variant_batches(size, cu_count())[k] if size else F
    batch, cfgs, which, first = AC.tile(fam, cfgs_f, which_f, B)
    eng, dbg, out = _solve(pkg, routes, batch, cfgs, T, base, n, True)
    _, _, plain = _solve(pkg, routes, batch, cfgs, T, base, n, False)
    for key in STEP_KEYS:                                                   # what is checked is the production instantiation
        assert np.array_equal(_bits(plain[key]), _bits(out[key])), key
    for key, v in out.items():                                              # a tiled copy is the first copy
        assert np.array_equal(_bits(v), _bits(v[first])), key
    fig = _against_oracle(out, ref, n, (T, form), egos=slice(0, F))
    if kind == "stock":
        kkt_check(eng, batch, dbg, cfgs)
    # the vertex
    G, h = qp_constraints(T, eng.dt, fam.x0[:, 2], fam.speed, cfgs_f, base.MIN_SPEED, base.MAX_STEER_RAD, jerk=kind == "jerk")
    worst = dict(err_u=0.0, err_lam=0.0)
    for b, o in exact.items():
        u = np.stack([out["oa"][b], out["od"][b]], axis=1).reshape(-1)
        if kind == "jerk":
            u = CC.with_acc0(u, out["oa"][b][0], out["ov"][b], eng.dt)
        act = AC.active_rows(out["active_mask"][b], 8 * T)
        m = CC.measure(QX, QX.symmetric(out["H"][b]), out["g"][b], G, h[b], u, out["lam"][b], act, _widths(fam, cfgs_f, b, T, base, kind))
        assert len(act) == n and not m["singular"] and m["lam_min"] >= 0.0 and CC.certificate_passes(m), (b, m)
        bars = dict(err_u=CC.bar(o["err_u"], o["u_max"]), err_lam=CC.bar(o["err_lam"], o["lam_max"]))
        for key, bar in bars.items():
            print(f"T={T} {form} ego {b}: {key}={m[key]:.1e} (oracle {o[key]:.1e}, bar {bar:.1e})")
            assert m[key] <= bar, (b, key, m[key], o[key], bar)
            worst[key] = max(worst[key], m[key] / bar)
    assert len(exact) == N_EXACT or kind == "jerk"
    print(f"step T={T} B={B} {form} {kind}: {fig}, longest solve {int(out['n_iter'].max())}, exact vertex solve on {len(exact)} egos: largest figure / bar {worst}")
    if form == "mixed":
        _, stock_cfgs, _ = AC.full_set_stock_case(pkg.synth, routes, base, F, T)
        _, _, alone = _solve(pkg, routes, batch, [stock_cfgs[i] for i in first], T, base, n, True)
        stock = which == 1
        for key, v in out.items():
            assert np.array_equal(_bits(v[stock]), _bits(alone[key][stock])), key
        assert not np.array_equal(out["oa"][~stock], alone["oa"][~stock])


@pytest.fixture(scope="module")
def plain_form(tmp_path_factory):
    """Every case of full_set_child in a child process with JSIM_HELP_MAX_B=0: one wave per ego, no helpers."""
    out = str(tmp_path_factory.mktemp("full_set") / "plain.npz")
    r = subprocess.run([sys.executable, os.path.abspath(CH.__file__), out], env=dict(os.environ, JSIM_HELP_MAX_B="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        d = {key: z[key] for key in z.files}
    assert str(d["help_max_b"]) == "0"
    return d


@pytest.mark.parametrize("T", HELP_HORIZONS)
def test_helper_form_equals_plain_form(pkg, routes, plain_form, T):
    """(b) The family at its own size (below one ego per CU: the kernel with helper wavefronts) against the same step in a process
    without helpers: outputs, H, g and multipliers byte for byte, in every form."""
    assert "JSIM_HELP_MAX_B" not in os.environ
    for form in FORMS:
        here = CH.step(pkg, routes, T, form)
        for key, v in here.items():
            w = plain_form[f"{form}_T{T}_{key}"]
            assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), (form, key)
        assert n_active(here["active_mask"].view(np.uint32)).max() == 2 * T and np.all(here["status"] == 0)


def _tick_inputs(eng, loop, F):
    """The first F egos' inputs of the tick to come, as an EgoBatch-like set of arrays."""
    return dict(x0=loop.x0[:F].cpu().numpy().copy(), target_ind=eng.target_ind[:F].cpu().numpy().copy(), oa=eng.oa[:F].cpu().numpy().copy(),
                od=eng.od[:F].cpu().numpy().copy())


def _tick_against_oracle(pkg, oracle, routes, eng, fam, cfgs_f, which_f, inp, F, where):
    """The tick just made against the oracle's step on the inputs the tick had (the path length as the glue left it)."""
    now = replace(fam, x0=inp["x0"], target_ind=inp["target_ind"], oa=inp["oa"], od=inp["od"], path_len=eng.path_len[:F].cpu().numpy().astype(fam.path_len.dtype))
    ref = AC.oracle_steps(oracle, routes, now, cfgs_f, which_f)
    out = {key: getattr(eng, key)[:F].cpu().numpy() for key in ("status", "target_ind", "n_iter", "active_mask", "oa", "od")}
    fig = _against_oracle(out, ref, 2 * eng.T, where)
    return fig, int(AC.full_reached(oracle, ref, 2 * eng.T).sum())


def _loops(pkg, oracle, routes, T, size, scenario):
    """(c) K ticks on the "drops" form tiled to the row's loop batch: host ticks (each against the oracle), then fused; bit for bit."""
    base = _base(pkg, T)
    fam, cfgs_f, which_f, _, _ = reference(pkg, oracle, routes, T, "drops")
    F = len(cfgs_f)
    B = GA.loop_batch(size, cu_count()) if size else F
    batch, cfgs, which, first = AC.tile(fam, cfgs_f, which_f, B)
    snaps, full = [], []
    for fused in (False, True):
        eng = engine(pkg, routes, batch, T, config=base)
        eng.set_ego_configs(cfgs)
        x0 = torch.from_numpy(batch.x0).cuda()
        if scenario:
            sc = pkg.ScenarioLoop(eng, x0, [], hist_cap=K, max_age=0, record=K)
            loop, drv = sc.loop, sc
        else:
            loop = drv = pkg.ClosedLoop(eng, x0, hist_cap=K, max_age=0, record=K)
        if fused:
            drv.run(2); drv.run(K - 2)
        else:
            worst = 0.0
            for k in range(K):
                inp = _tick_inputs(eng, loop, F)
                drv.tick()
                fig, nf = _tick_against_oracle(pkg, oracle, routes, eng, fam, cfgs_f, which_f, inp, F, (T, "tick", k))
                full.append(nf)
                worst = max(worst, fig["err_u"])
        torch.cuda.synchronize()
        more = dict(traj_idx=sc.pre.traj_idx, prev_len=sc.pre.prev_len, col=sc.pre.col_flag, pst=sc.pre.status) if scenario else {}
        snaps.append(GA._snap(eng, loop, **more))
    GA._same(snaps[0], snaps[1], "fused")
    assert int(snaps[0]["n_respawn"]) == 0 and int((snaps[0]["flags"][:K] & 1).sum()) == 0          # nobody respawned, nobody failed
    firsts = torch.from_numpy(first).cuda()
    for key in ("hist", "x0", "oa", "od", "active_mask", "n_iter"):                                 # a tiled copy is the first copy
        v = snaps[0][key]
        assert GA._eq(v, v.index_select(1 if key in GA.BY_TICK else 0, firsts)), key
    print(f"{'scenario' if scenario else 'closed'} loop T={T} B={B} K={K}: egos of {F} at the full set per tick (oracle on the tick's inputs) {full}, "
          f"worst |du| {worst:.2e}")
    assert 2 * full[0] >= F and 2 * sum(full[1:]) >= F, full


@pytest.mark.parametrize("T,size", CLOSED_CASES)
def test_closed_loop_at_the_full_set(pkg, oracle, routes, T, size):
    """(c) Six ticks of ClosedLoop on every row without the glue and on the LDS kernel: jsim_mpc_run_ticks equals tick by tick bit
    for bit in state, History and controller buffers; every host tick against the oracle's step on that tick's inputs -- status,
    mask and iteration count on the compared egos, u* within 1e-6; the full set is still reached on later ticks (the share the CPU
    test asserts on the oracle's own closed loop, here on the device's inputs)."""
    _loops(pkg, oracle, routes, T, size, False)


@pytest.mark.parametrize("T,size", SCENARIO_CASES)
def test_scenario_loop_at_the_full_set(pkg, oracle, routes, T, size):
    """(c) on the rows with the glue inside and on the LDS kernel's host ticks: six ticks of ScenarioLoop without traffic (the glue
    leaves the path alone); jsim_loop_run_scenario equals the host ticks bit for bit, the glue's buffers included; every host
    tick against the oracle as in the closed loop."""
    _loops(pkg, oracle, routes, T, size, True)
