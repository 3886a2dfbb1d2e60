"""The solve under the weights of the reference's sensitivity study -- zeros included -- and on the Hessians they make: every
single-step register kernel at every dispatch boundary, the LDS kernel and the acceleration-state variant, certified against an
exact-arithmetic reference.  Run with -m gpu on an MI355X.

The cases are tests/conditioning_cases.py (30 sweep rows + 4 extreme rows, 3 states each; classes "pd" / "singular" written
there, for the stock model and for the acceleration-state variant, and proved by tests/test_conditioning_cpu.py), laid out one ego
per case through set_ego_configs -- the weights as they are, zeros included -- and tiled cyclically up to the batch size at which
the dispatch takes the kernel (a four-wave row's 97 egos hold fewer than the 102 cases: it runs the list from both ends).

Per kernel, one solve with debug buffers and one without:
  * status, oa, od, active_mask of the plain run == the debug run bit for bit (what is certified is the production instantiation);
  * tiled copies == the first copy bit for bit (H, g, multipliers included);
  * every status in {0, 1}; every output finite where the status is 0;
  * class "pd": status and active set == the oracle's; the certificate (tests/qp_exact.py, exact arithmetic on the kernel's own
    H, g and the rows of gpu_helpers.qp_constraints): feasibility, multipliers >= 0, duality-gap bound; u* and the multipliers of
    the active rows against the exact solve on the active set;
  * class "singular": status 0 implies that the certificate passes (whatever H's rank, it bounds f(u) - f*).
No status-0 ego skips the certificate: a tiled copy IS the first copy, bit for bit.  Bars: for each case the oracle's own figure
(gap, primal violation, distance from the exact solve of ITS problem) x 16 -- another summation order, fast_rsqrt's <= 1 ulp --
with a floor of 1e-13 max(1, |value|) (conditioning_cases.bar); both sides are printed.
The acceleration-state variant's decision vector has a free acc_0 behind the 2T inputs which the step does not return; it is
recovered from the predicted speeds (v_1 = v_0 + dt (acc_0 + u0_0)), for the oracle's yardstick in the same way.

Kernels of one horizon agree on the statuses of the singular cases (one test runs them side by side).  The kernels with the loop
glue inside have no single-step entry: they run the first tick of a ScenarioLoop without traffic, whose applied controls are held
against the exact solve.  The sweep's own run -- 10 closed-loop ticks from the standstill under all 30 rows -- fused equals tick
by tick, is finite, and follows the oracle's closed loop under every row whose first tick is "pd"."""
import importlib
from dataclasses import replace

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import conditioning_cases as CC
import qp_exact as QX
import refqp_tools as RT
from gpu_helpers import (cu_count, debug_bufs, engine, oracle_params, oracle_params_list, qp_constraints, variant_batches, variant_id)

pytestmark = pytest.mark.gpu
CFG = importlib.import_module(PKG_NAME + ".config")
NON_PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if not r[2])
PRE_ROWS = tuple(r for r in CFG.REG_VARIANTS if r[2])
N = len(CC.CASES)
STEP_CASES = ([pytest.param(r[1], (r, k), "stock", id=variant_id(r) + (f"-b{k}" if k else ""))
               for r in NON_PRE_ROWS for k in range(len(variant_batches(r, 256)))] +
              [pytest.param(24, 2 * N + 5, "stock", id="lds-T24"), pytest.param(13, 2 * N + 5, "jerk", id="jerk-T13")])
DT = 0.2
_YARD = {}


def _base(pkg, kind, T):
    return replace(pkg.mpc_jerk.config if kind == "jerk" else pkg.MPCConfig.from_json(), T=T)


def _batch_size(size):
    """The batch size of a case: fixed, or variant_batches(row, this device's CU count)[k], where the dispatch takes the row."""
    if isinstance(size, int):
        return size
    row, k = size
    return variant_batches(row, cu_count())[k]


def _constraints(batch, cfgs, T, base, kind):
    return qp_constraints(T, DT, batch.x0[:, 2], batch.speed, cfgs, base.MIN_SPEED, base.MAX_STEER_RAD, jerk=kind == "jerk")


def _widths(batch, cfgs, b, T, base, kind):
    return CC.box_widths(cfgs[b], T, base.MAX_STEER_RAD, jerk=(batch.speed[b], base.MIN_SPEED, DT) if kind == "jerk" else None)


def yardstick(oracle, pkg, routes, T, kind="stock"):
    """Per case name, for a horizon and kind (cached): the oracle's step and, where its status is 0, conditioning_cases.measure of
    it -- with the exact solve for the "pd" cases."""
    if (kind, T) not in _YARD:
        base = _base(pkg, kind, T)
        batch, cfgs, _, cases = CC.make_batch(pkg.synth, routes, T, N, base)
        G, h = _constraints(batch, cfgs, T, base, kind)
        out = {}
        for b, c in enumerate(cases):
            r = CC.oracle_step(oracle, oracle_params(oracle, cfgs[b]), routes, batch, b)
            pd = CC.cls_of(c, kind) == "pd"
            assert r["status"] == 0 or not pd, c.name
            if r["status"] == 0:
                r["m"] = CC.measure(QX, r["H"], r["g"], G, h[b], r["u"], r["lam"], r["active"], _widths(batch, cfgs, b, T, base, kind), exact=pd)
                assert CC.certificate_passes(r["m"]) and not (pd and r["m"]["singular"]), c.name
            out[c.name] = r
        _YARD[(kind, T)] = out
    return _YARD[(kind, T)]


def _run(pkg, routes, batch, cfgs, T, base, n, debug):
    eng = engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    dbg = debug_bufs(eng, n) if debug else None
    eng.solve(torch.from_numpy(batch.x0).cuda(), debug=dbg)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy() for k in ("status", "oa", "od", "active_mask", "ox", "oy", "ov", "oyaw", "n_iter", "target_ind")}
    if debug:
        out.update({k: v.cpu().numpy() for k, v in dbg.items()})
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _answer(dbg, b, kind):
    """(u, H) of ego b of a debug run: the decision vector (acc_0 recovered under the acceleration-state variant) and the symmetric H."""
    u = np.stack([dbg["oa"][b], dbg["od"][b]], axis=1).reshape(-1)
    if kind == "jerk":
        u = CC.with_acc0(u, dbg["oa"][b][0], dbg["ov"][b], DT)
    return u, QX.symmetric(dbg["H"][b])


def _launch_and_check(pkg, routes, T, B, base, kind, cases):
    """One debug and one plain solve of B egos tiled from `cases`; the bit-for-bit and finiteness properties; returns what the
    certification needs."""
    batch, cfgs, which, cases = CC.make_batch(pkg.synth, routes, T, B, base, cases=cases)
    n = 2 * T + (1 if kind == "jerk" else 0)
    dbg, plain = _run(pkg, routes, batch, cfgs, T, base, n, True), _run(pkg, routes, batch, cfgs, T, base, n, False)
    for k in ("status", "oa", "od", "active_mask"):                      # what is certified is the production instantiation
        assert np.array_equal(_bits(plain[k]), _bits(dbg[k])), k
    first = np.arange(B) % len(cases)
    for k, v in dbg.items():                                             # a tiled copy is the first copy
        assert np.array_equal(_bits(v), _bits(v[first])), k
    st = dbg["status"]
    assert np.all((st == 0) | (st == 1)), np.unique(st)
    ok = st == 0
    for k in ("oa", "od", "ox", "oy", "ov", "oyaw", "H", "g", "lam"):
        assert np.all(np.isfinite(dbg[k][ok])), k
    assert np.all(dbg["oa"][~ok] == 0) and np.all(dbg["od"][~ok] == 0)   # a failed solve: cold start next tick
    G, h = _constraints(batch, cfgs, T, base, kind)
    return batch, cfgs, cases, dbg, G, h


def _certify(c, kind, T, base, batch, cfgs, b, dbg, G, h, yard, worst):
    """Ego b (the first copy of case c) against its class's rule."""
    st = int(dbg["status"][b])
    act = list(np.flatnonzero(RT.active_bits(dbg["active_mask"][b:b + 1], 8 * T)[0]))
    D = _widths(batch, cfgs, b, T, base, kind)
    if CC.cls_of(c, kind) == "singular":                                 # status 0 implies the certificate passes
        if st == 0:
            u, H = _answer(dbg, b, kind)
            m = CC.measure(QX, H, dbg["g"][b], G, h[b], u, dbg["lam"][b], act, D, exact=False)
            print(f"{kind} T={T} {c.name:16s} singular status 0 (oracle {yard[c.name]['status']}): gap={m['gap']:.1e} primal={m['primal']:.1e} f={m['f']:.3e}")
            assert CC.certificate_passes(m), (c.name, m)
        else:
            print(f"{kind} T={T} {c.name:16s} singular status {st} (oracle {yard[c.name]['status']})")
        return
    r = yard[c.name]
    assert st == 0 and act == r["active"], (c.name, st)
    u, H = _answer(dbg, b, kind)
    m = CC.measure(QX, H, dbg["g"][b], G, h[b], u, dbg["lam"][b], act, D)
    o = r["m"]
    bars = dict(gap=CC.bar(o["gap"], o["f"]), primal=CC.bar(o["primal"], np.abs(h[b]).max()), err_u=CC.bar(o["err_u"], o["u_max"]),
                err_lam=CC.bar(o["err_lam"], o["lam_max"]))
    print(f"{kind} T={T} {c.name:16s} pd       " + " ".join(f"{k}={m[k]:.1e} (oracle {o[k]:.1e}, bar {bars[k]:.1e})" for k in bars))
    assert not m["singular"] and m["lam_min"] >= 0.0 and CC.certificate_passes(m), (c.name, m)
    for k in bars:
        assert m[k] <= bars[k], (c.name, k, m[k], o[k], bars[k])
        worst[k] = max(worst[k], m[k] / bars[k])


@pytest.mark.parametrize("T,size,kind", STEP_CASES)
def test_step_certified_under_the_sweep_weights(pkg, oracle, routes, T, size, kind):
    B, base = _batch_size(size), _base(pkg, kind, T)
    yard = yardstick(oracle, pkg, routes, T, kind)
    worst, done = dict(gap=0.0, primal=0.0, err_u=0.0, err_lam=0.0), set()
    for order in ((CC.CASES,) if B >= N else (CC.CASES, CC.CASES[::-1])):       # fewer egos than cases: the list from both ends
        batch, cfgs, cases, dbg, G, h = _launch_and_check(pkg, routes, T, B, base, kind, order)
        for b in range(min(B, N)):                                       # the first copy of every case; the others are it, bit for bit
            if cases[b].name not in done:
                _certify(cases[b], kind, T, base, batch, cfgs, b, dbg, G, h, yard, worst)
                done.add(cases[b].name)
    assert len(done) == N
    print(f"{kind} T={T} B={B}: largest figure / bar {worst}")


SINGULAR_CASES = tuple(c for c in CC.CASES if c.cls == "singular")


@pytest.mark.parametrize("T", (13, 20, 40))
def test_kernels_of_one_horizon_agree_on_the_singular_statuses(pkg, routes, monkeypatch, T):
    """The six singular cases, R entries of exactly 0 included (an exactly zero pivot: the factorisations' clamp), on every
    single-step register kernel of the horizon at every dispatch boundary and on the LDS kernel at the same horizon
    (JSIM_FORCE_LDS_KERNEL), side by side: the same status for every case on every kernel, and the properties of the step test."""
    base = _base(pkg, "stock", T)
    sizes = [(variant_id(r) + f"-b{k}", B) for r in NON_PRE_ROWS if r[1] == T for k, B in enumerate(variant_batches(r, cu_count()))]
    seen = {}
    for name, B in sizes + [("lds", 2 * len(SINGULAR_CASES))]:
        if name == "lds":
            monkeypatch.setenv("JSIM_FORCE_LDS_KERNEL", "1")
        batch, cfgs, cases, dbg, G, h = _launch_and_check(pkg, routes, T, B, base, "stock", SINGULAR_CASES)
        seen[name] = dbg["status"][:len(cases)].tolist()
        for b, c in enumerate(cases):
            if dbg["status"][b] == 0:
                u, H = _answer(dbg, b, "stock")
                assert CC.certificate_passes(QX.certificate(H, dbg["g"][b], G, h[b], u, dbg["lam"][b], _widths(batch, cfgs, b, T, base, "stock"))), (name, c.name)
    print(f"T={T}: statuses of {[c.name for c in SINGULAR_CASES]}: {seen}")
    assert len(seen) >= 2 and len({tuple(v) for v in seen.values()}) == 1, seen


@pytest.mark.parametrize("T,row", [pytest.param(r[1], r, id=variant_id(r)) for r in PRE_ROWS])
def test_glue_kernels_first_tick_under_the_sweep_weights(pkg, oracle, routes, T, row):
    """The kernels with the loop glue inside, which have no single-step entry: the first tick of a ScenarioLoop without traffic
    (the glue then leaves the path alone) is the step of the case's state.  Its applied controls (steer, acceleration) of every
    "pd" case against the exact solve's first inputs under the bars of the step test; everything finite; tiled copies bit for
    bit; fused equals tick by tick."""
    B, base = variant_batches(row, cu_count())[0], _base(pkg, "stock", T)
    yard = yardstick(oracle, pkg, routes, T)
    worst, done = 0.0, set()
    for order in ((CC.CASES,) if B >= N else (CC.CASES, CC.CASES[::-1])):       # fewer egos than cases: the list from both ends
        batch, cfgs, which, cases = CC.make_batch(pkg.synth, routes, T, B, base, cases=order)
        G, h = _constraints(batch, cfgs, T, base, "stock")
        hist = []
        for fused in (True, False):
            eng = engine(pkg, routes, batch, T, config=base)
            eng.set_ego_configs(cfgs)
            sc = pkg.ScenarioLoop(eng, torch.from_numpy(batch.x0).cuda(), [], hist_cap=2, max_age=0)
            if fused:
                sc.run(2)
            else:
                sc.tick(); sc.tick()
            torch.cuda.synchronize()
            hist.append(sc.loop.hist[:2].cpu().numpy())
        assert np.array_equal(_bits(hist[0]), _bits(hist[1])) and np.all(np.isfinite(hist[0]))
        first = np.arange(B) % N
        assert np.array_equal(_bits(hist[0]), _bits(hist[0][:, first]))
        for b, c in enumerate(cases[:min(B, N)]):
            done.add(c.name)
            if c.cls != "pd":
                continue
            r = yard[c.name]
            ue, _, _ = QX.solve_on(r["H"], r["g"], G, h[b], r["active"])
            d = max(abs(hist[0][0, b, 0] - ue[1]), abs(hist[0][0, b, 1] - ue[0]))           # (di, ai) = (delta_0, a_0)
            lim = CC.bar(r["m"]["err_u"], r["m"]["u_max"])
            assert d <= lim, (c.name, d, lim)
            worst = max(worst, d / lim)
    assert len(done) == N
    print(f"T={T} B={B} {variant_id(row)}: first-tick controls against the exact solve, largest error / bar {worst:.2f}")


@pytest.mark.parametrize("T", (13, 20))
def test_standstill_sweep_closed_loop(pkg, oracle, routes, T):
    """The sweep's own run: 10 closed-loop ticks from state a under all 30 rows.  jsim_mpc_run_ticks equals tick by tick bit for
    bit; every record is finite; under every row whose first tick is "pd" the applied controls follow the oracle's closed loop
    within 1e-7 (the bar of the free-running loops of tests/test_gpu_active_set.py) and the ego drives off."""
    K, base = 10, _base(pkg, "stock", T)
    cases = CC.SWEEP_CASES_A
    B = len(cases)
    batch, cfgs, which, _ = CC.make_batch(pkg.synth, routes, T, B, base, cases=cases)
    snaps = []
    for fused in (False, True):
        eng = engine(pkg, routes, batch, T, config=base)
        eng.set_ego_configs(cfgs)
        loop = pkg.ClosedLoop(eng, torch.from_numpy(batch.x0).cuda(), hist_cap=K, max_age=0, record=K)
        if fused:
            loop.run(K // 2 - 1); loop.run(K - (K // 2 - 1))
        else:
            for _ in range(K):
                loop.tick()
        torch.cuda.synchronize()
        snaps.append(dict(hist=loop.hist.cpu().numpy(), x0=loop.x0.cpu().numpy(), rec=loop.recorder.rec.cpu().numpy(),
                          flags=loop.recorder.flags.cpu().numpy(), status=eng.status.cpu().numpy(), oa=eng.oa.cpu().numpy(),
                          od=eng.od.cpu().numpy(), target_ind=eng.target_ind.cpu().numpy()))
    for k in snaps[0]:
        assert np.array_equal(_bits(snaps[0][k]), _bits(snaps[1][k])), k
    s = snaps[0]
    assert np.all(np.isfinite(s["hist"])) and np.all(np.isfinite(s["rec"])) and np.all(np.isfinite(s["x0"]))
    ps = oracle_params_list(oracle, cfgs, which)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    state = oracle.loop_state_from_batch(batch, T)
    r = oracle.closed_loop_per_config(ps, which, state, cx, cy, cyaw, off, K, max_age=0, n_threads=8)
    d = np.abs(s["hist"] - r["hist"]).max(axis=(0, 2))
    dx = np.abs(s["x0"] - state["x0"]).max(axis=1)
    for b, c in enumerate(cases):
        print(f"T={T} {c.name:16s} {c.cls:8s} |d(di, ai)| {d[b]:.1e} |dx| {dx[b]:.1e} v after {K} ticks {s['x0'][b, 2]:.3f} (oracle {state['x0'][b, 2]:.3f})")
    pd = np.array([c.cls == "pd" for c in cases])
    assert pd.sum() == B - 1 and np.all(s["status"][pd] == 0) and d[pd].max() <= 1e-7 and dx[pd].max() <= 1e-7, (d, dx)
    # drove off: at most 2 m/s^2 for 2 s; the oracle's slowest row (R_acc = 10) reaches 1.76 m/s; without w_para nothing pulls forward
    moves = np.array([c.row != "w_para=0" for c in cases])
    assert np.all(s["x0"][pd & moves, 2] > 1.0) and np.all(np.abs(s["x0"][~moves, 2]) < 1e-6), s["x0"][:, 2]
