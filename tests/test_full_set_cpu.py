"""The premises of tests/test_gpu_full_set.py, on the oracle alone: the full-set family of tests/active_set_cases.py does bring the
active-set loop to a working set of all 2T variables -- at every horizon with a register kernel and T = 24 (the LDS kernel), in every
form and at every family size the GPU cases use (they tile the family up to their kernel's dispatch size) -- and the oracle's answer
there is the vertex an exact solve gives.  Every choice of the family (start speed, draw) rests on what is printed here.

What the oracle's trace shows, and what is therefore asserted:
  * every family ego solves; at least half of a batch reach max_q == 2T and end with 2T active bits;
  * the "adds" form reaches it by 2T adds and nothing else on at least half of a batch (at T <= 24 and T = 40 a few further egos
    reach it with one or two drops: printed, and not counted);
  * the "drops" form meets, per batch, hundreds of dependent entering rows and drops (FLOORS["dependent"] of
    tests/test_active_set_cpu.py holds many times over).  Its drops leave from the middle of the working set: a drop at position 0
    does not occur at T >= 20 and one at the last position not at T = 24 .. 32, in 12 draws each -- those two floors stay with
    the off-path tight family, which test_active_set_cpu.py holds to them and to max_q == 2T - 1;
  * an iteration that BEGINS at q == 2T with a violated row (orc_trace.full_entering; the row depends on the working set by
    necessity: a pure dual step and a forced drop) is no rarity in the "drops" form: hundreds per batch.  The "adds" form has none.
"""
import importlib
from dataclasses import replace

import numpy as np
import pytest

import active_set_cases as AC
import conditioning_cases as CC
import qp_exact as QX
from conftest import PKG_NAME
from gpu_helpers import n_active, oracle_params_list, qp_constraints

CFG = importlib.import_module(PKG_NAME + ".config")
HORIZONS = tuple(sorted({r[1] for r in CFG.REG_VARIANTS} | {24}))
FORMS = ("drops", "adds", "mixed")
N_EXACT = 6                      # egos per horizon held against the exact vertex solve
LOOP_TICKS = 6
_FAMILY = {}


@pytest.fixture(scope="module")
def gpu_cases():
    """tests/test_gpu_full_set.py as a module: its parameter lists are plain data."""
    return importlib.import_module("test_gpu_full_set")


def _base(pkg, T, kind="stock"):
    return replace(pkg.mpc_jerk.config if kind == "jerk" else pkg.MPCConfig.from_json(), T=T)


def family(pkg, oracle, routes, T, form, kind="stock"):
    """(batch, cfgs, which, ref) of the family at its own size, the oracle's traced steps beside it (cached)."""
    key = (T, form, kind)
    if key not in _FAMILY:
        batch, cfgs, which = AC.full_set_case(pkg.synth, routes, _base(pkg, T, kind), AC.FULL_B[form], T, form)
        _FAMILY[key] = (batch, cfgs, which, AC.oracle_steps(oracle, routes, batch, cfgs, which))
    return _FAMILY[key]


def test_the_counter_counts_an_entering_row_at_a_full_working_set(oracle):
    """min |u - (5, 5)|^2 / 2 with u0 <= -1, u1 <= -1, u0 - u1 <= -1: the first two rows enter first (violated by 6, the third by
    0) and bind both variables (q = n = 2) at (-1, -1), where the third row is violated by 1 -- the iteration the counter counts.
    The row depends on the working set: a pure dual step drops the first row, and the optimum (-2, -1) holds rows two and three
    with multipliers 13 and 7.  Without the third row the counter stays 0 at the same q."""
    H, g = np.eye(2), np.array([-5.0, -5.0])
    G, h = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, -1.0]]), np.array([-1.0, -1.0, -1.0])
    t = oracle.TRACE
    st, u, lam, it, rec = oracle.solve_qp(H, g, G, h, trace=True)
    assert st == 0 and np.allclose(u, [-2.0, -1.0], atol=1e-14) and np.allclose(lam, [0.0, 13.0, 7.0], atol=1e-13)
    assert rec.tolist() == [3, 1, rec[t["drops_first"]], rec[t["drops_last"]], 1, 2, oracle.END_OPTIMAL, 1] and it == 4
    assert rec[t["drops_first"]] + rec[t["drops_last"]] == 1          # (which of the two positions row one holds is the entering order's)
    st, u, lam, it, rec = oracle.solve_qp(H, g, G[:2], h[:2], trace=True)
    assert st == 0 and rec.tolist() == [2, 0, 0, 0, 0, 2, oracle.END_OPTIMAL, 0] and it == 2


def test_builders_are_seeded_and_say_what_they_build(pkg, routes):
    T = 20
    base = _base(pkg, T)
    for form in FORMS:
        B = AC.FULL_B[form]
        assert 48 <= B <= 96
        one, two = (AC.full_set_case(pkg.synth, routes, base, B, T, form) for _ in range(2))
        assert all(np.array_equal(getattr(one[0], f), getattr(two[0], f)) for f in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od"))
        assert one[1] == two[1] and np.array_equal(one[2], two[2])
        batch, cfgs, which = one
        assert np.all(batch.x0[:, 2] == AC.full_v0(T)) and not batch.oa.any() and not batch.od.any()
        full = cfgs[0]
        assert (full.MAX_ACCEL, full.MAX_DECEL, full.Q_v_yaw, full.Qf, full.R) == (0.05, -0.05, [1.0, 0.5], [1.0, 1.0, 1.0, 0.5], [0.01, 1e-4])
        assert full.MAX_DSTEER == (3000.0 if form == "adds" else 0.4)
        if form == "mixed":
            assert np.array_equal(which, np.arange(B) % 2) and all(cfgs[b] == base for b in range(1, B, 2)) and all(cfgs[b] == full for b in range(0, B, 2))
            b2, c2, w2 = AC.full_set_stock_case(pkg.synth, routes, base, B, T)
            assert np.array_equal(b2.x0, batch.x0) and np.array_equal(w2, which) and all(c == base for c in c2)
        else:
            assert not which.any() and all(c == full for c in cfgs)
    tb, tc, tw, first = AC.tile(batch, cfgs, which, 257)
    assert len(tc) == 257 and np.array_equal(first, np.arange(257) % 96) and np.array_equal(tb.x0, batch.x0[first]) and tc[96] == cfgs[0]
    assert np.array_equal(tw, which[first]) and np.array_equal(tb.path_id[96:192], batch.path_id)


def test_every_kernel_row_has_a_full_set_case(gpu_cases):
    """A row of config.REG_VARIANTS without a full-set case fails here: the one-step cases cover the rows without the glue, the
    closed loops too, the scenario loops the rows with it; the helper form's horizons are those of the rows with helpers."""
    step = {p.values[1] for p in gpu_cases.STEP_CASES}
    closed = {p.values[1] for p in gpu_cases.CLOSED_CASES}
    scen = {p.values[1] for p in gpu_cases.SCENARIO_CASES}
    forms = {p.values[2] for p in gpu_cases.STEP_CASES}
    for row in CFG.REG_VARIANTS:
        if row[2]:
            assert row in scen, row
        else:
            assert row in step and row in closed, row
    assert forms == set(FORMS) and gpu_cases.LDS_T in {p.values[0] for p in gpu_cases.STEP_CASES if isinstance(p.values[1], int)}
    assert set(gpu_cases.HELP_HORIZONS) == set(CFG.HELP_HORIZONS) == {13, 15, 16, 20, 25}
    for row in CFG.REG_VARIANTS:              # a row's further dispatch boundaries are run where its kernel form changes there
        if not row[2] and row[0] == 1 and (1, row[1], False, 2, False) in CFG.REG_VARIANTS:
            assert {k for p in gpu_cases.STEP_CASES if p.values[1] == row for k in [p.values[3]]} >= {0, len(gpu_cases.variant_batches(row, 256)) - 1}, row


@pytest.mark.parametrize("T", HORIZONS)
def test_the_family_reaches_the_full_working_set(pkg, oracle, routes, T):
    t = oracle.TRACE
    n = 2 * T
    for form in FORMS:
        batch, cfgs, which, ref = family(pkg, oracle, routes, T, form)
        fam = which == 0
        tr = ref["trace"]
        full = AC.full_reached(oracle, ref, n)
        assert np.array_equal(full, (tr[:, t["max_q"]] == n) & (n_active(ref["active_mask"]) == n))
        tot = AC.trace_totals(oracle, tr[fam])
        entering = int(tr[:, t["full_entering"]].sum())
        clean = full & (tr[:, t["drops"]] == 0) & (ref["n_iter"] == n)
        keep = AC.compared(ref)
        print(f"T={T} {form} B={len(cfgs)} v0={AC.full_v0(T)}: full set on {int(full.sum())} of {int(fam.sum())} family egos ({int(clean.sum())} by 2T adds alone), "
              f"iterations beginning at q = 2T: {entering}, longest solve {int(ref['n_iter'].max())}, compared {int(keep.sum())} of {len(cfgs)}; {tot}")
        assert np.all(ref["status"] == 0) and np.all(tr[:, t["end"]] == oracle.END_OPTIMAL)
        assert np.all(tr[:, t["max_q"]] <= n) and not full[~fam].any()
        assert 2 * int(full.sum()) >= int(fam.sum()), (T, form, int(full.sum()))
        assert np.array_equal(tr[:, t["adds"]] + tr[:, t["drops"]], ref["n_iter"]) and np.all(tr[full, t["adds"]] - tr[full, t["drops"]] == n)
        assert (~keep).sum() <= AC.FULL_LEFT_OUT * len(cfgs), (T, form, int((~keep).sum()))
        assert 2 * int((full & keep).sum()) >= int(fam.sum())                              # the compared egos still hold the case
        if form == "adds":
            assert 2 * int(clean.sum()) >= int(fam.sum()), (T, int(clean.sum()))
            assert tot["dependent"] == 0 and entering == 0
            assert np.all(tr[clean, t["adds"]] == n)
        else:
            assert tot["dependent"] >= 20 and tot["drops"] >= int(fam.sum()) and ref["n_iter"][fam].max() > n, tot
            assert entering >= 100, entering                                                # the state after the full set: entered again
            assert np.all(tr[~fam, t["full_entering"]] == 0)
        if form == "mixed":                                      # the stock rows finish sooner and never fill the working set
            assert np.median(ref["n_iter"][~fam]) < np.median(ref["n_iter"][fam]) and tr[~fam, t["max_q"]].max() < n, (T, ref["n_iter"])


@pytest.mark.parametrize("T", HORIZONS)
def test_the_oracle_at_the_vertex_against_the_exact_solve(pkg, oracle, routes, T):
    """With 2T independent active rows u* solves G_A u = h_A whatever H and g are, and the multipliers solve G_A' lam = -(H u + g).
    qp_exact's KKT solve on the active set gives both (and gives the same u with H = I, g = 0: the vertex does not depend on the
    cost); its certificate bounds f(u) - f*.  Six full-set egos per horizon.  The bars of the oracle: G_A holds 1, -1 and
    multiples of dt, and a backward-stable solve then keeps u to a few hundred ulp of its size -- 1e-12 max(1, |u|) --; the
    multipliers carry H's conditioning through H u + g: 1e-9 max(1, |lam|), ten times under the ECOS tolerance the certificate is
    held to.  Two deliberately wrong restatements each change the result on every one of the six egos: the vertex solve without
    its last active row, and a mask without its last bit."""
    batch, cfgs, which, ref = family(pkg, oracle, routes, T, "drops")
    base = _base(pkg, T)
    n, m = 2 * T, 8 * T
    G, h = qp_constraints(T, pkg.synth.DT, batch.x0[:, 2], batch.speed, cfgs, base.MIN_SPEED, base.MAX_STEER_RAD)
    egos = np.flatnonzero(AC.full_reached(oracle, ref, n) & AC.compared(ref))[:N_EXACT]
    assert len(egos) == N_EXACT
    worst = dict(err_u=0.0, err_lam=0.0, gap=0.0, primal=0.0)
    for b in egos:
        act = AC.active_rows(ref["active_mask"][b], m)
        assert len(act) == n and np.linalg.matrix_rank(G[act]) == n
        H = QX.symmetric(ref["H"][b])
        mm = CC.measure(QX, H, ref["g"][b], G, h[b], ref["u"][b], ref["lam"][b], act, CC.box_widths(cfgs[b], T, base.MAX_STEER_RAD))
        assert not mm["singular"] and CC.certificate_passes(mm) and mm["infeasible"] <= 1e-12, (T, b, mm)
        assert mm["err_u"] <= 1e-12 * max(1.0, mm["u_max"]) and mm["err_lam"] <= 1e-9 * max(1.0, mm["lam_max"]), (T, b, mm)
        ue, le, _ = QX.solve_on(H, ref["g"][b], G, h[b], act)
        u_any, _, _ = QX.solve_on(np.eye(n), np.zeros(n), G, h[b], act)
        assert np.array_equal(ue, u_any)                                               # the vertex: G_A u = h_A alone
        assert np.abs(G[act] @ ue - h[b][act]).max() <= 1e-15 and le.min() > 0.0
        for k in worst:
            worst[k] = max(worst[k], mm[k])
        # wrong on purpose: the comparison sees the last position
        u_short, l_short, _ = QX.solve_on(H, ref["g"][b], G, h[b], act[:-1])
        assert np.abs(u_short - ref["u"][b]).max() > 1e6 * 1e-12 * max(1.0, mm["u_max"]), (T, b)
        short = ref["active_mask"][b].copy()
        short[act[-1] >> 5] &= ~np.uint32(1 << (act[-1] & 31))
        assert n_active(short[None])[0] == n - 1 and not np.array_equal(short, ref["active_mask"][b])
        thr = 1e-9 * max(1.0, float(np.abs(ref["g"][b]).max()))
        assert ref["lam"][b][act[-1]] > AC.FULL_MARGIN * thr                           # .. and the multiplier check of kkt_check would, too
    print(f"T={T}: the oracle against the exact vertex solve on egos {egos.tolist()}: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("T", HORIZONS)
def test_the_full_set_is_carried_over_the_ticks(pkg, oracle, routes, T):
    """Six ticks of the oracle's closed loop on the "drops" form, the solve of every tick traced on that tick's inputs: how many
    egos still reach the full set.  The first tick starts cold, the later ones from the tick before, at another speed (the
    family's reach depends on v0: FULL_V0): at T = 13, 15, 16, 25 and 40 nine egos in ten stay at the full set on every tick, at T = 20 until the
    last, at T = 24 six to ten of the 64, and at T = 30 and 32 the count swings between 0 and 58 from tick to tick (printed).
    Asserted: half of the batch on the first tick, and over the five later ticks together half a batch of ego-ticks."""
    batch, cfgs, which, _ = family(pkg, oracle, routes, T, "drops")
    ps = oracle_params_list(oracle, cfgs, which)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    state = oracle.loop_state_from_batch(batch, T)
    per_tick = []
    for k in range(LOOP_TICKS):
        now = oracle.mpc_step_batch_per_config(ps, which, state["x0"], state["path_id"], state["path_len"], state["speed"], cx, cy, cyaw,
                                               off, state["target_ind"], state["oa"], state["od"], n_threads=16, trace=True)
        assert np.all(now["status"] == 0), (T, k)
        per_tick.append(int(AC.full_reached(oracle, now, 2 * T).sum()))
        r = oracle.closed_loop_per_config(ps, which, state, cx, cy, cyaw, off, 1, max_age=0, n_threads=16)
        assert r["n_fail"] == 0 and r["n_respawn"] == 0, (T, k)
    print(f"T={T}: egos of {len(cfgs)} at the full set per tick {per_tick}")
    assert 2 * per_tick[0] >= len(cfgs) and 2 * sum(per_tick[1:]) >= len(cfgs), per_tick


def test_the_acceleration_state_variant(pkg, oracle, routes):
    """NX = 5 at T = 13 (n = 2T + 1: the free acc_0 behind the inputs).  From the trace: most egos end at q = 2T, the working set of
    all 2T + 1 variables is reached by one ego of 64 ("drops") and two of 48 ("adds"), and 13 iterations of the "drops" batch begin at
    q = n.  The family solves, and the egos compared on the GPU keep the margin."""
    T = 13
    t = oracle.TRACE
    for form in ("drops", "adds"):
        batch, cfgs, which, ref = family(pkg, oracle, routes, T, form, "jerk")
        q = ref["trace"][:, t["max_q"]]
        keep = AC.compared(ref)
        print(f"NX=5 T={T} {form}: largest working set {np.bincount(q)[2 * T - 2:].tolist()} egos at q = {2 * T - 2} .., iterations beginning at "
              f"q = n: {int(ref['trace'][:, t['full_entering']].sum())}, longest solve {int(ref['n_iter'].max())}, compared {int(keep.sum())} of {len(cfgs)}")
        assert np.all(ref["status"] == 0) and q.max() == 2 * T + 1 and 2 * int((q >= 2 * T).sum()) >= len(cfgs)
        assert (~keep).sum() <= AC.FULL_LEFT_OUT * len(cfgs)
