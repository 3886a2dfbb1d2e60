"""The CPU side of tests/test_gpu_conditioning.py: the proof, from the oracle and an exact-arithmetic reference alone, that the
cases of tests/conditioning_cases.py (the reference's sensitivity sweep, zeros included, and four rows beyond it) are what they claim.

  * the class of every case ("pd" / "singular") from the oracle's H at T = 13, 20, 24, 30, 40, and under the acceleration-state
    variant (NX = 5, its own list of singular cases) at T = 13;
  * the oracle's status on the singular cases, recorded as it is;
  * the oracle's condensed (H, g, G, h) against the problem the reference's own `_linear_mpc_control` emitted under every sweep
    row (tests/golden/sweep_qp.npz), x eliminated generically -- and that a weight of zero drops its term there;
  * the rows of G u <= h the tests build themselves, the acceleration-state variant's included, against the oracle's;
  * the oracle's certificate (qp_exact.certificate: stationarity, feasibility, multipliers, duality-gap bound) on every case it
    solves and, for every "pd" case, its distance from the exact solve on its final active set, printed for every case: the
    yardstick of the GPU bars (16 x these figures);
  * qp_exact itself against Fraction arithmetic."""
import importlib
from dataclasses import replace
from fractions import Fraction

import numpy as np
import pytest

from conftest import PKG_NAME, load_golden
import conditioning_cases as CC
import qp_exact as QX
import qp_sparse_numpy as QS
import refqp_tools as RT
from gpu_helpers import oracle_params, qp_constraints

CFG = importlib.import_module(PKG_NAME + ".config")
TS = (13, 20, 24, 30, 40)
COND_MAX = 1e13
EPS = 2.0 ** -52
# what the oracle returns for the singular cases, at every horizon of TS (w_para=0@a: the acceleration-state variant only): rounding noise in the pivots lets the
# standstill problems with Rd[1] > 0 through (status 0 -- and the answer passes the certificate: the flat direction costs nothing);
# an exactly zero pivot is ORC_BAD_INPUT (3)
RAW_STATUS = {"R_steer=0@a": 0, "R_zero@a": 0, "steer_free@a": 3, "acc_free@a": 3, "acc_free@b": 3, "acc_free@c": 3, "w_para=0@a": 0}
KINDS = [pytest.param("stock", T, id=f"T{T}") for T in TS] + [pytest.param("jerk", 13, id="jerk-T13")]


def _base(pkg, kind, T):
    return replace(pkg.mpc_jerk.config if kind == "jerk" else CFG.MPCConfig(), T=T)


def _problem(pkg, routes, kind, T):
    """(base, batch, cfgs, cases, G, h, D of ego b) of a kind and horizon, one ego per case."""
    base = _base(pkg, kind, T)
    batch, cfgs, _, cases = CC.make_batch(pkg.synth, routes, T, len(CC.CASES), base)
    G, h = qp_constraints(T, 0.2, batch.x0[:, 2], batch.speed, cfgs, base.MIN_SPEED, base.MAX_STEER_RAD, jerk=kind == "jerk")
    D = lambda b: CC.box_widths(cfgs[b], T, base.MAX_STEER_RAD, jerk=(batch.speed[b], base.MIN_SPEED, 0.2) if kind == "jerk" else None)
    return base, batch, cfgs, cases, G, h, D


def _cond(H):
    ev = np.linalg.eigvalsh(H)
    return (ev[-1] / ev[0] if ev[0] > 0 else np.inf), ev[0]


def test_case_list_is_the_script_and_carries_its_classes():
    assert [w for _, w in CC.SWEEP_ROWS[:5]] == [dict(w_perp=float(v)) for v in (0, 1, 10, 20, 50)]
    assert [w["R"] for _, w in CC.SWEEP_ROWS[10:20]] == [[0.0, .01], [.01, .01], [.1, .01], [1.0, .01], [10.0, .01],
                                                        [.1, 0.0], [.1, .01], [.1, .1], [.1, 1.0], [.1, 10.0]]
    assert [w["Rd"] for _, w in CC.SWEEP_ROWS[20:]] == [[0.0, 1.0], [1.0, 1.0], [5.0, 1.0], [10.0, 1.0], [20.0, 1.0],
                                                       [10.0, 0.0], [10.0, .01], [10.0, .1], [10.0, 1.0], [10.0, 10.0]]
    assert len({c.name for c in CC.CASES}) == len(CC.CASES) == 3 * 34
    sing = [c for c in CC.CASES if c.cls == "singular"]
    assert len(sing) * 10 <= len(CC.CASES) + 9 and {c.name for c in sing} == set(RAW_STATUS) - {"w_para=0@a"}   # about a tenth, enumerated by name
    assert {c.name for c in CC.CASES if CC.cls_of(c, "jerk") == "singular"} == set(RAW_STATUS)
    for c in sing:                                      # only: a standstill with a zero steering weight; both acceleration weights zero
        w = dict(CC.DEFAULTS); w.update(c.weights)
        assert (c.state == "a" and w["R"][1] == 0.0) or (w["R"][0] == 0.0 and w["Rd"][0] == 0.0)
    cfg = CC.config_of(CC.CASES[0], CFG.MPCConfig(), 20)
    assert cfg.T == 20 and cfg.Rd == [10.0, 1.0] and cfg.R == [0.1, 0.01] and cfg.w_perp == 0.0


@pytest.mark.parametrize("kind,T", KINDS)
def test_classes_from_the_oracles_hessian(pkg, oracle, routes, kind, T):
    """ "pd" <=> H positive definite with cond(H) <= 1e13 -- under the acceleration-state variant too, whose H has the free acc_0
    and its own list of singular cases; the oracle's status on the singular cases as it is today; the rows of G u <= h the tests
    build against the oracle's."""
    base, batch, cfgs, cases, G, h, D = _problem(pkg, routes, kind, T)
    rt = routes[CC.ROUTE]
    for b, c in enumerate(cases):
        p = oracle_params(oracle, cfgs[b])
        r = CC.oracle_step(oracle, p, routes, batch, b)
        cond, lmin = _cond(r["H"])
        cls = CC.cls_of(c, kind)
        print(f"{kind} T={T} {c.name:16s} {cls:8s} cond(H)={cond:9.2e} lambda_min={lmin:9.2e} oracle status {r['status']}")
        assert (cls == "pd") == (lmin > 0 and cond <= COND_MAX), c.name
        assert r["status"] == (RAW_STATUS[c.name] if cls == "singular" else 0), c.name
        if b % 3 == 2 or cls == "singular":                            # (the rows depend on the state and the limits, not on the weights)
            x0 = batch.x0[b]
            _, xref, _, rend, _ = oracle.calc_ref_trajectory(p, x0[0], x0[1], x0[2], rt[:, 0], rt[:, 1], rt[:, 2], int(batch.target_ind[b]))
            _, _, _, Go, ho, skip, _, _ = oracle.build_qp(p, xref, oracle.predict_motion(p, x0, batch.oa[b], batch.od[b]), x0, rend, float(batch.speed[b]))
            keep = ~skip.astype(bool)
            assert list(np.flatnonzero(~keep)) == [2 * T - 2, 3 * T - 1] and not G[~keep].any()
            assert np.abs(Go[keep] - G[keep]).max() <= 1e-15 and np.abs(ho[keep] - h[b][keep]).max() <= 1e-15, c.name


def test_condensed_qp_equals_the_reference_emitted_problem(pkg, oracle, routes):
    """tests/golden/sweep_qp.npz (T = 13, states a and c, the 30 sweep rows): reference window bit for bit, (H, g, G, h) <= 1e-9
    relative -- and within the bars of tests/test_ref_qp_cpu.py; a zero weight drops its term."""
    g = load_golden("sweep_qp.npz")
    names = [str(s) for s in g["name"]]
    by_name = {c.name: c for c in CC.CASES}
    assert len(names) == 60 and {n.split("@")[1] for n in names} == {"a", "c"} and {n.split("@")[0] for n in names} == set(dict(CC.SWEEP_ROWS))
    T, worst = 13, dict(dH=0.0, dg=0.0, dG=0.0, dh=0.0)
    P_of = {}
    for i, name in enumerate(names):
        c = by_name[name]
        batch, cfgs, _, _ = CC.make_batch(pkg.synth, routes, T, 1, CFG.MPCConfig(), cases=(c,))
        assert np.array_equal(batch.x0[0], g["x0"][i]) and batch.speed[0] == g["speed"][i]
        P, q, c0, A, b, G, h = RT.emitted_problem(g, i)
        P_of[name] = P
        Hr, gr, Gr, hr, Phi, phi = QS.condense(P, q, A, b, G, h, T)
        for p in (oracle_params(oracle, cfgs[0]),):
            rt, x0 = routes[CC.ROUTE], batch.x0[0]
            st, xref, idx, rend, tind = oracle.calc_ref_trajectory(p, x0[0], x0[1], x0[2], rt[:, 0], rt[:, 1], rt[:, 2], int(batch.target_ind[0]))
            assert st == 0 and tind == g["target_ind_out"][i] and np.array_equal(xref, g["xref"][i])
            xbar = oracle.predict_motion(p, x0, batch.oa[0], batch.od[0])
            _, H, gv, Go, ho, skip, _, _ = oracle.build_qp(p, xref, xbar, x0, rend, float(batch.speed[0]))
            keep = ~skip.astype(bool)
            worst["dH"] = max(worst["dH"], np.abs(H - Hr).max() / np.abs(Hr).max())
            worst["dg"] = max(worst["dg"], np.abs(gv - gr).max() / max(1.0, np.abs(gr).max()))
            worst["dG"] = max(worst["dG"], np.abs(Go[keep] - Gr[keep]).max())
            worst["dh"] = max(worst["dh"], np.abs(ho[keep] - hr[keep]).max())
        # the rows of G u <= h the tests build themselves (gpu_helpers.qp_constraints) are the emitted ones too
        Gq, hq = qp_constraints(T, 0.2, batch.x0[:, 2], batch.speed, cfgs, CFG.MPCConfig().MIN_SPEED, CFG.MPCConfig().MAX_STEER_RAD)
        assert np.abs(Gq[keep] - Gr[keep]).max() <= 1e-12 and np.abs(hq[0][keep] - hr[keep]).max() <= 1e-12
    print(worst)
    assert max(worst.values()) <= 1e-9, worst
    assert max(worst["dH"], worst["dG"], worst["dh"]) <= 1e-12 and worst["dg"] <= 1e-11, worst       # the bars of tests/test_ref_qp_cpu.py
    nx = 4 * (T + 1)
    for s in ("a", "c"):                                # the cost term of a weight is there with 0.01 and gone with 0
        for row0, row1, col in (("R_acc=0", "R_acc=0.01", 0), ("R_steer=0", "R_steer=0.01", 1)):
            d = P_of[f"{row1}@{s}"] - P_of[f"{row0}@{s}"]
            want = np.zeros_like(d)
            ui = nx + 2 * np.arange(T) + col
            want[ui, ui] = 0.01
            assert np.abs(d - want).max() <= 2 * np.spacing(np.abs(P_of[f"{row1}@{s}"]).max()), (row0, s)     # (R + 2 Rd rounds once per side)
            assert np.all(np.diag(P_of[f"Rd_{'acc' if col == 0 else 'steer'}=0@{s}"])[ui] == ([0.1, 0.01][col]))   # no Rd share left


@pytest.mark.parametrize("kind,T", KINDS)
def test_oracle_certificate_and_distance_from_the_exact_solve(pkg, oracle, routes, kind, T):
    """Every "pd" case solves, passes the certificate, and lies within 16 eps cond(H) max(1, |u|) of the exact solve on its final
    active set (a backward-stable solve delivers eps cond(H)).  These figures, times 16, are the GPU bars.  A singular case the
    oracle solves all the same (rounding noise in the pivots) passes the certificate too: the direction that costs nothing does not
    change f.  Under the acceleration-state variant the free acc_0 is recovered from the predicted speeds, as for the kernels."""
    base, batch, cfgs, cases, G, h, D = _problem(pkg, routes, kind, T)
    worst = dict(gap=0.0, primal=0.0, err_u=0.0, err_lam=0.0, infeasible=0.0)
    for b, c in enumerate(cases):
        cls = CC.cls_of(c, kind)
        r = CC.oracle_step(oracle, oracle_params(oracle, cfgs[b]), routes, batch, b)
        if r["status"] != 0:
            assert cls == "singular", c.name
            continue
        cond, _ = _cond(r["H"])
        m = CC.measure(QX, r["H"], r["g"], G, h[b], r["u"], r["lam"], r["active"], D(b), exact=cls == "pd")
        assert CC.certificate_passes(m), (c.name, m)
        if cls == "singular":
            print(f"{kind} T={T} {c.name:16s} {cls:8s} gap={m['gap']:.1e} (f={m['f']:.3e}) primal={m['primal']:.1e} |r|={m['r_inf']:.1e}")
            continue
        assert not m["singular"], c.name
        print(f"{kind} T={T} {c.name:16s} {cls:8s} cond(H)={cond:8.2e} active {len(r['active']):2d} gap={m['gap']:.1e} (f={m['f']:.3e}) "
              f"primal={m['primal']:.1e} |r|={m['r_inf']:.1e} err_u={m['err_u']:.1e} err_lam={m['err_lam']:.1e} "
              f"exact solve on the set violates a row by {max(m['infeasible'], 0.0):.1e}")
        assert m["err_u"] <= 16 * EPS * cond * max(1.0, m["u_max"]), (c.name, m)
        for k in worst:
            worst[k] = max(worst[k], m[k])
    print(f"{kind} T={T}: worst over the pd cases {worst}")


# ---- qp_exact against exact rational arithmetic ---------------------------------------------------------------------------
def _frac_solve(K, rhs):
    """Gauss-Jordan in Fractions."""
    n = len(rhs)
    M = [[Fraction(float(v)) for v in row] + [Fraction(float(r))] for row, r in zip(K, rhs)]
    for i in range(n):
        piv = next(r for r in range(i, n) if M[r][i] != 0)
        M[i], M[piv] = M[piv], M[i]
        M[i] = [v / M[i][i] for v in M[i]]
        for r in range(n):
            if r != i and M[r][i] != 0:
                M[r] = [a - M[r][i] * bb for a, bb in zip(M[r], M[i])]
    return [M[i][n] for i in range(n)]


def test_qp_exact_against_fractions():
    H = np.array([[4.0, 1.0, 0.5, 0.0], [1.0, 3.0, 0.25, 0.1], [0.5, 0.25, 2.0, 0.3], [0.0, 0.1, 0.3, 1e-7]])
    g = np.array([-1.0, 0.3, 0.7, -0.2])
    G = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.2, 0.2], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    h = np.array([0.1, 0.3, 0.5, 3.0])
    W = [0, 1]                                           # (the optimal set of this problem)
    K = np.block([[H, G[W].T], [G[W], np.zeros((2, 2))]])
    zf = _frac_solve(K, np.concatenate([-g, h[W]]))
    u, lw, z = QX.solve_on(H, g, G, h, W)
    assert max(abs(QX.MP.mpf(f.numerator) / QX.MP.mpf(f.denominator) - v) for f, v in zip(zf, z)) <= QX.MP.mpf(10) ** -40
    assert np.array_equal(u, [float(f) for f in zf[:4]]) and np.array_equal(lw, [float(f) for f in zf[4:]])
    # the certificate of a perturbed answer, every figure against Fractions
    up = u + np.array([-1e-9, -2e-9, 0.0, -3e-3])      # (into the feasible set: the gap bounds f(u) - f* for feasible u)
    lam = np.zeros(4); lam[W] = lw; lam[2] = 1e-6
    D = np.array([12.0, 1.5, 12.0, 1.5])
    ce = QX.certificate(H, g, G, h, up, lam, D)
    F = lambda a: [Fraction(float(v)) for v in a]
    Hf, Gf, uf, lf = [F(r) for r in H], [F(r) for r in G], F(up), F(lam)
    r = [sum(Hf[i][j] * uf[j] for j in range(4)) + Fraction(float(g[i])) + sum(Gf[k][i] * lf[k] for k in range(4)) for i in range(4)]
    slack = [Fraction(float(h[k])) - sum(Gf[k][j] * uf[j] for j in range(4)) for k in range(4)]
    gap = sum(abs(ri) * Fraction(float(d)) for ri, d in zip(r, D)) + sum(abs(l) * abs(s) for l, s in zip(lf, slack))
    f = sum(uf[i] * Hf[i][j] * uf[j] for i in range(4) for j in range(4)) / 2 + sum(Fraction(float(a)) * b for a, b in zip(g, uf))
    assert ce["gap"] == float(gap) and ce["r_inf"] == float(max(abs(v) for v in r)) and ce["f"] == float(f)
    assert ce["primal"] == float(max(Fraction(0), max(-s for s in slack))) and ce["lam_min"] == 0.0
    # the bound it is for: f(up) - f* <= gap, f* the optimum (here: the solve on the optimal set, which is feasible with lam >= 0)
    assert np.all(G @ u - h <= 1e-15) and np.all(lw >= 0)
    fstar = 0.5 * u @ H @ u + g @ u
    assert 0.0 <= ce["f"] - fstar <= ce["gap"]
    # singular at working precision: refused, not answered
    Hs = H.copy(); Hs[3] = 0.0; Hs[:, 3] = 0.0
    with pytest.raises(QX.SingularKKT):
        QX.solve_on(Hs, g, G, h, [0])                    # (u_3 costs nothing and no row of the set holds it)
    Hr = Hs.copy(); Hr[3, 3] = 1e-30; Hr[2, 3] = Hr[3, 2] = 1e-15 * np.sqrt(2.0)     # 2 x 2 block of rank one up to rounding
    with pytest.raises(QX.SingularKKT):
        QX.solve_on(Hr, g, G, h, [0])
    with pytest.raises(QX.SingularKKT):
        QX.solve_on(H, g, G, h, [0, 0])
    Hn = Hs.copy(); Hn[3, 3] = 1e-17                     # badly scaled only (cond 1e17 from one diagonal entry): solved, exactly
    zf = _frac_solve(np.block([[Hn, G[W].T], [G[W], np.zeros((2, 2))]]), np.concatenate([-g, h[W]]))
    assert np.array_equal(QX.solve_on(Hn, g, G, h, W)[0], [float(f) for f in zf[:4]])
