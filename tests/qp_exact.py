"""A high-precision reference for the condensed QP  min 1/2 u'Hu + g'u  s.t.  G u <= h.  Test infrastructure; shares nothing with
oracle/ or csrc/: it takes the problem and an answer as float64 arrays and evaluates them EXACTLY -- every float64 is an integer
times a power of two, so sums and products of them are integer arithmetic (Python ints, as mpmath's own numbers are); figures
are rounded once, at the end.  Solutions come back as mpmath numbers of 60 digits.

  certificate(H, g, G, h, u, lam, D)   how good (u, lam) is, whatever H's rank: the stationarity residual r = Hu + g + G'lam, the
      primal violation max(Gu - h, 0), min lam, and   gap = sum_i |r_i| D_i + sum_j |lam_j| |slack_j|  >=  f(u) - f*   whenever
      u is feasible, lam >= 0 and the feasible points u' have |u'_i - u_i| <= D_i (the box rows give D): for convex f,
      f(u') >= f(u) + grad f(u)'(u' - u) = f(u) + r'(u' - u) - lam'(Gu' - Gu) >= f(u) - sum |r_i| D_i - lam'(h - Gu).
  solve_on(H, g, G, h, W)              the equality-constrained optimum on active set W: the KKT system [[H, Gw'], [Gw, 0]]
      (u, lam_W) = (-g, h_W) by a float64 inverse with exact residuals (iterative refinement of a 220-bit fixed-point iterate);
      SingularKKT when the system is singular at working precision (the float64 factor does not contract the residual)."""
import math

import mpmath
import numpy as np

DIGITS = 60
MP = mpmath.mp.clone()
MP.dps = DIGITS
X_BITS = 220               # the iterate of solve_on: integers / 2^220 (66 digits behind the point)
TOL_BITS = 160             # converged: residual <= 2^-160 (1e-48) of the right-hand side


class SingularKKT(ArithmeticError):
    pass


def _fix(a, bits=None):
    """(ints, bits): the float64 array `a` as an object array of Python ints with a == ints / 2^bits EXACTLY; bits: at least
    that many (default: as many as the smallest entry needs)."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise SingularKKT("non-finite input")
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)                        # exact: |m| < 1 with 53 bits
    need = int(max(0, (53 - e[a != 0]).max(initial=0)))
    bits = need if bits is None else max(int(bits), need)
    sh = (e.astype(np.int64) - 53 + bits).ravel()
    out = np.empty(a.size, dtype=object)
    for k, (v, s) in enumerate(zip(mi.ravel().tolist(), sh.tolist())):
        out[k] = (v << s) if v else 0
    return out.reshape(a.shape), bits


def _flt(i, bits):
    """int / 2^bits, correctly rounded (Python's true division of ints is)."""
    return i / (1 << bits) if bits >= 0 else float(i << -bits)


def symmetric(H):
    """The symmetric matrix a kernel's lower triangle stands for."""
    return np.tril(H) + np.tril(H, -1).T


def certificate(H, g, G, h, u, lam, D):
    """dict(r_inf, primal, lam_min, gap, f): see the module text.  H symmetric [n, n]; G [m, n]; D [n] the box widths."""
    lam = np.asarray(lam, dtype=np.float64)
    S = max(_fix(x)[1] for x in (H, g, G, h, u, lam, D))         # one scale for all: products carry 2S, 3S
    Hi, gi, Gi, hi, ui, li, Di = (_fix(x, S)[0] for x in (H, g, G, h, u, lam, D))
    one = 1 << S
    Hu = Hi.dot(ui)
    rows = np.flatnonzero(lam != 0.0)
    r = Hu + gi * one
    if len(rows):
        r = r + Gi[rows].T.dot(li[rows])
    slack = hi * one - Gi.dot(ui)
    ab = np.frompyfunc(abs, 1, 1)
    gap = int(ab(r).dot(Di)) + (int(ab(li[rows]).dot(ab(slack[rows]))) if len(rows) else 0)
    f2 = int(ui.dot(Hu)) + 2 * one * int(gi.dot(ui))             # 2 f at scale 3S
    return dict(r_inf=_flt(int(max(ab(r))), 2 * S), primal=_flt(max(0, int(max(-slack))), 2 * S), lam_min=float(lam.min(initial=0.0)),
                gap=_flt(gap, 3 * S), f=_flt(f2, 3 * S + 1))


def solve_on(H, g, G, h, W, max_refine=200):
    """(u, lam_W, z): u and lam_W as float64 arrays rounded from the solution of the KKT system on rows W, and the solution
    itself, z = (u, lam_W), as mpmath numbers."""
    H, G = np.asarray(H, dtype=np.float64), np.asarray(G, dtype=np.float64)
    W = np.asarray(W, dtype=np.int64)
    n, k = H.shape[0], len(W)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = H
    K[:n, n:] = G[W].T
    K[n:, :n] = G[W]
    rhs = np.concatenate([-np.asarray(g, dtype=np.float64), np.asarray(h, dtype=np.float64)[W]])
    SK = max(_fix(K)[1], _fix(rhs)[1])
    Ki, bi = _fix(K, SK)[0], _fix(rhs, SK)[0]
    # the iterate's fixed point sits X_BITS below the right-hand side's leading bit (a tiny g gives a tiny u)
    XB = X_BITS + max(0, -int(math.frexp(float(np.abs(rhs).max(initial=0.0)))[1]))
    # the float64 approximate inverse, of the matrix equilibrated by powers of two (exact) so that it sees the best conditioning
    s = np.exp2(-np.round(np.log2(np.maximum(np.abs(K).max(axis=1), 1e-300)) / 2))
    Ks = K * s[:, None] * s[None, :]
    try:
        inv = np.linalg.inv(Ks)
    except np.linalg.LinAlgError as e:
        raise SingularKKT(str(e))
    if not np.all(np.isfinite(inv)) or np.linalg.norm(Ks, 1) * np.linalg.norm(inv, 1) > 2.0 ** 52:
        raise SingularKKT("singular to float64")                  # (a consistent singular system could still be `solved`)
    inv = inv * s[:, None] * s[None, :]
    x = np.zeros(n + k, dtype=object)
    x[:] = 0
    bX = bi * (1 << XB)
    ab = np.frompyfunc(abs, 1, 1)
    scale = int(max(ab(bX))) or 1
    prev = None
    for _ in range(max_refine):
        res = bX - Ki.dot(x)                                     # exact, at scale SK + XB
        nrm = int(max(ab(res)))
        if nrm <= scale >> TOL_BITS:
            z = [MP.ldexp(MP.mpf(int(v)), -XB) for v in x]
            zf = np.array([_flt(int(v), XB) for v in x])
            return zf[:n], zf[n:], z
        if prev is not None and 4 * nrm > prev:                  # the float64 inverse no longer contracts: cond(K) ~ 1 / eps
            raise SingularKKT(f"refinement stalls at a residual of {nrm / scale:.1e} of the right-hand side")
        prev = nrm
        dx = inv.dot(np.array([int(v) / nrm for v in res]))     # float64 correction for the residual scaled to 1
        if not np.all(np.isfinite(dx)):
            raise SingularKKT("non-finite correction")
        for j, d in enumerate(dx.tolist()):                      # x += dx * nrm / 2^SK, in fixed point
            m, e = math.frexp(d)
            v, sh = int(math.ldexp(m, 53)) * nrm, 53 - e + SK
            x[j] += (v >> sh) if sh >= 0 else (v << -sh)
    raise SingularKKT("refinement did not converge")
