"""The reference's own `MPC.step` (main/lib/mpc.py, run under the recording cvxpy stand-in) on FRESH seeded egos, against the
oracle -- the same comparison tests/golden/make_golden_refqp.py makes before it writes the fixtures, on cases no other fixture
holds.  The reference's steps on these egos are stored in tests/golden/ref_qp_live_T*.npz (`make_golden_refqp.py live`, the
build container only), so the comparison needs nothing outside the repository."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import refqp_tools as RT


@pytest.mark.parametrize("T,n", ((13, 120), (20, 100), (30, 70), (40, 50)))
def test_reference_step_live_vs_oracle(oracle, pkg, routes, T, n):
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_refqp as M
    import qp_sparse_numpy as QS
    g = load_golden(f"ref_qp_live_T{T}.npz")
    # the stored inputs are the seeded egos the reference was run on
    b = pkg.synth.make_ego_batch(routes, n, T, seed=M.LIVE_SEED + T, truncate=True, near_end_frac=0.25)
    assert len(g["x0"]) == n and np.array_equal(g["x0"], b.x0) and np.array_equal(g["path_id"], b.path_id)
    assert np.array_equal(g["path_len"], b.path_len) and np.array_equal(g["target_ind_in"], b.target_ind)
    assert np.array_equal(g["speed"], b.speed) and np.array_equal(g["oa_in"], b.oa) and np.array_equal(g["od_in"], b.od)
    figs = []
    for i in range(n):
        c = (b.x0[i].copy(), int(b.path_id[i]), int(b.path_len[i]), int(b.target_ind[i]), float(b.speed[i]), b.oa[i].copy(),
             b.od[i].copy(), "live")
        P, q, c0, A, bb, G, h = RT.emitted_problem(g, i)
        r = dict(P=P, q=q, A=A, b=bb, G=G, h=h)
        out = dict(status=int(g["status"][i]), target_ind=int(g["target_ind_out"][i]), xref=g["xref"][i], lam=g["lam"][i],
                   **{k: g[k][i] for k in ("oa", "od", "ox", "oy", "ov", "oyaw")})
        figs.append(M.compare_with_oracle(oracle, QS, pkg, T, routes[c[1]], c, r, out))
    mx = lambda k: max(f.get(k, 0.0) for f in figs)
    assert all(f["status_equal"] and f["target_equal"] and f["xref_equal"] for f in figs)
    assert mx("dH") <= 1e-12 and mx("dG") <= 1e-12 and mx("dh") <= 1e-12 and mx("dg") <= 1e-11
    assert mx("du") <= 1e-8 and mx("dx") <= 1e-8
    assert all(f.get("active_in_tight", True) for f in figs)
    assert all(f.get("active_equal", True) for f in figs if not f.get("degenerate"))
    assert sum("du" in f for f in figs) >= n - 2
