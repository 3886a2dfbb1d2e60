"""Issue slots taken out of the owner wave's path (profiles/r20_issue_slots.txt) must not change a bit of any result:

  * S2's x and y sums now run only when the debug entry asks for xbar.  One step through jsim_mpc_step_debug with xbar requested and
    one through jsim_mpc_step give the same oa, od, status, target_ind and n_iter byte for byte, and xbar is what it was: the CPU
    oracle's predict_motion within 1e-12 (the bar tests/test_oracle_golden.py and tests/test_gpu_parity.py hold against the stage
    fixtures) and, at T = 13 and 20, the stage fixtures' own xbar within the same 1e-12;
  * one wait per staged chunk and 16-byte column reads changed the instructions around the Cholesky, the rows of J and the
    active-set loop: a 6-tick fused launch equals the same loop tick by tick, byte for byte, on egos whose solves add and drop rows.

8 egos at T = 13 and 20 -- with helper wavefronts (this process: B = 8 is below one ego per CU) and without (JSIM_HELP_MAX_B=0,
read once per process: one child process runs those cases) -- and at T = 32 (four waves per ego, one form).  The two forms run the
same arithmetic and must agree byte for byte as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

import issue_slots_cases as C
from gpu_helpers import oracle_params

pytestmark = pytest.mark.gpu
FORMS = [(T, f) for T in C.FIXTURE_HORIZONS for f in ("help", "plain")] + [(32, "four-wave")]
IDS = [f"T{T}-{f}" for T, f in FORMS]


@pytest.fixture(scope="module")
def here(pkg, routes):
    """Every case in this process (helper wavefronts where the horizon has them)."""
    assert "JSIM_HELP_MAX_B" not in os.environ
    return C.run_all(pkg, routes)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """T = 13 and 20 in a child process with JSIM_HELP_MAX_B=0: one wave per ego, no helpers."""
    out = str(tmp_path_factory.mktemp("issue_slots") / "plain.npz")
    r = subprocess.run([sys.executable, os.path.abspath(C.__file__), out], env=dict(os.environ, JSIM_HELP_MAX_B="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        d = {k: z[k] for k in z.files}
    assert str(d["help_max_b"]) == "0"
    return d


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("T,form", FORMS, ids=IDS)
def test_debug_entry_and_normal_entry_agree_and_xbar_is_unchanged(pkg, oracle, routes, here, plain, T, form):
    d = plain if form == "plain" else here
    for k in C.STEP_KEYS:
        _same(d[f"dbg_T{T}_{k}"], d[f"std_T{T}_{k}"], ("debug vs normal entry", k))
        if form == "plain":
            _same(d[f"std_T{T}_{k}"], here[f"std_T{T}_{k}"], ("one wave vs helpers", k))
    batch, cfg = C.ego_set(pkg, routes, T)
    st, n_iter = d[f"std_T{T}_status"], d[f"std_T{T}_n_iter"]
    assert np.all(st == 0) and n_iter.min() > 0, (st, n_iter)          # every ego went through S2 and solved
    p = oracle_params(oracle, cfg)
    want = np.stack([oracle.predict_motion(p, batch.x0[b], batch.oa[b], batch.od[b]) for b in range(C.B)])
    assert np.ptp(want[:, 3], axis=1).min() > 1e-3                      # the yaw moves: the rollout integrates a steering angle
    err = float(np.abs(d[f"dbg_T{T}_xbar"] - want).max())
    print(f"T = {T} {form}: iterations per ego {n_iter}, max |xbar - oracle| {err:.2e}")
    assert err <= 1e-12, err
    if form == "plain":
        _same(d[f"dbg_T{T}_xbar"], here[f"dbg_T{T}_xbar"], "xbar, one wave vs helpers")
    if T in C.FIXTURE_HORIZONS:
        _, gx, gst = C.fixture_set(pkg, T)
        feas = (gst == 0) & (d[f"fix_T{T}_status"] != 1)        # (as tests/test_gpu_parity.py: the reference ran S2 for these)
        assert np.all(gst == 0) and feas.sum() >= C.B - 2
        ferr = float(np.abs(d[f"fix_T{T}_xbar"] - gx)[feas].max())
        print(f"T = {T} {form}: max |xbar - stage fixture| {ferr:.2e} on {int(feas.sum())} egos")
        assert ferr <= 1e-12, ferr


@pytest.mark.parametrize("T,form", FORMS, ids=IDS)
def test_fused_launch_equals_tick_by_tick(pkg, oracle, routes, here, plain, T, form):
    d = plain if form == "plain" else here
    n_iter = d[f"ticked_T{T}_n_iter"]
    # the premise, on the CPU oracle's trace of the first tick: these solves add AND drop rows
    batch, cfg = C.ego_set(pkg, routes, T)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    ref = oracle.mpc_step_batch(oracle_params(oracle, cfg), batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off,
                                batch.target_ind, batch.oa, batch.od, trace=True)
    adds, drops = int(ref["trace"][:, oracle.TRACE["adds"]].sum()), int(ref["trace"][:, oracle.TRACE["drops"]].sum())
    print(f"T = {T} {form}: iterations per tick and ego {n_iter.tolist()}; oracle, first tick: {adds} adds, {drops} drops")
    assert adds > 0 and drops > 0 and np.all(ref["status"] == 0) and n_iter[0].min() > 0
    assert np.array_equal(d[f"fused_T{T}_iters"], n_iter.sum(axis=0))
    for k in C.LOOP_KEYS:
        _same(d[f"fused_T{T}_{k}"], d[f"ticked_T{T}_{k}"], ("fused vs tick by tick", k))
        if form == "plain":
            _same(d[f"fused_T{T}_{k}"], here[f"fused_T{T}_{k}"], ("one wave vs helpers", k))
