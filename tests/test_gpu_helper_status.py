"""The column split of the factorisation (the owner wave factors columns [0, NS), helper 2 the rest), the helper-timeout status and the
per-launch iteration counters must not change a bit of any result (profiles/r22_split_factor.txt).

8 egos at every horizon with a helper kernel (13, 15, 16, 20, 25; the split is compiled at 13 .. 20) -- with helper wavefronts (this
process: B = 8 is below one ego per CU) and without (JSIM_HELP_MAX_B=0, read once per process: one child process runs those cases).
Inputs and what each case stores: tests/helper_status_cases.py; that the planted egos fail the way they are meant to is decided on
the CPU oracle in tests/test_helper_status_cpu.py.

  * step: oa, od, status, target_ind, n_iter, the active mask, and H and g from the debug entry are byte-identical between the two
    forms; u* is within 1e-6 of the CPU oracle where it solves (the bar tests/test_gpu_active_set.py holds for these limits).
  * closed loop: 18 ticks in three fused launches == the same ticks one by one == the plain form, byte for byte, with an ego that
    fails inside the active-set loop and one that fails in front of it in the batch (the latter flushes the helpers' commands
    beside the hand-over of the columns); ClosedLoop at all five horizons, ScenarioLoop (glue inside) at 13 and 20.
  * counters: jsim_mpc_iter_totals after each launch equals the sum of the single ticks' n_iter per ego, failing egos included:
    after one launch, across two launches without reset, and from zero after a reset.

Pivot guard: no step input here reaches the factorisation's `!(ck > 0) -> 1e-300` guard: the step test takes every H from the debug
entry and asserts that its smallest eigenvalue is far above rounding (printed), so every pivot is positive.  The loops' H are not
captured; their egos solve or fail on their limits, never on H.  The guard is one text for both sides of the split
(csrc/mpc_step_reg_chol.inc)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helper_status_cases as C
import issue_slots_cases as IS
from gpu_helpers import oracle_params

pytestmark = pytest.mark.gpu
LOOPS = [(T, "") for T in C.HORIZONS] + [(T, "s") for T in C.PRE_HORIZONS]
LOOP_IDS = [f"T{T}-{'scenario' if s else 'closed'}" for T, s in LOOPS]


@pytest.fixture(scope="module")
def here(pkg, routes):
    """Every case in this process (helper wavefronts)."""
    assert "JSIM_HELP_MAX_B" not in os.environ
    return C.run_all(pkg, routes)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """Every case in a child process with JSIM_HELP_MAX_B=0: one wave per ego, no helpers."""
    out = str(tmp_path_factory.mktemp("helper_status") / "plain.npz")
    r = subprocess.run([sys.executable, os.path.abspath(C.__file__), out], env=dict(os.environ, JSIM_HELP_MAX_B="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        d = {k: z[k] for k in z.files}
    assert str(d["help_max_b"]) == "0"
    return d


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("T", C.HORIZONS)
def test_step_with_and_without_helpers(pkg, oracle, routes, here, plain, T):
    sets = ["step"] + (["fix"] if T in C.FIXTURE_HORIZONS else [])
    for name in sets:
        for k in C.STEP_KEYS + ("H", "g"):
            _same(here[f"{name}_T{T}_{k}"], plain[f"{name}_T{T}_{k}"], (name, k))
        H = np.tril(here[f"{name}_T{T}_H"])                       # (lower triangle valid)
        emin = float(np.linalg.eigvalsh(H + np.swapaxes(np.tril(H, -1), 1, 2)).min())
        print(f"T = {T} {name}: smallest eigenvalue of H over the egos {emin:.3e}")
        assert emin > 1e-6, emin                                   # positive definite with a margin: the pivot guard is not reached
    batch, cfg = IS.ego_set(pkg, routes, T)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    ref = oracle.mpc_step_batch(oracle_params(oracle, cfg), batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off,
                                batch.target_ind, batch.oa, batch.od)
    st = here[f"step_T{T}_status"]
    assert np.array_equal(st, ref["status"]) and np.all(st == 0), (st, ref["status"])
    err = max(float(np.abs(here[f"step_T{T}_oa"] - ref["oa"]).max()), float(np.abs(here[f"step_T{T}_od"] - ref["od"]).max()))
    print(f"T = {T}: iterations per ego {here[f'step_T{T}_n_iter']}, max |u* - oracle| {err:.2e}")
    assert err <= 1e-6, err
    assert np.array_equal(here[f"step_T{T}_active_mask"].view(np.uint32), ref["active_mask"])


@pytest.mark.parametrize("T,s", LOOPS, ids=LOOP_IDS)
def test_loops_fused_ticked_and_plain(here, plain, T, s):
    f, t = f"{s}fused_T{T}_", f"{s}ticked_T{T}_"
    for k in C.LOOP_KEYS:
        _same(here[f + k], here[t + k], ("fused vs tick by tick", k))
        _same(here[f + k], plain[f + k], ("helpers vs one wave, fused", k))
        _same(here[t + k], plain[t + k], ("helpers vs one wave, tick by tick", k))
    st = here[t + "status_by_tick"]
    _same(st, plain[t + "status_by_tick"], "status per tick")
    _same(here[t + "n_iter"], plain[t + "n_iter"], "n_iter per tick")
    # both kinds of failure are in the launch from its first tick on, beside egos that solve
    n_iter = here[t + "n_iter"]
    assert st[0, C.IN_LOOP] == 1 and n_iter[0, C.IN_LOOP] >= 2, (st[0], n_iter[0])
    assert st[0, C.BEFORE_LOOP] == 1 and n_iter[0, C.BEFORE_LOOP] == 0, (st[0], n_iter[0])
    assert set(np.unique(st)) <= {0, 1} and (st[0] == 0).sum() >= C.B - 3, st[0]
    print(f"T = {T} {'scenario' if s else 'closed'} loop: failed ticks per ego {(st != 0).sum(axis=0).tolist()}, "
          f"iteration totals {n_iter.sum(axis=0).tolist()}")


@pytest.mark.parametrize("T,s", LOOPS, ids=LOOP_IDS)
@pytest.mark.parametrize("form", ("help", "plain"))
def test_iteration_totals_per_launch(here, plain, T, s, form):
    d = plain if form == "plain" else here
    n_iter = d[f"{s}ticked_T{T}_n_iter"].reshape(C.LAUNCHES, C.TICKS, C.B).sum(axis=1)     # per launch and ego
    tot = d[f"{s}fused_T{T}_totals"]
    assert n_iter[0, C.IN_LOOP] >= 2                                                       # the failing ego's iterations count
    assert np.array_equal(tot[0], n_iter[0]), ("one launch", tot[0], n_iter[0])
    assert np.array_equal(tot[1], n_iter[0] + n_iter[1]), ("two launches, no reset", tot[1], n_iter[:2].sum(axis=0))
    assert np.array_equal(tot[2], tot[1]), "the resetting read returns the totals"
    assert np.array_equal(tot[3], n_iter[2]), ("from zero after the reset", tot[3], n_iter[2])
    assert tot[0].max() > 2 * T
