"""The one-wave kernels' back substitution r = R^-1 d1 on the 64-bit DPP row broadcast: columns
below 16 through v_fmac_f64 row_newbcast, always all sixteen; columns from 16 on by v_readlane behind one test of q > 16.  The new
steps take the same operands in the same order, so nothing may change by a bit.  Run with -m gpu on an MI355X.

Inputs: tests/backsub_cases.py -- 48 egos x 3-4 ticks at T = 13, 20 and 30 (virtual speed rows) whose solves stay within 8 rows,
end inside the first 16-lane row, pass 16 rows and stay above, fall back from above 16 rows, and drop a row at 16 or fewer;
tests/test_backsub_cpu.py proves that on the oracle's trace.  Every one-wave row of the variant table at these horizons runs them:
the rows with helper wavefronts in this process (48 egos are below one ego per CU), the one-wave-per-ego rows in a child process
with JSIM_HELP_MAX_B=0, T = 20's two-waves-per-SIMD row in another with JSIM_W2_MIN_B=1 as well (the library reads both once per
process); the rows with the glue inside through the scenario loop.

  * against the oracle (ClosedLoop, tick by tick): tick 0's status and active masks equal, its warm starts within 1e-6, every
    tick's applied controls and visited states within 1e-7, path indices equal, the oracle's iteration count on at least 0.9 of
    the solvable egos of every tick -- the bars of tests/test_gpu_active_set.py;
  * fused == tick by tick == every other kernel form of the horizon, byte for byte;
  * all of them == tests/golden/backsub_parent.npz, recorded from the library of the commit before the change
    (tests/golden/make_golden_backsub.py), byte for byte."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import backsub_cases as C
from conftest import PKG_NAME, load_golden
from gpu_helpers import W2_MIN_B, cu_count, variant_id

pytestmark = pytest.mark.gpu
CFG = importlib.import_module(PKG_NAME + ".config")
ONE_WAVE_ROWS = tuple(r for r in CFG.REG_VARIANTS if r[0] == 1 and r[1] in C.HORIZONS)
CASES = [(T, e) for T in C.HORIZONS for e in C.ENTRIES]
CHILD_ENVS = {"one_wave": dict(JSIM_HELP_MAX_B="0"), "two_per_simd": dict(JSIM_HELP_MAX_B="0", JSIM_W2_MIN_B="1")}


def row_taken(T, B, pre, help_max_b, w2_min_b):
    """select_reg_variant of csrc/reg_variants.h (tests/test_host_cpu.py holds the header to this table's dispatch)."""
    rows = set(CFG.REG_VARIANTS)
    help_, w2, w1 = (1, T, pre, 1, True), (1, T, pre, 2, False), (1, T, pre, 1, False)
    if B <= help_max_b and help_ in rows:
        return help_
    if w2 in rows and (w1 not in rows or B >= w2_min_b):
        return w2
    assert w1 in rows
    return w1


def rows_run(cu):
    """{row: where it runs} over this process and the two child processes."""
    out = {}
    for T, entry in CASES:
        out.setdefault(row_taken(T, C.B, entry == "run_scenario", cu, W2_MIN_B), "this process")
    for name, env in CHILD_ENVS.items():
        for entry, T in C.script_cases(env):
            out.setdefault(row_taken(T, C.B, entry == "run_scenario", int(env["JSIM_HELP_MAX_B"]), int(env.get("JSIM_W2_MIN_B", W2_MIN_B))), name)
    return out


@pytest.fixture(scope="module")
def golden():
    with load_golden("backsub_parent.npz") as z:
        d = {k: z[k] for k in z.files}
    assert d["seeds"].tolist() == [C.SEEDS[T] for T in C.HORIZONS] and d["ticks"].tolist() == [C.TICKS[T] for T in C.HORIZONS]
    return d


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """The fused loops in child processes under CHILD_ENVS: {name: {"<entry>_T<T>_<key>": array}}."""
    assert "JSIM_HELP_MAX_B" not in os.environ and "JSIM_W2_MIN_B" not in os.environ
    tmp = tmp_path_factory.mktemp("backsub")
    procs = {}
    for name, env in CHILD_ENVS.items():
        out = str(tmp / (name + ".npz"))
        procs[name] = (out, subprocess.Popen([sys.executable, os.path.abspath(C.__file__), out], env=dict(os.environ, **env),
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    res = {}
    for name, (out, p) in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-4000:])
        with np.load(out) as z:
            res[name] = {k: z[k] for k in z.files}
        assert str(res[name]["help_max_b"]) == "0" and str(res[name]["w2_min_b"]) == CHILD_ENVS[name].get("JSIM_W2_MIN_B", "")
    return res


def test_every_one_wave_row_of_the_horizons_is_run():
    run = rows_run(cu_count())
    print({variant_id(r): w for r, w in run.items()})
    assert set(run) == set(ONE_WAVE_ROWS) and len(ONE_WAVE_ROWS) == 11
    assert C.B <= cu_count()


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("T,entry", CASES, ids=[f"T{T}-{e}" for T, e in CASES])
def test_same_bytes_in_every_form_and_as_the_parent(pkg, routes, oracle, golden, children, T, entry):
    fused = C.run_case(pkg, routes, entry, T)
    ticked = C.run_case(pkg, routes, entry, T, fused=False)
    forms = {"tick by tick": ticked, "parent fixture": {k: golden[f"{entry}_T{T}_{k}"] for k in C.KEYS}}
    for name, d in children.items():
        if f"{entry}_T{T}_hist" in d:
            forms[name] = {k: d[f"{entry}_T{T}_{k}"] for k in C.KEYS}
    assert ("one_wave" in forms) == (T <= 20) and ("two_per_simd" in forms) == ((T, entry) == (20, "run_ticks"))
    for name, d in forms.items():
        for k in C.KEYS:
            _same_bytes(fused[k], d[k], (name, k))
    n_iter = np.stack([p["n_iter"] for p in ticked["per_tick"]])
    print(f"T={T} {entry}: {len(forms) + 1} forms agree; iterations per tick {n_iter.sum(axis=1).tolist()}, longest solve {int(n_iter.max())}")
    assert n_iter.max() > 2 * T                                     # a solve with drops among them (more iterations than variables)
    if entry != "run_ticks":
        return
    # the oracle's closed loop beside the ticked run
    ref = C.oracle_ticks(T)
    found = C.paths_taken(oracle, ref)
    assert all(found[p] for p in C.PATHS)
    step0, dev0 = ref[0]["step"], ticked["per_tick"][0]
    assert np.array_equal(dev0["status"], step0["status"]) and set(step0["status"]) == {0, 1}
    ok = step0["status"] == 0
    assert np.array_equal(dev0["active_mask"].view(np.uint32)[ok], step0["active_mask"][ok])
    err = max(np.abs(dev0["oa"] - step0["oa"])[ok].max(), np.abs(dev0["od"] - step0["od"])[ok].max())
    assert err <= 1e-6, err
    assert np.all(dev0["oa"][~ok] == 0) and np.all(dev0["od"][~ok] == 0)
    worst_x = worst_u = 0.0
    for k, (r, d) in enumerate(zip(ref, ticked["per_tick"])):
        solv = r["step"]["status"] == 0
        assert np.array_equal(d["status"], r["step"]["status"]), k
        same = float((d["n_iter"] == r["step"]["n_iter"])[solv].mean())
        assert same >= 0.9, (k, same)
        worst_x = max(worst_x, float(np.abs(d["x0"] - r["x0"]).max()))
        worst_u = max(worst_u, float(np.abs(ticked["hist"][k] - r["hist"]).max()))
        assert np.array_equal(d["target_ind"], r["target_ind"]), k
    print(f"T={T}: tick 0 max|du| {err:.2e}; over {len(ref)} ticks worst |dx| {worst_x:.2e}, worst |d(di, ai)| {worst_u:.2e}")
    assert worst_x <= 1e-7 and worst_u <= 1e-7, (worst_x, worst_u)
