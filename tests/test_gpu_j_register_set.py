"""J's row keeps one register set through the active-set loop (compiler fact 7): that changed which registers
the add (Householder) and the drop (Givens) of an iteration write, and must not change a bit.  The kernel forms of one horizon run
the same arithmetic, so their closed loops must agree byte for byte on ego sets whose solves add AND drop rows
(tests/j_register_set_cases.py; tests/test_j_register_set_cpu.py shows the same on the CPU oracle):

  T = 13, 20 through jsim_mpc_run_ticks and T = 13 through jsim_loop_run_scenario, 8 egos x 6 ticks: the form with three helper
  wavefronts (B = 8 is below one ego per CU) against the one-wave form (JSIM_HELP_MAX_B=0, read once per process: a child process),
  and against the same loop tick by tick;
  T = 30 (virtual speed rows) and T = 40 (four-wave kernel), 4 egos x 4 ticks: fused against tick by tick."""
import os
import subprocess
import sys

import numpy as np
import pytest

import j_register_set_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sroutes(pkg):
    return C.synthetic_routes(pkg)


@pytest.fixture(scope="module")
def one_wave(tmp_path_factory):
    """Every one-wave case run in a child process with JSIM_HELP_MAX_B=0: {"<entry>_T<T>_<key>": array}."""
    out = str(tmp_path_factory.mktemp("j_register_set") / "one_wave.npz")
    env = dict(os.environ, JSIM_HELP_MAX_B="0")
    r = subprocess.run([sys.executable, os.path.abspath(C.__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out) as z:
        d = {k: z[k] for k in z.files}
    assert str(d["help_max_b"]) == "0"
    return d


def _long_solve_and_drops(n_iter, T):
    """The GPU's own iteration counters show what the ego set was chosen for: a solve of more than 2T iterations (hence with drops:
    an iteration adds or drops a row and the working set holds at most 2T), and solves that add rows at all."""
    assert n_iter.max() > 2 * T, n_iter
    assert (n_iter > 0).sum() > n_iter.size // 2


@pytest.mark.parametrize("entry,T", C.ONE_WAVE, ids=[f"{e}-T{t}" for e, t in C.ONE_WAVE])
def test_helper_form_equals_one_wave_form_and_tick_by_tick(pkg, sroutes, one_wave, entry, T):
    assert "JSIM_HELP_MAX_B" not in os.environ and C.B1 <= 64      # this process: helpers at B <= CU count
    fused = C.run_case(pkg, sroutes, entry, T)
    ticked = C.run_case(pkg, sroutes, entry, T, fused=False)
    _long_solve_and_drops(ticked["n_iter"], T)
    print(f"{entry} T = {T}: iterations per ego {fused['iters']}, longest solve {ticked['n_iter'].max()}")
    assert np.array_equal(fused["iters"], ticked["n_iter"].sum(axis=0))
    for k in C.KEYS:
        a, b = fused[k], one_wave[f"{entry}_T{T}_{k}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), ("helpers vs one wave", k)
        if k != "iters":
            assert a.tobytes() == ticked[k].tobytes(), ("fused vs tick by tick", k)


@pytest.mark.parametrize("T", (30, 40))
def test_fused_equals_tick_by_tick_on_the_long_horizons(pkg, sroutes, T):
    fused = C.run_case(pkg, sroutes, "run_ticks", T)
    ticked = C.run_case(pkg, sroutes, "run_ticks", T, fused=False)
    _long_solve_and_drops(ticked["n_iter"], T)
    print(f"T = {T}: iterations per ego {fused['iters']}, longest solve {ticked['n_iter'].max()}")
    assert np.array_equal(fused["iters"], ticked["n_iter"].sum(axis=0))
    for k in C.KEYS:
        if k != "iters":
            assert fused[k].dtype == ticked[k].dtype and fused[k].tobytes() == ticked[k].tobytes(), ("fused vs tick by tick", k)
