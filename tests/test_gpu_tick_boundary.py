"""The helpers' hand-over across the tick boundary (HB_NEXT): in a fused launch of the glue-free kernels with
helper wavefronts, helper 1 steps the plant, rolls the new warm start out and linearises about it, helpers 2 and 3 scan for the nearest
index -- all for the NEXT tick, under this tick's outputs and tail.  The same operations run on the same operands in the same order
as when the owner does them, so nothing may change by a bit.  Run with -m gpu on an MI355X.

Inputs: tests/tick_boundary_cases.py -- per row of csrc/reg_variants.h with helpers and without the glue, 64 egos x 12 ticks (256 egos
once at T = 20) that mix respawns every third tick, goals reached inside the launch, failures inside and before the active-set loop,
a nearest-index anomaly, an ego without a path, 2, 3 and 6 points of path left, and a failing tick behind a good one.

  * the fused launch == 12 launches of one tick (which never hand over), byte for byte;
  * == the same fused launch with JSIM_HELP_MAX_B=0 (no helper wavefronts; a child process), byte for byte;
  * T = 13 and 20 == tests/golden/tick_boundary_parent.npz, byte for byte: the fused launches as the library of commit d381c12
    ("Test the solve on the sensitivity study's weights and singular Hessians", the commit before the hand-over) computed them
    (tests/golden/make_golden_tick_boundary.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tick_boundary_cases as C
from conftest import load_golden
from gpu_helpers import PLANT_FAIL, cu_count

pytestmark = pytest.mark.gpu
IDS = [f"T{T}-B{B}" for T, B in C.ROWS]


@pytest.fixture(scope="module")
def one_wave(tmp_path_factory):
    """Every row's fused launch in a child process under JSIM_HELP_MAX_B=0."""
    assert "JSIM_HELP_MAX_B" not in os.environ
    out = str(tmp_path_factory.mktemp("tick_boundary") / "one_wave.npz")
    p = subprocess.run([sys.executable, os.path.abspath(C.__file__), out], env=dict(os.environ, JSIM_HELP_MAX_B="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    with np.load(out) as z:
        d = {k: z[k] for k in z.files}
    assert str(d["help_max_b"]) == "0"
    return d


@pytest.fixture(scope="module")
def golden():
    with load_golden("tick_boundary_parent.npz") as z:
        return {k: z[k] for k in z.files}


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_helpers_take_these_batches():
    assert max(B for _, B in C.ROWS) <= cu_count()


@pytest.mark.parametrize("T,B", C.ROWS, ids=IDS)
def test_fused_equals_single_ticks_one_wave_and_parent(pkg, routes, one_wave, golden, T, B):
    fused = C.run_case(pkg, routes, T, B)
    ticked = C.run_case(pkg, routes, T, B, fused=False)
    forms = {"tick by tick": ticked, "JSIM_HELP_MAX_B=0": {k: one_wave[f"T{T}_B{B}_{k}"] for k in C.KEYS}}
    if (T, B) in C.GOLDEN_ROWS:
        forms["parent fixture"] = {k: golden[f"T{T}_B{B}_{k}"] for k in C.KEYS}
    for name, d in forms.items():
        for k in C.KEYS:
            _same_bytes(fused[k], d[k], (name, k))
    # the batch holds what it is meant to hold (from the launches of one tick)
    st = np.stack([p["status"] for p in ticked["per_tick"]])      # [K][B]
    age = np.stack([p["age"] for p in ticked["per_tick"]])
    print(f"T={T} B={B}: {len(forms) + 1} forms agree; respawns {int(fused['n_respawn'][0])}, failing solves {int((st != 0).sum())} of {st.size}, "
          f"iterations {int(fused['iters'].sum())}")
    for e in C.RESPAWN:
        assert age[:, e].tolist() == [1, 2, 0] * (C.K // 3), e          # respawned by age every third tick
    for e in C.GOAL:
        assert np.any(age[:, e] == 0), e                                 # .. by reaching the goal (their age never runs out)
    assert np.all(st[:, C.HAIRPIN] == 2) and np.all(st[:, C.NO_PATH] == 3)
    assert np.all(st[:, [C.LEN2, C.LEN3, C.NEAR_END]] == 0)
    assert st[0, PLANT_FAIL] == 1 and st[0, 7] == 1 and st[0, 15] == 1   # before the loop; the planted rows inside it
    g = st[:, C.GOOD_THEN_FAIL]
    assert g[0] == 0 and g[-1] == 1 and np.all(np.diff((g != 0).astype(int)) >= 0), g.tolist()   # good ticks, then failing ones
    # a failing last tick keeps the last good tick's predicted states and clears the warm start
    assert np.all(fused["oa"][C.GOOD_THEN_FAIL] == 0) and np.any(fused["ox"][C.GOOD_THEN_FAIL] != 0)
