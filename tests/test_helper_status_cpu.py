"""CPU side of tests/test_gpu_helper_status.py: the plumbing of JSIM_HELPER_TIMEOUT (no GPU test makes a column fail to arrive) and
the premises of the case module, decided with the oracle."""
import os
import re
import types

import numpy as np
import pytest
import torch

import active_set_cases as AC
import helper_status_cases as C
from conftest import REPO
from gpu_helpers import oracle_batch_per_config


def test_header_document_and_binding_agree_on_the_status(pkg):
    cabi = pkg._cabi
    K = pkg._header.header().constants
    assert [K["JSIM_" + n] for n in ("OK", "INFEASIBLE", "NEAREST_ANOMALY", "NO_PATH", "HELPER_TIMEOUT")] == [0, 1, 2, 3, 4]
    assert (cabi.STATUS_OK, cabi.STATUS_INFEASIBLE, cabi.STATUS_NEAREST_ANOMALY, cabi.STATUS_NO_PATH, cabi.STATUS_HELPER_TIMEOUT) == (0, 1, 2, 3, 4)
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert re.search(r"\b4 `JSIM_HELPER_TIMEOUT`", doc) and "JsimError" in doc
    # the kernels use the header's name, and the owner reads the helpers' word behind the phase's closing barrier
    src = open(os.path.join(REPO, pkg.__name__, "csrc", "mpc_step_reg.inc")).read()
    assert "status = JSIM_HELPER_TIMEOUT" in src and "hb_tmo = 1" in src and "readfirstlane(hb_tmo)" in src


def test_check_status_raises_on_the_timeout_only(pkg):
    cabi = pkg._cabi
    cabi.check_status(np.array([0, 1, 2, 3, 0], dtype=np.int32), "x")
    with pytest.raises(cabi.JsimError, match=r"JSIM_HELPER_TIMEOUT.*ego\(s\) \[1, 3\]"):
        cabi.check_status(np.array([0, 4, 1, 4], dtype=np.int32), "x")


def test_read_back_raises_the_status(pkg):
    """BatchedMPC.read_back on a stand-in engine whose arena holds a status of 4: the exception reaches the caller."""
    layout, off = {}, 0
    for name, dt, shape in (("oa", torch.float64, (3, 2)), ("status", torch.int32, (3,)), ("n_iter", torch.int32, (3,))):
        n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        layout[name] = (off, n, dt, shape)
        off += n
    arena = torch.zeros(off, dtype=torch.uint8)
    eng = types.SimpleNamespace(_arena=arena, _arena_layout=layout)
    out = pkg.BatchedMPC.read_back(eng)
    assert out["status"].tolist() == [0, 0, 0] and out["oa"].shape == (3, 2)
    o, n, dt, shape = layout["status"]
    arena[o:o + n].view(dt)[2] = pkg._cabi.STATUS_HELPER_TIMEOUT
    with pytest.raises(pkg._cabi.JsimError, match=r"read_back.*status 4.*\[2\]"):
        pkg.BatchedMPC.read_back(eng)


@pytest.mark.parametrize("T", C.HORIZONS)
def test_the_mixed_set_has_one_failing_ego_of_each_kind(pkg, oracle, routes, T):
    """On the oracle's trace of the first tick: IN_LOOP ends inside the active-set loop after iterations, BEFORE_LOOP in front of it
    without one, the others solve; and arithmetic alone (active_set_cases.contradiction) names the same two egos."""
    batch, cfgs, which, base = C.mixed_set(pkg, routes, T)
    _, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=2, trace=True)
    end = ref["trace"][:, oracle.TRACE["end"]]
    assert end[C.IN_LOOP] == oracle.END_INFEASIBLE_IN_LOOP and ref["n_iter"][C.IN_LOOP] >= 2
    assert end[C.BEFORE_LOOP] == oracle.END_BEFORE_LOOP and ref["n_iter"][C.BEFORE_LOOP] == 0
    others = np.setdiff1d(np.arange(C.B), [C.IN_LOOP, C.BEFORE_LOOP])
    assert np.all(end[others] == oracle.END_OPTIMAL) and np.all(ref["status"][others] == 0)
    assert ref["status"][C.IN_LOOP] == 1 and ref["status"][C.BEFORE_LOOP] == 1
    assert np.flatnonzero(AC.contradictory(batch, cfgs, pkg.synth.DT)).tolist() == [C.IN_LOOP, C.BEFORE_LOOP]
