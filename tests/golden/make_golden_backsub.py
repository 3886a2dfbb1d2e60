#!/usr/bin/env python3
"""Fixture for tests/test_gpu_backsub.py: what the library of the commit BEFORE the back substitution moved onto the 64-bit row
broadcast computes on the closed loops of tests/backsub_cases.py -- every horizon (13, 20, 30) through both fused entry points
(jsim_mpc_run_ticks, jsim_loop_run_scenario), in the default dispatch (helper wavefronts at T = 13 and 20).  The new steps use the
same operands in the same order, so every kernel form has to reproduce these bytes.  Written to tests/golden/backsub_parent.npz,
data only: the applied controls of every tick, the final warm starts, states, status, path indices, active masks and the per-ego
iteration totals.

usage (on an MI355X, from the repo root; the parent commit's library built out of tree, e.g. from a worktree of that commit with
JSIM_LIB_OUT=/path/libjsim_mpc_parent.so python av-simulation-at-intersections_amd/build.py):
    JSIM_LIB_PATH=/path/libjsim_mpc_parent.so python tests/golden/make_golden_backsub.py [out.npz]"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import backsub_cases as C                                             # noqa: E402


def main(path):
    assert "JSIM_HELP_MAX_B" not in os.environ and "JSIM_W2_MIN_B" not in os.environ
    pkg = importlib.import_module(C.PKG_NAME)
    cabi = importlib.import_module(C.PKG_NAME + "._cabi")
    out = C.record(pkg, C.smoothed_routes(pkg), [(e, T) for T in C.HORIZONS for e in C.ENTRIES])
    out["seeds"] = np.array([C.SEEDS[T] for T in C.HORIZONS], dtype=np.int64)
    out["ticks"] = np.array([C.TICKS[T] for T in C.HORIZONS], dtype=np.int64)
    np.savez_compressed(path, **out)
    print("library", cabi.LIB_PATH)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "backsub_parent.npz"))
