#!/usr/bin/env python3
"""Fixture for tests/test_gpu_tick_boundary.py: what the library of the commit BEFORE the helpers took the next tick's head under
the current tick's tail computes on the fused launches of tests/tick_boundary_cases.py -- T = 13 and 20 at 64 egos, 12 ticks, in
the default dispatch (helper wavefronts).  The hand-over runs the same operations on the same operands in the same order, so the
new library has to reproduce these bytes.  Written to tests/golden/tick_boundary_parent.npz, data only: the applied controls of
every tick, final states, warm starts, predicted states, status, path indices, active masks, iteration counts and totals, ages and
the respawn count.

usage (on an MI355X, from the repo root; the parent commit's library built out of tree, e.g. from a worktree of that commit with
JSIM_LIB_OUT=/path/libjsim_mpc_parent.so python av-simulation-at-intersections_amd/build.py):
    JSIM_LIB_PATH=/path/libjsim_mpc_parent.so python tests/golden/make_golden_tick_boundary.py [out.npz]"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import tick_boundary_cases as C                                       # noqa: E402


def main(path):
    assert "JSIM_HELP_MAX_B" not in os.environ
    pkg = importlib.import_module(C.PKG_NAME)
    cabi = importlib.import_module(C.PKG_NAME + "._cabi")
    out = C.record(pkg, C.smoothed_routes(pkg), C.GOLDEN_ROWS)
    out["rows"] = np.array(C.GOLDEN_ROWS, dtype=np.int64)
    out["ticks"] = np.array(C.K, dtype=np.int64)
    np.savez_compressed(path, **out)
    print("library", cabi.LIB_PATH)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tick_boundary_parent.npz"))
