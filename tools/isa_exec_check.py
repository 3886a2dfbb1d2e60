#!/usr/bin/env python3
"""Command-line entry of the build-time ISA guard, which lives in the package (av-simulation-at-intersections_amd/isa_exec_check.py,
where the pattern it finds is explained).  Loaded by file path, like the other tools, it exposes the same check() / kernels().

usage: isa_exec_check.py file.s [kernel-name-substring]      exit status 1 if any finding
"""
import importlib.util
import os
import sys

_spec = importlib.util.spec_from_file_location(
    "isa_exec_check", os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "av-simulation-at-intersections_amd",
                                   "isa_exec_check.py"))
_guard = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_guard)
check, check_kernel, kernels, main = _guard.check, _guard.check_kernel, _guard.kernels, _guard.main

if __name__ == "__main__":
    sys.exit(main())
