"""`lib.multi_trajectory_generator` -> the MI355X route planner's multi-trajectory class under the reference's name (same
constructor, run() and run_all() as main/lib/multi_trajectory_generator.py / main/planner/multi_trajectory_planner.py:44-269; all
(e, p, o) combinations of run_all() are searched in one launch of jsim_plan_routes_weighted)."""
import importlib as _importlib
import os as _os
import sys as _sys

_REPO = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _REPO not in _sys.path:
    _sys.path.insert(0, _REPO)
_m = _importlib.import_module("av-simulation-at-intersections_amd.planner")
MotionPrimitiveSearch = _m.MultiTrajectorySearch
NodeType = tuple
