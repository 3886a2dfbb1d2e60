#!/usr/bin/env python3
"""Fixture for the projection of every recorded pose onto a path: the REFERENCE's own calc_nearest_index
(main/lib/trajectories.py:89-97), called with start_index = 0 and a State per pose, on every pose and path of tests/tracking_cases.py.
Written to tests/golden/tracking.npz, data only.

`idx` [cases][ticks] holds the reference's return value, -1 where the pose is not finite (the reference is not asked: np.argmin of
NaNs has no meaning here).  The cases' poses, flags, path indices and paths are stored beside it, so that the CPU test can tell a
changed case from a changed result.  The condition of tracking_cases.condition() -- apart from the constructed exact ties every
discrete choice has a margin >= 1e-9 -- is asserted here and its smallest margin stored (`margin`); the restatement's idx is
checked against the reference's right here.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_tracking.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import tracking_cases as KC                                           # noqa: E402


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            import matplotlib
            matplotlib.use("Agg")
            from lib.simulation import State
            from lib.trajectories import calc_nearest_index
            return State, calc_nearest_index
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def main():
    State, calc_nearest_index = load_reference()
    cs, paths = KC.cases(), KC.paths()
    A = KC.recorder_arrays(cs)
    mine = KC.restate(A)
    margin = KC.condition(cs, mine)
    idx = np.full((len(cs), KC.N), -1, dtype=np.int32)
    for b, c in enumerate(cs):
        path = paths[c["path"]]
        cx, cy = np.ascontiguousarray(path[:, 0]), np.ascontiguousarray(path[:, 1])
        for k, (x, y, yaw) in enumerate(c["ego"].tolist()):
            if np.isfinite([x, y, yaw]).all():
                idx[b, k] = calc_nearest_index(State(x=x, y=y, yaw=yaw, v=0.0), cx, cy, 0)
        assert np.array_equal(idx[b], mine["idx"][:, b]), (c["label"], np.flatnonzero(idx[b] != mine["idx"][:, b]))
        print(f"case {b} ({c['label']}): path {c['path']} of {len(path)} points, idx {idx[b][idx[b] >= 0].min()} .. {idx[b].max()}")
    print(f"{len(cs)} cases, {int((idx >= 0).sum())} reference calls; smallest margin apart from the ties {margin:.3g}")
    out = {"n_cases": np.int64(len(cs)), "labels": np.array([c["label"] for c in cs]), "ego": np.stack([c["ego"] for c in cs]),
           "flags": np.stack([c["flags"] for c in cs]), "path": np.array([c["path"] for c in cs], dtype=np.int32),
           "path_off": np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64), "points": np.concatenate(paths),
           "idx": idx, "margin": np.float64(margin)}
    path = os.path.join(HERE, "tracking.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
