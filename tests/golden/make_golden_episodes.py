#!/usr/bin/env python3
"""Fixture for the History columns of the per-episode table: the REFERENCE's own lib.simulation.History
(main/lib/simulation.py:64-88), filled through its store() the way HistorySimulation does it (:53-61: the spawn entry with
a = delta = xref_deviation = 0, then one entry per tick), one History per episode of every ego of tests/episode_cases.py, and plain
numpy reductions of its lists.  Written to tests/golden/episodes.npz, data only.  The reference has no episode summary of its own;
nothing else of it is used.

Per tick count of TICK_COUNTS and per episode, in the table's row order: ego, k0, n (= len(history) - 1), t_end (history.t[-1]),
length (np.sum of the sqrt(dx * dx + dy * dy) between consecutive entries), v_mean, v_max, a_min, a_max, delta_absmax, dev_max,
dev_mean (np.nanmax / np.nanmean; NaN where every tick's deviation is NaN), dev_tick (np.nanargmax; -1).  An episode without a tick
has NaN / -1.  `digest`: the SHA-256 of the cases' rec and flags, so that the test sees whether the cases are the stored ones.

usage (needs the reference checkout next to the repository, or JSIM_REFERENCE = its main/ directory; from the repo root):
    python tests/golden/make_golden_episodes.py"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import episode_cases as EC                                            # noqa: E402

TICK_COUNTS = (129, 200)
DOUBLES = ("t_end", "length", "v_mean", "v_max", "a_min", "a_max", "delta_absmax", "dev_max", "dev_mean")
END = 2 | 4


def load_reference():
    for cand in (os.environ.get("JSIM_REFERENCE"), os.path.join(os.path.dirname(REPO), "reference", "main")):
        if cand and os.path.isdir(os.path.join(cand, "lib")):
            sys.path.insert(0, cand)
            from lib.simulation import History, State
            return History, State
    raise SystemExit("reference checkout not found (set JSIM_REFERENCE to its main/ directory)")


def digest(A):
    return hashlib.sha256(np.ascontiguousarray(A["rec"]).tobytes() + np.ascontiguousarray(A["flags"]).tobytes()).hexdigest()


def main():
    History, State = load_reference()
    A = EC.recorder_arrays()
    out = {"tick_counts": np.array(TICK_COUNTS), "digest": np.array(digest(A)), "dt": np.array(0.1)}
    for n in TICK_COUNTS:
        rows = []
        for b in range(A["rec"].shape[1]):
            ends = [int(k) for k in np.flatnonzero(A["flags"][:n, b] & END)]
            for e, (k0, k1) in enumerate(zip([0] + [k + 1 for k in ends], [k + 1 for k in ends] + [n])):
                s = A["x_first"][b] if e == 0 else A["x_spawn"][b]
                h = History(sample_time=0.1)
                h.store(State(x=s[0], y=s[1], yaw=s[3], v=s[2]), a=0., delta=0., xref_deviation=0.)
                for r in A["rec"][k0:k1, b]:
                    h.store(State(x=r[0], y=r[1], yaw=r[2], v=r[3]), a=r[5], delta=r[4], xref_deviation=r[6])
                row = {"ego": b, "k0": k0, "n": len(h.x) - 1, "dev_tick": -1, "t_end": h.t[-1]}
                row.update({k: np.nan for k in DOUBLES[1:]})
                if k1 > k0:
                    dx, dy = np.diff(h.x), np.diff(h.y)
                    dev = np.array(h.xref_deviation[1:])
                    row.update(length=np.sum(np.sqrt(dx * dx + dy * dy)), v_mean=np.mean(h.v[1:]), v_max=np.max(h.v[1:]), a_min=np.min(h.a[1:]),
                               a_max=np.max(h.a[1:]), delta_absmax=np.max(np.abs(h.delta[1:])))
                    if not np.isnan(dev).all():
                        row.update(dev_max=np.nanmax(dev), dev_mean=np.nanmean(dev), dev_tick=k0 + int(np.nanargmax(dev)))
                rows.append(row)
        for k in ("ego", "k0", "n", "dev_tick"):
            out[f"{k}_{n}"] = np.array([r[k] for r in rows], dtype=np.int32)
        for k in DOUBLES:
            out[f"{k}_{n}"] = np.array([r[k] for r in rows], dtype=np.float64)
    path = os.path.join(HERE, "episodes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {n: len(out[f"ego_{n}"]) for n in TICK_COUNTS}, "episodes")


if __name__ == "__main__":
    main()
