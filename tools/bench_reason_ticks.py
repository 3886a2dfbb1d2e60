#!/usr/bin/env python3
"""The per-tick stakeholder reasons of a recorded run as ONE launch (Recorder.reasons, jsim_loop_eval_reasons): a ScenarioLoop at
T = 13 with one cyclist, B = 256 and B = 4096 egos, 300 recorded ticks.

Timed: the whole Recorder.reasons() call -- argument checks, the uploads of par / threshold / veh_of / carry, the launch, the
read-back of val [300][B][4], timers, trig, first and carry -- wall ms as the median / min / max of --runs calls after --warmup
untimed ones.  Beside it: the numpy restatement (tests/reason_ticks_numpy.py) on the same arrays, downloaded once outside the timed
region, best of 3.  Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_reason_ticks.py [--runs 9] [--warmup 2] [--ticks 300] [--out profiles/NAME.txt]
"""
import numpy as np

import recorder_bench as RB


def cyclist_ahead(x0):
    """One cyclist, half a metre beside and six metres ahead of ego 0."""
    x, y = (float(v) for v in x0[0, :2].cpu())
    return [dict(kind="arterial", x_init=x + 0.5, y_init=y + 6.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None,
                 dims=dict(L=1.0, width=0.45, extra_length=0.64))]


def main():
    a = RB.arguments(runs=9, warmup=2)
    torch, pkg = RB.setup("bench_reason_ticks")
    import reason_ticks_numpy as TN
    K = a.ticks
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "gpu_ms": {}, "numpy_ms": {}, "max_rel_err": {}, "replans": {}}
    for B in (256, 4096):
        r = RB.recorded_loop(pkg, torch, B, K, cyclist_ahead, max_age=60, frame_window=20)
        ts, out = RB.timed(r.reasons, a.runs, a.warmup)
        res["gpu_ms"][str(B)] = RB.stats(ts)
        host = [t.cpu().numpy() for t in (r.rec, r.flags, r.obs, r.x0_first, r.loop.x0_spawn)]
        tn, ref = RB.timed(lambda: TN.eval_ticks(*host, out["veh_of"], out["par"], out["threshold"]), 3)
        res["numpy_ms"][str(B)] = min(tn)
        val = np.stack([out["policymaker"], out["driver"], out["cyclist"], out["distance"]], axis=2)
        assert np.array_equal(out["timers"], ref["timers"]) and np.array_equal(out["first_replan"], ref["first"])
        res["max_rel_err"][str(B)] = float(np.max(np.abs(val - ref["val"]) / np.abs(ref["val"])))
        res["replans"][str(B)] = int(out["replan"].sum())
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
