#!/usr/bin/env python3
"""The clearance and first contact of a recorded run as ONE launch (Recorder.conflicts, jsim_loop_eval_conflicts): a ScenarioLoop
at T = 13 with config 3's four scripted vehicles, B = 256 and B = 4096 egos, 300 recorded ticks, frame_window 0 and 3.

Timed: the whole Recorder.conflicts() call -- argument checks, the uploads of the two range tables, the launch, the read-back of
clear, who, row, hit_tick, hit_frame [300][B] and hit_xy [300][B][2] -- wall ms as the median / min / max of --runs calls after
--warmup untimed ones.  Beside it: the numpy restatement (tests/conflicts_numpy.py) on the same arrays, downloaded once outside the
timed region, best of 3; history.conflict_episodes on the device result; the read-back of rec and obs_rec that an evaluation on
the host would start with; and the launch alone (the entry point on buffers that stay on the device, then a synchronise, no
read-back), which tells the kernel's share of the call from the read-back's.  Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_conflicts.py [--runs 9] [--warmup 2] [--ticks 300] [--out profiles/NAME.txt]
"""
import numpy as np

import recorder_bench as RB


def launch_alone(pkg, torch, r, out, w, warmup, runs):
    """Wall ms of jsim_loop_eval_conflicts + synchronise on device buffers allocated once: the call without its read-back."""
    eng = r.loop.eng
    B, n, dev = eng.B, r.rec.shape[0], eng.device
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    veh, mate = up(out["veh_range"]), up(out["mate_range"])
    ego = np.array(out["ego_shape"])
    outs = r._outputs("conflicts", n)
    p = lambda t: t.data_ptr()
    call = lambda: eng.lib.jsim_loop_eval_conflicts(eng._ctx, B, n, p(r.rec), p(r.flags), r.n_obs, p(r.obs), p(r.x0_first), p(r.loop.x0_spawn),
                                                    p(veh), p(mate), None, ego.ctypes.data, w, *[p(t) for t in outs.values()], None)
    return RB.launch_alone(pkg, torch, eng, "jsim_loop_eval_conflicts", call, runs, warmup)


def main():
    a = RB.arguments(runs=9, warmup=2)
    torch, pkg = RB.setup("bench_conflicts")
    import conflicts_numpy as CN
    K = a.ticks
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "vehicles": len(pkg.workloads.OBSTACLE_SPECS), "gpu_ms": {},
           "numpy_ms": {}, "launch_ms": {}, "episodes_ms": {}, "readback_ms": {}, "max_clear_err": {}, "contacts": {}, "episodes": {}}
    for B in (256, 4096):
        r = RB.recorded_loop(pkg, torch, B, K)
        eng = r.loop.eng
        tr, (host_rec, host_obs) = RB.timed(lambda: (r.rec.cpu().numpy(), r.obs.cpu().numpy()), 3)   # what a host evaluation starts with
        res["readback_ms"][str(B)] = min(tr)
        host = [host_rec, r.flags.cpu().numpy(), host_obs, r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy()]
        for w in (0, 3):
            key = f"{B}/w{w}"
            ts, out = RB.timed(lambda: r.conflicts(frame_window=w), a.runs, a.warmup)
            res["gpu_ms"][key] = RB.stats(ts)
            res["launch_ms"][key] = RB.stats(launch_alone(pkg, torch, r, out, w, a.warmup, a.runs))["median"]
            tn, ref = RB.timed(lambda: CN.eval_conflicts(*host, out["veh_range"], out["mate_range"], eng.vehicle_shapes, out["ego_shape"], w), 3)
            res["numpy_ms"][key] = min(tn)
            te, eps = RB.timed(lambda: pkg.history.conflict_episodes(out, host[1]), 3)
            res["episodes_ms"][key] = min(te)
            for k in RB.output_keys(pkg, "conflicts", "i"):
                assert np.array_equal(out[k], ref[k]), (key, k)
            assert np.array_equal(out["hit_xy"], ref["hit_xy"], equal_nan=True), key
            res["max_clear_err"][key] = float(np.max(np.abs(out["clear"] - ref["clear"]) / np.maximum(1.0, np.abs(ref["clear"]))))
            res["contacts"][key] = int(sum(e["contact"] for ep in eps for e in ep))
            res["episodes"][key] = int(sum(len(ep) for ep in eps))
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
