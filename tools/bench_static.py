#!/usr/bin/env python3
"""The static-obstacle clearance and contact of a recorded run as ONE launch (Recorder.static_conflicts, jsim_loop_eval_static): a
ScenarioLoop at T = 13 with config 3's four scripted vehicles, B = 4096 egos (and 256), 300 recorded ticks, every ego against the
24 obstacles of the reference's intersection(1, 1) (planner.intersection_obstacles(1, 1)), without and with its four hidden boxes.

Timed: the whole Recorder.static_conflicts() call -- the row builder, argument checks, the upload of set_of and of the tables, the
launch, the read-back of clear, who, hit, off_tick [300][B] -- wall ms as the median / min / max of --runs calls after --warmup
untimed ones (the read-back ends the call, so the clock stops behind a synchronising copy).  Beside it: the launch alone (the entry
point on buffers that stay on the device, then a synchronise, no read-back), which tells the kernel's share of the call from the
read-back's; the numpy restatement (tests/static_numpy.py) on the same arrays, downloaded once outside the timed region, best of
2; history.static_episodes on the device result.  The device result is compared with the restatement (who, hit and
off_tick exactly, clear within 1e-12): a difference is reported in the JSON line and ends the run with an error.  Prints one JSON
line and, with --out, writes it there.

    python3 tools/bench_static.py [--runs 30] [--warmup 3] [--ticks 300] [--out profiles/NAME.txt]
"""
import numpy as np

import recorder_bench as RB


def launch_alone(pkg, torch, r, out, rows, hidden, warmup, runs):
    """Wall ms of jsim_loop_eval_static + synchronise on device buffers allocated once: the call without its read-back."""
    eng = r.loop.eng
    B, n, dev = eng.B, r.rec.shape[0], eng.device
    sof = torch.from_numpy(np.ascontiguousarray(out["set_of"], dtype=np.int32)).to(dev)
    ego, off = np.array(out["ego_shape"]), np.array([0, len(rows)], dtype=np.int32)
    outs = r._outputs("static", n)
    p = lambda t: t.data_ptr()
    call = lambda: eng.lib.jsim_loop_eval_static(eng._ctx, B, n, p(r.rec), p(r.flags), p(r.x0_first), p(r.loop.x0_spawn), p(sof), 1,
                                                 off.ctypes.data, len(rows), rows.ctypes.data, ego.ctypes.data, hidden,
                                                 *[p(t) for t in outs.values()], None)
    return RB.launch_alone(pkg, torch, eng, "jsim_loop_eval_static", call, runs, warmup)


def main():
    a = RB.arguments(runs=30, warmup=3)
    torch, pkg = RB.setup("bench_static")
    import static_numpy as SN
    K = a.ticks
    obstacles = pkg.planner.intersection_obstacles(1, 1)
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "obstacles": len(obstacles), "gpu_ms": {}, "numpy_ms": {},
           "launch_ms": {}, "episodes_ms": {}, "readback_ms": {}, "max_clear_err": {}, "mismatches": {}, "ticks_touching": {}, "episodes": {},
           "output_bytes": {}}
    for B in (256, 4096):
        r = RB.recorded_loop(pkg, torch, B, K)
        tr, host_rec = RB.timed(lambda: r.rec.cpu().numpy(), 3)         # what a host evaluation starts with
        res["readback_ms"][str(B)] = min(tr)
        host = [host_rec, r.flags.cpu().numpy(), r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy()]
        res["output_bytes"][str(B)] = K * B * (8 + 4 + 4 + 4)
        for hidden in (0, 1):
            key = f"{B}/hidden{hidden}"
            ts, out = RB.timed(lambda: r.static_conflicts(obstacles, include_hidden=bool(hidden)), a.runs, a.warmup)
            res["gpu_ms"][key] = RB.stats(ts)
            rows = pkg.planner.static_obstacle_rows(obstacles, out["margin"])
            res["launch_ms"][key] = RB.stats(launch_alone(pkg, torch, r, out, rows, hidden, a.warmup, a.runs))["median"]
            tn, ref = RB.timed(lambda: SN.eval_static(*host, out["set_of"], [0, len(rows)], rows, out["ego_shape"], bool(hidden)), 2)
            res["numpy_ms"][key] = min(tn)
            te, eps = RB.timed(lambda: pkg.history.static_episodes(out, host[1]), 2)
            res["episodes_ms"][key] = min(te)
            res["mismatches"][key] = {k: int((out[k] != ref[k]).sum()) for k in RB.output_keys(pkg, "static", "i")}
            res["max_clear_err"][key] = float(np.max(np.abs(out["clear"] - ref["clear"]) / np.maximum(1.0, np.abs(ref["clear"]))))
            res["ticks_touching"][key] = int(out["contact"].sum())
            res["episodes"][key] = int(sum(len(ep) for ep in eps))
    differs = any(v for m in res["mismatches"].values() for v in m.values()) or max(res["max_clear_err"].values()) > 1e-12
    RB.emit(res, a.out, "the device result differs from the restatement: see mismatches / max_clear_err" if differs else None)


if __name__ == "__main__":
    main()
