#!/usr/bin/env python3
"""The time gaps of a recorded run as ONE launch (Recorder.gaps, jsim_loop_eval_gaps): a ScenarioLoop at T = 30 with config 3's four
scripted vehicles, 4096 egos, 300 recorded ticks, windows 20 and 63 under the episode rule.

Per window, as medians / min / max over --runs rounds after --warmup untimed ones: the launch alone (the entry point on buffers
that stay on the device, then a synchronise, no read-back) and the whole Recorder.gaps() call -- argument checks, the uploads of the
two range tables, the launch, the read-back of off [300][B][8] and the four episode outputs, gap and who made on the host.  Beside
them, on the same buffers: jsim_loop_eval_conflicts at frame_window 20, launch alone and whole call, timed the same way; and the
numpy restatement (tests/gaps_numpy.py) on arrays downloaded once outside the timed region, once per window.  Every window's result
is checked against the restatement (exactly: every output is an integer) and, at window 20, against the contact of the conflicts call.
Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_gaps.py [--runs 5] [--warmup 1] [--ticks 300] [--egos 4096] [--horizon 30] [--out profiles/NAME.txt]
"""
import numpy as np

import recorder_bench as RB

WINDOWS = (20, 63)


def launch_alone(pkg, torch, r, out, name, window_args, outputs, warmup, runs):
    """Wall ms of entry point `name` + synchronise on device buffers allocated once: the call without its read-back."""
    eng = r.loop.eng
    B, n, dev = eng.B, r.rec.shape[0], eng.device
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    veh, mate = up(out["veh_range"]), up(out["mate_range"])
    ego, shapes = np.array(out["ego_shape"]), eng.vehicle_shapes
    shapes = None if shapes is None else np.ascontiguousarray(shapes, dtype=np.float64).ctypes.data
    p = lambda t: t.data_ptr()
    call = lambda: getattr(eng.lib, name)(eng._ctx, B, n, p(r.rec), p(r.flags), r.n_obs, p(r.obs), p(r.x0_first), p(r.loop.x0_spawn), p(veh),
                                          p(mate), shapes, ego.ctypes.data, *window_args, *[p(t) for t in outputs], None)
    return RB.stats(RB.launch_alone(pkg, torch, eng, name, call, runs, warmup))


def main():
    a = RB.arguments(runs=5, warmup=1, egos=4096, horizon=30)
    torch, pkg = RB.setup("bench_gaps")
    import gaps_numpy as GN
    W = pkg.workloads
    B, K, T = a.egos, a.ticks, a.horizon
    routes = W.route_table(False)[0]
    eng, x0 = W.make_engine(routes, W.ego_batch(routes, B, T, rank=2), T, "cuda:0")
    loop = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS, max_age=W.MAX_AGE, hist_cap=K, record=K)
    loop.run(K)
    torch.cuda.synchronize()
    r = loop.recorder
    host = [r.rec.cpu().numpy(), r.flags.cpu().numpy(), r.obs.cpu().numpy(), r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy()]
    res = {"egos": B, "ticks": K, "T": T, "vehicles": len(W.OBSTACLE_SPECS), "runs": a.runs, "warmup": a.warmup, "within": "episode",
           "episodes": int(sum(r.episodes()["count"])), "launch_ms": {}, "call_ms": {}, "numpy_ms": {}, "ticks_with_a_gap": {}, "episode_gaps": {}}
    # the merged kernel at frame_window 20 on the same buffers
    ts, con = RB.timed(lambda: r.conflicts(frame_window=20), a.runs, a.warmup)
    res["conflicts_w20_call_ms"] = RB.stats(ts)
    outs = r._outputs("conflicts", K).values()
    res["conflicts_w20_launch_ms"] = launch_alone(pkg, torch, r, con, "jsim_loop_eval_conflicts", (20,), outs, a.warmup, a.runs)
    for w in WINDOWS:
        ts, out = RB.timed(lambda: r.gaps(window=w), a.runs, a.warmup)
        res["call_ms"][f"w{w}"] = RB.stats(ts)
        outs = r._outputs("gaps", K).values()
        res["launch_ms"][f"w{w}"] = launch_alone(pkg, torch, r, out, "jsim_loop_eval_gaps", (w, 0), outs, a.warmup, a.runs)
        tn, ref = RB.timed(lambda: GN.eval_gaps(*host, out["veh_range"], out["mate_range"], eng.vehicle_shapes, out["ego_shape"], w, 0), 1)
        res["numpy_ms"][f"w{w}"] = tn[0]
        for k in RB.output_keys(pkg, "gaps") + ("gap", "who"):
            assert np.array_equal(out[k], ref[k]), (w, k)
        if w == 20:
            assert np.array_equal(out["gap"] >= 0, con["contact"])
        eps = pkg.history.gap_episodes(out, host[1], eng.dt)
        gaps = np.array([e["gap"] for ep in eps for e in ep if e["gap"] >= 0])
        res["ticks_with_a_gap"][f"w{w}"] = int((out["gap"] >= 0).sum())
        res["episode_gaps"][f"w{w}"] = {"with_one": int(gaps.size), "median": float(np.median(gaps)) if gaps.size else None,
                                        "vehicle_first": int(sum(e["first"] == "vehicle" for ep in eps for e in ep)),
                                        "ego_first": int(sum(e["first"] == "ego" for ep in eps for e in ep))}
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
