#!/usr/bin/env python3
"""Every recorded pose projected onto its route as ONE launch (Recorder.tracking, jsim_loop_eval_tracking): a ScenarioLoop at T = 13
with config 3's four scripted vehicles, B = 256 and 4096 egos, 300 recorded ticks, each ego on its planned route.

Per batch size: the launch alone, between two HIP events on the engine's stream, on buffers that stay on the device (median / min /
max of --runs launches after --warmup untimed ones); the whole Recorder.tracking() call -- argument checks, the launch, the
read-back of idx, seg, s, d, e_yaw [300][B] and of ep_i, ep_d, the path table kept on the recorder from the first call -- wall ms,
timed the same way, and each of the seven device-to-host copies by itself (copy_ms); the numpy restatement (tests/tracking_numpy.py) on arrays downloaded once outside the timed region, median of
--numpy-runs; history.tracking_episodes on the device result.  The device result is compared with the restatement (integers
exactly, doubles within 1e-12 * max(1, |value|)): a difference is reported in the JSON line and ends the run with an error.
Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_tracking.py [--runs 9] [--warmup 2] [--numpy-runs 3] [--ticks 300] [--egos 0] [--out profiles/NAME.txt]
"""
import statistics
import sys

import numpy as np

import recorder_bench as RB


def launch_alone(pkg, torch, r, warmup, runs):
    """ms between two events around jsim_loop_eval_tracking on device buffers allocated once: the call without its read-back."""
    eng = r.loop.eng
    d = r._tracking_device()                                        # (the table is on the device; these outputs are written again)
    px, py, pyaw, off, arc = r._tracking_table["dev"]
    p = lambda t: t.data_ptr()
    B, n = eng.B, d["idx"].shape[0]
    ts = []
    for run in range(warmup + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = eng.lib.jsim_loop_eval_tracking(eng._ctx, B, n, p(r.rec), p(r.flags), p(eng.path_id), int(px.numel()), p(px), p(py), p(pyaw),
                                             len(eng.paths), p(off), p(arc), *[p(d[k]) for k in RB.output_keys(pkg, "tracking")],
                                             eng._stream())
        t1.record()
        torch.cuda.synchronize()
        pkg._cabi.check(rc, eng._ctx, "jsim_loop_eval_tracking")
        if run >= warmup:
            ts.append(t0.elapsed_time(t1))
    return RB.stats(ts)


def main():
    a = RB.arguments(runs=9, warmup=2, numpy_runs=3, egos=0)
    torch, pkg = RB.setup("bench_tracking")
    import tracking_numpy as TN
    K = a.ticks
    ints, doubles = RB.output_keys(pkg, "tracking", "i"), RB.output_keys(pkg, "tracking", "f")
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "numpy_runs": a.numpy_runs, "path_points": {}, "launch_ms": {}, "call_ms": {},
           "copy_ms": {}, "numpy_ms": {}, "episodes_ms": {}, "output_bytes": {}, "episodes": {}, "max_err": {}, "mismatches": {}, "d_rms_median": {}}
    for B in ((a.egos,) if a.egos else (256, 4096)):
        r = RB.recorded_loop(pkg, torch, B, K)
        eng, key = r.loop.eng, str(B)
        pts = [len(eng.paths[int(i)]) for i in eng.path_id.cpu().numpy()]
        res["path_points"][key] = {"min": min(pts), "mean": float(np.mean(pts)), "max": max(pts)}
        ts, out = RB.timed(r.tracking, a.runs, a.warmup)
        res["call_ms"][key] = RB.stats(ts)
        res["launch_ms"][key] = launch_alone(pkg, torch, r, a.warmup, a.runs)
        dev = r._tracking_device()                                  # each output's device-to-host copy by itself
        for k in RB.output_keys(pkg, "tracking"):
            res["copy_ms"].setdefault(key, {})[k] = statistics.median(RB.timed(lambda: dev[k].cpu().numpy(), a.runs, a.warmup)[0])
        print(f"B = {B}: launch {res['launch_ms'][key]}, call {res['call_ms'][key]}; the restatement next", file=sys.stderr, flush=True)
        res["output_bytes"][key] = K * B * (4 + 4 + 8 + 8 + 8 + 4 * TN.NI + 8 * TN.ND)
        host = r.rec.cpu().numpy(), r.flags.cpu().numpy()
        tn, ref = RB.timed(lambda: TN.eval_tracking(*host, out["path_id"], eng.paths), a.numpy_runs)
        res["numpy_ms"][key] = statistics.median(tn)
        te, eps = RB.timed(lambda: pkg.history.tracking_episodes(out, host[1], eng.dt), 2)
        res["episodes_ms"][key] = min(te)
        res["episodes"][key] = int(sum(len(ep) for ep in eps))
        res["d_rms_median"][key] = float(np.nanmedian([e["d_rms"] for ep in eps for e in ep]))
        res["mismatches"][key] = {k: int((out[k] != ref[k]).sum()) for k in ints}
        with np.errstate(invalid="ignore"):
            res["max_err"][key] = {k: float(np.nanmax(np.abs(out[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])), initial=0.0)) for k in doubles}
        res["mismatches"][key]["nan"] = int(sum((np.isnan(out[k]) != np.isnan(ref[k])).sum() for k in doubles))
    differs = any(v for m in res["mismatches"].values() for v in m.values()) or max(v for m in res["max_err"].values() for v in m.values()) > 1e-12
    RB.emit(res, a.out, "the device result differs from the restatement: see mismatches / max_err" if differs else None)


if __name__ == "__main__":
    main()
