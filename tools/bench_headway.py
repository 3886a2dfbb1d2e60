#!/usr/bin/env python3
"""Every recorded vehicle projected onto the ego's route as ONE launch (Recorder.headway, jsim_loop_eval_headway): a ScenarioLoop at
T = 13 with config 3's four scripted vehicles, B = 256 and 4096 egos, 300 recorded ticks, each ego on its planned route.

Per batch size, with the per-place outputs (places=True) and without (places=False): the launch alone, between two HIP events on
the engine's stream, on buffers that stay on the device (median / min / max of --runs launches after --warmup untimed ones), and the
whole Recorder.headway() call -- argument checks, the launch, the read-back, the path table kept on the recorder from the first call
-- wall ms, timed the same way.  Beside them jsim_loop_eval_tracking's launch on the same recording (tools/bench_tracking.py's own
measurement: one search per lane against headway's 2 + 2 * 4), the ratio of the two launches, and the numpy restatement
(tests/headway_numpy.py) on arrays downloaded once outside the timed region: on the first --numpy-egos egos (it takes about a
second per thousand ego-ticks; numpy_ms is that time, numpy_ms_scaled the same per ego times B).  The device result of those egos is
compared with the restatement (integers exactly, inf and NaN in the same slots, doubles within 1e-12): a difference is reported in
the JSON line and ends the run with an error.  Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_headway.py [--runs 9] [--warmup 2] [--numpy-egos 256] [--ticks 300] [--egos 0] [--out profiles/NAME.txt]
"""
import sys

import numpy as np

import bench_tracking as BT
import recorder_bench as RB


def launch_alone(pkg, torch, r, places, warmup, runs):
    """ms between two events around jsim_loop_eval_headway on device buffers allocated once: the call without its read-back."""
    import ctypes as C
    eng = r.loop.eng
    d = r._headway_device(places=places)                            # (the table is on the device; these outputs are written again)
    px, py, pyaw, off, arc = r._tracking_table["dev"]
    p = lambda t: None if t is None else t.data_ptr()
    B, n = eng.B, d["lead"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(eng.device)
    veh, mate = up(d["veh_range"]), up(d["mate_range"])
    ego = (C.c_double * 3)(*d["ego_shape"])
    shapes = None if eng.vehicle_shapes is None or not r.n_obs else np.ascontiguousarray(eng.vehicle_shapes, dtype=np.float64)
    ts = []
    for run in range(warmup + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = eng.lib.jsim_loop_eval_headway(eng._ctx, B, n, p(r.rec), p(r.flags), r.n_obs, p(r.obs), p(r.x0_first), p(r.loop.x0_spawn), p(veh),
                                            p(mate), None if shapes is None else shapes.ctypes.data, C.cast(ego, C.c_void_p), p(eng.path_id),
                                            int(px.numel()), p(px), p(py), p(pyaw), len(eng.paths), p(off), p(arc), 0.0,
                                            *[p(d.get(k)) for k in RB.output_keys(pkg, "headway")], eng._stream())   # (no places: NULL)
        t1.record()
        torch.cuda.synchronize()
        pkg._cabi.check(rc, eng._ctx, "jsim_loop_eval_headway")
        if run >= warmup:
            ts.append(t0.elapsed_time(t1))
    return RB.stats(ts)


def main():
    a = RB.arguments(runs=9, warmup=2, numpy_egos=256, egos=0)
    torch, pkg = RB.setup("bench_headway")
    import headway_numpy as HN
    K = a.ticks
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "numpy_egos": a.numpy_egos, "vehicles": {}, "path_points": {},
           "launch_ms": {}, "launch_ms_no_places": {}, "call_ms": {}, "call_ms_no_places": {}, "tracking_launch_ms": {}, "launch_ratio": {},
           "numpy_ms": {}, "numpy_ms_scaled": {}, "output_bytes": {}, "episodes": {}, "lead_ticks": {}, "max_err": {}, "mismatches": {}}
    for B in ((a.egos,) if a.egos else (256, 4096)):
        r = RB.recorded_loop(pkg, torch, B, K)
        eng, key = r.loop.eng, str(B)
        pts = [len(eng.paths[int(i)]) for i in eng.path_id.cpu().numpy()]
        res["path_points"][key] = {"min": min(pts), "mean": float(np.mean(pts)), "max": max(pts)}
        res["vehicles"][key] = r.n_obs
        ts, out = RB.timed(r.headway, a.runs, a.warmup)
        res["call_ms"][key] = RB.stats(ts)
        res["call_ms_no_places"][key] = RB.stats(RB.timed(lambda: r.headway(places=False), a.runs, a.warmup)[0])
        res["launch_ms"][key] = launch_alone(pkg, torch, r, True, a.warmup, a.runs)
        res["launch_ms_no_places"][key] = launch_alone(pkg, torch, r, False, a.warmup, a.runs)
        res["tracking_launch_ms"][key] = BT.launch_alone(pkg, torch, r, a.warmup, a.runs)
        res["launch_ratio"][key] = res["launch_ms"][key]["median"] / res["tracking_launch_ms"][key]["median"]
        print(f"B = {B}: launch {res['launch_ms'][key]}, tracking's {res['tracking_launch_ms'][key]}, call {res['call_ms'][key]}; the restatement next",
              file=sys.stderr, flush=True)
        res["output_bytes"][key] = K * B * (4 + 4 + 8 * 4 + 4 * HN.NI + 8 * HN.ND + 3 * 8 * 8)
        m = min(B, a.numpy_egos)                                    # (no mates here: any leading part of the batch stands alone)
        host = (r.rec[:, :m].cpu().numpy(), r.flags[:, :m].cpu().numpy(), r.obs.cpu().numpy(), r.x0_first[:m].cpu().numpy(), r.loop.x0_spawn[:m].cpu().numpy(),
                out["veh_range"][:m], np.zeros((m, 2), dtype=np.int32), eng.vehicle_shapes, out["ego_shape"], out["path_id"][:m], eng.paths, 0.0)
        assert not out["mate_range"].any()
        tn, ref = RB.timed(lambda: HN.eval_headway(*host), 1)
        res["numpy_ms"][key], res["numpy_ms_scaled"][key] = tn[0], tn[0] * B / m
        eps = pkg.history.headway_episodes(out, r.flags.cpu().numpy(), eng.dt)
        res["episodes"][key] = int(sum(len(ep) for ep in eps))
        res["lead_ticks"][key] = int((out["lead"] >= 0).sum())
        res["mismatches"][key] = {k: int((out[k][:, :m] != ref[k]).sum()) for k in RB.output_keys(pkg, "headway", "i")}
        doubles = RB.output_keys(pkg, "headway", "f")
        res["mismatches"][key]["nan_inf"] = int(sum((np.isnan(out[k][:, :m]) != np.isnan(ref[k])).sum() + (np.isinf(out[k][:, :m]) != np.isinf(ref[k])).sum()
                                                    for k in doubles))
        err = {}
        for k in doubles:
            fin = np.isfinite(ref[k]) & np.isfinite(out[k][:, :m])
            err[k] = float((np.abs(out[k][:, :m][fin] - ref[k][fin]) / np.maximum(1.0, np.abs(ref[k][fin]))).max(initial=0.0))
        res["max_err"][key] = err
    differs = any(v for m in res["mismatches"].values() for v in m.values()) or max(v for m in res["max_err"].values() for v in m.values()) > 1e-12
    RB.emit(res, a.out, "the device result differs from the restatement: see mismatches / max_err" if differs else None)


if __name__ == "__main__":
    main()
