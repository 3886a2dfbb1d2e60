#!/usr/bin/env python3
"""One row per recorded episode, reduced on the device (Recorder.summary, jsim_loop_summarise_episodes), against the path it
replaces: a ScenarioLoop at T = 13 with config 3's four scripted vehicles, B egos (--B 256,4096), 300 recorded ticks, every ego
against the 24 obstacles of intersection(1, 1) and with vehicle 0 as its cyclist -- the workload of tools/bench_conflicts.py and
tools/bench_static.py.

Timed, wall ms: (a) the whole Recorder.summary(conflicts=True, static=dict(obstacles=...), reasons=True) call -- the three
evaluations with their outputs kept on the device, the count of end flags, the three launches of the summary, the read-back of
ep_off and the table -- as the median / min / max of --runs calls after --warmup untimed ones; (b) the path it replaces on the same
records: Recorder.conflicts(), .static_conflicts(), .reasons() with their read-backs, then history.conflict_episodes,
history.static_episodes and history.reason_series, as the median / min / max of --host-runs passes, with each part's median beside
it; (c) the summary's three launches alone (the entry point on per-tick series that stay on the device, then a synchronise).
Also: the bytes read back each way, the rows, rows per second, and whether the table's clearance columns equal the host
functions' (a difference ends the run with an error).  Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_episodes.py [--B 256,4096] [--runs 9] [--warmup 2] [--host-runs 3] [--ticks 300] [--out profiles/NAME.txt]
"""
import statistics
import time

import numpy as np

import recorder_bench as RB


def launches_alone(pkg, torch, r, obstacles, warmup, runs):
    """Wall ms of jsim_loop_summarise_episodes + synchronise on per-tick series and a table allocated once."""
    eng, H = r.loop.eng, pkg.history
    B, n, dev = eng.B, r._n(), eng.device
    c, s, q = r._conflicts_device(n=n), r._static_device(obstacles, n=n), r._reasons_device(n=n)
    cap = int(H.episodes(r.flags[:n].cpu().numpy())["count"].sum())
    off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    ep_i = torch.empty(cap, len(H.EP_INT), dtype=torch.int32, device=dev)
    ep_d = torch.empty(cap, len(H.EP_DOUBLE), dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    keys = lambda name, skip=(): H.EVALUATORS[name].keys(skip)           # (the table of episodes takes no row and no timers)
    series = [p(c[k]) for k in keys("conflicts", ("row",))] + [p(s[k]) for k in keys("static")] + [p(q[k]) for k in keys("reasons", ("timers",))]
    call = lambda: eng.lib.jsim_loop_summarise_episodes(eng._ctx, B, n, p(r.rec), p(r.flags), p(r.x0_first), p(r.loop.x0_spawn), *series, cap,
                                                        p(off), p(ep_i), p(ep_d), None)
    return RB.launch_alone(pkg, torch, eng, "jsim_loop_summarise_episodes", call, runs, warmup)


def main():
    a = RB.arguments(runs=9, warmup=2, B="256,4096", host_runs=3)
    torch, pkg = RB.setup("bench_episodes")
    W, H = pkg.workloads, pkg.history
    K = a.ticks
    obstacles = pkg.planner.intersection_obstacles(1, 1)
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "host_runs": a.host_runs, "vehicles": len(W.OBSTACLE_SPECS),
           "obstacles": len(obstacles), "summary_ms": {}, "launches_ms": {}, "replaced_ms": {}, "replaced_parts_ms": {}, "rows": {},
           "rows_per_s": {}, "summary_bytes": {}, "replaced_bytes": {}, "mismatches": {}}
    for B in (int(x) for x in a.B.split(",")):
        r = RB.recorded_loop(pkg, torch, B, K)
        eng = r.loop.eng
        key = str(B)
        ts, s = RB.timed(lambda: r.summary(conflicts=True, static=dict(obstacles=obstacles), reasons=True), a.runs, a.warmup)
        res["summary_ms"][key] = RB.stats(ts)
        res["launches_ms"][key] = RB.stats(launches_alone(pkg, torch, r, obstacles, a.warmup, a.runs))
        E = len(s["ego"])
        res["rows"][key] = E
        res["rows_per_s"][key] = E / (res["summary_ms"][key]["median"] * 1e-3)
        res["summary_bytes"][key] = (B + 1) * 8 + E * (4 * len(H.EP_INT) + 8 * len(H.EP_DOUBLE))
        n = r._n()
        res["replaced_bytes"][key] = n * B * ((8 + 4 * 4 + 16) + (8 + 3 * 4) + (32 + 16 + 4)) + B * (4 + 24)
        flags = r.flags[:n].cpu().numpy()
        whole, parts = [], {k: [] for k in ("conflicts", "static_conflicts", "reasons", "conflict_episodes", "static_episodes", "reason_series")}
        for _ in range(a.host_runs):
            t = [time.perf_counter()]
            veh = r.conflicts(); t.append(time.perf_counter())
            st = r.static_conflicts(obstacles); t.append(time.perf_counter())
            rs = r.reasons(); t.append(time.perf_counter())
            ce = H.conflict_episodes(veh, flags); t.append(time.perf_counter())
            se = H.static_episodes(st, flags); t.append(time.perf_counter())
            H.reason_series(rs, flags, eng.dt); t.append(time.perf_counter())
            whole.append((t[-1] - t[0]) * 1e3)
            for k, d in zip(parts, np.diff(t)):
                parts[k].append(d * 1e3)
        res["replaced_ms"][key] = RB.stats(whole)
        res["replaced_parts_ms"][key] = {k: statistics.median(v) for k, v in parts.items()}
        flat = lambda eps, k: np.array([e[k] for ep in eps for e in ep])
        res["mismatches"][key] = {
            "veh_clear": int((~np.isclose(s["veh_clear"], flat(ce, "min_clear"), rtol=0, atol=0, equal_nan=True)).sum()),
            "veh_hit_tick": int((s["veh_hit_tick"] != flat(ce, "tick")).sum()),
            "st_clear": int((~np.isclose(s["st_clear"], flat(se, "min_clear"), rtol=0, atol=0, equal_nan=True)).sum()),
            "st_off_tick": int((s["st_off_tick"] != flat(se, "tick")).sum()),
            "st_ticks_off": int((s["st_ticks_off"] != flat(se, "ticks_off")).sum())}
    differs = any(v for m in res["mismatches"].values() for v in m.values())
    RB.emit(res, a.out, "the table differs from the host functions: see mismatches" if differs else None)


if __name__ == "__main__":
    main()
