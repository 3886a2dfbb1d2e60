"""What the loop benches of tools/ (bench_traffic, bench_shapes, bench_history, bench_interacting, bench_scenario_loop) share:
a ScenarioLoop of the workloads' egos, the timed run, the common fields of a JSON line and the rocprofv3 kernel summary."""
import csv
import glob
import json
import os
import time


def scenario_loop(pkg, routes, B, T, specs, **kw):
    """ScenarioLoop over workloads.ego_batch(routes, B, T) on device 0, with config 3's max_age."""
    W = pkg.workloads
    eng, x0 = W.make_engine(routes, W.ego_batch(routes, B, T), T, "cuda:0")
    return pkg.ScenarioLoop(eng, x0, specs, max_age=W.MAX_AGE, **kw)


def timed_run(loop, warmup, ticks, each_tick=None):
    """Seconds of `ticks` device-synchronised ticks after run(warmup): one run(ticks), or with each_tick `ticks` x (tick(),
    each_tick())."""
    import torch
    loop.run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if each_tick is None:
        loop.run(ticks)
    else:
        for _ in range(ticks):
            loop.tick()
            each_tick()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loop_fields(loop, ticks, dt):
    """The fields every loop bench prints for `ticks` ticks that took dt seconds."""
    eng = loop.loop.eng
    return {"egos": eng.B, "T": eng.T, "ticks": ticks, "vehicles": loop.obst.n, "ego_steps_per_s": round(eng.B * ticks / dt),
            "ms_per_tick": round(dt / ticks * 1e3, 4), "cut_last_tick": int(loop.pre.col_flag.sum().item()),
            "failed_last_tick": int((eng.status != 0).sum().item())}


def summarize(out_dir):
    """Kernel time by name from rocprofv3's *kernel_stats.csv under out_dir: total, and the obstacle kernels' share."""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {out_dir}")
    for path in files:
        rows = list(csv.DictReader(open(path)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        by = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in rows}
        obst = {n: v for n, v in by.items() if n.startswith("obstacle_")}
        t_obst = sum(v[1] for v in obst.values())
        print(json.dumps({"stats": os.path.relpath(path, out_dir), "kernel_ms": round(tot / 1e6, 3),
                          "obstacle_share": round(t_obst / tot, 4) if tot else None,
                          "kernels": {n.split("(")[0][:60]: {"calls": c, "ms": round(t / 1e6, 3), "share": round(t / tot, 4)}
                                      for n, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1])}}), flush=True)
