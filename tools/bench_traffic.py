#!/usr/bin/env python3
"""Traffic sets at config 3's scale: 4096 egos, T = 30, four scripted vehicles per ego, the workload run three ways --
  shared     config 3 itself: every ego meets workloads.OBSTACLE_SPECS (ScenarioLoop.run: one rollout, one prediction, fused)
  per_ego    every ego its own set of four t-intersection / roundabout / no vehicles (workloads.traffic_batch, 16384 vehicles in
             all; ScenarioLoop(traffic_of=...).run: gridded rollout + prediction, fused launches of traffic_chunk_ticks ticks)
  per_group  1024 intersections of four interacting egos (workloads.interacting_batch), each with its own set of four
             (InteractingLoop(traffic_of=...).run: host ticks)
Prints one JSON line per way: ego-steps/s over `ticks` device-synchronised ticks after `warmup` ticks, ms per tick and the
ego-ticks cut at the last tick.

The kernel-time share of the obstacle rollout and prediction comes from a profiled run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python3 tools/bench_traffic.py --ways per_ego
    python3 tools/bench_traffic.py --summarize OUT        # the share of every obstacle_* / *_pre_tick / MPC kernel

    python3 tools/bench_traffic.py [--egos 4096] [--ticks 60] [--warmup 10] [--ways shared per_ego per_group]
"""
import argparse
import importlib
import json
import os
import sys

from loop_bench import loop_fields, scenario_loop, summarize, timed_run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ways", nargs="+", default=["shared", "per_ego", "per_group"], choices=["shared", "per_ego", "per_group"])
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    pkg = importlib.import_module("av-simulation-at-intersections_amd")
    W = pkg.workloads
    routes = W.route_table(False)[0]
    T, B = a.horizon, a.egos
    for way in a.ways:
        if way == "per_group":
            batch, sizes = W.interacting_batch(routes, B // 4, T, seed=1)
            eng, x0 = W.make_engine(routes, batch, T, "cuda:0")
            sets, tog = W.traffic_batch(B // 4, seed=2, vehicles=4)
            loop = pkg.InteractingLoop(eng, x0, group_sizes=sizes, obstacle_specs=sets, max_age=W.MAX_AGE, traffic_of=tog)
        elif way == "shared":
            loop = scenario_loop(pkg, routes, B, T, W.OBSTACLE_SPECS)
        else:
            sets, tof = W.traffic_batch(B, seed=2, vehicles=4)
            loop = scenario_loop(pkg, routes, B, T, sets, traffic_of=tof)
        dt = timed_run(loop, a.warmup, a.ticks)
        print(json.dumps({"way": way, **loop_fields(loop, a.ticks, dt)}), flush=True)


if __name__ == "__main__":
    main()
