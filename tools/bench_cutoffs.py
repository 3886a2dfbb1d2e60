#!/usr/bin/env python3
"""The collision cut-off of every recorded tick (Recorder.cutoffs, jsim_loop_eval_cutoffs) beside the fused run that made the
recording: a ScenarioLoop at T = 30 with config 3's four scripted vehicles, 4096 egos, 300 recorded ticks.

The replay redoes the glue share of the run -- progress index, resampling, collision rows, cut-off, once per ego and tick -- so its
time is set beside the run's own, taken in the same process, the two alternating: per round a fresh loop runs its --ticks ticks
(timed: the run call and a synchronise), then its recorder is replayed (timed: the entry point's launches on device outputs and a
synchronise; and the whole Recorder.cutoffs() call with its read-back).  Medians over --runs rounds after --warmup untimed ones.
Every round checks the replay against what the live loop left: the carry is the loop's glue state, and the last tick's status, hit
and cut-off are the loop's pre_status, col_flag and path_len.  Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_cutoffs.py [--runs 5] [--warmup 1] [--ticks 300] [--egos 4096] [--horizon 30] [--out profiles/NAME.txt]
"""
import time

import recorder_bench as RB


def main():
    a = RB.arguments(runs=5, warmup=1, egos=4096, horizon=30)
    if a.runs < 3:
        raise SystemExit("bench_cutoffs: a median of fewer than three rounds says little (--runs >= 3)")
    torch, pkg = RB.setup("bench_cutoffs")
    W = pkg.workloads
    B, K, T = a.egos, a.ticks, a.horizon
    routes = W.route_table(False)[0]
    batch = W.ego_batch(routes, B, T, rank=2)
    run_ms, launch_ms, call_ms = [], [], []
    hits = refused = 0
    for rnd in range(a.warmup + a.runs):
        eng, x0 = W.make_engine(routes, batch, T, "cuda:0")
        loop = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS, max_age=W.MAX_AGE, record=K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(K)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d = loop.recorder._cutoffs_device()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out = loop.recorder.cutoffs()
        t3 = time.perf_counter()
        if rnd >= a.warmup:
            run_ms.append((t1 - t0) * 1e3)
            launch_ms.append((t2 - t1) * 1e3)
            call_ms.append((t3 - t2) * 1e3)
        pre = loop.pre
        ok = pre.status == 0
        assert torch.equal(d["carry"][:, 0], pre.traj_idx.to(torch.int32)) and torch.equal(d["carry"][:, 1], pre.prev_len)
        assert torch.equal(d["carry"][:, 2], eng.path_len) and torch.equal(d["cut"][-1], eng.path_len)
        assert torch.equal(d["status"][-1], pre.status) and torch.equal(d["hit"][-1][ok], pre.col_flag[ok])
        hits, refused = int(out["hit"].sum()), int((out["status"] != 0).sum())
    res = {"egos": B, "ticks": K, "T": T, "vehicles": len(W.OBSTACLE_SPECS), "runs": a.runs, "warmup": a.warmup,
           "run_ms": RB.stats(run_ms), "replay_launch_ms": RB.stats(launch_ms), "replay_call_ms": RB.stats(call_ms),
           "replay_over_run": RB.stats(launch_ms)["median"] / RB.stats(run_ms)["median"], "ego_ticks_cut_off": hits,
           "ego_ticks_refused": refused}
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
