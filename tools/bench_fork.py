#!/usr/bin/env python3
"""Forking a recorded run (ScenarioLoop.fork, jsim_loop_fork_state, jsim_loop_obstacles_at) beside the fused run that made the
recording: a ScenarioLoop at T = 30 with config 3's four scripted vehicles, 4096 egos, 300 recorded ticks, every ego forked at a
tick of its own (seeded, 0 .. --ticks).

Per round, alternating: a fresh loop runs its --ticks ticks (timed: the run call and a synchronise); the two kernels alone on
buffers allocated once -- every ego's fork state, and the vehicles of every row advanced to the row's tick (4 x --egos vehicles in
one call) -- with a synchronise (timed); the whole fork() call, which builds the new engine and loop around them (timed).  Medians
over --runs rounds after --warmup untimed ones.  Every round checks the fork against the recording: a row forked at tick 0 has the
loop's first state, the forked loop's states are the kernel's, and each row's vehicles equal the recorded get() tuples of its tick.
Prints one JSON line and, with --out, writes it there.

    python3 tools/bench_fork.py [--runs 5] [--warmup 1] [--ticks 300] [--egos 4096] [--horizon 30] [--out profiles/NAME.txt]
"""
import ctypes
import time

import numpy as np

import recorder_bench as RB


def main():
    a = RB.arguments(runs=5, warmup=1, egos=4096, horizon=30)
    if a.runs < 3:
        raise SystemExit("bench_fork: a median of fewer than three rounds says little (--runs >= 3)")
    torch, pkg = RB.setup("bench_fork")
    W = pkg.workloads
    B, K, T = a.egos, a.ticks, a.horizon
    routes = W.route_table(False)[0]
    batch = W.ego_batch(routes, B, T, rank=2)
    ego = np.arange(B, dtype=np.int32)
    at = np.random.default_rng(7).integers(0, K + 1, B).astype(np.int32)
    at[:2] = 0, K                                                         # both ends are among the rows
    nv = len(W.OBSTACLE_SPECS)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                         # noqa: E731
    run_ms, kern_ms, fork_ms = [], [], []
    sets = 0
    for rnd in range(a.warmup + a.runs):
        eng, x0 = W.make_engine(routes, batch, T, "cuda:0")
        loop = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS, max_age=W.MAX_AGE, record=K)
        first = x0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(K)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rec = loop.recorder
        # the two kernels alone: outputs and the vehicles' tables allocated ahead of the clock
        xs = torch.empty(B, 4, dtype=torch.float64, device=eng.device)
        k0 = torch.empty(B, dtype=torch.int32, device=eng.device)
        state0, param = loop.obst._state0.repeat(B, 1), loop.obst.param.repeat(B, 1)
        ticks = np.repeat(at, nv).astype(np.int32)
        state = torch.empty_like(state0)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rc1 = eng.lib.jsim_loop_fork_state(eng._ctx, B, K, *rec._buffers(), B, ego.ctypes.data, at.ctypes.data, ptr(xs), ptr(k0), eng._stream())
        rc2 = eng.lib.jsim_loop_obstacles_at(eng._ctx, B * nv, ptr(state0), ptr(param), None, ticks.ctypes.data, ptr(state), eng._stream())
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        pkg._cabi.check(rc1, eng._ctx, "jsim_loop_fork_state")
        pkg._cabi.check(rc2, eng._ctx, "jsim_loop_obstacles_at")
        fork = loop.fork(ego, at)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if rnd >= a.warmup:
            run_ms.append((t1 - t0) * 1e3)
            kern_ms.append((t3 - t2) * 1e3)
            fork_ms.append((t4 - t3) * 1e3)
        assert torch.equal(xs[0], first[0]) and int(k0[0]) == 0
        assert torch.equal(fork.loop.x0, xs) and torch.equal(fork.loop.age, torch.from_numpy(at).to(eng.device) - k0)
        obs = rec.obs[:K]
        rows = torch.from_numpy(np.flatnonzero(at < K)).to(eng.device)
        got = state.reshape(B, nv, 4)[rows][:, :, :2]
        assert torch.equal(got, obs[torch.from_numpy(at[at < K].astype(np.int64)).to(eng.device)][:, :, :2])
        so, oo = fork.traffic
        mine = fork.obst.state.reshape(-1, nv, 4)[torch.from_numpy(so.astype(np.int64)).to(eng.device)]
        assert torch.equal(mine, state.reshape(B, nv, 4))                 # the forked loop's vehicles, row by row
        sets = len(oo) - 1
        fork.loop.eng.close()
        eng.close()
    res = {"egos": B, "ticks": K, "T": T, "vehicles": nv, "runs": a.runs, "warmup": a.warmup, "rows": B, "traffic_sets_of_the_fork": sets,
           "run_ms": RB.stats(run_ms), "fork_kernels_ms": RB.stats(kern_ms), "fork_call_ms": RB.stats(fork_ms),
           "kernels_over_run": RB.stats(kern_ms)["median"] / RB.stats(run_ms)["median"],
           "fork_over_run": RB.stats(fork_ms)["median"] / RB.stats(run_ms)["median"]}
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
