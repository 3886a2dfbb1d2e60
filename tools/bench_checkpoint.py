#!/usr/bin/env python3
"""Checkpoints (checkpoint_every=, jsim_loop_checkpoint_save / _load) beside the fused run they cut: a
ScenarioLoop at T = 30 with config 3's four scripted vehicles, 4096 egos, 300 recorded ticks.

Per round, alternating: a fresh loop without checkpoints runs its --ticks ticks in one call (the baseline: the run as it was before
checkpoints existed), then a fresh loop for each C of --every (100, 25, 5) runs the same ticks cut at its checkpoint ticks; each
timed as the run call and a synchronise.  Then, on the last loop: one save launch alone (the slot written again, with a
synchronise), and a warm fork of every ego at the last checkpointed tick (the whole fork() call, which builds the new engine and
loop, and a synchronise).  Medians over --runs rounds after --warmup untimed ones.  Every round checks that each run with
checkpoints left the baseline's records and that the fork's state is the slot's.  Prints one JSON line and, with --out, writes
it there.

    python3 tools/bench_checkpoint.py [--runs 5] [--warmup 1] [--ticks 300] [--egos 4096] [--horizon 30] [--every 100,25,5] [--out profiles/NAME.txt]
"""
import time

import numpy as np

import recorder_bench as RB


def main():
    a = RB.arguments(runs=5, warmup=1, egos=4096, horizon=30, every="100,25,5")
    if a.runs < 3:
        raise SystemExit("bench_checkpoint: a median of fewer than three rounds says little (--runs >= 3)")
    torch, pkg = RB.setup("bench_checkpoint")
    W = pkg.workloads
    B, K, T = a.egos, a.ticks, a.horizon
    every = [int(c) for c in a.every.split(",")]
    routes = W.route_table(False)[0]
    batch = W.ego_batch(routes, B, T, rank=2)
    same = lambda x, y: torch.equal(x.nan_to_num(nan=-7.0), y.nan_to_num(nan=-7.0))   # noqa: E731

    def run(**kw):
        """(a fresh loop after K ticks, the wall ms of its run call + synchronise)."""
        eng, x0 = W.make_engine(routes, batch, T, "cuda:0")
        loop = pkg.ScenarioLoop(eng, x0, W.OBSTACLE_SPECS, max_age=W.MAX_AGE, record=K, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(K)
        torch.cuda.synchronize()
        return loop, (time.perf_counter() - t0) * 1e3

    base_ms, cut_ms, save_ms, fork_ms = [], {c: [] for c in every}, [], []
    slot_bytes = rows = 0
    for rnd in range(a.warmup + a.runs):
        keep = rnd >= a.warmup
        plain, ms = run()
        if keep:
            base_ms.append(ms)
        loop = None
        for c in every:
            if loop is not None:
                loop.loop.eng.close()
            loop, ms = run(checkpoint_every=c)
            if keep:
                cut_ms[c].append(ms)
            assert same(loop.recorder.rec, plain.recorder.rec) and torch.equal(loop.recorder.flags, plain.recorder.flags)
            assert torch.equal(loop.recorder.obs, plain.recorder.obs) and len(loop.checkpoints) == (K - 1) // c + 1
        ck = loop._ck
        slot, tick = loop.checkpoints[-1]
        slot_bytes = int(ck._bytes.sum())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ck._copy(slot, False)                   # (the loop back at the slot's tick, so that the save writes what the slot holds)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ck._copy(slot, True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        fork = loop.fork(np.arange(B), tick, warm=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if keep:
            save_ms.append((t2 - t1) * 1e3)
            fork_ms.append((t3 - t2) * 1e3)
        assert torch.equal(fork.loop.x0, ck.slabs["x0"][slot]) and torch.equal(fork.loop.eng.oa, ck.slabs["oa"][slot])
        assert torch.equal(fork.obst.state, ck.slabs["obs_state"][slot]) and torch.equal(fork.pre.traj_idx, ck.slabs["traj_idx"][slot])
        rows = fork.loop.eng.B
        for lp in (fork, loop, plain):
            lp.loop.eng.close()
    base = RB.stats(base_ms)["median"]
    res = {"egos": B, "ticks": K, "T": T, "vehicles": len(W.OBSTACLE_SPECS), "runs": a.runs, "warmup": a.warmup, "slot_bytes": slot_bytes,
           "run_ms": RB.stats(base_ms),
           "run_checkpointed_ms": {str(c): RB.stats(v) for c, v in cut_ms.items()},
           "checkpointed_over_run": {str(c): RB.stats(v)["median"] / base for c, v in cut_ms.items()},
           "pieces": {str(c): len(pkg.history.checkpoint_cuts(0, K, c, K)) for c in every},
           "save_launch_ms": RB.stats(save_ms), "warm_fork_rows": rows, "warm_fork_call_ms": RB.stats(fork_ms)}
    RB.emit(res, a.out)


if __name__ == "__main__":
    main()
