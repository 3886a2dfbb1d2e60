#!/usr/bin/env python3
"""Every recorded prediction scored as ONE launch (Recorder.predictions, jsim_loop_score_predictions), on three
recordings at T = 13:
  shared       --ticks ticks of 4096 egos with config 3's four shared vehicles (ScenarioLoop): the four vehicle rows, and with
               egos="constant" the 4096 ego rows as well
  interacting  1024 groups of 4 interacting egos (workloads.interacting_batch, InteractingLoop under the constant rule): the egos scored
  per_ego      tools/bench_traffic.py's per-ego traffic: every ego its own set of up to four vehicles (14762 rows)

Per recording: the launch alone, between two HIP events on the engine's stream, on buffers that stay on the device (median / min /
max of --runs launches after --warmup untimed ones); the whole Recorder.predictions() call with its read-back (wall ms, timed the
same way); the numpy restatement (tests/predictions_numpy.py) on the first --numpy-rows rows (numpy_ms; numpy_ms_scaled = per row
times V), whose result the device's is compared with (integers exactly, doubles within 1e-9); and what making the same predictions
costs where Recorder.cutoffs() makes them -- written to memory, by the loops' predictors: the egos' as ego_predict_kernel on
ticks x B rows in chunks of a 512 MiB budget (jsim_loop_predict_egos: cutoffs()' own launches), the vehicles' as one
jsim_loop_predict_obstacles per tick where there are at most eight (`per_tick_calls`: cutoffs() makes them in one gridded launch
per chunk, which no entry point exposes), else as the egos' kernel on ticks x n_obs rows (`dense_stand_in`: the same arithmetic per
row).  For the interacting recording the constant rule's error curve (history.prediction_curve, mean over the ego rows) goes with it.
Prints one JSON line and, with --out, writes it there.

The prediction launches of Recorder.cutoffs() themselves, from a kernel trace of their own (one run per recording):
    rocprofv3 --kernel-trace -d OUT/NAME --output-format csv -- python3 tools/bench_predictions.py --trace-cutoffs NAME
    python3 tools/bench_predictions.py --summarize OUT

--rule plan: the interacting recording made with record_plans=True, once under each mate prediction.  Per
recording: jsim_loop_score_plan_predictions' launch alone; beside it jsim_loop_predict_egos_plan over the same ticks x B rows --
the call that makes the same predictions and writes them to memory, on slabs of the plan record in chunks of the 512 MiB budget --,
jsim_loop_score_predictions' launch with the egos (the constant rule, on the same recording) and the whole
Recorder.predictions(egos="plan") call with its read-back; then both rules' mean error by look-ahead, ade, fde and mean hold time.
`speed_bar_met`: the new launch's median is no more than the writing call's median plus that call's own min-max spread.

    python3 tools/bench_predictions.py [--runs 9] [--warmup 2] [--ticks 300] [--numpy-rows 16] [--only NAME] [--out profiles/NAME.txt]
    python3 tools/bench_predictions.py --rule plan [--runs 9] [--warmup 2] [--ticks 300] [--out FILE]
"""
import sys

import numpy as np

import recorder_bench as RB


def record(pkg, torch, name, K, **interacting_kw):
    W = pkg.workloads
    routes = W.route_table(False)[0]
    if name == "shared":
        return RB.recorded_loop(pkg, torch, 4096, K), "constant"
    if name == "interacting":
        batch, sizes = W.interacting_batch(routes, 1024, RB.T, seed=1)
        eng, x0 = W.make_engine(routes, batch, RB.T, "cuda:0")
        loop = pkg.InteractingLoop(eng, x0, group_sizes=sizes, max_age=W.MAX_AGE, hist_cap=K, record=K, **interacting_kw)
    else:
        sets, tof = W.traffic_batch(4096, seed=2, vehicles=4)
        eng, x0 = W.make_engine(routes, W.ego_batch(routes, 4096, RB.T), RB.T, "cuda:0")
        loop = pkg.ScenarioLoop(eng, x0, sets, max_age=W.MAX_AGE, traffic_of=tof, hist_cap=K, record=K)
    loop.run(K)
    torch.cuda.synchronize()
    return loop.recorder, None


def events(torch, fn, runs, warmup):
    ts = []
    for run in range(warmup + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if run >= warmup:
            ts.append(t0.elapsed_time(t1))
    return RB.stats(ts)


def launch_alone(pkg, torch, r, egos, runs, warmup):
    eng = r.loop.eng
    d = r._predictions_device(egos=egos, steps=False)
    p = lambda t: None if t is None else t.data_ptr()
    n = d["pt_i"].shape[0]

    def call():
        rc = eng.lib.jsim_loop_score_predictions(eng._ctx, eng.B, n, p(r.rec), p(r.flags), r.n_obs, p(r.obs), p(r.x0_first), p(r.loop.x0_spawn),
                                                 int(d["egos"]), d["n_steps"], d["tol"], p(d["pt_i"]), p(d["pt_d"]), p(d["step_sum"]),
                                                 p(d["step_cnt"]), None, eng._stream())
        pkg._cabi.check(rc, eng._ctx, "jsim_loop_score_predictions")
    return events(torch, call, runs, warmup), d


def written_predictions(pkg, torch, r, d, runs, warmup):
    """What the same predictions cost made the way cutoffs() makes them (see the module's text)."""
    eng, S, n = r.loop.eng, d["n_steps"], d["pt_i"].shape[0]
    p = lambda t: t.data_ptr()
    out = {}

    def ego_kernel(rows):
        chunk = max(1, min(rows, (512 << 20) // (S * 32 + 80)))
        x0, di = torch.zeros(chunk, 4, dtype=torch.float64, device=eng.device), torch.zeros(chunk, 2, dtype=torch.float64, device=eng.device)
        x0[:, 2] = 5.0

        def call():
            for lo in range(0, rows, chunk):
                pkg._cabi.check(eng.lib.jsim_loop_predict_egos(eng._ctx, min(chunk, rows - lo), p(x0), p(di), S, None, eng._stream()), eng._ctx,
                                "jsim_loop_predict_egos")
        return events(torch, call, runs, warmup)
    if d["egos"]:
        out["egos_ms"] = ego_kernel(n * eng.B)
    if 0 < r.n_obs <= 8:
        pred = torch.zeros(r.n_obs, S, 3, dtype=torch.float64, device=eng.device)

        def call():
            for k in range(n):
                pkg._cabi.check(eng.lib.jsim_loop_predict_obstacles(eng._ctx, r.n_obs, p(r.obs[k]), S, p(pred), eng._stream()), eng._ctx,
                                "jsim_loop_predict_obstacles")
        out["vehicles_ms"], out["vehicles_how"] = events(torch, call, runs, warmup), "per_tick_calls"
    elif r.n_obs > 8:
        out["vehicles_ms"], out["vehicles_how"] = ego_kernel(n * r.n_obs), "dense_stand_in"
    return out


def trace_cutoffs(pkg, torch, name, K):
    """Under `rocprofv3 --kernel-trace`: one untimed Recorder.cutoffs(), then one between two fork_state launches (a kernel nothing
    else here launches), so that --summarize can tell the replay's own prediction launches from the loop's."""
    r, _ = record(pkg, torch, name, K)
    r._cutoffs_device()
    torch.cuda.synchronize()
    r.fork_state(0, 0)
    r._cutoffs_device()
    r.fork_state(0, 0)
    torch.cuda.synchronize()


def summarize(out_dir):
    """Per *kernel_trace.csv under out_dir: the kernels between the two fences, ms by name, and the prediction launches' total."""
    import csv
    import glob
    import json
    import os
    for path in sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)):
        rows = sorted(csv.DictReader(open(path)), key=lambda q: int(q["Start_Timestamp"]))
        fences = [i for i, q in enumerate(rows) if "fork_state_kernel" in q["Kernel_Name"]]
        if len(fences) != 2:
            raise SystemExit(f"{path}: {len(fences)} fences, not 2")
        by = {}
        for q in rows[fences[0] + 1:fences[1]]:
            k = q["Kernel_Name"].split("(")[0]
            c, t = by.get(k, (0, 0))
            by[k] = (c + 1, t + int(q["End_Timestamp"]) - int(q["Start_Timestamp"]))
        pred = sum(t for k, (c, t) in by.items() if any(w in k for w in ("obstacle_predict_kernel", "ego_predict_kernel", "cutoff_mate_state_kernel")))
        print(json.dumps({"trace": os.path.relpath(path, out_dir), "prediction_launches_ms": pred / 1e6,
                          "kernels": {k: {"calls": c, "ms": t / 1e6} for k, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1])}}), flush=True)


def plan_rule(pkg, torch, a):
    """--rule plan: see the module's text."""
    K = a.ticks
    res = {"rule": "plan", "ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "recordings": {}}
    p = lambda t: None if t is None else t.data_ptr()
    for mode in ("constant", "plan"):
        r, _ = record(pkg, torch, "interacting", K, mate_prediction=mode, record_plans=True)
        eng = r.loop.eng
        B, T = eng.B, eng.T
        d = r._predictions_device(egos="plan")
        n, S, tol = d["pt_i"].shape[0], d["n_steps"], d["tol"]
        oa, od, st = r.plans.values()

        def score_plan():
            pkg._cabi.check(eng.lib.jsim_loop_score_plan_predictions(eng._ctx, B, n, p(r.rec), p(r.flags), p(r.x0_first), p(r.loop.x0_spawn), p(oa),
                                                                     p(od), p(st), S, tol, p(d["pt_i"]), p(d["pt_d"]), p(d["step_sum"]),
                                                                     p(d["step_cnt"]), None, eng._stream()), eng._ctx, "jsim_loop_score_plan_predictions")
        rows = n * B
        chunk = max(1, min(rows, (512 << 20) // (S * 32 + 80)))
        x0, di = torch.zeros(chunk, 4, dtype=torch.float64, device=eng.device), torch.zeros(chunk, 2, dtype=torch.float64, device=eng.device)
        x0[:, 2] = 5.0
        oa_f, od_f, st_f = oa.view(-1, T), od.view(-1, T), st.view(-1)

        def write_plan():
            for lo in range(0, rows, chunk):
                pkg._cabi.check(eng.lib.jsim_loop_predict_egos_plan(eng._ctx, min(chunk, rows - lo), p(x0), p(oa_f[lo:]), p(od_f[lo:]), p(st_f[lo:]),
                                                                    p(di), S, None, eng._stream()), eng._ctx, "jsim_loop_predict_egos_plan")
        new, alt = events(torch, score_plan, a.runs, a.warmup), events(torch, write_plan, a.runs, a.warmup)
        const_launch, _ = launch_alone(pkg, torch, r, "constant", a.runs, a.warmup)
        ts, out = RB.timed(lambda: r.predictions(egos="plan"), a.runs, a.warmup)
        row = {"mate_prediction": mode, "B": B, "rows_per_launch": B, "predictions": rows, "n_steps": S, "tol": tol,
               "score_plan_launch_ms": new, "predict_egos_plan_written_ms": alt, "written_chunks": -(-rows // chunk),
               "speed_bar_ms": alt["median"] + (alt["max"] - alt["min"]), "speed_bar_met": new["median"] <= alt["median"] + (alt["max"] - alt["min"]),
               "score_constant_launch_ms": const_launch, "call_ms": RB.stats(ts), "plan_record_bytes": int(sum(t.numel() * t.element_size() for t in r.plans.values()))}
        for rule, o in (("plan", out), ("constant", r.predictions(egos="constant"))):
            t, _ = pkg.history.prediction_curve(o, eng.dt)
            with np.errstate(invalid="ignore"):
                mean = np.nansum(o["step_sum"], axis=0) / np.maximum(o["step_cnt"].sum(axis=0), 1)
            pick = [0, 4, 9, 14, 19, 24, 29, S - 1] if S >= 30 else list(range(S))
            held = o["hold"] >= o["n"]                                      # within tol on every scored sample
            row[rule] = {"t": [round(float(v), 3) for v in t[pick]], "mean_error": [float(v) for v in mean[pick]],
                         "ade_mean": float(np.nanmean(o["ade"])), "fde_mean": float(np.nanmean(o["fde"])), "hold_mean_s": float(o["hold"].mean() * eng.dt),
                         "held_to_the_end_share": float(held.mean()), "samples": int(o["step_cnt"].sum())}
        res["recordings"][mode] = row
        print(f"{mode}: {row}", file=sys.stderr, flush=True)
        del r, d, oa, od, st, oa_f, od_f, st_f, out
        torch.cuda.empty_cache()
    RB.emit(res, a.out)


def main():
    a = RB.arguments(runs=9, warmup=2, numpy_rows=16, only="", trace_cutoffs="", summarize="", rule="constant")
    if a.summarize:
        return summarize(a.summarize)
    torch, pkg = RB.setup("bench_predictions")
    if a.rule == "plan":
        return plan_rule(pkg, torch, a)
    if a.rule != "constant":
        raise SystemExit(f"--rule must be constant or plan, got {a.rule!r}")
    if a.trace_cutoffs:
        return trace_cutoffs(pkg, torch, a.trace_cutoffs, a.ticks)
    import predictions_numpy as PN
    K = a.ticks
    res = {"ticks": K, "T": RB.T, "runs": a.runs, "warmup": a.warmup, "numpy_rows": a.numpy_rows, "recordings": {}}
    worst, wrong = 0.0, 0
    for name in ((a.only,) if a.only else ("shared", "interacting", "per_ego")):
        r, extra = record(pkg, torch, name, K)
        eng = r.loop.eng
        for egos in ((None, extra) if extra else (None,)):
            key = name if egos is None else f"{name}+egos"
            launch, d = launch_alone(pkg, torch, r, egos, a.runs, a.warmup)
            ts, out = RB.timed(lambda: r.predictions(egos=egos), a.runs, a.warmup)
            V, S = out["ade"].shape[1], out["n_steps"]
            row = {"B": eng.B, "n_obs": r.n_obs, "rows": V, "egos": out["egos"], "n_steps": S, "tol": out["tol"], "launch_ms": launch,
                   "call_ms": RB.stats(ts), "output_bytes": K * V * (4 * 3 + 8 * 6) + V * S * 12,
                   "written_predictions": written_predictions(pkg, torch, r, d, a.runs, a.warmup)}
            print(f"{key}: {V} rows, launch {launch}, call {row['call_ms']}; the restatement next", file=sys.stderr, flush=True)
            # the restatement on the first vehicle rows and the first ego rows
            m = min(a.numpy_rows, V)
            mv = min(m, r.n_obs) if not out["egos"] else min(m // 2, r.n_obs)
            me = min(m - mv, eng.B) if out["egos"] else 0
            obs = r.obs[:K, :mv].cpu().numpy() if mv else None
            L_obs = np.full(mv, eng.L) if eng.vehicle_shapes is None else np.asarray(eng.vehicle_shapes)[:mv, 3]
            host = (r.rec[:K, :max(me, 1)].cpu().numpy(), r.flags[:K, :max(me, 1)].cpu().numpy(), obs, r.x0_first[:max(me, 1)].cpu().numpy(),
                    r.loop.x0_spawn[:max(me, 1)].cpu().numpy())
            tn, ref = RB.timed(lambda: PN.eval_predictions(*host, me > 0, S, out["tol"], eng.dt, L_obs, eng.L), 1)
            rows = list(range(mv)) + [r.n_obs + b for b in range(me)]
            row["numpy_ms"], row["numpy_ms_scaled"] = tn[0], tn[0] * V / max(len(rows), 1)
            for j, k in enumerate(pkg.history.PS_INT):
                wrong += int((out[k][:, rows] != ref["pt_i"][:, :, j]).sum())
            for j, k in enumerate(pkg.history.PS_DOUBLE):
                mine, want = out[k][:, rows], ref["pt_d"][:, :, j]
                wrong += int((np.isnan(mine) != np.isnan(want)).sum())
                worst = max(worst, float(np.nanmax(np.abs(mine - want), initial=0.0)))
            t, curve = pkg.history.prediction_curve(out, eng.dt)
            first = r.n_obs if out["egos"] else 0
            with np.errstate(invalid="ignore"):
                mean = np.nansum(out["step_sum"][first:], axis=0) / np.maximum(out["step_cnt"][first:].sum(axis=0), 1)
            row["curve_of"] = "egos" if out["egos"] else "vehicles"
            row["curve"] = {"t": [round(float(v), 3) for v in t[[0, 4, 9, 14, 19, 24, 29, S - 1]]] if S >= 30 else t.tolist(),
                            "mean_error": [float(v) for v in (mean[[0, 4, 9, 14, 19, 24, 29, S - 1]] if S >= 30 else mean)]}
            row["ade_mean"], row["fde_mean"], row["hold_mean_s"] = (float(np.nanmean(out["ade"][:, first:])), float(np.nanmean(out["fde"][:, first:])),
                                                                     float(out["hold"][:, first:].mean() * eng.dt))
            res["recordings"][key] = row
        del r
        torch.cuda.empty_cache()
    res["max_err"], res["mismatches"] = worst, wrong
    RB.emit(res, a.out, "the device result differs from the restatement: see max_err / mismatches" if wrong or worst > 1e-9 else None)


if __name__ == "__main__":
    main()
