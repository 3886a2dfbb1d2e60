"""What the GPU tests of the recorder's evaluators hold a LIVE recorder to, in one place, so that a test of another workload (route
traffic: tests/test_gpu_traffic_route_glue.py) holds its recording to the same restatements at the same bars: conflicts
(tests/test_gpu_conflicts.py), gaps (tests/test_gpu_gaps.py), headway (tests/test_gpu_headway.py), tracking
(tests/test_gpu_tracking.py) and the replayed cut-offs (tests/test_gpu_cutoffs.py).  Moved here from those files as they stood;
each file imports its own back under the names it had."""
import numpy as np
import torch

import conflicts_numpy as CN
import gap_cases as GC
import gaps_numpy as GN
import headway_numpy as HN
import tracking_numpy as TN

# ---- conflicts (jsim_loop_eval_conflicts, Recorder.conflicts)
CONFLICTS_BAR = 1e-12


def clear_err(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def conflicts_equal_restatement(out, ref, what):
    for k in ("who", "row", "hit_tick", "hit_frame"):
        assert np.array_equal(out[k], ref[k]), (what, k)
    assert np.array_equal(out["hit_xy"], ref["hit_xy"], equal_nan=True), what
    err = clear_err(out["clear"], ref["clear"])
    print(f"{what}: clear against the restatement, maximum error {err:.3g}")
    assert err <= CONFLICTS_BAR, (what, err)
    return err


def conflicts_restate_recorder(r, res):
    obs = r.obs.cpu().numpy() if r.obs is not None else None
    shapes = r.loop.eng.vehicle_shapes
    return CN.eval_conflicts(r.rec.cpu().numpy(), r.flags.cpu().numpy(), obs, r.x0_first.cpu().numpy(), r.loop.x0_spawn.cpu().numpy(),
                             res["veh_range"], res["mate_range"], shapes, res["ego_shape"], res["frame_window"])


# ---- gaps (jsim_loop_eval_gaps, Recorder.gaps): every output is an integer, every comparison exact
GAPS_ALL = ("off", "gap", "who", "ep_gap", "ep_tick", "ep_who", "ep_off")


def gaps_assert_same(out, ref, what):
    for k in GAPS_ALL:
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), (what, k)


def gaps_restate_recorder(r, res):
    obs = r.obs.cpu().numpy() if r.obs is not None else None
    n = res["off"].shape[0]
    return GN.eval_gaps(r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy(), None if obs is None else obs[:n], r.x0_first.cpu().numpy(),
                        r.loop.x0_spawn.cpu().numpy(), res["veh_range"], res["mate_range"], r.loop.eng.vehicle_shapes, res["ego_shape"],
                        res["window"], GN.WITHIN[res["within"]])


def gaps_check_recorder(pkg, r, n, what):
    """Both rules at windows 20 and 63 against the restatement on the recorder's own arrays, the equivalence with conflicts(), and
    gap_episodes' split."""
    flags = r.flags[:n].cpu().numpy()
    found = {}
    for rule in GC.RULES:
        for w in (20, 63):
            res = r.gaps(window=w, within=rule)
            assert res["off"].shape == (n, r.loop.eng.B, 8) and res["off"].dtype == np.int8 and (res["window"], res["within"]) == (w, rule)
            gaps_assert_same(res, gaps_restate_recorder(r, res), (what, rule, w))
            eps = pkg.history.gap_episodes(res, flags, r.loop.eng.dt)
            assert [len(e) for e in eps] == r.episodes()["count"].tolist()
            found[rule, w] = [e["gap"] for ep in eps for e in ep]
    wide = r.gaps(window=20)
    assert wide["within"] == "episode"
    for w in (0, 1, 3, 20):
        contact = r.conflicts(frame_window=w)["contact"]
        assert np.array_equal((wide["gap"] >= 0) & (wide["gap"] <= w), contact), (what, w)
        assert np.array_equal(r.gaps(window=w)["gap"] >= 0, contact), (what, w)
    print(f"{what}: episode gaps at window 63 {found['episode', 63]}; under the record rule {found['record', 63]}")
    return found


# ---- headway (jsim_loop_eval_headway, Recorder.headway): the bars of tests/test_gpu_headway.py, whose docstring derives them
HEADWAY_INTS = ("lead", "ttc_who", "ep_i")
HEADWAY_PLACES = ("gap", "lat", "rate")
HEADWAY_TICKS = ("lead_gap", "thw", "ttc", "u_ego")
HEADWAY_DOUBLES = HEADWAY_TICKS + ("ep_d",) + HEADWAY_PLACES
HEADWAY_KEYS = ("lead", "lead_gap", "thw", "ttc", "ttc_who", "u_ego", "ep_i", "ep_d") + HEADWAY_PLACES      # the entry point's order
HEADWAY_OF_VALUE = ("thw", "ttc", "ep_d.thw_min", "ep_d.ttc_min", "ep_d.thw_mean")   # relative to the value itself
HEADWAY_EP_D = ("gap_min", "thw_min", "ttc_min", "thw_mean")
HEADWAY_SEEN = {"gap": 7.11e-15, "lat": 3.67e-15, "rate": 1.59e-15, "lead_gap": 5.11e-15, "thw": 2.47e-16, "ttc": 1.01e-15, "u_ego": 2.22e-16,
                "ep_d.gap_min": 0.0, "ep_d.thw_min": 0.0, "ep_d.ttc_min": 0.0, "ep_d.thw_mean": 2.39e-16}    # the first run's largest errors, rounded up
HEADWAY_CAP = 1e-12
HEADWAY_BARS = {k: min(4.0 * v, HEADWAY_CAP) for k, v in HEADWAY_SEEN.items()}


def headway_relative(out, ref, of_value):
    """|device - restatement| relative to max(1, |restatement|), or to the value itself; inf and NaN must sit in the same slots."""
    assert out.shape == ref.shape and np.array_equal(np.isnan(out), np.isnan(ref)) and np.array_equal(np.isinf(out), np.isinf(ref))
    fin = np.isfinite(ref)
    assert np.array_equal(out[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])     # the sign of an inf
    scale = np.abs(ref[fin]) if of_value else np.maximum(1.0, np.abs(ref[fin]))
    err = np.abs(out[fin] - ref[fin])
    assert np.all(err[scale == 0.0] == 0.0)                               # (a 0.0 is exact on both sides)
    return float((err[scale > 0.0] / scale[scale > 0.0]).max(initial=0.0))


def headway_errors(out, ref, what, worst=None, keys=HEADWAY_DOUBLES):
    """Integers exact; inf and NaN where the restatement has them; prints the largest relative error per double output (ep_d by
    column), then asserts each within its bar.  `worst` collects the largest over several calls."""
    seen = {}
    for k in HEADWAY_INTS:
        assert out[k].dtype == np.int32 and np.array_equal(out[k], ref[k]), (what, k, np.argwhere(out[k] != ref[k])[:5])
    for k in keys:
        if k == "ep_d":
            seen.update({f"ep_d.{name}": headway_relative(out[k][..., j], ref[k][..., j], f"ep_d.{name}" in HEADWAY_OF_VALUE)
                         for j, name in enumerate(HEADWAY_EP_D)})
        else:
            seen[k] = headway_relative(out[k], ref[k], k in HEADWAY_OF_VALUE)
    print(f"{what}: largest relative error {seen}")
    if worst is not None:
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= HEADWAY_BARS[k] for k, v in seen.items()), (what, {k: v for k, v in seen.items() if v > HEADWAY_BARS[k]})
    return seen


def headway_same_bits(a, b, what, keys=HEADWAY_KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def headway_restate_recorder(r, res, paths):
    n = res["lead"].shape[0]
    obs = r.obs.cpu().numpy() if r.obs is not None else None
    return HN.eval_headway(r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy(), None if obs is None else obs[:n], r.x0_first.cpu().numpy(),
                           r.loop.x0_spawn.cpu().numpy(), res["veh_range"], res["mate_range"], r.loop.eng.vehicle_shapes, res["ego_shape"],
                           res["path_id"], paths, res["margin"])


def headway_check_recorder(pkg, r, n, what, worst, paths=None, path_id=None, margin=0.0):
    """headway() against the restatement on the recorder's own arrays, places=False, and headway_episodes' split."""
    eng = r.loop.eng
    res = r.headway(paths=paths, path_id=path_id, margin=margin)
    assert res["lead"].shape == (n, eng.B) and res["gap"].shape == (n, eng.B, 8) and res["ep_i"].shape == (n, eng.B, 7) and res["ep_d"].shape == (n, eng.B, 4)
    assert res["margin"] == margin
    ref = headway_restate_recorder(r, res, eng.paths if paths is None else paths)
    headway_errors(res, ref, what, worst)
    bare = r.headway(paths=paths, path_id=path_id, margin=margin, places=False)
    assert not any(k in bare for k in HEADWAY_PLACES)
    headway_same_bits(bare, res, what, keys=[k for k in HEADWAY_KEYS if k not in HEADWAY_PLACES])
    eps = pkg.history.headway_episodes(res, r.flags[:n].cpu().numpy(), eng.dt)
    assert [len(e) for e in eps] == r.episodes()["count"].tolist()
    assert all(e["time_following"] == e["lead_ticks"] * eng.dt for ep in eps for e in ep)
    print(f"{what}: per ego (ticks, lead ticks, smallest gap, smallest thw, smallest ttc) of the first episode "
          f"{[(e[0]['n'], e[0]['lead_ticks'], round(e[0]['gap_min'], 3), round(e[0]['thw_min'], 3), round(e[0]['ttc_min'], 3)) for e in eps]}")
    return res


# ---- tracking (jsim_loop_eval_tracking, Recorder.tracking)
TRACKING_INTS, TRACKING_DOUBLES = ("idx", "seg", "ep_i"), ("s", "d", "e_yaw", "ep_d")
TRACKING_BAR = 1e-12


def tracking_errors(out, ref, what):
    """Integers exact, NaN where the restatement has NaN; returns the largest |device - restatement| / max(1, |restatement|) per
    double output (ep_d by column), after asserting it is within the bar."""
    worst = {}
    for k in TRACKING_INTS:
        assert out[k].dtype == np.int32 and np.array_equal(out[k], ref[k]), (what, k)
    for k in TRACKING_DOUBLES:
        assert out[k].shape == ref[k].shape and np.array_equal(np.isnan(out[k]), np.isnan(ref[k])), (what, k)
        with np.errstate(invalid="ignore"):
            rel = np.nan_to_num(np.abs(out[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])), nan=0.0)
        if k == "ep_d":
            worst.update({f"ep_d.{name}": float(rel[..., j].max(initial=0.0)) for j, name in enumerate(("d_max", "d2_mean", "yaw_max", "s_first", "s_last"))})
        else:
            worst[k] = float(rel.max(initial=0.0))
    print(f"{what}: largest relative error {worst}")
    assert max(worst.values()) <= TRACKING_BAR, (what, worst)
    return worst


def tracking_restate_recorder(r, n, paths, path_id):
    return TN.eval_tracking(r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy(), path_id, paths)


def tracking_check_recorder(pkg, r, n, what, paths=None, path_id=None):
    """tracking() against the restatement on the recorder's own arrays, and tracking_episodes' split."""
    eng = r.loop.eng
    res = r.tracking(paths=paths, path_id=path_id)
    assert res["idx"].shape == (n, eng.B) and res["ep_i"].shape == (n, eng.B, 2) and res["ep_d"].shape == (n, eng.B, 5)
    use_paths = eng.paths if paths is None else paths
    own = eng.path_id.cpu().numpy() if paths is None else np.zeros(eng.B, dtype=np.int32)
    assert np.array_equal(res["path_id"], own if path_id is None else np.broadcast_to(path_id, (eng.B,)))
    ref = tracking_restate_recorder(r, n, use_paths, res["path_id"])
    tracking_errors(res, ref, what)
    assert len(res["arc"]) == len(use_paths) and all(np.array_equal(a, b) for a, b in zip(res["arc"], ref["arc"]))
    assert (res["idx"] >= 0).all() and np.isfinite(res["d"]).all()
    eps = pkg.history.tracking_episodes(res, r.flags[:n].cpu().numpy(), eng.dt, stations=[1.0, 5.0], free_speed=float(eng.speed.max()))
    assert [len(e) for e in eps] == r.episodes()["count"].tolist()
    print(f"{what}: path ids {res['path_id'].tolist()}, per ego (ticks, d_max, d_rms, progress, delay) of the first episode "
          f"{[(e[0]['n'], round(e[0]['d_max'], 3), round(e[0]['d_rms'], 3), round(e[0]['progress'], 2), round(e[0]['delay'], 2)) for e in eps]}")
    return res


# ---- the replayed cut-offs (jsim_loop_eval_cutoffs, Recorder.cutoffs) against a live loop's glue
def live_rows(rows):
    """The per-tick reads of a live loop, stacked like the replay's outputs.  A tick the glue refused keeps the loop's col_flag as it
    was; the replay reports no hit there (the header's rule), so that is what the live series says too."""
    d = {k: torch.stack([r[k] for r in rows]) for k in rows[0]}
    d["hit"] = torch.where(d["status"] == 0, d["hit"], torch.zeros_like(d["hit"]))
    return d


def assert_replay_equals_live(rep, live, what, keys=("status", "idx", "cut", "hit")):
    for k in keys:
        assert torch.equal(rep[k], live[k].to(rep[k].dtype)), (what, k)
    hit = rep["hit"] != 0
    assert bool(torch.isnan(rep["col_xy"][~hit]).all()) and bool((rep["first"][~hit] == -1).all()), what
    assert bool(torch.isfinite(rep["col_xy"][hit]).all()) and bool((rep["first"][hit] >= 0).all()), what
    if "col_xy" in live:
        assert torch.equal(rep["col_xy"][hit], live["col_xy"][hit]) and torch.equal(rep["first"][hit], live["first"][hit]), what


def run1_rows(loop, K):
    """K x run(1) of a loop: the live path_len, col_flag, pre_status and progress index behind every tick, and which egos the tick
    respawned (their progress index has been reset by then)."""
    eng, pre = loop.loop.eng, loop.pre
    rows, resp = [], []
    for _ in range(K):
        loop.run(1)
        rows.append({"status": pre.status.clone(), "idx": pre.traj_idx.clone(), "hit": pre.col_flag.clone(), "cut": eng.path_len.clone()})
        resp.append((loop.loop.age == 0).clone())
    torch.cuda.synchronize()
    return live_rows(rows), torch.stack(resp)


def assert_replay_equals_run1(rep, live, resp, what):
    assert_replay_equals_live(rep, live, what, keys=("status", "cut", "hit"))
    assert torch.equal(rep["idx"][~resp], live["idx"][~resp].to(torch.int32)), what
