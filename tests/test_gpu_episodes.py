"""One row per recorded episode on the device (jsim_loop_summarise_episodes, Recorder.summary): every ego of
episode_cases in one launch at ten tick counts and with every choice of groups, against the plain-loop restatement; a cut launch
against the long one; the batch layout; the scan across a workgroup tile; a table that is too small; and a ScenarioLoop and an
InteractingLoop, whose summary is compared with the restatement on the recorder's own downloaded arrays and with the host-side
conflict_episodes / static_episodes.

Bars: every integer column, minimum, maximum and copied value exact.  The three sums (length, v_mean, dev_mean) within
1e-12 x max(1, |value|) of math.fsum: at most 200 non-negative terms, each addition off by at most 1.1e-16 of the running sum, behind
one square root per term -- 200 x 1.1e-16 = 2.2e-14, section 17's bar for `clear`."""
import numpy as np
import pytest
import torch

import episode_cases as EC
import episodes_numpy as EN
from gpu_helpers import W, iroutes, loop_engine, sub_batch  # noqa: F401

pytestmark = pytest.mark.gpu
BAR = 1e-12
COLS = EN.EP_INT + EN.EP_DOUBLE
VEH, ST, RS = ("clear", "who", "hit_tick", "hit_frame", "hit_xy"), ("clear", "who", "hit", "off_tick"), ("val", "trig")
SENTINEL = -77


@pytest.fixture(scope="module")
def eng(pkg, W, iroutes):
    """Any engine: the call needs its context, not its batch."""
    return loop_engine(pkg, iroutes, W.ego_batch(iroutes, 3, 13, rank=2), 13)[0]


@pytest.fixture(scope="module")
def arrays():
    return EC.recorder_arrays()


@pytest.fixture(scope="module")
def series(arrays):
    """The per-tick inputs of every tick count, made once (by the three restatements)."""
    return {n: EC.per_tick(arrays, n) for n in EC.TICK_COUNTS}


def launch(pkg, eng, A, groups, n, egos=None, cap=None):
    """jsim_loop_summarise_episodes on the first n ticks of recorder arrays (egos: these egos only, in this order); groups = (veh,
    st, rs), each a dict of [n][B] arrays or None.  The table is allocated for every row and filled with SENTINEL; cap: the ep_cap
    that is passed (default: the number of rows).  Returns ep_off and one numpy array per column, of every allocated row."""
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    B, m = len(idx), max(n, 1)
    dev = eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pad = lambda a: a if n else np.zeros((1,) + a.shape[1:], dtype=a.dtype)           # (no tick: still a valid pointer)
    rec, flags = up(A["rec"][:m, idx]), up(A["flags"][:m, idx].astype(np.int32))
    xf, xs = up(A["x_first"][idx]), up(A["x_spawn"][idx])
    total = B + int((A["flags"][:n, idx] & 6 != 0).sum())
    held, ptrs = [], []
    for g, keys in zip(groups, (VEH, ST, RS)):
        for k in keys:
            if g is None:
                ptrs.append(None)
            else:
                a = pad(np.asarray(g[k])[:, idx])
                held.append(up(a.astype(np.float64 if a.dtype.kind == "f" else np.int32)))
                ptrs.append(held[-1].data_ptr())
    off = torch.full((B + 1,), SENTINEL, dtype=torch.int64, device=dev)
    ep_i = torch.full((total, len(EN.EP_INT)), SENTINEL, dtype=torch.int32, device=dev)
    ep_d = torch.full((total, len(EN.EP_DOUBLE)), float(SENTINEL), dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    rc = eng.lib.jsim_loop_summarise_episodes(eng._ctx, B, n, p(rec), p(flags), p(xf), p(xs), *ptrs, total if cap is None else cap,
                                              p(off), p(ep_i), p(ep_d), None)
    pkg._cabi.check(rc, eng._ctx, "jsim_loop_summarise_episodes")
    torch.cuda.synchronize()
    I, D = ep_i.cpu().numpy(), ep_d.cpu().numpy()
    out = {"ep_off": off.cpu().numpy()}
    out.update({k: I[:, j].copy() for j, k in enumerate(EN.EP_INT)})
    out.update({k: D[:, j].copy() for j, k in enumerate(EN.EP_DOUBLE)})
    return out


def restate(pkg, A, groups, n, egos=None):
    idx = np.arange(A["rec"].shape[1]) if egos is None else np.asarray(egos)
    cut = [None if g is None else {k: np.asarray(v)[:, idx] for k, v in g.items()} for g in groups]
    return EN.summarise(pkg.history, A["rec"][:n, idx], A["flags"][:n, idx], A["x_first"][idx], A["x_spawn"][idx], *cut)


def bits(out, rows):
    """The rows as raw bytes per column: a comparison bit for bit (NaN payloads and signed zeros included)."""
    return {k: out[k][rows].tobytes() for k in COLS}


@pytest.fixture(scope="module")
def whole(pkg, eng, arrays, series):
    return launch(pkg, eng, arrays, series[EC.N], EC.N)


def test_all_cases_in_one_launch(pkg, eng, arrays, series, whole):
    worst = 0.0
    for n in EC.TICK_COUNTS:
        veh, st, rs = series[n]
        for name, groups in (("all", (veh, st, rs)), ("veh", (veh, None, None)), ("st", (None, st, None)), ("rs", (None, None, rs)),
                             ("none", (None, None, None))):
            out = whole if (n == EC.N and name == "all") else launch(pkg, eng, arrays, groups, n)
            ref = restate(pkg, arrays, groups, n)
            err = EN.compare(out, ref, BAR)
            print(f"{n} ticks, groups {name}: {len(ref['ego'])} rows, sums against math.fsum, maximum error {err:.3g}")
            worst = max(worst, err)
            if name == "all" and n != EC.N:
                # a cut launch: every episode that ended before n is the long launch's row, bit for bit
                done = 0
                for b in range(len(out["ep_off"]) - 1):
                    r0, r1 = int(out["ep_off"][b]), int(out["ep_off"][b + 1]) - 1       # (the last one is the running episode)
                    w0 = int(whole["ep_off"][b])
                    assert bits(out, slice(r0, r1)) == bits(whole, slice(w0, w0 + r1 - r0)), (n, b)
                    assert np.all(out["end"][r0:r1] > 0) and out["end"][r1] == 0
                    done += r1 - r0
                assert done == len(ref["ego"]) - len(out["ep_off"]) + 1
    print(f"jsim_loop_summarise_episodes, 87 egos x {EC.TICK_COUNTS} ticks x 5 choices of groups: sums maximum error {worst:.3g}")
    # the events are where the cases put them
    off = whole["ep_off"]
    assert off[EC.EVERY + 1] - off[EC.EVERY] == EC.N + 1 and off[EC.NEVER + 1] - off[EC.NEVER] == 1
    three = slice(int(off[EC.THREE]), int(off[EC.THREE + 1]))
    assert whole["k0"][three].tolist() == [0, 61, 131, EC.N] and whole["n"][three].tolist() == [61, 70, 69, 0]
    assert np.isnan(whole["length"][three][-1]) and whole["end"][three][-1] == 0
    assert whole["dev_tick"][off[1]] == 30 and whole["dev_max"][off[1]] == 7.0          # ego 1: 7.0 on ticks 30 and 100
    assert np.isnan(whole["dev_max"][off[13]]) and whole["dev_tick"][off[13]] == -1 and np.isnan(whole["dev_mean"][off[13]])
    assert whole["failed"][off[EC.NEVER]] == 4


def test_every_tick_ends_an_episode_at_129_ticks(pkg, eng, arrays, series):
    out = launch(pkg, eng, arrays, series[129], 129, egos=[EC.EVERY])
    assert out["ep_off"].tolist() == [0, 130] and out["n"].tolist() == [1] * 129 + [0] and out["k0"].tolist() == list(range(130))
    assert out["end"][:129].tolist() == [(1, 2, 1)[j % 3] for j in range(129)]                 # GOAL, AGE, both = GOAL


def test_batch_layout_is_immaterial(pkg, eng, arrays, series, whole):
    B = arrays["rec"].shape[1]
    groups = series[EC.N]

    def same_rows(out, egos):
        assert np.array_equal(np.diff(out["ep_off"]), np.diff(whole["ep_off"])[egos]) and out["ep_off"][0] == 0
        for j, b in enumerate(egos):
            mine, theirs = slice(int(out["ep_off"][j]), int(out["ep_off"][j + 1])), slice(int(whole["ep_off"][b]), int(whole["ep_off"][b + 1]))
            assert np.all(out["ego"][mine] == j)
            a, w = bits(out, mine), bits(whole, theirs)
            assert all(a[k] == w[k] for k in COLS if k != "ego"), (b, [k for k in COLS if a[k] != w[k]])

    for egos in ([EC.EVERY], [EC.THREE, EC.NEVER, EC.EVERY], list(range(B))[::-1][:65]):
        same_rows(launch(pkg, eng, arrays, groups, EC.N, egos=egos), egos)
    for b in range(B):
        same_rows(launch(pkg, eng, arrays, groups, EC.N, egos=[b]), [b])


def test_scan_across_a_workgroup_tile(pkg, eng):
    B, n = 1025, 3
    flags = np.zeros((n, B), dtype=np.int32)
    for b in range(B):
        flags[:b % 3, b] = (2, 4)[b % 2]
    k = np.arange(n, dtype=np.float64)[:, None]
    rec = np.zeros((n, B, 7))
    rec[:, :, 0], rec[:, :, 3] = 0.5 * (k + 1) + np.arange(B), 1.0 + k
    A = {"rec": rec, "flags": flags, "x_first": np.stack([np.arange(B, dtype=np.float64)] + [np.zeros(B)] * 3, axis=1), "x_spawn": np.zeros((B, 4))}
    out = launch(pkg, eng, A, (None, None, None), n)
    want = np.concatenate([[0], np.cumsum(1 + np.arange(B) % 3)])
    assert np.array_equal(out["ep_off"], want) and out["ep_off"][1024] == 2047 and out["ep_off"][B] == 2049   # (ego 1024 is the second tile's first)
    EN.compare(out, restate(pkg, A, (None, None, None), n), BAR)


def test_a_table_that_is_too_small(pkg, eng, arrays, series, whole):
    total = int(whole["ep_off"][-1])
    out = launch(pkg, eng, arrays, series[EC.N], EC.N, cap=total - 5)
    assert np.array_equal(out["ep_off"], whole["ep_off"]) and out["ep_off"][-1] == total       # the caller sees the cap was too small
    assert bits(out, slice(0, total - 5)) == bits(whole, slice(0, total - 5))
    for k in COLS:
        assert np.all(out[k][total - 5:] == SENTINEL), k
    none = launch(pkg, eng, arrays, series[EC.N], EC.N, cap=0)
    assert np.array_equal(none["ep_off"], whole["ep_off"]) and all(np.all(none[k] == SENTINEL) for k in COLS)


# ---- loops ----
CYCLIST_DIMS = dict(L=1.0, width=0.45, extra_length=0.64)
T, K = 13, 70


def _loop(pkg, W, iroutes):
    """Three egos, one per start position 1..3, with a cyclist beside the first; max_age 25: two respawns within the 70 ticks."""
    big = W.ego_batch(iroutes, 64, T, rank=2)
    starts = big.path_id // 3
    batch = sub_batch(big, np.array([int(np.flatnonzero(starts == s)[0]) for s in range(3)]))
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    x, y = (float(v) for v in x0[0, :2].cpu())
    cyclist = dict(kind="arterial", x_init=x + 0.5, y_init=y + 6.0, speed=5 / 3.6, initial_speed=5 / 3.6, offset=None, dims=CYCLIST_DIMS)
    sets = [pkg.planner.intersection_obstacles(int(p) // 3 + 1, int(p) % 3 + 1) for p in batch.path_id]
    return pkg.ScenarioLoop(eng, x0, [cyclist], hist_cap=K, max_age=25, frame_window=20, record=K), sets


def _restate_recorder(pkg, r, veh=None, st=None, rs=None):
    """The restatement on the recorder's downloaded arrays and on what its public methods return."""
    n = min(r.ticks_run, r.cap)
    if rs is not None:
        rs = {"val": np.stack([rs[k] for k in ("policymaker", "driver", "cyclist", "distance")], axis=2), "trig": rs["replan"].astype(np.int32)}
    return EN.summarise(pkg.history, r.rec[:n].cpu().numpy(), r.flags[:n].cpu().numpy(), r.x0_first.cpu().numpy(),
                        r.loop.x0_spawn.cpu().numpy(), veh, st, rs)


def same_dict(a, b):
    eq = lambda x, y: (x == y) or (isinstance(x, float) and isinstance(y, float) and x != x and y != y)
    return a.keys() == b.keys() and all(eq(a[k], b[k]) for k in a)


def assert_rows_equal_host_episodes(pkg, s, flags, veh=None, st=None):
    rows = pkg.history.episode_rows(s)
    for key, host in (("conflicts", None if veh is None else pkg.history.conflict_episodes(veh, flags)),
                      ("static", None if st is None else pkg.history.static_episodes(st, flags))):
        if host is None:
            assert all(key not in ep for eps in rows for ep in eps)
            continue
        assert [len(e) for e in rows] == [len(e) for e in host]
        for b, eps in enumerate(host):
            for e, ep in enumerate(eps):
                assert same_dict(rows[b][e][key], ep), (key, b, e, rows[b][e][key], ep)


def test_scenario_loop_summary(pkg, W, iroutes):
    run, sets = _loop(pkg, W, iroutes)
    run.run(K)
    r = run.recorder
    kw = dict(conflicts=True, reasons=True, static=dict(obstacles=sets, set_of=np.arange(3)))
    s = r.summary(**kw)
    veh, st, rs = r.conflicts(), r.static_conflicts(sets, set_of=np.arange(3)), r.reasons()
    flags = r.flags.cpu().numpy()
    assert s["ep_off"].tolist() == np.concatenate([[0], np.cumsum(r.episodes()["count"])]).tolist() and (np.diff(s["ep_off"]) >= 3).all()
    err = EN.compare(s, _restate_recorder(pkg, r, veh, st, rs), BAR)
    print(f"ScenarioLoop, run(70): {len(s['ego'])} episodes, sums against math.fsum, maximum error {err:.3g}")
    assert np.array_equal(s["duration"], s["n"] * r.loop.eng.dt) and s["conflicts"]["frame_window"] == 0 and s["static"]["set_of"].tolist() == [0, 1, 2]
    assert np.isfinite(s["veh_clear"][s["n"] > 0]).all() and np.isfinite(s["st_clear"][s["n"] > 0]).all() and (s["end"] == 2).any()
    assert_rows_equal_host_episodes(pkg, s, flags, veh, st)
    # the reasons' minima are those of history.reason_series
    series = pkg.history.reason_series(rs, flags, r.loop.eng.dt)
    rows = pkg.history.episode_rows(s)
    for b, eps in enumerate(series):
        for e, ep in enumerate(eps):
            for key, col in (("reasons_policymaker_values", "pm_min"), ("reasons_driver_values", "driver_min"), ("reasons_cyclist_values", "cyclist_min")):
                assert rows[b][e][col] == min(ep[key]) if ep[key] else rows[b][e][col] != rows[b][e][col], (b, e, col)
    # each group alone, and none: the other groups' columns hold NaN / -1 / 0
    only = r.summary(conflicts=dict(frame_window=3))
    EN.compare(only, _restate_recorder(pkg, r, r.conflicts(frame_window=3)), BAR)
    assert only["static"] is None and only["reasons"] is None and np.isnan(only["st_clear"]).all() and np.all(only["replan_tick"] == -1)
    EN.compare(r.summary(), _restate_recorder(pkg, r), BAR)

    ticks, _ = _loop(pkg, W, iroutes)
    for _ in range(K):
        ticks.tick()
    t = ticks.recorder.summary(**kw)
    assert np.array_equal(s["ep_off"], t["ep_off"])
    for k in COLS:
        assert s[k].tobytes() == t[k].tobytes(), ("70 x tick()", k)

    for bad in (dict(static=True), dict(static=dict(set_of=0)), dict(conflicts=dict(frame_window=21)), dict(reasons=5),
                dict(reasons=dict(threshold=np.ones(2))), dict(static=dict(obstacles=sets, set_of=7))):
        with pytest.raises(ValueError):
            r.summary(**bad)


def test_interacting_loop_summary(pkg, W, iroutes):
    batch = W.ego_batch(iroutes, 2, T, rank=2)
    eng, x0 = loop_engine(pkg, iroutes, batch, T)
    il = pkg.InteractingLoop(eng, x0, group_sizes=[2], hist_cap=40, max_age=30, frame_window=20, record=40)
    il.run(40)
    r = il.recorder
    sets = [pkg.planner.intersection_obstacles(int(p) // 3 + 1, int(p) % 3 + 1) for p in batch.path_id]
    s = r.summary(conflicts=dict(frame_window=1), static=dict(obstacles=sets, set_of=np.arange(2)))
    veh, st = r.conflicts(frame_window=1), r.static_conflicts(sets, set_of=np.arange(2))
    assert s["conflicts"]["mate_range"].tolist() == [[0, 2], [0, 2]] and s["reasons"] is None
    err = EN.compare(s, _restate_recorder(pkg, r, veh, st), BAR)
    print(f"InteractingLoop, two egos, 40 ticks: {len(s['ego'])} episodes, sums maximum error {err:.3g}")
    assert (np.diff(s["ep_off"]) >= 2).all() and np.isfinite(s["veh_clear"][s["n"] > 0]).all() and np.all(s["veh_who"][s["n"] > 0] == 0)
    assert_rows_equal_host_episodes(pkg, s, r.flags.cpu().numpy(), veh, st)
    with pytest.raises(ValueError):                                   # no vehicle records: no cyclist to evaluate
        r.summary(reasons=True)
