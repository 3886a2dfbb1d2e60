"""The premises of tests/test_gpu_active_set.py, on the oracle alone: with the oracle's trace (oracle_py: trace=True, the orc_trace
of mpc_oracle.h) the inputs of tests/active_set_cases.py do take the paths they are built for, at every horizon with a register
kernel and T = 24 (the LDS kernel) and at every batch size the GPU cases use on an MI355X's 256 CUs.  A horizon that misses a floor
gets another seed in active_set_cases.SEEDS -- on this evidence, never on a device's."""
import importlib

import numpy as np
import pytest

import active_set_cases as AC
from conftest import PKG_NAME
from gpu_helpers import PLANT_DECEL, PLANT_FAIL, oracle_batch_per_config, oracle_params, oracle_params_list, sub_batch

CFG = importlib.import_module(PKG_NAME + ".config")
HORIZONS = tuple(sorted({r[1] for r in CFG.REG_VARIANTS} | {24}))
CU = 256
FLOORS = dict(dependent=20, drops_first=1, drops_last=1)     # per batch; beside them: a working set of 2T - 1, a solve longer than 2T


@pytest.fixture(scope="module")
def gpu_cases():
    """tests/test_gpu_active_set.py as a module: its parameter lists are plain data."""
    return importlib.import_module("test_gpu_active_set")


def _base(pkg, T, **kw):
    from dataclasses import replace
    return replace(pkg.MPCConfig.from_json(), T=T, **kw)


def test_trace_changes_nothing_and_adds_up(pkg, oracle, routes):
    """A traced run returns the untraced run's arrays bit for bit; per ego adds - drops is the final working set (>= the active
    rows), every iteration but a failing last one is an add or a drop, and the three wrappers (batch, single step, bare solve)
    report the same record."""
    T, B = 20, 40
    base = _base(pkg, T)
    batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
    _, plain = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=2)
    ps, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=2, trace=True)
    assert set(ref) - set(plain) == {"trace"} and ref["trace"].shape == (B, len(oracle.TRACE_FIELDS)) and ref["trace"].dtype == np.int32
    for k in plain:
        assert np.array_equal(plain[k], ref[k]), k
    t, tr = oracle.TRACE, ref["trace"]
    ok = ref["status"] == 0
    assert np.array_equal(tr[:, t["end"]] == oracle.END_OPTIMAL, ok)
    assert np.array_equal(tr[ok, t["adds"]] + tr[ok, t["drops"]], ref["n_iter"][ok])
    in_loop = tr[:, t["end"]] == oracle.END_INFEASIBLE_IN_LOOP
    assert np.array_equal(tr[in_loop, t["adds"]] + tr[in_loop, t["drops"]] + 1, ref["n_iter"][in_loop])
    n_act = np.unpackbits(np.ascontiguousarray(ref["active_mask"]).view(np.uint8), axis=1).sum(axis=1)
    assert np.all((tr[:, t["adds"]] - tr[:, t["drops"]])[ok] >= n_act[ok]) and np.all(tr[:, t["max_q"]] <= 2 * T)
    assert tr[PLANT_FAIL].tolist() == [0, 0, 0, 0, 0, 0, oracle.END_BEFORE_LOOP, 0] and ref["n_iter"][PLANT_FAIL] == 0
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    for b in (0, int(AC.planted(B)[0][0]), int(AC.planted(B)[1][0]), PLANT_FAIL):
        o, n = off[batch.path_id[b]], batch.path_len[b]
        r = oracle.mpc_step(ps[which[b]], (batch.x0[b, 0], batch.x0[b, 1], batch.x0[b, 3], batch.x0[b, 2]), cx[o:o + n], cy[o:o + n],
                            cyaw[o:o + n], int(batch.target_ind[b]), batch.speed[b], oa=batch.oa[b], od=batch.od[b], trace=True)
        assert r["trace"].tolist() == tr[b].tolist() and r["status"] == ref["status"][b], b
    # the bare solve: one violated row, one add
    H, g = np.eye(2), np.zeros(2)
    st, u, lam, it, rec = oracle.solve_qp(H, g, np.array([[1.0, 0.0]]), np.array([-1.0]), trace=True)
    assert (st, it) == (0, 1) and np.allclose(u, [-1.0, 0.0]) and rec.tolist() == [1, 0, 0, 0, 0, 1, oracle.END_OPTIMAL, 0]
    assert oracle.solve_qp(H, g, np.array([[1.0, 0.0]]), np.array([-1.0]))[3] == 1
    # .. and rows that contradict each other (x0 <= -1, x0 >= 0): the in-loop exit after one add
    st, u, lam, it, rec = oracle.solve_qp(H, g, np.array([[1.0, 0.0], [-1.0, 0.0]]), np.array([-1.0, 0.0]), trace=True)
    assert (st, it) == (1, 2) and rec.tolist() == [1, 0, 0, 0, 1, 1, oracle.END_INFEASIBLE_IN_LOOP, 0]


def test_contradiction_is_plain_arithmetic(pkg):
    """The reference for "this ego must fail": the planted rows contradict themselves, their neighbours' rows do not."""
    dt, speed = pkg.synth.DT, pkg.synth.SPEED
    for T in HORIZONS:
        base = _base(pkg, T)
        a, b, tight = AC.a_config(base, T), AC.b_config(base, T), AC.tight_config(base, T)
        assert AC.contradiction(speed - AC.A_MARGIN, speed, dt, T, a) == "v_1 >= v0 + dt * 1 * MAX_DECEL > speed"
        assert a.MAX_DECEL == 0.5 > (speed - (speed - AC.A_MARGIN)) / dt                    # a_0 >= 0.5 against a_0 <= 0.05
        why = AC.contradiction(AC.B_V0, speed, dt, T, b)
        assert why is not None and why.endswith("MAX_ACCEL < MIN_SPEED") and AC.B_V0 + dt * T * b.MAX_ACCEL < base.MIN_SPEED
        assert AC.contradiction(AC.B_V0, speed, dt, T, base) is None and AC.contradiction(speed - AC.A_MARGIN, speed, dt, T, base) is None
        assert all(AC.contradiction(v, speed, dt, T, tight) is None for v in (0.0, 4.0, speed))
        assert AC.contradiction(AC.V0_ABOVE, speed, dt, T, base) == "v0 > speed" and AC.contradiction(-5.5, speed, dt, T, base) == "v0 < MIN_SPEED"


def test_builders_are_seeded_and_plant_where_they_say(pkg, routes):
    T, B = 20, 64
    base = _base(pkg, T)
    one, two = AC.mixed_case(pkg.synth, routes, base, B, T), AC.mixed_case(pkg.synth, routes, base, B, T)
    assert all(np.array_equal(getattr(one[0], f), getattr(two[0], f)) for f in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od"))
    assert one[1] == two[1] and np.array_equal(one[2], two[2])
    batch, cfgs, which = one
    ea, eb = AC.planted(B)
    assert ea.tolist() == [7, 23, 39, 55] and eb.tolist() == [15, 31, 47, 63] and PLANT_FAIL == 12
    assert np.all(which[ea] == AC.ROW_A) and np.all(which[eb] == AC.ROW_B) and which[PLANT_FAIL] == AC.ROW_V0
    assert (which == AC.ROW_TIGHT).sum() == B - 9
    assert all(which[n] == AC.ROW_TIGHT for e in np.concatenate([ea, eb]) for n in (e - 1, e + 1) if n < B)     # solvable neighbours
    assert cfgs[7].MAX_DECEL == 0.5 and (cfgs[15].MAX_ACCEL, cfgs[15].MAX_DECEL) == (-3.0, -10.0) and cfgs[PLANT_FAIL].MAX_DECEL == PLANT_DECEL
    assert (cfgs[0].MAX_ACCEL, cfgs[0].MAX_DECEL, cfgs[0].MAX_DSTEER) == (0.05, -0.05, 0.4) and AC.b_config(base, 25).MAX_ACCEL == -1.5
    assert not batch.oa.any() and not batch.od.any() and batch.x0[PLANT_FAIL, 2] == 9.5
    plain = pkg.synth.make_ego_batch(routes, B, T, seed=AC.seed_of(T), truncate=False, near_end_frac=0.0)
    assert np.allclose(np.hypot(*(batch.x0[:, :2] - plain.x0[:, :2]).T), AC.LATERAL) and np.allclose(batch.x0[:, 3] - plain.x0[:, 3], AC.DYAW)
    b3, c3, w3 = AC.mixed_case(pkg.synth, routes, base, B, T, plant=False)
    assert np.array_equal(b3.x0, batch.x0) and np.array_equal(w3, which) and all(c3[e] == base for e in np.concatenate([ea, eb]))
    assert all(c3[e] == cfgs[e] for e in range(B) if which[e] in (AC.ROW_TIGHT, AC.ROW_V0))


@pytest.mark.parametrize("T", HORIZONS)
def test_families_alone(pkg, oracle, routes, T):
    """Each family under one configuration, 96 egos: every A and every B ego ends by the in-loop exit after adds and drops, every
    off-path tight ego is solvable, and the tight family alone holds the floors."""
    B = 96
    base = _base(pkg, T)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    t = oracle.TRACE
    for family in ("tight", "A", "B"):
        batch, cfg = AC.family_case(pkg.synth, routes, base, B, T, family)
        ref = oracle.mpc_step_batch(oracle_params(oracle, cfg), batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off,
                                    batch.target_ind, batch.oa, batch.od, n_threads=16, trace=True)
        tot = AC.trace_totals(oracle, ref["trace"])
        print(f"T={T} {family}: {tot}, longest solve {ref['n_iter'].max()}")
        if family == "tight":
            assert np.all(ref["status"] == 0) and tot["max_q"] == 2 * T - 1 and ref["n_iter"].max() > 2 * T
            assert all(tot[k] >= v for k, v in FLOORS.items()), tot
        else:
            assert np.all(ref["status"] == 1) and tot["in_loop"] == B and AC.contradictory(batch, [cfg] * B, pkg.synth.DT).all()
            assert ref["trace"][:, t["adds"]].min() >= 1 and tot["drops"] >= B


def _mixed_premises(pkg, oracle, routes, T, B, base, what):
    batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
    _, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=16, trace=True)
    t, tr = oracle.TRACE, ref["trace"]
    tot = AC.trace_totals(oracle, tr)
    pl = np.concatenate(AC.planted(B))
    print(f"{what} T={T} B={B}: {tot}, longest solve {ref['n_iter'].max()}, planted iterations {ref['n_iter'][pl].min()}..{ref['n_iter'][pl].max()}")
    assert np.all(tr[pl, t["end"]] == oracle.END_INFEASIBLE_IN_LOOP) and tr[pl, t["adds"]].min() >= 1 and tr[pl, t["drops"]].min() >= 1, (T, B)
    assert tr[PLANT_FAIL, t["end"]] == oracle.END_BEFORE_LOOP and tot["max_iters"] == 0 and tot["before_loop"] == 1, (T, B)
    assert np.array_equal(ref["status"] == 1, AC.contradictory(batch, cfgs, pkg.synth.DT)) and set(ref["status"]) == {0, 1}, (T, B)
    assert (ref["status"] == 1).sum() == len(pl) + 1 and np.all(ref["status"][which == AC.ROW_TIGHT] == 0), (T, B)
    assert all(tot[k] >= v for k, v in FLOORS.items()), (T, B, tot)
    assert tot["max_q"] == 2 * T - 1 and ref["n_iter"][ref["status"] == 0].max() > 2 * T, (T, B, tot)
    return ref


@pytest.mark.parametrize("T", HORIZONS)
def test_mixed_batch_takes_the_paths(pkg, oracle, routes, gpu_cases, T):
    """For every (T, B) of the one-step GPU cases at 256 CUs: every planted A / B ego ends by the in-loop exit with at least one add
    and one drop before it; the egos with status 1 are exactly the arithmetic-contradictory ones; the off-path tight egos all
    solve; and per batch at least 20 dependent rows, a drop at position 0, a drop at the last position, a working set of 2T - 1
    (and none of 2T: these families end there, the full-set family of tests/test_full_set_cpu.py goes on) and a solve longer than 2T.  With MAX_ITER = 3 the planted egos' traces are
    those of one pass: they fail on the first."""
    one, _ = gpu_cases.oracle_shapes(CU)
    assert {s[0] for s in one} == set(HORIZONS)
    sizes = [B for t_, B in one if t_ == T]
    assert sizes
    for B in sorted(set(sizes)):
        ref = _mixed_premises(pkg, oracle, routes, T, B, _base(pkg, T), "step")
        if (T, B) in gpu_cases.MAX_ITER_SHAPES:
            ref3 = _mixed_premises(pkg, oracle, routes, T, B, _base(pkg, T, MAX_ITER=3), "MAX_ITER=3")
            pl = np.concatenate(AC.planted(B))
            assert np.array_equal(ref3["trace"][pl], ref["trace"][pl]) and np.array_equal(ref3["n_iter"][pl], ref["n_iter"][pl])
            ok = ref["status"] == 0
            assert ref3["n_iter"][ok].sum() > ref["n_iter"][ok].sum() and np.abs(ref3["oa"] - ref["oa"])[ok].max() > 1e-3


@pytest.mark.parametrize("T", HORIZONS)
def test_planted_egos_fail_on_every_tick(pkg, oracle, routes, gpu_cases, T):
    """For every (T, B, K) of the closed loops against the oracle: in K ticks the planted egos fail on every tick, by the in-loop
    exit after at least one completed iteration, brake with their row's MAX_DECEL and keep their steering until the age limit
    respawns them; n_fail of closed_loop_per_config is ticks x planted egos plus the failures of the v0-above-limit ego run alone."""
    _, loops = gpu_cases.oracle_shapes(CU)
    assert {s[0] for s in loops} == set(HORIZONS)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    t = oracle.TRACE
    for B, K in sorted({(B, K) for t_, B, K in loops if t_ == T}):
        assert K == (6 if T <= 25 else 4)
        base = _base(pkg, T)
        batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
        ps = oracle_params_list(oracle, cfgs, which)
        pl = np.concatenate(AC.planted(B))
        state = oracle.loop_state_from_batch(batch, T)
        state["di_ai"][:, 0] = gpu_cases.LOOP_DI
        n_fail, hist = 0, []
        for k in range(K):
            now = oracle.mpc_step_batch_per_config(ps, which, state["x0"], state["path_id"], state["path_len"], state["speed"], cx, cy, cyaw,
                                                   off, state["target_ind"], state["oa"], state["od"], n_threads=16, trace=True)
            assert np.all(now["trace"][pl, t["end"]] == oracle.END_INFEASIBLE_IN_LOOP) and np.all(now["n_iter"][pl] >= 2), (T, B, k)
            assert np.all(now["status"][which == AC.ROW_TIGHT] == 0), (T, B, k)
            r = oracle.closed_loop_per_config(ps, which, state, cx, cy, cyaw, off, 1, max_age=gpu_cases.LOOP_MAX_AGE, n_threads=16)
            assert r["n_fail"] == (now["status"] != 0).sum(), (T, B, k)
            n_fail += r["n_fail"]
            hist.append(r["hist"][0])
        hist = np.array(hist)
        for e in pl:
            assert np.all(hist[:, e, 1] == cfgs[e].MAX_DECEL), (T, B, e)
            assert np.array_equal(hist[:, e, 0], np.where(np.arange(K) < gpu_cases.LOOP_MAX_AGE, gpu_cases.LOOP_DI, 0.0)), (T, B, e)
        alone = sub_batch(batch, np.array([PLANT_FAIL]))
        s1 = oracle.loop_state_from_batch(alone, T)
        s1["di_ai"][:, 0] = gpu_cases.LOOP_DI
        r1 = oracle.closed_loop(ps[AC.ROW_V0], s1, cx, cy, cyaw, off, K, max_age=gpu_cases.LOOP_MAX_AGE)
        print(f"loop T={T} B={B} K={K}: n_fail {n_fail} = {K} x {len(pl)} + {r1['n_fail']}")
        assert n_fail == K * len(pl) + r1["n_fail"] and r1["n_fail"] >= 1 and hist[0, PLANT_FAIL, 1] == PLANT_DECEL, (T, B)


def test_the_way_to_the_exit_is_decided_by_rounding(pkg, oracle, routes):
    """Why the GPU test holds the iteration counts of the planted egos to no bar of their own.  With every yaw changed in its last
    bits (a few ulps: H, and so J and r = R^-1 d1, change by rounding alone) the oracle gives every ego the same status and every
    solvable ego the same iteration count, but most planted egos another one: on the way to "no step length" the components of r
    that are zero in exact arithmetic carry noise whose sign decides whether a position is dropped first."""
    for T, B in ((24, 48), (20, 257), (40, 97)):
        base = _base(pkg, T)
        batch, cfgs, which = AC.mixed_case(pkg.synth, routes, base, B, T)
        _, a = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, trace=True)
        batch.x0[:, 3] *= 1 + 1e-15
        _, b = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, trace=True)
        pl = np.concatenate(AC.planted(B))
        ok = a["status"] == 0
        same = a["n_iter"] == b["n_iter"]
        print(f"T={T} B={B}: same iteration count after the change: solvable egos {same[ok].mean():.3f}, planted egos {same[pl].mean():.3f}")
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["active_mask"], b["active_mask"])
        assert same[ok].mean() >= 0.9 and np.all(b["trace"][pl, oracle.TRACE["end"]] == oracle.END_INFEASIBLE_IN_LOOP)
