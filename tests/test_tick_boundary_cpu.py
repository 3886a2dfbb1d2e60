"""What tests/test_gpu_tick_boundary.py stands on, without a device: its rows are the rows of csrc/reg_variants.h with helper
wavefronts and without the glue -- all of them --, its batches hold the egos their description names, and the fixture recorded from
the parent commit's library has the arrays and shapes the comparison reads."""
import importlib
import os

import numpy as np

import tick_boundary_cases as C
from conftest import PKG_NAME, REPO, load_golden
from gpu_helpers import PLANT_FAIL

CFG = importlib.import_module(PKG_NAME + ".config")


def test_rows_cover_every_glue_free_helper_row_of_the_variant_table():
    header = open(os.path.join(REPO, PKG_NAME, "csrc", "reg_variants.h")).read()
    horizons = C.help_rows(header)
    assert horizons == sorted(r[1] for r in CFG.REG_VARIANTS if r[0] == 1 and r[4] and not r[2]) and len(horizons) == 5
    assert sorted({T for T, _ in C.ROWS}) == horizons
    assert all((T, 64) in C.ROWS for T in horizons) and (20, 256) in C.ROWS and len(C.ROWS) == len(horizons) + 1
    assert C.ROWS[:2] == ((13, 64), (20, 64)) == C.GOLDEN_ROWS         # the glue-free rows of the stock and the headline horizon first
    assert C.K == 12 and C.K % C.MAX_AGE == 0


def test_batch_holds_what_it_names(pkg, routes):
    import active_set_cases as AC
    T, B = 20, 64
    rts, batch, cfgs, age, base = C.case(pkg, routes, T, B)
    again = C.case(pkg, routes, T, B)
    assert all(np.array_equal(getattr(batch, f), getattr(again[1], f)) for f in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od"))
    assert len(rts) == len(routes) + 1 and len(routes) == 12             # (the caller's table is left alone)
    assert age[list(C.RESPAWN)].tolist() == [0] * 4 and np.all(np.delete(age, C.RESPAWN) + C.K < 0)
    for e in C.GOAL:
        r = rts[int(batch.path_id[e])]
        assert np.array_equal(batch.x0[e, :2], r[-1, :2]) and abs(batch.x0[e, 2]) <= 0.3 and batch.path_len[e] == len(r)
    # the hairpin: the three nearest points are one leg's point 10, the other leg's point above it, point 11 -- no two of them neighbours
    hp = rts[int(batch.path_id[C.HAIRPIN])]
    near = np.argsort(np.hypot(hp[:, 0] - batch.x0[C.HAIRPIN, 0], hp[:, 1] - batch.x0[C.HAIRPIN, 1]), kind="stable")[:3]
    assert near.tolist() == [10, 2 * C.HAIRPIN_N - 1 - 10, 11]
    assert abs(near[1] - near[2]) != 2 and abs(near[0] - near[1]) != 1    # neither rule of the nearest-index search holds
    left = batch.path_len - batch.target_ind
    assert [int(left[e]) for e in (C.LEN2, C.LEN3, C.NEAR_END)] == [2, 3, 6]
    # solvable now, not for long: every a_t >= MAX_DECEL > 0, so v_T >= v0 + T dt MAX_DECEL, which is 0.055 below the limit
    e, dt = C.GOOD_THEN_FAIL, pkg.synth.DT
    assert AC.contradiction(float(batch.x0[e, 2]), float(batch.speed[e]), dt, T, cfgs[e]) is None
    assert AC.contradiction(float(batch.x0[e, 2]) + 0.06, float(batch.speed[e]), dt, T, cfgs[e]) is not None
    # the mixed batch's own failures are still there
    ea, eb = AC.planted(B)
    assert 7 in ea and 15 in eb and batch.x0[PLANT_FAIL, 2] > batch.speed[PLANT_FAIL]
    special = set(C.RESPAWN) | set(C.GOAL) | {C.HAIRPIN, C.NO_PATH, C.LEN2, C.LEN3, C.NEAR_END, C.GOOD_THEN_FAIL}
    assert not special & (set(ea) | set(eb) | {PLANT_FAIL}) and len(special) == 12


def test_parent_fixture_has_the_arrays_the_comparison_reads():
    with load_golden("tick_boundary_parent.npz") as z:
        d = {k: z[k] for k in z.files}
    assert d["rows"].tolist() == [list(r) for r in C.GOLDEN_ROWS] and int(d["ticks"]) == C.K
    assert set(d) == {f"T{T}_B{B}_{k}" for T, B in C.GOLDEN_ROWS for k in C.KEYS} | {"rows", "ticks"}
    for T, B in C.GOLDEN_ROWS:
        g = {k: d[f"T{T}_B{B}_{k}"] for k in C.KEYS}
        assert g["hist"].shape == (C.K, B, 2) and g["state"].shape == (B, 4) and g["oa"].shape == g["od"].shape == (B, T)
        assert all(g[k].shape == (B, T + 1) for k in ("ox", "oy", "ov", "oyaw"))
        assert all(g[k].shape == (B,) for k in ("status", "target_ind", "n_iter", "iters", "age"))
        assert g["active_mask"].shape == (B, (8 * T + 31) // 32) and g["n_respawn"].shape == (1,)
        assert all(g[k].dtype == np.float64 for k in ("hist", "state", "oa", "od", "ox", "oy", "ov", "oyaw"))
        # what the parent's library made of the batch: every kind of tick end is in it
        assert g["status"][C.HAIRPIN] == 2 and g["status"][C.NO_PATH] == 3 and g["status"][C.GOOD_THEN_FAIL] == 1
        assert g["status"][C.LEN2] == 0 and int(g["n_respawn"][0]) >= 4 * (C.K // C.MAX_AGE) + 2
        assert g["age"][list(C.RESPAWN)].tolist() == [0] * 4
