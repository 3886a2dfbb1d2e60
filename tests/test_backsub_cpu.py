"""The premises of tests/test_gpu_backsub.py, on the oracle alone: with the oracle's per-solve trace (adds, drops, largest working
set) the batches of tests/backsub_cases.py take every path of the one-wave kernels' back substitution at every horizon used -- a
working set that stays within 8 rows, one that ends inside the first 16-lane row, one that passes 16 rows and stays above, one that
falls back from above 16 rows to 16 or fewer, and a drop while no more than 16 rows are held.  A horizon that misses one gets another
seed in backsub_cases.SEEDS -- on this evidence, never on a device's."""
import importlib

import numpy as np
import pytest

import backsub_cases as C
from conftest import PKG_NAME

CFG = importlib.import_module(PKG_NAME + ".config")


def test_the_cases_cover_every_one_wave_row_of_their_horizons():
    """13 and 20 have every one-wave form (helpers, two waves per SIMD, the glue inside), 30 the virtual speed rows; the GPU test
    derives its rows from the variant table, so a new row at these horizons is run without a list to edit."""
    rows = [r for r in CFG.REG_VARIANTS if r[0] == 1 and r[1] in C.HORIZONS]
    assert {r[1] for r in rows} == set(C.HORIZONS) and C.B <= 64 and max(C.TICKS.values()) <= 8
    assert any(r[4] for r in rows) and any(r[3] == 2 for r in rows) and any(r[2] for r in rows)
    assert any(r[1] > 20 for r in rows)                                        # T > 20: virtual speed rows (csrc/mpc_step_reg.inc)


def test_builder_is_seeded_and_mixes_the_families(pkg, routes):
    import active_set_cases as AC
    T = 20
    one, two = C.case(pkg, routes, T), C.case(pkg, routes, T)
    assert all(np.array_equal(getattr(one[0], f), getattr(two[0], f)) for f in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od"))
    assert one[1] == two[1] and np.array_equal(one[2], two[2])
    batch, cfgs, which, base = one
    assert [(which == k).sum() for k in (C.ROW_STOCK, C.ROW_A, C.ROW_TIGHT)] == [16, 16, 16]
    assert which[:12].tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert cfgs[0] == base and cfgs[4] == AC.a_config(base, T) and cfgs[8] == AC.tight_config(base, T)
    a = which == C.ROW_A
    assert np.array_equal(batch.x0[a, 2], batch.speed[a] - AC.A_MARGIN) and not batch.oa.any() and not batch.od.any()
    plain = pkg.synth.make_ego_batch(routes, C.B, T, seed=C.SEEDS[T], truncate=False, near_end_frac=0.0)
    moved = np.hypot(*(batch.x0[:, :2] - plain.x0[:, :2]).T)
    want = np.where(which == C.ROW_TIGHT, 1.0, np.array(C.SCALES)[np.arange(C.B) % 4]) * AC.LATERAL
    assert np.allclose(moved, want) and np.allclose(batch.x0[:, 3] - plain.x0[:, 3], want / AC.LATERAL * AC.DYAW)
    assert AC.contradictory(batch, cfgs, pkg.synth.DT).tolist() == a.tolist()


@pytest.mark.parametrize("T", C.HORIZONS)
def test_every_path_of_the_back_substitution_is_taken(oracle, T):
    ticks = C.oracle_ticks(T)
    assert len(ticks) == C.TICKS[T]
    found = C.paths_taken(oracle, ticks)
    print(f"T={T} seed {C.SEEDS[T]}: " + ", ".join(f"{p} {len(v)}" for p, v in found.items()) +
          f"; first fall_back (tick, ego) {found['fall_back'][:1]}, first low_drop {found['low_drop'][:1]}")
    assert all(found[p] for p in C.PATHS), {p: len(v) for p, v in found.items()}
    t = oracle.TRACE
    # what the selections mean, on the first solve of each: the trace's own numbers
    k, b = found["small"][0]
    assert 1 <= ticks[k]["step"]["trace"][b, t["max_q"]] <= 8
    k, b = found["fall_back"][0]
    tr = ticks[k]["step"]["trace"][b]
    assert tr[t["max_q"]] >= 17 and tr[t["adds"]] - tr[t["drops"]] <= 16 and tr[t["drops"]] >= 1
    k, b = found["above"][0]
    tr = ticks[k]["step"]["trace"][b]
    assert tr[t["adds"]] - tr[t["drops"]] >= 17 and ticks[k]["step"]["status"][b] == 0
    k, b = found["one_row"][0]
    tr = ticks[k]["step"]["trace"][b]
    assert 9 <= tr[t["adds"]] - tr[t["drops"]] <= tr[t["max_q"]] <= 16
    k, b = found["low_drop"][0]
    tr = ticks[k]["step"]["trace"][b]
    assert tr[t["drops"]] >= 1 and tr[t["max_q"]] <= 16
    # solvable and failing egos side by side on every tick: the stock and tight rows solve, the A rows fail inside the loop
    _, _, which, _ = C.case(importlib.import_module(PKG_NAME), C.smoothed_routes(importlib.import_module(PKG_NAME)), T)
    st0 = ticks[0]["step"]["status"]
    assert np.all(st0[which != C.ROW_A] == 0) and np.all(st0[which == C.ROW_A] == 1)
    assert np.all(ticks[0]["step"]["trace"][which == C.ROW_A, t["end"]] == oracle.END_INFEASIBLE_IN_LOOP)
