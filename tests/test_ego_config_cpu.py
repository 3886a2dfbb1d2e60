"""The CPU side of the per-ego table tests (tests/test_gpu_ego_config.py): the oracle's per-configuration wrappers, the proof --
from the oracle alone -- that the inputs of the GPU cases leave few egos out of the control comparison and do exercise the
limits, the header's row layout against the row set_ego_configs builds, and that every register kernel has a per-ego case."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, REPO
from gpu_helpers import (PLANT_EGOS, PLANT_FAIL, PLANT_LOOSE, PLANT_TIGHT, PLANT_TWINS, ego_config_case, ego_config_pool,
                         ego_config_table, n_active, oracle_batch_per_config, oracle_params, oracle_params_list, variant_id)

CFG = importlib.import_module(PKG_NAME + ".config")


@pytest.fixture(scope="module")
def gpu_cases():
    """tests/test_gpu_ego_config.py as a module: its parameter lists are plain data."""
    return importlib.import_module("test_gpu_ego_config")


def _base(pkg, kind, T):
    from dataclasses import replace
    return replace(pkg.mpc_jerk.config if kind == "jerk" else pkg.MPCConfig.from_json(), T=T)


def test_per_config_batch_equals_the_plain_wrappers(pkg, oracle, routes):
    """mpc_step_batch_per_config with one configuration is mpc_step_batch, bit for bit; with the pool and the planted rows it is
    mpc_step called ego by ego with that ego's parameters."""
    T, B = 20, 40
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    args = (batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off, batch.target_ind, batch.oa, batch.od)
    p = oracle_params(oracle, cfgs[0])
    one = oracle.mpc_step_batch_per_config([None, None, p], np.full(B, 2), *args, n_threads=2)
    plain = oracle.mpc_step_batch(p, *args)
    assert one.keys() == plain.keys()
    for k in plain:
        assert one[k].dtype == plain[k].dtype and np.array_equal(one[k], plain[k]), k
    assert len(set(which)) > 12 and sorted(which[list(PLANT_EGOS)]) == [12, 13, 14, 15, 16]
    ps, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=2)
    for b in range(B):
        o, n = off[batch.path_id[b]], batch.path_len[b]
        r = oracle.mpc_step(oracle_params(oracle, cfgs[b]), (batch.x0[b, 0], batch.x0[b, 1], batch.x0[b, 3], batch.x0[b, 2]), cx[o:o + n],
                            cy[o:o + n], cyaw[o:o + n], int(batch.target_ind[b]), batch.speed[b], oa=batch.oa[b], od=batch.od[b])
        assert ref["status"][b] == r["status"] and ref["target_ind"][b] == r["target_ind"] and ref["n_iter"][b] == r["n_iter"], b
        assert np.array_equal(ref["xref"][b], r["xref"]) and np.array_equal(ref["active_mask"][b], r["active_mask"]), b
        if r["status"] == 0:
            for k in ("oa", "od", "ox", "oy", "ov", "oyaw"):
                assert np.array_equal(ref[k][b], r[k]), (k, b)
    assert np.array_equal(batch.x0[PLANT_TWINS[0]], batch.x0[PLANT_TWINS[1]]) and ref["status"][PLANT_FAIL] == 1
    with pytest.raises(ValueError):
        oracle.mpc_step_batch_per_config(ps, which[:-1], *args)
    with pytest.raises(ValueError):
        oracle.mpc_step_batch_per_config(ps[:-1] + [oracle.make_params(T=T + 1)], which, *args)


def test_closed_loop_per_config_equals_closed_loop(pkg, oracle, routes):
    """closed_loop_per_config with one configuration is closed_loop; with several, each group's egos are that group run alone."""
    T, B, K = 13, 24, 6
    batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, truncate=False)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    p = oracle_params(oracle, cfgs[0])
    s1, s2 = oracle.loop_state_from_batch(batch, T), oracle.loop_state_from_batch(batch, T)
    r1 = oracle.closed_loop(p, s1, cx, cy, cyaw, off, K, max_age=4)
    r2 = oracle.closed_loop_per_config([p], np.zeros(B, dtype=int), s2, cx, cy, cyaw, off, K, max_age=4)
    assert np.array_equal(r1["hist"], r2["hist"]) and all(r1[k] == r2[k] for k in ("n_respawn", "n_iter_sum", "n_fail"))
    assert all(np.array_equal(s1[k], s2[k]) for k in s1) and r1["n_respawn"] >= B
    ps = oracle_params_list(oracle, cfgs, which)
    s3 = oracle.loop_state_from_batch(batch, T)
    r3 = oracle.closed_loop_per_config(ps, which, s3, cx, cy, cyaw, off, K, max_age=4)
    k = which[PLANT_FAIL]
    sel = np.flatnonzero(which == k)
    s4 = {name: np.ascontiguousarray(a[sel]) for name, a in oracle.loop_state_from_batch(batch, T).items()}
    r4 = oracle.closed_loop(ps[k], s4, cx, cy, cyaw, off, K, max_age=4)
    assert np.array_equal(r3["hist"][:, sel], r4["hist"]) and np.array_equal(s3["x0"][sel], s4["x0"])
    assert r3["hist"][0, PLANT_FAIL, 1] == -3.7 and r3["n_fail"] >= 1


def test_gpu_cases_exclude_few_egos_and_exercise_the_limits(pkg, oracle, routes, gpu_cases):
    """Cases 1 and 6 of tests/test_gpu_ego_config.py compare controls only where the oracle's status is 0.  From the oracle alone,
    for every (T, B) they use at an MI355X's 256 CUs, with their seeds: at most 1/16 of the egos are left out (the planted failure
    included) -- per tick in the closed loops of case 6 -- and at least half the egos end with a non-empty active set, so a change
    of the draw cannot quietly turn the comparisons into unconstrained solves; the planted rows do what they are planted for."""
    shapes = gpu_cases.oracle_compared_shapes(256)
    assert len(shapes) >= 18 and {s[0] for s in shapes} == {13, 15, 16, 20, 24, 25, 30, 32, 40}
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    for T, B, kind, batch_kw, ticks in shapes:
        batch, cfgs, which = ego_config_case(pkg.synth, routes, T, B, base=_base(pkg, kind, T), **dict(batch_kw))
        ps, ref = oracle_batch_per_config(oracle, pkg.synth, routes, batch, cfgs, which, n_threads=8)
        ok = ref["status"] == 0
        na = n_active(ref["active_mask"])
        print(f"T={T} B={B} {kind} ticks={ticks}: status != 0 for {(~ok).sum()} (cap {B // gpu_cases.EXCLUDED_MAX}), non-empty active "
              f"sets {(na[ok] > 0).sum()}, rows active on the tight / loose planted egos {na[PLANT_TIGHT]} / {na[PLANT_LOOSE]}")
        assert (~ok).sum() <= B // gpu_cases.EXCLUDED_MAX, (T, B, kind)
        assert (na[ok] > 0).sum() >= B / 2, (T, B, kind)
        a, b = PLANT_TWINS
        assert not ok[PLANT_FAIL] and ok[a] and ok[b] and ok[PLANT_TIGHT] and ok[PLANT_LOOSE], (T, B, kind)
        assert max(np.abs(ref["oa"][a] - ref["oa"][b]).max(), np.abs(ref["od"][a] - ref["od"][b]).max()) > 1e-2, (T, B, kind)
        assert na[PLANT_TIGHT] > na[PLANT_LOOSE], (T, B, kind)
        if ticks:
            state = oracle.loop_state_from_batch(batch, T)
            for k in range(ticks):
                r = oracle.closed_loop_per_config(ps, which, state, cx, cy, cyaw, off, 1, max_age=70, n_threads=8, record=False)
                assert r["n_fail"] <= B // gpu_cases.EXCLUDED_MAX, (T, B, k)


def test_table_row_layout_matches_the_header(pkg):
    """The field order of a table row as include/jsim_mpc.h documents it (the comment above JSIM_EGO_CFG_DOUBLES) against the row
    BatchedMPC.set_ego_configs builds from an MPCConfig.  BatchedMPC needs a device, so the method runs on a stand-in that has the
    attributes it touches and a library whose jsim_mpc_set_ego_config accepts anything."""
    from dataclasses import replace
    text = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    m = re.search(r"\{([^{}]*)\}\.\s*\n[^\n]*\n#define JSIM_EGO_CFG_DOUBLES (\d+)", text)
    assert m, "the row's field list above JSIM_EGO_CFG_DOUBLES"
    body = re.sub(r"\([^()]*\)", "", m.group(1).replace("\n *", " "))            # drop the parenthesised remarks
    names = []
    for item in (s.strip() for s in body.split(",")):
        rng = re.fullmatch(r"(\w+)\[(\d+)\.\.(\d+)\]", item)
        if rng:
            names += [f"{rng.group(1)}[{i}]" for i in range(int(rng.group(2)), int(rng.group(3)) + 1)]
        else:
            names.append(item)
    assert len(names) == int(m.group(2)) == pkg.BatchedMPC.EGO_CFG_DOUBLES == 16
    assert names == ["w_perp", "w_para", "R[0]", "R[1]", "Rd[0]", "Rd[1]", "Q_v_yaw[0]", "Q_v_yaw[1]", "Qf[0]", "Qf[1]", "Qf[2]", "Qf[3]",
                     "MAX_DSTEER [rad/s]", "MAX_ACCEL", "MAX_DECEL", "reserved"]
    cfg = replace(pkg.MPCConfig(), T=7, w_perp=101.0, w_para=102.0, R=[103.0, 104.0], Rd=[105.0, 106.0], Q_v_yaw=[107.0, 108.0],
                  Qf=[109.0, 110.0, 111.0, 112.0], MAX_DSTEER=113.0, MAX_ACCEL=114.0, MAX_DECEL=-115.0)

    def value(name):
        if name == "reserved":
            return 0.0
        if name == "MAX_DSTEER [rad/s]":
            return cfg.max_dsteer_rad                    # the JSON's degrees per second, in radians
        idx = re.fullmatch(r"(\w+)\[(\d+)\]", name)
        return float(getattr(cfg, idx.group(1))[int(idx.group(2))]) if idx else float(getattr(cfg, name))

    class Lib:
        calls = []
        def jsim_mpc_set_ego_config(self, ctx, ptr):
            self.calls.append(ptr)
            return 0

    eng = object.__new__(pkg.BatchedMPC)
    eng.lib, eng._ctx, eng.B, eng.T, eng.device = Lib(), None, 3, 7, torch.device("cpu")
    eng.set_ego_configs([cfg] * 3)
    assert eng._pe.shape == (3, 16) and eng._pe.dtype == torch.float64 and len(Lib.calls) == 1
    assert eng._pe[1].tolist() == [value(n) for n in names]


def test_every_register_kernel_has_a_per_ego_case(gpu_cases):
    """Every row of config.REG_VARIANTS is in the parameter ids of the per-ego cases: the rows without the glue in the single step
    against the oracle (every boundary size), in the table-of-context-rows case, the row-b-means-ego-b case and the fused closed
    loop; the rows with the glue in the fused scenario loop.  A row added to the table without a per-ego case fails here."""
    ids = lambda params: {p.id for p in params}
    for row in CFG.REG_VARIANTS:
        name = variant_id(row)
        if row[2]:
            assert name in ids(gpu_cases.SCENARIO_CASES) and name in ids(gpu_cases.SAME_CASES), name
        else:
            for cases in (gpu_cases.STEP_CASES, gpu_cases.SAME_CASES, gpu_cases.ROW_CASES, gpu_cases.CLOSED_LOOP_CASES):
                assert name in ids(cases), name
    assert {"lds-T24", "jerk-T13"} <= ids(gpu_cases.STEP_CASES)
    assert len(gpu_cases.STEP_CASES) == sum(len(gpu_cases.variant_batches(r, 256)) for r in gpu_cases.NON_PRE_ROWS) + 2
    for mark in ("step_against_oracle_with_table", "table_of_context_rows_changes_nothing", "row_b_means_ego_b",
                 "fused_ticks_equal_single_ticks_with_table", "fused_scenario_loop_equals_tick_by_tick_with_table"):
        assert callable(getattr(gpu_cases, "test_" + mark))


def test_pool_and_table_draws():
    """The pool holds distinct configurations in the ranges of test_per_ego_weights_one_batch; the table picks from it with a seed
    and plants its rows at fixed neighbouring indices."""
    pool = ego_config_pool(20)
    assert len(pool) == 12 and len({(c.w_perp, c.MAX_ACCEL) for c in pool}) == 12 and all(c.T == 20 for c in pool)
    assert all(5 <= c.w_perp <= 40 and 0.5 <= c.MAX_ACCEL <= 3 and -10 <= c.MAX_DECEL <= -3 and 10 <= c.MAX_DSTEER <= 60 for c in pool)
    cfgs, which = ego_config_table(pool, 64)
    cfgs2, which2 = ego_config_table(pool, 64)
    assert np.array_equal(which, which2) and cfgs == cfgs2 and len(set(which[which < 12])) >= 10
    assert PLANT_EGOS == (10, 11, 12, 13, 14) and all(which[e] >= 12 for e in PLANT_EGOS)
    assert all(cfgs[b] is pool[which[b]] for b in range(64) if b not in PLANT_EGOS)
    a, b = PLANT_TWINS
    assert (cfgs[a].MAX_ACCEL, cfgs[a].w_perp, cfgs[b].MAX_ACCEL, cfgs[b].w_perp) == (0.5, 5.0, 3.0, 40.0) and cfgs[a].R == cfgs[b].R
    assert cfgs[PLANT_FAIL].MAX_DECEL == -3.7 and (cfgs[PLANT_TIGHT].MAX_ACCEL, cfgs[PLANT_TIGHT].MAX_DSTEER) == (0.05, 0.4)
