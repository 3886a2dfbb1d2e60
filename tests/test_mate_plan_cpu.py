"""Interacting egos that share their MPC plans (InteractingLoop(mate_prediction="plan"), jsim_loop_set_mate_prediction,
jsim_loop_predict_egos_plan) without a GPU: the numpy restatement of the rule (tests/mate_plan_numpy.py)
against the reference's own Simulation.step (tests/golden/mate_plan.npz), the reference's interactive loop under the rule
(tests/golden/loop_interact_plan_T13.npz) replayed by the restatement and the oracle's glue, the two entry points against the
header, and the refusal of an unknown mode before any device work."""
import os
import types

import numpy as np
import pytest

from conftest import REPO, load_golden
import mate_plan_numpy as MP
from mate_plan_numpy import plan_cases

NEW_EXPORTS = ("jsim_loop_set_mate_prediction", "jsim_loop_predict_egos_plan")


def test_fixture_holds_the_cases_the_kernel_can_go_wrong_at():
    cs = {c["name"]: c for c in plan_cases()}
    shapes = {(c["T"], c["n_steps"]) for c in cs.values()}
    assert {(13, 35), (40, 35), (13, 1), (13, 64), (40, 64), (20, 35)} <= shapes
    assert np.abs(cs["steer_clamp"]["od"]).max() > MP.MAX_STEER and abs(cs["failed_clamp"]["delta_last"]) > MP.MAX_STEER
    assert cs["failed"]["status"] != 0 and cs["failed_clamp"]["status"] != 0 and np.abs(cs["failed"]["oa"]).max() > 0
    assert not cs["zero_plan"]["oa"].any() and not cs["zero_plan"]["od"].any() and cs["zero_plan"]["delta_last"] != 0
    assert np.all(cs["stopping"]["pred"][2:] == cs["stopping"]["pred"][2])          # stands from the third sample on


def test_restated_rule_equals_the_references_simulation_step():
    """Every case: poses and circle centres to 1e-12 (same libm, same operation order: they differ by rounding of the last bit at
    most, |coordinate| <= 100 m)."""
    worst = 0.0
    for c in plan_cases():
        x, y, v, yaw = c["x0"]
        p = MP.predict_plan(x, y, v, yaw, c["oa"], c["od"], c["status"], c["delta_last"], c["n_steps"])
        assert p.shape == c["pred"].shape
        worst = max(worst, float(np.abs(p - c["pred"]).max()), float(np.abs(MP.circle_centres(p) - c["cc"]).max()))
        assert worst <= 1e-12, (c["name"], worst)
    print(f"plan rule restated: max difference to the reference's rollout {worst:.2e}")


def test_rule_inputs():
    """The index meaning, stated on numbers: step i takes element i + 1, the tail holds the last steering at a = 0, a failed
    solve takes (0, delta_last), a plan longer than the prediction is not read to its end."""
    oa, od = np.arange(1.0, 6.0), np.arange(10.0, 15.0)
    a, d = MP.plan_inputs(oa, od, 0, 9.0, 7)
    assert a.tolist() == [2, 3, 4, 5, 0, 0, 0] and d.tolist() == [11, 12, 13, 14, 14, 14, 14]
    a, d = MP.plan_inputs(oa, od, 1, 9.0, 3)
    assert a.tolist() == [0, 0, 0] and d.tolist() == [9, 9, 9]
    a, d = MP.plan_inputs(oa, od, 0, 9.0, 2)
    assert a.tolist() == [2, 3] and d.tolist() == [11, 12]


def test_plan_sharing_reference_loop_replayed_by_the_restatement_and_the_oracle_glue():
    """Every tick, every ego of loop_interact_plan_T13.npz: the restated prediction from the stored plan equals the prediction the
    other ego saw to 1e-12, and the oracle's glue on the restated predictions reproduces the recorded progress index, path length
    and collision flag exactly."""
    g = load_golden("loop_interact_plan_T13.npz")
    ticks, preds = g["ticks"], g["preds"]
    full = [g["smoothed0"], g["smoothed1"]]
    dl = float(g["dl"])
    import loop_oracle as LO
    assert LO.extra_cutoff_margin(dl) == int(g["margin"]) and int(g["frame_window"]) == 20
    n_ticks, n, n_steps = preds.shape[:3]
    delta_last = np.zeros((n_ticks, n))
    delta_last[1:] = ticks[:-1, :, 12]
    delta_last *= 1.0 - ticks[..., 14]                                      # 0 after a respawn
    # element 0 of the held plan is the input applied last tick; a respawned controller holds zeros
    same_run = ticks[1:, :, 14] == 0
    assert np.array_equal(g["plan_oa"][1:, :, 0][same_run], ticks[:-1, :, 13][same_run])
    assert np.array_equal(g["plan_od"][1:, :, 0][same_run], ticks[:-1, :, 12][same_run])
    assert not g["plan_oa"][ticks[..., 14] == 1].any() and not g["plan_oa"][0].any()
    n_cut, n_differ, worst = 0, 0, 0.0
    for i in range(n_ticks):
        rest = []
        for k in range(n):
            x, y, yaw, v = ticks[i, k, :4]
            p = MP.predict_plan(x, y, v, yaw, g["plan_oa"][i, k], g["plan_od"][i, k], 0 if g["plan_ok"][i, k] else 1,
                                delta_last[i, k], n_steps)
            worst = max(worst, float(np.abs(p - preds[i, k]).max()))
            rest.append(p)
        n_differ += any(np.abs(rest[k][:, :2] - MP.predict_constant(ticks[i, k, 0], ticks[i, k, 1], ticks[i, k, 3], ticks[i, k, 2],
                                                                   delta_last[i, k], n_steps)[:, :2]).max() > 0.1 for k in range(n))
        for j in range(n):
            x, y, yaw, v, idx_in, prev_len, idx_out, plen, hit = ticks[i, j, :9]
            st, idx, path_len, col = MP.pre_tick((x, y, yaw, v), int(idx_in), None if prev_len < 0 else int(prev_len), full[j],
                                                 [rest[k] for k in range(n) if k != j], dl, frame_window=20)
            assert st == 0 and idx == int(idx_out) and path_len == int(plen) and (col is not None) == bool(hit), (i, j)
            n_cut += bool(hit)
    assert worst <= 1e-12, worst
    assert n_cut >= 10 and n_cut == int(ticks[:, :, 8].sum())
    assert n_differ >= 10
    assert ticks[:, :, 14].sum() >= 1 and not ticks[:, :, 11].any()
    print(f"plan-sharing loop: {n_ticks} ticks, {n_cut} ego-ticks cut by the other ego, {n_differ} ticks whose prediction differs "
          f"from the constant rule's by more than 0.1 m, max prediction difference {worst:.2e}")


def test_fixtures_stay_within_the_size_of_the_interacting_one():
    limit = os.path.getsize(os.path.join(REPO, "tests", "golden", "loop_interact_T13.npz"))
    for name in ("mate_plan.npz", "loop_interact_plan_T13.npz"):
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", name)) <= limit, name


def test_mate_prediction_exports_declared_in_the_header(pkg):
    hdr = pkg._header.header()
    for name in NEW_EXPORTS:
        assert hdr.functions[name].ret == "int", name
    assert hdr.constants["JSIM_MATE_CONSTANT"] == 0 and hdr.constants["JSIM_MATE_PLAN"] == 1
    assert pkg._cabi.MATE_PREDICTION == {"constant": 0, "plan": 1}
    pkg.build.build()
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_predict_egos_plan.argtypes) == len(hdr.functions["jsim_loop_predict_egos_plan"].params) == 10
    assert len(lib.jsim_loop_set_mate_prediction.argtypes) == 2
    assert lib.jsim_loop_set_mate_prediction(None, 1) == -22                 # null ctx: refused before anything else
    assert lib.jsim_loop_predict_egos_plan(None, 4, None, None, None, None, None, 35, None, None) == -22
    # the signatures that do not change
    assert len(lib.jsim_loop_predict_egos.argtypes) == 7
    assert len(lib.jsim_loop_run_interacting.argtypes) == len(lib.jsim_loop_run_scenario.argtypes)


@pytest.mark.parametrize("mode", ["nonsense", "", None, 1, "Plan"])
def test_interacting_loop_rejects_an_unknown_mate_prediction_before_device_work(pkg, mode):
    """An object with nothing but B stands in for the engine: the mode is checked before the engine is touched."""
    eng = types.SimpleNamespace(B=4)
    with pytest.raises(ValueError, match="mate_prediction"):
        pkg.InteractingLoop(eng, None, group_sizes=[4], mate_prediction=mode)
