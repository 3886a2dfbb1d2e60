"""Stakeholder reasons: score the planner's candidate trajectories and pick one (jsim_score_trajectories).

The function surface of main/scenarios/overtaking_cyclist_bidirectional_road.py that perform_replan (:290-407) calls after
run_all: create_following_trajectory (:410-445), evaluate_trajectories_for_reasons (:1233-1428), evaluate_trajectories_with_weights
(:1641-1864), generate_stakeholder_weight_table (:1431-1604) with balance_function (:1191-1231) and compute_predicted_trajectory
(:244-266), with the same arguments and return shapes.  Every evaluation is ONE launch of the HIP kernel, the whole weight table
included; score_situations is the batched entry for many situations at once.  There is no CPU path: without the HIP library or a
HIP device the calls raise.

The per-tick half of the same study -- evaluate_reasons (:2007-2027) and the replan trigger reasons_evaluation (:1907-1940) -- is
evaluated from a loop's recorder (closed_loop.Recorder.reasons, jsim_loop_eval_reasons); tick_inputs checks
its arguments and situation_at turns one of its ticks into a situation for score_situations."""
from __future__ import annotations

import csv
import ctypes as C

import numpy as np

from . import _cabi
from .history import AGE, GOAL

MAX_CAND, MAX_RES = 8, 320
# a situation's parameter row, in the order of the header's JSIM_REASON_* enum; the reference's values (lib/parameters.py,
# lib/mpc.py MAX_ACCEL, lib/simulation.py Simulation.MAX_SPEED, BicycleModelDimensions' width, BicycleRealDimensions' wheelbase)
PAR_NAMES = ("dt", "max_accel", "max_speed", "centerline", "width", "ref_d", "buf_d", "thr_d", "ref_c", "buf_c", "thr_c", "wheelbase")
DEFAULT_PAR = {"dt": 0.1, "max_accel": 2.0, "max_speed": 30.0 / 3.6, "centerline": 0.0, "width": 2.0, "ref_d": 10.0, "buf_d": 2.0,
               "thr_d": 8.0, "ref_c": 8.0, "buf_c": 2.0, "thr_c": 5.0, "wheelbase": 1.0}
IDEAL = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)                # (cyclist, driver, policymaker)
AGENT_WEIGHTS = {"policymaker": 1 / 9, "driver": 4 / 9, "cyclist": 4 / 9}   # the fixed row of evaluate_trajectories_for_reasons (:1360-1365)
DETAIL_KEYS = ("policymaker", "driver", "cyclist_comfort", "cyclist_time", "cyclist_combined")


def par_row(**over) -> np.ndarray:
    p = dict(DEFAULT_PAR)
    p.update(over)
    return np.array([p[k] for k in PAR_NAMES], dtype=np.float64)


def default_layout(n_cand: int):
    """The reference's list: planned candidates, the following one last, scored with the time of the one before it."""
    if n_cand == 0:
        return [], []
    return [0] * (n_cand - 1) + [1], list(range(n_cand - 1)) + [max(n_cand - 2, 0)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def score_situations(situations, weights, forms, ideal=IDEAL, device: int = 0, detail: bool = True, resampled: bool = True) -> dict:
    """One launch for S situations x their candidates x W weight rows.

    situations: dicts with `candidates` (list of (n, 3) [x, y, yaw] arrays), `ego` (x, y, yaw, v), `cyclist` (the get() tuple
    x, y, v, yaw, a, steering), `now` (policymaker, driver, cyclist values, time_elapsed_driver, time_passed_cyclist) and optionally
    `par` (a par_row), `modes` and `time_from` (default_layout otherwise).  weights [W][3] = (policymaker, driver, cyclist), forms [W].
    Returns the C call's arrays, `cand_off` among them; nothing is raised for a candidate with a status."""
    S = len(situations)
    cand_off = np.zeros(S + 1, dtype=np.int32)
    pts, pt_len, mode, tfrom = [], [], [], []
    for s, sit in enumerate(situations):
        cands = [np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1, 3)) for c in sit["candidates"]]
        md, tf = default_layout(len(cands))
        mode += list(sit.get("modes", md))
        tfrom += list(sit.get("time_from", tf))
        pts += cands
        pt_len += [len(c) for c in cands]
        cand_off[s + 1] = cand_off[s] + len(cands)
    ctot = int(cand_off[-1])
    pt_off = np.concatenate([[0], np.cumsum(pt_len)]).astype(np.int32)
    pts = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts else np.zeros((0, 3))
    mode, tfrom = np.asarray(mode, dtype=np.int32), np.asarray(tfrom, dtype=np.int32)
    ego = np.ascontiguousarray([s["ego"] for s in situations], dtype=np.float64).reshape(S, 4)
    cyc = np.ascontiguousarray([s["cyclist"] for s in situations], dtype=np.float64).reshape(S, 6)
    now = np.ascontiguousarray([s["now"] for s in situations], dtype=np.float64).reshape(S, 5)
    par = np.ascontiguousarray([s.get("par", par_row()) for s in situations], dtype=np.float64).reshape(S, len(PAR_NAMES))
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, 3)
    W = len(w)
    form = np.ascontiguousarray(forms, dtype=np.int32).reshape(W)
    idl = np.ascontiguousarray(ideal, dtype=np.float64).reshape(3)
    out = {"cand_off": cand_off, "status": np.zeros(ctot, dtype=np.int32), "n_samples": np.zeros(ctot, dtype=np.int32),
           "ct": np.empty(ctot), "avg": np.empty((ctot, 4)), "scores": np.empty((W, ctot)), "best": np.zeros((W, S), dtype=np.int32),
           "detail": np.empty((ctot, 5, MAX_RES)) if detail else None, "resampled": np.empty((ctot, MAX_RES, 3)) if resampled else None}
    lib = _cabi.load()
    rc = lib.jsim_score_trajectories(int(device), S, _ptr(cand_off), _ptr(pt_off), _ptr(pts), _ptr(mode), _ptr(tfrom), _ptr(ego), _ptr(cyc),
                                     _ptr(now), _ptr(par), W, _ptr(w), _ptr(form), _ptr(idl), _ptr(out["status"]), _ptr(out["n_samples"]),
                                     _ptr(out["ct"]), _ptr(out["avg"]), _ptr(out["scores"]), _ptr(out["best"]), _ptr(out["detail"]),
                                     _ptr(out["resampled"]))
    _cabi.check(rc, None, "jsim_score_trajectories")
    return out


def _situation(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
               reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver, time_passed_cyclist, **layout):
    over = {}
    if car_dimensions is not None:
        over["width"] = float(car_dimensions.bounding_box_size[0])
    if bicycle_dimensions is not None:
        over["wheelbase"] = float(bicycle_dimensions.distance_back_to_front_wheel)
    sit = {"candidates": [t[0] if isinstance(t, (tuple, list)) else t for t in trajectories_full],
           "ego": (state.x, state.y, state.yaw, state.v), "cyclist": tuple(moving_obstacles[0].get()),
           "now": (reasons_policymaker_reg_compliance, reasons_driver_time_eff, reasons_cyclist_comfort, time_elapsed_driver, time_passed_cyclist),
           "par": par_row(**over)}
    sit.update(layout)
    return sit


def _raise_on_status(out):
    bad = np.nonzero(out["status"])[0]
    if len(bad):
        raise ValueError(f"candidate {int(bad[0])}: status {int(out['status'][bad[0]])} (2: too few points or a completion time the "
                         f"reference has no defined behaviour for; 4: more than {MAX_RES} resampled points)")


def _evaluations(out, row, pol_col):
    evals = []
    for c in range(len(out["status"])):
        m = int(out["n_samples"][c])
        d = out["detail"][c]
        lens = (m - 1, m - 1, m, m, m - 1)
        evals.append({"trajectory_idx": c, "total_score": float(out["scores"][row, c]), "completion_time": float(out["ct"][c]),
                      "avg_scores": {"policymaker": float(out["avg"][c, pol_col]), "driver": float(out["avg"][c, 2]), "cyclist": float(out["avg"][c, 3])},
                      "detailed_scores": {k: d[q, :n].tolist() for q, (k, n) in enumerate(zip(DETAIL_KEYS, lens))}})
    return evals


def _result(trajectories_full, out, row, pol_col):
    evals = _evaluations(out, row, pol_col)
    best = int(out["best"][row, 0])
    return {"scores": [float(x) for x in out["scores"][row]], "best_idx": best, "best_trajectory": trajectories_full[best],
            "best_evaluation": evals[best], "all_evaluations": evals}


def compute_predicted_trajectory(state, trajectory_res, last_index=None, device: int = 0):
    """The candidate resampled by the distance the ego covers per DT (:244-266)."""
    sit = {"candidates": [trajectory_res], "ego": (state.x, state.y, state.yaw, state.v), "cyclist": (0.0,) * 6, "now": (1.0, 1.0, 1.0, 0.0, 0.0),
           "modes": [0 if last_index is None else 1], "time_from": [0]}
    out = score_situations([sit], np.zeros((0, 3)), np.zeros(0, dtype=np.int32), device=device, detail=False)
    if out["status"][0] == 4 or out["n_samples"][0] < 1:
        _raise_on_status(out)
    return out["resampled"][0, :int(out["n_samples"][0])].copy()


def create_following_trajectory(state, trajectories_full, device: int = 0):
    """The "stay behind the cyclist" candidate (:410-445): candidate 0 resampled and timed in one launch, then the reference's
    np.arange / pad / truncate expressions on the host."""
    first = trajectories_full[0][0] if isinstance(trajectories_full[0], (tuple, list)) else trajectories_full[0]
    sit = {"candidates": [first], "ego": (state.x, state.y, state.yaw, state.v), "cyclist": (0.0,) * 6, "now": (1.0, 1.0, 1.0, 0.0, 0.0),
           "modes": [0], "time_from": [0]}
    out = score_situations([sit], np.zeros((0, 3)), np.zeros(0, dtype=np.int32), device=device, detail=False)
    _raise_on_status(out)
    n = int(out["n_samples"][0])
    follow = out["resampled"][0, :n].copy()
    ct = float(out["ct"][0])
    dt = DEFAULT_PAR["dt"]
    ys = np.arange(follow[0, 1], follow[0, 1] + (ct * state.v), (state.v * dt))
    if len(ys) < n:
        ys = np.append(ys, np.repeat(ys[-1], n - len(ys)))
    else:
        ys = ys[:n]
    follow[:, 1] = ys
    follow[:, 0] = follow[0, 0]
    follow[:, 2] = follow[0, 2]
    return follow


def balance_function(weights, ideal_weights=None):
    """Deviation of the weights from the ideal ones times the smallest weight / ideal ratio (:1191-1231); the kernel computes the
    same expression per weight row."""
    n = len(weights)
    if ideal_weights is None:
        ideal_weights = [1 / n] * n
    if len(ideal_weights) != n:
        raise ValueError("ideal_weights must have the same length as weights")
    ratio = min(w / i for w, i in zip(weights, ideal_weights))
    rms = np.sqrt(sum((w - i) ** 2 for w, i in zip(weights, ideal_weights)) / n)
    return (1 - (rms / np.sqrt(sum(i ** 2 for i in ideal_weights)))) * ratio


def evaluate_trajectories_for_reasons(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                                      reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver=0.0,
                                      time_passed_cyclist=0.0, device: int = 0):
    sit = _situation(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                     reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver, time_passed_cyclist)
    w = AGENT_WEIGHTS
    out = score_situations([sit], [(w["policymaker"], w["driver"], w["cyclist"])], [0], device=device)
    _raise_on_status(out)
    return dict(AGENT_WEIGHTS), _result(trajectories_full, out, 0, 0)


def evaluate_trajectories_with_weights(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                                       reasons_driver_time_eff, reasons_policymaker_reg_compliance, policymaker_weight, driver_weight,
                                       cyclist_weight, time_elapsed_driver=0.0, time_passed_cyclist=0.0, device: int = 0):
    if policymaker_weight == 0.0 and driver_weight == 0.0 and cyclist_weight == 0.0:      # (:1670-1679)
        return {"scores": [0.0] * len(trajectories_full), "best_idx": 0, "best_trajectory": trajectories_full[0] if len(trajectories_full) else None,
                "best_evaluation": None, "all_evaluations": []}
    sit = _situation(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                     reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver, time_passed_cyclist)
    out = score_situations([sit], [(policymaker_weight, driver_weight, cyclist_weight)], [1], device=device)
    _raise_on_status(out)
    return _result(trajectories_full, out, 0, 1)


def weight_triples(weight_step):
    """The (policymaker, driver, cyclist) grid of :1464-1500, rounded as there; in sorted order."""
    precision = max(int(-np.log10(weight_step)) + 2, 6)
    values = np.arange(0, 1.0 + weight_step / 2, weight_step)
    combos = set()
    for policy_w in values:
        for driver_w in values:
            cyclist_w = round(1.0 - policy_w - driver_w, precision)
            if 0 <= cyclist_w <= 1.0 + 1e-9:
                combos.add((round(round(policy_w, precision), precision), round(round(driver_w, precision), precision), round(cyclist_w, precision)))
    return sorted(t for t in combos if abs(t[0] + t[1] + t[2] - 1.0) <= 1e-6), precision


def _label(best_indices):
    names = [f"Traj {i}" for i in best_indices[:4]]
    if len(names) == 1:
        return names[0]
    if len(names) == 2:
        return f"{names[0]} and {names[1]}"
    return ", ".join(names[:-1]) + f", and {names[-1]}"


def generate_stakeholder_weight_table(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                                      reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver, time_passed_cyclist,
                                      weight_step=0.1, save_path=None, device: int = 0):
    """(policy_data, driver_data, cyclist_data) of :1431-1604: every weight triple of the grid scored in ONE launch; rows, the 1e-6
    best-label rule, the split by dominant weight and the sort orders as in :1511-1580.  save_path: the rows as CSV."""
    triples, precision = weight_triples(weight_step)
    sit = _situation(trajectories_full, moving_obstacles, state, car_dimensions, bicycle_dimensions, reasons_cyclist_comfort,
                     reasons_driver_time_eff, reasons_policymaker_reg_compliance, time_elapsed_driver, time_passed_cyclist)
    out = score_situations([sit], triples, [1] * len(triples), device=device, detail=False, resampled=False)
    _raise_on_status(out)
    groups = ([], [], [])
    for (policy_w, driver_w, cyclist_w), row in zip(triples, out["scores"]):
        scores = [0.0 if x < 0 else float(x) for x in row]
        top = max(scores)
        if top > 1.0:
            scores = [x / top for x in scores]
            top = max(scores)
        best = [i for i, x in enumerate(scores) if abs(x - top) < 0.000001]
        line = [policy_w, driver_w, cyclist_w] + [scores[i] if i < len(scores) else 0.0 for i in range(4)] + [_label(best)]
        big = max(policy_w, driver_w, cyclist_w)
        if big == policy_w or (policy_w == driver_w and policy_w == cyclist_w):
            groups[0].append(line)
        elif big == driver_w:
            groups[1].append(line)
        else:
            groups[2].append(line)
    policy_data = sorted(groups[0], key=lambda x: (round(x[0], precision), round(x[1], precision)))
    driver_data = sorted(groups[1], key=lambda x: (round(x[1], precision), round(x[0], precision)))
    cyclist_data = sorted(groups[2], key=lambda x: (round(x[2], precision), round(x[0], precision)))
    if save_path:
        with open(save_path, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(["policy_w", "driver_w", "cyclist_w", "Traj 0", "Traj 1", "Traj 2", "Traj 3", "best_traj_label"])
            wr.writerows(policy_data + driver_data + cyclist_data)
    return policy_data, driver_data, cyclist_data


# ---- per-tick reasons of a recorded run (jsim_loop_eval_reasons): the host side of Recorder.reasons ----
def tick_inputs(B, n_obs, dt, par=None, threshold=0.7, cyclist=None, carry=None, default_cyclist=None):
    """Recorder.reasons' arguments as the arrays the C call takes: par [B][12], threshold [B], veh_of [B] int32, carry [B][3].
    What the C call cannot check without a device read is refused here (ValueError): a par that is not one row or [B] rows of
    finite numbers, DT <= 0, a threshold or carry that is not finite or of the wrong shape, a cyclist outside -1 .. n_obs - 1."""
    par = np.asarray(par_row(dt=dt) if par is None else par, dtype=np.float64)
    if par.ndim == 1:
        par = np.broadcast_to(par, (B, par.size))
    if par.shape != (B, len(PAR_NAMES)) or not np.isfinite(par).all():
        raise ValueError(f"par must be one row or [{B}] rows of {len(PAR_NAMES)} finite numbers (reasons.par_row)")
    if not (par[:, 0] > 0.0).all():
        raise ValueError("par: DT must be positive")
    thr = np.asarray(threshold, dtype=np.float64)
    thr = np.broadcast_to(thr, (B,)) if thr.ndim == 0 else thr
    if thr.shape != (B,) or not np.isfinite(thr).all():
        raise ValueError(f"threshold must be one finite number or [{B}]")
    veh = (default_cyclist() if default_cyclist is not None else np.zeros(B, dtype=np.int32)) if cyclist is None else np.asarray(cyclist)
    veh = np.broadcast_to(veh, (B,)) if veh.ndim == 0 else veh
    if veh.shape != (B,) or not np.issubdtype(veh.dtype, np.integer) or veh.min(initial=0) < -1 or veh.max(initial=-1) >= n_obs:
        raise ValueError(f"cyclist must be one vehicle index or [{B}], each -1 (none) or 0..{n_obs - 1}")
    car = np.zeros((B, 3)) if carry is None else np.asarray(carry, dtype=np.float64)
    if car.shape != (B, 3) or not np.isfinite(car).all():
        raise ValueError(f"carry must be [{B}][3] finite numbers")
    return np.array(par), np.array(thr), np.array(veh, dtype=np.int32), np.array(car)


def situation_at(recorder, b: int, k: int, candidates, reasons=None, **layout) -> dict:
    """The situation (score_situations) of ego b at the start of recorded tick k, from a loop's recorder: `ego` (x, y, yaw, v) is the
    state the tick started from, `cyclist` the recorded get() tuple of the ego's cyclist, `now` that tick's three values and two
    timers, `par` the row they were evaluated with -- what perform_replan is handed when the trigger fires on tick k
    (main/scenarios/overtaking_cyclist_bidirectional_road.py:149-161).  reasons: the dict of recorder.reasons() (evaluated with
    its defaults when None); layout: `modes` / `time_from` of the candidates when they are not the reference's list."""
    r = recorder.reasons() if reasons is None else reasons
    n = r["policymaker"].shape[0]
    if not (0 <= k < n) or not (0 <= b < r["policymaker"].shape[1]):
        raise ValueError(f"ego {b}, tick {k}: the evaluation holds {n} ticks of {r['policymaker'].shape[1]} egos")
    veh = int(r["veh_of"][b])
    if veh < 0:
        raise ValueError(f"ego {b} has no cyclist")
    fl = int(recorder.flags[k - 1, b].item()) if k > 0 else 0
    if k == 0 or fl & (GOAL | AGE):                           # (the tick starts at the spawn state)
        x, y, v, yaw = (recorder.x0_first if k == 0 else recorder.loop.x0_spawn)[b].cpu().numpy().tolist()
    else:
        x, y, yaw, v = recorder.rec[k - 1, b, :4].cpu().numpy().tolist()
    sit = {"candidates": list(candidates), "ego": (x, y, yaw, v), "cyclist": tuple(recorder.obs[k, veh].cpu().numpy().tolist()),
           "now": (float(r["policymaker"][k, b]), float(r["driver"][k, b]), float(r["cyclist"][k, b]), float(r["timers"][k, b, 0]),
                   float(r["timers"][k, b, 1])), "par": np.array(r["par"][b])}
    sit.update(layout)
    return sit
