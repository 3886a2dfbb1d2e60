"""The cases of tests/golden/reasons.npz (made by tests/golden/make_golden_reasons.py from the reference) as plain Python: loaded once
and shared by the CPU and GPU tests of the stakeholder-reasons scoring."""
import ctypes
import functools
import os

import numpy as np

import reasons_numpy as RN
from conftest import GOLDEN

KEYS = ("policymaker", "driver", "cyclist_comfort", "cyclist_time", "cyclist_combined")
FIXED_ROW = (1 / 9, 4 / 9, 4 / 9)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "reasons.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def cases():
    """One dict per case: the situation in the form reasons.score_situations takes, plus the reference's results."""
    g = fixture()
    pm = np.load(os.path.join(GOLDEN, "planner_multi.npz"), allow_pickle=False)
    out = []
    for i in range(int(g["n_cases"])):
        cands = [g["pool_" + s[5:]] if s.startswith("pool:") else np.asarray(pm[s[3:]], dtype=np.float64) for s in g[f"c{i}_src"].tolist()]
        cands.append(g[f"c{i}_follow"])
        case = {"label": str(g[f"c{i}_label"]), "candidates": cands, "ego": tuple(g[f"c{i}_ego"]), "cyclist": tuple(g[f"c{i}_cyc"]),
                "now": tuple(g[f"c{i}_now"]), "par": g["par"].copy()}
        for k in ("scores", "best", "w_scores", "w_best", "ct", "ct0", "avg", "m", "detail", "cyc_idx", "in_range", "follow"):
            case["ref_" + k] = g[f"c{i}_{k}"]
        case["tables"] = None
        if bool(g[f"c{i}_has_table"]):
            case["tables"] = tuple((g[f"c{i}_table_{n}"], g[f"c{i}_table_{n}_label"].tolist()) for n in ("policy", "driver", "cyclist"))
        out.append(case)
    return out


def situation(case):
    return {k: case[k] for k in ("candidates", "ego", "cyclist", "now", "par")}


@functools.lru_cache(maxsize=None)
def restated():
    """The numpy restatement on every case with the two reference rows (form 0 fixed row, form 1 W_FIXED): computed once."""
    w = [FIXED_ROW, tuple(fixture()["w_fixed"])]
    res = []
    for c in cases():
        modes, tf = RN.default_layout(len(c["candidates"]))
        res.append(RN.score_situation(c["candidates"], modes, tf, c["ego"], c["cyclist"], c["now"], c["par"], w, [0, 1]))
    return res


def close(a, b, rtol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


class State:
    def __init__(self, x, y, yaw, v):
        self.x, self.y, self.yaw, self.v = x, y, yaw, v


class Cyclist:
    def __init__(self, tup):
        self.tup = tuple(tup)

    def get(self):
        return self.tup


def raw_call(pkg, sits, weights=(FIXED_ROW,), forms=(0,), ideal=RN.IDEAL, null=(), edit=None, device=0):
    """jsim_score_trajectories through ctypes with every table editable (edit(tables) before the call) or nulled: (rc, tables)."""
    t = {}
    cands = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for s in sits for c in s["candidates"]]
    t["cand_off"] = np.concatenate([[0], np.cumsum([len(s["candidates"]) for s in sits])]).astype(np.int32)
    t["pt_off"] = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int32)
    t["pts"] = np.ascontiguousarray(np.concatenate(cands, axis=0)) if cands else np.zeros((0, 3))
    layouts = [RN.default_layout(len(s["candidates"])) for s in sits]
    t["mode"] = np.array([m for s, l in zip(sits, layouts) for m in s.get("modes", l[0])], dtype=np.int32)
    t["time_from"] = np.array([m for s, l in zip(sits, layouts) for m in s.get("time_from", l[1])], dtype=np.int32)
    t["ego"] = np.array([s["ego"] for s in sits], dtype=np.float64)
    t["cyc"] = np.array([s["cyclist"] for s in sits], dtype=np.float64)
    t["now"] = np.array([s["now"] for s in sits], dtype=np.float64)
    t["par"] = np.array([s.get("par", RN.DEFAULT_PAR) for s in sits], dtype=np.float64)
    t["w"] = np.array(weights, dtype=np.float64).reshape(-1, 3)
    t["form"] = np.array(forms, dtype=np.int32)
    t["ideal"] = np.array(ideal, dtype=np.float64)
    if edit:
        edit(t)
    S, W, ctot = len(sits), len(t["w"]), int(t["cand_off"][-1]) if t["cand_off"][-1] > 0 else len(cands)
    t["status"] = np.full(ctot, -7, dtype=np.int32)
    t["n_samples"] = np.full(ctot, -7, dtype=np.int32)
    t["ct"], t["avg"], t["scores"] = np.zeros(ctot), np.zeros((ctot, 4)), np.zeros((W, ctot))
    t["best"] = np.full((W, S), -7, dtype=np.int32)
    order = ("cand_off", "pt_off", "pts", "mode", "time_from", "ego", "cyc", "now", "par", "w", "form", "ideal", "status", "n_samples", "ct",
             "avg", "scores", "best")
    p = {k: (None if k in null else t[k].ctypes.data_as(ctypes.c_void_p)) for k in order}
    rc = pkg._cabi.load().jsim_score_trajectories(device, S, p["cand_off"], p["pt_off"], p["pts"], p["mode"], p["time_from"], p["ego"], p["cyc"],
                                                  p["now"], p["par"], W, p["w"], p["form"], p["ideal"], p["status"], p["n_samples"], p["ct"],
                                                  p["avg"], p["scores"], p["best"], None, None)
    return rc, t
