"""The cases of tests/test_gpu_helper_status.py and tests/test_helper_status_cpu.py: 8 egos at every horizon that has a kernel with
helper wavefronts (13, 15, 16, 20, 25), in that form and in the plain one-wave form.

  step   one step through the debug entry with H and g requested, on two ego sets: the off-path tight family of
         tests/active_set_cases.py with its draw's warm start (issue_slots_cases.ego_set) and, where the fixture exists (13, 20), the
         first 8 egos of tests/golden/stages_T<T>.npz.
  loop   LAUNCHES launches of TICKS ticks each of ClosedLoop on a mixed batch -- fused (one call per launch) and tick by tick -- and, at
         the horizons whose helper kernel has the loop glue inside (13, 20), of ScenarioLoop with the stock scripted vehicles.  The
         mixed batch is the off-path tight family with two failing egos planted through the per-ego table: IN_LOOP (active_set_cases'
         family A: the solver finds the contradiction inside the active-set loop, after iterations) and BEFORE_LOOP (v0 above the speed
         limit: the exit in front of the loop, no iteration).  Beside the buffers the loops leave, every launch's per-ego iteration
         totals (jsim_mpc_iter_totals): read without reset after launches 1 and 2, with reset after launch 2, and again after launch 3.

Run as a script this module runs every case in ITS process and stores the outputs in an .npz: the kernel form follows
JSIM_HELP_MAX_B, which the library reads once per process.
usage: helper_status_cases.py out.npz"""
import importlib
import os
import sys
from dataclasses import replace

import numpy as np

import active_set_cases as AC
import issue_slots_cases as IS
from gpu_helpers import PLANT_DECEL

PKG_NAME = IS.PKG_NAME
HORIZONS = (13, 15, 16, 20, 25)      # csrc/reg_variants.h: the rows with HELP
PRE_HORIZONS = (13, 20)              # .. with PRE and HELP
FIXTURE_HORIZONS = IS.FIXTURE_HORIZONS
B, TICKS, LAUNCHES = 8, 6, 3
IN_LOOP, BEFORE_LOOP = 5, 6          # the planted egos
STEP_KEYS = ("oa", "od", "status", "target_ind", "n_iter", "active_mask")
LOOP_KEYS = IS.LOOP_KEYS
MAX_AGE = 400                        # no respawn inside the 18 ticks


def mixed_set(pkg, routes, T):
    """(batch, cfgs, which): the off-path tight family, ego IN_LOOP an infeasible-A ego, ego BEFORE_LOOP above its speed limit."""
    base = replace(pkg.MPCConfig.from_json(), T=T)
    batch = AC.off_path_batch(pkg.synth, routes, B, T)
    rows = {AC.ROW_TIGHT: AC.tight_config(base, T), AC.ROW_A: AC.a_config(base, T), AC.ROW_V0: replace(base, T=T, MAX_DECEL=PLANT_DECEL)}
    which = np.full(B, AC.ROW_TIGHT, dtype=np.int64)
    batch.x0[IN_LOOP, 2] = batch.speed[IN_LOOP] - AC.A_MARGIN
    batch.x0[BEFORE_LOOP, 2] = AC.V0_ABOVE
    which[IN_LOOP], which[BEFORE_LOOP] = AC.ROW_A, AC.ROW_V0
    return batch, [rows[k] for k in which], which, base


def step(pkg, routes, batch, T, **kw):
    """One step of a fresh engine through jsim_mpc_step_debug with H and g requested."""
    import torch
    eng = IS._engine(pkg, routes, batch, T, **kw)
    n = 2 * T
    dbg = {"H": torch.zeros(eng.B, n, n, dtype=torch.float64, device=eng.device), "g": torch.zeros(eng.B, n, dtype=torch.float64, device=eng.device)}
    eng.solve(torch.from_numpy(batch.x0).to(eng.device), debug=dbg)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in STEP_KEYS}
    out.update({k: v.cpu().numpy().copy() for k, v in dbg.items()})
    return out


def _totals(pkg, eng, reset):
    cabi = importlib.import_module(PKG_NAME + "._cabi")
    tot = np.zeros(eng.B, dtype=np.uint64)
    cabi.check(eng.lib.jsim_mpc_iter_totals(eng._ctx, eng.B, tot.ctypes.data, 1 if reset else 0), eng._ctx, "jsim_mpc_iter_totals")
    return tot.astype(np.int64)


def loop(pkg, routes, T, fused, scenario):
    """LAUNCHES x TICKS ticks on the mixed batch.  fused: "totals" [4, B] as the module docstring lists them; tick by tick: "n_iter"
    [LAUNCHES * TICKS, B] and "status_by_tick"."""
    import torch
    batch, cfgs, _, base = mixed_set(pkg, routes, T)
    eng = IS._engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    x0 = torch.from_numpy(batch.x0).to(eng.device)
    K = LAUNCHES * TICKS
    if scenario:
        sc = pkg.ScenarioLoop(eng, x0, pkg.workloads.OBSTACLE_SPECS, hist_cap=K, max_age=MAX_AGE)
        lp, drv = sc.loop, sc
    else:
        lp = drv = pkg.ClosedLoop(eng, x0, hist_cap=K, max_age=MAX_AGE)
    out = {}
    if fused:
        tot = []
        for n in range(LAUNCHES):
            drv.run(TICKS)
            torch.cuda.synchronize()
            tot.append(_totals(pkg, eng, reset=False))
            if n == 1:
                tot.append(_totals(pkg, eng, reset=True))
        out["totals"] = np.stack(tot)
    else:
        n_iter, st = [], []
        for _ in range(K):
            drv.tick()
            n_iter.append(eng.n_iter.cpu().numpy().astype(np.int64))
            st.append(eng.status.cpu().numpy().copy())
        out["n_iter"], out["status_by_tick"] = np.stack(n_iter), np.stack(st)
    torch.cuda.synchronize()
    d = dict(hist=lp.hist[:K], oa=eng.oa, od=eng.od, state=lp.x0, status=eng.status, target_ind=eng.target_ind)
    out.update({k: v.cpu().numpy().copy() for k, v in d.items()})
    return out


def run_all(pkg, routes):
    """{"<case>_T<T>_<key>": array} of every case in this process's kernel form."""
    out = {}
    for T in HORIZONS:
        batch, cfg = IS.ego_set(pkg, routes, T)
        cases = {"step": step(pkg, routes, batch, T, config=cfg), "fused": loop(pkg, routes, T, True, False),
                 "ticked": loop(pkg, routes, T, False, False)}
        if T in FIXTURE_HORIZONS:
            cases["fix"] = step(pkg, routes, IS.fixture_set(pkg, T)[0], T)
        if T in PRE_HORIZONS:
            cases["sfused"], cases["sticked"] = loop(pkg, routes, T, True, True), loop(pkg, routes, T, False, True)
        for name, d in cases.items():
            for k, v in d.items():
                out[f"{name}_T{T}_{k}"] = v
    return out


def main(path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    pkg = importlib.import_module(PKG_NAME)
    out = run_all(pkg, IS.synth_routes(pkg))
    out["help_max_b"] = np.array(os.environ.get("JSIM_HELP_MAX_B", ""))
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
