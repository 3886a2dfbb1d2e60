"""The one-step cases of tests/test_gpu_full_set.py that compare the two one-wave kernel forms: the full-set family of
tests/active_set_cases.py, every form at its own size (48 .. 96 egos: below one ego per CU, so the dispatch takes the kernel with
helper wavefronts), at every horizon that has such a kernel, through the debug entry with H, g and the multipliers requested.

Run as a script this module runs every case in ITS process and stores the outputs in an .npz: the kernel form follows
JSIM_HELP_MAX_B, which the library reads once per process.
usage: full_set_child.py out.npz"""
import importlib
import os
import sys
from dataclasses import replace

import numpy as np

import active_set_cases as AC
import issue_slots_cases as IS

PKG_NAME = IS.PKG_NAME
HORIZONS = (13, 15, 16, 20, 25)      # csrc/reg_variants.h: the rows with HELP
FORMS = ("drops", "adds", "mixed")
KEYS = ("oa", "od", "status", "target_ind", "n_iter", "active_mask")


def step(pkg, routes, T, form):
    """One debug step of the family's form at its own size."""
    import torch
    base = replace(pkg.MPCConfig.from_json(), T=T)
    batch, cfgs, _ = AC.full_set_case(pkg.synth, routes, base, AC.FULL_B[form], T, form)
    eng = IS._engine(pkg, routes, batch, T, config=base)
    eng.set_ego_configs(cfgs)
    n, f = 2 * T, dict(dtype=torch.float64, device=eng.device)
    dbg = {"H": torch.zeros(eng.B, n, n, **f), "g": torch.zeros(eng.B, n, **f), "lam": torch.zeros(eng.B, 8 * T, **f)}
    eng.solve(torch.from_numpy(batch.x0).to(eng.device), debug=dbg)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in KEYS}
    out.update({k: v.cpu().numpy().copy() for k, v in dbg.items()})
    return out


def run_all(pkg, routes):
    """{"<form>_T<T>_<key>": array} of every case in this process's kernel form."""
    return {f"{form}_T{T}_{k}": v for T in HORIZONS for form in FORMS for k, v in step(pkg, routes, T, form).items()}


def main(path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    pkg = importlib.import_module(PKG_NAME)
    out = run_all(pkg, IS.synth_routes(pkg))
    out["help_max_b"] = np.array(os.environ.get("JSIM_HELP_MAX_B", ""))
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
