"""The checkpoints of a loop restated in plain Python and numpy, one element at a time: where run(n) is cut
and which slot is saved ahead of each piece, walked tick by tick; the gather of jsim_loop_checkpoint_load, row by row and vehicle
by vehicle.  Written from the entry points' descriptions in include/jsim_mpc.h, not from the package's code."""
import numpy as np


def cuts(t0, n, every, cap):
    """[(slot, ticks)] of run(n) from tick t0, found by walking the ticks one at a time: a tick that is a multiple of `every` and
    <= cap is saved to slot tick // every and starts a new piece; every other tick goes on with the piece it is in."""
    out = []
    for t in range(t0, t0 + n):
        due = t % every == 0 and t <= cap
        if due or not out:
            out.append([t // every if due else -1, 0])
        out[-1][1] += 1
    return [tuple(p) for p in out]


def saved_ticks(t0, n, every, cap):
    """The ticks a run of n ticks from t0 saves."""
    return [t for t in range(t0, t0 + n) if t % every == 0 and t <= cap]


def gather(slabs, ego, slot):
    """{name: [R]...}: row r of every slab [n_slots][B]... is ego ego[r] of slot slot[r]."""
    out = {}
    for name, slab in slabs.items():
        rows = np.empty((len(ego),) + slab.shape[2:], dtype=slab.dtype)
        for r in range(len(ego)):
            rows[r] = slab[slot[r]][ego[r]]
        out[name] = rows
    return out


def vehicles(obs_slab, veh_src, veh_slot):
    """[n_veh][4]: vehicle o is vehicle veh_src[o] of slot veh_slot[o] of obs_slab [n_slots][n_obs][4]."""
    out = np.empty((len(veh_src), 4), dtype=obs_slab.dtype)
    for o in range(len(veh_src)):
        out[o] = obs_slab[veh_slot[o]][veh_src[o]]
    return out


def load(slabs, per, ego, slot, veh_src, veh_slot):
    """jsim_loop_checkpoint_load on host slabs: the rows of every per-ego array (per[name] == "ego") and the vehicles' states
    ("vehicle"); an array with one value per loop ("loop") is not gathered."""
    out = gather({k: v for k, v in slabs.items() if per[k] == "ego"}, ego, slot)
    out.update({k: vehicles(v, veh_src, veh_slot) for k, v in slabs.items() if per[k] == "vehicle"})
    return out


def fork_traffic(set_of_row, at, obs_off):
    """The traffic sets of a fork: one per (source set, tick) in order of first appearance.  Returns (tof [rows], veh_src, veh_tick):
    the new vehicles, set after set, as (source vehicle, tick) pairs."""
    keys, tof = [], []
    for s, k in zip(set_of_row, at):
        if (s, k) not in keys:
            keys.append((s, k))
        tof.append(keys.index((s, k)))
    veh_src = [o for s, _ in keys for o in range(obs_off[s], obs_off[s + 1])]
    veh_tick = [k for s, k in keys for _ in range(obs_off[s], obs_off[s + 1])]
    return tof, veh_src, veh_tick
