"""Checkpoints of a running loop (jsim_loop_checkpoint_save / _load) without a GPU: where run(n) is cut
(history.checkpoint_cuts) against a tick-by-tick walk; the gather against the numpy restatement (tests/checkpoint_numpy.py) on
hand-made slabs; history.CHECKPOINT against the loops' attribute names and the entry points' argument lists; the refusals that
need no context; the header, binding and INTEGRATION rows; and the .npz round trip."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import checkpoint_numpy as CN
from conftest import REPO


# ---- 1. the cut rule ----
@pytest.mark.parametrize("C", (1, 2, 25, 64))
def test_cuts_around_every_multiple_and_the_cap(pkg, C):
    H = pkg.history
    for cap in sorted({0, 1, C - 1, C, C + 1, 3 * C - 1, 3 * C, 3 * C + 1} - {-1}):
        marks = sorted({0, cap, cap + 1, cap + 2 * C} | {m * C + d for m in range(5) for d in (-1, 0, 1) if m * C + d >= 0})
        for t0 in marks:
            for t1 in marks:
                if t1 < t0:
                    continue
                got = H.checkpoint_cuts(t0, t1 - t0, C, cap)
                assert got == CN.cuts(t0, t1 - t0, C, cap), (C, cap, t0, t1)
                assert sum(m for _, m in got) == t1 - t0 and all(m >= 1 for _, m in got)
                # what is saved: every multiple of C in [t0, t1) up to cap, to the slot of its tick, within the loop's slots
                t, saved = t0, []
                for slot, m in got:
                    if slot >= 0:
                        assert slot * C == t and slot < H.checkpoint_slots(C, cap)
                        saved.append(t)
                    t += m
                assert saved == CN.saved_ticks(t0, t1 - t0, C, cap)


def test_cuts_spelt_out(pkg):
    cuts = pkg.history.checkpoint_cuts
    assert cuts(0, 100, 25, 100) == [(0, 25), (1, 25), (2, 25), (3, 25)]               # the end state is saved by the next run
    assert cuts(100, 1, 25, 100) == [(4, 1)]                                           # .. as slot cap // C, the last one
    assert cuts(10, 50, 25, 100) == [(-1, 15), (1, 25), (2, 10)] and cuts(10, 39, 25, 100) == [(-1, 15), (1, 24)]
    assert cuts(0, 300, 100, 120) == [(0, 100), (1, 200)]                              # beyond cap: neither saved nor cut
    assert cuts(130, 500, 100, 120) == [(-1, 500)]
    assert cuts(7, 0, 5, 50) == [] and cuts(0, 3, 1, 1) == [(0, 1), (1, 2)]
    assert pkg.history.checkpoint_slots(25, 100) == 5 and pkg.history.checkpoint_slots(25, 99) == 4 and pkg.history.checkpoint_slots(1, 7) == 8
    for bad in ((-1, 1, 1, 1), (0, -1, 1, 1), (0, 1, 0, 1), (0, 1, 1, -1)):
        with pytest.raises(ValueError, match="checkpoint_cuts needs"):
            cuts(*bad)


def test_a_tick_that_is_not_checkpointed_names_its_neighbours(pkg):
    at = pkg.history.checkpoint_at
    st = np.array([0, 25, 50, -1, 53, 50])
    assert at(st, [0, 50, 53, 25]).tolist() == [0, 2, 4, 1]                            # of two slots with one tick the lower
    for k, near in ((30, "25 and 50"), (51, "50 and 53"), (60, "53"), (-1, "0")):
        with pytest.raises(ValueError, match=rf"row 1: tick {k} is not checkpointed \(the nearest checkpointed ticks: {near}\)"):
            at(st, [0, k])
    with pytest.raises(ValueError, match="nearest checkpointed ticks: none"):
        at(np.array([-1, -1]), [0])


# ---- 2. the gather ----
def slabs_for(pkg, n_slots, B, T, n_obs, seed):
    """Hand-made slabs of every array of history.CHECKPOINT: distinct numbers everywhere."""
    rng = np.random.default_rng(seed)
    dims = {"B": B, "T": T, "n_obs": n_obs}
    out = {}
    for a in pkg.history.CHECKPOINT:
        shape = (n_slots,) + tuple(dims.get(d, d) for d in a.shape)
        if 0 in shape:
            continue
        v = rng.permutation(int(np.prod(shape))).reshape(shape)
        out[a.name] = (v + 0.25).astype(a.dtype) if a.dtype is np.float64 else v.astype(a.dtype)
    return out


@pytest.mark.parametrize("B, n_slots, n_obs, ego, slot, veh", (
    (6, 5, 5, [0, 5, 3, 3, 3, 1], [0, 4, 2, 2, 1, 4], ([0, 1, 4, 4], [0, 0, 4, 2])),    # duplicates; the first and the last slot
    (1, 3, 2, [0, 0, 0], [2, 0, 1], ([1, 0], [2, 2])),                                # B = 1
    (4, 2, 0, [3, 2, 1, 0], [1, 1, 0, 0], ([], [])),                                  # no vehicles
    (3, 1, 1, [2], [0], ([0], [0])),                                                  # one slot, one row
))
def test_gather_restatement_on_hand_made_slabs(pkg, B, n_slots, n_obs, ego, slot, veh):
    """The restatement the device gather is held against (tests/test_gpu_checkpoint.py), itself against numpy's own indexing."""
    H = pkg.history
    T = 13
    slabs = slabs_for(pkg, n_slots, B, T, n_obs, seed=B)
    got = CN.load(slabs, {a.name: a.per for a in H.CHECKPOINT}, ego, slot, *veh)
    assert set(got) == {a.name for a in H.CHECKPOINT if a.per != "loop" and a.name in slabs}
    assert "tick_counter" not in got and "n_respawn" not in got                       # one value per loop: a fork starts its own
    for k, v in got.items():
        want = slabs[k][np.array(veh[1], dtype=int), np.array(veh[0], dtype=int)] if k == "obs_state" else slabs[k][np.array(slot), np.array(ego)]
        assert v.dtype == slabs[k].dtype and np.array_equal(v, want), k
    assert got["oa"].shape == (len(ego), T) and got["x0"].shape == (len(ego), 4) and ("obs_state" in got) == (n_obs > 0)
    r = len(ego) - 1                                                                  # spelt out: the last row, element by element
    assert got["oa"][r].tolist() == [slabs["oa"][slot[r], ego[r], t] for t in range(T)] and got["age"][r] == slabs["age"][slot[r]][ego[r]]


def test_two_traffic_sets_share_a_set_per_source_set_and_tick(pkg):
    # six egos in two source sets (two vehicles, one vehicle), forked at two ticks: rows of one source set and one tick share a set
    obs_off, set_of = [0, 2, 3], [0, 1, 0, 1, 0, 0]
    ego, at = [0, 1, 2, 3, 4, 5, 0], [25, 25, 25, 50, 50, 25, 50]
    tof, veh_src, veh_tick = CN.fork_traffic([set_of[e] for e in ego], at, obs_off)
    assert tof == [0, 1, 0, 2, 3, 0, 3] and veh_src == [0, 1, 2, 2, 0, 1] and veh_tick == [25, 25, 25, 50, 50, 50]
    slabs = slabs_for(pkg, 3, 6, 13, 3, seed=9)
    at_slot = lambda ticks: pkg.history.checkpoint_at([0, 25, 50], ticks)             # noqa: E731
    got = CN.load(slabs, {a.name: a.per for a in pkg.history.CHECKPOINT}, ego, at_slot(at), veh_src, at_slot(veh_tick))
    assert np.array_equal(got["obs_state"][3], slabs["obs_state"][2, 2]) and np.array_equal(got["obs_state"][1], slabs["obs_state"][1, 1])
    assert np.array_equal(got["oa"][6], slabs["oa"][2, 0]) and np.array_equal(got["oa"][0], slabs["oa"][1, 0])


# ---- 3. the layout is the loops' ----
NOT_STATE = {"eng.ox", "eng.oy", "eng.ov", "eng.oyaw", "eng.xref", "eng.active_mask", "eng.n_iter",   # the step's outputs
             "self.hist", "ob.get_buf",                                                               # written, never read by a tick
             "eng.path_id", "eng.speed", "ob.param"}                                                  # tables no tick writes
OWNER = {"self": "loop", "loop": "loop", "eng": "eng", "pre": "pre", "ob": "obst"}


def test_layout_names_the_loops_attributes(pkg):
    H, CL = pkg.history, pkg.closed_loop
    rows = H.CHECKPOINT
    assert len({a.name for a in rows}) == len(rows) <= H.CHECKPOINT_MAX_ARRAYS == pkg._cabi.CKPT_MAX_ARRAYS
    assert {a.per for a in rows} == {"ego", "loop", "vehicle"} and {a.owner for a in rows} == {"loop", "eng", "pre", "obst"}
    src = {"loop": inspect.getsource(CL.ClosedLoop), "eng": inspect.getsource(pkg.batched.BatchedMPC),
           "pre": inspect.getsource(CL.PreTick), "obst": inspect.getsource(CL.ScriptedObstacles)}
    for a in rows:
        assert re.search(rf"self\.{a.attr}\b[^\n]*=|\(\"{a.attr}\", torch\.", src[a.owner]), (a.owner, a.attr)   # (an attribute, or of the arena)
        assert a.dtype in (np.float64, np.int32, np.int64)
        assert a.shape[0] == {"ego": "B", "vehicle": "n_obs", "loop": 1}[a.per]
    # every device pointer the entry points take is a row of the layout or is known not to be state
    seen = set()
    for fn in (CL.ClosedLoop._loop_args, CL.ClosedLoop._advance_args, CL._GlueLoop._run_args):
        seen |= set(re.findall(r"_ptr\((\w+\.\w+)\)", inspect.getsource(fn)))
    state = {f"{o}.{a}" for o, a in (s.split(".") for s in seen - NOT_STATE)}
    assert {(OWNER[s.split(".")[0]], s.split(".")[1]) for s in state} <= {(a.owner, a.attr) for a in rows}
    # .. and beside the argument lists: what the glue writes through the context (the speed cut-off)
    assert {(a.owner, a.attr) for a in rows} - {(OWNER[s.split(".")[0]], s.split(".")[1]) for s in state} == {("eng", "cv_cut")}
    assert not NOT_STATE - seen                                                        # (the list above names nothing that is not there)


# ---- 4. refusals that need no context ----
def test_constructor_refusals_come_before_any_device_work(pkg):
    for make in (lambda **kw: pkg.ClosedLoop(None, None, **kw), lambda **kw: pkg.ScenarioLoop(None, None, [], **kw),
                 lambda **kw: pkg.InteractingLoop(None, None, group_sizes=[1], **kw)):
        with pytest.raises(ValueError, match="checkpoint_every needs a recorder"):
            make(checkpoint_every=5)
        for bad in (0, -3, 2.5, True, "5"):
            with pytest.raises(ValueError, match="checkpoint_every must be an integer >= 1"):
                make(checkpoint_every=bad, record=10)


def test_entry_point_refusals_without_a_context(pkg):
    lib = pkg._cabi.load()
    err = lambda: lib.jsim_last_error(None).decode()                                   # noqa: E731
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                   # noqa: E731
    ptrs = lambda *v: np.array(v, dtype=np.uint64)                                     # noqa: E731
    i32 = lambda *v: np.array(v, dtype=np.int32)                                       # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)                                       # noqa: E731
    save = lib.jsim_loop_checkpoint_save
    for n, src, dst, nbytes, msg in ((-1, ptrs(8), ptrs(16), i64(8), "n_arrays=-1"), (33, ptrs(8), ptrs(16), i64(8), "n_arrays=33 (0..32)"),
                                     (2, ptrs(8, 0), ptrs(16, 32), i64(8, 8), "array 1: null pointer"),
                                     (1, ptrs(8), ptrs(16), i64(-4), "array 0: bytes=-4"), (1, ptrs(8), ptrs(16), i64(6), "array 0: bytes=6"),
                                     (1, ptrs(10), ptrs(16), i64(8), "multiples of 4"), (1, ptrs(8), ptrs(16), i64(8), "null ctx"),
                                     (0, ptrs(8), ptrs(16), i64(8), "null ctx")):
        assert save(None, n, vp(src), vp(dst), vp(nbytes), None) == -22 and msg in err(), msg
    assert save(None, 1, None, vp(ptrs(16)), vp(i64(8)), None) == -22 and "null pointer" in err()
    load = lib.jsim_loop_checkpoint_load
    ok = dict(B=3, n_slots=2, written=i32(1, 0), n_rows=2, ego=i32(0, 2), slot=i32(0, 0), n_fields=1, slab=ptrs(64), dst=ptrs(128),
              row_bytes=i64(8), n_obs=2, obs_slab=ctypes.c_void_p(256), n_veh=1, veh_src=i32(1), veh_slot=i32(0), obs_state=ctypes.c_void_p(512))

    def call(**kw):
        a = {**ok, **kw}
        arr = lambda v: None if v is None else (v if isinstance(v, ctypes.c_void_p) else vp(v))   # noqa: E731
        return load(None, a["B"], a["n_slots"], arr(a["written"]), a["n_rows"], arr(a["ego"]), arr(a["slot"]), a["n_fields"], arr(a["slab"]),
                    arr(a["dst"]), arr(a["row_bytes"]), a["n_obs"], a["obs_slab"], a["n_veh"], arr(a["veh_src"]), arr(a["veh_slot"]),
                    a["obs_state"], None)

    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n_rows=-1), "n_rows=-1"), (dict(n_fields=33), "n_fields=33 (max 32)"), (dict(n_veh=-2), "n_veh=-2"),
                    (dict(ego=None), "null pointer"), (dict(written=None), "null pointer"), (dict(obs_state=None), "null pointer"),
                    (dict(slab=ptrs(0)), "field 0: null pointer"), (dict(row_bytes=i64(0)), "field 0: row_bytes=0"),
                    (dict(row_bytes=i64(10)), "field 0: row_bytes=10"), (dict(dst=ptrs(130)), "multiples of 4"),
                    (dict(ego=i32(0, 3)), "row 1: ego=3 outside [0, B=3)"), (dict(ego=i32(-1, 0)), "row 0: ego=-1"),
                    (dict(slot=i32(0, 1)), "row 1: slot=1 is not a written slot"), (dict(slot=i32(2, 0)), "row 0: slot=2 is not a written slot"),
                    (dict(slot=i32(-1, 0)), "row 0: slot=-1"), (dict(veh_src=i32(2)), "vehicle 0: source=2 outside [0, n_obs=2)"),
                    (dict(veh_slot=i32(1)), "vehicle 0: slot=1 is not a written slot"), ({}, "null ctx"),
                    (dict(n_rows=0, n_veh=0), "null ctx")):
        assert call(**kw) == -22 and msg in err(), msg


# ---- 5. header, binding and documentation ----
def test_header_binding_and_integration_rows(pkg):
    hdr = pkg._header.header()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    lib = pkg._cabi.load()
    for name, n_args in (("jsim_loop_checkpoint_save", 6), ("jsim_loop_checkpoint_load", 18)):
        args = [arg for _, arg in hdr.functions[name].params]
        assert len(args) == n_args == len(getattr(lib, name).argtypes), name
        assert f"`{name}`" in doc
        for arg in args:
            if arg not in ("ctx", "stream"):
                assert f"`{arg}" in doc or arg in doc.split(name, 1)[1][:3000], (name, arg)
    assert hdr.constants["JSIM_CKPT_MAX_ARRAYS"] == pkg._cabi.CKPT_MAX_ARRAYS
    assert hdr.constants["JSIM_ABI_VERSION"] == 2
    assert lib.jsim_abi_version() == 2
    # the kernels are the plan unit's: the main unit sees their declarations only
    csrc = os.path.join(REPO, pkg.__name__, "csrc")
    assert '#include "checkpoint.inc"' in open(os.path.join(csrc, "jsim_plan.hip")).read()
    inc = open(os.path.join(csrc, "checkpoint.inc")).read()
    assert inc.index("#ifndef JSIM_PLAN_TU") < inc.index("__global__ void checkpoint_copy_kernel(const CkptCopyP P);") < inc.index("#else")
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 30." in design and all(f"`{a.name}`" in design.split("## 30.", 1)[1] for a in pkg.history.CHECKPOINT)


# ---- 6. the file ----
def test_npz_round_trip(pkg, tmp_path):
    H = pkg.history
    slabs = slabs_for(pkg, 4, 5, 13, 3, seed=2)
    st = np.array([0, 25, -1, 75])
    path = str(tmp_path / "ck.npz")
    np.savez(path, **H.checkpoint_file(slabs, 25, 99, st, "ScenarioLoop"))
    back, meta = H.read_checkpoint_file(path)
    assert list(back) == [a.name for a in H.CHECKPOINT if a.name in slabs]             # the layout's order
    for k, v in slabs.items():
        assert back[k].dtype == v.dtype and np.array_equal(back[k], v), k
    assert meta["every"] == 25 and meta["cap"] == 99 and meta["kind"] == "ScenarioLoop" and np.array_equal(meta["slot_tick"], st)
    # a ClosedLoop's file: the glue's and the vehicles' arrays are not there
    few = {k: v for k, v in slabs.items() if k in ("x0", "age", "oa", "od", "tick_counter")}
    np.savez(path, **H.checkpoint_file(few, 5, 20, st, "ClosedLoop"))
    assert list(H.read_checkpoint_file(path)[0]) == ["x0", "age", "tick_counter", "oa", "od"]
    with pytest.raises(ValueError, match="not in history.CHECKPOINT"):
        H.checkpoint_file({**few, "ox": slabs["oa"]}, 5, 20, st, "ClosedLoop")
    np.savez(path, x0=slabs["x0"])
    with pytest.raises(ValueError, match="not a checkpoint file"):
        H.read_checkpoint_file(path)
    bad = H.checkpoint_file(few, 5, 20, st, "ClosedLoop")
    bad["age"] = bad["age"].astype(np.int64)
    np.savez(path, **bad)
    with pytest.raises(ValueError, match="'age' is int64"):
        H.read_checkpoint_file(path)
    bad = H.checkpoint_file(few, 5, 20, st, "ClosedLoop")
    bad["oa"] = bad["oa"][:3]
    np.savez(path, **bad)
    with pytest.raises(ValueError, match="'oa' is float64"):
        H.read_checkpoint_file(path)
