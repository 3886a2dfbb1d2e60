"""The collision cut-off glue (jsim_pre_tick_ego, csrc/loop_pre_tick.inc) on the GPU at its chunk edges and table limits, in every place
it is compiled into: loop_pre_tick_kernel (PreTick.run with the debug buffers), group_pre_tick_kernel (the first tick of an
InteractingLoop), every PRE row of the register kernels and the LDS kernel's host ticks (ScenarioLoop), and the C-ABI's refusals.

The cases are tests/pre_tick_edge_cases.py's, the expected values tests/golden/pre_tick_edges.npz's (reference-made where the reference
can make a case, else made by the numpy restatement); the fused loops are compared tick by tick with tests/shapes_numpy.loop_pre_tick.
Nothing under the reference is read.  Every comparison is exact: the outputs are indices and copied path points, and the cases keep every
tested distance 1e-9 m from its threshold (tests/test_pre_tick_edges_cpu.py), a thousand times what the predictions are held to."""
import importlib

import numpy as np
import pytest
import torch

import loop_oracle as LO
import pre_tick_edge_cases as E
import shapes_numpy as SN
from conftest import PKG_NAME
from gpu_helpers import REG_VARIANTS, assert_state_equal, cu_count, loop_state, variant_batch, variant_id

PRE_ROWS = tuple(r for r in REG_VARIANTS if r[2])

pytestmark = pytest.mark.gpu

SENT_LEN, SENT_FLAG = 1, 7                          # what path_len / col_flag hold before a launch that must leave them alone


def assert_bits_equal(a, b, what):
    """assert_state_equal bit for bit: a NaN (the xref deviation of a tick whose solve failed) equals itself."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = (t.view(torch.int64) if t.dtype == torch.float64 else t for t in (a[k].contiguous(), b[k].contiguous()))
        if not torch.equal(x, y):
            where = torch.nonzero(x != y)
            raise AssertionError((what, k, int(where.shape[0]), where[:6].tolist(), a[k][tuple(where[0])].item(), b[k][tuple(where[0])].item()))


def pre_tick_for(pkg, paths, key, mode="truncate"):
    """(engine, PreTick, device prediction) for the launch `key` of pre_tick_edge_cases.launches() with one ego per path."""
    w, ns, obst, shapes, dl, mf = key
    kw = {}
    if mode == "speed_cutoff":
        m = importlib.import_module(PKG_NAME + ".mpc_with_speed")
        kw = dict(config=m.config, cv=[np.full(len(p), m.MAX_SPEED) for p in paths])
    eng = pkg.BatchedMPC(paths, np.arange(len(paths), dtype=np.int32), dl=dl, T=13, smooth=False, **kw)
    bikes = len(shapes) > 0 and all(s == E.BIKE for s in shapes)
    pre = pkg.PreTick(eng, frame_window=w, time_horizon=E.horizon_of(ns), margin_factor=mf, mode=mode, obstacle_dims=E.BIKE_DIMS if bikes else None)
    assert pre.n_steps == ns and pre.frame_window == w and pre.margin == mf * int(np.ceil(E.EGO_R / dl))
    mixed = len(set(shapes)) > 1
    pred = pre.predict(torch.tensor(obst, dtype=torch.float64, device=eng.device).reshape(len(obst), 6), shapes=np.array(shapes) if mixed else None)
    return eng, pre, pred


def launch(pkg, key, idxs, mode="truncate"):
    """One launch of loop_pre_tick_kernel for the cases idxs; returns per-case dicts of everything it wrote."""
    cs = [E.cases()[i] for i in idxs]
    eng, pre, pred = pre_tick_for(pkg, [c["path"] for c in cs], key, mode)
    dev, B = eng.device, len(cs)
    x0 = torch.tensor([[c["state"][0], c["state"][1], c["state"][2], c["state"][3]] for c in cs], dtype=torch.float64, device=dev)
    pre.traj_idx.copy_(torch.tensor([c["idx"] for c in cs], dtype=torch.int64))
    pre.prev_len.copy_(torch.tensor([c["prev"] for c in cs], dtype=torch.int32))
    out = eng.path_len if mode == "truncate" else pre.cut
    out.fill_(SENT_LEN)
    pre.col_flag.fill_(SENT_FLAG)
    pre.status.fill_(-7)
    dbg = {"res_idx": torch.full((B, E.MAX_RES), -1, dtype=torch.int32, device=dev), "n_res": torch.full((B,), -1, dtype=torch.int32, device=dev)}
    pre.run(x0, debug=dbg)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dict(status=pre.status, traj_idx=pre.traj_idx, path_len=out, col=pre.col_flag, first=pre.first_idx,
                                               xy=pre.col_xy, n_res=dbg["n_res"], res=dbg["res_idx"]).items()}
    return [{k: v[b] for k, v in got.items()} for b in range(B)], pred.cpu().numpy()


def check_case(c, x, g):
    """A device result g against the fixture's entry x."""
    lab = c["label"]
    assert int(g["status"]) == x["status"], (lab, g["status"])
    if x["status"] != 0:                             # a status: the ego's loop state stays as it was
        assert (int(g["traj_idx"]), int(g["path_len"]), int(g["col"])) == (c["idx"], SENT_LEN, SENT_FLAG), lab
        return 0
    assert int(g["traj_idx"]) == x["traj_idx"], (lab, g["traj_idx"])
    assert int(g["n_res"]) == x["n_res"] and np.array_equal(g["res"][:x["n_res"]], x["kept"]) and np.all(g["res"][x["n_res"]:] == -1), (lab, g["n_res"])
    assert int(g["col"]) == int(x["hit"]) and int(g["path_len"]) == x["path_len"] and int(g["first"]) == x["first_idx"], (lab, g["col"], g["path_len"], g["first"])
    if x["hit"]:
        assert tuple(float(v) for v in g["xy"]) == x["col_xy"], (lab, g["xy"])
    return int(x["hit"])


def test_loop_pre_tick_kernel_at_its_edges(pkg):
    """Every case, the cases that share (frame_window, n_steps, obstacles, shapes, dl, margin) in one launch, one ego each with its own path."""
    n_cut = n = 0
    for key, idxs in E.launches():
        got, pred = launch(pkg, key, idxs)
        for i, g in zip(idxs, got):
            c = E.cases()[i]
            n_cut += check_case(c, E.expected(i), g)
            n += 1
            if c["obst"]:
                host = np.stack(E.predictions(c))
                np.testing.assert_allclose(pred, host, rtol=0, atol=1e-12)
                if c["tie"]:                         # v = 0, yaw = 0: the prediction is exact on host and device
                    assert np.array_equal(pred.view(np.uint64), host.view(np.uint64)), c["label"]
    print(f"loop_pre_tick_kernel: {n} cases in {len(E.launches())} launches, {n_cut} cut egos")
    assert n == len(E.cases()) and n_cut >= 50


def test_speed_cutoff_mode_writes_the_same_cut(pkg):
    """The speed-cut-off glue on every sixth launch: the cut-off index goes to the controller's buffer, the path length stays full."""
    n_cut = n = 0
    for key, idxs in E.launches()[::6]:
        got, _ = launch(pkg, key, idxs, mode="speed_cutoff")
        for i, g in zip(idxs, got):
            n_cut += check_case(E.cases()[i], E.expected(i), g)
            n += 1
    print(f"loop_pre_tick_kernel, speed cut-off: {n} cases, {n_cut} cut egos")
    assert n >= 12 and n_cut >= 4


def test_all_cases_of_a_launch_in_reverse_order(pkg):
    """The launch with the most cases, reversed: an ego's answer does not depend on its place in the batch."""
    key, idxs = max(E.launches(), key=lambda kv: len(kv[1]))
    assert len(idxs) >= 5
    fwd, _ = launch(pkg, key, idxs)
    back, _ = launch(pkg, key, idxs[::-1])
    for a, b in zip(fwd, back[::-1]):
        assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("k", range(len(E.group_cases())), ids=lambda k: E.group_cases()[k]["label"].replace(" ", "-"))
def test_group_pre_tick_kernel_at_its_edges(pkg, k):
    """The group cases as the first tick of an InteractingLoop: scripted vehicles, then the group mates, gathered by the ego's wavefront."""
    g = E.group_cases()[k]
    B = len(g["paths"])
    base = len(E.cases()) + sum(len(q["paths"]) for q in E.group_cases()[:k])
    eng = pkg.BatchedMPC(g["paths"], np.arange(B, dtype=np.int32), dl=2.0, T=13, smooth=False)
    x0 = torch.from_numpy(g["x0"]).to(eng.device)
    il = pkg.InteractingLoop(eng, x0, group_sizes=g["sizes"], obstacle_specs=g["specs"], frame_window=g["w"])
    egos = E.group_ego_cases(g)
    mates = il.pred_egos().cpu().numpy()             # the mates' predictions, as the tick will make them
    for e in range(B):
        host = np.stack(E.predictions(egos[e]))[len(g["specs"]):]
        np.testing.assert_allclose(mates[[m for m in range(B) if m != e]], host, rtol=0, atol=1e-12)
    il.tick()
    torch.cuda.synchronize()
    st, idx, col, plen, age = (t.cpu().numpy() for t in (il.pre.status, il.pre.traj_idx, il.pre.col_flag, eng.path_len, il.loop.age))
    n_cut = 0
    for e in range(B):
        x = E.expected(base + e)
        assert x["digest"] == E.digest(egos[e])
        assert (int(st[e]), int(col[e]), int(plen[e])) == (x["status"], int(x["hit"]), x["path_len"]), (g["label"], e, st[e], col[e], plen[e])
        if age[e] != 0:                              # (a respawned ego's glue starts over)
            assert int(idx[e]) == x["traj_idx"], (g["label"], e)
        n_cut += int(x["hit"])
    print(f"group_pre_tick_kernel, {g['label']}: {B} egos, {n_cut} cut")
    assert n_cut >= 1


def test_refusals_leave_everything_alone(pkg):
    """-22 with a message for frame_window 33 and -1, a 9th obstacle, n_steps 0 and 65; traj_idx, path_len, col_flag, status and the
    registered prediction stay: the launch after the refusals repeats the one before them."""
    i = next(i for i, c in enumerate(E.cases()) if c["label"] == "a culled obstacle between two near ones, hit on the one after it")
    c = E.cases()[i]
    eng, pre, pred = pre_tick_for(pkg, [c["path"]], E.launch_key(c))
    x0 = torch.tensor([[c["state"][0], c["state"][1], c["state"][2], c["state"][3]]], dtype=torch.float64, device=eng.device)
    Err = pkg._cabi.JsimError

    def run():
        pre.traj_idx.fill_(c["idx"])
        pre.prev_len.fill_(c["prev"])
        pre.run(x0)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in dict(traj_idx=pre.traj_idx, path_len=eng.path_len, col=pre.col_flag, status=pre.status, first=pre.first_idx,
                                              xy=pre.col_xy).items()}

    before = run()
    assert int(before["col"]) == 1 and int(before["path_len"]) == E.expected(i)["path_len"]
    pre.prev_len.fill_(c["prev"])
    for w in (33, -1):
        pre.frame_window = w
        with pytest.raises(Err, match=r"\(-22\): \S"):
            pre.run(x0)
    pre.frame_window = c["w"]
    nine = torch.tensor([E.parked(5.0 * k, 3.0) for k in range(9)], dtype=torch.float64, device=eng.device)
    with pytest.raises(Err, match=r"\(-22\): .*n_obs=9"):
        pre.predict(nine)
    for ns in (0, 65):
        pre.n_steps = ns
        with pytest.raises(Err, match=rf"\(-22\): .*n_steps={ns}"):
            pre.predict(nine[:3].contiguous())
    pre.n_steps, pre.n_obs = c["n_steps"], len(c["obst"])
    torch.cuda.synchronize()
    now = dict(traj_idx=pre.traj_idx, path_len=eng.path_len, col=pre.col_flag, status=pre.status, first=pre.first_idx, xy=pre.col_xy)
    assert_state_equal(before, {k: v.clone() for k, v in now.items()}, "refusal")
    assert_state_equal(before, run(), "the registered prediction")


# ------------------------------------------------------------------------------------------------ the glue inside the fused loops
FUSED = ((0, 1), (1, 35), (32, 64), (32, 1))       # (frame_window, n_steps): both ends of both tables, and frame_window far above n_steps
K_TICKS = 10
LONG = 4                                            # the path of 330 points 2 m apart: more than 320 resampled points, status 4 every tick


def fused_paths():
    return [E.straight(700, 0.1), E.straight(700, 0.1, y=6.0), E.arc(700, 0.1, 40.0), E.straight(650, 0.1, x0=5.0, y=-7.0), E.straight(330, 2.0, y=40.0)]


def fused_vehicles():
    """Eight arterial vehicles (they drive straight up from x_init, y_init): parked ones on and beside the paths, slow and fast
    crossers, three of them cyclists."""
    A, bike = E.arterial, E.BIKE_DIMS
    return [A(30.0, -1.0), A(22.0, 2.6, dims=bike), A(45.0, -20.0, speed=4.0), A(15.0, -14.0, speed=2.0, dims=bike), A(38.0, 7.5),
            A(27.0, -8.5), A(55.0, -30.0, speed=8.0, dims=bike), A(60.0, 38.0)]


TEMPLATES = ((0, 0, 0.0), (0, 40, 5.0), (0, 150, E.VMAX), (1, 0, 3.0), (1, 200, 8.0), (2, 0, 2.0), (2, 100, 6.0), (3, 0, 4.0), (3, 120, 0.0),
             (LONG, 0, 0.0), (0, 250, 9.0), (2, 330, 1.0))            # (path, start index, speed)


def fused_loop(pkg, T, B, w, ns, record):
    paths = fused_paths()
    tpl = [TEMPLATES[b % len(TEMPLATES)] for b in range(B)]
    pid = np.array([t[0] for t in tpl], dtype=np.int32)
    x0 = np.array([[paths[p][i, 0], paths[p][i, 1], v, paths[p][i, 2]] for p, i, v in tpl])
    eng = pkg.BatchedMPC(paths, pid, dl=0.1, T=T, smooth=False)
    sc = pkg.ScenarioLoop(eng, torch.from_numpy(x0).to(eng.device), fused_vehicles(), hist_cap=K_TICKS, frame_window=w, record=record)
    sc.pre.n_steps = ns                              # the loops read it at run time
    return sc, paths, pid


@pytest.mark.parametrize("w,ns", FUSED)
@pytest.mark.parametrize("row", PRE_ROWS + (None,), ids=lambda r: "lds-T24" if r is None else variant_id(r))
def test_fused_loops_at_the_table_limits(pkg, row, w, ns):
    """Every PRE register kernel at its first dispatch size, and T = 24 (the LDS kernel): run(K) equals K x tick() bit for bit in loop
    state and recorder, and every host tick equals shapes_numpy.loop_pre_tick fed the tick-start state and the tick's get() tuples."""
    T, B = (24, 48) if row is None else (row[1], variant_batch(row, cu_count()))
    sc, paths, pid = fused_loop(pkg, T, B, w, ns, record=K_TICKS)
    eng = sc.loop.eng
    shapes = [tuple(r) for r in sc.shapes]
    assert len(shapes) == E.MAX_OBS and E.BIKE in shapes and E.CAR in shapes
    full_len = eng.path_len.cpu().numpy().copy()
    memo, n_cut, n_long = {}, 0, 0
    for k in range(K_TICKS):
        xs, idx_in, prev, len_in = (t.cpu().numpy().copy() for t in (sc.loop.x0, sc.pre.traj_idx, sc.pre.prev_len, eng.path_len))
        sc.tick()
        get = sc.obst.get_buf[: sc.obst.n].cpu().numpy()
        st, idx, col, plen, first, xy, age = (t.cpu().numpy() for t in (sc.pre.status, sc.pre.traj_idx, sc.pre.col_flag, eng.path_len, sc.pre.first_idx,
                                                                         sc.pre.col_xy, sc.loop.age))
        preds = [LO.predict_obstacle(*o, L=sh[3], horizon=E.horizon_of(ns)) for o, sh in zip(get, shapes)]
        for b in range(B):
            if pid[b] == LONG:                       # refused: the ego's glue state stays as it was
                assert st[b] == E.STATUS_TABLE and plen[b] == len_in[b] == full_len[b] and (age[b] == 0 or idx[b] == idx_in[b]), (k, b, st[b], plen[b])
                n_long += 1
                continue
            key = (int(pid[b]), xs[b].tobytes(), int(idx_in[b]), int(prev[b]))
            if key not in memo:
                memo[key] = SN.loop_pre_tick((xs[b, 0], xs[b, 1], xs[b, 3], xs[b, 2]), int(idx_in[b]), None if prev[b] < 0 else int(prev[b]), paths[pid[b]],
                                             [tuple(o) for o in get], 0.1, shapes, frame_window=w, preds=preds)
            r = memo[key]
            assert r[0] == 0 and st[b] == 0, (k, b, st[b])
            assert (r[2], r[3] is not None, r[4]) == (int(plen[b]), bool(col[b]), int(first[b])), (k, b, r, plen[b], col[b], first[b])
            assert r[3] is None or tuple(r[3]) == tuple(float(v) for v in xy[b]), (k, b)
            if age[b] != 0:
                assert r[1] == int(idx[b]), (k, b)
            n_cut += bool(col[b])
        memo.clear()
    torch.cuda.synchronize()
    ticks = loop_state(sc)
    fused, _, _ = fused_loop(pkg, T, B, w, ns, record=K_TICKS)
    fused.run(K_TICKS)
    torch.cuda.synchronize()
    assert_bits_equal(ticks, loop_state(fused), "run(K) against K ticks")
    print(f"{'lds-T24' if row is None else variant_id(row)}, frame_window {w}, n_steps {ns}: {B} egos x {K_TICKS} ticks, {n_cut} ego-ticks cut, {n_long} refused")
    assert n_cut >= 1 and n_long >= K_TICKS
