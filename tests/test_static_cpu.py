"""Static-obstacle clearance and contact per recorded tick (jsim_loop_eval_static) without a GPU: the numpy
restatement against the reference-made fixture (tests/golden/static.npz) at every tick count and both hidden settings, its
vectorised form against plain loops, the fixture's conditions asserted again from the stored data, the events each case is named
after, planner.static_obstacle_rows / intersection_obstacles / intersection_query against the reference-made rows,
history.static_episodes against plain loops, and the C entry point's declaration, binding and -22 list against the cross-compiled
library."""
import hashlib
import os
import re

import numpy as np
import pytest

import conflicts_numpy as CN
import static_cases as SC
import static_numpy as SN
from conftest import REPO

BAR = 1e-12


@pytest.fixture(scope="module")
def cs():
    return SC.cases()


@pytest.fixture(scope="module")
def arrays(cs):
    return SC.recorder_arrays(cs)


@pytest.fixture(scope="module")
def full(arrays):
    """The restatement of the whole run per hidden setting, with its margins."""
    out = {}
    for hidden in SC.HIDDEN:
        stats = {}
        out[hidden] = (SC.restate(arrays, SC.fixture(), hidden, stats=stats), stats)
    return out


def clear_err(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def test_cases_and_sets_are_the_stored_ones(cs):
    g = SC.fixture()
    assert int(g["n_cases"]) == len(cs) == 29 and g["ego"].shape == (29, SC.N, 3) and g["hit"].shape == (2, SC.N, 29)
    for b, c in enumerate(cs):
        assert str(g["labels"][b]) == c["label"] and bool(g["exact"][b]) == c["exact"] and int(g["set_of"][b]) == c["set"]
        assert np.array_equal(g["ego"][b], c["ego"]) and np.array_equal(g["flags"][b], c["flags"])
    assert g["car_shape"].tolist() == list(SC.CAR) and float(g["margin"]) == SC.R and g["set_names"].tolist() == list(SC.SET_NAMES)
    off, rows = g["set_off"], g["rows"]
    assert off[0] == 0 and off[-1] == len(rows) and len(off) == len(SC.SET_NAMES) + 1
    count = lambda s: (int(off[s + 1] - off[s]), int((rows[off[s]:off[s + 1], 0] == 0).sum()), int((rows[off[s]:off[s + 1], 0] == 1).sum()),
                       int(rows[off[s]:off[s + 1], 1].sum()))
    assert count(0) == (24, 16, 8, 4) and count(1)[::3] == (29, 8) and count(2)[::3] == (16, 3)
    assert [count(s)[0] for s in range(3, 9)] == [0, 1, 2, 2, 1, 1] and count(5)[3] == 2
    assert np.all(rows[rows[:, 0] == 0, 2] == 4) and np.all(rows[rows[:, 0] == 1, 2] == 8) and not rows[:, 7].any()
    assert np.flatnonzero(g["exact"]).tolist() == [0, 26, 28]


def test_restatement_reproduces_the_reference_at_every_cut(arrays, full):
    """Every (case, tick count, hidden setting): hit, who and off_tick exact, clear within the bar.  None is left out."""
    g = SC.fixture()
    compared, worst = 0, 0.0
    for hidden in SC.HIDDEN:
        for n in SC.TICK_COUNTS:
            mine = full[hidden][0] if n == SC.N else SC.restate(arrays, g, hidden, n=n)
            hit, who, clear = g["hit"][hidden, :n], g["who"][hidden, :n], g["clear"][hidden, :n]
            assert mine["hit"].shape == (n, len(g["labels"]))
            assert np.array_equal(mine["hit"], hit) and np.array_equal(mine["who"], who), (hidden, n)
            assert np.array_equal(mine["off_tick"], SC.expected_off_tick(hit, g["flags"].T)), (hidden, n)
            worst = max(worst, clear_err(mine["clear"], clear))
            compared += mine["hit"].shape[1]
    assert compared == 29 * len(SC.TICK_COUNTS) * 2 and len(SC.TICK_COUNTS) == 9
    print(f"restatement against the reference-made fixture: clear maximum error {worst:.3g}")
    assert worst <= BAR


def test_vectorised_form_equals_plain_loops(arrays):
    g = SC.fixture()
    egos = [0, 4, 6, 8, 9, 10, 17, 21, 24, 25, 26, 27, 28]
    for hidden, n in ((0, 129), (1, 70)):
        fast, slow = SC.restate(arrays, g, hidden, n=n, egos=egos), SC.restate(arrays, g, hidden, n=n, egos=egos, loops=True)
        for k in fast:
            assert np.array_equal(fast[k], slow[k], equal_nan=True), (hidden, n, k)
    # a set index outside the sets is an empty set
    args = (arrays["rec"][:5, :2], arrays["flags"][:5, :2], arrays["x_first"][:2], arrays["x_spawn"][:2])
    for f in (SN.eval_static, SN.eval_static_loops):
        out = f(*args, np.array([-1, 9]), g["set_off"], g["rows"], SC.CAR, True)
        assert np.isnan(out["clear"]).all() and all(np.all(out[k] == -1) for k in ("who", "hit", "off_tick"))


def test_fixture_conditions_hold(cs, arrays, full):
    g = SC.fixture()
    exact = g["exact"]
    for hidden in SC.HIDDEN:
        stats = full[hidden][1]
        assert np.array_equal(stats["hp_margin"], g["hp_margin"][hidden]) and np.array_equal(stats["who_margin"], g["who_margin"][hidden])
        assert (stats["hp_margin"][~exact] >= 1e-9).all() and (stats["who_margin"][~exact] >= 1e-9).all()
    # the exact cases are exact: ties of 0.0, a half-plane value of 0.0 and one of 4.4e-16
    assert g["who_margin"][0, 0] == 0.0 and g["who_margin"][0, 26] == 0.0 and g["hp_margin"][0, 28] == 0.0
    on, off = SC.exact_edge_poses()
    right = g["rows"][g["set_off"][8]][8:11]
    assert right.tolist() == [1.0, 0.0, -(1.0 + SC.R)]
    v = [float(SN.halfplane_values(right[None], p[0] + 1.0 * SC.CAR[1], 0.0)[0]) for p in (on, off)]
    assert v == [0.0, 4.440892098500626e-16] == g["edge_values"].tolist()
    # check_collision's matrix product against the unfused expression, for every stored point and obstacle of its set
    n_values = 0
    for b, c in enumerate(cs):
        s = c["set"]
        pts = np.concatenate([CN.circle_centres(c["ego"], SC.CAR[0]), CN.circle_centres(c["ego"], SC.CAR[1])]).T        # [2][2N]
        for row in g["rows"][g["set_off"][s]:g["set_off"][s + 1]]:
            hp = row[8:8 + 3 * int(row[2])].reshape(-1, 3)
            product = (hp @ np.vstack([pts, np.ones(pts.shape[1])])) <= 0
            assert np.array_equal(product, SN.halfplane_values(hp, pts[0], pts[1]) <= 0.0), (b, row[:3])
            n_values += product.size
    assert n_values == 539200


def test_fixture_meets_the_kernel_structure(cs, full):
    """The events each case is named after are where the name says (the figures are those of the issue)."""
    g = SC.fixture()
    hit, clear, who = g["hit"], g["clear"], g["who"]
    touching = lambda h, b: np.flatnonzero(hit[h, :, b] >= 0).tolist()
    # up the start lane: the pavement, obstacle 13, from x = 4.0 on; clear +0.586, +0.086, -0.414, -0.914
    assert [sorted(set(hit[0, :, b].tolist())) for b in range(4)] == [[-1], [-1], [13], [13]]
    assert np.allclose(clear[0, :, :4], [2.0 - SC.R, 1.5 - SC.R, 1.0 - SC.R, 0.5 - SC.R], rtol=0, atol=1e-12)
    assert [round(float(clear[0, 0, b]), 3) for b in range(4)] == [0.586, 0.086, -0.414, -0.914]
    assert np.all(who[0, :, 0] == 0) and np.all(who[0, :, 1:4] == 13)                          # the exact tie: the lowest index
    # the drifts: one circle only inside the pavement's inflated box
    pav = g["rows"][g["set_off"][0] + 13]
    inside = lambda b, cc: (SN.halfplane_values(pav[8:20].reshape(4, 3), *CN.circle_centres(cs[b]["ego"], cc).T) <= 0).all(axis=0)
    assert inside(4, SC.CAR[1]).any() and not inside(4, SC.CAR[0]).any() and np.array_equal(hit[0, :, 4] == 13, inside(4, SC.CAR[1]))
    assert inside(5, SC.CAR[0]).any() and not inside(5, SC.CAR[1]).any() and np.array_equal(hit[0, :, 5] == 13, inside(5, SC.CAR[0]))
    # the right turn: the corner island's octagon, touched in the middle of the turn only and with a positive clearance throughout
    t = touching(0, 6)
    assert t == list(range(t[0], t[-1] + 1)) and 0 < t[0] < 64 < 128 < t[-1] < SC.N - 1 and set(hit[0, t, 6].tolist()) == {11}
    assert clear[0, :, 6].min() > 0.38 and np.all(who[0, t, 6] == 11)
    # inside a hidden box only
    assert touching(0, 7) == [] and np.all(hit[1, :, 7] == 22) and np.all(clear[1, :, 7] == -SC.R) and np.all(who[1, :, 7] == 22)
    assert np.all(who[0, :, 7] == 0) and clear[0, :, 7].min() > 0.4
    assert touching(0, 8) != [] and set(hit[0, :, 8].tolist()) - {-1} == {12, 14} and touching(0, 9) == []
    assert np.isnan(clear[:, :, 10]).all() and np.all(who[:, :, 10] == -1) and np.all(hit[:, :, 10] == -1)      # the empty set
    assert [touching(0, b) for b in range(11, 17)] == [[k] for k in SC.EVENT_TICKS]
    # touching while clear: the box corner, the octagon at 45 and 22.5 degrees
    assert touching(0, 17) == [k for k in range(SC.N) if k not in (63, 64)] and round(float(clear[0, 0, 17]), 3) == 0.386
    assert touching(0, 27) == list(range(100)) and [round(float(clear[0, k, 27]), 3) for k in (0, 50, 100, 150)] == [0.486, 0.186, 0.686, 0.386]
    assert np.all(clear[0, :, 18] == -SC.R) and np.all(hit[0, :, 18] == 0)                     # a centre inside
    # episodes: the first touching tick of each
    off = {b: SC.expected_off_tick(hit[0], g["flags"].T)[:, b] for b in range(19, 25)}
    firsts = lambda b: {int(k): int(v) for k, v in enumerate(off[b]) if v >= 0 or k in [e[0] for e in CN.episodes_of(cs[b]["flags"])]}
    assert [firsts(b) for b in (19, 20, 21)] == [{0: 27, k + 1: k + 28} for k in (62, 63, 64)]
    assert firsts(22) == {0: -1, 1: 28} and firsts(23) == {0: 27} and cs[23]["flags"][SC.N - 1] != 0
    assert firsts(24) == {0: 0, 101: 101, 102: 102, 103: 103} and touching(0, 24) == [0, 1, 101, 102, 103, 104]
    # all hidden; the tie; the exact edge
    assert np.isnan(clear[0, :, 25]).all() and touching(0, 25) == [] and len(touching(1, 25)) == SC.N and set(hit[1, :, 25].tolist()) == {0, 1}
    assert np.all(who[0, :, 26] == 0) and np.all(clear[0, :, 26] == 2.0 - SC.R)
    assert touching(0, 28) == list(range(0, SC.N, 2))
    assert np.array_equal(full[0][0]["hit"], hit[0]) and np.array_equal(full[1][0]["hit"], hit[1])


class _Box:
    """An obstacle as the row builder sees the reference's: duck-typed."""
    def __init__(self, xy1, xy2, hidden, planes):
        self.xy1, self.xy2, self.hidden, self._planes = xy1, xy2, hidden, planes

    def to_convex(self, margin):
        assert margin == SC.R
        return self._planes


class _Circle:
    def __init__(self, radius, xy_center, hidden, planes):
        self.radius, self.xy_center, self.hidden, self._planes = radius, xy_center, hidden, planes

    def to_convex(self, margin):
        assert margin == SC.R
        return self._planes


def test_row_builder_reproduces_the_reference_made_rows(pkg):
    P = pkg.planner
    g = SC.fixture()
    rows, off = g["rows"], g["set_off"]
    prim = lambda q: ("box", (q[2], q[3]), (q[4], q[5]), bool(q[1])) if q[0] == 0 else ("circle", q[2], (q[3], q[4]), bool(q[1]))
    for s in range(len(SC.SET_NAMES)):
        mine = P.static_obstacle_rows([prim(q) for q in g["prims"][off[s]:off[s + 1]]], SC.R)
        assert mine.shape == (off[s + 1] - off[s], 32) and mine.tobytes() == rows[off[s]:off[s + 1]].tobytes(), s
        if s >= 3:
            assert P.static_obstacle_rows(SC.SYNTHETIC[s], SC.R).tobytes() == mine.tobytes(), s
    # the library's own intersection: the primitives, the rows and the query's half-planes
    prims = P.intersection_obstacles(1, 1)
    assert len(prims) == 24 and [p[3] for p in prims] == [False] * 20 + [True] * 4
    assert P.static_obstacle_rows(prims, SC.R).tobytes() == rows[:24].tobytes()
    for sp in (1, 2, 3, 4):
        q = P.intersection_query(sp, 2, SC.R)
        assert len(q.obstacles) == 24
        for hp, p in zip(q.obstacles, P.intersection_obstacles(sp, 2)):
            want = P.box_halfplanes(p[1], p[2], SC.R) if p[0] == "box" else P.circle_halfplanes(p[1], p[2], SC.R)
            assert hp.tobytes() == want.tobytes()
    for hp, row in zip(P.intersection_query(1, 1, SC.R).obstacles, rows[:24]):
        assert hp.reshape(-1).tobytes() == row[8:8 + hp.size].tobytes()
    # every one- and two-lane intersection against the digests of the rows the reference's builders made
    assert g["intersection_rows"].tolist() == [list(c) for c in SC.intersection_configs()] and len(g["intersection_rows"]) == 60
    for (nl, sp, tn, sl, gl), want in zip(SC.intersection_configs(), g["intersection_digests"]):
        mine = P.static_obstacle_rows(P.intersection_obstacles(sp, tn, sl, gl, nl), SC.R)
        assert mine.shape == (24, 32) and mine[:, 1].tolist() == [0.0] * 20 + [1.0] * 4
        assert hashlib.sha256(mine.tobytes()).hexdigest() == str(want), (nl, sp, tn, sl, gl)
    # duck-typed objects: geometry and hidden from the attributes, the half-planes from the object's own to_convex(margin)
    objs = [_Box(tuple(r[3:5]), tuple(r[5:7]), bool(r[1]), r[8:20].reshape(4, 3)) if r[0] == 0 else
            _Circle(r[5], tuple(r[3:5]), bool(r[1]), r[8:32].reshape(8, 3)) for r in rows[off[1]:off[2]]]
    assert P.static_obstacle_rows(objs, SC.R).tobytes() == rows[off[1]:off[2]].tobytes()

    class Scenario:
        obstacles = objs
    assert P.scenario_obstacles(Scenario()) == objs and P.static_obstacle_rows([], 0.0).shape == (0, 32)
    for bad in (dict(obstacles=[("cone", 1.0, (0, 0))], margin=1.0), dict(obstacles=[object()], margin=1.0),
                dict(obstacles=prims, margin=-0.1), dict(obstacles=prims, margin=np.nan), dict(obstacles=prims, margin=np.inf),
                dict(obstacles=[_Box((0, 0), (1, 1), False, np.zeros((9, 3)))], margin=SC.R)):
        with pytest.raises(ValueError):
            P.static_obstacle_rows(**bad)


def test_static_episodes_and_threshold_crossings(pkg, cs, full):
    H = pkg.history
    g = SC.fixture()
    flags = g["flags"].T
    res = full[0][0]
    eps = H.static_episodes(res, flags)
    assert len(eps) == len(cs)
    for b in range(len(cs)):
        bounds = H.episode_bounds(flags[:, b])
        assert len(eps[b]) == len(bounds)
        for ep, (k0, k1, _) in zip(eps[b], bounds):                      # plain loops
            tick, n_off, best = -1, 0, None
            for k in range(k0, k1):
                if res["hit"][k, b] >= 0:
                    n_off += 1
                    tick = k if tick < 0 else tick
                c = res["clear"][k, b]
                if c == c and (best is None or c < best[0]):
                    best = (float(c), k, int(res["who"][k, b]))
            want = {"contact": tick >= 0, "tick": tick, "obstacle": int(res["hit"][tick, b]) if tick >= 0 else -1, "ticks_off": n_off,
                    "min_clear": best[0] if best else float("nan"), "min_clear_tick": best[1] if best else -1,
                    "closest_obstacle": best[2] if best else -1}
            assert set(ep) == set(want)
            assert all(ep[k] == want[k] or (k == "min_clear" and np.isnan(ep[k]) and np.isnan(want[k])) for k in want), (b, k0, ep, want)
    assert [e["tick"] for e in eps[24]] == [0, 101, 102, 103] and [e["ticks_off"] for e in eps[24]] == [2, 1, 1, 2]
    assert len(eps[23]) == 2 and eps[23][1] == {"contact": False, "tick": -1, "obstacle": -1, "min_clear_tick": -1, "closest_obstacle": -1,
                                                "ticks_off": 0, "min_clear": eps[23][1]["min_clear"]} and np.isnan(eps[23][1]["min_clear"])
    assert eps[2][0]["obstacle"] == 13 and eps[2][0]["ticks_off"] == SC.N and isinstance(eps[2][0]["min_clear"], float)
    assert np.isnan(eps[10][0]["min_clear"]) and eps[10][0]["closest_obstacle"] == -1
    # threshold_crossings applies to clear: the drift goes off the road once
    assert H.threshold_crossings(res["clear"][:, 4], 0.0).tolist() == [int(np.flatnonzero(res["clear"][:, 4] <= 0.0)[0])]


NAMES = ("rec", "flags", "x_first", "x_spawn", "set_of", "n_sets", "set_off", "n_rows", "rows", "ego_shape", "include_hidden",
         "clear", "who", "hit", "off_tick")


def test_entry_point_is_declared_and_bound(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    args = [a for _, a in pkg._header.header().functions["jsim_loop_eval_static"].params]
    assert len(args) == 19 and args == ["ctx", "B", "n_ticks", *NAMES, "stream"]
    assert pkg._header.constant("JSIM_STATIC_ROW") == pkg.planner.STATIC_ROW == SN.ROW == 32
    for cite in ("main/lib/obstacles.py:157-176", "main/lib/mp_search_ww_generic.py:199-215", "main/lib/trajectories.py:11-55"):
        assert cite in hdr
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_eval_static.argtypes) == 19
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert re.search(r"^\| `jsim_loop_eval_static` \|", doc, flags=re.M)
    assert callable(pkg.closed_loop.Recorder.static_conflicts) and callable(pkg.history.static_episodes)
    assert callable(pkg.planner.static_obstacle_rows) and callable(pkg.planner.scenario_obstacles)
    src = open(os.path.join(REPO, "av-simulation-at-intersections_amd", "csrc", "jsim_mpc.hip")).read()
    assert '#include "static_conflicts.inc"' in src and src.index('#include "conflicts.inc"') < src.index('#include "static_conflicts.inc"')


def test_argument_errors_without_gpu(pkg):
    """The header's -22 list: from the host, before any device call (there is no device here and no context to launch on)."""
    lib = pkg._cabi.load()
    g = SC.fixture()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                 # a non-null address; no refused call reads it
    ego = np.array(SC.CAR)
    rows = np.ascontiguousarray(g["rows"][:26])                         # the intersection and, as a second set, its first two again
    rows[24:26] = rows[:2]
    off = np.array([0, 24, 24, 26], dtype=np.int32)
    keep = []

    def call(B=1, n=1, ctx=None, **over):
        a = {k: p for k in NAMES}
        a.update(n_sets=3, set_off=off.ctypes.data, n_rows=26, rows=rows.ctypes.data, ego_shape=ego.ctypes.data, include_hidden=0)
        a.update(over)
        rc = lib.jsim_loop_eval_static(ctx, B, n, *[a[k] for k in NAMES], None)
        return rc, lib.jsim_last_error(None).decode()

    def table(i, j, v):
        t = rows.copy()
        t[i, j] = v
        keep.append(t)
        return dict(rows=t.ctypes.data)

    def offsets(*v):
        keep.append(np.array(v, dtype=np.int32))
        return dict(set_off=keep[-1].ctypes.data)

    def shape(f=SC.CAR[0], r=SC.CAR[1], radius=SC.CAR[2]):
        keep.append(np.array([f, r, radius]))
        return dict(ego_shape=keep[-1].ctypes.data)

    who = "jsim_loop_eval_static: "
    bad = [(dict(B=-1), "B=-1"), (dict(n=-1), "n_ticks=-1"), (dict(n_sets=-1), "n_sets=-1"), (dict(n_rows=-2), "n_rows=-2"),
           (dict(include_hidden=2), "include_hidden=2"), (dict(include_hidden=-1), "include_hidden=-1"),
           (dict(ego_shape=None), "null ego_shape"), (dict(set_off=None), "null set_off with n_sets=3"), (dict(rows=None), "null rows"),
           (dict(rows=None, n_sets=0, set_off=None, n_rows=1), "null rows"),
           (shape(radius=0.0), "ego_shape: radius 0"), (shape(radius=-1.0), "ego_shape: radius -1"), (shape(radius=np.inf), "ego_shape: radius inf"),
           (shape(radius=np.nan), "ego_shape: radius nan"), (shape(f=np.nan), "ego_shape: a circle offset"), (shape(r=np.inf), "ego_shape: a circle offset"),
           (offsets(1, 24, 24, 26), "set_off[0]=1"), (offsets(0, 24, 23, 26), "set_off decreases at set 1"), (offsets(0, 24, 24, 25), "set_off ends at 25"),
           (dict(n_rows=27), "set_off ends at 26, not at n_rows=27"), (dict(n_sets=0, set_off=None), "set_off ends at 0, not at n_rows=26"),
           (table(3, 0, 2.0), "rows[3]: kind 2"), (table(3, 0, 0.5), "rows[3]: kind 0.5"), (table(3, 0, np.nan), "rows[3]: kind nan"),
           (table(25, 1, 2.0), "rows[25]: hidden 2"), (table(0, 1, -1.0), "rows[0]: hidden -1"),
           (table(1, 2, 0.0), "rows[1]: n_hp 0"), (table(1, 2, 9.0), "rows[1]: n_hp 9"), (table(1, 2, 2.5), "rows[1]: n_hp 2.5"), (table(1, 2, np.nan), "rows[1]: n_hp nan"),
           (table(0, 4, np.inf), "rows[0]: geometry entry 4"), (table(1, 6, np.nan), "rows[1]: geometry entry 6"),
           (table(0, 19, np.nan), "rows[0]: half-plane entry 19"), (table(1, 31, np.inf), "rows[1]: half-plane entry 31"),
           (table(1, 5, 0.0), "rows[1]: circle radius 0"), (table(1, 5, -1.0), "rows[1]: circle radius -1"),
           (table(0, 3, 1.5), "rows[0]: box with x1 > x2 or y1 > y2"), (table(0, 4, -11.0), "rows[0]: box with x1 > x2 or y1 > y2")]
    for kw, msg in bad:
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in NAMES:
        if k in ("n_sets", "set_off", "n_rows", "rows", "ego_shape", "include_hidden"):
            continue
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null device pointer", (k, rc, err)
        rc, err = call(n=0, **{k: None})                                  # also with nothing to do
        assert rc == -22, k
    rc, err = call()                                                      # every argument good: the missing context is what is left
    assert rc == -22 and err == who + "null ctx"
    good = [dict(include_hidden=1), dict(n=0), dict(B=0), dict(n_sets=0, set_off=None, rows=None, n_rows=0),
            dict(n_sets=0, n_rows=0), table(0, 20, np.nan), table(0, 7, np.nan),      # beyond a box's four half-planes; the reserved entry
            {**offsets(0, 0, 0, 0), "n_rows": 0}]                                     # three empty sets
    for kw in good:
        rc, err = call(**kw)                                              # none of these is an error of its own
        assert rc == -22 and err == who + "null ctx", (kw, err)
    assert not buf.any()
