"""The time gap per recorded tick (jsim_loop_eval_gaps) without a GPU: the numpy restatement against the
reference-made fixture (tests/golden/gaps.npz: per episode the least frame_window at which the reference's own function hits) at
every tick count and window, against conflicts_numpy tick for tick, its own rows regenerated bit for bit, its vectorised form
against plain loops, the fixture's condition and events, history.gap_episodes, and the C entry point's declaration, binding and -22
list against the cross-compiled library."""
import functools
import os
import re

import numpy as np
import pytest

import conflict_cases as TC
import gap_cases as GC
import gaps_numpy as GN
from conftest import REPO


@pytest.fixture(scope="module")
def cs():
    return GC.cases()


@pytest.fixture(scope="module")
def arrays(cs):
    return GC.recorder_arrays(cs)


@pytest.fixture(scope="module")
def restated(arrays):
    """restated(window, rule, n): the restatement, made once per argument set."""
    return functools.lru_cache(maxsize=None)(lambda w, rule, n=GC.N: GC.restate(arrays, w, rule, n=n))


def test_cases_are_the_stored_ones(cs):
    g = GC.fixture()
    assert int(g["n_cases"]) == len(cs) == 47 and g["ego"].shape == (47, GC.N, 3)
    for b, c in enumerate(cs):
        assert str(g["labels"][b]) == c["label"] and bool(g["restated"][b]) == c["restated"]
        assert np.array_equal(g["ego"][b], c["ego"]) and np.array_equal(g["flags"][b], c["flags"])
        assert g["kinds"][b].tolist() == [("car", "bike").index(k) for k in c["kinds"]] + [-1] * (8 - len(c["kinds"]))
        for i, v in enumerate(c["vehicles"]):
            assert np.array_equal(g["vehicles"][b, i], v), (b, i)
    assert g["car_shape"].tolist() == list(GC.CAR) and g["bike_shape"].tolist() == list(GC.BIKE)
    assert np.flatnonzero(g["restated"]).tolist() == [41, 42, 43, 44, 45, 46]
    assert sorted({len(c["vehicles"]) for c in cs}) == [0, 1, 2, 3, 8]
    # every (tick count, case, episode) has its record: no case is left out of any comparison
    want = sum(len(GN.episodes_of(c["flags"][:n])) for c in cs for n in GC.TICK_COUNTS)
    assert len(g["records"]) == want and len({tuple(r[:3]) for r in g["records"].tolist()}) == want
    assert g["records"].dtype == np.int32 and g["records"][:, 3].min() == -1 and g["records"][:, 3].max() == 63


def test_restatement_reproduces_the_reference(cs, restated):
    """ep_gap under the episode rule: at window 63 the least frame_window at which the reference hits, at a smaller window that value
    where it fits and -1 where it does not."""
    g = GC.fixture()
    ref_made = ~g["restated"]
    seen = set()
    for n in GC.TICK_COUNTS:
        made, least = GC.expected(g, n)
        assert np.array_equal(made.sum(0), [len(GN.episodes_of(c["flags"][:n])) for c in cs])
        m = made & ref_made[None, :]
        for w in (63, 0, 1, 20, 62):
            mine = restated(w, "episode", n)
            want = np.where(least <= w, least, -1)
            assert np.array_equal(mine["ep_gap"][m], want[m]), (n, w)
            assert np.all(mine["ep_gap"][~made] == -1) and np.all(mine["ep_off"][~made] == GN.NONE), (n, w)
            assert np.all(mine["ep_tick"][~made] == -1) and np.all(mine["ep_who"][~made] == -1), (n, w)
        seen |= set(least[m].tolist())
    assert {-1, 0, 1, 2, 5, 16, 35, 62, 63} <= seen


def test_restatement_made_rows_regenerate_bit_for_bit(restated):
    g = GC.fixture()
    for n in GC.TICK_COUNTS:
        made, least = GC.expected(g, n)
        m = made & g["restated"][None, :]
        assert m.any() and np.array_equal(restated(63, "episode", n)["ep_gap"][m], least[m]), n


@pytest.mark.parametrize("which", ("gaps", "conflicts"))
def test_a_gap_within_w_is_a_contact_at_frame_window_w(which, arrays, restated):
    """Tick for tick: 0 <= gap <= w under the episode rule exactly when conflicts_numpy's frame of that tick has a touching row at
    frame_window w -- on these cases and on tests/conflict_cases.py's, whole and cut."""
    A = arrays if which == "gaps" else TC.recorder_arrays(TC.cases())
    some = 0
    for n in (GC.N, 129, 64):
        wide = restated(20, "episode", n) if which == "gaps" else GC.restate(A, 20, "episode", n=n)
        for w in (0, 1, 3, 20):
            contact = TC.restate(A, w, n=n)["row"] >= 0
            assert np.array_equal((wide["gap"] >= 0) & (wide["gap"] <= w), contact), (which, n, w)
            if n == GC.N:                                              # the window itself, not only a cut of a wider one
                assert np.array_equal(GC.restate(A, w, "episode")["gap"] >= 0, contact), (which, w)
            some += int(contact.sum())
    assert some > 1000


def test_vectorised_form_equals_plain_loops(cs):
    """Both rules, on a case of every kind: a crossing each way, the tie, the lane, eight vehicles, chunk edges, respawns, the
    spawn point, the mixed list and the mates."""
    sub = [cs[b] for b in (5, 14, 20, 23, 28, 31, 36, 39, 40, 41)] + cs[42:]
    A = GC.recorder_arrays(sub)
    for w, rule, n in ((63, "episode", 130), (63, "record", 130), (1, "episode", 66)):
        fast, slow = GC.restate(A, w, rule, n=n), GC.restate(A, w, rule, n=n, loops=True)
        for k in fast:
            assert np.array_equal(fast[k], slow[k]), (w, rule, n, k)
        assert (fast["gap"] >= 0).any()


def test_fixture_condition_holds(arrays):
    stats = {}
    GC.restate(arrays, 63, "record", stats=stats)
    assert stats["margin"] == float(GC.fixture()["margin"]) >= 1e-9


def test_fixture_meets_the_kernel_structure(cs, restated):
    """The events each case is named after are where the name says."""
    ep, rc = restated(63, "episode"), restated(63, "record")
    first = lambda r, b, k0=0: (int(r["ep_gap"][k0, b]), int(r["ep_off"][k0, b]))
    # the crossing: every least offset, the ego first (negative) and the vehicle first
    b = 0
    for g, least in zip(GC.CROSS_G, GC.CROSS_LEAST):
        for s in ((1,) if g == 0 else (1, -1)):
            assert first(ep, b) == ((least, -s * least) if least >= 0 else (-1, GN.NONE)), (g, s)
            b += 1
    assert b == 17 and first(ep, 17) == (-1, GN.NONE) and first(ep, 18) == (24, 24) and first(ep, 19) == (45, -45)
    # the tie: -9 and +9 both touch on tick 100, nothing between does
    assert ep["off"][100, 20, 0] == -9 and (ep["off"][:100, 20] == GN.NONE).all() and (ep["off"][101:, 20] == GN.NONE).all()
    assert restated(20, "episode")["off"][100, 20, 0] == -9 and (restated(1, "episode")["off"][:, 20] == GN.NONE).all()
    only_after = GC.restate(GC.recorder_arrays([dict(cs[20], vehicles=[GC.blip(GC.still(GC.FAR), GC.BESIDE, [91])])]), 63, "episode")
    assert only_after["off"][100, 0, 0] == 9
    # the lane: the leader went first, the follower comes after
    assert first(ep, 21) == (8, 8) and first(ep, 22) == (26, -26) and ep["off"][100, 23, :3].tolist() == [8, -26, GN.NONE]
    assert first(ep, 24)[0] == 0 and first(ep, 25) == (-1, GN.NONE)                      # the car's radius touches, the cyclist's does not
    assert (ep["off"][:, 26] == GN.NONE).all() and (ep["gap"][:, 26] == -1).all()       # no vehicles
    assert [int((ep["off"][:, b] != GN.NONE).any(axis=0).sum()) for b in (28, 29)] == [7, 7]   # one of the eight is more than 63 ticks away
    # chunk edges
    assert ep["off"][64, 30, :2].tolist() == [63, -63] and (ep["ep_who"][0, 30], ep["ep_tick"][0, 30]) == (0, 64)
    assert ep["off"][63, 31, :3].tolist() == [63, GN.NONE, GN.NONE] and ep["off"][64, 31, :3].tolist() == [GN.NONE, -63, GN.NONE]
    assert ep["off"][0, 32, 0] == -63 and ep["off"][199, 33, 0] == 63 and (restated(62, "episode")["gap"][:, 30:34] == -1).all()
    assert first(ep, 34) == (-1, GN.NONE)
    # ends on 62, 63, 64: the car passes behind the first episode's end -- only the record rule counts it there
    for j, k in enumerate((62, 63, 64)):
        b = 35 + j
        assert GN.episodes_of(cs[b]["flags"]) == [(0, k), (k + 1, GC.N - 1)]
        assert first(ep, b) == (-1, GN.NONE) and first(rc, b) == (15, -15) and first(ep, b, k + 1) == first(rc, b, k + 1) == (38 + j, 38 + j)
    assert GN.episodes_of(cs[38]["flags"]) == [(0, 100), (101, 101), (102, GC.N - 1)] and first(ep, 38, 101) == (0, 0)
    assert GN.episodes_of(cs[39]["flags"])[:4] == [(0, 4), (5, 6), (7, 7), (8, 10)]
    assert [first(ep, 39, k0)[0] for k0 in (0, 5, 7, 8, 11)] != [first(rc, 39, k0)[0] for k0 in (0, 5, 7, 8, 11)]
    # beside the spawn point 3 ticks before the respawn
    assert first(ep, 40, 80) == (-1, GN.NONE) and first(rc, 40, 80) == (3, 3) and rc["ep_tick"][80, 40] == 80
    # mates see each other with opposite signs
    assert first(ep, 42) == (5, -5) and first(ep, 43) == (5, 5)
    assert first(ep, 45) == (4, -4) and first(ep, 45, 100)[0] == 30


def test_gap_episodes(pkg):
    H = pkg.history
    assert (H.GAP_NONE, H.GAP_MAX_WINDOW) == (GN.NONE, GN.MAX_WINDOW)
    flags = np.zeros((6, 2), dtype=np.int32)
    flags[2, 0], flags[5, 1] = H.GOAL, H.AGE
    off = np.full((6, 2, 8), H.GAP_NONE, dtype=np.int8)
    off[0, 0, 1], off[1, 0, 0], off[1, 0, 1], off[2, 0, 1] = 7, -3, 5, -3
    off[4, 0, 2] = 0
    res = {"off": off, "ep_gap": np.full((6, 2), -1), "ep_tick": np.full((6, 2), -1), "ep_who": np.full((6, 2), -1), "ep_off": np.full((6, 2), H.GAP_NONE)}
    res["ep_gap"][0, 0], res["ep_tick"][0, 0], res["ep_who"][0, 0], res["ep_off"][0, 0] = 3, 1, 0, -3
    res["ep_gap"][3, 0], res["ep_tick"][3, 0], res["ep_who"][3, 0], res["ep_off"][3, 0] = 0, 4, 2, 0
    eps = H.gap_episodes(res, flags, 0.2)
    assert [len(e) for e in eps] == [2, 2] == [len(H.episode_bounds(flags[:, b])) for b in range(2)]
    none = (-1, None, -1)
    a, b = eps[0]
    assert a == {"gap": 3, "seconds": 3 * 0.2, "tick": 1, "vehicle": 0, "first": "ego", "per_vehicle": [(3, -3, 1), (3, -3, 2)] + [none] * 6}
    assert b == {"gap": 0, "seconds": 0.0, "tick": 4, "vehicle": 2, "first": None, "per_vehicle": [none, none, (0, 0, 4)] + [none] * 5}
    c, d = eps[1]                                                         # nothing within the window; then an episode without a tick yet
    assert c == {"gap": -1, "seconds": None, "tick": -1, "vehicle": -1, "first": None, "per_vehicle": [none] * 8} == d
    res["ep_off"][0, 0] = 3
    assert H.gap_episodes(res, flags, 0.2)[0][0]["first"] == "vehicle"
    assert all(isinstance(a[k], t) for k, t in (("gap", int), ("seconds", float), ("tick", int), ("vehicle", int)))


def test_gap_episodes_of_the_cases(pkg, cs, arrays, restated):
    r = restated(63, "episode")
    eps = pkg.history.gap_episodes(r, arrays["flags"], 0.1)
    assert [len(e) for e in eps] == [len(GN.episodes_of(c["flags"])) for c in cs]
    assert eps[23][0]["per_vehicle"][:3] == [(8, 8, 8), (26, -26, 0), (-1, None, -1)] and eps[23][0]["first"] == "vehicle"
    assert eps[22][0]["first"] == "ego" and eps[0][0]["first"] is None and eps[0][0]["seconds"] == 0.0 and eps[8][0]["seconds"] == 16 * 0.1
    for b, ep in enumerate(eps):
        for e, (k0, k1) in zip(ep, GN.episodes_of(cs[b]["flags"])):
            assert (e["gap"], e["tick"], e["vehicle"]) == (r["ep_gap"][k0, b], r["ep_tick"][k0, b], r["ep_who"][k0, b])
            have = [v[0] for v in e["per_vehicle"] if v[0] >= 0]
            assert (min(have) if have else -1) == e["gap"]


NAMES = ("rec", "flags", "n_obs", "obs_rec", "x_first", "x_spawn", "veh_range", "mate_range", "shapes", "ego_shape", "window", "within",
         "off", "ep_gap", "ep_tick", "ep_who", "ep_off")
OUTPUTS = NAMES[-5:]


def test_entry_point_is_declared_and_bound(pkg):
    hdr = open(os.path.join(REPO, "include", "jsim_mpc.h")).read()
    args = [a for _, a in pkg._header.header().functions["jsim_loop_eval_gaps"].params]
    assert args == ["ctx", "B", "n_ticks", *NAMES, "stream"]
    assert "#define JSIM_GAP_NONE (-128)" in hdr and "#define JSIM_GAP_MAX_WINDOW 63" in hdr and "#define JSIM_ABI_VERSION 2 " in hdr
    assert "main/lib/collision_avoidance.py:68-166" in hdr and "main/planner/moving_obstacle_avoidance.py:59-76" in hdr
    assert len(pkg._cabi.load().jsim_loop_eval_gaps.argtypes) == len(args) == 21
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    row = re.search(r"^\| `jsim_loop_eval_gaps` \|(.*)$", doc, flags=re.M)
    assert row and "main/lib/collision_avoidance.py:68-124" in row.group(1) and "Recorder.gaps" in row.group(1)
    assert callable(pkg.closed_loop.Recorder.gaps) and callable(pkg.closed_loop.Recorder._gaps_device) and callable(pkg.history.gap_episodes)
    csrc = os.path.join(REPO, "av-simulation-at-intersections_amd", "csrc")
    src = open(os.path.join(csrc, "jsim_mpc.hip")).read()
    assert src.index("#else /* !JSIM_KERNEL_TU") < src.index('#include "conflicts.inc"') < src.index('#include "gaps.inc"') < src.index('#include "fork.inc"')
    inc = open(os.path.join(csrc, "gaps.inc")).read()
    assert all(k in inc for k in ("jcf_list(V, b)", "jcf_vehicle_row(V, L, i)", "jcf_vehicle_pose(V, L, i, kv,", "jrw_segments(C,", "extern __shared__ double2"))
    assert "asm" not in inc and "atomic" not in inc
    assert "dx * dx + dy * dy" in inc and "d2 <= thr_sq" in inc and "\n## 23. " in open(os.path.join(REPO, "DESIGN.md")).read()


def test_argument_errors_without_gpu(pkg):
    """The header's -22 list: from the host, before any device call (there is no device here and no context to launch on)."""
    lib = pkg._cabi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data                                                 # a non-null address; no refused call reads it
    ego = np.array(GC.CAR)
    shapes = np.array([[*GC.CAR, 2.86], [*GC.BIKE, 1.0]])

    def call(B=1, n=1, ctx=None, **over):
        a = {k: p for k in NAMES}
        a.update(n_obs=2, window=20, within=0, ego_shape=ego.ctypes.data, shapes=shapes.ctypes.data)
        a.update(over)
        rc = lib.jsim_loop_eval_gaps(ctx, B, n, *[a[k] for k in NAMES], None)
        return rc, lib.jsim_last_error(None).decode()

    who = "jsim_loop_eval_gaps: "
    bad_ego = lambda **kw: np.array([kw.get("f", GC.CAR[0]), kw.get("r", GC.CAR[1]), kw.get("radius", GC.CAR[2])])
    bad_row = shapes.copy()
    bad_row[1, 2] = 0.0
    keep = [bad_ego(radius=v) for v in (0.0, -1.0, np.inf, np.nan)] + [bad_ego(f=np.nan)]
    for kw, msg in ((dict(B=-1), "B=-1"), (dict(n=-1), "n_ticks=-1"), (dict(n_obs=-3), "n_obs=-3"), (dict(obs_rec=None), "null obs_rec with n_obs=2"),
                    (dict(window=-1), "window=-1 outside [0, 63]"), (dict(window=64), "window=64 outside [0, 63]"),
                    (dict(within=2), "within=2"), (dict(within=-1), "within=-1"), (dict(ego_shape=None), "null ego_shape"),
                    (dict(ego_shape=keep[0].ctypes.data), "ego_shape: radius 0"), (dict(ego_shape=keep[1].ctypes.data), "ego_shape: radius -1"),
                    (dict(ego_shape=keep[2].ctypes.data), "ego_shape: radius inf"), (dict(ego_shape=keep[3].ctypes.data), "ego_shape: radius nan"),
                    (dict(ego_shape=keep[4].ctypes.data), "ego_shape: a circle offset"), (dict(shapes=bad_row.ctypes.data), "shapes row 1")):
        rc, err = call(**kw)
        assert rc == -22 and err.startswith(who) and msg in err, (kw, rc, err)
    for k in ("rec", "flags", "x_first", "x_spawn", "veh_range", "mate_range"):
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null device pointer", (k, rc, err)
        assert call(n=0, **{k: None})[0] == -22, k                         # also with nothing to do
    for k in OUTPUTS:
        rc, err = call(**{k: None})
        assert rc == -22 and err == who + "null output " + k, (k, rc, err)
        assert call(B=0, **{k: None})[0] == -22, k
    rc, err = call()                                                      # every argument good: the missing context is what is left
    assert rc == -22 and err == who + "null ctx"
    for kw in (dict(obs_rec=None, n_obs=0), dict(shapes=None), dict(window=0), dict(window=63), dict(within=1), dict(n=0), dict(B=0)):
        rc, err = call(**kw)                                              # none of these is an error of its own
        assert rc == -22 and err == who + "null ctx", kw
    assert not buf.any()
