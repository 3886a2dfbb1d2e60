"""The edge cases of the collision cut-off glue (tests/pre_tick_edge_cases.py) on the CPU: the restatement equals the fixture
tests/golden/pre_tick_edges.npz exactly on every case, every case is what its label says, its inputs keep the 1e-9 m margin, and each
of a list of deliberately wrong variants of the restatement -- the mistakes the kernel's structure invites -- disagrees with the fixture
on at least one case in what the device returns.  No GPU, no kernel is touched."""
import numpy as np
import pytest

import loop_oracle as LO
import pre_tick_edge_cases as E
import shapes_numpy as SN

OUT = ("status", "traj_idx", "n_res", "hit", "first_idx", "col_xy", "path_len")        # what the device returns, besides the kept indices


def same_outputs(r, x):
    plen = -1 if r["path_len"] is None else r["path_len"]
    return all(r[k] == x[k] for k in OUT if k != "path_len") and plen == x["path_len"] and np.array_equal(r["kept"], x["kept"])


def test_fixture_is_of_these_cases():
    g, cases = E.fixture(), E.cases()
    n_group = sum(len(q["paths"]) for q in E.group_cases())
    assert int(g["n_cases"]) == len(cases) and len(g["status"]) == len(cases) + n_group
    for i, c in enumerate(cases):
        x = E.expected(i)
        assert x["digest"] == E.digest(c) and str(g["label"][i]) == c["label"], c["label"]
        assert x["ref_made"] == E.reference_made(c, E.restated()[i]), c["label"]
    made = int(g["ref_made"][:len(cases)].sum())
    print(f"{len(cases)} cases, {made} reference-made, {len(cases) - made} restatement-made; {n_group} egos in {len(E.group_cases())} interacting groups")
    assert made >= 80
    assert g["n_res"].max() > E.MAX_RES and (g["n_res"] == E.MAX_RES).any() and {0, 2, E.STATUS_TABLE} <= set(g["status"].tolist())


def test_restatement_equals_the_fixture():
    """pre_tick_edge_cases.run, shapes_numpy.loop_pre_tick, first_collision (nested loops) and first_collision_fast on every case."""
    for i, (c, r) in enumerate(zip(E.cases(), E.restated())):
        x = E.expected(i)
        assert same_outputs(r, x), (c["label"], r, x)
        assert (r["row"] if r["row"] is not None else (-1,) * 5) == x["row"], c["label"]
        if r["status"] == E.STATUS_TABLE:
            continue
        x_, y_, v_, yaw_ = c["state"]
        preds = E.predictions(c)
        st, idx, plen, xy, first, o = SN.loop_pre_tick((x_, y_, yaw_, v_), c["idx"], None if c["prev"] < 0 else c["prev"], c["path"], c["obst"], c["dl"],
                                                       c["shapes"], margin_factor=c["margin_factor"], frame_window=c["w"], preds=preds)
        assert st == x["status"], c["label"]
        if st != 0:
            continue
        assert (idx, plen, xy is not None, first) == (x["traj_idx"], x["path_len"], x["hit"], x["first_idx"]), c["label"]
        assert xy is None or (tuple(xy) == x["col_xy"] and o == x["row"][2]), c["label"]
        detailed = c["path"][idx:]
        res = detailed[x["kept"]]
        assert np.array_equal(np.flatnonzero(LO.resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), v_))), x["kept"]), c["label"]
        for fn in (SN.first_collision, SN.first_collision_fast):
            col = fn(res, detailed, preds, c["shapes"], frame_window=c["w"])
            assert (col is not None) == x["hit"] and (col is None or (col[:2] == x["col_xy"] and col[2:] == (x["first_idx"], x["row"][2]))), (c["label"], fn.__name__)


def test_every_case_is_what_its_label_says():
    Rs = []
    for c, r in zip(E.cases(), E.restated()):
        want = dict(c["want"])
        for k in ("n_res", "status", "hit", "row", "R", "culled", "first_idx", "path_len", "traj_idx", "sample"):
            if k in want:
                assert r[k] == want.pop(k), (c["label"], k, r[k])
        if "frame" in want:
            assert r["row"][0] == want.pop("frame"), c["label"]
        if "clamp" in want:
            margin = c["margin_factor"] * int(np.ceil(E.EGO_R / c["dl"]))
            cidx = int(np.argmax(np.hypot(c["path"][:, 0] - r["col_xy"][0], c["path"][:, 1] - r["col_xy"][1]) <= 0.001))
            assert r["hit"] and (r["path_len"] == r["traj_idx"] + 1) == want["clamp"] == (cidx - margin < r["traj_idx"] + 1), c["label"]
            want.pop("clamp")
        if want.pop("second_lap", False):
            lap = len(c["path"]) // 2
            assert r["traj_idx"] >= lap and np.array_equal(c["path"][r["traj_idx"] + r["first_idx"]], c["path"][r["traj_idx"] + r["first_idx"] - lap]), c["label"]
            assert E.run(c, ("mm_search_from_idx",))["path_len"] > r["path_len"], c["label"]
        for k in want.pop("keeps", ()):
            assert k in r["kept"], (c["label"], k)
        for k in want.pop("drops", ()):
            assert k not in r["kept"], (c["label"], k)
        if want.pop("order_sensitive", False):
            detailed = c["path"][r["traj_idx"]:]
            tree = E.resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), c["state"][2]), ("tree_cumsum",))
            diff = np.setxor1d(np.flatnonzero(tree), r["kept"])
            assert 1 <= len(diff), c["label"]
        assert not want, (c["label"], want)
        if c["obst"] and r["status"] == 0:
            Rs.append(r["R"])
        # the cull, restated here once more: the bounding circles of the ego's and the obstacle's circle centres stay apart
        if c["obst"] and r["status"] == 0:
            res = c["path"][r["traj_idx"]:][r["kept"]]
            for o, (p, sh) in enumerate(zip(E.predictions(c), c["shapes"])):
                e = np.concatenate([LO.circle_centres(res, xo) for xo in E.EGO_OFFS])
                q = np.concatenate([LO.circle_centres(p, xo) for xo in sh[:2]])
                gap = np.min(np.hypot(e[:, None, 0] - q[None, :, 0], e[:, None, 1] - q[None, :, 1]))
                assert (o not in r["culled"]) or gap > E.EGO_R + sh[2], (c["label"], o)
    assert min(Rs) < 64 and any(64 < R < 128 for R in Rs) and max(Rs) > 2000
    assert {0, 1, 2, 10, 15, 16, 31, 32} <= {c["w"] for c in E.cases()} and {1, 2, 35, 63, 64} <= {c["n_steps"] for c in E.cases()}
    assert {1, 2, 5, 8} <= {len(c["obst"]) for c in E.cases()}
    # the group cases: who is hit, who also touches in that frame, who is near but does not touch
    for g in E.group_cases():
        egos = E.group_ego_cases(g)
        for e, o in g.get("hit_o", {}).items():
            assert E.run(egos[e])["row"][2] == o, (g["label"], e)
        for e, o in g.get("also", {}).items():
            r = E.run(egos[e])
            res = egos[e]["path"][r["traj_idx"]:][r["kept"]]
            touch = E.pair_table(res, E.predictions(egos[e]), egos[e]["shapes"], egos[e]["w"])[1]
            assert touch[r["row"][0], :, o].any() and o > r["row"][2], (g["label"], e)
        for e, o in g.get("near", {}).items():
            r = E.run(egos[e])
            assert o not in r["culled"] and egos[e]["shapes"][o] == E.BIKE and r["row"][2] != o, (g["label"], e)


def test_inputs_keep_their_margin():
    """Every tested pair distance and every path-point distance of a case that is no exact tie is at least 1e-9 m from its threshold:
    device and host sin / cos differ by ulps (the predictions are held to 1e-12), so every comparison may be exact."""
    least = np.inf
    for c, r in zip(E.cases(), E.restated()):
        if not c["tie"]:
            assert r["margin"] >= E.MARGIN, (c["label"], r["margin"])
            least = min(least, r["margin"])
    for g in E.group_cases():
        for c in E.group_ego_cases(g):
            assert E.run(c)["margin"] >= E.MARGIN, c["label"]
    ties = [c for c in E.cases() if c["tie"]]
    assert len(ties) == 4
    for c in ties:                                                  # the tie is exact: the pair's squared distance IS the threshold's double (or the next)
        sh = c["shapes"][0]
        d2 = E.pair_table(c["path"], E.predictions(c), c["shapes"], 0)[0][0, 1, 0, 0, 0]
        t = E.sqrt_threshold(E.EGO_R + sh[2])
        assert d2 == (t if c["want"]["hit"] else np.nextafter(t, np.inf)), c["label"]
    print(f"smallest margin of the cases that are no tie: {least:.3e} m")


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_a_wrong_variant_is_caught(mutant):
    flipped = [c["label"] for i, c in enumerate(E.cases()) if not same_outputs(E.run(c, (mutant,)), E.expected(i))]
    print(f"{mutant}: disagrees with the fixture on {len(flipped)} cases")
    assert len(flipped) >= 1
