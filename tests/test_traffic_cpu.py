"""Traffic sets (ScenarioLoop / InteractingLoop traffic_of, jsim_loop_set_traffic) without a GPU: the host-side layout and its
refusals, the C-ABI entry against the header and the ctypes binding, the seeded workload and the sharding refusal."""
import ctypes
import os
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_SPEC = dict(direction=1, turning=False, speed=25 / 3.6, offset=2.0)


@pytest.fixture(scope="module")
def CL(pkg):
    return pkg.closed_loop


def test_traffic_layout_accepts_good_layouts(CL):
    sets = [[T_SPEC] * 2, [], [T_SPEC] * 8, [T_SPEC]]
    set_of, obs_off = CL.traffic_layout(6, sets, [0, 1, 2, 3, 0, 2])
    assert set_of.dtype == np.int32 and obs_off.dtype == np.int32
    assert set_of.tolist() == [0, 1, 2, 3, 0, 2]
    assert obs_off.tolist() == [0, 2, 2, 10, 11]
    # interacting: traffic_of per group, expanded to the egos; 1 + 3 mates and 0 + 7 mates both fit
    set_of, obs_off = CL.traffic_layout(12, sets, [3, 1], group_off=np.array([0, 4, 12]))
    assert set_of.tolist() == [3] * 4 + [1] * 8 and obs_off.tolist() == [0, 2, 2, 10, 11]
    set_of, _ = CL.traffic_layout(0, [[]], [])
    assert set_of.size == 0


@pytest.mark.parametrize("B, sets, traffic_of, group_off, what", [
    (3, [[T_SPEC]], [0, 0], None, "must hold 3"),                          # wrong length
    (3, [[T_SPEC], []], [0, 2, 1], None, "set indices"),                   # index out of range
    (2, [[T_SPEC], []], [0, -1], None, "set indices"),                     # negative index
    (2, [[T_SPEC] * 9, []], [1, 1], None, "9 vehicles"),                   # a set of 9, even unused
    (2, [[T_SPEC]], [0.0, 0.0], None, "must hold 2"),                      # not integers
    (8, [[T_SPEC] * 6, []], [0, 1], [0, 4, 8], "group mates"),             # 6 + 3 mates > 8
    (8, [[T_SPEC] * 2, []], [0], [0, 8], "group mates"),                   # 2 + 7 mates > 8
    (8, [[T_SPEC] * 2, []], [0, 1, 1], [0, 4, 8], "one per group"),        # per-ego length where groups are given
    (0, [], [], None, "at least one"),                                     # no sets
])
def test_traffic_layout_refusals(CL, B, sets, traffic_of, group_off, what):
    with pytest.raises(ValueError, match=what):
        CL.traffic_layout(B, sets, traffic_of, group_off=None if group_off is None else np.array(group_off))


def test_traffic_layout_group_limit_is_per_group(CL):
    """The limit is the set's vehicles + that group's mates: 5 + 3 and 0 + 7 fit side by side, 1 + 7 too."""
    sets = [[T_SPEC] * 5, [], [T_SPEC]]
    set_of, _ = CL.traffic_layout(20, sets, [0, 1, 2], group_off=np.array([0, 4, 12, 20]))
    assert set_of.tolist() == [0] * 4 + [1] * 8 + [2] * 8


def test_set_traffic_null_ctx_is_refused(pkg):
    lib = pkg._cabi.load()
    set_of = np.zeros(4, dtype=np.int32)
    obs_off = np.array([0, 2], dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    assert lib.jsim_loop_set_traffic(None, 4, 1, p(set_of), p(obs_off), 0) == -22
    assert b"null ctx" in lib.jsim_last_error(None)
    assert lib.jsim_loop_set_traffic(None, 0, 0, None, None, 0) == -22


def test_set_traffic_is_declared_exported_and_documented(pkg):
    assert len(pkg._header.header().functions["jsim_loop_set_traffic"].params) == 6
    lib = pkg._cabi.load()
    assert len(lib.jsim_loop_set_traffic.argtypes) == 6 and lib.jsim_loop_set_traffic.restype is ctypes.c_int
    assert "`jsim_loop_set_traffic`" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert pkg._cabi.load().jsim_abi_version() == 2


def test_traffic_batch_is_seeded_and_reference_like(pkg):
    W = pkg.workloads
    sets, tof = W.traffic_batch(512, seed=4)
    sets2, tof2 = W.traffic_batch(512, seed=4)
    assert sets == sets2 and np.array_equal(tof, tof2) and np.array_equal(tof, np.arange(512))
    kinds = {s.get("kind", "t_intersection") for st in sets for s in st}
    assert kinds == {"t_intersection", "roundabout"}
    assert any(len(st) == 0 for st in sets) and max(len(st) for st in sets) <= 8
    for st in sets:
        for s in st:
            assert s["direction"] in (1, -1) and s["offset"] is not None
            if s.get("kind", "t_intersection") == "t_intersection":
                assert 0.5 <= s["offset"] <= 5.0 and 20 / 3.6 <= s["speed"] <= 30 / 3.6
    assert {s["turning"] for st in sets for s in st} == {True, False}
    sets3, tof3 = W.traffic_batch(100, seed=1, n_sets=7)
    assert len(sets3) == 7 and tof3.shape == (100,) and tof3.min() >= 0 and tof3.max() < 7
    pkg.closed_loop.traffic_layout(100, sets3, tof3)          # a valid layout as it comes


def test_cabi_gather_refuses_a_traffic_layout_across_ranks(pkg):
    eng = types.SimpleNamespace(traffic_layout=(np.zeros(4, np.int32), np.array([0, 1], np.int32)), lib=None, _ctx=None)
    with pytest.raises(ValueError, match="not sharded"):
        pkg.sharding.CabiGather(eng, rank=0, world=2, unique_id=bytes(128))
