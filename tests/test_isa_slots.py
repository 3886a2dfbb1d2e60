"""tools/isa_slots.py: waits, padding, narrowed LDS reads and address adds per kernel and loop depth of a device listing.

A short synthetic listing with one nested loop and known counts: the classes are told apart (ds_read_b64 is not ds_read2_b64 nor
ds_read_b128; v_add_u32 in both encodings, v_add_f64 not), every instruction is counted once in its block's loop depth, comments,
directives and labels are not instructions, a second kernel starts from zero, and --split-at cuts the same stream at a marker."""
import importlib.util
import os

from conftest import REPO

LISTING = """
	.text
_Z4kernv:                               ; @_Z4kernv
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	v_mov_b32_e32 v1, 0
.LBB0_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_2 Depth 2
	ds_read_b128 v[4:7], v1 offset:16
	ds_read2_b64 v[8:11], v2 offset1:1
	v_add_u32_e32 v2, 0x3608, v1
	s_waitcnt lgkmcnt(1)
	v_fma_f64 v[12:13], v[4:5], v[6:7], v[12:13]
	s_nop 0
	s_memtime s[2:3]
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
	ds_read_b64 v[14:15], v1 offset:8
	s_waitcnt lgkmcnt(0)
	v_add_f64 v[12:13], v[12:13], v[14:15]
	s_waitcnt lgkmcnt(0)
	v_add_u32_e64 v3, s0, v3
	s_nop 1
	s_nop 0
	s_cbranch_scc1 .LBB0_2
; %bb.3:                                ;   in Loop: Header=BB0_1 Depth=1
	ds_read2_b64 v[8:11], v2 offset0:2 offset1:3
	s_waitcnt lgkmcnt(0)
	s_cbranch_scc1 .LBB0_1
; %bb.4:
	s_memtime s[2:3]
	s_waitcnt vmcnt(0)
	s_endpgm
.Lfunc_end0:
	.size	_Z4kernv, .Lfunc_end0-_Z4kernv
_Z5kern2v:                              ; @_Z5kern2v
; %bb.0:
	v_add_u32_e32 v0, 1, v0
	s_endpgm
"""

KEYS = ("total", "s_waitcnt", "s_nop", "ds_read2_b64", "ds_read_b64", "v_add_u32")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_slots", os.path.join(REPO, "tools", "isa_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _row(d):
    return tuple(d[k] for k in KEYS)


def test_counts_per_kernel_and_loop_depth(tmp_path):
    T = _tool()
    assert T.CLASSES == KEYS[1:]
    f = tmp_path / "nested.s"
    f.write_text(LISTING)
    res = T.count(str(f))
    assert list(res) == ["_Z4kernv", "_Z5kern2v"]
    k = res["_Z4kernv"]
    assert sorted(k) == [0, 1, 2]
    #                     total wait nop read2 b64 add
    assert _row(k[0]) == (6, 2, 0, 0, 0, 0)       # entry block and the exit block
    assert _row(k[1]) == (10, 2, 1, 2, 0, 1)      # the outer loop's header and its latch block
    assert _row(k[2]) == (8, 2, 2, 0, 1, 1)       # the inner loop
    assert _row(res["_Z5kern2v"][0]) == (2, 0, 0, 0, 0, 1)
    assert list(T.count(str(f), "kern2")) == ["_Z5kern2v"]
    text = T.render(res)
    assert text.splitlines()[0].split() == ["kernel", "depth"] + list(KEYS)
    assert [ln.split()[1:] for ln in text.splitlines() if ln.startswith("_Z4kernv") and " all " in ln] == [["all", "24", "6", "3", "2", "1", "2"]]


def test_split_at_a_marker_instruction(tmp_path):
    T = _tool()
    f = tmp_path / "nested.s"
    f.write_text(LISTING)
    seg = T.segments(str(f), "_Z4kernv", "s_memtime")["_Z4kernv"]
    assert [_row(s) for s in seg] == [(10, 2, 1, 1, 0, 1), (12, 3, 2, 1, 1, 1), (2, 1, 0, 0, 0, 0)]
    assert sum(s["total"] for s in seg) == 24
    assert len(T.render_segments({"_Z4kernv": seg}).splitlines()) == 4
