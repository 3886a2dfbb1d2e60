"""tools/isa_loop_copies.py: runs of register-to-register moves inside loops of the device listing.

J's row must keep ONE register set through the active-set loop (compiler fact 7).  Where it does not, the
bottom of the step-2 loop holds one copy per column: the tool finds that run in an excerpt of the listing of the commit before the
fix, does not flag short legitimate move sequences, and finds no run of 16 or more in any register kernel's active-set loop of the
library build() produced."""
import importlib.util
import os
import re

import pytest

from conftest import GOLDEN, REPO


def _tool():
    spec = importlib.util.spec_from_file_location("isa_loop_copies", os.path.join(REPO, "tools", "isa_loop_copies.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


EXCERPT = os.path.join(GOLDEN, "isa_T20_merge_block_two_register_sets.txt")

SHORT = """
_Z4kernv:                               ; @_Z4kernv
; %bb.0:
	v_mov_b32_e32 v1, 0
.LBB0_1:                                ; =>This Loop Header: Depth=1
	v_mov_b64_e32 v[2:3], v[4:5]
	v_mov_b64_e32 v[6:7], v[8:9]
	s_mov_b32 s4, s5
	v_mov_b32_e32 v10, v11
	v_accvgpr_read_b32 v12, a0
	v_accvgpr_write_b32 a1, v13
	v_mov_b64_e32 v[14:15], v[16:17]
	v_mov_b64_e32 v[18:19], v[20:21]
	v_add_f64 v[2:3], v[2:3], v[6:7]
	v_mov_b32_e32 v22, 0
	v_mov_b32_e32 v23, s6
	v_mov_b32_e32 v24, 0x3ff00000
	v_mov_b64_e32 v[26:27], 0
	v_mov_b32_e32 v28, s7
	v_mov_b32_e32 v29, 1.0
	v_mov_b32_dpp v30, v31 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
	v_mov_b32_e32 v32, s8
	v_mov_b32_e32 v33, s9
	s_cbranch_scc1 .LBB0_1
; %bb.2:
	v_mov_b64_e32 v[2:3], v[4:5]
	v_mov_b64_e32 v[6:7], v[8:9]
	v_mov_b64_e32 v[10:11], v[12:13]
	v_mov_b64_e32 v[14:15], v[16:17]
	v_mov_b64_e32 v[18:19], v[20:21]
	v_mov_b64_e32 v[22:23], v[24:25]
	v_mov_b64_e32 v[26:27], v[28:29]
	v_mov_b64_e32 v[30:31], v[32:33]
	v_mov_b64_e32 v[34:35], v[36:37]
	s_endpgm
"""

UNANNOTATED = """
_Z5kern2v:                              ; @_Z5kern2v
; %bb.0:
	v_mov_b32_e32 v1, 0
.LBB1_1:
	v_add_u32_e32 v1, 1, v1
; %bb.2:
	v_mov_b64_e32 v[2:3], v[4:5]
	v_mov_b64_e32 v[6:7], v[8:9]
	v_mov_b64_e32 v[10:11], v[12:13]
	s_mov_b64 s[0:1], s[2:3]
	v_mov_b64_e32 v[14:15], v[16:17]
	v_mov_b64_e32 v[18:19], v[20:21]
	v_mov_b64_e32 v[22:23], v[24:25]
	v_mov_b64_e32 v[26:27], v[28:29]
	v_mov_b64_e32 v[30:31], v[32:33]
	s_cbranch_vccnz .LBB1_1
; %bb.3:
	s_endpgm
"""


def test_tool_finds_the_forty_copies_of_the_parent_merge_block():
    """The excerpt: the merge block of `mpc_step_reg_kernel<20, false, 1, true>` one commit back, 40 v_mov_b64 of J's columns with
    four more copies of loop-carried scalars of the lane in front of them and scalar moves in between -- one run."""
    T = _tool()
    text = open(EXCERPT).read()
    assert len(re.findall(r"^\tv_mov_b64_e32 v\[\d+:\d+\], v\[\d+:\d+\]$", text, re.M)) >= 40
    found = T.scan(EXCERPT)
    assert len(found) == 1
    kernel, block, line, n, depth = found[0]
    assert kernel.startswith("_Z19mpc_step_reg_kernelILi20ELb0ELi1ELb1E") and block == ".LBB3_610" and depth == 2
    assert n == 44 and n >= 40
    assert T.scan(EXCERPT, min_run=45) == []


def test_tool_does_not_flag_short_or_non_copy_sequences(tmp_path):
    """Seven copies (scalar moves between them ignored), then an instruction, then moves of literals / SGPRs / a DPP move: nothing
    to report.  Nine copies outside any loop: not reported either.  Eight copies in a block that is in a loop only by its position
    between a label and the branch back to it (no annotation): reported, with depth 0."""
    T = _tool()
    short = tmp_path / "short.s"
    short.write_text(SHORT)
    assert T.scan(str(short)) == []
    assert [r[1:] for r in T.scan(str(short), min_run=7)] == [(".LBB0_1", 6, 7, 1)]
    un = tmp_path / "unannotated.s"
    un.write_text(UNANNOTATED)
    assert [(r[1], r[3], r[4]) for r in T.scan(str(un))] == [("%bb.2", 8, 0)]


# Register kernels knowingly left with a run of >= 16 moves inside the active-set loop: {kernel symbol: reason}.  None.
KNOWN = {}


def test_shipped_register_kernels_keep_j_in_one_register_set(pkg):
    """In the library build() produced no register kernel has a run of 16 or more register-to-register moves in a block of its
    active-set loop.  The tick loop is loop depth 1 of every register kernel, the active-set loop and all it contains depth >= 2:
    every block at depth >= 2 is held to the bound (Cholesky and the other loops of a tick with it)."""
    asm = os.path.join(pkg.build.OBJ_DIR, "jsim_mpc-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no device listing (library not built in this tree: build() writes it)")
    T = _tool()
    kernels = {k: bl for k, bl in T.blocks(asm).items() if re.match(r"_Z\d+mpc_step_reg4?_kernel", k)}
    assert len(kernels) == len(pkg.config.REG_VARIANTS) == 24
    bad = []
    for k, bl in kernels.items():
        assert max(b["depth"] for b in bl) >= 2, k      # the annotations the depth filter relies on are there
        for block, line, n, depth in T.runs(bl, 16):
            if depth >= 2 and k not in KNOWN:
                bad.append(f"{k} block {block} line {line}: {n} moves at loop depth {depth}")
    assert bad == []
