"""The build-time ISA guard (the package's isa_exec_check.py, wired into build.py): the pattern that made round 2's T = 30 build
attribute multipliers to the wrong rows -- a vector copy in a JOIN block in front of that block's exec restore -- is found in a
minimal reproduction of the failing listing, legitimate shapes (a then-block whose tail holds the merged restore, an
out-of-line then-block, a divergent loop's exit) are not flagged, and the library build() produced has no finding."""
import importlib
import os
import re

import pytest

from conftest import PKG_NAME


def _tool():
    return importlib.import_module(PKG_NAME + ".isa_exec_check")


BAD = """
_Z4kernv:                               ; @_Z4kernv
; %bb.0:
	v_mov_b32_e32 v33, 1
	s_and_saveexec_b64 s[4:5], s[6:7]
; %bb.705:                              ;   in Loop: Header=BB13_31 Depth=1
	v_accvgpr_read_b32 v30, a68
	v_and_or_b32 v0, v0, s6, v30
; %bb.706:                              ;   in Loop: Header=BB13_31 Depth=1
	v_accvgpr_write_b32 a46, v33
	v_accvgpr_write_b32 a10, v229
	s_mov_b32 s39, s70
	s_or_b64 exec, exec, s[4:5]
	v_add_f64 v[30:31], v[4:5], v[2:3]
	s_endpgm
"""
GOOD = """
_Z4kernv:                               ; @_Z4kernv
; %bb.0:
	v_cmp_lt_u32_e32 vcc, 19, v2
	s_and_saveexec_b64 s[0:1], vcc
	s_cbranch_execz .LBB13_168
.LBB13_197:                             ; then-block with the merged restore in its tail
	v_mov_b32_e32 v3, 0
	global_load_dwordx2 v[4:5], v3, s[2:3] offset:160
	s_or_b64 exec, exec, s[0:1]
	v_cmp_lt_u32_e32 vcc, 20, v2
	s_and_saveexec_b64 s[0:1], vcc
	s_cbranch_execnz .LBB13_169
.LBB13_198:                             ; join block: the restore comes first
	s_mov_b32 s39, s70
	v_readlane_b32 s8, v251, 0
	s_or_b64 exec, exec, s[0:1]
	v_mov_b32_e32 v3, 0
	s_branch .LBB13_200
.LBB13_169:                             ; out-of-line then-block, target of the execnz branch, restore duplicated into it
	v_mov_b32_e32 v3, 0
	s_or_b64 exec, exec, s[0:1]
	s_branch .LBB13_198
.LBB13_168:
	s_or_b64 exec, exec, s[0:1]
.LBB13_200:                             ; divergent loop
	v_add_u32_e32 v10, 0x200, v10
	s_andn2_b64 exec, exec, s[2:3]
	s_cbranch_execnz .LBB13_200
; %bb.694:
	s_or_b64 exec, exec, s[2:3]
	s_and_saveexec_b64 s[4:5], vcc
; %bb.1:                                ; nested: inner restore, more then-code, outer restore
	v_mov_b32_e32 v1, 0
	s_and_saveexec_b64 s[6:7], s[8:9]
; %bb.2:
	v_mov_b32_e32 v2, 0
; %bb.3:
	s_or_b64 exec, exec, s[6:7]
	v_mov_b32_e32 v3, 0
	s_or_b64 exec, exec, s[4:5]
	s_and_saveexec_b64 s[6:7], s[4:5]
	s_cbranch_execz .LBB13_389
.LBB13_382:                             ; a region with uniform control flow inside ...
	s_cmpk_lt_u32 s45, 0x1000
	s_cbranch_scc1 .LBB13_384
; %bb.383:
	global_store_dword v13, v12, s[14:15]
.LBB13_384:
	s_andn2_b64 vcc, exec, s[14:15]
	s_cbranch_vccnz .LBB13_386
; %bb.385:
	ds_write_b32 v2, v12
.LBB13_386:                             ; ... whose last block does real work and ends with the merged restore
	v_or_b32_e32 v7, s15, v7
	v_mov_b32_e32 v18, s40
	s_or_b64 exec, exec, s[6:7]
.LBB13_389:
	s_endpgm
"""
BAD_B = """
_Z5kern2v:                              ; @_Z5kern2v
; %bb.0:
	s_and_saveexec_b64 s[4:5], s[6:7]
	s_cbranch_execz .LBB1_2
; %bb.1:
	v_add_f64 v[0:1], v[0:1], v[2:3]
.LBB1_2:                                ; the skip target = the join block, with a copy in front of its restore
	v_accvgpr_write_b32 a46, v33
	s_or_b64 exec, exec, s[4:5]
	s_endpgm
"""


def test_guard_finds_the_round2_pattern_and_only_that(tmp_path):
    T = _tool()
    bad, good = tmp_path / "bad.s", tmp_path / "good.s"
    bad.write_text(BAD); good.write_text(GOOD)
    f = T.check(str(bad))
    assert len(f) == 1 and f[0][1] == "%bb.706" and [c for _, c in f[0][3]] == ["v_accvgpr_write_b32 a46, v33", "v_accvgpr_write_b32 a10, v229"]
    assert T.check(str(good)) == []
    badb = tmp_path / "bad_b.s"
    badb.write_text(BAD_B)
    fb = T.check(str(badb))
    assert len(fb) == 1 and fb[0][1] == ".LBB1_2"


def test_shipped_library_has_no_finding(pkg):
    """build() (the driver's build check, __graft_entry__.build) leaves the device listing under build/obj; the in-tree library
    was installed from there only after this check passed -- repeated here on the listing itself."""
    asm = os.path.join(pkg.build.OBJ_DIR, "jsim_mpc-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm):
        pytest.skip("no device listing (library not built in this tree: build() writes it)")
    T = _tool()
    assert T.check(asm) == []
    # the listing really is the library's: its register kernels are exactly the rows of csrc/reg_variants.h (config.REG_VARIANTS)
    want = {f"_Z20mpc_step_reg4_kernelILi{t}ELb{int(p)}EEv2KP5TickP4PreK" if w == 4 else
            f"_Z19mpc_step_reg_kernelILi{t}ELb{int(p)}ELi{e}ELb{int(h)}EEv2KP5TickP4PreK" for w, t, p, e, h in pkg.config.REG_VARIANTS}
    assert len(want) == 24
    assert {k for k in T.kernels(asm) if re.match(r"_Z\d+mpc_step_reg4?_kernel", k)} == want
    # and the guard refuses to install: a listing with the pattern raises
    bad = os.path.join(os.path.dirname(asm), "_guard_selftest.s")
    open(bad, "w").write(BAD)
    try:
        with pytest.raises(RuntimeError, match="exec restore"):
            pkg.build.check_isa(bad)
    finally:
        os.remove(bad)
