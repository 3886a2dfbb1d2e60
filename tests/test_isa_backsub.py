"""The device listing build() leaves behind: in every one-wave register kernel the back substitution's columns below 16 are sixteen
fused FMAs on the 64-bit row broadcast (csrc/mpc_step_reg.inc, bs_step2) inside the active-set loop,
in the order 15 .. 0, with no v_readlane_b32 among them, their hazard padding in place, and at most one uniform branch in front;
no register kernel has scratch; the ISA guard has no finding and every row of the variant table is there."""
import importlib.util
import os
import re

import pytest

from conftest import REPO

STEP = re.compile(r"^v_fmac_f64_dpp (v\[\d+:\d+\]), (v\[\d+:\d+\]), v\[\d+:\d+\] row_newbcast:(\d+) row_mask:0xf bank_mask:0xf$")
ONE_WAVE = re.compile(r"^_Z19mpc_step_reg_kernelILi(\d+)ELb([01])ELi([12])ELb([01])E")
REG_KERNEL = re.compile(r"^_Z\d+mpc_step_reg4?_kernel")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(pkg):
    path = os.path.join(pkg.build.OBJ_DIR, "jsim_mpc-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(path):
        pytest.skip("no device listing (library not built in this tree: build() writes it)")
    return path


@pytest.fixture(scope="module")
def kernels(asm):
    return {k: bl for k, bl in _tool("isa_loop_copies").blocks(asm).items() if REG_KERNEL.match(k)}


def _valu(op):
    return op.startswith("v_") and not op.startswith("v_readlane") and not op.startswith("v_readfirstlane")


def test_sixteen_row_broadcast_steps_and_one_branch_in_every_one_wave_kernel(pkg, kernels):
    one_wave = {k: bl for k, bl in kernels.items() if ONE_WAVE.match(k)}
    rows = {(1, int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(4) == "1") for m in map(ONE_WAVE.match, one_wave)}
    assert rows == {r for r in pkg.config.REG_VARIANTS if r[0] == 1} and len(one_wave) == 20
    for k, bl in one_wave.items():
        flat = [(i, ln, c) for i, b in enumerate(bl) for ln, c in b["code"]]
        steps = [(n, i, STEP.match(c)) for n, (i, ln, c) in enumerate(flat) if c.startswith("v_fmac_f64_dpp")]
        assert all(m for _, _, m in steps), k
        assert [int(m.group(3)) for _, _, m in steps] == list(range(15, -1, -1)), k            # 2T >= 26 columns: never fewer than 16
        assert len({m.group(1) for _, _, m in steps}) == 1 and all(m.group(1) == m.group(2) for _, _, m in steps), k   # one running value
        first, last = steps[0][0], steps[-1][0]
        assert all(bl[i]["depth"] >= 2 for _, i, _ in steps), k                                # inside the active-set loop
        between = [c.split()[0] for _, _, c in flat[first:last + 1]]
        assert not any(op.startswith("v_readlane") for op in between), k
        assert not any(op.startswith("s_cbranch") or op == "s_branch" for op in between), k
        # the hazard: no DPP read of the running value in the two slots behind the vector instruction that wrote it
        run = steps[0][2].group(1)
        for n, _, _ in steps:
            slots = 0                                    # issue slots between the last vector write of the running value and the step
            for _, _, c in reversed(flat[:n]):
                op = c.split()
                if op[0] == "s_nop":
                    slots += int(op[1]) + 1
                elif _valu(op[0]) and len(op) > 1 and op[1].rstrip(",") == run:
                    pytest.fail(f"{k}: {c!r} writes {run} {slots} slot(s) in front of {flat[n][2]!r}")
                else:
                    slots += 1
                if slots >= 2:
                    break
        # at most one uniform branch in front: nothing branches inside the steps' block ahead of them, and at most one branch
        # (the q > 16 test that skips the columns from 16 on) enters it
        b0 = bl[steps[0][1]]
        head = [c.split()[0] for ln, c in b0["code"] if ln < flat[first][1]]
        assert not any(op.startswith("s_cbranch") or op == "s_branch" for op in head), k
        entering = [(n, c) for n, (_, _, c) in enumerate(flat) if c.split()[0].startswith(("s_cbranch", "s_branch")) and c.split()[1] == b0["label"]]
        assert len(entering) <= 1, (k, entering)
        for n, c in entering:
            cmp_ = next(x[2] for x in reversed(flat[:n]) if x[2].startswith("s_cmp_"))        # (the scheduler may put work between)
            assert c.startswith("s_cbranch_scc") and cmp_.split()[-1] in ("16", "17"), (k, cmp_, c)


def test_no_register_kernel_has_scratch_and_none_is_missing(pkg, asm, kernels):
    assert len(kernels) == len(pkg.config.REG_VARIANTS) == 24
    text = open(asm).read()
    for k in kernels:
        m = re.search(r"\.amdhsa_kernel " + re.escape(k) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
        assert m, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1) == "0", k
        assert re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", m.group(1)).group(1) == "0", k


def test_isa_guard_has_no_finding(asm):
    assert _tool("isa_exec_check").check(asm) == []
