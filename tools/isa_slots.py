#!/usr/bin/env python3
"""Diagnostic: issue slots that compute nothing, per kernel and loop depth, in hipcc's -S output (gfx950).

A wave that has a SIMD to itself pays about the same for every instruction it issues, whatever the class
(profiles/r01_ubench_issue_cost.txt), so the instructions that only wait, pad or form an address are counted beside the total:
  s_waitcnt     waits (the compiler puts one in front of every use of a staged LDS read)
  s_nop         hazard padding
  ds_read2_b64  two 8-byte LDS reads in one instruction: what a 16-byte read becomes once it has lost its 16-byte alignment
  ds_read_b64   8-byte LDS reads
  v_add_u32     address arithmetic (an LDS read whose offset does not fit the instruction's immediate needs one)
The counts are static: instructions in the listing, not instructions executed.  The depth is hipcc's loop annotation of the
block (0: outside every loop); in the register kernels depth 1 is the tick loop, depth >= 2 the active-set loop and what it contains.

usage: isa_slots.py [file.s] [kernel-name-substring] [--split-at s_memtime]    (default file: the listing build.py leaves in build/obj)
--split-at OP: instead of per loop depth, per stretch of the listing between two OP instructions (the phase stamps of a
-DJSIM_STAMPS build: one s_memtime each).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_loop_copies  # noqa: E402  (the listing's kernels and blocks are read once, there)

CLASSES = ("s_waitcnt", "s_nop", "ds_read2_b64", "ds_read_b64", "v_add_u32")


def _class(op):
    for c in CLASSES:
        if op == c or op.startswith(c + "_e"):   # v_add_u32_e32 / _e64
            return c
    return None


def count(path, only=None):
    """{kernel: {depth: {"total": n, class: n, ..}}} over the kernels of a listing (every depth that occurs has every key)."""
    res = {}
    for k, bl in isa_loop_copies.blocks(path).items():
        if only and only not in k:
            continue
        per = res.setdefault(k, {})
        for b in bl:
            row = per.setdefault(b["depth"], dict.fromkeys(("total",) + CLASSES, 0))
            for _, code in b["code"]:
                row["total"] += 1
                c = _class(code.split()[0])
                if c:
                    row[c] += 1
    return res


def segments(path, only=None, marker="s_memtime"):
    """{kernel: [row]}: the kernel's instructions in listing order, cut behind every `marker` instruction.  In a -DJSIM_STAMPS
    build every phase stamp is one s_memtime, so segment i is what the listing holds between stamp i - 1 and stamp i (the phases of
    a tick are straight-line code in listing order; the blocks of the active-set loop are cut at its own stamps)."""
    res = {}
    for k, bl in isa_loop_copies.blocks(path).items():
        if only and only not in k:
            continue
        rows = res.setdefault(k, [dict.fromkeys(("total",) + CLASSES, 0)])
        for b in bl:
            for _, code in b["code"]:
                op = code.split()[0]
                rows[-1]["total"] += 1
                c = _class(op)
                if c:
                    rows[-1][c] += 1
                if op == marker:
                    rows.append(dict.fromkeys(("total",) + CLASSES, 0))
    return res


def render_segments(res):
    lines = [f"{'kernel':<62} {'seg':>5} {'total':>7} " + " ".join(f"{c:>12}" for c in CLASSES)]
    for k, rows in res.items():
        for i, row in enumerate(rows):
            lines.append(f"{k:<62} {i:>5} {row['total']:>7} " + " ".join(f"{row[c]:>12}" for c in CLASSES))
    return "\n".join(lines)


def render(res):
    head = f"{'kernel':<62} {'depth':>5} {'total':>7} " + " ".join(f"{c:>12}" for c in CLASSES)
    lines = [head]
    for k in res:
        allrow = dict.fromkeys(("total",) + CLASSES, 0)
        for d in sorted(res[k]):
            row = res[k][d]
            lines.append(f"{k:<62} {d:>5} {row['total']:>7} " + " ".join(f"{row[c]:>12}" for c in CLASSES))
            for key in allrow:
                allrow[key] += row[key]
        lines.append(f"{k:<62} {'all':>5} {allrow['total']:>7} " + " ".join(f"{allrow[c]:>12}" for c in CLASSES))
    return "\n".join(lines)


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    marker = None
    if "--split-at" in argv:
        i = argv.index("--split-at")
        marker = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    path = argv[1] if len(argv) > 1 else os.path.join(here, "..", "build", "obj", "jsim_mpc-hip-amdgcn-amd-amdhsa-gfx950.s")
    only = argv[2] if len(argv) > 2 else None
    print(render_segments(segments(path, only, marker)) if marker else render(count(path, only)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
