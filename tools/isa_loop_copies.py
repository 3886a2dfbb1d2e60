#!/usr/bin/env python3
"""Diagnostic: runs of register-to-register moves inside loops, per kernel, in hipcc's -S output (gfx950).

A long unbroken run of v_mov_b64 / v_mov_b32 / v_accvgpr_* in a loop block is how a loop-carried array that the register allocator
keeps in TWO register sets shows up: one set is read, the other written, and a merge block copies the whole array back
(compiler fact 7: the 40 v_mov_b64 of J's row at the bottom of the active-set loop at T = 20).

A move counts when it copies a vector register to a vector register (a literal, an SGPR or a DPP / SDWA source is not a copy).
Scalar moves between the vector moves (s_mov_*) do not break a run; any other instruction, a label or a branch does.
"Inside a loop": the block carries hipcc's `in Loop:` / `Loop Header` annotation, or lies between a label and a branch back to it.
The depth printed is the annotation's (0 where there is none).  In the register kernels depth 1 is the tick loop, the active-set
loop and everything inside it is depth >= 2.

usage: isa_loop_copies.py [file.s] [kernel-name-substring] [--min N]      (default file: the listing build.py leaves in build/obj)
"""
import os
import re
import sys

MIN_RUN = 8
KERNEL = re.compile(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
FALL = re.compile(r"^; (%bb\.\d+):")
LOOP_NOTE = re.compile(r"in Loop:|Loop Header")
DEPTH = re.compile(r"(?:in Loop: Header=\S+|Loop Header:) Depth=(\d+)")
REG = r"(?:[va]\d+|[va]\[\d+:\d+\])"
MOVE = re.compile(r"^(v_mov_b64|v_mov_b32|v_accvgpr_read_b32|v_accvgpr_write_b32|v_accvgpr_mov_b32)(?:_e32|_e64)?\s+" + REG + r",\s*" + REG + r"\s*$")
SCALAR_MOVE = re.compile(r"^s_mov_b(32|64)\s")


def blocks(path):
    """{kernel symbol: [block]}, block = {"label", "line", "loop" (in a loop), "depth" (hipcc's loop depth, 0: not annotated),
    "code": [(line number, instruction)]}."""
    out, cur = {}, None
    for ln, raw in enumerate(open(path), 1):
        line = raw.rstrip("\n")
        m = KERNEL.match(line)
        if m and not line.startswith("."):
            cur = out.setdefault(m.group(1), [])
            cur.append({"label": "entry", "line": ln, "loop": False, "depth": 0, "code": []})
            continue
        if cur is None:
            continue
        m = LABEL.match(line) or FALL.match(line)
        if m:
            d = DEPTH.search(line)
            cur.append({"label": m.group(1), "line": ln, "loop": bool(LOOP_NOTE.search(line)), "depth": int(d.group(1)) if d else 0, "code": []})
            continue
        if line.lstrip().startswith(";") and cur[-1]["code"] == [] and LOOP_NOTE.search(line):
            cur[-1]["loop"] = True          # the annotation continues on comment lines under the label (nested loops)
            d = DEPTH.search(line)
            if d and not cur[-1]["depth"]:  # (the first depth named is the block's own: `in Loop:` / `This Loop Header`)
                cur[-1]["depth"] = int(d.group(1))
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith("."):
            continue
        cur[-1]["code"].append((ln, code))
        if code.split()[0] == "s_endpgm":
            cur = None
    return out


def mark_back_edges(bl):
    """Blocks between a label and a later branch to it are in a loop, annotated or not."""
    at = {b["label"]: i for i, b in enumerate(bl)}
    for i, b in enumerate(bl):
        for _, c in b["code"]:
            op = c.split()
            if (op[0].startswith("s_cbranch") or op[0] == "s_branch") and len(op) > 1 and op[1] in at and at[op[1]] <= i:
                for k in range(at[op[1]], i + 1):
                    bl[k]["loop"] = True


def runs(bl, min_run=MIN_RUN):
    """[(block label, line of the first move, length, loop depth)] of every run of >= min_run moves in a loop block."""
    mark_back_edges(bl)
    res = []
    for b in bl:
        if not b["loop"]:
            continue
        n, first = 0, 0
        for ln, c in b["code"] + [(0, "end")]:
            if MOVE.match(c):
                if n == 0:
                    first = ln
                n += 1
            elif SCALAR_MOVE.match(c):
                continue
            else:
                if n >= min_run:
                    res.append((b["label"], first, n, b["depth"]))
                n = 0
    return res


def scan(path, only=None, min_run=MIN_RUN):
    """[(kernel, block label, line, length, loop depth)] over the kernels of a listing."""
    res = []
    for k, bl in blocks(path).items():
        if only and only not in k:
            continue
        res += [(k, lab, ln, n, d) for lab, ln, n, d in runs(bl, min_run)]
    return res


def main(argv):
    min_run = MIN_RUN
    if "--min" in argv:
        i = argv.index("--min")
        min_run = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    here = os.path.dirname(os.path.abspath(__file__))
    path = argv[1] if len(argv) > 1 else os.path.join(here, "..", "build", "obj", "jsim_mpc-hip-amdgcn-amd-amdhsa-gfx950.s")
    only = argv[2] if len(argv) > 2 else None
    found = scan(path, only, min_run)
    for k, lab, ln, n, d in found:
        print(f"{k:<62} block {lab:<12} depth {d} line {ln:>7}: {n} moves")
    print(f"{len(found)} run(s) of >= {min_run} register-to-register moves inside loops")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
