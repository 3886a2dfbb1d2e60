"""Reader of include/jsim_mpc.h, the one statement of the C-ABI: its functions, jsim_cfg's fields and its integer constants.

Pure Python: no library load and nothing else of the package, so history.py, tests and tools can use it without the .so.  The
header is regular (clang-formatted declarations, one closed vocabulary of types); the reader handles that and refuses everything
else with the offending text -- it never guesses.
"""
from __future__ import annotations

import functools
import os
import re
from typing import NamedTuple

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsim_mpc.h")

RETURNS = ("int", "void", "const char *")
SCALARS = ("int", "int32_t", "int64_t", "double", "size_t")
_POINTER = re.compile(r"(?:const )?\w+ (?:\*+(?:const )?)*\*+")                    # `const void *const *`, `jsim_ctx **`, `int8_t *`
_DECL_HEAD = re.compile(r"^[ \t]*([A-Za-z_][\w \t*]*?)[ \t]*\b(jsim_\w+)[ \t]*\(", re.M)
_DECL_TAIL = re.compile(r"([^;{}()]*)\)\s*;")


class HeaderError(ValueError):
    pass


class Function(NamedTuple):
    name: str
    ret: str
    params: tuple          # ((C type text, name), ...), () for (void)


class Field(NamedTuple):
    name: str
    ctype: str             # int32_t or double
    length: int            # 0: a scalar


class Header(NamedTuple):
    functions: dict        # name -> Function, in declaration order
    fields: tuple          # jsim_cfg's Fields, in order
    constants: dict        # JSIM_* #defines with an integer value and every enumerator


def _ctype(text: str) -> str:
    """A type's text in one spelling: single spaces, each run of stars after one space (`double*x` and `double * x` alike)."""
    return re.sub(r"(\*+)", r" \1", re.sub(r"\s*\*\s*", "*", " ".join(text.split())))


def _param(text: str, where: str):
    m = re.fullmatch(r"(.*?)(\w+)", " ".join(text.split()))
    ctype = _ctype(m.group(1)) if m else ""
    if ctype not in SCALARS and not _POINTER.fullmatch(ctype):
        raise HeaderError(f"{where}: parameter {text.strip()!r} is no `<type> <name>` of a type the binding knows")
    return ctype, m.group(2)


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" if "\n" in m.group() else " ", text, flags=re.S)
    functions = {}
    for m in _DECL_HEAD.finditer(text):
        ret, name = _ctype(m.group(1)), m.group(2)
        tail = _DECL_TAIL.match(text, m.end())
        if ret not in RETURNS or not tail:
            raise HeaderError(f"not a declaration the reader knows: {text[m.start():].split(chr(10), 1)[0].strip()!r}")
        params = " ".join(tail.group(1).split())
        functions[name] = Function(name, ret, () if params in ("", "void") else tuple(_param(p, name) for p in params.split(",")))
    fields = []
    body = re.search(r"typedef\s+struct\s+jsim_cfg\s*\{(.*?)\}\s*jsim_cfg\s*;", text, re.S)
    for member in filter(None, (s.strip() for s in body.group(1).split(";"))) if body else ():
        m = re.fullmatch(r"(int32_t|double)\s+(.*)", member, re.S)
        if not m:
            raise HeaderError(f"jsim_cfg: member {member!r} is neither int32_t nor double")
        for d in m.group(2).split(","):
            dm = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
            if not dm:
                raise HeaderError(f"jsim_cfg: declarator {d.strip()!r} of {member!r}")
            fields.append(Field(dm.group(1), m.group(1), int(dm.group(2) or 0)))
    constants = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(JSIM_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    for enum in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        value = -1
        for item in filter(None, (s.strip() for s in enum.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*\(?(-?\d+)\)?)?", item)
            if not m:
                raise HeaderError(f"enumerator {item!r}: its value is no integer literal")
            value = int(m.group(2)) if m.group(2) else value + 1
            constants[m.group(1)] = value
    return Header(functions, tuple(fields), constants)


@functools.lru_cache(maxsize=None)
def header() -> Header:
    """include/jsim_mpc.h, read once per process."""
    with open(PATH) as f:
        return parse(f.read())


def constant(name: str) -> int:
    return header().constants[name]
