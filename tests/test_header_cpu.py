"""include/jsim_mpc.h is the one statement of the C-ABI: the reader (_header.py) on crafted text -- every kind of
type, the layouts it must handle, the four things it refuses -- and, on the real header, the binding and the Python constants that
are derived from it.  The literal argument counts in the other *_cpu.py files are the independent check on the reader."""
import ctypes as C
import re

import pytest

CRAFTED = """
#ifndef CRAFTED_H
#define CRAFTED_H
#define JSIM_VERSION 3 /* 3: a comment behind the value */
#define JSIM_NONE (-128)
#define JSIM_WINDOW 63
#define JSIM_RATIO 0.5
typedef struct jsim_cfg {
    int32_t T;   /* horizon; 1 <= T */
    double dt, dl;
    double R[2], Qf[4]; // two arrays
    int32_t nx;
} jsim_cfg;
typedef struct jsim_ctx jsim_ctx;
enum { JSIM_OK = 0, JSIM_BAD = 1, JSIM_WORSE = 4 };
enum { JSIM_COL_A = 0, JSIM_COL_B, JSIM_COL_C, JSIM_COL_N };
enum { JSIM_FIRST, JSIM_JUMP = (7), JSIM_NEXT, JSIM_BELOW = -2, JSIM_ABOVE, };
int jsim_version(void);
const char *jsim_error(const jsim_ctx *ctx);
void jsim_destroy(jsim_ctx *ctx);
int jsim_create(const jsim_cfg *cfg, int device_id, jsim_ctx **out);
/* a declaration over three lines, with comments inside its parameter list; jsim_in_a_comment(int x) is no declaration */
int jsim_copy(jsim_ctx *ctx, int32_t n, int64_t k, double tol, size_t bytes, const void *const *src, void *const *dst,
              int8_t *off /* host, [n][4] */, const double *rows, // the rows
              void *stream);
#endif
"""


def test_reader_on_crafted_text(pkg):
    h = pkg._header.parse(CRAFTED)
    assert list(h.functions) == ["jsim_version", "jsim_error", "jsim_destroy", "jsim_create", "jsim_copy"]      # declaration order
    f = h.functions
    assert f["jsim_version"] == ("jsim_version", "int", ())                                                      # (void)
    assert f["jsim_error"] == ("jsim_error", "const char *", (("const jsim_ctx *", "ctx"),))
    assert f["jsim_destroy"] == ("jsim_destroy", "void", (("jsim_ctx *", "ctx"),))
    assert f["jsim_create"].params == (("const jsim_cfg *", "cfg"), ("int", "device_id"), ("jsim_ctx **", "out"))
    assert f["jsim_copy"].ret == "int" and f["jsim_copy"].params == (
        ("jsim_ctx *", "ctx"), ("int32_t", "n"), ("int64_t", "k"), ("double", "tol"), ("size_t", "bytes"), ("const void *const *", "src"),
        ("void *const *", "dst"), ("int8_t *", "off"), ("const double *", "rows"), ("void *", "stream"))
    assert h.fields == (("T", "int32_t", 0), ("dt", "double", 0), ("dl", "double", 0), ("R", "double", 2), ("Qf", "double", 4),
                        ("nx", "int32_t", 0))
    assert h.constants == {"JSIM_VERSION": 3, "JSIM_NONE": -128, "JSIM_WINDOW": 63,                # JSIM_RATIO, CRAFTED_H: no integers
                           "JSIM_OK": 0, "JSIM_BAD": 1, "JSIM_WORSE": 4, "JSIM_COL_A": 0, "JSIM_COL_B": 1, "JSIM_COL_C": 2, "JSIM_COL_N": 3,
                           "JSIM_FIRST": 0, "JSIM_JUMP": 7, "JSIM_NEXT": 8, "JSIM_BELOW": -2, "JSIM_ABOVE": -1}
    # one spelling of a type, however the text spaces it
    assert pkg._header.parse("int jsim_f(const double* a, jsim_ctx * * b,\n\tconst void * const *c);").functions["jsim_f"].params == (
        ("const double *", "a"), ("jsim_ctx **", "b"), ("const void *const *", "c"))


@pytest.mark.parametrize("text, offending", [
    # a line that starts a declaration of a jsim_* function and does not parse
    ("int jsim_open(int32_t n;", "int jsim_open(int32_t n;"),
    ("int jsim_body(int32_t n) { return n; }", "int jsim_body(int32_t n)"),
    ("int jsim_callback(void (*fn)(int), int32_t n);", "int jsim_callback("),
    # a return or parameter type outside the vocabulary
    ("long jsim_count(void);", "long jsim_count("),
    ("int32_t jsim_count(void);", "int32_t jsim_count("),
    ("int jsim_f(jsim_ctx *ctx, unsigned n);", "unsigned n"),
    ("int jsim_f(jsim_ctx *ctx, float x);", "float x"),
    ("int jsim_f(jsim_ctx *ctx, double);", "'double'"),
    ("int jsim_f(jsim_ctx *ctx, double xy[2]);", "double xy[2]"),
    # a struct member that is neither int32_t nor double
    ("typedef struct jsim_cfg { int32_t T; float dt; } jsim_cfg;", "float dt"),
    ("typedef struct jsim_cfg { double *p; } jsim_cfg;", "*p"),
    # an enumerator whose value is no integer literal
    ("enum { JSIM_A = 1, JSIM_B = JSIM_A + 1 };", "JSIM_B = JSIM_A + 1"),
    ("enum { JSIM_A = 1 << 2 };", "JSIM_A = 1 << 2"),
])
def test_reader_refuses_rather_than_guesses(pkg, text, offending):
    with pytest.raises(pkg._header.HeaderError, match=re.escape(offending)):
        pkg._header.parse(text)


def test_reader_stands_alone(pkg):
    src = open(pkg._header.__file__).read()
    assert not re.search(r"^\s*(from \.|import ctypes|from ctypes|import numpy|import torch)", src, re.M)
    assert pkg._header.header() is pkg._header.header()                       # read once per process
    assert pkg._header.PATH == pkg.build.INC + "/jsim_mpc.h"


def test_every_declared_function_is_in_the_library_and_bound_by_the_rule(pkg):
    h, cabi = pkg._header.header(), pkg._cabi
    # whatever is followed by `(` outside a comment is a function the reader found
    bare = re.sub(r"/\*.*?\*/", " ", open(pkg._header.PATH).read(), flags=re.S)
    assert set(re.findall(r"\b(jsim_\w+)\s*\(", bare)) == set(h.functions) == set(cabi.EXPORTS) and len(cabi.EXPORTS) == len(h.functions)
    so = C.CDLL(pkg.build.build())
    lib = cabi.load()
    scalar = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t}
    for f in h.functions.values():
        assert hasattr(so, f.name), f.name
        fn = getattr(lib, f.name)
        assert fn.restype is {"int": C.c_int, "const char *": C.c_char_p, "void": None}[f.ret], f.name
        assert len(fn.argtypes) == len(f.params), f.name
        for got, (t, name) in zip(fn.argtypes, f.params):
            want = scalar[t] if "*" not in t else (C.POINTER(cabi.JsimCfg) if t == "const jsim_cfg *" else
                                                   C.POINTER(C.c_void_p) if t == "jsim_ctx **" else C.c_void_p)
            assert got is want, (f.name, name, t)
    assert lib.jsim_abi_version() == cabi.ABI_VERSION == h.constants["JSIM_ABI_VERSION"] == 2


def test_cfg_struct_is_the_headers(pkg):
    h, cfg = pkg._header.header(), pkg._cabi.JsimCfg
    assert C.sizeof(cfg) == 8 + 8 * (3 + 2 + 2 + 2 + 2 + 4 + 2 + 3 + 3 + 1 + 2) + 8 + 8        # tests/test_host_cpu.py's sum
    assert len(h.fields) == len(cfg._fields_) == 24
    for (name, ct), f in zip(cfg._fields_, h.fields):
        base = {"int32_t": C.c_int32, "double": C.c_double}[f.ctype]
        assert name == f.name and (ct is base * f.length if f.length else ct is base), name
    assert [f.name for f in h.fields if f.length] == ["R", "Rd", "Q_v_yaw", "Qf", "R_end"]


def test_python_constants_are_the_headers(pkg):
    K, H, cabi = pkg._header.header().constants, pkg.history, pkg._cabi
    # each column tuple is as long as its enumerator says
    for cols, count in ((H.FIELDS, "JSIM_REC_FIELDS"), (H.EP_INT, "JSIM_EP_NI"), (H.EP_DOUBLE, "JSIM_EP_ND"), (H.TRK_INT, "JSIM_TRK_NI"),
                        (H.TRK_DOUBLE, "JSIM_TRK_ND"), (H.HW_INT, "JSIM_HW_NI"), (H.HW_DOUBLE, "JSIM_HW_ND"), (H.PS_INT, "JSIM_PS_NI"),
                        (H.PS_DOUBLE, "JSIM_PS_ND"), (pkg.reasons.PAR_NAMES, "JSIM_REASON_NPAR")):
        assert len(cols) == K[count], count
    assert (H.FAILED, H.GOAL, H.AGE) == (K["JSIM_REC_FAILED"], K["JSIM_REC_GOAL"], K["JSIM_REC_AGE"]) == (1, 2, 4)
    assert (H.GAP_NONE, H.GAP_MAX_WINDOW) == (K["JSIM_GAP_NONE"], K["JSIM_GAP_MAX_WINDOW"]) == (-128, 63)
    assert (H.MAX_OBS, H.MAX_PRED) == (K["JSIM_MAX_OBS"], K["JSIM_MAX_PRED"]) == (8, 64)
    assert pkg.planner.STATIC_ROW == K["JSIM_STATIC_ROW"] == 32
    assert H.CHECKPOINT_MAX_ARRAYS == cabi.CKPT_MAX_ARRAYS == K["JSIM_CKPT_MAX_ARRAYS"] == 32
    assert (cabi.STATUS_OK, cabi.STATUS_INFEASIBLE, cabi.STATUS_NEAREST_ANOMALY, cabi.STATUS_NO_PATH, cabi.STATUS_HELPER_TIMEOUT) == tuple(
        K["JSIM_" + n] for n in ("OK", "INFEASIBLE", "NEAREST_ANOMALY", "NO_PATH", "HELPER_TIMEOUT")) == (0, 1, 2, 3, 4)
    assert cabi.MATE_PREDICTION == {"constant": K["JSIM_MATE_CONSTANT"], "plan": K["JSIM_MATE_PLAN"]} == {"constant": 0, "plan": 1}
    # the two limits of the public entry points are the header's alone: the sources define neither again
    inc = open(pkg.build.SRC.replace("jsim_mpc.hip", "loop_pre_tick.inc")).read()
    assert not re.search(r"#\s*define\s+JSIM_MAX_(OBS|PRED)\b", inc) and "JSIM_MAX_OBS" in inc and "JSIM_MAX_PRED" in inc
