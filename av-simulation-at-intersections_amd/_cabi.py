"""ctypes binding of libjsim_mpc.so, derived from include/jsim_mpc.h (_header.py reads it): the struct, every prototype and every
constant below are the header's.  Thin: pointers + sizes only.

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded this module
raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _header
from .config import MPCConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JSIM_LIB_PATH") or os.path.join(_HERE, "libjsim_mpc.so")  # JSIM_LIB_PATH: A/B runs of diagnostic builds
_H = _header.header()
_K = _H.constants
ABI_VERSION = _K["JSIM_ABI_VERSION"]
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = {"int": C.c_int, "const char *": C.c_char_p, "void": None}


class JsimCfg(C.Structure):
    _fields_ = [(f.name, _SCALARS[f.ctype] * f.length if f.length else _SCALARS[f.ctype]) for f in _H.fields]


_POINTERS = {"const jsim_cfg *": C.POINTER(JsimCfg), "jsim_ctx **": C.POINTER(C.c_void_p)}   # every other pointer: c_void_p
EXPORTS = tuple(_H.functions)
CKPT_MAX_ARRAYS = _K["JSIM_CKPT_MAX_ARRAYS"]

_lib = None


class JsimError(RuntimeError):
    pass


# per-ego status of a step / tick
STATUS_OK, STATUS_INFEASIBLE, STATUS_NEAREST_ANOMALY, STATUS_NO_PATH, STATUS_HELPER_TIMEOUT = (
    _K["JSIM_" + n] for n in ("OK", "INFEASIBLE", "NEAREST_ANOMALY", "NO_PATH", "HELPER_TIMEOUT"))
# how jsim_loop_run_interacting predicts an ego for its group mates
MATE_PREDICTION = {"constant": _K["JSIM_MATE_CONSTANT"], "plan": _K["JSIM_MATE_PLAN"]}


def check_status(status, what: str) -> None:
    """Raise on a status that is a fault of the library, not an outcome of the controller: JSIM_HELPER_TIMEOUT (a helper
    wavefront's bounded wait ran out; that ego's tick was treated like a failed solve).  `status`: host array of per-ego status."""
    bad = [int(b) for b in (status == STATUS_HELPER_TIMEOUT).nonzero()[0]]
    if bad:
        raise JsimError(f"{what}: status {STATUS_HELPER_TIMEOUT} (JSIM_HELPER_TIMEOUT) on ego(s) {bad[:8]}"
                        f"{' ..' if len(bad) > 8 else ''}: a helper wavefront gave up waiting for a column of the factor")


def load() -> C.CDLL:
    """Load the HIP library; raise if it is absent (no fallback path exists).  Every function the header declares gets its
    restype and argtypes from its declaration."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise JsimError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "The MPC path is HIP-only; there is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for f in _H.functions.values():
        fn = getattr(lib, f.name)
        fn.restype = _RETURNS[f.ret]
        fn.argtypes = [_SCALARS.get(t) or _POINTERS.get(t, C.c_void_p) for t, _ in f.params]
    if lib.jsim_abi_version() != ABI_VERSION:
        raise JsimError(f"libjsim_mpc.so ABI {lib.jsim_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def make_cfg(config: MPCConfig, T: int, dt: float, dl: float, L: float) -> JsimCfg:
    c = JsimCfg()
    c.T = int(T)
    c.max_iter = int(config.MAX_ITER)
    c.dt, c.dl, c.L = float(dt), float(dl), float(L)
    c.w_perp, c.w_para = float(config.w_perp), float(config.w_para)
    c.R[:] = [float(v) for v in config.R]
    c.Rd[:] = [float(v) for v in config.Rd]
    c.Q_v_yaw[:] = [float(v) for v in config.Q_v_yaw]
    c.Qf[:] = [float(v) for v in config.Qf]
    c.R_end[:] = [float(v) for v in config.R_END]
    c.max_dsteer = config.max_dsteer_rad
    c.max_accel = float(config.MAX_ACCEL)
    c.max_decel = float(config.MAX_DECEL)
    c.max_steer = float(config.MAX_STEER_RAD)
    c.max_speed = float(config.MAX_SPEED)
    c.min_speed = float(config.MIN_SPEED)
    c.min_ref_speed = float(config.MIN_REF_SPEED)
    c.goal_dis = float(config.GOAL_DIS)
    c.stop_speed = float(config.STOP_SPEED)
    c.nx = int(config.NX)
    c.jerk_weight = float(config.JERK_WEIGHT)
    return c


def check(rc: int, ctx=None, what: str = "jsim call") -> None:
    if rc != 0:
        msg = load().jsim_last_error(ctx)
        raise JsimError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
