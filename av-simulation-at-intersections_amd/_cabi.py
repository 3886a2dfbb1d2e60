"""ctypes binding of libjsim_mpc.so (include/jsim_mpc.h).  Thin: pointers + sizes only.

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded this module
raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

from .config import MPCConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JSIM_LIB_PATH") or os.path.join(_HERE, "libjsim_mpc.so")  # JSIM_LIB_PATH: A/B runs of diagnostic builds
ABI_VERSION = 2


class JsimCfg(C.Structure):
    _fields_ = [
        ("T", C.c_int32), ("max_iter", C.c_int32),
        ("dt", C.c_double), ("dl", C.c_double), ("L", C.c_double),
        ("w_perp", C.c_double), ("w_para", C.c_double),
        ("R", C.c_double * 2), ("Rd", C.c_double * 2), ("Q_v_yaw", C.c_double * 2),
        ("Qf", C.c_double * 4), ("R_end", C.c_double * 2),
        ("max_dsteer", C.c_double), ("max_accel", C.c_double), ("max_decel", C.c_double),
        ("max_steer", C.c_double), ("max_speed", C.c_double), ("min_speed", C.c_double),
        ("min_ref_speed", C.c_double), ("goal_dis", C.c_double), ("stop_speed", C.c_double),
        ("nx", C.c_int32), ("reserved_", C.c_int32), ("jerk_weight", C.c_double),
    ]


EXPORTS = (
    "jsim_abi_version", "jsim_last_error", "jsim_mpc_create", "jsim_mpc_destroy", "jsim_mpc_set_paths",
    "jsim_mpc_step", "jsim_mpc_step_debug", "jsim_plant_step", "jsim_loop_advance", "jsim_mpc_run_ticks", "jsim_mpc_set_launch_order", "jsim_mpc_get_launch_order", "jsim_mpc_iter_totals",
    "jsim_loop_set_geometry", "jsim_loop_set_obstacle_geometry", "jsim_loop_predict_obstacles", "jsim_loop_pre_tick",
    "jsim_mpc_set_path_speed", "jsim_mpc_set_speed_cutoff", "jsim_mpc_update_cfg", "jsim_mpc_set_ego_config", "jsim_loop_obstacles",
    "jsim_mpc_xref_deviation_goal", "jsim_loop_run_scenario",
    "jsim_loop_set_groups", "jsim_loop_predict_egos", "jsim_loop_run_interacting",
    "jsim_loop_set_mate_prediction", "jsim_loop_predict_egos_plan",
    "jsim_loop_set_traffic", "jsim_loop_set_recorder", "jsim_loop_set_vehicle_shapes",
    "jsim_comm_unique_id", "jsim_comm_init", "jsim_mpc_gather", "jsim_comm_destroy", "jsim_plan_routes",
    "jsim_plan_routes_weighted", "jsim_score_trajectories", "jsim_loop_eval_reasons", "jsim_loop_eval_conflicts",
    "jsim_loop_eval_static", "jsim_loop_summarise_episodes", "jsim_loop_eval_cutoffs", "jsim_loop_fork_state", "jsim_loop_obstacles_at",
    "jsim_loop_eval_gaps", "jsim_loop_eval_tracking", "jsim_loop_eval_headway", "jsim_loop_score_predictions",
    "jsim_loop_set_plan_recorder", "jsim_loop_score_plan_predictions", "jsim_loop_eval_cutoffs_plan",
    "jsim_loop_checkpoint_save", "jsim_loop_checkpoint_load",
)
CKPT_MAX_ARRAYS = 32   # JSIM_CKPT_MAX_ARRAYS

_lib = None


class JsimError(RuntimeError):
    pass


# per-ego status of a step / tick (include/jsim_mpc.h; 3: the ego has no path)
STATUS_OK, STATUS_INFEASIBLE, STATUS_NEAREST_ANOMALY, STATUS_NO_PATH, STATUS_HELPER_TIMEOUT = 0, 1, 2, 3, 4
# how jsim_loop_run_interacting predicts an ego for its group mates (JSIM_MATE_CONSTANT, JSIM_MATE_PLAN)
MATE_PREDICTION = {"constant": 0, "plan": 1}


def check_status(status, what: str) -> None:
    """Raise on a status that is a fault of the library, not an outcome of the controller: JSIM_HELPER_TIMEOUT (a helper
    wavefront's bounded wait ran out; that ego's tick was treated like a failed solve).  `status`: host array of per-ego status."""
    bad = [int(b) for b in (status == STATUS_HELPER_TIMEOUT).nonzero()[0]]
    if bad:
        raise JsimError(f"{what}: status {STATUS_HELPER_TIMEOUT} (JSIM_HELPER_TIMEOUT) on ego(s) {bad[:8]}"
                        f"{' ..' if len(bad) > 8 else ''}: a helper wavefront gave up waiting for a column of the factor")


def load() -> C.CDLL:
    """Load the HIP library; raise if it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise JsimError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "The MPC path is HIP-only; there is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.jsim_abi_version.restype = C.c_int
    lib.jsim_abi_version.argtypes = []
    lib.jsim_last_error.restype = C.c_char_p
    lib.jsim_last_error.argtypes = [vp]
    lib.jsim_mpc_create.restype = C.c_int
    lib.jsim_mpc_create.argtypes = [C.POINTER(JsimCfg), C.c_int, C.POINTER(vp)]
    lib.jsim_mpc_destroy.restype = None
    lib.jsim_mpc_destroy.argtypes = [vp]
    lib.jsim_mpc_set_paths.restype = C.c_int
    lib.jsim_mpc_set_paths.argtypes = [vp, vp, vp, vp, vp, i32]
    lib.jsim_mpc_step.restype = C.c_int
    lib.jsim_mpc_step.argtypes = [vp, i32] + [vp] * 16
    lib.jsim_mpc_step_debug.restype = C.c_int
    lib.jsim_mpc_step_debug.argtypes = [vp, i32] + [vp] * 21
    lib.jsim_plant_step.restype = C.c_int
    lib.jsim_plant_step.argtypes = [vp, i32] + [vp] * 6
    lib.jsim_loop_advance.restype = C.c_int
    lib.jsim_loop_advance.argtypes = [vp, i32] + [vp] * 11 + [i32, vp, vp, i32, vp, vp]
    lib.jsim_loop_set_geometry.restype = C.c_int
    lib.jsim_loop_set_geometry.argtypes = [vp, dbl, dbl, dbl]
    lib.jsim_loop_set_obstacle_geometry.restype = C.c_int
    lib.jsim_loop_set_obstacle_geometry.argtypes = [vp, dbl, dbl, dbl, dbl]
    lib.jsim_loop_predict_obstacles.restype = C.c_int
    lib.jsim_loop_predict_obstacles.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.jsim_loop_pre_tick.restype = C.c_int
    lib.jsim_loop_pre_tick.argtypes = [vp, i32] + [vp] * 9 + [i32, i32, vp, vp, vp]
    lib.jsim_mpc_set_path_speed.restype = C.c_int
    lib.jsim_mpc_set_path_speed.argtypes = [vp, vp]
    lib.jsim_mpc_set_speed_cutoff.restype = C.c_int
    lib.jsim_mpc_set_speed_cutoff.argtypes = [vp, vp]
    lib.jsim_mpc_update_cfg.restype = C.c_int
    lib.jsim_mpc_update_cfg.argtypes = [vp, C.POINTER(JsimCfg)]
    lib.jsim_mpc_set_ego_config.restype = C.c_int
    lib.jsim_mpc_set_ego_config.argtypes = [vp, vp]
    lib.jsim_loop_obstacles.restype = C.c_int
    lib.jsim_loop_obstacles.argtypes = [vp, i32, vp, vp, vp, i32, vp]
    lib.jsim_mpc_set_launch_order.restype = C.c_int
    lib.jsim_mpc_set_launch_order.argtypes = [vp, i32]
    lib.jsim_mpc_get_launch_order.restype = C.c_int
    lib.jsim_mpc_get_launch_order.argtypes = [vp, i32, vp, vp]
    lib.jsim_mpc_iter_totals.restype = C.c_int
    lib.jsim_mpc_iter_totals.argtypes = [vp, i32, vp, i32]
    lib.jsim_mpc_run_ticks.restype = C.c_int
    lib.jsim_mpc_run_ticks.argtypes = [vp, i32, i32] + [vp] * 19 + [i32, vp, vp, i32, vp, vp]
    lib.jsim_loop_run_scenario.restype = C.c_int
    #                                       ctx B    ticks  x0..n_iter,di_ai,x0_spawn,target_spawn,age  max_age hist tick cap  n_resp
    lib.jsim_loop_run_scenario.argtypes = ([vp, i32, i32] + [vp] * 19 + [i32, vp, vp, i32, vp] +
                                           # traj_idx prev_len col_flag pre_status  window margin n_obs state param get  n_steps speed_cutoff stream
                                           [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, vp])
    lib.jsim_loop_set_groups.restype = C.c_int
    lib.jsim_loop_set_groups.argtypes = [vp, i32, i32, vp]
    lib.jsim_loop_set_traffic.restype = C.c_int
    lib.jsim_loop_set_traffic.argtypes = [vp, i32, i32, vp, vp, i32]
    lib.jsim_loop_set_vehicle_shapes.restype = C.c_int
    lib.jsim_loop_set_vehicle_shapes.argtypes = [vp, i32, vp]
    lib.jsim_loop_set_recorder.restype = C.c_int
    lib.jsim_loop_set_recorder.argtypes = [vp, i32, i32, vp, vp, i32, vp]
    lib.jsim_loop_predict_egos.restype = C.c_int
    lib.jsim_loop_predict_egos.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    lib.jsim_loop_set_mate_prediction.restype = C.c_int
    lib.jsim_loop_set_mate_prediction.argtypes = [vp, i32]
    lib.jsim_loop_predict_egos_plan.restype = C.c_int
    lib.jsim_loop_predict_egos_plan.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    lib.jsim_loop_run_interacting.restype = C.c_int
    lib.jsim_loop_run_interacting.argtypes = lib.jsim_loop_run_scenario.argtypes
    lib.jsim_mpc_xref_deviation_goal.restype = C.c_int
    lib.jsim_mpc_xref_deviation_goal.argtypes = [vp, i32] + [vp] * 9
    lib.jsim_comm_unique_id.restype = C.c_int
    lib.jsim_comm_unique_id.argtypes = [vp]
    lib.jsim_comm_init.restype = C.c_int
    lib.jsim_comm_init.argtypes = [vp, vp, i32, i32]
    lib.jsim_mpc_gather.restype = C.c_int
    lib.jsim_mpc_gather.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    lib.jsim_comm_destroy.restype = C.c_int
    lib.jsim_comm_destroy.argtypes = [vp]
    lib.jsim_plan_routes.restype = C.c_int
    #                               dev  R    start goal box tol hp hp_off  n_obs  r_off mp_pts mp_len  n_prim n_pts cc  cc_off wh wc  max_path  outs
    lib.jsim_plan_routes.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32] + [vp] * 7
    lib.jsim_plan_routes_weighted.restype = C.c_int
    #                                        ... as above ...                                                wh  wc form max_path cap  outs
    lib.jsim_plan_routes_weighted.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32] + [vp] * 7
    lib.jsim_score_trajectories.restype = C.c_int
    #                                      dev  S    cand_off pt_off pts mode time_from ego cyc now par  W    w   form ideal  outs
    lib.jsim_score_trajectories.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp] + [vp] * 8
    lib.jsim_loop_eval_reasons.restype = C.c_int
    #                                     ctx B    ticks rec flags n_obs obs_rec x_first x_spawn veh_of par threshold carry  outs      stream
    lib.jsim_loop_eval_reasons.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp] + [vp] * 4 + [vp]
    lib.jsim_loop_eval_conflicts.restype = C.c_int
    #                                       ctx B    ticks rec flags n_obs obs_rec x_first x_spawn veh_range mate_range shapes ego_shape w  outs  stream
    lib.jsim_loop_eval_conflicts.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32] + [vp] * 6 + [vp]
    lib.jsim_loop_eval_gaps.restype = C.c_int
    #                                  ctx B    ticks rec flags n_obs obs_rec x_first x_spawn veh_range mate_range shapes ego_shape window within outs stream
    lib.jsim_loop_eval_gaps.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32] + [vp] * 5 + [vp]
    lib.jsim_loop_eval_tracking.restype = C.c_int
    #                                      ctx B    ticks rec flags path_id n_pts px py pyaw n_paths path_off arc outs  stream
    lib.jsim_loop_eval_tracking.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp] + [vp] * 7 + [vp]
    lib.jsim_loop_eval_headway.restype = C.c_int
    #                                     ctx B    ticks rec flags n_obs obs_rec x_first x_spawn veh_range mate_range shapes ego_shape
    lib.jsim_loop_eval_headway.argtypes = ([vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp] +
                                           # path_id n_pts px py pyaw n_paths path_off arc margin outs (8 + 3 per place) stream
                                           [vp, i32, vp, vp, vp, i32, vp, vp, dbl] + [vp] * 11 + [vp])
    lib.jsim_loop_eval_static.restype = C.c_int
    #                                    ctx B    ticks rec flags x_first x_spawn set_of n_sets set_off n_rows rows ego_shape hidden outs  stream
    lib.jsim_loop_eval_static.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, i32] + [vp] * 4 + [vp]
    lib.jsim_loop_summarise_episodes.restype = C.c_int
    #                                           ctx B    ticks rec flags x_first x_spawn  veh_ (5) st_ (4) rs_ (2)  ep_cap ep_off ep_i ep_d stream
    lib.jsim_loop_summarise_episodes.argtypes = [vp, i32, i32, vp, vp, vp, vp] + [vp] * 11 + [i32, vp, vp, vp, vp]
    lib.jsim_loop_eval_cutoffs.restype = C.c_int
    #                                     ctx B    ticks rec flags n_obs obs_rec x_first x_spawn window margin n_steps speed interacting chunk first carry outs      stream
    lib.jsim_loop_eval_cutoffs.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp] + [vp] * 6 + [vp]
    lib.jsim_loop_score_predictions.restype = C.c_int
    #                                          ctx B    ticks rec flags n_obs obs_rec x_first x_spawn egos n_steps tol pt_i pt_d step_sum step_cnt err stream
    lib.jsim_loop_score_predictions.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, dbl] + [vp] * 5 + [vp]
    lib.jsim_loop_set_plan_recorder.restype = C.c_int
    #                                          ctx B    cap  plan_oa plan_od plan_status
    lib.jsim_loop_set_plan_recorder.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.jsim_loop_score_plan_predictions.restype = C.c_int
    #                                               ctx B    ticks rec flags x_first x_spawn plan_oa plan_od plan_status n_steps tol outs     stream
    lib.jsim_loop_score_plan_predictions.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, dbl] + [vp] * 5 + [vp]
    lib.jsim_loop_eval_cutoffs_plan.restype = C.c_int                    # jsim_loop_eval_cutoffs', the three plan pointers ahead of stream
    lib.jsim_loop_eval_cutoffs_plan.argtypes = lib.jsim_loop_eval_cutoffs.argtypes[:-1] + [vp] * 3 + [vp]
    lib.jsim_loop_fork_state.restype = C.c_int
    #                                   ctx B    ticks rec flags x_first x_spawn n_rows ego at x0  k0  stream
    lib.jsim_loop_fork_state.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.jsim_loop_obstacles_at.restype = C.c_int
    #                                     ctx n_obs state0 param wheelbase ticks state stream
    lib.jsim_loop_obstacles_at.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.jsim_loop_checkpoint_save.restype = C.c_int
    #                                        ctx n_arrays src dst bytes stream
    lib.jsim_loop_checkpoint_save.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.jsim_loop_checkpoint_load.restype = C.c_int
    #                                        ctx B    n_slots written n_rows ego slot n_fields slab dst row_bytes n_obs obs_slab n_veh veh_src veh_slot obs_state stream
    lib.jsim_loop_checkpoint_load.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]
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
