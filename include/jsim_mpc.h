/*
 * jsim_mpc.h -- C-ABI of libjsim_mpc.so: the MI355X (gfx950) batched replacement for the reference's
 * per-timestep MPC solve.  extern "C", plain pointers and sizes, no torch / C++ types.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo root):
 *   jsim_mpc_create      <- module-level config load main/lib/mpc.py:15-39 (main/config/mpc_config.json)
 *                           + MPC.__init__ scalars (dl, dt, car_dimensions.L)   main/lib/mpc.py:246-275
 *   jsim_mpc_set_paths   <- MPC.__init__ cx/cy/cyaw + MPC.set_trajectory_fromarray  main/lib/mpc.py:257-261,279-282
 *                           (truncation = per-ego path_len passed to jsim_mpc_step)
 *   jsim_mpc_step        <- MPC.step -> _iterative_linear_mpc_control -> _calc_ref_trajectory,
 *                           _predict_motion, _linear_mpc_control (cvxpy->ECOS)    main/lib/mpc.py:284-303,214-242,89-211
 *                           with calc_nearest_index_in_direction                  main/lib/trajectories.py:100-126
 *                           and Simulation.step / Bicycle.step for the rollout    main/lib/simulation.py:35-47, main/bicycle/main.py:28-41
 *   jsim_plant_step      <- HistorySimulation.step / Simulation.step (the per-vehicle loop's plant update)
 *                           main/lib/simulation.py:35-47,58-61 ; main/scenarios/mpc_intersection.py:163
 *   jsim_loop_advance    <- the rest of the loop body: plant update, history, `if mpc.is_goal(state): break`
 *                           main/scenarios/mpc_intersection.py:99-101,163 ; main/lib/simulation.py:64-88 (History)
 *   jsim_mpc_run_ticks   <- `for i in itertools.count():` itself, main/scenarios/mpc_intersection.py:99 (K iterations per call)
 *   jsim_mpc_set_path_speed / _set_speed_cutoff / _update_cfg <- the data-only MPC variants main/lib/mpc_with_speed.py,
 *                           main/lib/mpc_sensitivity.py
 *   jsim_mpc_xref_deviation_goal <- MPC.get_current_xref_deviation / MPC.is_goal  main/lib/mpc.py:305-330
 *
 * Conventions
 *   - All array arguments of jsim_mpc_step / jsim_plant_step / ..._goal are DEVICE pointers (HBM), caller-owned,
 *     no allocation inside those calls; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     jsim_mpc_set_paths takes HOST pointers (one-time upload into the context's resident path table).
 *   - Ego-major rows: a wavefront owns one ego, so every per-ego array is one contiguous row
 *     (x0 [B][4], oa/od [B][T], ox/oy/ov/oyaw [B][T+1], xref [B][4][T+1], active_mask [B][ceil(8T/32)]).
 *   - State order is the MPC's [x, y, v, yaw] (main/lib/mpc.py:291), NOT State's (x, y, yaw, v).
 *   - Return value: 0 on success, negative on error (-EINVAL style); never throws.  jsim_last_error()
 *     returns a message for the last failing call on that context (or globally when ctx == NULL).
 *   - Per-ego status (int32): 0 ok; 1 QP infeasible / not converged (reference: prints
 *     "Error: Cannot solve mpc..." and returns None, main/lib/mpc.py:207-209 -- outputs ox..oyaw are left
 *     untouched, oa/od are zeroed = the reference's cold start after None, caller applies ai = MAX_DECEL);
 *     2 nearest-index anomaly (reference raises Exception("something wrong"), main/lib/trajectories.py:120 --
 *     nothing but status is written for that ego).
 *   - Active-constraint indices (bit i of active_mask) use the canonical row order of the reference's
 *     constraint list main/lib/mpc.py:187-194:
 *       D  steer-rate rows  2t (+), 2t+1 (-), t = 0..T-2        [0, 2T-2)
 *       VU v_t <= speed,     t = 0..T                            [2T-2, 3T-1)
 *       VL v_t >= MIN_SPEED, t = 0..T                            [3T-1, 4T)
 *       AU a_t <= MAX_ACCEL                                      [4T, 5T)
 *       AL a_t >= MAX_DECEL                                      [5T, 6T)
 *       S  +-delta_t <= MAX_STEER rows 6T+2t (+), 6T+2t+1 (-)    [6T, 8T)
 *     bit set <=> the row is in the final working set with multiplier > 1e-9 * max(1, ||g||_inf).
 */
#ifndef JSIM_MPC_H
#define JSIM_MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JSIM_ABI_VERSION 2 /* 2: jsim_cfg ends with nx, reserved_, jerk_weight */
#define JSIM_MAX_T 48 /* two (2T)x(2T+1) fp64 tiles must fit the 160 KiB LDS of one CU */
#define JSIM_MAX_OBS 8   /* obstacles one ego's glue can hold: its scripted vehicles, then its group mates */
#define JSIM_MAX_PRED 64 /* samples of the longest prediction (n_steps): one lane of a wavefront each */

typedef struct jsim_cfg {
    int32_t T;        /* horizon; 1 <= T <= JSIM_MAX_T (stock 13) */
    int32_t max_iter; /* MAX_ITER (1..16; stock value 1): linearisation passes per step, main/lib/mpc.py:231 */
    double dt, dl, L;
    double w_perp, w_para;
    double R[2], Rd[2], Q_v_yaw[2];
    double Qf[4];     /* as in the JSON; multiplied by T inside (main/lib/mpc.py:28) */
    double R_end[2];  /* diag(10,10), main/lib/mpc.py:181 */
    double max_dsteer; /* rad/s */
    double max_accel, max_decel;
    double max_steer, max_speed, min_speed; /* Simulation.* main/lib/simulation.py:23-25 */
    double min_ref_speed;                   /* 10/3.6, main/lib/mpc.py:99 */
    double goal_dis, stop_speed;
    int32_t nx;          /* 4: main/lib/mpc.py.  5: main/lib/mpc_jerk.py -- acceleration state x[4] with A[4][4] = 1, A[2][4] = dt,
                          * B[4][0] = dt (:67-78), x[4,0] free (:193): the condensed QP has 2T + 1 variables (acc_0 last), oa =
                          * u[0,:] is the input of that state; runs on the LDS-resident kernel */
    int32_t reserved_;
    double jerk_weight;  /* jerk_penalty_weight of (x[4,t+1] - x[4,t])^2, t < T-1 (main/lib/mpc_jerk.py:31,190); nx == 5 only */
} jsim_cfg;

typedef struct jsim_ctx jsim_ctx;

/* Per-ego status of a step / tick.  JSIM_NO_PATH: the ego has no path (path_len < 1).  JSIM_HELPER_TIMEOUT: an internal fault of the kernels with
 * helper wavefronts -- a helper's bounded wait for a column of the factor ran out; the tick is treated like a failed solve (nothing
 * of the controller is updated, the loops brake with MAX_DECEL), and the Python layer raises JsimError when it reads the status. */
enum { JSIM_OK = 0, JSIM_INFEASIBLE = 1, JSIM_NEAREST_ANOMALY = 2, JSIM_NO_PATH = 3, JSIM_HELPER_TIMEOUT = 4 };

int jsim_abi_version(void);
const char *jsim_last_error(const jsim_ctx *ctx);

int jsim_mpc_create(const jsim_cfg *cfg, int device_id, jsim_ctx **out);
void jsim_mpc_destroy(jsim_ctx *ctx);

/* HOST pointers.  cyaw must already be smoothed (MPC.__init__ does it on the host, in place).  Also fills the context's table of
 * the yaws' sin / cos (32 B per point; the register kernels read it instead of evaluating them in every tick -- same values);
 * JSIM_PATH_TRIG=0 in the environment at the time of the call leaves it out.  Synchronises the device. */
int jsim_mpc_set_paths(jsim_ctx *ctx, const double *cx, const double *cy, const double *cyaw,
                       const int64_t *path_off /*[n_paths+1]*/, int32_t n_paths);

/* One MPC.step for B egos.  In/out: target_ind [B], oa/od [B][T] (warm start in, solution out).
 * Optional outputs may be NULL: ox, oy, ov, oyaw, xref, active_mask, n_iter. */
int jsim_mpc_step(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                  const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa,
                  double *od, double *ox, double *oy, double *ov, double *oyaw, double *xref,
                  uint32_t *active_mask, int32_t *status, int32_t *n_iter, void *stream);

/* Same, plus stage-level outputs for parity tests (any may be NULL):
 * xbar [B][4][T+1], ref_idx [B][T+1], H [B][n][n] (lower triangle valid), g [B][n], lam [B][8T]; n = 2T (2T + 1 with nx == 5). */
int jsim_mpc_step_debug(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                        const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa,
                        double *od, double *ox, double *oy, double *ov, double *oyaw, double *xref,
                        uint32_t *active_mask, int32_t *status, int32_t *n_iter, double *xbar,
                        int64_t *ref_idx, double *H, double *g, double *lam, void *stream);

/* Controller output + plant update for B egos: (di, ai) = (od[b][0], oa[b][0]) when status[b]==0, else
 * ai = MAX_DECEL and di = di_prev[b] (main/lib/mpc.py:298-303); then Simulation.step on x0 in place.
 * di_ai [B][2] in/out (previous steer in, applied (steer, accel) out). */
int jsim_plant_step(jsim_ctx *ctx, int32_t B, double *x0, const double *oa, const double *od,
                    const int32_t *status, double *di_ai, void *stream);

/* One tick of closed-loop bookkeeping for a batch, the rest of the per-vehicle loop body
 * (main/scenarios/mpc_intersection.py:99-163): (di, ai) selection + plant step as jsim_plant_step, optional
 * history record hist[tick][B][2] (tick = a device counter this call increments, so the call can be replayed
 * from a hipGraph), and replacement of finished egos: an ego for which MPC.is_goal holds on its new state
 * (main/lib/mpc.py:314-330; the loop's `break`, :101) or whose age reaches max_age ticks (<=0: never) restarts
 * from x0_spawn/target_spawn with a cold controller (oa = od = 0, di = ai = 0). n_respawn (optional) counts them. */
int jsim_loop_advance(jsim_ctx *ctx, int32_t B, double *x0, double *oa, double *od, const int32_t *status,
                      double *di_ai, int64_t *target_ind, const int32_t *path_id, const int32_t *path_len,
                      const double *x0_spawn, const int64_t *target_spawn, int32_t *age, int32_t max_age,
                      double *hist, int32_t *tick, int32_t hist_cap, uint64_t *n_respawn, void *stream);

/* ---- MPC variants that differ from main/lib/mpc.py only in data ----
 * jsim_mpc_set_path_speed: per-point speed reference cv (HOST array aligned with cx/cy/cyaw of jsim_mpc_set_paths, or NULL
 *   to switch it off): xref[2] = cv[idx] instead of 0, main/lib/mpc_with_speed.py:85-110.
 * jsim_mpc_set_speed_cutoff: caller-owned DEVICE array [B] (or NULL): ego b's reference is zeroed from that path index on
 *   (set_trajectory_fromarray(trajectory, cutoff_idx), main/lib/mpc_with_speed.py:276-282); entries < 0 mean no cut-off.
 * jsim_mpc_update_cfg: replace weights / limits between solves (same T), which is what main/lib/mpc_sensitivity.py does by
 *   re-reading its JSON inside every solve (:153-166).  The other differences of the variants are parameter values:
 *   mpc_with_speed uses w_perp = 10, Q_v_yaw = (20, 0.5), MAX_DECEL = -5 and speed limit Simulation.MAX_SPEED. */
int jsim_mpc_set_path_speed(jsim_ctx *ctx, const double *cv);
int jsim_mpc_set_speed_cutoff(jsim_ctx *ctx, const int32_t *cv_cut);
int jsim_mpc_update_cfg(jsim_ctx *ctx, const jsim_cfg *cfg);

/* Per-ego weights and limits: a whole sensitivity sweep (main/scenarios/mpc_sensitivity_analysis*.py run the loop once per
 * parameter set, rewriting config/mpc_config_sensitivity.json in between) as ONE batch -- ego b solves with its own row of
 * cfg, a caller-owned DEVICE array [B][JSIM_EGO_CFG_DOUBLES] in the JSON's own units.
 * PRECONDITION: R[0] > 0 and R[1] > 0 in every row, as jsim_mpc_create / jsim_mpc_update_cfg demand of the context's R.  The
 *   kernels factor H = L L' without a status and rely on H >= 2 min(R) I; the table lives on the device and is NOT checked.  The
 *   study's own sweeps contain R entries of 0 (at a standstill a zero steering weight leaves H singular; DESIGN.md section 4,
 *   "Conditioning").  What a row with an R entry of 0 gets: a pivot that is not positive is replaced by 1e-300, every loop stays
 *   bounded, the status is 0 or 1 -- the same on every kernel of a horizon -- and a status-0 answer is optimal in value
 *   (tests/test_gpu_conditioning.py); along a direction that costs nothing the answer is not unique, and a status of 1 makes the
 *   ego brake like any failed solve.  A caller who wants a unique answer keeps R > 0 (1e-8 is enough for cond(H) <= 1e13 up to T = 40).
 * The row:
 *   { w_perp, w_para, R[0], R[1], Rd[0], Rd[1], Q_v_yaw[0], Q_v_yaw[1], Qf[0..3] (unscaled; x T inside, mpc.py:28),
 *     MAX_DSTEER [rad/s], MAX_ACCEL, MAX_DECEL, reserved }.
 * Everything else (T, dt, dl, L, R_end, speed limits, goal test) stays with the context's jsim_cfg.  NULL switches back. */
#define JSIM_EGO_CFG_DOUBLES 16
int jsim_mpc_set_ego_config(jsim_ctx *ctx, const double *cfg);

/* ---- the loop glue that produces the truncated path, main/scenarios/mpc_intersection.py:104-140 ----
 * jsim_loop_set_geometry: the car's two collision circles (offsets of their centres from the rear axle along the body
 *   axis, radius) = car_dimensions.circle_centers / .radius, main/lib/car_dimensions.py:62-79; precomputes the circle
 *   centres of every path point (main/lib/trajectories.py:11-55).  Call after jsim_mpc_set_paths or before; either order.
 * jsim_loop_predict_obstacles: MovingObstaclesPrediction.state_prediction for n_obs obstacles (<= 8), n_steps samples
 *   (<= 64; the loop uses len(arange(0, 7.0, DT)) = 35), main/lib/moving_obstacles_prediction.py:21-47.
 *   obst [n_obs][6] = (x, y, v, yaw, a, steer) as MovingObstacle*.get() returns them; pred [n_obs][n_steps][3] = (x, y, yaw).
 * jsim_loop_pre_tick: per ego -- progress index traj_idx on the FULL path (in/out; skipped when it sits on the last point
 *   of the previous truncated path, :106-109), resample_curve of the remaining path with the accelerate-to-MAX_SPEED
 *   spacing (:111-120, main/lib/trajectories.py:58-86), check_collision_moving_cars against the predictions with
 *   +-frame_window frame offsets (main/lib/collision_avoidance.py:68-124), get_cutoff_curve_by_position_idx minus `margin`
 *   (:133-140, main/lib/collision_avoidance.py:168-180).  path_len [B] out = cut-off length (full length if no collision) --
 *   exactly what jsim_mpc_step takes.  prev_path_len [B]: previous tick's path_len, -1 before the first tick.
 *   status: 0 ok, 2 nearest-index anomaly, 4 resampled path longer than the kernel's 320-point table. */
int jsim_loop_set_geometry(jsim_ctx *ctx, double cc_front, double cc_rear, double radius);
/* n_ticks ticks of the WHOLE scenario loop (main/scenarios/mpc_intersection.py:99-163) for B egos and n_obs scripted obstacle
 * vehicles: obstacle get() -> prediction -> progress index / resample / collision / cut-off (jsim_loop_pre_tick) -> MPC.step ->
 * plant, history, goal (jsim_loop_advance) -> obstacle step().  Arguments as in jsim_mpc_run_ticks, jsim_loop_pre_tick
 * (traj_idx, prev_path_len in/out; path_len, col_flag, pre_status out) and jsim_loop_obstacles (obs_state in/out, obs_param,
 * obs_get [n_obs][6] out).  speed_cutoff = 1: the glue of main/scenarios/mpc_intersection_new_ref.py:122-139 -- the path
 * stays whole (path_len must hold the full lengths) and the cut-off index goes to the buffer registered with
 * jsim_mpc_set_speed_cutoff.  With a register kernel (T = 13, 15, 16, 20, 25, 30, 32, 40) and MAX_ITER = 1 it is three launches: obstacles rolled forward n_ticks ticks, their predictions for
 * every tick, and ONE fused launch in which every ego's wave runs its own glue + solve + plant n_ticks times; otherwise the
 * same ticks as separate launches.  Identical results either way. */
int jsim_loop_run_scenario(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id, int32_t *path_len,
                           const double *speed, int64_t *target_ind, double *oa, double *od, double *ox, double *oy, double *ov,
                           double *oyaw, double *xref, uint32_t *active_mask, int32_t *status, int32_t *n_iter, double *di_ai,
                           const double *x0_spawn, const int64_t *target_spawn, int32_t *age, int32_t max_age, double *hist,
                           int32_t *tick, int32_t hist_cap, uint64_t *n_respawn, int64_t *traj_idx, int32_t *prev_path_len,
                           int32_t *col_flag, int32_t *pre_status, int32_t frame_window, int32_t margin, int32_t n_obs,
                           double *obs_state, const double *obs_param, double *obs_get, int32_t n_steps, int32_t speed_cutoff,
                           void *stream);
/* Obstacles of another shape than the ego (main/scenarios/overtaking_cyclist_bidirectional_road.py:122-133: the cyclist's
 * BicycleRealDimensions): their two circles and wheelbase -- used by the prediction (MovingObstaclesPrediction(...,
 * car_dimensions=bicycle_dimensions)) and by the collision rows of check_collision_moving_bicycle,
 * main/lib/collision_avoidance.py:126-166 (min_distance = car radius + bicycle radius, same row order).  Without this call
 * the obstacles have the ego's geometry (check_collision_moving_cars). */
int jsim_loop_set_obstacle_geometry(jsim_ctx *ctx, double cc_front, double cc_rear, double radius, double wheelbase);
/* ---- Per-vehicle shapes: a car AND a cyclist in one loop.  The reference has two collision checks,
 * check_collision_moving_cars (main/lib/collision_avoidance.py:85-124) and check_collision_moving_bicycle
 * (main/lib/collision_avoidance.py:126-165), which differ in the obstacle's circles and in min_distance = car radius + the obstacle's radius, and one prediction,
 * main/lib/moving_obstacles_prediction.py:21-47, which takes the obstacle's wheelbase and circles from its car_dimensions.
 * jsim_loop_set_vehicle_shapes: shapes [n][4] (HOST) = (cc_front, cc_rear, radius, wheelbase) of each scripted vehicle -- the
 *   arguments of jsim_loop_set_obstacle_geometry -- in the order of the obstacle tables: [n_obs] of a shared obstacle list, or
 *   the [total] flat order of jsim_loop_set_traffic.  Vehicle i is predicted and stepped with its own wheelbase, its circle
 *   centres use its own offsets, and an ego circle touches one of its circles when sqrt(dx^2 + dy^2) <= ego radius + radius_i
 *   -- in the bounding-circle prune, the pair table and the first touching point of the detailed path alike.  Row order,
 *   first-hit rule, cut-off and margin are unchanged.  n = 0 clears the table: every vehicle has the global obstacle geometry
 *   again.  Needs jsim_loop_set_geometry first (the thresholds follow a later call of it).  Registering a table (and that
 *   later call) waits for the device to finish what is in flight, on every stream, before the device copies are replaced.
 *   Refused (-22), the previous table kept: a radius or wheelbase that is not positive, an offset that is not finite.
 *   While a table is registered, jsim_loop_obstacles, jsim_loop_predict_obstacles, jsim_loop_pre_tick, jsim_loop_run_scenario
 *   and jsim_loop_run_interacting refuse (-22) an n_obs (a total, with a traffic layout) other than n; a call without any
 *   obstacle (n_obs = 0) passes.  jsim_loop_run_interacting runs scripted vehicles of any shape beside the group mates, which
 *   keep the ego's shape and the ego / ego threshold; without a table it still refuses after jsim_loop_set_obstacle_geometry.
 *   A table in which every row is the global geometry changes no result bit. */
int jsim_loop_set_vehicle_shapes(jsim_ctx *ctx, int32_t n, const double *shapes /* host, [n][4] */);
/* Scripted obstacle vehicles of main/lib/moving_obstacles.py -- MovingObstacleTIntersection (:166-232, kind 0),
 * MovingObstacleRoundabout (:28-124, kind 1), MovingObstacleArterial (:126-164, kind 2): state [n_obs][4] = (xc, yc, theta,
 * counter) in/out, param [n_obs][8] = (direction +-1, turning 0/1, speed, offset seconds (<= 0: none), x_turn, dt, kind,
 * initial_speed).  Writes the `get()` tuples (x, y, v, yaw, 0, steer) of the CURRENT state to `get` (may be NULL) -- the input
 * of jsim_loop_predict_obstacles -- and, when do_step != 0, advances the state by one `step()`. */
int jsim_loop_obstacles(jsim_ctx *ctx, int32_t n_obs, double *state, const double *param, double *get, int32_t do_step,
                        void *stream);
/* ---- Route vehicles (kind 3): a scripted vehicle that follows any polyline at a scripted speed.  Bicycle.step
 * (main/bicycle/main.py:28-41) is explicit Euler -- every tick a straight move of length v * dt along the heading -- so a
 * reference vehicle played back along its own recorded poses is a special case of the rule below.
 * jsim_loop_set_traffic_routes: the table of n_routes polylines, HOST arrays x, y, yaw [off[n_routes]] and off [n_routes + 1]
 *   (route r owns the points off[r] .. off[r + 1] - 1).  yaw must be continuous along a route (no 2 pi jumps).  Per route the
 *   device sums the arc length S[0] = 0, S[j] = S[j-1] + sqrt(dx^2 + dy^2) in index order in fp64.  n_routes = 0 clears the
 *   table.  Refused (-22), the previous table kept: a null context, a negative count, offsets that do not start at 0 or
 *   decrease, a null array with n_routes > 0, a coordinate or yaw that is not finite.  The call waits for the device to finish
 *   what is in flight, on every stream, before the device copies are replaced.
 * A route vehicle is a row of jsim_loop_obstacles' tables: param = (route, end, speed, offset_s, s0, dt, 3.0, period_ticks),
 *   state = (x, y, yaw, counter).  Only the counter is read; the pose slots are outputs, rewritten on every call.
 * The pose at a counter c (L: the vehicle's own wheelbase, as for the other kinds):
 *   1. c' = c mod period_ticks if period_ticks >= 1, else c.
 *   2. n0 = floor(offset_s / dt) + 1 if offset_s > 0, else 0 (kind 0's `counter > offset / dt`).
 *   3. m = max(0, c' - n0).
 *   4. s = s0 + m * (speed * dt).
 *   5. s < S_end (the route's length): j = the largest index with S[j] <= s and j <= n - 2; if S[j+1] - s <= 1e-9 and
 *      j + 1 <= n - 2, j + 1 is taken (a vehicle that lands on a vertex takes the segment ahead, whatever the rounding).
 *      f = (s - S[j]) / (S[j+1] - S[j]) (0 on a zero-length segment); x, y, yaw = p[j] + f * (p[j+1] - p[j]);
 *      v = speed if c' >= n0 else 0; steer = atan(L * (yaw[j+1] - yaw[j]) / (S[j+1] - S[j])) (0 on a zero-length segment).
 *   6. s >= S_end: end = 1 ("stop") holds the last point, end = 0 ("leave") parks the vehicle at (JSIM_ROUTE_PARK,
 *      JSIM_ROUTE_PARK, 0); v = 0 and steer = 0 either way.
 *   7. A route of fewer than two points behaves as "stop" at its point (an empty one: at the origin).
 *   8. The route index is clamped into the table.
 * get() writes (x, y, v, yaw, 0, steer) of the current counter; step() is counter += 1, then the pose of the new counter.
 * The prediction is unchanged (MovingObstaclesPrediction on the get() tuple).  A kind-3 row while no table is registered is
 * stepped as kind 0. */
#define JSIM_ROUTE_PARK 1000000 /* metres: where a route vehicle that has left stands, far from every road and finite */
int jsim_loop_set_traffic_routes(jsim_ctx *ctx, int32_t n_routes, const double *x, const double *y, const double *yaw,
                                 const int32_t *off /* host, [n_routes + 1] */);
int jsim_loop_predict_obstacles(jsim_ctx *ctx, int32_t n_obs, const double *obst, int32_t n_steps, double *pred, void *stream);
int jsim_loop_pre_tick(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id, int64_t *traj_idx,
                       const int32_t *prev_path_len, int32_t *path_len, int32_t *col_flag, double *col_xy,
                       int32_t *first_idx, int32_t *status, int32_t frame_window, int32_t margin,
                       int32_t *dbg_res_idx /*[B][320]*/, int32_t *dbg_n_res, void *stream);

/* ---- Interacting egos: several automated vehicles at one intersection that react to each other
 * (main/scenarios/interactive_mpc.py:117-190).  The obstacles of an ego are the scripted vehicles (spec order) and then the
 * OTHER egos of its group (ascending batch index); egos in different groups never affect each other.
 * jsim_loop_set_groups: group_off [n_groups + 1] (HOST) cuts the batch into contiguous groups, group_off[0] = 0,
 *   group_off[n_groups] = B, 1..8 egos per group.  n_groups = 0 clears the groups.
 * jsim_loop_predict_egos: every ego predicted like an obstacle, MovingObstaclesPrediction(x, y, v, yaw, a = 0,
 *   steering = di_ai[b][0]) with the ego's wheelbase and circles -- bit for bit what jsim_loop_predict_obstacles gives for
 *   that tuple.  x0 [B][4], di_ai [B][2]; pred [B][n_steps][3] = (x, y, yaw) or NULL.
 * jsim_loop_run_interacting: n_ticks Jacobi ticks (every prediction from the tick-start states), arguments as
 *   jsim_loop_run_scenario: obstacles get() -> their prediction -> the egos' prediction -> glue per ego -> MPC.step -> plant,
 *   history, goal / respawn -> glue reset of respawned egos -> obstacles step().  Separate launches per tick.  Refused (-22):
 *   no groups for this B, n_obs + (largest group - 1) > 8, speed_cutoff != 0, or after jsim_loop_set_obstacle_geometry
 *   without a shape table (jsim_loop_set_vehicle_shapes: then the collision rows have one distance threshold).  A group of one ego gives jsim_loop_run_scenario's results. */
int jsim_loop_set_groups(jsim_ctx *ctx, int32_t B, int32_t n_groups, const int32_t *group_off);
int jsim_loop_predict_egos(jsim_ctx *ctx, int32_t B, const double *x0, const double *di_ai, int32_t n_steps, double *pred,
                           void *stream);
int jsim_loop_run_interacting(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id, int32_t *path_len,
                              const double *speed, int64_t *target_ind, double *oa, double *od, double *ox, double *oy,
                              double *ov, double *oyaw, double *xref, uint32_t *active_mask, int32_t *status, int32_t *n_iter,
                              double *di_ai, const double *x0_spawn, const int64_t *target_spawn, int32_t *age, int32_t max_age,
                              double *hist, int32_t *tick, int32_t hist_cap, uint64_t *n_respawn, int64_t *traj_idx,
                              int32_t *prev_path_len, int32_t *col_flag, int32_t *pre_status, int32_t frame_window,
                              int32_t margin, int32_t n_obs, double *obs_state, const double *obs_param, double *obs_get,
                              int32_t n_steps, int32_t speed_cutoff, void *stream);

/* ---- Interacting egos that share their MPC plans (intent sharing).  How jsim_loop_run_interacting
 * predicts an ego for its group mates is context state: JSIM_MATE_CONSTANT (the default: jsim_loop_predict_egos' rule) or
 * JSIM_MATE_PLAN, THE RULE: ego m at the start of a tick has the state x0[m] = (x, y, v, yaw), the controls of its last solve
 * oa[m][0..T-1], od[m][0..T-1] as the engine holds them (element 0 is the input applied last tick; zeros before the first solve
 * and after a respawn), that solve's status[m], and the steering applied last tick di_ai[m][0].  The input of prediction step
 * i = 0 .. n_steps - 1 is, with j = i + 1,
 *     status[m] == JSIM_OK:  (a, delta) = (oa[m][j], od[m][j]) while j <= T - 1, then (0, od[m][T - 1]) -- the plan's last
 *                            steering held at constant speed; a plan longer than n_steps is not read to its end;
 *     any other status:      (0, di_ai[m][0]) for every step.
 *   Each step is the plant's (Simulation.step, main/lib/simulation.py:35-47, with the wheelbase and the clamps
 *   jsim_loop_advance uses): delta clamped to +-MAX_STEER; x += v cos(yaw) dt, y += v sin(yaw) dt; yaw += (v / L) tan(delta) dt
 *   with the speed from BEFORE the update; v += a dt, clamped to [MIN_SPEED, MAX_SPEED].  Sample i is the pose after step i (the
 *   first lies one dt ahead); circle centres and the bounding circle are made from the samples as jsim_loop_predict_egos makes them.
 * jsim_loop_set_mate_prediction: the mode jsim_loop_run_interacting uses from now on (nothing else reads it).  Any other value:
 *   -22, the mode stays as it was.
 * jsim_loop_predict_egos_plan: the counterpart of jsim_loop_predict_egos under THE RULE, T the context's.  x0 [B][4], oa and od
 *   [B][T], status [B], di_ai [B][2] (DEVICE); pred [B][n_steps][3] = (x, y, yaw) or NULL.  Same checks: geometry set, B >= 0,
 *   1 <= n_steps <= 64, no null pointer. */
#define JSIM_MATE_CONSTANT 0
#define JSIM_MATE_PLAN 1
int jsim_loop_set_mate_prediction(jsim_ctx *ctx, int32_t mode);
int jsim_loop_predict_egos_plan(jsim_ctx *ctx, int32_t B, const double *x0, const double *oa, const double *od,
                                const int32_t *status, const double *di_ai, int32_t n_steps, double *pred, void *stream);

/* ---- Traffic sets: each ego of a batch meets its own scripted vehicles (the reference's studies vary offsets, speeds, turning
 * and kind of the traffic: main/scenarios/mpc_intersection.py, mpc_intersection_new_ref.py, mpc_roundabout.py).
 * jsim_loop_set_traffic: set_of [B] (HOST) gives each ego its set, obs_off [n_sets + 1] (HOST) the sets' vehicles in the
 *   obstacle tables: set s is vehicles obs_off[s] .. obs_off[s + 1] - 1, obs_off[0] = 0, non-decreasing, 0..8 per set.
 *   n_sets = 0 clears the layout.  chunk_ticks: ticks per fused launch of jsim_loop_run_scenario, 0 = as many as fit a
 *   512 MiB budget of precomputed predictions (total x n_steps x 32 B per tick, plus 80 B per vehicle).  Refused (-22), the
 *   previous layout kept: set_of out of range, obs_off not starting at 0 or decreasing, a set of more than 8 vehicles.
 *   While a layout is registered, n_obs of jsim_loop_run_scenario / jsim_loop_run_interacting is the TOTAL obs_off[n_sets]
 *   (obs_state, obs_param, obs_get [total][4 | 8 | 6]); they refuse (-22) another B or total, and jsim_loop_run_interacting
 *   refuses a group whose egos have different sets or whose set's vehicles + group mates exceed 8.  All vehicles of all sets
 *   step once per tick.  Ego e's results equal those of a run in which set set_of[e] is the shared obstacles, bit for bit. */
int jsim_loop_set_traffic(jsim_ctx *ctx, int32_t B, int32_t n_sets, const int32_t *set_of, const int32_t *obs_off,
                          int32_t chunk_ticks);

/* ---- Per-tick History of every ego (lib.simulation.History, main/lib/simulation.py:50-88, and the scripts' obstacles_positions,
 * main/scenarios/mpc_intersection.py:166-177), recorded by the loop entry points where the state lives.
 * jsim_loop_set_recorder: caller-owned DEVICE buffers; cap = 0 clears.  While registered, jsim_loop_advance, jsim_mpc_run_ticks,
 *   jsim_loop_run_scenario and jsim_loop_run_interacting write slot k = the device tick counter of the tick (the one hist uses;
 *   slots k >= cap are dropped, the counter keeps counting):
 *   rec [cap][B][7] = x, y, yaw, v after the plant step and before any respawn (History's field order), the applied delta and a,
 *     and xref_deviation = what jsim_mpc_xref_deviation_goal gives for that tick's ox[0], oy[0], target_ind (NaN when the solve
 *     failed);
 *   flags [cap][B] = JSIM_REC_* bits;
 *   obs_rec [cap][n_obs][6] (NULL / n_obs = 0: not recorded) = the scripted vehicles' get() tuples of the tick, ahead of their
 *     step() -- all vehicles of a traffic layout.
 *   Refused (-22), nothing changed: B < 0, cap < 0, n_obs < 0, cap > 0 with a null rec / flags, or an obs_rec whose n_obs is not
 *   the registered traffic layout's total.  The loop entry points refuse (-22) a run while
 *   a recorder is registered for another B, a run without a tick counter, and (scenario / interacting, obs_rec given) another n_obs. */
enum { JSIM_REC_FIELDS = 7, JSIM_REC_FAILED = 1, JSIM_REC_GOAL = 2, JSIM_REC_AGE = 4 };
int jsim_loop_set_recorder(jsim_ctx *ctx, int32_t B, int32_t cap, double *rec, int32_t *flags, int32_t n_obs, double *obs_rec);

/* n_ticks consecutive closed-loop ticks, each = jsim_mpc_step followed by jsim_loop_advance, with identical results.
 * For the horizons that have the fused register-resident kernel (T = 13, 20) this is ONE launch in which every
 * wavefront runs all n_ticks for its own ego (egos are independent, so none waits for the slowest solve of a tick);
 * other horizons fall back to 2 * n_ticks launches.  The per-step outputs (ox .. n_iter) hold the LAST tick's values. */
int jsim_mpc_run_ticks(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id,
                       const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa, double *od,
                       double *ox, double *oy, double *ov, double *oyaw, double *xref, uint32_t *active_mask,
                       int32_t *status, int32_t *n_iter, double *di_ai, const double *x0_spawn,
                       const int64_t *target_spawn, int32_t *age, int32_t max_age, double *hist, int32_t *tick,
                       int32_t hist_cap, uint64_t *n_respawn, void *stream);

/* Launch order of the fused closed-loop launches (jsim_mpc_run_ticks, jsim_loop_run_scenario).  No reference counterpart:
 * the reference runs one vehicle per process (main/scenarios/mpc_intersection.py:99); this is scheduling of the batch only.
 * With 512 <= B <= 65536 workgroup b of a launch is given the ego that ranked b-th by the active-set iterations it needed in
 * the previous launch of this context (most first), so that the egos far from their paths do not start last; results are
 * those of the identity order bit for bit.  On by default (JSIM_LAUNCH_ORDER=0 in the environment turns it off);
 * jsim_mpc_set_launch_order overrides the environment for one context.  jsim_mpc_get_launch_order copies the order used by
 * the last launch and the iteration counts that launch recorded to HOST arrays [B] (either may be NULL); it synchronises. */
int jsim_mpc_set_launch_order(jsim_ctx *ctx, int32_t enabled);
int jsim_mpc_get_launch_order(jsim_ctx *ctx, int32_t B, int32_t *order, uint32_t *work);

/* Per-ego running totals of active-set iterations since the last reset, over every tick run through jsim_mpc_run_ticks,
 * jsim_loop_run_scenario and jsim_loop_run_interacting: fused launches and separate launches per tick alike (no register kernel,
 * MAX_ITER > 1 with a tick's count summed over its passes, JSIM_FORCE_LDS_KERNEL, the interacting glue).  Single steps
 * (jsim_mpc_step) do not count.  No reference counterpart (the reference never sees its solver's iterations,
 * main/lib/mpc.py:196-199); this is the measurement hook bench.py takes mean iterations, algorithmic flops and the straggler
 * statistic of the TIMED launches from.  Copies totals [B] to a HOST array (may be NULL) and, with reset != 0, clears them; it
 * synchronises. */
int jsim_mpc_iter_totals(jsim_ctx *ctx, int32_t B, uint64_t *totals, int32_t reset);

/* ---- the route planner: A* over motion primitives, a batch of route queries at once ----
 * Replaces MotionPrimitiveSearch(scenario, car_dimensions, mps, margin).run() -- main/lib/mp_search_ww_generic.py:136-257 with
 * main/lib/a_star.py:31-78 and main/lib/obstacles.py:157-176 -- which every scenario script calls once before its loop
 * (main/scenarios/mpc_intersection.py:63-64) and whose (M, 3) [x, y, yaw] trajectory becomes the MPC's path.  One wavefront
 * searches one route; n_routes routes in one launch.  HOST pointers in and out (a one-time precompute: the output is what
 * jsim_mpc_set_paths takes).
 *   start, goal [R][3] (x, y, theta); goal_box [R][4] = (x1, y1, x2, y2) of the scenario's goal_area box; tol [R] =
 *   allowed_goal_theta_difference.  Obstacles as half-plane sets a x + b y + c <= 0 (Obstacle.to_convex(margin)): hp [.][3],
 *   hp_off [n_obs_total + 1] per obstacle, route_obs_off [R + 1] = each route's obstacles.  Primitives: mp_pts
 *   [n_prim][n_pts][3], mp_len [n_prim] (total_length), cc_pts [.][2] / cc_off [n_prim + 1] = the collision-check points of each
 *   primitive in its own frame (_create_collision_points, :118-136).  wh [5] = (dist, theta, steering, obstacle, center) of the
 *   heuristic, wc [4] = (dist, steering, obstacle, center) of the edge cost (:29-33; the scenarios use the defaults
 *   (1, 2.7, 15, 0, 0) / (1, 5, 0.1, 0)).
 *   node_cap: search workspace per route in nodes, ~100 B each (16384 covers the reference's 18 standard routes a hundred
 *   times over; the longest lane change of the two-lane scenario makes 85k; a route that reports status 4 wants more).
 *   Out: status [R] (0 found; 1 no solution -- the reference raises Exception("No solution found."); 4 search workspace
 *   exhausted; 5 obstacle / primitive set too large for the kernel; 6 path longer than max_path), cost [R], n_prims [R],
 *   prims [R][max_path] (primitive index per segment), nodes [R][max_path + 1][3], traj [R][max_path * (n_pts - 1)][3] (the first
 *   n_prims * (n_pts - 1) rows are the trajectory, path_to_full_trajectory :245-257), n_expanded [R]. */
int jsim_plan_routes(int device_id, int32_t n_routes, const double *start, const double *goal, const double *goal_box,
                     const double *tol, const double *hp, const int32_t *hp_off, int32_t n_obs_total,
                     const int32_t *route_obs_off, const double *mp_pts, const double *mp_len, int32_t n_prim, int32_t n_pts,
                     const double *cc_pts, const int32_t *cc_off, const double *wh, const double *wc, int32_t max_path,
                     int32_t node_cap, int32_t *status, double *cost, int32_t *n_prims, int32_t *prims, double *nodes, double *traj,
                     int32_t *n_expanded);

/* The same search with the weights PER ROUTE: wh [R][5], wc [R][4] and form [R] in place of the launch-wide wh [5], wc [4]; every other
 * argument as in jsim_plan_routes, which is this call with its one row repeated and form 0.  Replaces one planner run per weight
 * set -- main/planner/Planner_Sensitivity_TrueCost.py / Planner_Sensitivity_Heuristic.py (a MotionPrimitiveSearch per set) and
 * main/planner/multi_trajectory_planner.py:242-269 run_all (one A* per (e, p, o) of wh_ego x wh_policy x wh_other; call site
 * main/scenarios/overtaking_cyclist_bidirectional_road.py:337) -- by one launch: the same query repeated with one row each.
 *   form [R]: 0 = the cost terms of main/lib/mp_search_ww_generic.py (:166-190 heuristic, :202-243 edge cost);
 *             1 = those of main/planner/multi_trajectory_planner.py: heuristic :185-201 = wh[0] hypot(x - gx, y - gy) +
 *                 wh[1] |((theta - gtheta) + pi) mod 2 pi - pi| + wh[2] steering_change(node, goal) (wh[3], wh[4] are not read); the
 *                 edge's obstacle term :137-141 is guarded by wc[2] != 0 (the generic file guards it by wh[3] != 0, :230) and is
 *                 1 / d for d > 0, inf otherwise.
 *   -22 before any device call for a null table, a form outside {0, 1} or a weight that is not finite. */
int jsim_plan_routes_weighted(int device_id, int32_t n_routes, const double *start, const double *goal, const double *goal_box,
                              const double *tol, const double *hp, const int32_t *hp_off, int32_t n_obs_total,
                              const int32_t *route_obs_off, const double *mp_pts, const double *mp_len, int32_t n_prim, int32_t n_pts,
                              const double *cc_pts, const int32_t *cc_off, const double *wh, const double *wc, const int32_t *form,
                              int32_t max_path, int32_t node_cap, int32_t *status, double *cost, int32_t *n_prims, int32_t *prims,
                              double *nodes, double *traj, int32_t *n_expanded);

/* ---- stakeholder reasons: score the planner's candidate trajectories and pick one, every weight row in one launch ----
 * Replaces what perform_replan does with the candidates of run_all (main/scenarios/overtaking_cyclist_bidirectional_road.py:290-407):
 * evaluate_trajectories_for_reasons (:1233-1428, weight row form 0), evaluate_trajectories_with_weights (:1641-1864, form 1) and the
 * loop of generate_stakeholder_weight_table (:1431-1604: the whole evaluation repeated once per weight triple), with
 * compute_predicted_trajectory (:244-266), calculate_trajectory_completion_time (:1867-1905), lib/trajectories.py:58-86 resample_curve,
 * lib/moving_obstacles_prediction.py:21-47 and lib/reasons_evaluation.py inside.  One workgroup per situation, one wavefront per
 * candidate; the per-sample work is done once and only the weighted sum, the balance factor and the arg-max per weight row.
 * HOST pointers in and out (a replan is an event, not a tick).
 *   cand_off [n_sit + 1]: situation s owns candidates cand_off[s] .. cand_off[s + 1] - 1 (at most JSIM_MAX_CAND); Ctot = cand_off[n_sit].
 *   pt_off [Ctot + 1], pts [.][3]: each candidate's raw (x, y, yaw) points.  mode [Ctot]: 0 = a planned candidate (resampled by the
 *   speed the ego can reach), 1 = the following candidate (last_index=True: resampled by DT v).  time_from [Ctot]: the candidate of
 *   the same situation, by index within it, whose completion time this one is scored with -- itself, or one that names itself (the
 *   reference's appended following candidate reuses the time of the candidate before it, :1257-1263).
 *   ego [n_sit][4] = x, y, yaw, v; cyc [n_sit][6] = the cyclist's get() tuple x, y, v, yaw, a, steering; now [n_sit][5] = the current
 *   policymaker, driver and cyclist values, then time_elapsed_driver and time_passed_cyclist; par [n_sit][JSIM_REASON_NPAR] in the
 *   order of the enum below.  w [n_w][3] = (policymaker, driver, cyclist) weights per row, form [n_w]: 0 = avg_policymaker over the
 *   first m - 2 samples and no clamp (:1354), 1 = over m - 1 and clamped to [0, 1] (:1785, :1815).  ideal [3] = (cyclist, driver,
 *   policymaker) ideal weights of balance_function (:1191-1231).
 *   Out: status [Ctot] (0; 2 = the reference has no defined behaviour: fewer than 2 raw points, fewer than 3 resampled ones, a
 *   completion time of fewer than 2 steps of DT or not finite, a resampling step that is not positive; 4 = more than JSIM_MAX_RES
 *   resampled points, or a prediction of more than 65536 steps), n_samples [Ctot], ct [Ctot] (the completion time used),
 *   avg [Ctot][4] = policymaker over m - 2, policymaker over m - 1, driver, cyclist; scores [n_w][Ctot]; best [n_w][n_sit] = first
 *   arg-max by index within the situation (-1: no candidate with status 0).  A candidate with a status has NaN in ct, avg and
 *   scores and never wins.  Optional (NULL: not wanted): detail [Ctot][5][JSIM_MAX_RES] = the policymaker, driver, cyclist_comfort,
 *   cyclist_time and cyclist_combined arrays of detailed_scores (m - 1, m - 1, m, m, m - 1 entries, NaN behind them),
 *   resampled [Ctot][JSIM_MAX_RES][3] (n_samples rows, NaN behind them).
 *   -22 before any device call: a null required table, offsets that do not start at 0 or decrease, more than JSIM_MAX_CAND
 *   candidates in a situation, a time_from outside its situation or naming a candidate that names another, a mode or form outside
 *   {0, 1}, a number that is not finite, DT <= 0, an ideal weight <= 0 (balance_function divides by each of them; the reference
 *   raises ZeroDivisionError on a zero). */
enum { JSIM_MAX_CAND = 8, JSIM_MAX_RES = 320 };
enum { JSIM_REASON_DT = 0, JSIM_REASON_MAX_ACCEL, JSIM_REASON_MAX_SPEED, JSIM_REASON_CENTERLINE, JSIM_REASON_WIDTH,
       JSIM_REASON_REF_D, JSIM_REASON_BUF_D, JSIM_REASON_THR_D, JSIM_REASON_REF_C, JSIM_REASON_BUF_C, JSIM_REASON_THR_C,
       JSIM_REASON_WHEELBASE, JSIM_REASON_NPAR };
int jsim_score_trajectories(int device_id, int32_t n_sit, const int32_t *cand_off, const int32_t *pt_off, const double *pts,
                            const int32_t *mode, const int32_t *time_from, const double *ego, const double *cyc, const double *now,
                            const double *par, int32_t n_w, const double *w, const int32_t *form, const double *ideal,
                            int32_t *status, int32_t *n_samples, double *ct, double *avg, double *scores, int32_t *best,
                            double *detail, double *resampled);

/* ---- stakeholder reasons per recorded tick, and the replan trigger: one pass over the History recorder's buffers ----
 * Replaces what the loop of main/scenarios/overtaking_cyclist_bidirectional_road.py does once per tick: evaluate_reasons (:127-128,
 * :2007-2027, with evaluate_distance_to_centerline, evaluate_time_following and evaluate_distance_to_obstacle of
 * lib/reasons_evaluation.py inside) and the replan trigger reasons_evaluation (:141-142, :1907-1940), and so the three series
 * save_vehicle_data (:2486) writes.  Both read only the ego's (x, y) at the start of the tick, moving_obstacles[0].get()[:2] ahead of
 * its step(), and two timers and one flag carried from the tick before: all of it is in the recorder (jsim_loop_set_recorder), so the
 * evaluation runs after the loop, on any stretch of recorded ticks.  One wavefront per ego, 64 ticks at a time; the timers are the
 * reference's additions (one `+ DT` per in-range tick, in order).  DEVICE pointers; one launch on `stream`.
 *   rec [n_ticks][B][7], flags [n_ticks][B], obs_rec [n_ticks][n_obs][6] (NULL: no ego has a cyclist): the recorder's buffers.
 *   x_first [B][4], x_spawn [B][4] (the MPC's order x, y, v, yaw): each ego's state at the start of tick 0 and its respawn state.
 *   The ego's position at the start of tick k is x_first (k = 0), x_spawn (flags[k - 1] has JSIM_REC_GOAL or JSIM_REC_AGE: the tick
 *   starts an episode) or rec[k - 1].  veh_of [B]: the vehicle of obs_rec that is the ego's moving_obstacles[0]; -1: none -- then
 *   the driver and cyclist values and the distance are NaN, the timers never advance, the policymaker value is still evaluated, and
 *   NaN never triggers.  par [B][JSIM_REASON_NPAR]: the rows of jsim_score_trajectories; DT, the centreline, the width and the six
 *   range / threshold entries are read.  threshold [B]: ReasonParameters.REASONS_THRESHOLD (0.7 in the reference).
 *   carry [B][3], in and out: time_elapsed_driver, time_passed_cyclist and replan_tracker (0 / 1) as the next tick meets them, so
 *   that a long run can be evaluated in pieces (x_first is then the state the piece starts from).  An episode's first tick starts
 *   from timers of 0 and a tracker of False, and so does the carry behind a last record that ended its episode.
 *   Out: val [n_ticks][B][4] = policymaker, driver, cyclist, distance; timers [n_ticks][B][2] = the two timers after the tick;
 *   trig [n_ticks][B]: bit 0 = replan_needed, bits 1-3 = policymaker / driver / cyclist below the threshold (the names the
 *   reference logs); first [B] = the first tick with replan_needed, or -1.
 *   Refused (-22) before any device call: B < 0, n_ticks < 0, obs_rec given with n_obs < 1, a null pointer other than obs_rec and
 *   stream, a null ctx.  n_ticks = 0 or B = 0 returns 0 and writes nothing (carry unchanged).  A veh_of >= n_obs and a DT that is not
 *   finite and positive would need a device read to detect: the Python surface (Recorder.reasons) refuses them with ValueError; the
 *   kernel treats such a veh_of as -1 and otherwise computes with what it is given. */
int jsim_loop_eval_reasons(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                           const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_of,
                           const double *par, const double *threshold, double *carry, double *val, double *timers, int32_t *trig,
                           int32_t *first, void *stream);

/* ---- clearance and first contact per recorded tick: the realised poses of a run against the vehicles it met ----
 * Answers what main/planner/moving_obstacle_avoidance.py (:44-76) asks of whole realised trajectories with
 * check_collision_moving_cars / check_collision_moving_bicycle (main/lib/collision_avoidance.py:85-166): did the ego touch a
 * vehicle, when and where, and how close did it get -- per episode of every ego, from the recorder's buffers
 * (jsim_loop_set_recorder), after the loop.  One wavefront per ego, 64 ticks at a time.  DESIGN.md section 17 is the contract.
 *   DEVICE pointers: rec [n_ticks][B][7], flags [n_ticks][B], obs_rec [n_ticks][n_obs][6], x_first [B][4], x_spawn [B][4] exactly as
 *   jsim_loop_eval_reasons takes them (the ego's pose at the start of tick k by the same rule, yaw included; a vehicle's pose is
 *   entries 0, 1 and 3 of obs_rec[k]); veh_range [B][2]: the ego's vehicles [lo, hi) among the n_obs recorded ones; mate_range
 *   [B][2]: the batch range [mlo, mhi) of its group mates, itself skipped (a mate's sample is its own start-of-tick pose); the
 *   vehicles come first, then the mates, JSIM_MAX_OBS (8) in all; and every output.
 *   HOST pointers: shapes [n_obs][4] = the rows of jsim_loop_set_vehicle_shapes (cc_front, cc_rear, radius, wheelbase; the wheelbase
 *   is not read), NULL: every vehicle has the ego's shape; ego_shape [3] = cc_front, cc_rear, radius (jsim_loop_set_geometry's
 *   values).  A vehicle's threshold is ego radius + its own radius, made here on the host together with the largest double whose
 *   square root does not exceed it, so that a row touches exactly when sqrt(dx * dx + dy * dy) <= threshold.  Mates have the ego's
 *   shape.  The table is copied to the device inside the call (one synchronising copy when shapes is given).
 *   frame_window w in [0, 20]: the rows of a tick's frame are the reference's pair table, row = ((a * n_veh + i) * (2w + 1) +
 *   (off + w)) * 2 + c (ego circle a, vehicle i, offset off, vehicle circle c), the vehicle taken at the episode's frame
 *   clamp(f - off, 0, N - 1).
 *   Out, per ego and tick [n_ticks][B]: clear = the minimum of dist - threshold over the rows with off = 0 (negative: overlap),
 *   who = that row's vehicle (the lowest row on ties), row = the frame's first touching row over all offsets or -1; without
 *   vehicles NaN / -1 / -1.  Per episode, at the slot of its first tick (every other slot -1 / -1 / NaN): hit_tick = the first
 *   tick whose frame has a touching row or -1; hit_frame and hit_xy [n_ticks][B][2] = the reference's return value for the episode
 *   (x, y, first_frame_idx): the ego's recorded pose at the earliest frame whose front circle touches the first touching row's
 *   vehicle circle, or whose rear circle does when the front one never does (`np.argmax(mask) % len`); it can precede hit_tick.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B < 0, n_ticks < 0, n_obs < 0; obs_rec NULL with
 *   n_obs > 0; frame_window outside [0, 20]; a null pointer other than obs_rec (n_obs = 0), shapes and stream; an ego radius that is
 *   not positive and finite, a circle offset or a shapes radius likewise; a null ctx.  n_ticks = 0 or B = 0 returns 0 and writes
 *   nothing.  A range outside [0, n_obs] / [0, B] or a list of more than 8 would need a device read to detect: the Python surface
 *   (Recorder.conflicts) refuses it with ValueError; the kernel clamps, so it never reads outside the tables. */
int jsim_loop_eval_conflicts(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                             const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                             const int32_t *mate_range, const double *shapes, const double *ego_shape, int32_t frame_window,
                             double *clear, int32_t *who, int32_t *row, int32_t *hit_tick, int32_t *hit_frame, double *hit_xy,
                             void *stream);

/* ---- the time gap between an ego and each vehicle per recorded tick: how close in time a pass was, and who went first ----
 * The post-encroachment time of a realised run, in ticks: for ego b, tick k and vehicle i of its list, offset `off` touches when
 * one of the four circle pairs of (the ego at tick k, vehicle i at tick k - off) touches.  off > 0: the vehicle stood in this place
 * off ticks before the ego did (the vehicle went first); off < 0: the ego went first.  It is the number that
 * check_collision_moving_cars / check_collision_moving_bicycle (main/lib/collision_avoidance.py:68-166) hold and never report: with
 * frame_window = w they test the ego's frame f against every vehicle at the frames f - w .. f + w (_offset_trajectories_by_frames),
 * and main/planner/moving_obstacle_avoidance.py:59-76 calls them on whole realised trajectories -- so an episode's smallest |off| is
 * the least frame_window at which the reference's own function reports a hit on it.  From the recorder's buffers
 * (jsim_loop_set_recorder), after the loop.  One wavefront per ego, 64 ticks at a time; the vehicles' circle centres of the ticks a
 * chunk reaches are made once per chunk and kept in LDS.  DESIGN.md section 23 is the contract.
 *   DEVICE pointers: rec, flags, obs_rec, x_first, x_spawn, veh_range, mate_range exactly as jsim_loop_eval_conflicts takes them (the
 *   same poses, the same list: the vehicles of veh_range, then the mates of mate_range with the ego itself skipped, JSIM_MAX_OBS (8)
 *   in all); and every output.  off must be 8-byte aligned (one 8-byte store per ego and tick).
 *   HOST pointers: shapes [n_obs][4] (NULL: every vehicle has the ego's shape) and ego_shape [3] as jsim_loop_eval_conflicts takes
 *   them; thresholds, circle centres and the comparison dx * dx + dy * dy <= thr_sq are that call's, operation for operation.
 *   window W in [0, JSIM_GAP_MAX_WINDOW]: the offsets -W .. W are tried.  within 0 ("episode", the reference's rule): only vehicle
 *   ticks k - off inside the ego's own episode count -- for the smallest |off| this equals the reference's clamp(f - off, 0, N - 1),
 *   a clamped row repeating a real frame pair of no larger real offset -- so that on every tick 0 <= min_i |off_i| <= w exactly
 *   when jsim_loop_eval_conflicts' row >= 0 at frame_window = w.  within 1 ("record"): every recorded tick 0 <= k - off < n_ticks
 *   counts, whatever the ego's episode: a scripted vehicle's obs_rec[k - off], a mate's own start-of-tick pose, respawns included.
 *   Out, per ego and tick: off [n_ticks][B][8] int8, byte i = the touching offset of smallest |off| of place i of the list, -o in
 *   front of +o on a tie (the reference's row order), JSIM_GAP_NONE where nothing touches within the window and for places
 *   i >= n_veh.  Per episode, at the slot of its first tick (the last record closes the running episode; every other slot
 *   -1 / -1 / -1 / JSIM_GAP_NONE), [n_ticks][B] int32 each: ep_gap = the smallest |off| over the episode's ticks and vehicles or
 *   -1, ep_tick = the first tick that has it, ep_who = the lowest place that has it on that tick, ep_off = that place's signed
 *   offset (JSIM_GAP_NONE without one).  An ego without vehicles and mates has JSIM_GAP_NONE / -1 everywhere.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: what jsim_loop_eval_conflicts refuses (B < 0,
 *   n_ticks < 0, n_obs < 0; obs_rec NULL with n_obs > 0; a null pointer other than obs_rec (n_obs = 0), shapes and stream; an ego
 *   radius that is not positive and finite, a circle offset or a shapes radius likewise; a null ctx); window outside
 *   [0, JSIM_GAP_MAX_WINDOW]; within other than 0 or 1; a null output.  n_ticks = 0 or B = 0 returns 0 and writes nothing.  A range
 *   outside its table or a list of more than 8: the kernel clamps and the Python surface (Recorder.gaps) refuses, as for
 *   jsim_loop_eval_conflicts. */
#define JSIM_GAP_NONE (-128)
#define JSIM_GAP_MAX_WINDOW 63
int jsim_loop_eval_gaps(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                        const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                        const int32_t *mate_range, const double *shapes, const double *ego_shape, int32_t window, int32_t within,
                        int8_t *off, int32_t *ep_gap, int32_t *ep_tick, int32_t *ep_who, int32_t *ep_off, void *stream);

/* ---- every recorded pose projected onto a path: progress, lateral offset, heading error ----
 * How well an ego followed the route it was given, and how far along it got and when: the question the reference answers with a
 * picture only -- plot_trajectories_comparison(..., reference_trajectory, ...) of main/scenarios/mpc_sensitivity_analysis*.py draws
 * the driven trajectories over the planned one.  (The recorder's xref_deviation is the controller's own number: the distance from
 * the first predicted state to the path point at target_ind, NaN on a failed solve.)  Per tick and episode of every ego, from the
 * recorder's buffers (jsim_loop_set_recorder), after the loop.  One wavefront per ego, 64 ticks at a time; the path's points are
 * wave-uniform scalar loads.  DESIGN.md section 24 is the contract.
 *   DEVICE pointers: rec [n_ticks][B][7], flags [n_ticks][B] as jsim_loop_eval_conflicts takes them; path_id [B] (int32); the path
 *   table px, py, pyaw, arc [n_pts] and path_off [n_paths + 1] (int64, as jsim_mpc_set_paths takes it on the host: path p is the
 *   points [path_off[p], path_off[p + 1])); and every output.  n_pts and n_paths are HOST counts.  The table is the call's own, not
 *   the context's (the context only gives the device and jsim_last_error): the engine's paths, the source paths of
 *   a fork, a lane centreline.  pyaw is the smoothed yaw as MPC.__init__ uploads it; arc is the arc length at every point, 0 at each
 *   path's first, made on the host: arc[i + 1] = arc[i] + sqrt(dx * dx + dy * dy), sequentially.
 *   The pose of tick k is rec[k] itself: x, y, yaw after the plant step (History.x[k], .y[k], .yaw[k]), not the start-of-tick pose.
 *   Per tick [n_ticks][B], with n = the points of path path_id[b] and indices relative to the path:
 *     idx (int32) = calc_nearest_index(state, cx, cy, 0) (main/lib/trajectories.py:89-97): the lowest i that minimises
 *       dx * dx + dy * dy, dx = px[i] - x, dy = py[i] - y, the sum unfused (np.argmin's first occurrence).
 *     seg (int32), t: of the segments j in {idx - 1, idx} within [0, n - 2], each from A = point j to B = point j + 1 with
 *       u = B - A, L2 = ux * ux + uy * uy, t = 0 when L2 == 0, else ((x - Ax) * ux + (y - Ay) * uy) / L2 clamped to [0, 1], foot
 *       A + t * u, q = rx * rx + ry * ry of the residual: the one with the smaller q, the lower on a tie.  n = 1: seg = 0, t = 0,
 *       the foot is the point.
 *     s (double) = arc[seg] + t * (arc[seg + 1] - arc[seg]); 0 for n = 1.
 *     d (double) = +sqrt(q) when ux * (y - Ay) - uy * (x - Ax) >= 0 (left of the direction of travel; n = 1: always), else -sqrt(q):
 *       |d| is the distance to the polyline, also beyond its ends.
 *     e_yaw (double) = ((a + pi) mod 2 pi) - pi with a = yaw - (pyaw[seg] + t * (pyaw[seg + 1] - pyaw[seg])) and Python's mod (fmod,
 *       plus 2 pi when negative).
 *     A pose that is not finite, a path_id outside [0, n_paths) or an empty path: idx = seg = -1, s = d = e_yaw = NaN.
 *   Per episode, at the slot of its first tick (the last record closes the running episode; every other slot -1 / NaN):
 *     ep_i [n_ticks][B][JSIM_TRK_NI]: TICKS, D_TICK (the first tick that holds the largest |d|, -1 without one);
 *     ep_d [n_ticks][B][JSIM_TRK_ND]: D_MAX (largest |d|), D2_MEAN (the mean of d * d over the episode's ticks that have a d, NaN
 *     without one), YAW_MAX (largest |e_yaw|), S_FIRST, S_LAST (s at the episode's first and last tick).  Maxima pass over NaN;
 *     the sum is added in a fixed order that depends on the ticks' places in their 64-tick chunks alone, so a finished episode's
 *     row does not depend on how many ticks follow it.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B, n_ticks, n_pts or n_paths < 0; a null pointer
 *   other than stream; n_paths = 0 with B > 0; a null ctx.  n_ticks = 0 or B = 0 returns 0 and writes nothing.  A path_off or
 *   path_id outside its table would need a device read to detect: the kernel clamps so that it never reads outside the tables,
 *   and the Python surface (Recorder.tracking) refuses with ValueError. */
enum { JSIM_TRK_TICKS = 0, JSIM_TRK_D_TICK, JSIM_TRK_NI };
enum { JSIM_TRK_D_MAX = 0, JSIM_TRK_D2_MEAN, JSIM_TRK_YAW_MAX, JSIM_TRK_S_FIRST, JSIM_TRK_S_LAST, JSIM_TRK_ND };
int jsim_loop_eval_tracking(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, const int32_t *path_id,
                            int32_t n_pts, const double *px, const double *py, const double *pyaw, int32_t n_paths,
                            const int64_t *path_off, const double *arc, int32_t *idx, int32_t *seg, double *s, double *d,
                            double *e_yaw, int32_t *ep_i, double *ep_d, void *stream);

/* ---- every recorded vehicle projected onto the ego's path: space headway, time headway, time to collision ----
 * How much road lay between an ego and a vehicle on the same path, and how long until it is gone: what the overtaking study
 * (main/scenarios/overtaking_cyclist_bidirectional_road.py) approximates with a Euclidean range -- create_following_trajectory keeps
 * a distance behind the cyclist, evaluate_time_following counts the time within a range of it, plot_distance draws that distance --
 * none of which is a distance along the road or tells a cyclist ahead from a car in the other lane.  Per tick, place and episode of
 * every ego, from the recorder's buffers (jsim_loop_set_recorder), after the loop.  One wavefront per ego, 64 ticks at a time; the
 * path's points are wave-uniform scalar loads and one loaded point serves every query of a group (the ego's two circle centres, then
 * the vehicles' four places to a pass, the rest in groups of 2 and 1).  DESIGN.md section 25 is the contract.
 *   DEVICE pointers: rec, flags, obs_rec, x_first, x_spawn, veh_range, mate_range exactly as jsim_loop_eval_conflicts takes them (the
 *   same list: the vehicles of veh_range, then the mates of mate_range with the ego itself skipped, JSIM_MAX_OBS (8) places in all);
 *   path_id, px, py, pyaw, path_off, arc exactly as jsim_loop_eval_tracking takes them (the table is the call's own); and every
 *   output.  HOST: n_obs, n_pts, n_paths, margin; shapes [n_obs][4] (NULL: every vehicle has the ego's shape) and ego_shape [3] as
 *   jsim_loop_eval_conflicts takes them: r_e = ego_shape[2], r_i = the vehicle's radius, thr_i = r_e + r_i made here on the host.
 *   Everything is taken at the start of tick k.  The ego's pose and speed follow the replay's rule: x_first (x, y, v, yaw) at
 *   k = 0, x_spawn behind a record that ended an episode, else rec[k - 1] (x, y, yaw, v = entries 0, 1, 2, 3); a scripted vehicle's
 *   are obs_rec[k] (x, y, v, yaw = entries 0, 1, 2, 3); a mate's are its own by the ego's rule.  Circle centres:
 *   (x + cos(yaw) * cc, y + sin(yaw) * cc) for cc_front and cc_rear, the ego's with its own shape, a vehicle's with its row of shapes
 *   (a mate, and any vehicle without a table: the ego's shape) -- jsim_loop_eval_conflicts' arithmetic, operation for operation.
 *   Each centre is projected onto path path_id[b] as jsim_loop_eval_tracking projects a pose: idx = calc_nearest_index(state, cx,
 *   cy, 0) (main/lib/trajectories.py:89-97: ascending, replaced on strict <), the segment of {idx - 1, idx} with the smaller residual
 *   (the lower on a tie), the foot clamped to it; s = the foot's arc length, d = the signed offset (left positive), ref = pyaw
 *   interpolated at the foot.  Intervals along the path: E = [min(s_front, s_rear) - r_e, max(s_front, s_rear) + r_e] of the ego,
 *   V_i likewise with r_i.  u_e = v_e * cos(yaw_e - ref) with ref at the ego's front centre's foot; u_i the same of the vehicle.
 *   Per place [n_ticks][B][8] (double; each of gap, lat, rate may be NULL only together: then none is written and every other
 *   output is the same):
 *     gap = V_i.lo - E.hi if that is > 0 (ahead), else V_i.hi - E.lo if that is < 0 (behind), else 0.0 (alongside);
 *     lat = the d of the vehicle's centre with the smaller |d|, the front centre's on a tie;
 *     rate = u_i - u_e (negative: the gap ahead closes);
 *     NaN for a place nobody holds and for a vehicle pose or speed that is not finite.
 *   A place is on the path when |lat| <= thr_i + margin.  Its ttc_i: 0 when gap == 0; gap / -rate when ahead and rate < 0;
 *   -gap / rate when behind and rate > 0; +inf when not closing; NaN off the path, absent or not finite.
 *   Per tick [n_ticks][B]: lead (int32) = the on-path place with the smallest gap >= 0, the lowest place on a tie, -1 without one;
 *   lead_gap = its gap (NaN without); thw = 0 when lead_gap == 0, lead_gap / u_e when u_e > 0, else +inf (NaN without a leader);
 *   ttc = the smallest ttc_i (NaN if every one is NaN), ttc_who (int32) = the lowest place that has it (-1); u_ego = u_e.  An ego
 *   pose or speed that is not finite, a path_id outside [0, n_paths), an empty path or an ego without vehicles and mates: -1 / NaN
 *   throughout, u_ego and the places included.
 *   Per episode, at the slot of its first tick (the last record closes the running episode; every other slot -1 / NaN):
 *     ep_i [n_ticks][B][JSIM_HW_NI]: TICKS, LEAD_TICKS (ticks with lead >= 0), GAP_TICK and GAP_WHO (the first tick that holds the
 *     smallest lead_gap and its lead), THW_TICK (the same of thw), TTC_TICK and TTC_WHO (of ttc and its ttc_who); -1 without one;
 *     ep_d [n_ticks][B][JSIM_HW_ND]: GAP_MIN, THW_MIN, TTC_MIN (minima pass over NaN; +inf counts), THW_MEAN (the mean of thw over
 *     the ticks where it is finite, NaN without one; added in a fixed order that depends on the ticks' places in their 64-tick chunks
 *     alone, so a finished episode's row does not depend on how many ticks follow it).
 *   The nearest index is global, as in jsim_loop_eval_tracking: a route that crosses itself is not served.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B, n_ticks, n_obs, n_pts or n_paths < 0; obs_rec
 *   NULL with n_obs > 0; n_paths = 0 with B > 0; a null pointer other than obs_rec (n_obs = 0), shapes, stream and the three of
 *   gap, lat, rate together; an ego radius that is not positive and finite, a circle offset or a shapes radius likewise; a margin
 *   that is not finite and >= 0; a null ctx.  n_ticks = 0 or B = 0 returns 0 and writes nothing.  A range outside its table, a list
 *   of more than 8, a path_id or a path_off outside its table would need a device read to detect: the kernel clamps so that it never
 *   reads outside the tables, and the Python surface (Recorder.headway) refuses with ValueError. */
enum { JSIM_HW_TICKS = 0, JSIM_HW_LEAD_TICKS, JSIM_HW_GAP_TICK, JSIM_HW_GAP_WHO, JSIM_HW_THW_TICK, JSIM_HW_TTC_TICK, JSIM_HW_TTC_WHO, JSIM_HW_NI };
enum { JSIM_HW_GAP_MIN = 0, JSIM_HW_THW_MIN, JSIM_HW_TTC_MIN, JSIM_HW_THW_MEAN, JSIM_HW_ND };
int jsim_loop_eval_headway(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                           const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                           const int32_t *mate_range, const double *shapes, const double *ego_shape, const int32_t *path_id,
                           int32_t n_pts, const double *px, const double *py, const double *pyaw, int32_t n_paths,
                           const int64_t *path_off, const double *arc, double margin, int32_t *lead, double *lead_gap, double *thw,
                           double *ttc, int32_t *ttc_who, double *u_ego, int32_t *ep_i, double *ep_d, double *gap, double *lat,
                           double *rate, void *stream);

/* ---- static-obstacle clearance and contact per recorded tick: the realised poses of a run against the scenario's obstacles ----
 * Answers for driven poses what the reference only asks of planned ones: check_collision (main/lib/obstacles.py:157-176) on
 * Obstacle.to_convex(margin) (:82-93 box, :134-148 circle) -- the planner's collision test, main/lib/mp_search_ww_generic.py:199-215
 * -- and BoxObstacle / CircleObstacle.distance_to_point (main/lib/obstacles.py:95-103, :150-154), at the two collision circle
 * centres of main/lib/trajectories.py:11-55 (car_trajectory_to_collision_point_trajectories) -- per tick and per episode of every
 * ego, from the recorder's buffers (jsim_loop_set_recorder), after the loop.  One wavefront per ego, 64 ticks at a time.  DESIGN.md
 * section 18 is the contract.
 *   DEVICE pointers: rec [n_ticks][B][7], flags [n_ticks][B], x_first [B][4], x_spawn [B][4] exactly as jsim_loop_eval_conflicts
 *   takes them (the ego's pose at the start of tick k by the same rule); set_of [B]: the ego's obstacle set; and every output.
 *   HOST pointers: set_off [n_sets + 1]: set s is the rows [set_off[s], set_off[s + 1]), in the order of the scenario's obstacles
 *   list (a set may be empty, its length has no cap); rows [n_rows][JSIM_STATIC_ROW]: per obstacle 0 kind (0 box, 1 circle), 1 hidden
 *   (0 / 1), 2 n_hp (1..8), 3-6 geometry (box: x1, y1, x2, y2; circle: cx, cy, r, 0), 7 reserved, 8-31 the half-planes [8][3] =
 *   (a, b, c) of to_convex(margin) in the reference's row order; ego_shape [3] = cc_front, cc_rear, radius (jsim_loop_set_geometry's
 *   values).  The tables are checked on the host and copied to the device inside the call (one synchronising copy).
 *   include_hidden 0: rows whose hidden entry is 1 are skipped, for touch and clearance alike (their indices still count).
 *   Out, per ego and tick [n_ticks][B]: clear = the minimum over the included obstacles and the two circle centres of
 *   distance_to_point(centre) - radius (-radius where a centre lies inside an obstacle), who = that obstacle's place in its set (the
 *   lowest on ties), hit = the lowest place of an obstacle for which, at one of the two centres, every half-plane has
 *   (a * x + b * y) + c <= 0 (the sum unfused, in that order), or -1; without an included obstacle NaN / -1 / -1.  Per episode, at the
 *   slot of its first tick (every other slot -1): off_tick = the first tick of the episode with hit >= 0, or -1.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B, n_ticks, n_sets or n_rows < 0; include_hidden not 0
 *   or 1; a null pointer other than stream (set_off and rows may be NULL with n_sets = 0 only); an ego radius that is not positive
 *   and finite, a circle offset that is not finite; offsets that do not start at 0, that decrease or that do not end at n_rows; a
 *   row with a kind or hidden entry other than 0 / 1, n_hp outside 1..8, a geometry or used half-plane entry that is not finite, a
 *   circle radius <= 0, a box with x1 > x2 or y1 > y2; a null ctx.  n_ticks = 0 or B = 0 returns 0 and writes nothing.  A set_of
 *   outside [0, n_sets) would need a device read to detect: the kernel treats it as an empty set, and the Python surface
 *   (Recorder.static_conflicts) refuses it with ValueError. */
enum { JSIM_STATIC_ROW = 32 };
int jsim_loop_eval_static(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, const double *x_first,
                          const double *x_spawn, const int32_t *set_of, int32_t n_sets, const int32_t *set_off, int32_t n_rows,
                          const double *rows, const double *ego_shape, int32_t include_hidden, double *clear, int32_t *who, int32_t *hit,
                          int32_t *off_tick, void *stream);

/* ---- one row per recorded episode ----
 * What a sweep asks of every episode -- did the ego arrive, how long did it take, how far did it drive and deviate, how close did
 * it come, did it touch, did it leave the road, did the replan trigger fire -- as a segmented reduction over the recorder's
 * buffers (jsim_loop_set_recorder) and over the per-tick outputs of the three jsim_loop_eval_* calls, all of which stay on the
 * device: three launches on `stream` (count, scan, summary), one wavefront per ego, 64 ticks at a time.  DESIGN.md section 19 is
 * the contract.
 *   DEVICE pointers, all of them.  rec [n_ticks][B][7], flags [n_ticks][B], x_first [B][4], x_spawn [B][4] exactly as the
 *   jsim_loop_eval_* calls take them.  Three optional groups, each NULL as a whole or given as a whole: veh_clear, veh_who,
 *   veh_hit_tick, veh_hit_frame [n_ticks][B] and veh_hit_xy [n_ticks][B][2] (jsim_loop_eval_conflicts' clear, who, hit_tick,
 *   hit_frame, hit_xy); st_clear, st_who, st_hit, st_off_tick [n_ticks][B] (jsim_loop_eval_static's clear, who, hit, off_tick);
 *   rs_val [n_ticks][B][4] and rs_trig [n_ticks][B] (jsim_loop_eval_reasons' val and trig).
 *   Episodes, per ego: a record whose flag has JSIM_REC_GOAL or JSIM_REC_AGE ends one (both bits: GOAL), the next tick starts one;
 *   the last episode is the running one and is always there, with no tick when the last record ended the one before: an ego has
 *   (its end flags) + 1 episodes.
 *   Out: ep_off [B + 1] (int64): the row of ego b's first episode, ep_off[B] the number of rows; rows ego-major, an ego's in
 *   order of time; ep_i [ep_cap][JSIM_EP_NI] and ep_d [ep_cap][JSIM_EP_ND], columns by the enumerators below.  Rows at or beyond
 *   ep_cap are not written; ep_off is complete in any case (ep_off[B] > ep_cap: the cap was too small).
 *   Integer columns: EGO; K0, N (first tick, ticks); END (0 running, 1 goal, 2 age); FAILED (ticks with JSIM_REC_FAILED); DEV_TICK
 *   (first tick of the largest xref_deviation); VEH_TICK (first tick of the smallest veh_clear), VEH_WHO (veh_who there),
 *   VEH_HIT_TICK, VEH_HIT_FRAME (copied from slot K0); ST_TICK, ST_WHO (likewise for st_clear), ST_OFF_TICK (copied from slot K0),
 *   ST_OBSTACLE (st_hit at ST_OFF_TICK; -1 when that is outside [0, n_ticks)), ST_TICKS_OFF (ticks with st_hit >= 0); REPLAN_TICK
 *   (first tick with rs_trig & 1).
 *   Double columns: LENGTH (the sum over the ticks of sqrt(dx * dx + dy * dy), unfused, from the start-of-tick pose -- x_first for
 *   tick 0, x_spawn behind an end flag, else rec[k - 1] -- to rec[k]); V_MEAN, V_MAX; A_MIN, A_MAX; DELTA_ABSMAX; DEV_MAX and
 *   DEV_MEAN (xref_deviation; the mean over the ticks whose deviation is not NaN); VEH_CLEAR (smallest), VEH_HIT_X, VEH_HIT_Y
 *   (copied from slot K0); ST_CLEAR (smallest); PM_MIN, DRIVER_MIN, CYCLIST_MIN, DIST_MIN (minima of rs_val's entries).
 *   Minima and maxima pass over NaN and compare numerically, their tick is the first that holds the value; nothing but NaN gives
 *   NaN / -1; a NULL group gives NaN / -1 / 0 in its columns; an episode without a tick gives NaN / -1 / 0 in every column but
 *   EGO, K0, N, END.  Integer columns, minima, maxima and copies are exact; the three sums are added in a fixed order that depends
 *   on the ticks' places in their 64-tick chunks alone, so a finished episode's row does not depend on how many ticks follow it.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B, n_ticks or ep_cap < 0; a group given in part; a
 *   null rec, flags, x_first, x_spawn, ep_off, ep_i or ep_d; a null ctx.  n_ticks = 0 writes one running episode without a tick
 *   per ego; B = 0 writes ep_off[0] = 0. */
enum { JSIM_EP_EGO = 0, JSIM_EP_K0, JSIM_EP_N, JSIM_EP_END, JSIM_EP_FAILED, JSIM_EP_DEV_TICK, JSIM_EP_VEH_TICK, JSIM_EP_VEH_WHO,
       JSIM_EP_VEH_HIT_TICK, JSIM_EP_VEH_HIT_FRAME, JSIM_EP_ST_TICK, JSIM_EP_ST_WHO, JSIM_EP_ST_OFF_TICK, JSIM_EP_ST_OBSTACLE,
       JSIM_EP_ST_TICKS_OFF, JSIM_EP_REPLAN_TICK, JSIM_EP_NI };
enum { JSIM_EP_LENGTH = 0, JSIM_EP_V_MEAN, JSIM_EP_V_MAX, JSIM_EP_A_MIN, JSIM_EP_A_MAX, JSIM_EP_DELTA_ABSMAX, JSIM_EP_DEV_MAX,
       JSIM_EP_DEV_MEAN, JSIM_EP_VEH_CLEAR, JSIM_EP_VEH_HIT_X, JSIM_EP_VEH_HIT_Y, JSIM_EP_ST_CLEAR, JSIM_EP_PM_MIN,
       JSIM_EP_DRIVER_MIN, JSIM_EP_CYCLIST_MIN, JSIM_EP_DIST_MIN, JSIM_EP_ND };
int jsim_loop_summarise_episodes(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                                 const double *x_first, const double *x_spawn, const double *veh_clear, const int32_t *veh_who,
                                 const int32_t *veh_hit_tick, const int32_t *veh_hit_frame, const double *veh_hit_xy,
                                 const double *st_clear, const int32_t *st_who, const int32_t *st_hit, const int32_t *st_off_tick,
                                 const double *rs_val, const int32_t *rs_trig, int32_t ep_cap, int64_t *ep_off, int32_t *ep_i,
                                 double *ep_d, void *stream);

/* ---- the collision cut-off of every recorded tick: what the glue ahead of MPC.step decided, rebuilt from the recorder ----
 * Each tick the reference's loops (main/scenarios/mpc_intersection.py:104-143, interactive_mpc.py and
 * overtaking_cyclist_bidirectional_road.py:111-169) find the progress index, resample the remaining path, predict the traffic, run
 * check_collision_moving_cars / check_collision_moving_bicycle and cut the path off before the predicted collision
 * (get_cutoff_curve_by_position_idx(...) - EXTRA_CUTOFF_MARGIN); visualize_frame shows the results (collision_xy, tmp_trajectory).
 * The fused loops compute them every tick and keep the last tick's only.  This call computes them again for every recorded tick,
 * after the run and without touching the loops' kernels: per tick it calls the loops' own device function on the ego's tick-start
 * state (x_first, x_spawn behind a record with JSIM_REC_GOAL / JSIM_REC_AGE, else rec[k - 1]: x, y, v, yaw), the vehicles' recorded
 * get() tuples of the tick (predicted again) and, for interacting egos, its group mates' tick-start states and the steering of
 * their records before (0 on tick 0 and behind a respawn; predicted again), so every value equals the live loop's bit for bit.
 * One wavefront per ego walks the ticks in order, in chunks of chunk_ticks ticks (0: as many as a 512 MiB budget of predictions
 * holds, the budget of the fused run's traffic chunks).  DESIGN.md section 21 is the contract.
 *   DEVICE pointers: rec [n_ticks][B][7], flags [n_ticks][B], obs_rec [n_ticks][n_obs][6], x_first [B][4], x_spawn [B][4] exactly as
 *   jsim_loop_eval_conflicts takes them; carry; and every output.
 *   frame_window, margin, n_steps, speed_cutoff (0 / 1): the glue arguments of the run that was recorded (jsim_loop_run_scenario);
 *   interacting 1: the run was jsim_loop_run_interacting's (the ego's obstacles are its vehicles, then its group mates).
 *   Everything else is read from the context as the loops read it, so the context must still hold the recorded loop's tables: the
 *   paths and their circle centres, the path ids of the egos as the last glue call took them (jsim_loop_run_scenario,
 *   jsim_loop_run_interacting, jsim_loop_pre_tick; the caller's device array, which must still be alive), the geometry, the
 *   limits of its configuration, the traffic layout, the vehicle shapes and the groups.
 *   Out, per ego and tick [n_ticks][B] (int32): status = the glue's pre_status of the tick; idx = the progress index after the
 *   tick's update; cut = what the loop wrote to path_len, or with speed_cutoff = 1 to the speed cut-off buffer; hit = 0 / 1; first
 *   = the index of the hit on the remaining path (jsim_loop_pre_tick's first_idx), -1 without a hit; col_xy [n_ticks][B][2] = the
 *   collision point, NaN without a hit.  A tick whose status is not 0 leaves idx and cut as they were and has hit = 0.
 *   first_tick: the ticks [first_tick, n_ticks) are evaluated and their rows of the outputs written (the buffers are those of the
 *   whole recording in any case: tick first_tick - 1's record gives the states and the steering tick first_tick starts from).
 *   carry [B][3] (int32), in and out: the progress index, the length of the previous tick's path (-1: none) and the current
 *   cut-off as tick first_tick meets them and as tick n_ticks would, so that a run can be evaluated in pieces.  NULL: the loops'
 *   own start -- 0, -1 and the full path length.  These three integers are all the state the glue carries from tick to tick, so,
 *   unlike the frame offsets of jsim_loop_eval_conflicts, a cut between any two ticks is exact.
 *   Refused (-22) before any device call, jsim_last_error naming the argument: B, n_ticks, n_obs, margin or chunk_ticks < 0; a
 *   first_tick outside [0, n_ticks]; obs_rec NULL with n_obs > 0; n_steps outside [1, 64]; frame_window outside [0, 32];
 *   speed_cutoff or interacting other than 0 / 1, or both 1; a null pointer other than obs_rec (n_obs = 0), carry and stream; a
 *   null ctx; a context without paths or geometry, or, with ticks to evaluate, without a glue call; an n_obs that is not the
 *   registered traffic total (a B that is not the layout's), or above 8 without a layout; interacting = 1 without registered
 *   groups for B, or with more vehicles and mates than 8; speed_cutoff = 1 without a registered speed cut-off
 *   (jsim_mpc_set_speed_cutoff); an n_obs that is not the shape table's.  first_tick = n_ticks (so n_ticks = 0) or B = 0 returns
 *   0 and writes nothing (carry unchanged). */
int jsim_loop_eval_cutoffs(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                           const double *obs_rec, const double *x_first, const double *x_spawn, int32_t frame_window, int32_t margin,
                           int32_t n_steps, int32_t speed_cutoff, int32_t interacting, int32_t chunk_ticks, int32_t first_tick,
                           int32_t *carry, int32_t *status, int32_t *idx, int32_t *cut, int32_t *hit, int32_t *first, double *col_xy,
                           void *stream);

/* ---- Forking a recorded run: the start of a new loop at any recorded tick ----
 * What perform_replan of main/scenarios/overtaking_cyclist_bidirectional_road.py (:394-402) has for nothing -- the same simulation and
 * the same cyclist going on under a new MPC object -- for a run that is over: a new loop (a new context, new paths, a cold controller)
 * whose rows start where egos of the recorded run stood at ticks of their own, meeting the scripted vehicles where they stood then.
 *
 * jsim_loop_fork_state: row r's state x0[r] = (x, y, v, yaw) of ego ego[r] at the start of tick at[r] -- x_first on tick 0, x_spawn
 * behind a record with JSIM_REC_GOAL / JSIM_REC_AGE, else the record before (the rule of jsim_loop_eval_cutoffs, by the same device
 * function) -- and k0[r], the first tick of the episode that tick belongs to: 0, or one behind the last record before at[r] with
 * JSIM_REC_GOAL or JSIM_REC_AGE (so at[r] - k0[r] is the ego's age there).  at[r] = n_ticks is the state after the last record.  One
 * ego may stand in any number of rows.  A pure function of the recorder's buffers; one wavefront per row.
 *   DEVICE pointers: rec [n_ticks][B][7], flags [n_ticks][B], x_first [B][4], x_spawn [B][4] as jsim_loop_eval_cutoffs takes them,
 *   x0 [n_rows][4], k0 [n_rows] (int32).  HOST pointers: ego [n_rows], at [n_rows].
 *   Refused (-22) before any device call: B, n_ticks or n_rows < 0; with n_rows > 0 a null pointer other than stream, an ego outside
 *   [0, B), an at outside [0, n_ticks]; a null ctx.  n_rows = 0 returns 0 and writes nothing.
 *
 * jsim_loop_obstacles_at: vehicle o's state[o] = (xc, yc, theta, counter) after ticks[o] ticks from state0[o], each tick being the
 * loops' two calls -- get() alone, then get() + step() (jsim_loop_obstacles with do_step 0, then 1; jsim_loop_run_scenario's
 * roll-forward) -- by the same device function, so the result is the live loop's obs_state bit for bit, the heading the roundabout
 * rule rewrites and the start-delay counter included.  Nothing else is written.  One thread per vehicle; n_obs has no limit of 8.
 *   DEVICE pointers: state0 [n_obs][4], param [n_obs][8] (jsim_loop_obstacles' layouts), wheelbase [n_obs] (NULL: every vehicle has the
 *   wheelbase jsim_loop_obstacles steps with: jsim_loop_set_obstacle_geometry's, else the configuration's L), state [n_obs][4].
 *   HOST pointer: ticks [n_obs].
 *   Refused (-22) before any device call: n_obs < 0; with n_obs > 0 a null pointer other than wheelbase and stream, a ticks[o] < 0;
 *   a null ctx.  n_obs = 0 returns 0 and writes nothing. */
int jsim_loop_fork_state(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, const double *x_first,
                         const double *x_spawn, int32_t n_rows, const int32_t *ego, const int32_t *at, double *x0, int32_t *k0,
                         void *stream);
int jsim_loop_obstacles_at(jsim_ctx *ctx, int32_t n_obs, const double *state0, const double *param, const double *wheelbase,
                           const int32_t *ticks, double *state, void *stream);

/* ---- every recorded prediction against what the vehicle then did ----
 * Every cut-off of the loops rests on MovingObstaclesPrediction(x, y, v, yaw, a, steer) of main/lib/moving_obstacles_prediction.py:
 * the vehicle held on a constant arc for n_steps * dt seconds.  After a run the recorder holds the exact input of every such
 * prediction and what the vehicle did next; this call gives the displacement error of each, in one launch, one wavefront per row,
 * without writing a prediction to memory.
 *   Rows: V = n_obs + (egos ? B : 0).  Row r < n_obs is recorded vehicle r, in the recorder's order (every vehicle of every set under
 *   a traffic layout); row n_obs + b is ego b under the constant rule (JSIM_MATE_CONSTANT).
 *   Input of tick k.  Vehicle: obs_rec[k][r] = (x, y, v, yaw, a, steer).  Ego: (x, y, v, yaw) at the start of tick k -- x_first on tick
 *   0, x_spawn behind a record with JSIM_REC_GOAL / JSIM_REC_AGE, else the record before, as jsim_loop_eval_cutoffs reads it --, a = 0,
 *   steer = field 4 of record k - 1, or 0 when k = 0 or record k - 1 ended an episode: what jsim_loop_run_interacting hands the
 *   constant rule and jsim_loop_eval_cutoffs hands it again.
 *   Prediction: tn = tan(steer); per step  x += v * cos(yaw) * dt;  y += v * sin(yaw) * dt;  v += a * dt;  yaw += (v / L) * tn * dt
 *   (unfused, in that order; the device function of jsim_loop_predict_obstacles, bit for bit).  dt is the context's; L is the
 *   vehicle's row of jsim_loop_set_vehicle_shapes, else jsim_loop_set_obstacle_geometry's wheelbase, else the configuration's L; an
 *   ego's is the configuration's L.  Sample j (from 0) is the pose after step j: (j + 1) * dt ahead.
 *   Truth of sample j.  Vehicle: fields 0, 1, 3 of obs_rec[k + j + 1][r]; it exists iff k + j + 1 <= n_ticks - 1.  Ego: fields 0, 1, 2 of
 *   rec[k + j][b] (the pose after that tick's plant step, before any respawn); it exists iff k + j <= ke(k), the first tick >= k whose
 *   record has JSIM_REC_GOAL | JSIM_REC_AGE, or n_ticks - 1 without one.  m = the scored samples: min(n_steps, n_ticks - 1 - k) for a
 *   vehicle, min(n_steps, ke - k + 1) for an ego.
 *   Out, per tick and row, with (dx, dy) = prediction - truth and e_j = sqrt(dx * dx + dy * dy) (unfused):
 *     pt_i [n_ticks][V][JSIM_PS_NI]: N = m; HOLD = the leading samples with e_j <= tol (m when none exceeds it); MAX_AT = the first j
 *     of the largest e_j;
 *     pt_d [n_ticks][V][JSIM_PS_ND]: ADE = (e_0 + e_1 + ... in step order) / m; FDE = e_(m-1); MAX; LON and LAT at sample m - 1 against
 *     the truth heading psi: LON = dx * cos(psi) + dy * sin(psi) (> 0: predicted farther ahead than the vehicle got), LAT =
 *     -dx * sin(psi) + dy * cos(psi); YAW = (yaw_pred - psi) wrapped to [-pi, pi) as jsim_loop_eval_tracking wraps e_yaw.
 *     With m = 0 the row holds 0, 0, -1 and NaN.
 *   Per row over all ticks: step_sum [V][n_steps] = the sum of e_j over the ticks that score sample j (added in a fixed order: the
 *   same call gives the same bits), step_cnt [V][n_steps] (int32) = how many do.  err [n_ticks][V][n_steps], which may be NULL: every
 *   e_j, NaN where a sample is not scored.
 *   DEVICE pointers throughout, as for jsim_loop_eval_cutoffs; HOST counts, egos (0 / 1) and tol.
 *   Refused (-22) before any device call and with nothing written: B, n_ticks or n_obs < 0; n_steps outside [1, 64]; egos other than
 *   0 / 1; a tol that is negative or not finite; obs_rec NULL with n_obs > 0; any other null pointer but err and stream; a null ctx; an
 *   n_obs that is not the registered traffic total (a B that is not the layout's) or not the shape table's.  V = 0 or n_ticks = 0
 *   returns 0 and writes nothing. */
enum { JSIM_PS_N = 0, JSIM_PS_HOLD, JSIM_PS_MAX_AT, JSIM_PS_NI };
enum { JSIM_PS_ADE = 0, JSIM_PS_FDE, JSIM_PS_MAX, JSIM_PS_LON, JSIM_PS_LAT, JSIM_PS_YAW, JSIM_PS_ND };
int jsim_loop_score_predictions(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                const double *obs_rec, const double *x_first, const double *x_spawn, int32_t egos, int32_t n_steps,
                                double tol, int32_t *pt_i, double *pt_d, double *step_sum, int32_t *step_cnt, double *err, void *stream);

/* ---- the shared plans of every tick: recorded, scored and replayed ----
 * Under JSIM_MATE_PLAN an ego is predicted from the controls its controller holds, and after a run nobody could say what those were.
 * jsim_loop_set_plan_recorder: caller-owned DEVICE buffers beside the registered recorder's, of its B and cap; cap = 0 clears.
 *   While registered, jsim_loop_run_interacting (under either mate prediction; no other entry point) writes slot k = the device
 *   tick counter at the start of the tick -- the slot the tick's History record goes to; slots k >= cap are dropped:
 *   plan_oa [cap][B][T], plan_od [cap][B][T] = oa, od and plan_status [cap][B] (int32) = status as the engine holds them at the
 *   start of the tick, before that tick's solve: what THE RULE above reads.  T is the context's.  The steering applied last tick is
 *   not recorded: it is field 4 of record k - 1, or 0 on tick 0 and behind a record with JSIM_REC_GOAL / JSIM_REC_AGE.  A slab of C
 *   consecutive ticks is a [C * B][T] batch for jsim_loop_predict_egos_plan, row = tick * B + ego.  The run itself is not changed.
 *   Refused (-22), nothing changed: B < 0, cap < 0, cap > 0 with a null buffer, a null ctx, cap > 0 with a B or cap that is not the
 *   registered recorder's (or without one).  jsim_loop_set_recorder, registering or clearing, clears the plan recorder too.
 *
 * jsim_loop_score_plan_predictions: jsim_loop_score_predictions for the egos under THE RULE.  Rows are the B egos.  For tick k and
 *   ego b: the state (x, y, v, yaw) at the start of tick k as jsim_loop_score_predictions reads an ego's; ok = plan_status[k][b] ==
 *   JSIM_OK; delta_last = field 4 of record k - 1, or 0 when k = 0 or record k - 1 ended an episode.  Step i = 0 .. n_steps - 1, with
 *   j = i + 1:  a_i = (ok && j < T) ? plan_oa[k][b][j] : 0;  delta_i = ok ? plan_od[k][b][min(j, T - 1)] : delta_last, clamped to
 *   +-max_steer;  vb = v;  x += vb * cos(yaw) * dt;  y += vb * sin(yaw) * dt;  yaw += (vb / L) * tan(delta_i) * dt;  v += a_i * dt;
 *   v = max_speed < v ? max_speed : v;  v = min_speed > v ? min_speed : v  (unfused, in that order: the samples are
 *   jsim_loop_predict_egos_plan's pred bit for bit).  T, dt, L, max_steer, max_speed and min_speed are the context's.
 *   Truth, m and every output are jsim_loop_score_predictions' for an ego row, with V = B: pt_i [n_ticks][B][JSIM_PS_NI], pt_d
 *   [n_ticks][B][JSIM_PS_ND], step_sum and step_cnt [B][n_steps], err [n_ticks][B][n_steps] or NULL.  One launch, one wavefront per
 *   ego, no prediction written to memory; step_sum is added in a fixed order: the same call gives the same bits.
 *   DEVICE pointers throughout: rec, flags, x_first, x_spawn as jsim_loop_score_predictions takes them, plan_oa, plan_od
 *   [n_ticks][B][T] and plan_status [n_ticks][B] as the plan recorder wrote them.  HOST counts and tol.
 *   Refused (-22) before any device call and with nothing written: B or n_ticks < 0; n_steps outside [1, 64]; a tol that is negative
 *   or not finite; any null pointer but err and stream; a null ctx.  B = 0 or n_ticks = 0 returns 0 and writes nothing.
 *
 * jsim_loop_eval_cutoffs_plan: jsim_loop_eval_cutoffs for a run under JSIM_MATE_PLAN: its arguments, then plan_oa, plan_od and
 *   plan_status as above (DEVICE, [n_ticks][B][T] and [n_ticks][B]: the buffers of the whole recording, like rec).  The group mates of
 *   every tick are predicted again by the kernel of jsim_loop_predict_egos_plan from the tick-start states, the recorded plans and
 *   delta_last; everything else is jsim_loop_eval_cutoffs, whose refusals hold, and: a null plan pointer; interacting = 0. */
int jsim_loop_set_plan_recorder(jsim_ctx *ctx, int32_t B, int32_t cap, double *plan_oa, double *plan_od, int32_t *plan_status);
int jsim_loop_score_plan_predictions(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                                     const double *x_first, const double *x_spawn, const double *plan_oa, const double *plan_od,
                                     const int32_t *plan_status, int32_t n_steps, double tol, int32_t *pt_i, double *pt_d,
                                     double *step_sum, int32_t *step_cnt, double *err, void *stream);
int jsim_loop_eval_cutoffs_plan(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                const double *obs_rec, const double *x_first, const double *x_spawn, int32_t frame_window, int32_t margin,
                                int32_t n_steps, int32_t speed_cutoff, int32_t interacting, int32_t chunk_ticks, int32_t first_tick,
                                int32_t *carry, int32_t *status, int32_t *idx, int32_t *cut, int32_t *hit, int32_t *first, double *col_xy,
                                const double *plan_oa, const double *plan_od, const int32_t *plan_status, void *stream);

/* ---- checkpoints of a running loop: rewind it, continue it elsewhere, fork it warm ----
 * All live state of a loop sits in caller-owned DEVICE arrays; the context holds tables only.  A checkpoint is a copy of those arrays
 * (the caller's list: closed_loop.py states it in history.CHECKPOINT) into slot s of caller-owned slabs [n_slots]..., taken between
 * two calls of a loop entry point; no loop kernel knows of it.
 *
 * jsim_loop_checkpoint_save: n_arrays copies, bytes[i] bytes from src[i] to dst[i], in ONE launch on `stream` (plain vector stores, 16
 *   bytes a thread where the pointers and the size allow it).  Saving slot s: src[i] = the live array, dst[i] = slab i + s * its slot
 *   size; restoring it: the same call with src and dst exchanged.  The table travels in the kernel's arguments: the call neither
 *   allocates nor synchronises, so it may stand between two fused launches on one stream.
 *   HOST arrays src, dst [n_arrays] of DEVICE pointers and bytes [n_arrays].
 *   Refused (-22) before any device call: n_arrays outside [0, JSIM_CKPT_MAX_ARRAYS]; with n_arrays > 0 a null array or a null entry;
 *   a bytes[i] that is negative or no multiple of 4; a pointer that is not 4-byte aligned; a null ctx.  n_arrays = 0 returns 0.
 *
 * jsim_loop_checkpoint_load: rows of written slots gathered into the arrays of a NEW loop (ctx is the new loop's).  Destination row
 *   r takes ego ego[r] of slot slot[r]: for every field i, row_bytes[i] bytes from slab[i] + (slot[r] * B + ego[r]) * row_bytes[i] to
 *   dst[i] + r * row_bytes[i].  One wavefront per row, the lanes side by side over the row's 4-byte words (the T doubles of oa and od:
 *   2 T lanes; a scalar: lane 0).  A second grid copies the scripted vehicles: destination vehicle o takes the 4 doubles (xc, yc,
 *   theta, counter) of vehicle veh_src[o] of slot veh_slot[o] from obs_slab [n_slots][n_obs][4] to obs_state [n_veh][4].  One ego and
 *   one vehicle may stand in any number of rows.  B and n_obs are the SOURCE loop's.
 *   HOST arrays: written [n_slots] (nonzero: the slot holds a checkpoint), ego, slot [n_rows], slab, dst [n_fields] (DEVICE
 *   pointers), row_bytes [n_fields], veh_src, veh_slot [n_veh].  DEVICE: the slabs, the destinations, obs_slab, obs_state.
 *   Refused (-22) before any device call: a negative size; n_fields > JSIM_CKPT_MAX_ARRAYS; a null pointer that a positive size
 *   needs; an ego outside [0, B); a slot or veh_slot outside [0, n_slots) or not written; a veh_src outside [0, n_obs); a row_bytes
 *   that is not a positive multiple of 4, a slab or dst that is not 4-byte aligned; a null ctx.  Nothing to copy returns 0. */
enum { JSIM_CKPT_MAX_ARRAYS = 32 };
int jsim_loop_checkpoint_save(jsim_ctx *ctx, int32_t n_arrays, const void *const *src, void *const *dst, const int64_t *bytes,
                              void *stream);
int jsim_loop_checkpoint_load(jsim_ctx *ctx, int32_t B, int32_t n_slots, const int32_t *written, int32_t n_rows, const int32_t *ego,
                              const int32_t *slot, int32_t n_fields, const void *const *slab, void *const *dst, const int64_t *row_bytes,
                              int32_t n_obs, const double *obs_slab, int32_t n_veh, const int32_t *veh_src, const int32_t *veh_slot,
                              double *obs_state, void *stream);

/* ---- the job's one exchange: the final trajectory gather over RCCL / xGMI ----
 * The reference has no multi-process code at all (its only multi-ego code is the serial Python loop of
 * main/scenarios/interactive_mpc.py:119-172); egos are independent (main/lib/mpc.py:141-211), so ranks own contiguous shards
 * of the ego batch and exchange nothing while solving.  These four calls are the gather of the per-rank result blocks:
 *   jsim_comm_unique_id: fills a 128-byte ncclUniqueId (rank 0 calls it and hands the bytes to the other ranks by any means).
 *   jsim_comm_init:      ncclCommInitRank on the context's device; the communicator then belongs to the context.
 *   jsim_mpc_gather:     ncclAllGather of bytes_per_rank bytes from `local` into `out` [n_ranks * bytes_per_rank] (DEVICE pointers)
 *                        on `stream`; comm == NULL uses the context's communicator, otherwise a caller-owned ncclComm_t.
 *   jsim_comm_destroy:   ncclCommDestroy (also done by jsim_mpc_destroy).
 * librccl is loaded on first use (dlopen; override with JSIM_RCCL_LIB): libjsim_mpc.so itself links only libamdhip64. */
int jsim_comm_unique_id(void *id128);
int jsim_comm_init(jsim_ctx *ctx, const void *id128, int32_t n_ranks, int32_t rank);
int jsim_mpc_gather(jsim_ctx *ctx, void *comm, const void *local, void *out, size_t bytes_per_rank, void *stream);
int jsim_comm_destroy(jsim_ctx *ctx);

/* deviation [B] (needs ox[b][0], oy[b][0]) and is_goal [B] (int32 0/1); goal = last point of the FULL path. */
int jsim_mpc_xref_deviation_goal(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                                 const int32_t *path_len, const int64_t *target_ind, const double *ox,
                                 const double *oy, double *deviation, int32_t *is_goal, void *stream);

#ifdef __cplusplus
}
#endif
#endif
