// The collision cut-off of every recorded tick (DESIGN.md section 21): what the glue ahead of MPC.step decided on each tick of a
// run -- main/scenarios/mpc_intersection.py:104-143, interactive_mpc.py and overtaking_cyclist_bidirectional_road.py:111-169: the
// progress index, whether check_collision_moving_cars / check_collision_moving_bicycle found a predicted collision, where, and the
// index the path was cut off at -- rebuilt after the run from the History recorder's buffers (jsim_loop_set_recorder) by calling
// jsim_pre_tick_ego, the function the loops call, on each tick's inputs.  Those are the ego's tick-start state (recorder_walk.inc's
// rule, with v), the vehicles' get() tuples of the tick (predicted again by obstacle_predict_kernel), for interacting egos the
// mates' tick-start states and last applied steering (predicted again by ego_predict_kernel), and three integers carried from
// tick to tick.  One wavefront per ego walks the ticks of a chunk in order; the loops' kernels are not touched.

enum { JSIM_CUT_CARRY = 3 }; // traj_idx, prev_len, cur_len

struct CutoffP {
    RecorderBuf R;
    PreP pre;                 // the glue's constants and tables; pre.n_obs = all recorded vehicles
    TrafficP X;
    GroupP G;                 // interacting: G.ego_cc / G.ego_bc hold the chunk's [C][B] predictions of the tick-start states
    int k0, C;                // the chunk: ticks [k0, k0 + C)
    int speed_cutoff, interacting;
    const double2 *pred_cc;   // [C][n_obs][n_steps][2] the vehicles' predictions of the chunk's ticks
    const double4 *pred_bc;   // [C][n_obs]
    int *carry;               // [B][JSIM_CUT_CARRY] in / out
    int *status, *idx, *cut, *hit, *first; // [n][B]
    double *col_xy;           // [n][B][2]
};

// (jct_state_at, an ego's state at the start of tick k, stands in recorder_walk.inc beside jrw_pose_at, whose rule it is)

// A NULL carry of the caller: the loops' own start -- progress index 0, no previous path (PreTick.__init__), the whole path
__global__ __launch_bounds__(256) void cutoff_carry_init_kernel(int B, const int *path_id, const long long *poff, int *carry)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int pid = path_id[b];
    carry[3 * b] = 0; carry[3 * b + 1] = -1; carry[3 * b + 2] = (int)(poff[pid + 1] - poff[pid]);
}

// Interacting egos: what ego_predict_kernel reads, for every ego and tick of the chunk as one flat batch of C * B rows (row =
// tick * B + ego): the tick-start state, and (delta, 0) with the delta the ego applied on the tick before -- its record's, which
// after a failed solve is the delta before that, as di_ai holds it (select_di_ai) -- or 0 on tick 0 and behind a respawn
__global__ __launch_bounds__(256) void cutoff_mate_state_kernel(RecorderBuf R, int k0, int C, double *x0, double *di_ai)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (size_t)C * R.B) return;
    const int t = (int)(r / R.B), e = (int)(r % R.B), k = k0 + t;
    double x, y, v, yaw;
    jct_state_at(R, e, k, x, y, v, yaw);
    x0[4 * r] = x; x0[4 * r + 1] = y; x0[4 * r + 2] = v; x0[4 * r + 3] = yaw;
    const bool fresh = k == 0 || jrw_is_end(R.flags[(size_t)(k - 1) * R.B + e]);
    di_ai[2 * r] = fresh ? 0.0 : R.rec[JSIM_REC_FIELDS * ((size_t)(k - 1) * R.B + e) + 4];
    di_ai[2 * r + 1] = 0.0;
}

__global__ __launch_bounds__(64) void cutoff_ticks_kernel(const CutoffP P)
{
    __shared__ PreScratch W;
    __shared__ double4 bc[JSIM_MAX_OBS];
    constexpr bool BLOCK = false;
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, ego = blockIdx.x, B = R.B;
    if (ego >= B) return;
    const int pid = P.pre.path_id[ego];
    const long long off = P.pre.poff[pid];
    const int Mfull = (int)(P.pre.poff[pid + 1] - off);
    const ObsSlice sl = traffic_slice(P.X, ego, P.pre.n_obs);
    const size_t per = (size_t)P.pre.n_steps * 2;
    int idx = P.carry[3 * ego], prev = P.carry[3 * ego + 1], cur = P.carry[3 * ego + 2];
    for (int t = 0; t < P.C; ++t) {
        const int k = P.k0 + t;
        double sx, sy, sv, syaw;
        jct_state_at(R, ego, k, sx, sy, sv, syaw);
        PreP Q = P.pre;
        Q.pred_cc = P.pred_cc + (size_t)t * P.pre.n_obs * per;   // this tick's predictions, all vehicles
        Q.pred_bc = P.pred_bc + (size_t)t * P.pre.n_obs;
        PreOut o;
        if (P.interacting) {                                     // as group_pre_tick_kernel
            GroupP G = P.G;
            G.ego_cc += (size_t)t * B * per;
            G.ego_bc += (size_t)t * B;
            Q.n_obs = group_gather_obstacles(Q, G, P.X, ego, lane, W, bc);
            o = jsim_pre_tick_ego<false, true>(Q, nullptr, bc, nullptr, W, lane, ego, off, Mfull, sx, sy, sv, idx, prev);
        } else {                                                 // as loop_pre_tick_kernel and the fused loops
            Q.n_obs = sl.n;
            o = jsim_pre_tick_ego(Q, Q.pred_cc + (size_t)sl.first * per, Q.pred_bc + sl.first,
                                  P.pre.othr ? P.pre.othr + sl.first : nullptr, W, lane, ego, off, Mfull, sx, sy, sv, idx, prev);
        }
        // the loops' rules (run_host_ticks; the PRE branch of mpc_step_reg.inc): a tick the glue refuses leaves the index and the
        // cut-off as they were; this tick's path is the next one's previous path; a record that ends the episode starts the next
        // tick like a new run (glue_reset_kernel)
        if (o.status == JSIM_OK) { idx = o.idx; cur = o.path_len; }
        const bool col = o.status == JSIM_OK && o.col;
        if (lane == 0) {
            const size_t q = (size_t)k * B + ego;
            P.status[q] = o.status; P.idx[q] = idx; P.cut[q] = cur; P.hit[q] = col ? 1 : 0; P.first[q] = col ? o.first : -1;
            P.col_xy[2 * q] = col ? o.cx : __builtin_nan(""); P.col_xy[2 * q + 1] = col ? o.cy : __builtin_nan("");
        }
        prev = P.speed_cutoff ? Mfull : cur;
        if (jrw_is_end(R.flags[(size_t)k * B + ego])) { idx = 0; prev = -1; }
        JSIM_PRE_SYNC(); // the scratch is reused by the next tick
    }
    if (lane == 0) { P.carry[3 * ego] = idx; P.carry[3 * ego + 1] = prev; P.carry[3 * ego + 2] = cur; }
}
