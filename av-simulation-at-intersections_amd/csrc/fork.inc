// Forking a recorded run (DESIGN.md section 22): the two cold-path kernels that give a new loop its start -- every row's ego state
// at the start of its own tick, gathered from the History recorder's buffers (jsim_loop_set_recorder) by jct_state_at, the rule the
// cut-off replay reads its states by, with the first tick of the episode that tick belongs to; and the scripted vehicles advanced
// from their start states by each one's own number of ticks, by obstacle_step_one in the loops' own two calls per tick.  What
// perform_replan of main/scenarios/overtaking_cyclist_bidirectional_road.py (:394-402) gets for nothing by letting the same
// simulation and the same cyclist go on under a new controller.  The loops' kernels are not touched.

struct ForkStateP {
    RecorderBuf R;
    int n_rows;
    const int *ego, *at;      // [n_rows] the ego and the tick (0 .. n_ticks) of every row
    double *x0;               // [n_rows][4] x, y, v, yaw at the start of the tick
    int *k0;                  // [n_rows] the first tick of the tick's episode
};

// One wavefront per row.  The episode's first tick: one behind the last end before `at`, found by walking the flags backwards 64 at
// a time, lane t owning tick hi - 1 - t; the mask is a ballot, so the branch on it is uniform.
__global__ __launch_bounds__(64) void fork_state_kernel(const ForkStateP P)
{
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, r = blockIdx.x;
    if (r >= P.n_rows) return;
    const int e = P.ego[r], at = P.at[r];
    int k0 = 0;
    for (int hi = at; hi > 0; hi -= 64) {
        const int k = hi - 1 - lane;
        const unsigned long long ends = __ballot(k >= 0 && jrw_is_end(R.flags[(size_t)k * R.B + e]));
        if (ends != 0ull) { k0 = hi - (int)__builtin_ctzll(ends); break; }
    }
    if (lane != 0) return;
    double x, y, v, yaw;
    jct_state_at(R, e, at, x, y, v, yaw);
    double *o = P.x0 + 4 * (size_t)r;
    o[0] = x; o[1] = y; o[2] = v; o[3] = yaw;
    P.k0[r] = k0;
}

struct ObsAtP {
    int n_obs;
    double L;                 // the wheelbase of every vehicle without one of its own
    const double *state0;     // [n_obs][4] xc, yc, theta, counter at tick 0
    const double *param;      // [n_obs][8] as ObsStepP's
    const double *wheelbase;  // [n_obs] or NULL
    const int *ticks;         // [n_obs] how many ticks each vehicle is advanced
    double *state;            // [n_obs][4] out
    const double4 *route_pt;  // the route table as ObsStepP's (NULL: none)
    const int *route_off;
    int n_routes;
};

// One thread per vehicle: obstacle_rollout_kernel's body, each vehicle for its own number of ticks and with nothing written but
// its state -- get() alone (the roundabout rule may rewrite the heading there), then get() + step()
__global__ __launch_bounds__(64) void obstacles_at_kernel(const ObsAtP P)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n_obs) return;
    for (int j = 0; j < 4; ++j) P.state[4 * (size_t)o + j] = P.state0[4 * (size_t)o + j];
    ObsStepP Q = {P.n_obs, 0, P.wheelbase ? P.wheelbase[o] : P.L, P.state, P.param, nullptr, nullptr, nullptr, 0, nullptr};
    Q.route_pt = P.route_pt; Q.route_off = P.route_off; Q.n_routes = P.n_routes;
    const int n = P.ticks[o];
    for (int k = 0; k < n; ++k) {
        Q.do_step = 0;
        obstacle_step_one(Q, o);
        Q.do_step = 1;
        obstacle_step_one(Q, o);
    }
}
