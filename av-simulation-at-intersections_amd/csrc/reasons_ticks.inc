// Stakeholder reasons per recorded tick and the replan trigger (DESIGN.md section 16): what the loop of
// main/scenarios/overtaking_cyclist_bidirectional_road.py does once per tick -- evaluate_reasons (:127-128, :2007-2027, with
// lib/reasons_evaluation.py inside) and reasons_evaluation (:141-142, :1907-1940) -- as one pass over the History recorder's
// buffers (jsim_loop_set_recorder), walked as recorder_walk.inc says: one wavefront per ego, ticks 64 at a time, lane t owns tick
// k0 + t.
//
// Lane-parallel: the ego's position at the start of the tick, the cyclist's recorded get(), the distance, the two in-range tests,
// the policymaker value and the distance factor.  In sequence, in the reference's order: the two timers (one `+ DT` per in-range
// tick from a running value that is uniform across the wavefront, lane t keeping the value after its own tick -- jrs_seq_prefix's
// pattern of reasons.inc, plus the reset to 0 on the first tick of an episode) and the replan tracker (a one-lane shift of a
// ballot, one carried bit between chunks).

struct ReasonTickP {
    RecorderBuf R;
    int n_obs;
    const double *obs_rec;    // [n][n_obs][6] or NULL (no ego has a cyclist)
    const int *veh_of;        // [B] the ego's cyclist among the n_obs vehicles, -1: none
    const double *par;        // [B][JSIM_REASON_NPAR]
    const double *threshold;  // [B]
    double *carry;            // [B][3] in / out
    double *val;              // [n][B][4]
    double *timers;           // [n][B][2]
    int *trig;                // [n][B]
    int *first;               // [B]
};

// One timer over the cnt ticks of a chunk: `reset` bit t puts it to 0 ahead of tick t, `in` bit t adds dt; lane t gets the value
// after tick t, run the value after the chunk's last tick.  The masks are ballots, so every branch is uniform.
__device__ __forceinline__ double jrt_seq_timer(double &run, unsigned long long in, unsigned long long reset, double dt, int cnt, int lane)
{
    double mine = run, r = run;
    for (int t = 0; t < cnt; ++t) {
        if ((reset >> t) & 1ull) r = 0.0;
        if ((in >> t) & 1ull) r = r + dt;
        if (lane == t) mine = r;
    }
    run = r;
    return mine;
}

__global__ __launch_bounds__(64) void reason_ticks_kernel(const ReasonTickP P)
{
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks;
    const double *par = P.par + (size_t)JSIM_REASON_NPAR * b;
    const double dt = par[JSIM_REASON_DT];
    const double half_w = par[JSIM_REASON_WIDTH] / 2, centre = par[JSIM_REASON_CENTERLINE];
    const double rng_d = par[JSIM_REASON_REF_D] + par[JSIM_REASON_BUF_D], thr_d = par[JSIM_REASON_THR_D];
    const double rng_c = par[JSIM_REASON_REF_C] + par[JSIM_REASON_BUF_C], thr_c = par[JSIM_REASON_THR_C];
    const double limit = P.threshold[b];
    int veh = P.obs_rec ? P.veh_of[b] : -1;
    if (veh >= P.n_obs) veh = -1;   // (the Python surface refuses it; here it only must not be read)
    const bool has = veh >= 0;
    double t_d = P.carry[3 * (size_t)b], t_c = P.carry[3 * (size_t)b + 1];
    unsigned long long tracker = P.carry[3 * (size_t)b + 2] != 0.0 ? 1ull : 0ull;
    int first = -1;

    RecChunk C = {};
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < n;
        // tick 0 starts no episode here: the carry says what it starts from
        jrw_enter(C, R, k0, jrw_end_mask(R, k, jrw_flag(R, b, k), false), false);
        const int cnt = C.cnt;
        const bool start = valid && ((C.s_cur >> lane) & 1ull) != 0ull;
        double ex = 0.0, ey = 0.0, eyaw, dist = NAN;
        if (valid) {
            jrw_pose_at(R, b, k, start, ex, ey, eyaw);
            if (has) {
                const double *c = P.obs_rec + 6 * ((size_t)k * P.n_obs + veh);
                const double dx = c[0] - ex, dy = c[1] - ey;
                dist = sqrt(dx * dx + dy * dy);
            }
        }
        const bool in_d = valid && has && dist < rng_d, in_c = valid && has && dist < rng_c;
        const double dc = (ex - half_w) - centre;
        const double pol = dc >= 0.0 ? 1.0 : exp(0.2 * dc);
        const double comfort = in_c ? exp(0.2 * (dist - rng_c)) : 1.0;

        const unsigned long long bs = __ballot(start);
        const double mine_d = jrt_seq_timer(t_d, __ballot(in_d), bs, dt, cnt, lane);
        const double mine_c = jrt_seq_timer(t_c, __ballot(in_c), bs, dt, cnt, lane);
        double drv = (in_d && mine_d >= thr_d) ? 1.0 / exp(0.2 * (mine_d - thr_d)) : 1.0;
        const double cyt = (in_c && mine_c >= thr_c) ? 1.0 / exp(0.2 * (mine_c - thr_c)) : 1.0;
        double cyc = cyt * comfort;
        if (!has) { drv = NAN; cyc = NAN; }

        // the trigger: needed = below and not tracker; tracker = below, False at an episode's first tick (NaN is never below)
        const bool lo_p = valid && pol < limit, lo_d = valid && drv < limit, lo_c = valid && cyc < limit;
        const unsigned long long bb = __ballot(lo_p || lo_d || lo_c);
        const unsigned long long before = ((bb << 1) | tracker) & ~bs;   // the tracker each tick meets
        const unsigned long long need = bb & ~before;
        tracker = (bb >> (cnt - 1)) & 1ull;
        if (first < 0 && need != 0ull) first = k0 + (int)__builtin_ctzll(need);

        if (valid) {
            const size_t r = (size_t)k * B + b;
            P.val[4 * r] = pol; P.val[4 * r + 1] = drv; P.val[4 * r + 2] = cyc; P.val[4 * r + 3] = dist;
            P.timers[2 * r] = mine_d; P.timers[2 * r + 1] = mine_c;
            P.trig[r] = (int)((need >> lane) & 1ull) | (lo_p ? 2 : 0) | (lo_d ? 4 : 0) | (lo_c ? 8 : 0);
        }
    }
    // the carry is the state the next tick starts from: a last record that ended its episode leaves a fresh one
    if (n > 0 && jrw_is_end(jrw_flag(R, b, n - 1))) { t_d = 0.0; t_c = 0.0; tracker = 0ull; }
    if (lane == 0) {
        P.carry[3 * (size_t)b] = t_d; P.carry[3 * (size_t)b + 1] = t_c; P.carry[3 * (size_t)b + 2] = tracker ? 1.0 : 0.0;
        P.first[b] = first;
    }
}
