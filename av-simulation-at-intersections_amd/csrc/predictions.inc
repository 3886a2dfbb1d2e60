// Every recorded prediction against what the vehicle then did (DESIGN.md section 28; the rule is stated in include/jsim_mpc.h).  Row
// r < n_obs is recorded vehicle r, row n_obs + b is ego b under the constant rule.  For tick k the row's prediction is
// obstacle_predict_one's recurrence, operation for operation, from the tuple the loop predicted from -- the vehicle's get() tuple of
// the tick, the ego's tick-start state (jct_state_at) with a = 0 and the steering of its record before -- and sample j is held
// against the recorded pose (j + 1) * dt later.  One wavefront per row, ticks 64 at a time, lane t owns tick k0 + t
// (recorder_walk.inc).  The truth poses a chunk can reach -- 63 + n_steps of them -- are staged once in LDS; lane t reads sample j at
// slot t + j, consecutive lanes consecutive 8-byte slots.  Every lane runs its own serial recurrence in registers: no prediction
// is written to memory.  The sums by look-ahead step are a wavefront butterfly per step, kept by lane j from chunk to chunk: a fixed
// order, no atomics, the same bits on every call.

struct PredScoreP {
    RecorderBuf R;            // the egos' records (rows n_obs ..)
    int n_obs, egos, n_steps;
    double dt, L_obs, L_ego, tol;
    const double *obs_rec;    // [n][n_obs][6]
    const double4 *shape;     // [n_obs] (cc0, cc1, radius, L) or NULL: L_obs for every vehicle
    int *pt_i;                // [n][V][JSIM_PS_NI]
    double *pt_d;             // [n][V][JSIM_PS_ND]
    double *step_sum;         // [V][n_steps]
    int *step_cnt;            // [V][n_steps]
    double *err;              // [n][V][n_steps] or NULL
};

enum { JPS_SLOTS = 64 + JSIM_MAX_PRED };

__global__ __launch_bounds__(64) void prediction_score_kernel(const PredScoreP P)
{
    __shared__ double tx[JPS_SLOTS], ty[JPS_SLOTS], tpsi[JPS_SLOTS];
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, r = blockIdx.x, B = R.B, n = R.n_ticks, S = P.n_steps;
    const int V = P.n_obs + (P.egos ? B : 0);
    if (r >= V) return;
    const bool ego = r >= P.n_obs;
    const int b = r - P.n_obs;
    const double dt = P.dt;
    const double L = ego ? P.L_ego : (P.shape ? P.shape[r].w : P.L_obs);
    const int span = 63 + S;                                    // the truth slots a chunk's lanes can reach

    unsigned long long e_cur = 0ull, e_next = ego ? jrw_end_mask(R, lane, jrw_flag(R, b, lane), true) : 0ull;
    double acc = 0.0;                                           // lane j: the sum of e_j over the ticks so far
    int cnt = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < n;
        if (ego) {                                              // the next chunk's ends ahead of the body: the horizon reaches into it
            e_cur = e_next;
            e_next = jrw_end_mask(R, k + 64, jrw_flag(R, b, k + 64), true);
        }
        // the truth poses this chunk can reach, once: slot s is the vehicle's tuple of tick k0 + s + 1, the ego's record of tick k0 + s
        for (int s = lane; s < span; s += 64) {
            const int kt = k0 + s + (ego ? 0 : 1);
            double x = 0.0, y = 0.0, psi = 0.0;
            if (kt < n) {
                const double *p = ego ? R.rec + JSIM_REC_FIELDS * ((size_t)kt * B + b) : P.obs_rec + 6 * ((size_t)kt * P.n_obs + r);
                const double q2 = p[2], q3 = p[3];
                x = p[0]; y = p[1]; psi = ego ? q2 : q3;
            }
            tx[s] = x; ty[s] = y; tpsi[s] = psi;
        }
        __syncthreads();

        // this lane's tick: the prediction's input and how many samples have a truth
        double x = 0.0, y = 0.0, v = 0.0, yaw = 0.0, a = 0.0, st = 0.0;
        int m = 0;
        if (valid) {
            if (ego) {
                jct_state_at(R, b, k, x, y, v, yaw);
                const bool fresh = k == 0 || jrw_is_end(R.flags[(size_t)(k - 1) * B + b]);
                const double d = R.rec[JSIM_REC_FIELDS * ((size_t)(k > 0 ? k - 1 : 0) * B + b) + 4];
                st = fresh ? 0.0 : d;
                const unsigned long long eb = e_cur >> lane;
                const int ke = eb ? k + (int)__builtin_ctzll(eb) : (e_next ? k0 + 64 + (int)__builtin_ctzll(e_next) : k0 + 128);
                m = ke - k + 1;
            } else {
                const double *p = P.obs_rec + 6 * ((size_t)k * P.n_obs + r);
                x = p[0]; y = p[1]; v = p[2]; yaw = p[3]; a = p[4]; st = p[5];
                m = n - 1 - k;
            }
            m = m < S ? m : S;
        }
        const double tn = tan(st);
        double sum = 0.0, mx = 0.0, fdx = 0.0, fdy = 0.0, fe = 0.0, fyaw = 0.0, fpsi = 0.0;
        int hold = 0, max_at = -1;
        bool holding = true;
        for (int j = 0; j < S; ++j) {
            x += v * cos(yaw) * dt;
            y += v * sin(yaw) * dt;
            v += a * dt;
            yaw += (v / L) * tn * dt;
            const bool scored = j < m;
            const double dx = x - tx[lane + j], dy = y - ty[lane + j], psi = tpsi[lane + j];
            const double e = sqrt(dx * dx + dy * dy);
            if (scored) {
                sum += e;
                holding = holding && e <= P.tol;
                hold += holding ? 1 : 0;
                if (j == 0 || e > mx) { mx = e; max_at = j; }
                fdx = dx; fdy = dy; fe = e; fyaw = yaw; fpsi = psi;     // (the last scored sample's stay)
            }
            if (P.err && valid) P.err[((size_t)k * V + r) * S + j] = scored ? e : __builtin_nan("");
            // the step's sum over the chunk's ticks: a butterfly, the same bits in every lane
            double part = scored ? e : 0.0;
            for (int w = 32; w > 0; w >>= 1) part += __shfl_xor(part, w);
            const int c = __popcll(__ballot(scored));
            if (lane == j) { acc += part; cnt += c; }
        }
        __syncthreads();                                        // the next chunk's poses replace these

        if (valid) {
            const size_t q = (size_t)k * V + r;
            int *const pi = P.pt_i + JSIM_PS_NI * q;
            double *const pd = P.pt_d + JSIM_PS_ND * q;
            const double nan = __builtin_nan("");
            const double cs = cos(fpsi), sn = sin(fpsi);
            const double lon = fdx * cs + fdy * sn, lat = -fdx * sn + fdy * cs;
            const double eyaw = jpl_pymod((fyaw - fpsi) + 3.141592653589793, 6.283185307179586) - 3.141592653589793;
            const bool any = m > 0;
            pi[JSIM_PS_N] = any ? m : 0; pi[JSIM_PS_HOLD] = any ? hold : 0; pi[JSIM_PS_MAX_AT] = max_at;
            pd[JSIM_PS_ADE] = any ? sum / (double)m : nan; pd[JSIM_PS_FDE] = any ? fe : nan; pd[JSIM_PS_MAX] = any ? mx : nan;
            pd[JSIM_PS_LON] = any ? lon : nan; pd[JSIM_PS_LAT] = any ? lat : nan; pd[JSIM_PS_YAW] = any ? eyaw : nan;
        }
    }
    if (lane < S) { P.step_sum[(size_t)r * S + lane] = acc; P.step_cnt[(size_t)r * S + lane] = cnt; }
}
