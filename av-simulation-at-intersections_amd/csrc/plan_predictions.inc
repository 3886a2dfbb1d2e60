// Every recorded plan-rule prediction against what the ego then did (DESIGN.md section 29; the rule is stated in include/jsim_mpc.h).
// Row b is ego b as its group mates predicted it under JSIM_MATE_PLAN: for tick k the controls its controller held at the start of
// the tick -- plan_oa[k][b], plan_od[k][b], plan_status[k][b] of the plan recorder (jsim_loop_set_plan_recorder) -- rolled through
// the plant's step from the tick-start state (jct_state_at), ego_plan_predict_kernel's recurrence operation for operation, and
// sample j held against the ego's record of tick k + j.  The walk, the truth slots, the outputs and the sums by look-ahead step are
// prediction_score_kernel's for an ego row (predictions.inc).  One wavefront per ego, ticks 64 at a time, lane t owns tick k0 + t.
// Consecutive lanes own consecutive ticks, whose plan rows lie B * T doubles apart in memory: the chunk's 64 rows of either array
// are loaded once, element after element across the lanes (each row's T doubles are contiguous), into an LDS tile whose rows are
// JPP_STRIDE doubles apart.  The stride is odd, so the 32 lanes of a ds_read_b64 group reading step j of their own rows fall on 32
// distinct bank pairs.  Every lane runs its own serial recurrence in registers: no prediction is written to memory.
//
// The two kernels of this file are compiled in a translation unit of their own (jsim_plan.hip, -DJSIM_PLAN_TU), so that they sit in a
// code object of their own and every code object the library had before them stays as it was, byte for byte; the rest of the
// library sees their parameter structs and declarations only.

enum { JPP_STRIDE = JSIM_MAX_T + 1, JPP_SLOTS = 64 + 64 }; // JPP_SLOTS: predictions.inc's JPS_SLOTS = 64 + JSIM_MAX_PRED (asserted there)
static_assert(JPP_STRIDE % 2 == 1, "an even row stride puts two lanes of a ds_read_b64 group on one bank pair");

// The plan recorder (jsim_loop_set_plan_recorder, DESIGN.md section 29): every ego's oa, od [B][T] and status [B] as they stand at
// the start of the tick -- what launch_ego_plan_predict reads -- to the slot of the device tick counter, where the tick's History
// record goes; ticks beyond cap are dropped.  One thread per element of oa.
struct PlanRecP {
    int B, T, cap;
    const int *tick;
    const double *oa, *od;
    const int *status;
    double *plan_oa, *plan_od; // [cap][B][T]
    int *plan_status;          // [cap][B]
};

struct PlanScoreP {
    RecorderBuf R;
    int n_steps, T;
    double dt, L, smax, vmax, vmin, tol; // wheelbase and clamps: the plant's, as EgoPlanP's
    const double *plan_oa;    // [n][B][T]
    const double *plan_od;    // [n][B][T]
    const int *plan_status;   // [n][B]
    int *pt_i;                // [n][B][JSIM_PS_NI]
    double *pt_d;             // [n][B][JSIM_PS_ND]
    double *step_sum;         // [B][n_steps]
    int *step_cnt;            // [B][n_steps]
    double *err;              // [n][B][n_steps] or NULL
};

#ifndef JSIM_PLAN_TU
__global__ void plan_record_kernel(PlanRecP P);
__global__ void plan_prediction_score_kernel(const PlanScoreP P);
#else
__global__ __launch_bounds__(256) void plan_record_kernel(PlanRecP P)
{
    const int k = *P.tick;
    if (k < 0 || k >= P.cap) return;
    const size_t n = (size_t)P.B * P.T, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { P.plan_oa[(size_t)k * n + i] = P.oa[i]; P.plan_od[(size_t)k * n + i] = P.od[i]; }
    if (i < (size_t)P.B) P.plan_status[(size_t)k * P.B + i] = P.status[i];
}

__global__ __launch_bounds__(64) void plan_prediction_score_kernel(const PlanScoreP P)
{
    __shared__ double tx[JPP_SLOTS], ty[JPP_SLOTS], tpsi[JPP_SLOTS];
    __shared__ double ta[64 * JPP_STRIDE], td[64 * JPP_STRIDE];
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks, S = P.n_steps, T = P.T;
    if (b >= B) return;
    const double dt = P.dt, L = P.L;
    const int span = 63 + S;                                    // the truth slots a chunk's lanes can reach

    unsigned long long e_cur = 0ull, e_next = jrw_end_mask(R, lane, jrw_flag(R, b, lane), true);
    double acc = 0.0;                                           // lane j: the sum of e_j over the ticks so far
    int cnt = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < n;
        e_cur = e_next;                                         // the next chunk's ends ahead of the body: the horizon reaches into it
        e_next = jrw_end_mask(R, k + 64, jrw_flag(R, b, k + 64), true);
        // the truth poses this chunk can reach, once: slot s is the ego's record of tick k0 + s
        for (int s = lane; s < span; s += 64) {
            const int kt = k0 + s;
            double x = 0.0, y = 0.0, psi = 0.0;
            if (kt < n) {
                const double *p = R.rec + JSIM_REC_FIELDS * ((size_t)kt * B + b);
                x = p[0]; y = p[1]; psi = p[2];
            }
            tx[s] = x; ty[s] = y; tpsi[s] = psi;
        }
        // the chunk's plans, once: element e of the [64][T] block is row e / T (tick k0 + row), column e % T; zeros beyond the records
        for (int e = lane; e < 64 * T; e += 64) {
            const int row = e / T, col = e - row * T, kt = k0 + row;
            double a = 0.0, d = 0.0;
            if (kt < n) {
                const size_t at = ((size_t)kt * B + b) * T + col;
                a = P.plan_oa[at]; d = P.plan_od[at];
            }
            ta[row * JPP_STRIDE + col] = a; td[row * JPP_STRIDE + col] = d;
        }
        __syncthreads();

        // this lane's tick: the prediction's input and how many samples have a truth
        double x = 0.0, y = 0.0, v = 0.0, yaw = 0.0, dl = 0.0;
        bool ok = false;
        int m = 0;
        if (valid) {
            jct_state_at(R, b, k, x, y, v, yaw);
            const bool fresh = k == 0 || jrw_is_end(R.flags[(size_t)(k - 1) * B + b]);
            const double d = R.rec[JSIM_REC_FIELDS * ((size_t)(k > 0 ? k - 1 : 0) * B + b) + 4];
            dl = fresh ? 0.0 : d;
            ok = P.plan_status[(size_t)k * B + b] == JSIM_OK;
            const unsigned long long eb = e_cur >> lane;
            const int ke = eb ? k + (int)__builtin_ctzll(eb) : (e_next ? k0 + 64 + (int)__builtin_ctzll(e_next) : k0 + 128);
            m = ke - k + 1;
            m = m < S ? m : S;
        }
        const double *const pa = ta + lane * JPP_STRIDE, *const pd = td + lane * JPP_STRIDE;
        // the held tail's steering, for a horizon of one element as well; steps j <= T - 1 replace it with their own
        double tn;
        {
            const double di = ok ? pd[T - 1] : dl;
            double dc = (P.smax < di) ? P.smax : di;
            dc = (-P.smax > dc) ? -P.smax : dc;
            tn = tan(dc);
        }
        double sum = 0.0, mx = 0.0, fdx = 0.0, fdy = 0.0, fe = 0.0, fyaw = 0.0, fpsi = 0.0;
        int hold = 0, max_at = -1;
        bool holding = true;
        for (int i = 0; i < S; ++i) {
            const int j = i + 1;
            double ai = 0.0;
            if (j < T) {                                        // (uniform) the plan's own element; behind it a = 0 and tan stays
                const double a_plan = pa[j], d_plan = pd[j];
                ai = ok ? a_plan : 0.0;
                const double di = ok ? d_plan : dl;
                double dc = (P.smax < di) ? P.smax : di;
                dc = (-P.smax > dc) ? -P.smax : dc;
                tn = tan(dc);
            }
            const double vb = v;
            x += vb * cos(yaw) * dt;
            y += vb * sin(yaw) * dt;
            yaw += (vb / L) * tn * dt;
            v += ai * dt;
            v = (P.vmax < v) ? P.vmax : v;
            v = (P.vmin > v) ? P.vmin : v;
            const bool scored = i < m;
            const double dx = x - tx[lane + i], dy = y - ty[lane + i], psi = tpsi[lane + i];
            const double e = sqrt(dx * dx + dy * dy);
            if (scored) {
                sum += e;
                holding = holding && e <= P.tol;
                hold += holding ? 1 : 0;
                if (i == 0 || e > mx) { mx = e; max_at = i; }
                fdx = dx; fdy = dy; fe = e; fyaw = yaw; fpsi = psi;     // (the last scored sample's stay)
            }
            if (P.err && valid) P.err[((size_t)k * B + b) * S + i] = scored ? e : __builtin_nan("");
            // the step's sum over the chunk's ticks: a butterfly, the same bits in every lane
            double part = scored ? e : 0.0;
            for (int w = 32; w > 0; w >>= 1) part += __shfl_xor(part, w);
            const int c = __popcll(__ballot(scored));
            if (lane == i) { acc += part; cnt += c; }
        }
        __syncthreads();                                        // the next chunk's poses and plans replace these

        if (valid) {
            const size_t q = (size_t)k * B + b;
            int *const pi = P.pt_i + JSIM_PS_NI * q;
            double *const pdo = P.pt_d + JSIM_PS_ND * q;
            const double nan = __builtin_nan("");
            const double cs = cos(fpsi), sn = sin(fpsi);
            const double lon = fdx * cs + fdy * sn, lat = -fdx * sn + fdy * cs;
            const double eyaw = jpl_pymod((fyaw - fpsi) + 3.141592653589793, 6.283185307179586) - 3.141592653589793;
            const bool any = m > 0;
            pi[JSIM_PS_N] = any ? m : 0; pi[JSIM_PS_HOLD] = any ? hold : 0; pi[JSIM_PS_MAX_AT] = max_at;
            pdo[JSIM_PS_ADE] = any ? sum / (double)m : nan; pdo[JSIM_PS_FDE] = any ? fe : nan; pdo[JSIM_PS_MAX] = any ? mx : nan;
            pdo[JSIM_PS_LON] = any ? lon : nan; pdo[JSIM_PS_LAT] = any ? lat : nan; pdo[JSIM_PS_YAW] = any ? eyaw : nan;
        }
    }
    if (lane < S) { P.step_sum[(size_t)b * S + lane] = acc; P.step_cnt[(size_t)b * S + lane] = cnt; }
}
#endif
