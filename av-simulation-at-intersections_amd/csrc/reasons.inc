// Stakeholder-reasons scoring of candidate trajectories (DESIGN.md section 14): what perform_replan does with the candidates of
// run_all -- main/scenarios/overtaking_cyclist_bidirectional_road.py:362-373 evaluate_trajectories_for_reasons (:1233-1428),
// evaluate_trajectories_with_weights (:1641-1864) once per weight triple of generate_stakeholder_weight_table (:1431-1604) -- as one
// launch: one workgroup per situation, one wavefront per candidate, then every thread of the workgroup over the weight rows.
//
// Per candidate (one wavefront): resample_curve (lib/trajectories.py:58-86) with the step of compute_predicted_trajectory
// (:244-266), calculate_trajectory_completion_time (:1867-1905), the cyclist's explicit Euler prediction
// (lib/moving_obstacles_prediction.py:21-47), the per-sample scores of lib/reasons_evaluation.py and their trimmed means.
// Everything the reference accumulates in sequence (np.cumsum, the completion time, the Euler states, the two in-range timers)
// is accumulated in the same order here: 64 values at a time, the running value uniform across the wavefront, each lane keeping
// the prefix that ends at its own element.  The per-sample scores are lane-parallel, the means a wavefront reduction.

#define JSIM_REASON_MAX_STEPS 65536   // Euler steps of the cyclist's prediction (completion time / DT); more is status 4
#define JRS_CHUNKS (JSIM_MAX_RES / 64)
#define JRS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

struct ReasonP {
    int n_sit, n_w, ctot;
    const int *cand_off;      // [S + 1]
    const int *pt_off;        // [Ctot + 1]
    const double *pts;        // [.][3]
    const int *mode;          // [Ctot]
    const int *time_from;     // [Ctot] index within the situation
    const double *ego;        // [S][4]
    const double *cyc;        // [S][6]
    const double *now;        // [S][5]
    const double *par;        // [S][JSIM_REASON_NPAR]
    const double *w;          // [W][3] (policymaker, driver, cyclist)
    const int *form;          // [W]
    double ideal[3];          // (cyclist, driver, policymaker)
    int *status, *n_samples;  // [Ctot]
    double *ct;               // [Ctot]
    double *avg;              // [Ctot][4]
    double *scores;           // [W][Ctot]
    int *best;                // [W][S]
    double *detail;           // [Ctot][5][JSIM_MAX_RES] or NULL
    double *resampled;        // [Ctot][JSIM_MAX_RES][3] or NULL
};

// run + v_0 + .. + v_lane in that order (what a sequential loop leaves at element `lane`); run becomes the sum over all 64 lanes
__device__ __forceinline__ double jrs_seq_prefix(double &run, double v, int lane)
{
    double mine = run, r = run;
#pragma unroll 8
    for (int t = 0; t < 64; ++t) {
        r = r + rdlane(v, t);
        if (lane == t) mine = r;
    }
    run = r;
    return mine;
}

__global__ __launch_bounds__(64 * JSIM_MAX_CAND) void score_trajectories_kernel(const ReasonP P)
{
    __shared__ double2 s_xy[JSIM_MAX_CAND][JSIM_MAX_RES];   // the resampled points (x, y) of each wavefront's candidate
    __shared__ double s_ct[JSIM_MAX_CAND];
    __shared__ double s_avg[JSIM_MAX_CAND][4];
    __shared__ int s_st[JSIM_MAX_CAND];

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, s = blockIdx.x;
    const int c0 = P.cand_off[s], C = P.cand_off[s + 1] - c0;
    const bool have = wv < C;
    const int gc = c0 + (have ? wv : 0);
    const double *par = P.par + (size_t)JSIM_REASON_NPAR * s;
    const double dt = par[JSIM_REASON_DT], acc_max = par[JSIM_REASON_MAX_ACCEL], vmax = par[JSIM_REASON_MAX_SPEED];
    const double v = P.ego[4 * (size_t)s + 3];
    double2 *const xy = s_xy[wv];
    int status = JSIM_OK, m = 0;
    double ct = NAN;

    // ---- steps 1-3: resample and time the candidate
    if (have) {
        const int p0 = P.pt_off[gc], n = P.pt_off[gc + 1] - p0;
        const double *pp = P.pts + 3 * (size_t)p0;
        const int md = P.mode[gc];
        const bool accel = md == 0 && v < vmax;
        const double dl_one = md == 1 ? dt * v : dt * vmax;
        if (n < 2 || (md == 1 && !(v > 0.0))) status = 2;
        else {
            double cum = 0.0, acc = 0.0;   // running np.cumsum of the steps and of MAX_ACCEL (uniform)
            long long kprev = 0;
            bool bad = false;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                const bool valid = i < n;
                const int cnt = (n - base) < 64 ? (n - base) : 64;
                double px = 0.0, py = 0.0, pyaw = 0.0, step = 0.0;
                if (valid) {
                    px = pp[3 * (size_t)i]; py = pp[3 * (size_t)i + 1]; pyaw = pp[3 * (size_t)i + 2];
                    if (i >= 1) {
                        const double dx = px - pp[3 * (size_t)(i - 1)], dy = py - pp[3 * (size_t)(i - 1) + 1];
                        step = sqrt(dx * dx + dy * dy);
                    }
                }
                double mycum = cum, myacc = acc, rc = cum, ra = acc;
#pragma unroll 8
                for (int t = 0; t < 64; ++t) {
                    rc = rc + rdlane(step, t);
                    ra = ra + acc_max;
                    if (lane == t) { mycum = rc; myacc = ra; }
                }
                cum = rdlane(mycum, cnt - 1);
                acc = rdlane(myacc, cnt - 1);
                long long ki = 0;
                if (valid) {
                    double dli = dl_one;
                    if (accel) {
                        const double sp = myacc + v;
                        dli = dt * (sp < vmax ? sp : vmax);
                    }
                    if (!(dli > 0.0)) bad = true;
                    ki = (long long)floor(mycum / dli);
                }
                long long kp = __shfl_up(ki, 1);
                if (lane == 0) kp = kprev;
                const bool keep = valid && (i == 0 || i == n - 1 || ki - kp >= 1);
                kprev = __shfl(ki, cnt - 1);
                const unsigned long long bal = __ballot(keep);
                const int slot = m + __popcll(bal & ((1ull << lane) - 1ull));
                if (keep && slot < JSIM_MAX_RES) {
                    xy[slot] = double2{px, py};
                    if (P.resampled) {
                        double *r = P.resampled + ((size_t)gc * JSIM_MAX_RES + slot) * 3;
                        r[0] = px; r[1] = py; r[2] = pyaw;
                    }
                }
                m += __popcll(bal);
            }
            if (__ballot(bad)) status = 2;          // a resampling step that is not positive
            else if (m > JSIM_MAX_RES) status = 4;  // resampled candidate longer than the kernel's table
            else if (m < 3) status = 2;
        }
        JRS_SYNC();
        if (status == JSIM_OK) {
            double vel = v, sum = 0.0;
            for (int base = 1; base < m; base += 64) {
                const int k = base + lane;
                double d = 0.0;
                if (k < m) {
                    const double2 a = xy[k], b = xy[k - 1];
                    const double dx = a.x - b.x, dy = a.y - b.y;
                    d = sqrt(dx * dx + dy * dy);
                }
                double myvel = vel, rv = vel;
#pragma unroll 8
                for (int t = 0; t < 64; ++t) {
                    rv = rv + acc_max;
                    rv = rv < vmax ? rv : vmax;
                    if (lane == t) myvel = rv;
                }
                vel = rv;
                const double q = k < m ? d / myvel : 0.0;
                (void)jrs_seq_prefix(sum, q, lane);
            }
            ct = sum;
        }
        if (lane == 0) { s_ct[wv] = ct; s_st[wv] = status; }
    }
    __syncthreads();

    // ---- steps 4-7 with the completion time of the candidate time_from names
    double a_trim = NAN, a_full = NAN, a_drv = NAN, a_cyc = NAN, ct_used = NAN;
    if (have && status == JSIM_OK) {
        const int donor = P.time_from[gc];
        ct_used = s_ct[donor];
        int nb = 0;
        if (s_st[donor] != JSIM_OK || !isfinite(ct_used)) status = 2;
        else {
            const double nbd = ceil(ct_used / dt);   // len(np.arange(0, ct, DT))
            if (!(nbd >= 2.0)) status = 2;
            else if (nbd > (double)JSIM_REASON_MAX_STEPS) status = 4;
            else nb = (int)nbd;
        }
        if (status == JSIM_OK) {
            const double *cy = P.cyc + 6 * (size_t)s;
            const double *now = P.now + 5 * (size_t)s;
            const double wheelbase = par[JSIM_REASON_WHEELBASE];
            const double idx_step = (double)(nb - 2) / (double)(m - 1);
            int ridx[JRS_CHUNKS];
            double dist[JRS_CHUNKS];
#pragma unroll
            for (int q = 0; q < JRS_CHUNKS; ++q) {
                const int j = 64 * q + lane;
                ridx[q] = j < m ? (j == m - 1 ? nb - 2 : (int)floor((double)j * idx_step)) : -1;
                dist[q] = 0.0;
            }
            // the cyclist: row i = the state after i + 1 Euler steps; rows 0 .. nb - 2 are sampled
            double cx = cy[0], cyy = cy[1], cv = cy[2], cyaw = cy[3];
            const double adt = cy[4] * dt, tans = tan(cy[5]);
            for (int base = 0; base < nb - 1; base += 64) {
                double rv = cv, ryaw = cyaw, pv = cv, pyaw = cyaw;
#pragma unroll 8
                for (int t = 0; t < 64; ++t) {
                    if (lane == t) { pv = rv; pyaw = ryaw; }
                    rv = rv + adt;
                    ryaw = ryaw + ((rv / wheelbase) * tans) * dt;
                }
                cv = rv; cyaw = ryaw;
                const double tx = (pv * cos(pyaw)) * dt, ty = (pv * sin(pyaw)) * dt;
                const double myx = jrs_seq_prefix(cx, tx, lane), myy = jrs_seq_prefix(cyy, ty, lane);
#pragma unroll
                for (int q = 0; q < JRS_CHUNKS; ++q) {
                    const int r = ridx[q] - base;
                    const double gx = __shfl(myx, r & 63), gy = __shfl(myy, r & 63);
                    if (r >= 0 && r < 64 && ridx[q] >= 0) {
                        const double2 e = xy[64 * q + lane];
                        const double dx = gx - e.x, dy = gy - e.y;
                        dist[q] = sqrt(dx * dx + dy * dy);
                    }
                }
            }
            const double half_w = par[JSIM_REASON_WIDTH] / 2, centre = par[JSIM_REASON_CENTERLINE];
            const double rng_d = par[JSIM_REASON_REF_D] + par[JSIM_REASON_BUF_D], thr_d = par[JSIM_REASON_THR_D];
            const double rng_c = par[JSIM_REASON_REF_C] + par[JSIM_REASON_BUF_C], thr_c = par[JSIM_REASON_THR_C];
            double t_d = now[3], t_c = now[4];   // the two timers, carried through the samples in order (uniform)
            double sp_trim = 0.0, sp_full = 0.0, sd = 0.0, sc = 0.0;
            double *det = P.detail ? P.detail + (size_t)gc * 5 * JSIM_MAX_RES : nullptr;
#pragma unroll
            for (int q = 0; q < JRS_CHUNKS; ++q) {
                const int j = 64 * q + lane;
                const bool valid = j < m;
                if (64 * q >= m) break;
                const double ex = valid ? xy[j].x : 0.0;
                const double dc = (ex - half_w) - centre;
                double pol = dc >= 0.0 ? 1.0 : exp(0.2 * dc);
                const bool in_d = valid && dist[q] < rng_d, in_c = valid && dist[q] < rng_c;
                const double comfort = in_c ? exp(0.2 * (dist[q] - rng_c)) : 1.0;
                const unsigned long long incl = (2ull << lane) - 1ull;
                const unsigned long long bd = __ballot(in_d), bc = __ballot(in_c);
                const int cl_d = __popcll(bd & incl), cl_c = __popcll(bc & incl), tot_d = __popcll(bd), tot_c = __popcll(bc);
                double mine_d = t_d, mine_c = t_c;
                for (int t = 1; t <= tot_d; ++t) { t_d = t_d + dt; if (cl_d == t) mine_d = t_d; }
                for (int t = 1; t <= tot_c; ++t) { t_c = t_c + dt; if (cl_c == t) mine_c = t_c; }
                double drv = (in_d && mine_d >= thr_d) ? 1.0 / exp(0.2 * (mine_d - thr_d)) : 1.0;
                const double cyt = (in_c && mine_c >= thr_c) ? 1.0 / exp(0.2 * (mine_c - thr_c)) : 1.0;
                double comb = comfort * cyt;
                if (j == 0) { pol = now[0]; drv = now[1]; comb = now[2]; }   // entry 0 = the situation's current values
                if (j < m - 1) { sp_full += pol; sd += drv; sc += comb; }     // the last sample is dropped
                if (j < m - 2) sp_trim += pol;
                if (det && valid) {
                    if (j < m - 1) { det[j] = pol; det[JSIM_MAX_RES + j] = drv; det[4 * JSIM_MAX_RES + j] = comb; }
                    det[2 * JSIM_MAX_RES + j] = comfort;
                    det[3 * JSIM_MAX_RES + j] = cyt;
                }
            }
            a_trim = wsum(sp_trim) / (double)(m - 2);
            a_full = wsum(sp_full) / (double)(m - 1);
            a_drv = wsum(sd) / (double)(m - 1);
            a_cyc = wsum(sc) / (double)(m - 1);
        }
    }
    if (have && lane == 0) {
        s_st[wv] = status;
        s_avg[wv][0] = a_trim; s_avg[wv][1] = a_full; s_avg[wv][2] = a_drv; s_avg[wv][3] = a_cyc;
        P.status[gc] = status;
        P.n_samples[gc] = m;
        if (status == JSIM_OK) {
            P.ct[gc] = ct_used;
            P.avg[4 * (size_t)gc] = a_trim; P.avg[4 * (size_t)gc + 1] = a_full; P.avg[4 * (size_t)gc + 2] = a_drv; P.avg[4 * (size_t)gc + 3] = a_cyc;
        }
    }
    __syncthreads();

    // ---- the weight rows: balance_function (:1191-1231), the weighted sum, form 1's clamp, first arg-max
    const double i0 = P.ideal[0], i1 = P.ideal[1], i2 = P.ideal[2];
    const double max_dev = sqrt((i0 * i0 + i1 * i1) + i2 * i2);
    for (int k = threadIdx.x; k < P.n_w; k += blockDim.x) {
        const double wp = P.w[3 * (size_t)k], wd = P.w[3 * (size_t)k + 1], wc = P.w[3 * (size_t)k + 2];
        const int f = P.form[k];
        double ratio = wc / i0;
        ratio = (wd / i1 < ratio) ? wd / i1 : ratio;
        ratio = (wp / i2 < ratio) ? wp / i2 : ratio;
        const double ssd = ((wc - i0) * (wc - i0) + (wd - i1) * (wd - i1)) + (wp - i2) * (wp - i2);
        const double bal = (1.0 - sqrt(ssd / 3.0) / max_dev) * ratio;
        int best = -1;
        double top = -INFINITY;
        for (int c = 0; c < C; ++c) {
            if (s_st[c] != JSIM_OK) continue;   // its score stays NaN and it never wins
            double sc = bal * ((wp * s_avg[c][f ? 1 : 0] + wd * s_avg[c][2]) + wc * s_avg[c][3]);
            if (f) { sc = sc < 1.0 ? sc : 1.0; sc = sc > 0.0 ? sc : 0.0; }
            P.scores[(size_t)k * P.ctot + c0 + c] = sc;
            if (sc > top) { top = sc; best = c; }
        }
        P.best[(size_t)k * P.n_sit + s] = best;
    }
}
