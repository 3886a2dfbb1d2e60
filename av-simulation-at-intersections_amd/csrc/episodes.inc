// One row per recorded episode (DESIGN.md section 19): the segmented reduction of the History recorder's buffers and of the per-tick
// series of sections 16-18 over the episodes of history.episode_bounds.  Three launches: episode_count_kernel (an ego's end flags by
// ballot and popcount), episode_scan_kernel (the exclusive prefix over the B counts, one workgroup tiling B with a carry) and
// episode_summary_kernel: one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t (the walk of recorder_walk.inc).
//
// Lane-parallel: the record, the start-of-tick pose (jrw_pose), the step length and the tick's entries of the optional series.
// Per episode segment of a chunk (its lanes [pos, e], from the chunk's end-flag ballot): every sum, minimum and maximum by a
// butterfly over the 64 lanes with the lanes outside the segment holding the operation's neutral value (0.0 / NaN), the tick of an
// extreme value from the ballot of the lanes that hold it.  An episode open at the chunk's end is carried as wave-uniform values
// (EpisodeAcc).  Chunks are aligned to tick 0 and a segment's butterfly sees the same 64 operands whatever follows the segment, so
// a finished episode's row does not depend on how many ticks follow it.  A row is written once, by lane 0, with plain stores.

struct EpisodeP {
    RecorderBuf R;
    int ep_cap;
    const double *veh_clear;  // [n][B] or NULL with its group (jsim_loop_eval_conflicts' outputs)
    const int *veh_who, *veh_hit_tick, *veh_hit_frame;
    const double *veh_hit_xy; // [n][B][2]
    const double *st_clear;   // [n][B] or NULL with its group (jsim_loop_eval_static's outputs)
    const int *st_who, *st_hit, *st_off_tick;
    const double *rs_val;     // [n][B][4] or NULL with its group (jsim_loop_eval_reasons' outputs)
    const int *rs_trig;       // [n][B]
    long long *ep_off;        // [B + 1]: the counts, then their exclusive prefix
    int *ep_i;                // [ep_cap][JSIM_EP_NI]
    double *ep_d;             // [ep_cap][JSIM_EP_ND]
};

// ---- launch 1: episodes per ego = its end flags + 1 (the running one), left in ep_off[b] ----
__global__ __launch_bounds__(64) void episode_count_kernel(const EpisodeP P)
{
    const int lane = threadIdx.x, b = blockIdx.x, n = P.R.n_ticks;
    int ends = 0;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        ends += __popcll(jrw_end_mask(P.R, k, jrw_flag(P.R, b, k), false));
    }
    if (lane == 0) P.ep_off[b] = (long long)ends + 1;
}

// ---- launch 2: ep_off[b] = the sum of the counts before b, ep_off[B] = the total; one workgroup, B in tiles of 1024 ----
__global__ __launch_bounds__(1024) void episode_scan_kernel(const EpisodeP P)
{
    __shared__ long long wave_sum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (int base = 0; base < P.R.B; base += 1024) {
        const int i = base + t;
        const long long c = i < P.R.B ? P.ep_off[i] : 0;
        long long incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long long before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const long long s = wave_sum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < P.R.B) P.ep_off[i] = carry + before + (incl - c);
        carry += total;
        __syncthreads();       // wave_sum is written again in the next tile
    }
    if (t == 0) P.ep_off[P.R.B] = carry;
}

// ---- launch 3 ----
__device__ __forceinline__ double jep_sum(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double jep_min(double v)    // fmin / fmax return the other operand for a NaN: NaN only when all are
{
    for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ double jep_max(double v)
{
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

// A running extreme value and the first tick that holds it.  `v` is NaN in the lanes outside the segment; `lo`: a minimum.
struct EpisodeExt { double v; int tick; };
__device__ __forceinline__ bool jep_extreme(EpisodeExt &E, double v, bool lo, int k0c, int &lane_of)
{
    const double m = lo ? jep_min(v) : jep_max(v);
    const bool better = m == m && (E.v != E.v || (lo ? m < E.v : m > E.v));    // strictly: the first occurrence stays
    if (better) {
        lane_of = (int)__builtin_ctzll(__ballot(v == m));
        E.v = m; E.tick = k0c + lane_of;
    }
    return better;
}

// What is carried of the open episode: wave-uniform
struct EpisodeAcc {
    int k0, n, failed, n_dev, st_ticks_off, replan_tick, veh_who, st_who;
    double length, v_sum, dev_sum, v_max, a_min, a_max, delta_absmax;
    EpisodeExt dev, veh, st;
    double rs[4];
};
__device__ __forceinline__ void jep_reset(EpisodeAcc &A, int k0)
{
    A.k0 = k0; A.n = 0; A.failed = 0; A.n_dev = 0; A.st_ticks_off = 0; A.replan_tick = -1; A.veh_who = -1; A.st_who = -1;
    A.length = 0.0; A.v_sum = 0.0; A.dev_sum = 0.0;
    A.v_max = NAN; A.a_min = NAN; A.a_max = NAN; A.delta_absmax = NAN;
    A.dev = EpisodeExt{NAN, -1}; A.veh = EpisodeExt{NAN, -1}; A.st = EpisodeExt{NAN, -1};
    for (int j = 0; j < 4; ++j) A.rs[j] = NAN;
}

// The episode's row; `end`: 0 running, 1 goal, 2 age.  Called by lane 0 alone.
__device__ __forceinline__ void jep_write(const EpisodeP &P, const EpisodeAcc &A, int b, long long row, int end)
{
    if (row >= (long long)P.ep_cap) return;
    int *I = P.ep_i + (size_t)row * JSIM_EP_NI;
    double *D = P.ep_d + (size_t)row * JSIM_EP_ND;
    const bool any = A.n > 0;
    const size_t q = (size_t)A.k0 * P.R.B + b;       // the slot of the episode's first tick (read only with a tick there)
    I[JSIM_EP_EGO] = b; I[JSIM_EP_K0] = A.k0; I[JSIM_EP_N] = A.n; I[JSIM_EP_END] = end;
    I[JSIM_EP_FAILED] = A.failed;
    I[JSIM_EP_DEV_TICK] = A.dev.tick;
    I[JSIM_EP_VEH_TICK] = A.veh.tick; I[JSIM_EP_VEH_WHO] = A.veh_who;
    const bool veh = any && P.veh_clear != nullptr;
    I[JSIM_EP_VEH_HIT_TICK] = veh ? P.veh_hit_tick[q] : -1;
    I[JSIM_EP_VEH_HIT_FRAME] = veh ? P.veh_hit_frame[q] : -1;
    I[JSIM_EP_ST_TICK] = A.st.tick; I[JSIM_EP_ST_WHO] = A.st_who;
    const int off = (any && P.st_clear != nullptr) ? P.st_off_tick[q] : -1;
    I[JSIM_EP_ST_OFF_TICK] = off;
    I[JSIM_EP_ST_OBSTACLE] = (off >= 0 && off < P.R.n_ticks) ? P.st_hit[(size_t)off * P.R.B + b] : -1;
    I[JSIM_EP_ST_TICKS_OFF] = A.st_ticks_off;
    I[JSIM_EP_REPLAN_TICK] = A.replan_tick;
    D[JSIM_EP_LENGTH] = any ? A.length : NAN;
    D[JSIM_EP_V_MEAN] = any ? A.v_sum / (double)A.n : NAN;
    D[JSIM_EP_V_MAX] = A.v_max;
    D[JSIM_EP_A_MIN] = A.a_min; D[JSIM_EP_A_MAX] = A.a_max;
    D[JSIM_EP_DELTA_ABSMAX] = A.delta_absmax;
    D[JSIM_EP_DEV_MAX] = A.dev.v;
    D[JSIM_EP_DEV_MEAN] = A.n_dev > 0 ? A.dev_sum / (double)A.n_dev : NAN;
    D[JSIM_EP_VEH_CLEAR] = A.veh.v;
    D[JSIM_EP_VEH_HIT_X] = veh ? P.veh_hit_xy[2 * q] : NAN;
    D[JSIM_EP_VEH_HIT_Y] = veh ? P.veh_hit_xy[2 * q + 1] : NAN;
    D[JSIM_EP_ST_CLEAR] = A.st.v;
    D[JSIM_EP_PM_MIN] = A.rs[0]; D[JSIM_EP_DRIVER_MIN] = A.rs[1]; D[JSIM_EP_CYCLIST_MIN] = A.rs[2]; D[JSIM_EP_DIST_MIN] = A.rs[3];
}

__global__ __launch_bounds__(64) void episode_summary_kernel(const EpisodeP P)
{
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks;
    long long row = P.ep_off[b];
    EpisodeAcc A;
    jep_reset(A, 0);
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        const int cnt = (n - k0c) < 64 ? (n - k0c) : 64;
        const size_t q = valid ? (size_t)k * B + b : 0;
        // this lane's tick
        int flag = 0, v_who = -1, s_who = -1, s_hit = -1, trig = 0;
        double step = 0.0, v = 0.0, a = NAN, delta = NAN, dev = NAN, v_clear = NAN, s_clear = NAN;
        double rs[4] = {NAN, NAN, NAN, NAN};
        if (valid) {
            flag = R.flags[q];
            const double *r = R.rec + JSIM_REC_FIELDS * q;
            double sx, sy, syaw;
            jrw_pose(R, b, k, sx, sy, syaw);
            const double dx = r[0] - sx, dy = r[1] - sy;
            step = sqrt(dx * dx + dy * dy);
            v = r[3]; delta = fabs(r[4]); a = r[5]; dev = r[6];
            if (P.veh_clear) { v_clear = P.veh_clear[q]; v_who = P.veh_who[q]; }
            if (P.st_clear) { s_clear = P.st_clear[q]; s_who = P.st_who[q]; s_hit = P.st_hit[q]; }
            if (P.rs_val) {
                for (int j = 0; j < 4; ++j) rs[j] = P.rs_val[4 * q + j];
                trig = P.rs_trig[q];
            }
        }
        const unsigned long long e_cur = jrw_end_mask(R, k, flag, false);
        // the segments of this chunk, written out here and not through jrw_segments: DESIGN.md section 20 has the measurement
        for (int pos = 0; pos < cnt;) {
            const unsigned long long rem = e_cur >> pos;
            const int e = rem ? pos + (int)__builtin_ctzll(rem) : cnt - 1;
            const bool ends = rem != 0ull;
            const bool in = lane >= pos && lane <= e;          // (e < cnt: every lane of the segment holds a tick)
            const unsigned long long seg = jrw_lanes(pos, e);
            int at = 0;
            A.n += e - pos + 1;
            A.failed += __popcll(__ballot(in && (flag & JSIM_REC_FAILED) != 0));
            A.length += jep_sum(in ? step : 0.0);
            A.v_sum += jep_sum(in ? v : 0.0);
            const bool has_dev = in && dev == dev;
            A.n_dev += __popcll(__ballot(has_dev));
            A.dev_sum += jep_sum(has_dev ? dev : 0.0);
            A.v_max = fmax(A.v_max, jep_max(in ? v : NAN));
            A.a_min = fmin(A.a_min, jep_min(in ? a : NAN));
            A.a_max = fmax(A.a_max, jep_max(in ? a : NAN));
            A.delta_absmax = fmax(A.delta_absmax, jep_max(in ? delta : NAN));
            jep_extreme(A.dev, in ? dev : NAN, false, k0c, at);
            if (P.veh_clear) {
                if (jep_extreme(A.veh, in ? v_clear : NAN, true, k0c, at)) A.veh_who = __shfl(v_who, at);
            }
            if (P.st_clear) {
                if (jep_extreme(A.st, in ? s_clear : NAN, true, k0c, at)) A.st_who = __shfl(s_who, at);
                A.st_ticks_off += __popcll(__ballot(in && s_hit >= 0));
            }
            if (P.rs_val) {
                for (int j = 0; j < 4; ++j) A.rs[j] = fmin(A.rs[j], jep_min(in ? rs[j] : NAN));
                const unsigned long long need = __ballot((trig & 1) != 0) & seg;
                if (A.replan_tick < 0 && need != 0ull) A.replan_tick = k0c + (int)__builtin_ctzll(need);
            }
            if (ends) {                                         // the episode ends with lane e's record
                const int f_end = __shfl(flag, e);
                if (lane == 0) jep_write(P, A, b, row, (f_end & JSIM_REC_GOAL) ? 1 : 2);
                ++row;
                jep_reset(A, k0c + e + 1);
            }
            pos = e + 1;
        }
    }
    if (lane == 0) jep_write(P, A, b, row, 0);                  // the running episode: always there, without a tick after an end
}
