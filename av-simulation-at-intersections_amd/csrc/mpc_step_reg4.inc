// mpc_step_reg4.inc -- register-resident MPC step for long horizons (written for T = 40: N = 2T = 80 decision variables):
// FOUR wavefronts per ego, TWO lanes per row.  (included by jsim_mpc.hip after reg_common.inc; same stages, decisions,
// tie rules and tolerances as the other kernels and as oracle/mpc_oracle.c)
//
// Why: with one lane per row a lane of the two-wave kernel carries 80 doubles of J = 160 VGPRs, the rest of the loop's state
// does not fit the 256 architectural VGPRs beside them (rows partly in AGPRs, 724 B of scratch) and every pass over a row is
// 80 dependent-issue FMAs.  Here a row is shared by an even / odd lane pair -- the even lane holds columns [0, T), the odd
// lane columns [T, 2T) -- so a lane carries 40 doubles, a pass is 40 FMAs, whatever is summed along a row (z = J2 d2, y = J2 v,
// the squared norms) is finished by ONE quad_perm DPP exchange inside the pair, and the kernel stays under 256 registers:
// no AGPR copies, no scratch, two workgroups per CU.
//
// Slot s = global lane >> 1 (128 slots), half = global lane & 1:
//   wave 0  slots   0..30   rows 0..30 of J          slot 31  ghost of row 31
//   wave 1  slots  32..61   rows 31..60              slot 62  ghost of row 61          (slot 63 idle)
//   wave 2  slots  64..82   rows 61..79              slots 83..95   speed rows t = 0..12:  dt * sum_{s<t} J[2s][:]
//   wave 3  slots  96..123  speed rows 13..40        slot 124 carries w = L^-1 g (u0 = -J w)     (slots 125..127 idle)
// The steer-rate rows of time t couple rows 2t+1 and 2t+3: the lane of row 2t+1 evaluates them against the slot two further
// on.  Where that partner lives in the next wave a GHOST repeats its arithmetic inside this wave -- lane-local functions of
// its own half row and of broadcast vectors, hence bit-identical -- and never offers candidate rows of its own.
// What crosses the waves goes through LDS behind s_barrier: the factor's column being eliminated, the four waves' winners of
// the entering-row search and the published row(s) of J (two barriers per active-set iteration), the Givens sweep of a
// drop.  Everything uniform (step lengths, ratio test, triangular solve with R, multipliers) is computed redundantly and
// identically in all four waves: working-set position k lives in lane k & 63, slot k >> 6, of EVERY wave.

__host__ __device__ constexpr int jsim_tile_wave4(int ntile, int a)
{
    // which of the four waves accumulates tile row a of H (costs (a + 1) * (T - 8a) MFMAs): T = 40 -> 40, 64, 72, 64, 40
    return ntile == 5 ? (a == 0 || a == 4 ? 0 : a) : (a & 3);
}

// The other lane of a pair: quad_perm [1,0,3,2].  The exchange must run with BOTH lanes active -- a DPP read from a lane that
// EXEC masks off returns 0 -- so its result is pinned where it stands: left to itself the compiler sinks the exchange into the
// `half == h ? own : partner's` select that consumes it and executes it for the receiving half only.
__device__ __forceinline__ double pair_swap(double v)
{
    double r = dpp_f64<DPP_QP_1032>(v);
    asm volatile("" : "+v"(r));
    return r;
}

#ifndef JSIM_REG4_MINW
#define JSIM_REG4_MINW 2 /* two workgroups (eight waves) per CU: at most 256 registers per lane */
#endif
// JSIM_PIN_WS (mpc_step_reg.inc): the working set's lane-distributed state (position k lives in lane k & 63: multiplier, 1 / R[k][k],
// canonical row id; and each pair's "my rows are in the set" bits) is written under a one-lane mask and read again many hundred
// instructions later.  Pinned right after every such write: the masked update stays where it stands, and the live ranges the
// allocator has to carry through the loop get shorter -- with these pins the kernel needs 232 registers and no scratch at all
// (256 and 12-20 B before).

template <int T, bool PRE>
__global__ __launch_bounds__(256, JSIM_REG4_MINW) void mpc_step_reg4_kernel(const KP P, const TickP K, const PreK Q)
{
    constexpr int N = 2 * T, NH = T, NR = 3 * T + 1, LD = N + 2, TP = T + 2, MW = (8 * T + 31) / 32, NP = N + 2;
    constexpr int NTILE = (N + 15) / 16;
    constexpr int G1 = 31, G2 = 61;           // the rows that have a ghost (slot 31 in wave 0, slot 62 in wave 1)
    constexpr int S2 = 64 + (N - G2);         // first speed-row slot
    constexpr int SW = S2 + T + 1;            // slot of w
    constexpr int CC = 8;                     // doubles per burst of broadcast reads
    static_assert((T & 1) == 0, "a half row must be a whole number of 16-byte pairs");
    static_assert(N > G2 + 2 && SW < 128, "slot map: rows 0..30 | 31..60 | 61..N-1 + speed rows | speed rows + w");
    static_assert(N <= 128 && NH % CC == 0, "");
    static_assert(!PRE || sizeof(PreScratch) <= sizeof(double) * N * LD, "the glue's scratch fits the Hessian area");

    __shared__ __attribute__((aligned(16))) double Hm[N * LD];   // H rows; then the factor's columns; then R (strict upper)
    __shared__ __attribute__((aligned(16))) double invv[NP];     // 1 / L[k][k]
    __shared__ __attribute__((aligned(16))) double gvec[NP];     // g
    __shared__ __attribute__((aligned(16))) double wvec[NP];     // w = L^-1 g
    constexpr int GSZ = 2 * N + 2 * NH;
    __shared__ __attribute__((aligned(16))) double gsvb[2 * GSZ]; // Givens (c, s) per column pair, identity outside a sweep, then NH identities -- twice: the drops alternate
    __shared__ __attribute__((aligned(16))) double drow12[2 * NP]; // d = Jhat'n+ : row la of Jhat, then the second row of a steer-rate normal
    double *const drow = drow12, *const drow2 = drow12 + NP;
    __shared__ __attribute__((aligned(16))) double dzv[4][NP];   // per wave: d with the working-set part zeroed (d2)
    __shared__ __attribute__((aligned(16))) double vzv[4][NP];   // per wave: Householder vector
    __shared__ __attribute__((aligned(16))) double rdv[NP];      // diagonal of R
    __shared__ __attribute__((aligned(16))) double uvec[NR + 5];
    __shared__ __attribute__((aligned(16))) double tq[TQ_COUNT * TP];
    __shared__ __attribute__((aligned(16))) double xwd[4][4];    // per wave: winner of the entering-row search (key, viol, dd)
    __shared__ int xwi[4][4];                                    // .. (la, lb, owner, obit) as slots
    __shared__ __attribute__((aligned(16))) double park[7][64];  // S3's per-time-step coefficients, parked across the active-set loop for S5
    // drop: per-wave scratch to shift the multipliers (positions 0 .. N-1) -- on top of the operand tables, dead once H is built
    static_assert(4 * (N + 2) * (sizeof(double) + sizeof(int)) <= sizeof(double) * TQ_COUNT * TP, "the drop scratch fits the table area");
    double (*const lamx)[N + 2] = reinterpret_cast<double (*)[N + 2]>(tq);
    int (*const actx)[N + 2] = reinterpret_cast<int (*)[N + 2]>(tq + 4 * (N + 2));
    __shared__ unsigned maskw[MW + 1];
    // what a lane would otherwise carry through the whole active-set loop in registers it does not have: the warm start of the
    // next tick (identical in the four waves: one copy) and the lane's two steepest-edge weights
    __shared__ __attribute__((aligned(16))) double wsv[2][T]; // [0]: accelerations, [1]: tan of the clamped steers
    __shared__ __attribute__((aligned(16))) double iwv[2][256];

    const int gl0 = threadIdx.x;
    if ((int)blockIdx.x >= P.B) return;
    const int ego = K.order ? K.order[blockIdx.x] : (int)blockIdx.x;
    if (P.pass > 0 && P.status[ego] != JSIM_OK) return; // failed in an earlier pass of this step: the failure stands
    const int pass = P.pass;
    const int it_base = (P.pass > 0 && P.n_iter) ? P.n_iter[ego] : 0;
    // launch constants parked in LDS and read back where they are used (see reg_common.inc)
    __shared__ KP Ps;
    __shared__ TickP Ks;
    if (gl0 == 0) {
        Ps = P; Ks = K;
        if (P.pe) jsim_apply_ego_cfg(Ps, P.pe, ego, P.T, P.dt);
    }
    __syncthreads();
    const volatile __attribute__((address_space(3))) KP &Pv = *(const volatile __attribute__((address_space(3))) KP *)&Ps;
    const volatile __attribute__((address_space(3))) TickP &Kv = *(const volatile __attribute__((address_space(3))) TickP *)&Ks;
    const int n_ticks = __builtin_amdgcn_readfirstlane(Kv.n_ticks);
    const int advance = __builtin_amdgcn_readfirstlane(Kv.advance);
    const int wave = __builtin_amdgcn_readfirstlane(gl0 >> 6);
    int gl = gl0, lane = gl0 & 63;

    // per-ego scalars come back from memory in vector registers: say that they are uniform
    const int pid = uni(gp(Pv.path_id)[ego]);
    const long long off = uni64(gp(Pv.poff)[pid]);
    long long M = uni64((long long)gp(Pv.path_len)[ego]);
    long long pre_idx = 0;
    int pre_prev = -1, pre_col = 0, pre_st = JSIM_OK, Mfull = 0, pre_cut = -1;
    ObsSlice pre_obs = {0, 0};   // the ego's slice of the obstacle tables: its traffic set, or all of them
    const double2 *pre_othr = nullptr; // .. and of the per-vehicle thresholds (NULL: no shape table)
    if (PRE) {
        pre_obs = traffic_slice(Q.traffic, ego, Q.pre.n_obs);
        pre_obs.first = uni(pre_obs.first); pre_obs.n = uni(pre_obs.n);
        if (Q.pre.othr) pre_othr = Q.pre.othr + pre_obs.first;
        pre_idx = Q.traj_idx[ego];
        pre_prev = Q.prev_len[ego];
        Mfull = (int)(gp(Pv.poff)[pid + 1] - off);
        if (Q.speed_cutoff) pre_cut = Q.cut_io[ego];
    }
    const double speed = uni(gp(Pv.speed)[ego]);
    const double dt = uni((double)Pv.dt);
    // `lane < T` (lane t of a wave speaks for time step t) is re-evaluated from the fenced lane id wherever it is needed: as a
    // variable it lived through the whole tick loop -- as a 0/1 vector register once the scalar registers ran out
#define tl (lane < T)
    // controller / plant state carried in registers across ticks (all four waves hold the same copy)
    long long s0 = uni64(gp(Pv.target_ind)[ego]);
    double sx = gp(Pv.x0)[4 * ego + 0], sy = gp(Pv.x0)[4 * ego + 1], sv = gp(Pv.x0)[4 * ego + 2], syaw = gp(Pv.x0)[4 * ego + 3];
#define WS_SET(a_, d_) do { if (wave == 0 && tl) { wsv[0][lane] = (a_); wsv[1][lane] = (d_); } } while (0)
    // (the steer entries as S2 uses them: tan of the clamped steer, evaluated once where the warm start is written -- here, and in S5 on
    //  the new solution, whose entry 0 is also the plant step's)
#define WS_TAN(d_, out_) do { const double sm_ = Pv.smax; double dc_ = (sm_ < (d_)) ? sm_ : (d_); dc_ = (-sm_ > dc_) ? -sm_ : dc_; out_ = tan(dc_); } while (0)
    {
        double wt0 = 0.0;
        if (wave == 0 && tl) { const double od0 = gp(Pv.od)[(size_t)ego * T + lane]; WS_TAN(od0, wt0); }
        WS_SET(gp(Pv.oa)[(size_t)ego * T + lane], wt0); // warm start, entry t; read back at S2 of every tick
    }
    __syncthreads();
    double di_prev = advance ? gp(Kv.di_ai)[2 * ego] : 0.0;
    double ai_last = advance ? gp(Kv.di_ai)[2 * ego + 1] : 0.0;
    int age = advance ? uni(gp(Kv.age)[ego]) : 0;
    const int hist_base = (advance && (Kv.hist || Kv.rec)) ? uni(*gp(Kv.tick)) : 0;
    double2 goal_xy = double2{0.0, 0.0};
    if (advance) { const jsim_d2v gq = ((JSIM_GAS const jsim_d2v *)Pv.pxy)[gp(Pv.poff)[pid + 1] - 1]; goal_xy = double2{uni(gq.x), uni(gq.y)}; }

    unsigned it_sum = 0; // active-set iterations of this launch's ticks, both S5 exits: added to work / iters behind the loop
    for (int tk = 0; tk < n_ticks; ++tk) {
    // (the lane id is re-derived from the execution mask count instead of keeping threadIdx.x alive across the kernel)
    // (.. from an opaque all-ones mask, or the count is computed once and kept alive all the same)
#define LANE_FENCE4() do { unsigned ones_ = ~0u; asm volatile("" : "+s"(ones_)); gl = (wave << 6) | (int)__builtin_amdgcn_mbcnt_hi(ones_, __builtin_amdgcn_mbcnt_lo(ones_, 0u)); asm volatile("" : "+v"(gl)); __builtin_assume(gl >= 0 && gl < 256); lane = gl & 63; } while (0)
    LANE_FENCE4();
    // the carried state is uniform: say so (scalar registers instead of 64 copies each)
    sx = uni(sx); sy = uni(sy); sv = uni(sv); syaw = uni(syaw); di_prev = uni(di_prev); ai_last = uni(ai_last);
    s0 = uni64(s0); M = uni64(M); age = uni(age);
    if (PRE) {
        PreScratch &W = *reinterpret_cast<PreScratch *>(Hm);
        PreP pre = Q.pre;
        pre.n_obs = pre_obs.n;
        const PreOut o = jsim_pre_tick_ego<true>(pre, Q.pred_cc_all + ((size_t)tk * Q.pre.n_obs + pre_obs.first) * Q.pre.n_steps * 2,
                                           Q.pred_bc_all + (size_t)tk * Q.pre.n_obs + pre_obs.first, pre_othr, W, lane, ego,
                                           off, Mfull, sx, sy, sv, pre_idx, pre_prev);
        pre_st = o.status;
        if (o.status == JSIM_OK) {
            pre_idx = o.idx; pre_col = o.col;
            if (Q.speed_cutoff) pre_cut = o.path_len; else M = o.path_len;
        }
        pre_prev = Q.speed_cutoff ? Mfull : (int)M;
        BLOCK_SYNC();
        LANE_FENCE4();
    }
    double a0n = 0.0, d0n = 0.0;
    int status = JSIM_OK;
    double p_sn = 0.0, p_cs = 0.0; // the plant step's sin / cos of the tick-start yaw: S2's lane 0, as uniform values
    bool p_sc = false;             // S2 ran in this tick
    double p_tn = 0.0;             // .. and tan of the clamped delta_0 of this tick's solution (S5)
    do {
    STAMP2(0);
    // ------------------------------------------------------------------ S1: nearest index in direction (every wave, redundantly)
    long long tind = s0;
    {
        long long len = M - s0;
        if (len < 0) len = 0;
        if (M < 1) {
            status = 3;
        } else if (len >= 3) {
            double b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
            int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
            JSIM_GAS const jsim_d2v *pp = (JSIM_GAS const jsim_d2v *)Pv.pxy + off + s0;
            const int ilen = (int)len;
#define INSERT_PT(p_, k_)                                                                      \
    {                                                                                          \
        const double dx = (p_).x - sx, dy = (p_).y - sy;                                       \
        const double d = sqrt(dx * dx + dy * dy); /* numpy: sqrt(add.reduce(x*x)) */           \
        if (d < b0) { b2 = b1; i2 = i1; b1 = b0; i1 = i0; b0 = d; i0 = (k_); }                 \
        else if (d < b1) { b2 = b1; i2 = i1; b1 = d; i1 = (k_); }                              \
        else if (d < b2) { b2 = d; i2 = (k_); }                                                \
    }
            int k = lane;
            for (; k + 192 < ilen; k += 256) {
                const jsim_d2v p0 = pp[k], p1 = pp[k + 64], p2 = pp[k + 128], p3 = pp[k + 192];
                INSERT_PT(p0, k) INSERT_PT(p1, k + 64) INSERT_PT(p2, k + 128) INSERT_PT(p3, k + 192)
            }
            for (; k < ilen; k += 64) {
                const jsim_d2v p0 = pp[k];
                INSERT_PT(p0, k)
            }
#undef INSERT_PT
            int gi[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double v = b0;
                int id = i0;
                wargmin_fast(v, id);
                gi[r] = id;
                if (i0 == id) { b0 = b1; i0 = i1; b1 = b2; i1 = i2; b2 = INFINITY; i2 = 0x7fffffff; }
            }
            const int g0 = gi[0], g1 = gi[1], g2 = gi[2];
            int d12 = g1 - g2; d12 = d12 < 0 ? -d12 : d12;
            int d01 = g0 - g1; d01 = d01 < 0 ? -d01 : d01;
            if (d12 == 2) tind = g0 + s0;
            else if (d01 == 1) tind = (g0 > g1 ? g0 : g1) + s0;
            else status = JSIM_NEAREST_ANOMALY;
        } else if (len == 2) {
            tind = s0 + 1;
        }
    }
    tind = uni64(tind); // the same in every lane (wave-wide arg-min): scalar registers
    if (status != JSIM_OK) { // the reference raises: nothing of the controller is updated
        if (gl == 0) {
            gp(Pv.status)[ego] = status;
            if (Pv.n_iter) gp(Pv.n_iter)[ego] = it_base;
        }
        break;
    }

    LANE_FENCE4();
    STAMP2(1);
    // ------------------------------------------------------------------ S1: travel -> idx -> xref   (lane t <= T of each wave)
    const int tl_idx = lane < T ? lane : T;
    double xr, yr, yawr, vr = 0.0;
    v4d ytr = v4d{0.0, 0.0, 0.0, 0.0}; // {c1, s1, c2, s2} of S3's weights, from the path table's trig (P.ptrig)
    bool rend;
    long long ik;
    {
        const double vref = (Pv.vref_min > sv) ? Pv.vref_min : sv;
        const double cstep = fabs(vref) * dt;
        double trav = cstep;
        if (pass == 0) {
#pragma unroll
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + cstep;
        } else { // re-linearisation pass: ov = the previous pass's predicted speeds (mpc.py:232,101)
            JSIM_GAS const double *ovp = gp((const double *)Pv.ov) + (size_t)ego * (T + 1);
            trav = fabs(ovp[0]) * dt;
#pragma unroll
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + fabs(ovp[j]) * dt;
        }
        ik = (long long)rint(trav / Pv.dl) + tind;
        if (ik > M - 1) ik = M - 1;
        const jsim_d2v pr = ((JSIM_GAS const jsim_d2v *)Pv.pxy)[off + ik];
        xr = pr.x; yr = pr.y; yawr = gp(Pv.pyaw)[off + ik];
        if (Pv.ptrig) ytr = ((JSIM_GAS const v4d *)Pv.ptrig)[off + ik]; // (here, not in S3: it rides the round trip of the two loads above)
        rend = (ik == M - 1);
        if (Pv.pcv) {
            const int cut = (PRE && Q.speed_cutoff) ? pre_cut : (Pv.cv_cut ? gp(Pv.cv_cut)[ego] : -1);
            vr = (cut < 0 || ik < cut) ? gp(Pv.pcv)[off + ik] : 0.0;
        }
    }
    if (speed - sv < -JSIM_FEAS_TOL || sv - Pv.vmin < -JSIM_FEAS_TOL) status = JSIM_INFEASIBLE;
    status = uni(status); // decided by vector compares of uniform values: a scalar from here on

    LANE_FENCE4();
    STAMP2(2);
    // ------------------------------------------------------------------ S2: rollout of the warm start
    double bx = sx, by = sy, bv = sv, bth = syaw, sn, cs;
    {
        const double vmaxp_ = Pv.vmax_plant, vmin_ = Pv.vmin;
        const double wa_t = tl ? wsv[0][lane] : 0.0;
        const double tan_t = tl ? wsv[1][lane] : 0.0; // tan of the clamped steer, evaluated where the warm start was written
        double vcur = sv;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            double vn = vcur + rdlane(wa_t, j) * dt;
            vn = (vmaxp_ < vn) ? vmaxp_ : vn;
            vn = (vmin_ > vn) ? vmin_ : vn;
            vcur = vn;
            if (lane == j + 1) bv = vn;
        }
        const double w = ((bv / Pv.L) * tan_t) * dt;
        double thcur = syaw;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            thcur = thcur + rdlane(w, j);
            if (lane == j + 1) bth = thcur;
        }
        sincos(bth, &sn, &cs);
        if (Pv.dbg_xbar) { // the x and y sums have one reader, the debug entry's xbar: no solve needs them
            const double ix = (bv * cs) * dt, iy = (bv * sn) * dt;
            double xcur = sx, ycur = sy;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                xcur = xcur + rdlane(ix, j);
                ycur = ycur + rdlane(iy, j);
                if (lane == j + 1) { bx = xcur; by = ycur; }
            }
        }
    }
    p_sn = rdlane(sn, 0); p_cs = rdlane(cs, 0); p_sc = true;
    if (wave == 0) {
        if (Pv.dbg_xbar && lane <= T) {
            double *xb = Pv.dbg_xbar + (size_t)ego * 4 * (T + 1);
            xb[0 * (T + 1) + lane] = bx; xb[1 * (T + 1) + lane] = by;
            xb[2 * (T + 1) + lane] = bv; xb[3 * (T + 1) + lane] = bth;
        }
        if (Pv.dbg_idx && lane <= T) Pv.dbg_idx[(size_t)ego * (T + 1) + lane] = ik;
        if (Pv.xref && lane <= T) {
            JSIM_GAS double *xf = gp((double *)Pv.xref) + (size_t)ego * 4 * (T + 1);
            xf[0 * (T + 1) + lane] = xr; xf[1 * (T + 1) + lane] = yr;
            xf[2 * (T + 1) + lane] = vr; xf[3 * (T + 1) + lane] = yawr;
        }
    }
    if (status == JSIM_INFEASIBLE) {
        LANE_FENCE4(); // a lane id of its own: the block must not keep an earlier phase's alive
        if (wave == 0 && tl) { gp(Pv.oa)[(size_t)ego * T + lane] = 0.0; gp(Pv.od)[(size_t)ego * T + lane] = 0.0; }
        WS_SET(0.0, 0.0); s0 = tind;
        if (Pv.amask && gl < MW) gp(Pv.amask)[(size_t)ego * MW + gl] = 0u;
        if (gl == 0) {
            gp(Pv.status)[ego] = status;
            gp(Pv.target_ind)[ego] = tind;
            if (Pv.n_iter) gp(Pv.n_iter)[ego] = it_base;
        }
        break;
    }

    LANE_FENCE4();
    STAMP2(3);
    // ------------------------------------------------------------------ S3: linearisation coefficients (lane t < T)
    { // S3 scope: al .. kt live on in `park`, not in registers
    double al = 0, be = 0, alp = 0, bep = 0, ccx = 0, ccy = 0, kt = 0;
    if (tl) {
        al = dt * cs;
        be = (-dt * bv) * sn;
        alp = dt * sn;
        bep = (dt * bv) * cs;
        ccx = ((dt * bv) * sn) * bth;
        ccy = ((-dt * bv) * cs) * bth;
        kt = (dt * bv) / Pv.L;
    }
    if (wave == 0) {
        park[0][lane] = al; park[1][lane] = be; park[2][lane] = alp; park[3][lane] = bep;
        park[4][lane] = ccx; park[5][lane] = ccy; park[6][lane] = kt;
    }
    {
        const double PA = wexscan_dpp(al, lane), PB = wexscan_dpp(be, lane);
        const double PAP = wexscan_dpp(alp, lane), PBP = wexscan_dpp(bep, lane);
        const double FX = sx + wexscan_dpp(fma(al, sv, fma(be, syaw, ccx)), lane);
        const double FY = sy + wexscan_dpp(fma(alp, sv, fma(bep, syaw, ccy)), lane);
        double Qxx = 0, Qxy = 0, Qyy = 0, qv = 0, qyaw = 0;
        if (lane >= 1 && lane <= T) {
            if (!rend) {
                double c1 = ytr.x, s1 = ytr.y, c2 = ytr.z, s2 = ytr.w;
                if (!Pv.ptrig) { // no table (JSIM_PATH_TRIG=0): what path_trig_kernel evaluates, here
                    const double a1 = yawr + 0.5 * M_PI;   // (sincos: one argument reduction per angle; the same values as cos() and sin() -- checked bit for bit)
                    sincos(a1, &s1, &c1); sincos(yawr, &s2, &c2);
                }
                Qxx = (c1 * c1) * Pv.w_perp + (c2 * c2) * Pv.w_para;
                Qxy = (c1 * s1) * Pv.w_perp + (c2 * s2) * Pv.w_para;
                Qyy = (s1 * s1) * Pv.w_perp + (s2 * s2) * Pv.w_para;
                qv = Pv.Qv; qyaw = Pv.Qyaw;
            } else {
                Qxx = Pv.Qf0; Qyy = Pv.Qf1; qv = Pv.Qf2; qyaw = Pv.Qf3;
            }
        }
        const double ex = FX - xr, ey = FY - yr, ev = sv - vr, eyaw = syaw - yawr;
        if (wave == 0 && lane <= T + 1) {
            const int t = lane;
            const bool in = lane <= T;
            tq[TQ_PA * TP + t] = PA; tq[TQ_PB * TP + t] = PB; tq[TQ_PAP * TP + t] = PAP; tq[TQ_PBP * TP + t] = PBP;
            tq[TQ_KT * TP + t] = kt;
            tq[TQ_QXX * TP + t] = in ? Qxx : 0; tq[TQ_QXY * TP + t] = in ? Qxy : 0; tq[TQ_QYY * TP + t] = in ? Qyy : 0;
            tq[TQ_QV * TP + t] = in ? qv : 0; tq[TQ_QYAW * TP + t] = in ? qyaw : 0;
            tq[TQ_QEX * TP + t] = in ? fma(Qxx, ex, Qxy * ey) : 0;
            tq[TQ_QEY * TP + t] = in ? fma(Qxy, ex, Qyy * ey) : 0;
            tq[TQ_QEV * TP + t] = in ? qv * ev : 0;
            tq[TQ_QEYAW * TP + t] = in ? qyaw * eyaw : 0;
            tq[TQ_REND * TP + t] = (in && rend) ? 1.0 : 0.0;
            tq[TQ_ONE * TP + t] = 1.0; tq[TQ_ZERO * TP + t] = 0.0;
        }
    }
    } // S3 scope
    BLOCK_SYNC();

    LANE_FENCE4();
    STAMP2(4);
    // ------------------------------------------------------------------ slot map of this lane
    // (re-derived from the fenced lane id at every phase boundary, like `lane` itself: otherwise the per-column exec masks of
    // all the unrolled phases are computed up front and kept -- SGPR pairs spilled to VGPR lanes, then VGPRs to scratch)
    int slot, half, jrow, tsp, cbase;
    bool ghost, realrow, isw;
#define SLOTMAP4()                                                                                      \
    do {                                                                                                \
        slot = gl >> 1; half = gl & 1;                                                                  \
        jrow = -1; ghost = false;           /* row of J held by this pair (ghosts included), -1: none */ \
        if (slot < G1) jrow = slot;                                                                     \
        else if (slot == G1) { jrow = G1; ghost = true; }                                               \
        else if (slot < G2 + 1) jrow = slot - 1;                                                        \
        else if (slot == G2 + 1) { jrow = G2; ghost = true; }                                           \
        else if (slot >= 64 && slot < S2) jrow = slot - 3;                                              \
        realrow = jrow >= 0 && !ghost;                                                                  \
        tsp = (slot >= S2 && slot < SW) ? slot - S2 : -1; /* speed row t */                             \
        isw = slot == SW;                                                                               \
        cbase = NH * half;                  /* first column of this lane's half row */                  \
    } while (0)
    SLOTMAP4();
#define SLOT_OF_ROW(r) ((r) < G1 ? (r) : ((r) < G2 ? (r) + 1 : (r) + 3))

    // ------------------------------------------------------------------ S4a: H = 2 S'QS (fp64 MFMA), tile rows split over the four waves
    double gi_own = 0.0;
    {
        const int kk = lane >> 4, cc = lane & 15;
        double c0[NTILE], c1[NTILE], p0[NTILE], p1[NTILE];
        int thr[NTILE];
        const bool isd_ = cc & 1; // 16 c is even: the column kind does not depend on the tile
        const int xrow = (kk < 2 ? (isd_ ? TQ_PB : TQ_PA) : TQ_ONE) * TP, yrow = (kk < 2 ? (isd_ ? TQ_PBP : TQ_PAP) : TQ_ONE) * TP;
        const int w0row = (kk == 0 ? TQ_QXX : kk == 1 ? TQ_QXY : kk == 2 ? TQ_QV : TQ_QYAW) * TP;
        const int w1row = (kk == 0 ? TQ_QXY : kk == 1 ? TQ_QYY : TQ_ZERO) * TP;
#pragma unroll
        for (int c = 0; c < NTILE; ++c) {
            const int col = 16 * c + cc;
            const bool vcol = col < N;
            const int s = vcol ? (col >> 1) : (T - 1);
            const double ks = tq[TQ_KT * TP + s];
            const double coef = vcol ? (isd_ ? ks : dt) : 0.0;
            const double c23 = !vcol ? 0.0 : (kk == 2 ? (isd_ ? 0.0 : dt) : (kk == 3 ? (isd_ ? ks : 0.0) : 0.0));
            c0[c] = kk < 2 ? coef : c23;
            c1[c] = kk < 2 ? coef : 0.0;
            p0[c] = kk < 2 ? tq[xrow + s + 1] : 0.0;
            p1[c] = kk < 2 ? tq[yrow + s + 1] : 0.0;
            thr[c] = vcol ? (kk < 2 ? s + 2 : s + 1) : (T + 2); // invalid columns never start
        }
        // g: waves 1 and 3 (the ones with fewer MFMAs) take one column each per lane
        const int gcol = wave == 1 ? lane : (wave == 3 ? 64 + lane : N);
        const int so = gcol < N ? (gcol >> 1) : (T - 1);
        const bool isdo = gcol & 1;
        const double kso = tq[TQ_KT * TP + so];
        const double coefo = gcol < N ? (isdo ? kso : dt) : 0.0;
        const double pox = isdo ? tq[TQ_PB * TP + so + 1] : tq[TQ_PA * TP + so + 1];
        const double poy = isdo ? tq[TQ_PBP * TP + so + 1] : tq[TQ_PAP * TP + so + 1];
        const int gxrow = (isdo ? TQ_PB : TQ_PA) * TP, gyrow = (isdo ? TQ_PBP : TQ_PAP) * TP;

        auto hbuild = [&](auto wsel) {
            constexpr int W = decltype(wsel)::value;
            constexpr bool GW = (W == 1 || W == 3);
            v4d acc[NTILE][NTILE];
#pragma unroll
            for (int a = 0; a < NTILE; ++a)
#pragma unroll
                for (int b = 0; b < NTILE; ++b) acc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 1; t <= T; ++t) {
                const double X = tq[xrow + t], Y = tq[yrow + t], W0 = tq[w0row + t], W1 = tq[w1row + t];
                double aval[NTILE], bval[NTILE];
#pragma unroll
                for (int c = 0; c < NTILE; ++c) {
                    const bool on = t >= thr[c];
                    const double S0 = on ? c0[c] * (X - p0[c]) : 0.0;
                    const double S1 = on ? c1[c] * (Y - p1[c]) : 0.0;
                    aval[c] = kk == 1 ? S1 : S0;
                    bval[c] = fma(W0, S0, W1 * S1);
                }
#pragma unroll
                for (int a = 0; a < NTILE; ++a) {
                    if (jsim_tile_wave4(NTILE, a) == W && t >= 8 * a + 1) {
#pragma unroll
                        for (int b = 0; b <= a; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[a], bval[b], acc[a][b], 0, 0, 0);
                    }
                }
                // g_i += S_t[:, i]' (Q_t e_t)
                if (GW && t > so) {
                    gi_own = fma(coefo, isdo ? tq[TQ_QEYAW * TP + t] : tq[TQ_QEV * TP + t], gi_own);
                    if (t >= so + 2) {
                        gi_own = fma(coefo * (tq[gxrow + t] - pox), tq[TQ_QEX * TP + t], gi_own);
                        gi_own = fma(coefo * (tq[gyrow + t] - poy), tq[TQ_QEY * TP + t], gi_own);
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < NTILE; ++a) {
                if (jsim_tile_wave4(NTILE, a) != W) continue;
#pragma unroll
                for (int b = 0; b <= a; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * a + kk + 4 * r, col = 16 * b + cc;
                        if (row < N && col < N) {
                            const double hv = 2.0 * acc[a][b][r];
                            Hm[row * LD + col] = hv;
                            if (a != b) Hm[col * LD + row] = hv;
                        }
                    }
            }
        };
        if (wave == 0) hbuild(std::integral_constant<int, 0>{});
        else if (wave == 1) hbuild(std::integral_constant<int, 1>{});
        else if (wave == 2) hbuild(std::integral_constant<int, 2>{});
        else hbuild(std::integral_constant<int, 3>{});
        gi_own = gcol < N ? 2.0 * gi_own : 0.0;
        if (gcol < N) gvec[gcol] = gi_own;
    }
    BLOCK_SYNC();
    LANE_FENCE4();
    SLOTMAP4();
    STAMP2(5);
    // half rows to registers, with the input cost R / R_end (mpc.py:180-183) and difference cost Rd (mpc.py:186) added
    double A[NH]; // columns cbase .. cbase + NH - 1 of row jrow of H; during the factorisation: the not yet eliminated part
    {
        const int i = realrow ? jrow : 0;
#pragma unroll
        for (int c = 0; c < NH; c += 2) {
            const double2 h2 = *(const double2 *)&Hm[i * LD + cbase + c];
            A[c] = h2.x; A[c + 1] = h2.y;
        }
        const int t = i >> 1, cu = i & 1;
        const double Rt = (tq[TQ_REND * TP + t] != 0.0) ? (cu ? Pv.Re1 : Pv.Re0) : (cu ? Pv.R1 : Pv.R0);
        const double rdc = 2.0 * (cu ? Pv.Rd1 : Pv.Rd0);
        const int nd = (T >= 2) ? ((t == 0 || t == T - 1) ? 1 : 2) : 0;
        const int il = i - cbase; // position of the diagonal inside this half (may fall outside)
#pragma unroll
        for (int c = 0; c < NH; ++c) {
            if (c == il) A[c] += 2.0 * Rt + nd * rdc;
            if (c == il + 2 || c + 2 == il) A[c] -= rdc;
        }
    }
    if (Pv.dbg_g && wave == 0) {
        for (int e = lane; e < N; e += 64) Pv.dbg_g[(size_t)ego * N + e] = gvec[e];
    }
    if (Pv.dbg_H && realrow) {
        double *Hd = Pv.dbg_H + (size_t)ego * N * N + (size_t)jrow * N + cbase;
#pragma unroll
        for (int c = 0; c < NH; ++c) Hd[c] = A[c];
    }
    double gmax;
    {
        double ga = lane < N ? fabs(gvec[lane]) : 0.0;
        if (lane + 64 < N) ga = fmax(ga, fabs(gvec[lane + 64]));
        gmax = uni(wmax_dpp(ga));
    }
    BLOCK_SYNC(); // every row of H is in registers: Hm now receives the factor's columns

    LANE_FENCE4();
    SLOTMAP4();
    STAMP2(6);
    // ------------------------------------------------------------------ S4b: Cholesky, right-looking by PANELS of PB columns, two barriers per panel
    // (Round 2 eliminated one column per barrier: 80 barriers, 933 cycles per column, each column a chain write -> barrier -> read
    // -> rsqrt -> pair exchange -> FMAs.)  A panel P = [p0, p0 + PB) lies in one half (NH % PB == 0):
    //   1. the lanes whose half holds P publish the current entries of their row in columns P:  Hm[(p0 + r) * LD + jrow];   barrier A
    //   2. EVERY lane reads the PB x PB diagonal block (broadcast) and factors it in registers -- redundantly, identical arithmetic,
    //      no exchange -- then solves its own row against it:  l_r = (a_r - sum_{s<r} l_s Lp[r][s]) / Lp[r][r]  (its a_r read back
    //      from what was published, so that both lanes of a pair compute the same l);
    //   3. rows below the panel store l (the scaled entries L[jrow][p0 + r]) over what they published;                        barrier B
    //      (the PB pivot rows store theirs after the barrier: the block they would overwrite is still being read, and nobody needs
    //      their entries before the forward substitution)
    //   4. trailing update  A[c] -= sum_r l_r L[c][p0 + r]  of the columns right of the panel, in the order r = 0 .. PB - 1.
    // The factor is now stored SCALED (Hm[k * LD + j] = L[j][k], j > k; invv[k] = 1 / L[k][k]).
    constexpr int PB = 8, NPH = NH / PB;
    static_assert(NH % PB == 0 && PB % 2 == 0, "a panel lies inside one half row");
    {
        JSIM_OPAQUE_ZERO(zc_);
        const double *const HmC = Hm + zc_;
        double *const invW = invv + zc_;
        const int rowi = realrow ? jrow : 0;      // (slots without a row of H act as row 0: dead after the first panel, never stored)
        auto chol_panel = [&](const int pi, auto hsel) __attribute__((always_inline)) {
            constexpr int hp = decltype(hsel)::value;
            const int pc = PB * pi, p0 = NH * hp + pc;
            if (realrow && half == hp && jrow >= p0) {
#pragma unroll
                for (int r = 0; r < PB; ++r) Hm[(p0 + r) * LD + jrow] = A[pc + r];
            }
            BLOCK_SYNC();
            // the diagonal block, lower triangle D[i][r] = Hm[(p0 + r) * LD + p0 + i] (i >= r), and this row's entries
            double Lp[PB][PB], inv[PB], a[PB];
#pragma unroll
            for (int r = 0; r < PB; ++r) {
#pragma unroll
                for (int i = (r & ~1); i < PB; i += 2) {
                    const double2 d2 = lds_ld2(&HmC[(p0 + r) * LD + p0 + i]);
                    Lp[i][r] = d2.x; Lp[i + 1][r] = d2.y;
                }
                a[r] = Hm[(p0 + r) * LD + rowi];
            }
            JSIM_STAGE();
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                double d = Lp[r][r];
#pragma unroll
                for (int s_ = 0; s_ < r; ++s_) d = fma(-Lp[r][s_], Lp[r][s_], d);
                if (!(d > 0.0)) d = 1e-300;
                inv[r] = fast_rsqrt(d);
#pragma unroll
                for (int i = r + 1; i < PB; ++i) {
                    double v = Lp[i][r];
#pragma unroll
                    for (int s_ = 0; s_ < r; ++s_) v = fma(-Lp[i][s_], Lp[r][s_], v);
                    Lp[i][r] = v * inv[r];
                }
            }
            double l[PB];
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                double v = a[r];
#pragma unroll
                for (int s_ = 0; s_ < r; ++s_) v = fma(-l[s_], Lp[r][s_], v);
                l[r] = v * inv[r];
                JSIM_PIN(l[r]);
            }
            if (gl == 0) {
#pragma unroll
                for (int r = 0; r < PB; ++r) invW[p0 + r] = inv[r];
            }
            if (realrow && half == hp && jrow >= p0 + PB) {
#pragma unroll
                for (int r = 0; r < PB; ++r) Hm[(p0 + r) * LD + jrow] = l[r];
            }
            BLOCK_SYNC();
            if (realrow && half == hp && jrow >= p0 && jrow < p0 + PB) {
#pragma unroll
                for (int r = 0; r < PB; ++r)
                    if (r < jrow - p0) Hm[(p0 + r) * LD + jrow] = l[r];
            }
            // trailing update: A[c] -= l_r L[c][p0 + r] for the columns right of the panel (low-half panels: the low lanes keep
            // "updating" their dead columns in step with the high lanes, which have all of theirs to do -- no masks)
            const int c_lo = hp ? pc + PB : 0;
            if (c_lo < NH) {
#pragma unroll
                for (int r = 0; r < PB; ++r) {
                    const double tmul = l[r];
                    const int k = p0 + r;
                    const int nch = (NH - c_lo + CC - 1) / CC;
                    double2 cb[2][CC / 2];
#pragma unroll
                    for (int c = c_lo; c < c_lo + CC && c < NH; c += 2) cb[0][(c - c_lo) / 2] = lds_ld2(&HmC[k * LD + cbase + c]);
#pragma unroll
                    for (int ch = 0; ch < nch; ++ch) {
                        const int h = c_lo + ch * CC;
                        if (ch + 1 < nch) {
#pragma unroll
                            for (int c = h + CC; c < h + 2 * CC && c < NH; c += 2) cb[(ch + 1) & 1][(c - h - CC) / 2] = lds_ld2(&HmC[k * LD + cbase + c]);
                        }
                        JSIM_STAGE();
#pragma unroll
                        for (int c = h; c < h + CC && c < NH; c += 2) {
                            const double2 c2 = cb[ch & 1][(c - h) / 2];
                            A[c] = fma(-tmul, c2.x, A[c]); JSIM_PIN(A[c]);
                            A[c + 1] = fma(-tmul, c2.y, A[c + 1]); JSIM_PIN(A[c + 1]);
                        }
                        JSIM_STAGE();
                    }
                }
            }
        };
#pragma unroll
        for (int pi = 0; pi < NPH; ++pi) chol_panel(pi, std::integral_constant<int, 0>{});
#pragma unroll
        for (int pi = 0; pi < NPH; ++pi) chol_panel(pi, std::integral_constant<int, 1>{});
    }
    BLOCK_SYNC();

    LANE_FENCE4();
    SLOTMAP4();
    STAMP2(7);
    // ------------------------------------------------------------------ half rows of the augmented J:  L y = rhs, panel by panel
    //   rows of J (ghosts too): rhs = e_row -> y = row of J = L^-T ; speed row t: rhs = dt * sum_{s<t} e_{2s} ; w: rhs = g
    // Panel P = [m0, m0 + PB): the pair's lane that holds columns P solves the PB x PB triangle in registers (the block's entries
    // are broadcast reads), hands the PB values y_r to its partner by DPP, and both lanes take  rhs_j -= L[j][m0 + r] y_r  for
    // their columns right of the panel (the low lanes of a low-half panel take a zero multiplier for the columns left of it).
    // No barrier: the factor is complete.  (Round 2: one column at a time, 603 cycles per column on one dependent chain.)
    double Jr[NH];
    {
        JSIM_OPAQUE_ZERO(zj_);
        const double *const HmJ = Hm + zj_, *const invJ = invv + zj_, *const gvJ = gvec + zj_;
        const int erow = jrow;                    // -1 for speed rows, w, idle slots
        const int nspd = tsp > 0 ? tsp : 0;       // even entries j < 2 * nspd of a speed row's right-hand side are dt
#pragma unroll
        for (int c = 0; c < NH; c += 2) {
            const int j = cbase + c;
            const double2 g2 = *(const double2 *)&gvJ[j];
            double r0 = isw ? g2.x : 0.0, r1 = isw ? g2.y : 0.0;
            r0 = (erow == j) ? 1.0 : r0;
            r1 = (erow == j + 1) ? 1.0 : r1;
            r0 = ((j >> 1) < nspd) ? dt : r0;
            Jr[c] = r0; Jr[c + 1] = r1;
        }
        auto fsub_panel = [&](const int pi, auto hsel) __attribute__((always_inline)) {
            constexpr int hm = decltype(hsel)::value;
            const int mc = PB * pi, m0 = NH * hm + mc;
            double Lp[PB][PB], inv[PB];
#pragma unroll
            for (int s_ = 0; s_ + 1 < PB; ++s_) {
#pragma unroll
                for (int i = ((s_ + 1) & ~1); i < PB; i += 2) {
                    const double2 d2 = lds_ld2(&HmJ[(m0 + s_) * LD + m0 + i]);
                    Lp[i][s_] = d2.x; Lp[i + 1][s_] = d2.y;
                }
            }
#pragma unroll
            for (int r = 0; r < PB; r += 2) { const double2 i2 = lds_ld2(&invJ[m0 + r]); inv[r] = i2.x; inv[r + 1] = i2.y; }
            JSIM_STAGE();
            double y[PB], ym[PB];
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                double v = Jr[mc + r];
#pragma unroll
                for (int s_ = 0; s_ < r; ++s_) v = fma(-Lp[r][s_], y[s_], v);
                y[r] = v * inv[r];
            }
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                const double yo = pair_swap(y[r]);              // (evaluated by both lanes: see pair_swap)
                ym[r] = (half == hm) ? y[r] : yo;
                if (half == hm) Jr[mc + r] = y[r];
            }
            const int c_lo = hm ? mc + PB : 0;
            if (c_lo < NH) {
#pragma unroll
                for (int r = 0; r < PB; ++r) {
                    const int m = m0 + r;
                    const double smul = ym[r];
                    const double smul_hi = half ? smul : 0.0;   // the multiplier where only the high lanes have a live column
                    const int nch = (NH - c_lo + CC - 1) / CC;
                    double2 cb[2][CC / 2];
#pragma unroll
                    for (int c = c_lo; c < c_lo + CC && c < NH; c += 2) cb[0][(c - c_lo) / 2] = lds_ld2(&HmJ[m * LD + cbase + c]);
#pragma unroll
                    for (int ch = 0; ch < nch; ++ch) {
                        const int h = c_lo + ch * CC;
                        if (ch + 1 < nch) {
#pragma unroll
                            for (int c = h + CC; c < h + 2 * CC && c < NH; c += 2) cb[(ch + 1) & 1][(c - h - CC) / 2] = lds_ld2(&HmJ[m * LD + cbase + c]);
                        }
                        JSIM_STAGE();
#pragma unroll
                        for (int c = h; c < h + CC && c < NH; c += 2) {
                            const double2 c2 = cb[ch & 1][(c - h) / 2];
                            // panel in the low half: its lanes update only the columns right of it, the high lanes every column;
                            // panel in the high half: the high lanes only (c_lo skips what lies left of it)
                            Jr[c] = fma(-c2.x, (!hm && c >= mc + PB) ? smul : smul_hi, Jr[c]); JSIM_PIN(Jr[c]);
                            Jr[c + 1] = fma(-c2.y, (!hm && c + 1 >= mc + PB) ? smul : smul_hi, Jr[c + 1]); JSIM_PIN(Jr[c + 1]);
                        }
                        JSIM_STAGE();
                    }
                }
            }
        };
#pragma unroll
        for (int pi = 0; pi < NPH; ++pi) fsub_panel(pi, std::integral_constant<int, 0>{});
#pragma unroll
        for (int pi = 0; pi < NPH; ++pi) fsub_panel(pi, std::integral_constant<int, 1>{});
    }
    if (isw) {
#pragma unroll
        for (int c = 0; c < NH; c += 2) *(double2 *)&wvec[cbase + c] = double2{Jr[c], Jr[c + 1]};
    }
    BLOCK_SYNC(); // w is published; nobody reads the factor's columns any more

    LANE_FENCE4();
    SLOTMAP4();
    STAMP2(8);
    // ------------------------------------------------------------------ unconstrained optimum  val = -Jhat w  (+ v0 on the speed rows)
    double val = 0.0;
    {
        double v0 = 0.0, v1 = 0.0;
        JSIM_OPAQUE_ZERO(zw_);
        const double *const wvW = wvec + zw_ + cbase;
#pragma unroll
        for (int h = 0; h < NH; h += CC) {
            double2 wb[CC / 2];
#pragma unroll
            for (int c = h; c < h + CC && c < NH; c += 2) wb[(c - h) / 2] = lds_ld2(&wvW[c]);
            JSIM_STAGE();
#pragma unroll
            for (int c = h; c < h + CC && c < NH; c += 2) {
                v0 = fma(-Jr[c], wb[(c - h) / 2].x, v0);
                v1 = fma(-Jr[c + 1], wb[(c - h) / 2].y, v1);
            }
            JSIM_PIN(v0); JSIM_PIN(v1);
            JSIM_STAGE();
        }
        const double vh = v0 + v1;
        val = vh + pair_swap(vh);
        if (tsp >= 0) val += sv;
    }
    // Hm becomes R (strict upper triangle, row k at Rm[k*LD + .]; zeros on/below the diagonal and from column q on)
    double *const Rm = Hm;
    for (int e = gl; e < N * LD / 2; e += 256) *(double2 *)&Rm[2 * e] = double2{0.0, 0.0};
    if (gl < GSZ) { gsvb[2 * gl] = 1.0; gsvb[2 * gl + 1] = 0.0; } // GSZ pairs = both buffers
    if (gl < 2) {
        drow[N + gl] = 0.0; drow2[N + gl] = 0.0;
#pragma unroll
        for (int w_ = 0; w_ < 4; ++w_) { dzv[w_][N + gl] = 0.0; vzv[w_][N + gl] = 0.0; }
    }
    BLOCK_SYNC();

    LANE_FENCE4();
    SLOTMAP4();
    STAMP2(9);
    // ------------------------------------------------------------------ Goldfarb-Idnani dual active-set iterations
    // candidate rows per pair as in the other register kernels (both lanes of a pair evaluate them identically); ghosts offer
    // none.  Ids and bounds are functions of the slot: they are re-derived inside every search (a dozen VALU instructions and
    // four LDS reads of the parked constants) instead of living in eight registers the loop does not have.
    // static steepest-edge weights  w = n'H^-1 n = ||Jhat'n||^2 at the start of the solve
    {
        double iw01, iw23;
        double rn0 = 0.0, rn1 = 0.0, dn0 = 0.0, dn1 = 0.0;
#pragma unroll
        for (int c = 0; c < NH; c += 2) {
            rn0 = fma(Jr[c], Jr[c], rn0); rn1 = fma(Jr[c + 1], Jr[c + 1], rn1);
            const double n0 = __shfl_down(Jr[c], 4), n1 = __shfl_down(Jr[c + 1], 4); // the slot two further on, same half
            const double e0 = n0 - Jr[c], e1 = n1 - Jr[c + 1];
            dn0 = fma(e0, e0, dn0); dn1 = fma(e1, e1, dn1);
        }
        const double rnh = rn0 + rn1, dnh = dn0 + dn1;
        const double rn = rnh + pair_swap(rnh), dn = dnh + pair_swap(dnh);
        iw01 = fast_rcp(rn > 0.0 ? rn : 1.0);
        iw23 = fast_rcp(dn > 0.0 ? dn : 1.0);
        iwv[0][gl] = iw01; iwv[1][gl] = iw23; // own entries, read back by the same lane in every search
    }

#ifdef JSIM_STAMPS
    long long gclk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gt0 = 0, gt1 = 0;
#endif
    int q = 0, iters = 0;
    int gpar = 0, glo = 0, ghi = -1;   // drops: which (c, s) buffer is next, and the rotations the previous drop left in the other one
    constexpr int max_iters = 50 * N + 100;
    unsigned abits = 0;                // which of this pair's candidate rows are in the working set
    double lam0 = 0.0, lam1 = 0.0;     // position lane (slot 0) / lane + 64 (slot 1): multiplier
    double rdg0 = 0.0, rdg1 = 0.0;     // .. 1 / R[k][k]
    int act0 = -1, act1 = -1;          // .. canonical row id
    for (;;) {
        LANE_FENCE4();
        SLOTMAP4();
        GSTAMP0();
        // ---- step 1: entering row = largest packed key over the four waves
        int p, la, lb, owner, obit;
        bool nega;
        double violp, dd;
        {
            int cid0 = -1, cid2 = -1;
            double ub0 = 0.0, lb1 = 0.0;
            {
                const double amax_ = Pv.amax, amin_ = Pv.amin, smax_ = Pv.smax, vmin_ = Pv.vmin;
                if (realrow) {
                    const int t = jrow >> 1;
                    const bool st_ = jrow & 1;
                    cid0 = st_ ? 6 * T + 2 * t : 4 * T + t;
                    ub0 = st_ ? smax_ : amax_; lb1 = st_ ? -smax_ : amin_;
                    if (st_ && t + 1 < T) cid2 = 2 * t;
                } else if (tsp > 0) {
                    cid0 = 2 * T - 2 + tsp;
                    ub0 = speed; lb1 = vmin_;
                }
            }
            const double iw01 = iwv[0][gl], iw23 = iwv[1][gl];
            const double dmx = Pv.dmax, thr23 = JSIM_VIOL_TOL * (1.0 + dmx);
            const double nxt = __shfl_down(val, 4);
            const double va = val - ub0, vb = lb1 - val;
            const bool up01 = va >= vb;
            const double v01 = up01 ? va : vb;
            // rhs of the row in terms of the step: u rows h = bound, speed rows h = bound - v0
            const double hoff = tsp >= 0 ? sv : 0.0;
            const double thr01 = JSIM_VIOL_TOL * (1.0 + fabs((up01 ? ub0 : lb1) - hoff));
            const int dc1 = tsp >= 0 ? T + 1 : ((jrow & 1) ? 1 : T); // canonical id of the lower-bound row = cid0 + dc1
            const bool ok01 = (cid0 >= 0) & !(abits & (up01 ? 1u : 2u)) & (v01 > thr01);
            const double k01 = ok01 ? jsim_key_pack(v01 * v01 * iw01, up01 ? cid0 : cid0 + dc1) : 0.0;
            const double e23 = nxt - val;
            const bool up23 = e23 >= 0.0;
            const double v23 = fabs(e23) - dmx;
            const bool ok23 = (cid2 >= 0) & !(abits & (up23 ? 4u : 8u)) & (v23 > thr23);
            const double k23 = ok23 ? jsim_key_pack(v23 * v23 * iw23, up23 ? cid2 : cid2 + 1) : 0.0;
            const bool t23 = k23 > k01;
            const double mykey = t23 ? k23 : k01;
            const double myviol = t23 ? v23 : v01;
            const double mydd = fast_rcp(t23 ? iw23 : iw01); // n'H^-1 n of the row (the dependence test only needs its scale)
            const int nxtslot = SLOT_OF_ROW(jrow + 2);       // the REAL slot of the steer-rate partner row
            const int mybit = t23 ? (up23 ? 2 : 3) : (up01 ? 0 : 1);
            const double win = wmax_dpp(mykey);
            if (win > 0.0) {
                if (mykey == win && half == 0) { // exactly one pair: the key carries the row id
                    xwd[wave][0] = win; xwd[wave][1] = myviol; xwd[wave][2] = mydd;
                    xwi[wave][0] = mybit >= 2 ? nxtslot : slot;
                    xwi[wave][1] = mybit >= 2 ? slot : -1;
                    xwi[wave][2] = slot;
                    xwi[wave][3] = mybit;
                }
            } else if (lane == 0) {
                xwd[wave][0] = 0.0;
            }
            BLOCK_SYNC();
            const double k0 = xwd[0][0], k1 = xwd[1][0], k2 = xwd[2][0], k3 = xwd[3][0];
            int ws = 0;
            double kw = k0;
            if (k1 > kw) { kw = k1; ws = 1; }
            if (k2 > kw) { kw = k2; ws = 2; }
            if (k3 > kw) { kw = k3; ws = 3; }
            ws = __builtin_amdgcn_readfirstlane(ws);
            violp = xwd[ws][1]; dd = xwd[ws][2];
            la = xwi[ws][0]; lb = xwi[ws][1]; owner = xwi[ws][2]; obit = xwi[ws][3];
            la = __builtin_amdgcn_readfirstlane(la); lb = __builtin_amdgcn_readfirstlane(lb);
            owner = __builtin_amdgcn_readfirstlane(owner); obit = __builtin_amdgcn_readfirstlane(obit);
            violp = uni(violp); dd = uni(dd);
            const double kwu = uni(kw);
            if (!(kwu > 0.0)) break; // no violated row in any wave: optimal
            p = 511 - (__double2loint(kwu) & 511);
            nega = !(obit & 1);
        }
#if defined(JSIM_STAMPS) || defined(JSIM_SPAN)
        if (Pv.dbg_max_gi >= 0 && q >= Pv.dbg_max_gi) break; // timing experiments only (diagnostic builds)
#endif
        GSTAMP(0);
        double lplus = 0.0;
        bool failed = false;

        for (;;) { // ---- step 2
            if (++iters > max_iters) { failed = true; break; }
            GSTAMP0();
            // d = Jhat' n+ : the owning pair(s) publish their half rows side by side (two lanes write at once)
            if (slot == la || slot == lb) {
                const int o2 = ((slot == lb) ? NP : 0) + cbase;
#pragma unroll
                for (int c = 0; c < NH; c += 2) *(double2 *)&drow12[o2 + c] = double2{Jr[c], Jr[c + 1]};
            }
            BLOCK_SYNC();
            // each wave needs every column: lane handles columns lane and lane + 64 (= working-set positions, too)
            double dA = 0.0, dB = 0.0;
            {
                dA = drow[lane];
                if (lb >= 0) dA -= drow2[lane];
                dA = nega ? -dA : dA;
            }
            if (lane + 64 < N) {
                dB = drow[lane + 64];
                if (lb >= 0) dB -= drow2[lane + 64];
                dB = nega ? -dB : dB;
            }
            double dq;
            {
                const int qi = q < N ? q : 0;
                dq = drow[qi];
                if (lb >= 0) dq -= drow2[qi];
                dq = nega ? -dq : dq;
                dq = uni(dq);
            }
            GSTAMP(1);
            double zpart = lane >= q ? dA * dA : 0.0;
            zpart = fma(lane + 64 >= q ? dB : 0.0, dB, zpart);
            const double zn = wsum_dpp(zpart);
            const double inrm = fast_rsqrt(zn > 1e-300 ? zn : 1e-300);
            const double nrm = zn * inrm;
            const double sg = dq >= 0.0 ? 1.0 : -1.0;
            {
                const double dzl = lane >= q ? dA : 0.0;
                dzv[wave][lane] = dzl;
                vzv[wave][lane] = lane == q ? dzl + sg * nrm : dzl;
            }
            if (lane + 64 < N) {
                const double dzl = lane + 64 >= q ? dB : 0.0;
                dzv[wave][lane + 64] = dzl;
                vzv[wave][lane + 64] = lane + 64 == q ? dzl + sg * nrm : dzl;
            }
            WAVE_SYNC();
            GSTAMP(2);
            // z = Jhat2 d2  and  y = Jhat2 v : each lane over its half row, the pair's two partial sums joined by DPP
            double z0 = 0.0, z1 = 0.0, y0 = 0.0, y1 = 0.0;
            {
                constexpr int ZC = 4, NCH = NH / ZC;
                const double *dzw = dzv[wave] + cbase, *vzw = vzv[wave] + cbase;
                double2 dzb[2][ZC / 2], vzb[2][ZC / 2];
#pragma unroll
                for (int c = 0; c < ZC; c += 2) { dzb[0][c / 2] = lds_ld2(&dzw[c]); vzb[0][c / 2] = lds_ld2(&vzw[c]); }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int h = ch * ZC;
                    if (ch + 1 < NCH) {
#pragma unroll
                        for (int c = h + ZC; c < h + 2 * ZC; c += 2) {
                            dzb[(ch + 1) & 1][(c - h - ZC) / 2] = lds_ld2(&dzw[c]);
                            vzb[(ch + 1) & 1][(c - h - ZC) / 2] = lds_ld2(&vzw[c]);
                        }
                    }
                    JSIM_STAGE();
#pragma unroll
                    for (int c = h; c < h + ZC; c += 2) {
                        const double2 dz2 = dzb[ch & 1][(c - h) / 2], vz2 = vzb[ch & 1][(c - h) / 2];
                        z0 = fma(Jr[c], dz2.x, z0); z1 = fma(Jr[c + 1], dz2.y, z1);
                        y0 = fma(Jr[c], vz2.x, y0); y1 = fma(Jr[c + 1], vz2.y, y1);
                    }
                    JSIM_PIN(z0); JSIM_PIN(z1); JSIM_PIN(y0); JSIM_PIN(y1);
                    JSIM_STAGE();
                }
            }
            const double zh = z0 + z1, yh = y0 + y1;
            const double z = zh + pair_swap(zh), y = yh + pair_swap(yh);
            GSTAMP(3);
            // r = R^-1 d1 : back substitution, position k in lane k & 63 / slot k >> 6 of this wave; rows of R scaled by
            // 1/R[k][k] at load; zeros below the diagonal / right of column q make all other steps no-ops
            double rl0 = dA * rdg0, rl1 = dB * rdg1;
            {
                const int r0i = lane;
                const int r1i = (lane + 64 < N) ? lane + 64 : 0;
#pragma unroll
                for (int blk = (N + 7) / 8 - 1; blk >= 0; --blk) {
                    if (q > 8 * blk) {
                        JSIM_STAGE(); // the block's loads stay inside its branch (hoisted above the nest, all ten blocks' rows were live at once)
                        const int jlo = 8 * blk, jhi = (8 * blk + 7 < N ? 8 * blk + 7 : N - 1);
                        if (jlo >= 64) { // the r_j come from slot 1; both slots are updated
                            double Ra[8], Rb[8];
#pragma unroll
                            for (int j = jlo; j <= jhi; ++j) { Ra[j - jlo] = Rm[r0i * LD + j] * rdg0; Rb[j - jlo] = Rm[r1i * LD + j] * rdg1; }
#pragma unroll
                            for (int j = jhi; j >= jlo; --j) {
                                const double rj = rdlane(rl1, j - 64);
                                rl1 = fma(-Rb[j - jlo], rj, rl1);
                                rl0 = fma(-Ra[j - jlo], rj, rl0);
                            }
                        } else {
                            double Ra[8];
#pragma unroll
                            for (int j = jlo; j <= jhi; ++j) Ra[j - jlo] = Rm[r0i * LD + j] * rdg0;
#pragma unroll
                            for (int j = jhi; j >= jlo; --j) rl0 = fma(-Ra[j - jlo], rdlane(rl0, j), rl0);
                        }
                        JSIM_STAGE();
                    }
                }
            }
            GSTAMP(4);
            // dual ratio test over both slots
            int l;
            double t1;
            {
                double bt = INFINITY;
                if (lane < q && rl0 > 0.0) bt = jsim_ratio_pack(lam0 * fast_rcp(rl0), lane);
                double bt1 = INFINITY;
                if (lane + 64 < q && rl1 > 0.0) bt1 = jsim_ratio_pack(lam1 * fast_rcp(rl1), lane + 64);
                bt = vmin_f64(bt, bt1);
                const double wn = wmin_dpp(bt);
                l = __double2loint(wn) & 127;
                t1 = isinf(wn) ? wn : jsim_ratio_trunc(wn);
            }
            const bool dependent = !(zn > JSIM_DEP_TOL * dd);
            double t2 = dependent ? INFINITY : violp * (inrm * inrm);
            if (t2 < 0.0) t2 = 0.0;
            if (isinf(t1) && isinf(t2)) { failed = true; break; }
            const bool full = (t2 <= t1);
            const double tstep = full ? t2 : t1;
            if (!dependent) { val = fma(tstep, z, val); violp = fma(-tstep, zn, violp); }
            if (lane < q) {
                const double lk = fma(-tstep, rl0, lam0);
                lam0 = lk < 0.0 ? 0.0 : lk;
            }
            if (lane + 64 < q) {
                const double lk = fma(-tstep, rl1, lam1);
                lam1 = lk < 0.0 ? 0.0 : lk;
            }
            lplus += tstep;

            GSTAMP(5);
            if (full) {
                // add p: one Householder reflection on d2; new R column [d1; rho]
                const double rho = -sg * nrm;
                const double beta = inrm * fast_rcp(nrm + fabs(dq));
                const double w = beta * y;
                {
                    constexpr int ZC = 4, NCH = NH / ZC;
                    const double *vzw = vzv[wave] + cbase;
                    double2 vzb[2][ZC / 2];
#pragma unroll
                    for (int c = 0; c < ZC; c += 2) vzb[0][c / 2] = lds_ld2(&vzw[c]);
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        const int h = ch * ZC;
                        if (ch + 1 < NCH) {
#pragma unroll
                            for (int c = h + ZC; c < h + 2 * ZC; c += 2) vzb[(ch + 1) & 1][(c - h - ZC) / 2] = lds_ld2(&vzw[c]);
                        }
                        JSIM_STAGE();
#pragma unroll
                        for (int c = h; c < h + ZC; c += 2) {
                            Jr[c] = fma(-w, vzb[ch & 1][(c - h) / 2].x, Jr[c]);
                            Jr[c + 1] = fma(-w, vzb[ch & 1][(c - h) / 2].y, Jr[c + 1]);
                        }
                        JSIM_STAGE();
                    }
                }
                if (wave == 0) {
                    if (lane < q) Rm[lane * LD + q] = dA;
                    if (lane + 64 < q) Rm[(lane + 64) * LD + q] = dB;
                    if (lane == 0) rdv[q] = rho;
                }
                if (q < 64) { if (lane == q) { rdg0 = -sg * inrm; act0 = p; lam0 = lplus; } }
                else { if (lane == q - 64) { rdg1 = -sg * inrm; act1 = p; lam1 = lplus; } }
                if (slot == owner) abits |= (1u << obit);
                JSIM_PIN_WS(lam0, rdg0, act0); JSIM_PIN_WS(lam1, rdg1, act1); JSIM_PIN(abits);
                GSTAMP(6);
                ++q;
            }
            jsim_join_row(Jr); // the drop reads the row as it stands HERE: one register set for J (jsim_mpc.hip; DESIGN.md section 5, fact 7)
            if (full) break; // the barrier of the next entering-row search orders the writes to R
            // partial step: drop working-set position l (Givens sweep on R in LDS by all threads, same rotations on J)
            {
                int pdrop;
                if (l >= 64) pdrop = __builtin_amdgcn_readlane(act1, l - 64);
                else pdrop = __builtin_amdgcn_readlane(act0, l);
                // Givens sweep on R: rotation j turns rows (j, j + 1) so that the sub-diagonal entry left by the departing column
                // vanishes.  ONE wave does it, lane = column, with row j + 1 of the running sweep carried in registers: per
                // rotation one fresh row from LDS (its address does not depend on the chain), the pivot by v_readlane, no barrier.
                // Every rotated row is written straight to where it ends up -- one column to the left, the dropped column closes.
                // Meanwhile the other waves close the rows above l up (they are not rotated, only shifted).
                double *const gcur = gsvb + gpar * GSZ;
                BLOCK_SYNC(); // every wave is through its triangular solve: R may change
                if (wave == 0) {
                    int dlane = lane; // the sweep's LDS addresses are computed here, not hoisted out of the iteration loop and spilled
                    asm volatile("" : "+v"(dlane));
                    const int colB = dlane + 64;
                    const bool vB = colB < N;
                    double x1A = Rm[l * LD + dlane], x1B = vB ? Rm[l * LD + colB] : 0.0; // row l as it stands
                    // the next row and the next diagonal entry are fetched one rotation ahead: their latency is off the chain
                    double x2A = (l + 1 < q) ? Rm[(l + 1) * LD + dlane] : 0.0, x2B = (vB && l + 1 < q) ? Rm[(l + 1) * LD + colB] : 0.0;
                    double b = rdv[l + 1 < N ? l + 1 : 0];
                    for (int j = l; j + 1 < q; ++j) {
                        const int jn = (j + 2 < q) ? j + 2 : j + 1;
                        const double x3A = Rm[jn * LD + dlane], x3B = vB ? Rm[jn * LD + colB] : 0.0;
                        const double bn = rdv[jn];
                        const double a = (j + 1 < 64) ? rdlane(x1A, (j + 1) & 63) : rdlane(x1B, (j + 1) & 63);
                        // (c, s) = (a, b) / hypot(a, b) through the reciprocal root (<= 1 ulp, like the other scalings of the loop):
                        // an IEEE square root and two IEEE divisions per rotation were most of a drop's time
                        const double h2 = fma(a, a, b * b);
                        const double ih = fast_rsqrt(h2 > 1e-300 ? h2 : 1e-300);
                        const double hh = h2 * ih;
                        double c = 1.0, s = 0.0;
                        if (hh > 0.0) { c = a * ih; s = b * ih; }
                        const double n1A = fma(c, x1A, s * x2A), n1B = fma(c, x1B, s * x2B);
                        if (dlane >= j + 2 && dlane < q) Rm[j * LD + dlane - 1] = n1A;
                        if (vB && colB >= j + 2 && colB < q) Rm[j * LD + colB - 1] = n1B;
                        x1A = fma(-s, x1A, c * x2A); x1B = fma(-s, x1B, c * x2B); // row j + 1 of the sweep so far
                        if (lane == 0) { *(double2 *)&gcur[2 * j] = double2{c, s}; rdv[j] = hh; Rm[j * LD + q - 1] = 0.0; }
                        x2A = x3A; x2B = x3B; b = bn;
                    }
                    if (lane == 0) Rm[(q - 1) * LD + q - 1] = 0.0;
                } else {
                    for (int k = wave - 1; k < l; k += 3) { // rows above l: columns l + 1 .. q - 1 move one to the left, column q - 1 empties
                        const int cA = l + lane, cB = l + lane + 64;
                        const double vA = (cA + 1 < q) ? Rm[k * LD + cA + 1] : 0.0;
                        const double vB2 = (cB + 1 < q) ? Rm[k * LD + cB + 1] : 0.0;
                        if (cA < q) Rm[k * LD + cA] = vA;
                        if (cB < q) Rm[k * LD + cB] = vB2;
                    }
                    if (wave == 1) { // the previous drop's rotations go back to identities: nobody reads that buffer any more
                        double *const gold = gsvb + (gpar ^ 1) * GSZ;
                        for (int e = glo + lane; e <= ghi; e += 64) { gold[2 * e] = 1.0; gold[2 * e + 1] = 0.0; }
                    }
                }
                BLOCK_SYNC(); // (c, s) of every rotation, the new diagonal and the new rows are in LDS
                // The same rotations on J's columns, along every row: rotation j turns columns (j, j + 1).  Low half first (rotations
                // 0 .. NH-2, the high lanes read identities), then the rotation that straddles the halves (columns NH-1 | NH, exchanged
                // by DPP), then the high half (rotations NH .. N-2, the low lanes read identities).  Only rotations l .. q-2 are not
                // identities: blocks of eight that lie outside are skipped (uniform branch), inside a block identity = exact no-op.
                {
                    const double *const csLow = half ? gcur + 2 * N : gcur;           // (c, s) of rotation c for this lane, low stage
                    const double *const csHigh = half ? gcur + 2 * NH : gcur + 2 * N; // .. of rotation NH + c, high stage
                    const int jl = l, jh = q - 2;
#pragma unroll
                    for (int st = 0; st < 2; ++st) {
                        const double *const csb_ = st ? csHigh : csLow;
#pragma unroll
                        for (int h = 0; h + 1 < NH; h += 8) {
                            const int g0 = st * NH + h, g1 = st * NH + (h + 7 < NH - 2 ? h + 7 : NH - 2);
                            if (g0 <= jh && g1 >= jl) {
                                double2 csb[8];
#pragma unroll
                                for (int c = h; c < h + 8 && c + 1 < NH; ++c) csb[c - h] = lds_ld2(&csb_[2 * c]);
                                JSIM_STAGE();
#pragma unroll
                                for (int c = h; c < h + 8 && c + 1 < NH; ++c) {
                                    const double2 cs2 = csb[c - h];
                                    const double x1 = Jr[c], x2 = Jr[c + 1];
                                    Jr[c] = fma(cs2.x, x1, cs2.y * x2);
                                    Jr[c + 1] = fma(-cs2.y, x1, cs2.x * x2);
                                    JSIM_PIN(Jr[c]);
                                }
                                JSIM_PIN(Jr[(h + 8 < NH ? h + 8 : NH - 1)]);
                                JSIM_STAGE();
                            }
                        }
                        if (st == 0 && NH - 1 >= jl && NH - 1 <= jh) { // rotation NH - 1: column NH - 1 (low lane's last) with column NH (high lane's first)
                            const double2 cs2 = lds_ld2(&gcur[2 * (NH - 1)]);
                            const double pl = pair_swap(Jr[NH - 1]), pf = pair_swap(Jr[0]);
                            const double x1 = half ? pl : Jr[NH - 1];  // column NH - 1
                            const double x2 = half ? Jr[0] : pf;       // column NH
                            const double n1 = fma(cs2.x, x1, cs2.y * x2), n2 = fma(-cs2.y, x1, cs2.x * x2);
                            if (half) Jr[0] = n2; else Jr[NH - 1] = n1;
                        }
                    }
                }
                // positions above l move down by one (per-wave copies through this wave's scratch)
                lamx[wave][lane] = lam0; actx[wave][lane] = act0;
                if (lane + 64 < N) { lamx[wave][lane + 64] = lam1; actx[wave][lane + 64] = act1; }
                WAVE_SYNC();
                if (lane >= l && lane + 1 < q) { lam0 = lamx[wave][lane + 1]; act0 = actx[wave][lane + 1]; rdg0 = fast_rcp(rdv[lane]); }
                if (lane == q - 1) { rdg0 = 0.0; lam0 = 0.0; act0 = -1; }
                if (lane + 64 >= l && lane + 65 < q) { lam1 = lamx[wave][lane + 65]; act1 = actx[wave][lane + 65]; rdg1 = fast_rcp(rdv[lane + 64]); }
                if (lane + 64 == q - 1) { rdg1 = 0.0; lam1 = 0.0; act1 = -1; }
                JSIM_PIN_WS(lam0, rdg0, act0); JSIM_PIN_WS(lam1, rdg1, act1);
                glo = l; ghi = q - 2; gpar ^= 1; // this drop's rotations are reset by the next drop, behind its first barrier
                --q;
                {
                    int drow_, dbit;
                    if (pdrop < 2 * T - 2) { drow_ = 2 * (pdrop >> 1) + 1; dbit = (pdrop & 1) ? 3 : 2; }
                    else if (pdrop < 3 * T - 1) { drow_ = -(pdrop - (2 * T - 2)) - 1; dbit = 0; }
                    else if (pdrop < 4 * T) { drow_ = -(pdrop - (3 * T - 1)) - 1; dbit = 1; }
                    else if (pdrop < 5 * T) { drow_ = 2 * (pdrop - 4 * T); dbit = 0; }
                    else if (pdrop < 6 * T) { drow_ = 2 * (pdrop - 5 * T); dbit = 1; }
                    else { drow_ = 2 * ((pdrop - 6 * T) >> 1) + 1; dbit = ((pdrop - 6 * T) & 1) ? 1 : 0; }
                    const int dslot = drow_ >= 0 ? SLOT_OF_ROW(drow_) : S2 + (-drow_ - 1); // negative: speed row t = -drow_ - 1
                    if (slot == dslot) abits &= ~(1u << dbit);
                    JSIM_PIN(abits);
                }
                GSTAMP(7); // (no barrier: what the next iteration reads of R, rdv and the scratch is ordered by the barrier of its search)
            }
        }
        if (failed) { status = JSIM_INFEASIBLE; break; }
    }

#ifdef JSIM_STAMPS
    if (Pv.dbg_clk && gl == 0)
        for (int i_ = 0; i_ < 8; ++i_) Pv.dbg_clk[(size_t)Pv.B * 16 + (size_t)ego * 8 + i_] = gclk[i_];
#endif
    LANE_FENCE4();
    STAMP2(10);
    // ------------------------------------------------------------------ S5: outputs
    if (status != JSIM_OK) {
        if (wave == 0 && tl) { gp(Pv.oa)[(size_t)ego * T + lane] = 0.0; gp(Pv.od)[(size_t)ego * T + lane] = 0.0; }
        WS_SET(0.0, 0.0); s0 = tind;
        if (Pv.amask && gl < MW) gp(Pv.amask)[(size_t)ego * MW + gl] = 0u;
        if (gl == 0) {
            gp(Pv.status)[ego] = status;
            gp(Pv.target_ind)[ego] = tind;
            if (Pv.n_iter) gp(Pv.n_iter)[ego] = it_base + iters;
        }
        it_sum += (unsigned)iters;
        break;
    }
    if (gl < MW) maskw[gl] = 0u;
    {
        const int slot_ = gl >> 1;
        if (!(gl & 1)) { // one lane per pair publishes the pair's value: u_row, or v_t behind them
            int jr_ = -1;
            if (slot_ < G1) jr_ = slot_;
            else if (slot_ > G1 && slot_ < G2 + 1) jr_ = slot_ - 1;
            else if (slot_ >= 64 && slot_ < S2) jr_ = slot_ - 3;
            if (jr_ >= 0) uvec[jr_] = val;
            if (slot_ >= S2 && slot_ < SW) uvec[N + slot_ - S2] = val;
        }
    }
    if (Pv.dbg_lam)
        for (int e = gl; e < 8 * T; e += 256) Pv.dbg_lam[(size_t)ego * 8 * T + e] = 0.0;
    BLOCK_SYNC();
    {
        const double thr = JSIM_ACT_TOL * fmax(1.0, gmax);
        if (wave == 0) {
            if (lane < q) {
                if (lam0 > thr) atomicOr(&maskw[act0 >> 5], 1u << (act0 & 31));
                if (Pv.dbg_lam) Pv.dbg_lam[(size_t)ego * 8 * T + act0] = lam0;
            }
            if (lane + 64 < q) {
                if (lam1 > thr) atomicOr(&maskw[act1 >> 5], 1u << (act1 & 31));
                if (Pv.dbg_lam) Pv.dbg_lam[(size_t)ego * 8 * T + act1] = lam1;
            }
        }
        BLOCK_SYNC();
        if (Pv.amask && gl < MW) gp(Pv.amask)[(size_t)ego * MW + gl] = maskw[gl];
    }
    {
        const double al = park[0][lane], be = park[1][lane], alp = park[2][lane], bep = park[3][lane];
        const double ccx = park[4][lane], ccy = park[5][lane], kt = park[6][lane];
        double a = 0.0, dl_ = 0.0;
        if (tl) { a = uvec[2 * lane]; dl_ = uvec[2 * lane + 1]; }
        const double vt = lane <= T ? uvec[N + lane] : sv;
        const double yt = syaw + wexscan_dpp(kt * dl_, lane);
        const double xt = sx + wexscan_dpp(fma(al, vt, fma(be, yt, ccx)), lane);
        const double yy = sy + wexscan_dpp(fma(alp, vt, fma(bep, yt, ccy)), lane);
        if (wave == 0 && tl) { gp(Pv.oa)[(size_t)ego * T + lane] = a; gp(Pv.od)[(size_t)ego * T + lane] = dl_; }
        double tn = 0.0; // tan of the new warm start's clamped steer: the next tick's S2, and the plant step below (entry 0)
        if (advance || tk + 1 < n_ticks) WS_TAN(dl_, tn);
        p_tn = rdlane(tn, 0);
        WS_SET(a, tn); s0 = tind;
        a0n = uvec[0]; d0n = uvec[1];
        if (wave == 0 && lane <= T) {
            const size_t o = (size_t)ego * (T + 1) + lane;
            if (Pv.ox) gp(Pv.ox)[o] = xt;
            if (Pv.oy) gp(Pv.oy)[o] = yy;
            if (Pv.ov) gp(Pv.ov)[o] = vt;
            if (Pv.oyaw) gp(Pv.oyaw)[o] = yt;
        }
    }
    if (gl == 0) {
        gp(Pv.status)[ego] = JSIM_OK;
        gp(Pv.target_ind)[ego] = tind;
        if (Pv.n_iter) gp(Pv.n_iter)[ego] = it_base + iters;
    }
    it_sum += (unsigned)iters;
    STAMP2(11);
    } while (0);

    // ---------------------------------------------------------------- rest of the loop body (jsim_loop_advance), all waves alike
    if (advance) {
        double di = di_prev, ai;
        if (status == JSIM_OK) { di = d0n; ai = a0n; }
        else ai = Pv.amin; // MAX_DECEL
        di_prev = di;
        ai_last = ai;
        if (Kv.hist && gl == 0) {
            const int k = hist_base + tk;
            if (k < Kv.hist_cap) { gp(Kv.hist)[((size_t)k * Pv.B + ego) * 2] = di; gp(Kv.hist)[((size_t)k * Pv.B + ego) * 2 + 1] = ai; }
        }
        // the recorder's xref deviation: the solve's ox[0], oy[0] is the tick-start pose (sx, sy), target_ind is s0
        if (Kv.rec && gl == 0 && hist_base + tk < Kv.rec_cap) {
            const jsim_d2v rq = ((JSIM_GAS const jsim_d2v *)Pv.pxy)[off + s0];
            jsim_rec_store_dev(gp(Kv.rec), hist_base + tk, Pv.B, ego,
                               status == JSIM_OK ? jsim_xref_deviation(double2{rq.x, rq.y}, gp(Pv.pyaw)[off + s0], sx, sy)
                                                 : __builtin_nan(""));
        }
        double dc = (Pv.smax < di) ? Pv.smax : di;
        dc = (-Pv.smax > dc) ? -Pv.smax : dc;
        double cy_ = p_cs, sy_ = p_sn; // S2's own (lane 0's bth is syaw itself)
        if (!p_sc) { cy_ = cos(syaw); sy_ = sin(syaw); } // the tick left before S2 (no path, nearest-index anomaly)
        double tn_;
        if (status == JSIM_OK) tn_ = p_tn;  // di is this solve's delta_0: S5 evaluated tan(dc)
        else tn_ = tan(dc);                // a failed tick steers with the previous di
        const double xd = sv * cy_, yd = sv * sy_, thd = (sv / Pv.L) * tn_;
        sx += xd * dt; sy += yd * dt; syaw += thd * dt;
        sv += ai * dt;
        sv = (Pv.vmax_plant < sv) ? Pv.vmax_plant : sv;
        sv = (Pv.vmin > sv) ? Pv.vmin : sv;
        bool isgoal = hypot(sx - goal_xy.x, sy - goal_xy.y) <= Kv.goal_dis;
        long long df = s0 - M;
        if ((df < 0 ? -df : df) >= 5) isgoal = false;
        // (uniform, but decided by vector compares: without the broadcast `age` and everything reset below live in vector registers)
        const bool goal = isgoal && fabs(sv) <= Kv.stop_speed, aged = age + 1 >= Kv.max_age;
        const bool done = uni((int)(goal || aged)) != 0;
        if (Kv.rec && gl == 0) { // the History record: the new state ahead of the respawn
            const int k = hist_base + tk;
            if (k < Kv.rec_cap)
                jsim_rec_store(gp(Kv.rec), gp(Kv.rec_flags), k, Pv.B, ego, sx, sy, syaw, sv, di, ai,
                               (status == JSIM_OK ? 0 : JSIM_REC_FAILED) | (goal ? JSIM_REC_GOAL : 0) | (aged ? JSIM_REC_AGE : 0));
        }
        if (done) {
            sx = gp(Kv.x0_spawn)[4 * ego]; sy = gp(Kv.x0_spawn)[4 * ego + 1]; sv = gp(Kv.x0_spawn)[4 * ego + 2]; syaw = gp(Kv.x0_spawn)[4 * ego + 3];
            s0 = gp(Kv.target_spawn)[ego];
            WS_SET(0.0, 0.0); di_prev = 0.0; ai_last = 0.0; age = 0;
            if (PRE) { pre_idx = 0; pre_prev = -1; }
            if (wave == 0 && tl) { gp(Pv.oa)[(size_t)ego * T + lane] = 0.0; gp(Pv.od)[(size_t)ego * T + lane] = 0.0; }
            if (gl == 0) {
                gp(Pv.target_ind)[ego] = s0;
                if (Kv.n_respawn) atomicAdd(Kv.n_respawn, 1ull);
            }
        } else {
            age += 1;
        }
    }
    BLOCK_SYNC(); // LDS scratch is reused by the next tick
    } // tick loop
    if (gl == 0) { // one read-modify-write per launch (see mpc_step_reg.inc)
        if (Kv.work) gp(Kv.work)[ego] += it_sum;
        if (Kv.iters) gp(Kv.iters)[ego] += (unsigned long long)it_sum;
    }
    if (advance && gl == 0) {
        gp(Kv.x0w)[4 * ego] = sx; gp(Kv.x0w)[4 * ego + 1] = sy; gp(Kv.x0w)[4 * ego + 2] = sv; gp(Kv.x0w)[4 * ego + 3] = syaw;
        gp(Kv.di_ai)[2 * ego] = di_prev;
        gp(Kv.di_ai)[2 * ego + 1] = ai_last;
        gp(Kv.age)[ego] = age;
    }
    if (PRE && gl == 0) {
        Q.traj_idx[ego] = pre_idx;
        Q.prev_len[ego] = pre_prev;
        if (Q.speed_cutoff) Q.cut_io[ego] = pre_cut; else Q.path_len_out[ego] = (int)M;
        Q.col_flag[ego] = pre_col;
        Q.pre_status[ego] = pre_st;
    }
#undef LANE_FENCE4
#undef WS_SET
#undef WS_TAN
#undef tl
#undef SLOT_OF_ROW
#undef SLOTMAP4
}
