// mpc_step_reg.inc -- register-resident fast path of the MPC step, one wavefront per ego (2T + 1 <= 64 lanes).
// (included by jsim_mpc.hip; same stages, same decisions, same tolerances as mpc_step_kernel)
//
// Why a second kernel: at the benchmark shape (256 egos on 256 CUs) every CU runs ONE wave, so nothing
// hides LDS latency; the LDS-resident kernel spends ~140 cycles per inner-loop step waiting on ds_read
// (profiles/r01_v1_lds_phase_stamps_T20.txt).  Here the factors never leave the register file:
//   * lane i < N = 2T   owns row i of J (N doubles, compile-time indexed after full unrolling);
//   * lane N + t        (3T + 1 <= 63 lanes, T <= 20) owns the "speed row" t:  dt * sum_{s<t} J[2s][:].  Every constraint
//                       normal is then +-(one row) or a difference of two rows of the augmented J, and v_t is updated by the
//                       same z = J2 d2 product that updates u.  Longer horizons (T <= 31) keep the speed rows VIRTUAL
//                       (see VS below): v_t by a prefix scan over the acceleration lanes, the row formed on demand;
//   * the entering row is published through LDS and read back as a broadcast vector (bursts of ds_read_b128 behind
//     scheduling barriers); reductions, arg-max / arg-min use DPP (quad_perm / row_mirror) + v_readlane, not ds_bpermute;
//   * R (strict upper triangle) lives in LDS, the back substitution runs on broadcasts of the running solution: the 64-bit DPP
//     row broadcast inside the first 16-lane row (columns below 16), v_readlane from column 16 on;
//   * PRE instantiations run the scenario loop's glue (loop_pre_tick.inc) inside the tick loop.

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) // all source lanes valid for the controls used with this
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }

// Two back-substitution steps on the 64-bit row broadcast (DESIGN.md section 5, fact 8).  One step is
//     v += (lane J of the caller's 16-lane row: v) * m,   m = R[k][J] * -(1 / R[k][k])  in lane k,
// ONE v_fmac_f64 with a DPP multiplicand (gfx90a and later; row_newbcast is the only DPP control 64-bit operations have) where the
// v_readlane form needs two v_readlane, an s_nop and the FMA.  A DPP source must not be read in the two issue slots after the vector
// instruction that wrote it, and the compiler's hazard pass does not look inside an asm statement, so the statement carries its own
// padding: both steps' products stand in front of the first step (two vector instructions behind whatever wrote v last), s_nop 1 in
// front of the second -- five slots for two steps.  r_hi, r_lo: R[k][J], R[k][J - 1].  Nothing of
// this may be reordered or sunk into a lane-masked region (a DPP read from a lane that EXEC masks off returns 0, fact 4): volatile.
template <int J>
__device__ __forceinline__ void bs_step2(double &v, double r_hi, double r_lo, double rdiag)
{
    static_assert(J >= 1 && J < 16, "row_newbcast selects a lane of the 16-lane row");
    double m_hi, m_lo; // (outputs of their own: tied to r_hi / r_lo, halves of one 16-byte read, each pair costs a register copy)
    asm volatile("v_mul_f64 %1, %3, -%5\n\t"
                 "v_mul_f64 %2, %4, -%5\n\t"
                 "v_fmac_f64_dpp %0, %0, %1 row_newbcast:%6 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_fmac_f64_dpp %0, %0, %2 row_newbcast:%7 row_mask:0xf bank_mask:0xf"
                 : "+v"(v), "=&v"(m_hi), "=&v"(m_lo) : "v"(r_hi), "v"(r_lo), "v"(rdiag), "n"(J), "n"(J - 1));
}
template <int LO, int J>
__device__ __forceinline__ void bs_steps(double &v, const double *r, double rdiag) // steps LO + J, LO + J - 1, .. LO on r[J] .. r[0] (J odd)
{
    bs_step2<LO + J>(v, r[J], r[J - 1], rdiag);
    if constexpr (J > 1) bs_steps<LO, J - 2>(v, r, rdiag);
}

#define DPP_QP_1032 0xB1 /* quad_perm [1,0,3,2] */
#define DPP_QP_2301 0x4E /* quad_perm [2,3,0,1] */
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_ROW_MIRROR 0x140
#define DPP_ROW_SHR(n) (0x110 + (n))

// wave sum, result uniform
__device__ __forceinline__ double wsum_dpp(double v)
{
    v += dpp_f64<DPP_QP_1032>(v);
    v += dpp_f64<DPP_QP_2301>(v);
    v += dpp_f64<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_f64<DPP_ROW_MIRROR>(v);
    return (rdlane(v, 0) + rdlane(v, 16)) + (rdlane(v, 32) + rdlane(v, 48));
}
// v_max_f64 / v_min_f64 without the canonicalising self-max the compiler puts in front of fmax / fmin (no NaN operands here)
__device__ __forceinline__ double vmax_f64(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin_f64(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double wmax_dpp(double v)
{
    v = vmax_f64(v, dpp_f64<DPP_QP_1032>(v));
    v = vmax_f64(v, dpp_f64<DPP_QP_2301>(v));
    v = vmax_f64(v, dpp_f64<DPP_ROW_HALF_MIRROR>(v));
    v = vmax_f64(v, dpp_f64<DPP_ROW_MIRROR>(v));
    return fmax(fmax(rdlane(v, 0), rdlane(v, 16)), fmax(rdlane(v, 32), rdlane(v, 48)));
}
__device__ __forceinline__ double wmin_dpp(double v)
{
    v = vmin_f64(v, dpp_f64<DPP_QP_1032>(v));
    v = vmin_f64(v, dpp_f64<DPP_QP_2301>(v));
    v = vmin_f64(v, dpp_f64<DPP_ROW_HALF_MIRROR>(v));
    v = vmin_f64(v, dpp_f64<DPP_ROW_MIRROR>(v));
    return fmin(fmin(rdlane(v, 0), rdlane(v, 16)), fmin(rdlane(v, 32), rdlane(v, 48)));
}
#define ARG_STEP(CTRL, BETTER)                                                   \
    {                                                                            \
        const double ov = dpp_f64<CTRL>(v);                                      \
        const int oi = dpp_i32<CTRL>(id);                                        \
        const bool take = (ov BETTER v) || (ov == v && oi < id);                 \
        v = take ? ov : v;                                                       \
        id = take ? oi : id;                                                     \
    }
#define ARG_ROWS(BETTER)                                                         \
    {                                                                            \
        double bv_ = rdlane(v, 0);                                               \
        int bi_ = __builtin_amdgcn_readlane(id, 0);                              \
        _Pragma("unroll") for (int r_ = 16; r_ < 64; r_ += 16)                   \
        {                                                                        \
            const double ov = rdlane(v, r_);                                     \
            const int oi = __builtin_amdgcn_readlane(id, r_);                    \
            const bool take = (ov BETTER bv_) || (ov == bv_ && oi < bi_);        \
            bv_ = take ? ov : bv_;                                               \
            bi_ = take ? oi : bi_;                                               \
        }                                                                        \
        v = bv_;                                                                 \
        id = bi_;                                                                \
    }
// arg-max on (v, id): larger v, ties -> smaller id; result uniform
__device__ __forceinline__ void wargmax_dpp(double &v, int &id)
{
    ARG_STEP(DPP_QP_1032, >) ARG_STEP(DPP_QP_2301, >) ARG_STEP(DPP_ROW_HALF_MIRROR, >) ARG_STEP(DPP_ROW_MIRROR, >)
    ARG_ROWS(>)
}
// arg-min on (v, id): smaller v, ties -> smaller id; result uniform
__device__ __forceinline__ void wargmin_dpp(double &v, int &id)
{
    ARG_STEP(DPP_QP_1032, <) ARG_STEP(DPP_QP_2301, <) ARG_STEP(DPP_ROW_HALF_MIRROR, <) ARG_STEP(DPP_ROW_MIRROR, <)
    ARG_ROWS(<)
}
#undef ARG_STEP
#undef ARG_ROWS
// the same answer for v >= 0 (no NaN) by another route: the wave minimum of v alone (3 instructions per DPP step instead of 12),
// then the lane that holds it -- by ballot; only when several lanes tie, the smallest id among them
__device__ __forceinline__ int wmin_i32_dpp(int v)
{
    int o;
    o = dpp_i32<DPP_QP_1032>(v); v = o < v ? o : v;
    o = dpp_i32<DPP_QP_2301>(v); v = o < v ? o : v;
    o = dpp_i32<DPP_ROW_HALF_MIRROR>(v); v = o < v ? o : v;
    o = dpp_i32<DPP_ROW_MIRROR>(v); v = o < v ? o : v;
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}
__device__ __forceinline__ void wargmin_fast(double &v, int &id)
{
    const double m = wmin_dpp(v);
    const unsigned long long eq = __ballot(v == m);
    int best;
    if (__popcll(eq) == 1) best = __builtin_amdgcn_readlane(id, (int)__builtin_ctzll(eq));
    else best = wmin_i32_dpp(v == m ? id : 0x7fffffff);
    v = m;
    id = best;
}

// exclusive prefix sum over the 64 lanes (Hillis-Steele inside each 16-lane row with row_shr, then row offsets)
__device__ __forceinline__ double wexscan_dpp(double v, int lane)
{
    double x = v;
    x += dpp_f64<DPP_ROW_SHR(1)>(x); // bound_ctrl: lanes without a source inside the row read 0
    x += dpp_f64<DPP_ROW_SHR(2)>(x);
    x += dpp_f64<DPP_ROW_SHR(4)>(x);
    x += dpp_f64<DPP_ROW_SHR(8)>(x);
    const double t0 = rdlane(x, 15), t1 = rdlane(x, 31), t2 = rdlane(x, 47);
    const int row = lane >> 4;
    double offs = 0.0;
    if (row >= 1) offs = t0;
    if (row >= 2) offs += t1;
    if (row >= 3) offs += t2;
    return (x + offs) - v;
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ double wincscan_dpp(double v, int lane)
{
    double x = v;
    x += dpp_f64<DPP_ROW_SHR(1)>(x);
    x += dpp_f64<DPP_ROW_SHR(2)>(x);
    x += dpp_f64<DPP_ROW_SHR(4)>(x);
    x += dpp_f64<DPP_ROW_SHR(8)>(x);
    const double t0 = rdlane(x, 15), t1 = rdlane(x, 31), t2 = rdlane(x, 47);
    const int row = lane >> 4;
    double offs = 0.0;
    if (row >= 1) offs = t0;
    if (row >= 2) offs += t1;
    if (row >= 3) offs += t2;
    return x + offs;
}

// reciprocal / reciprocal square root: hardware estimate + two Newton steps (<= 1 ulp for the normal, well-scaled
// operands of the active-set loop; S1-S3 keep IEEE division and sqrt because their outputs feed integers)
__device__ __forceinline__ double fast_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
__device__ __forceinline__ double fast_rsqrt(double x)
{
    double r = __builtin_amdgcn_rsq(x);
    double h = 0.5 * r, xr = x * r;   // Newton on r = x^-1/2:  r <- r + r * (1/2 - (x r)(r/2))
    double e = fma(-xr, h, 0.5);
    r = fma(r, e, r);
    h = 0.5 * r; xr = x * r;
    e = fma(-xr, h, 0.5);
    return fma(r, e, r);
}

__host__ __device__ static inline size_t jsim_reg_lds_doubles(int T)
{
    const size_t N = 2 * (size_t)T, NR = 3 * (size_t)T + 1;
    //      Hm/Lm/Rm      tq                       gsv     drow drow2 dz  vz       uvec          mask
    return N * (N + 1) + TQ_COUNT * ((size_t)T + 2) + 2 * N + 5 * (N + 2) + (NR + 4) + ((8 * (size_t)T + 31) / 32 + 1) / 2 + 2;
}

// Closed loop on the device (the per-vehicle loop of main/scenarios/mpc_intersection.py:99-163 for one ego per
// wavefront): n_ticks consecutive ticks of { MPC step ; (di, ai) selection ; plant step ; history ; goal test /
// respawn }.  Egos never wait for each other, the controller state (pose, remembered path index, warm start,
// previous steer) stays in registers between ticks.  n_ticks = 1 with advance = 0 is the plain MPC.step.
struct TickP {
    int n_ticks, advance, max_age, hist_cap, rec_cap;
    double max_decel, goal_dis, stop_speed;
    double *x0w;
    double *di_ai;
    const double *x0_spawn;
    const long long *target_spawn;
    int *age;
    double *hist;
    double *rec;   // the History recorder (jsim_loop_set_recorder): [rec_cap][B][JSIM_REC_FIELDS], flags [rec_cap][B]; NULL: none
    int *rec_flags;
    const int *tick;
    unsigned long long *n_respawn;
    // launch order (jsim_mpc.hip, launch_order_kernel): workgroup b solves ego order[b] -- the egos that needed the most
    // active-set iterations in the previous launch are dispatched first, so the launch does not end on a late-started
    // straggler -- and every ego adds the iterations it needed to work[ego] for the next launch.  Both NULL: identity.
    const int *order;
    unsigned *work;
    // per-ego running total of active-set iterations over every launch since jsim_mpc_iter_totals(..., reset) (NULL: not kept):
    // what bench.py derives mean iterations, flops and the straggler statistic of the TIMED launches from
    unsigned long long *iters;
};

// Forces a value to be computed where the statement stands: pure arithmetic is otherwise sunk towards its first use, and
// whatever it consumes (broadcast vectors just read from LDS) stays live until then -- in AGPRs or scratch.
#define JSIM_PIN(x) asm volatile("" : "+v"(x))
// The working set's lane-distributed state (position k lives in lane k: multiplier, 1 / R[k][k], canonical row id), pinned after a
// masked write to it so that the write stays where it stands.
#define JSIM_PIN_WS(lam_, rd_, id_) asm volatile("" : "+v"(lam_), "+v"(rd_), "+v"(id_))
// Both halves of a 16-byte broadcast read count as used from here on (placed at the pair's first use, where its wait stands anyway):
// a pair of which one half is dead is otherwise read as 8 bytes, and its neighbours lose their 16-byte alignment with it.
#define JSIM_PIN_PAIR(p_) asm volatile("" : "+v"((p_).x), "+v"((p_).y))

// Staged broadcast reads: the scheduling-barrier intrinsic carries no memory dependence, so plain LDS loads of later chunks
// get clustered above it; a compiler-level memory barrier beside it keeps a software pipeline in place.
#define JSIM_STAGE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); asm volatile("" ::: "memory"); } while (0)
// One wait for a whole chunk of staged broadcast reads, at the chunk's first use: lgkmcnt(n) alone (gfx9 encoding: the other counters
// at their maxima), n = the LDS operations issued AFTER the chunk (the next chunk's reads, a column's write).  The compiler otherwise
// puts a wait in front of every FMA pair of the chunk, and a wave alone on its SIMD pays an issue slot for each, satisfied or not
// (profiles/r20_ubench_wait_cost.txt: 4.4 ticks).  Its wait insertion sees this one and drops those of its own that it makes redundant;
// it drops none that is still needed, so an n that is too large costs the gain, never a value.  Only where the chunk was issued a
// stage ahead: on reads just issued one wait for all of them delays the first FMA by the whole burst (same file: 197 against 157 ticks).
#define JSIM_CHUNK_WAIT(n) __builtin_amdgcn_s_waitcnt(0xC07F | ((n) << 8))
__device__ __forceinline__ void jsim_chunk_wait(int n) // n: a constant once the loops around the call are unrolled
{
    switch (n) {
#define JSIM_CW_CASE(i) case i: JSIM_CHUNK_WAIT(i); break;
        JSIM_CW_CASE(0) JSIM_CW_CASE(1) JSIM_CW_CASE(2) JSIM_CW_CASE(3) JSIM_CW_CASE(4) JSIM_CW_CASE(5) JSIM_CW_CASE(6) JSIM_CW_CASE(7)
        JSIM_CW_CASE(8) JSIM_CW_CASE(9) JSIM_CW_CASE(10) JSIM_CW_CASE(11) JSIM_CW_CASE(12) JSIM_CW_CASE(13) JSIM_CW_CASE(14)
#undef JSIM_CW_CASE
    default: break; // (15 and more: the counter's maximum, nothing to say)
    }
}
// LDS base for constant-address reads of one phase: an opaque zero (see DESIGN.md: the compiler otherwise borrows a
// long-lived register that happens to hold zero, spills it, and reloads it before every ds_read).
#define JSIM_OPAQUE_ZERO(z) int z = 0; asm volatile("" : "+v"(z))

#ifndef JSIM_ZY_CHUNK
#define JSIM_ZY_CHUNK 8
#endif
#ifndef JSIM_CHUNK_WAITS
#define JSIM_CHUNK_WAITS 15 /* one bit per pipeline (see CHW); 0: every wait left to the compiler (A/B builds) */
#endif

#include "loop_pre_tick.inc"

// The loop glue inside the K-tick launch (PRE instantiations): per tick the ego's wave first does what loop_pre_tick_kernel
// does -- progress index, resampling, collision rows, cut-off -- against that tick's obstacle predictions (scripted
// obstacles do not depend on the egos: all K ticks are laid out up front), and the cut-off becomes this tick's path length.
struct PreK {
    PreP pre;                   // the glue's parameters (per-ego pointers inside are not used here)
    const double2 *pred_cc_all; // [n_ticks][n_obs][n_steps][2]
    const double4 *pred_bc_all; // [n_ticks][n_obs] bounding circles of those predictions
    long long *traj_idx;        // [B] in/out  progress index
    int *prev_len;              // [B] in/out  length of the previous truncated path (-1: none)
    int *path_len_out;          // [B] out     the last tick's path length
    int speed_cutoff;           // 1: the glue of mpc_intersection_new_ref.py -- the path stays whole, the cut-off index goes to
    int *cut_io;                //    the controller's speed cut-off [B] in/out (what jsim_mpc_set_speed_cutoff registered)
    int *col_flag;              // [B] out
    int *pre_status;            // [B] out
    TrafficP traffic;           // traffic sets: pre.n_obs is all sets' vehicles, each ego reads its set's slice (set_of NULL: all)
};

// ---------------------------------------------------------------------------------------------------------------------------
// HELP: three helper wavefronts beside the one that owns the ego (round 3).  At 256 egos every ego has a CU to itself and three of
// its four SIMDs idle; three phases of a step come off the owner's critical path without changing a bit of the result:
//   * the nearest-index scan over the remaining path (S1): the helpers scan, each keeps its three nearest points, the owner merges
//     the nine -- while the owner runs the rollout S2, which does not need the index;
//   * H = 2 S'QS: tile ROW w of the MFMA tiles (all its columns, all time steps, the same operands in the same order as the one-wave
//     kernel: bit-identical tiles) by wave w, straight into the Hessian's LDS area; the owner keeps tile row 0, the last helper g;
//   * J = L^-T (the forward substitutions on the rows of the augmented J) consumes the factor column by column, in the order the
//     Cholesky factorisation produces them: helper 1 runs it BESIDE the owner's factorisation, one column behind -- it polls the
//     pivots the owner publishes with the columns (invc) -- and hands the rows over through LDS (Jx).
//   * the factorisation's right half (SPLIT, where H outlives the owner's read of its rows): the chain of pivots stays one chain,
//     but the owner carries only columns [0, NS) of it and helper 2 the rest, each with half the FMAs, reads and waits a column.
// The active-set loop is one dependent chain per iteration and stays with the owner; the helpers sleep at a barrier.  Protocol: the owner posts a command (hb_cmd) and passes a barrier, works, passes a second barrier;
// the helpers loop { barrier; read command; work; barrier }.  Three such pairs per tick, flushed with HB_SKIP on the owner's early
// exits, HB_EXIT after the last tick.
//   * the tick boundary (NB: the glue-free kernels, DESIGN.md section 6): once the new solution stands in LDS (the top of S5) nothing of
//     the next tick's head needs the owner any more.  HB_NEXT opens a fourth pair there, which takes the place of the next tick's
//     HB_SCAN pair: helper 1 steps the plant, rolls the new warm start out (S2) and linearises about it (the part of S3 that needs
//     neither the nearest index nor the reference window), helpers 2 and 3 scan from the new position -- under the owner's outputs and
//     plant / goal / respawn tail.  The pair closes at the top of the next tick; a tick that respawned the ego throws the results away.
enum { HB_SKIP = 0, HB_SCAN = 1, HB_HBUILD = 2, HB_JBUILD = 3, HB_EXIT = 4, HB_NEXT = 5 };

// tan of the clamped steer: what the rollout S2 and the plant step turn with
__device__ __forceinline__ double jsim_clamped_tan(double d, double smax)
{
    double dc = (smax < d) ? smax : d;
    dc = (-smax > dc) ? -smax : dc;
    return tan(dc);
}
// Simulation.step (main/lib/simulation.py:35-47).  cy, sy: cos / sin of the yaw; tn: tan of the clamped steer.  Only the yaw needs tn,
// and nothing else needs the yaw: a caller that wants part of the new state passes anything for the rest and drops those results.
// (What HB_NEXT's two waves step with; the tick's tail keeps the same operations in its own text.)
template <class KPT> // (KP, defined by the including file; read where the text reads it)
__device__ __forceinline__ void jsim_plant_step(double &x, double &y, double &v, double &yaw, double cy, double sy, double tn, double ai, const KPT &P,
                                                double dt)
{
    const double xd = v * cy, yd = v * sy, thd = (v / P.L) * tn;
    x += xd * dt; y += yd * dt; yaw += thd * dt;
    v += ai * dt;
    v = (P.vmax_plant < v) ? P.vmax_plant : v;
    v = (P.vmin > v) ? P.vmin : v;
}

// A helper waits until a column of the factor is published: 1 / sqrt(pivot) of column k, invc[k], is set to -1 before the
// factorisation starts and written (never negative, whatever the pivot: the high word of -1.0 cannot come back) when column k and
// everything in front of it is in LDS -- the helper polls that word; no counter has to be kept by the publishing wave.  Written in
// assembly so that the loop does not exist for the compiler: as a C loop inside the fully unrolled forward substitution it kept that
// loop from being unrolled, Jr[] became dynamically indexed and was "promoted" to 100 KB of LDS.  Bounded (4M polls), so that a
// column that never arrives cannot hang the GPU: the function returns 1 when it gave up (0: published), the helper ORs that into
// `tmo`, posts it in hb_tmo, and the owner ends the tick with JSIM_HELPER_TIMEOUT.  A helper that has given up once polls every
// later column once only (`tmo` in: the poll count starts at its limit).
__device__ __forceinline__ int jsim_spin_published(const double *val_lds, int tmo)
{
    const unsigned addr = (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) const double *)val_lds;
    const int cnt0 = __builtin_amdgcn_readfirstlane(tmo) ? 0x3fffff : 0;
    int v, cnt, cur;
    asm volatile("s_mov_b32 %1, %4\n"
                 "1:\n\t"
                 "ds_read_b32 %0, %3 offset:4\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "v_readfirstlane_b32 %2, %0\n\t"
                 "s_add_u32 %1, %1, 1\n\t"
                 "s_cmp_lg_u32 %2, 0xbff00000\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "s_cmp_lt_u32 %1, 0x400000\n\t"
                 "s_cbranch_scc1 1b\n"
                 "2:"
                 : "=&v"(v), "=&s"(cnt), "=&s"(cur)
                 : "v"(addr), "s"(cnt0)
                 : "memory", "scc");
    return cur == (int)0xbff00000;
}

// tile row ROW of H = 2 S'QS -> Hm (both triangles); the operand formulas are the one-wave kernel's (S4a below)
template <int T, int ROW>
__device__ __forceinline__ void jsim_h_tile_row(const double *tq, double *Hm, int lane, double dt)
{
    constexpr int N = 2 * T, LD = N + 1, TP = T + 2;
    const int kk = lane >> 4, cc = lane & 15;
    double c0[ROW + 1], c1[ROW + 1], p0[ROW + 1], p1[ROW + 1];
    int thr[ROW + 1];
    const bool isd_ = cc & 1;
    const int xrow = (kk < 2 ? (isd_ ? TQ_PB : TQ_PA) : TQ_ONE) * TP, yrow = (kk < 2 ? (isd_ ? TQ_PBP : TQ_PAP) : TQ_ONE) * TP;
    const int w0row = (kk == 0 ? TQ_QXX : kk == 1 ? TQ_QXY : kk == 2 ? TQ_QV : TQ_QYAW) * TP;
    const int w1row = (kk == 0 ? TQ_QXY : kk == 1 ? TQ_QYY : TQ_ZERO) * TP;
#pragma unroll
    for (int c = 0; c <= ROW; ++c) {
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
        thr[c] = vcol ? (kk < 2 ? s + 2 : s + 1) : (T + 2);
    }
    v4d acc[ROW + 1];
#pragma unroll
    for (int b = 0; b <= ROW; ++b) acc[b] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 8 * ROW + 1; t <= T; ++t) {
        const double X = tq[xrow + t], Y = tq[yrow + t], W0 = tq[w0row + t], W1 = tq[w1row + t];
        double aval = 0.0, bval[ROW + 1];
#pragma unroll
        for (int c = 0; c <= ROW; ++c) {
            const bool on = t >= thr[c];
            const double S0 = on ? c0[c] * (X - p0[c]) : 0.0;
            const double S1 = on ? c1[c] * (Y - p1[c]) : 0.0;
            if (c == ROW) aval = kk == 1 ? S1 : S0;
            bval[c] = fma(W0, S0, W1 * S1);
        }
#pragma unroll
        for (int b = 0; b <= ROW; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aval, bval[b], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b <= ROW; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * ROW + kk + 4 * r, col = 16 * b + cc;
            if (row < N && col < N) {
                const double hv = 2.0 * acc[b][r];
                Hm[row * LD + col] = hv;
                if (ROW != b) Hm[col * LD + row] = hv;
            }
        }
}

// g_i = 2 sum_t S_t[:, i]' (Q_t e_t) for the lane's own column i (the one-wave kernel's g, S4a below: the same fused operations in the
// same order; what is skipped there is selected away here, so that the 100 table reads are issued in batches, not behind branches)
template <int T>
__device__ __forceinline__ double jsim_g_own(const double *tq, int lane, double dt)
{
    constexpr int N = 2 * T, TP = T + 2;
    const int so = lane < N ? (lane >> 1) : (T - 1);
    const bool isdo = lane & 1;
    const double kso = tq[TQ_KT * TP + so];
    const double coefo = lane < N ? (isdo ? kso : dt) : 0.0;
    const double pox = isdo ? tq[TQ_PB * TP + so + 1] : tq[TQ_PA * TP + so + 1];
    const double poy = isdo ? tq[TQ_PBP * TP + so + 1] : tq[TQ_PAP * TP + so + 1];
    const int gxrow = (isdo ? TQ_PB : TQ_PA) * TP, gyrow = (isdo ? TQ_PBP : TQ_PAP) * TP, evrow = (isdo ? TQ_QEYAW : TQ_QEV) * TP;
    double gi = 0.0;
#pragma unroll
    for (int t = 1; t <= T; ++t) {
        const double qe = tq[evrow + t], gx = tq[gxrow + t], gy = tq[gyrow + t], qx = tq[TQ_QEX * TP + t], qy = tq[TQ_QEY * TP + t];
        const double g1 = fma(coefo, qe, gi);
        gi = t > so ? g1 : gi;
        const double g2 = fma(coefo * (gx - pox), qx, gi);
        const double g3 = fma(coefo * (gy - poy), qy, g2);
        gi = t >= so + 2 ? g3 : gi;
    }
    return lane < N ? 2.0 * gi : 0.0;
}

// WPE = waves per SIMD the register budget is set for (amdgpu_waves_per_eu: 1 -> 512 registers, 2 -> 256).
//   T <= 13 (the reference's stock horizon): a row is 26 doubles and the kernel fits 256 registers without scratch, so two waves share a
//   SIMD at every batch size: 4096 egos 32.1 -> 44.9 M steps/s, 256 egos 7.43 -> 7.37 M.
//   T = 20: the 256-register form has 180 B of scratch (tick-loop values: ~50 accesses per tick, none in the active-set loop) and the LDS cut to 20.3 KB (the factor's columns on top of H, as the
//   virtual-speed-row kernel does) so that EIGHT egos share a CU.  It loses 1.5 % while every ego has a SIMD to itself (256 egos:
//   4.03 -> 3.96 M) and wins 21 % once there are more egos than SIMDs (4096 egos: 17.7 -> 21.5 M, round 3, same box, same kernels
//   otherwise): launch_reg picks it for B > 1024.  (Round 2 measured this budget as a loss -- 408 B of scratch then; the leaner drop
//   path of round 3 freed the registers.)
//   T = 30 (40.4 KB of LDS: four egos per CU either way) and the PRE instantiations (the loop glue's 28 KB) stay at one wave per SIMD.
template <int T, bool PRE, int WPE, bool HELP = false>
__global__ __launch_bounds__(HELP ? 256 : 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void mpc_step_reg_kernel(const KP Pin, const TickP K, const PreK Q)
{
    static_assert(!HELP || (WPE == 1 && (2 * T + 15) / 16 <= 4), "helpers: one wave per SIMD, one helper per tile row");
    KP P = Pin;
    if ((int)blockIdx.x >= Pin.B) return;
    const int ego = K.order ? K.order[blockIdx.x] : (int)blockIdx.x;
    if (Pin.pe) jsim_apply_ego_cfg(P, Pin.pe, ego, Pin.T, Pin.dt);
    constexpr int N = 2 * T, NR = 3 * T + 1, LD = N + 1, TP = T + 2, MW = (8 * T + 31) / 32;
    constexpr int NTILE = (N + 15) / 16;
    // 3T+1 > 63 lanes (21 <= T <= 31): the T+1 speed rows are VIRTUAL.  v_{t+1} = v_0 + dt * (a_0 + .. + a_t) is an inclusive
    // prefix sum over the even lanes, so lane 2t evaluates the two speed rows of time t+1 as its second candidate pair (the
    // odd lanes keep the steer-rate rows there); the row itself, dt * sum_{s<=t} Jhat[2s][:], is only materialised when a
    // speed row enters the working set (the even lanes put their rows side by side in LDS, lane j adds up column j).
    constexpr bool VS = NR >= 64;
    constexpr int NW = VS ? N : NR; // the lane that carries w = L^-1 g
    static_assert(NW < 64, "register path needs 2T+1 lanes (3T+2 with resident speed rows)");
    constexpr int NP = N + 2; // N is even, so every vector below stays 16-byte aligned
    // One wait per staged chunk (JSIM_CHUNK_WAIT) where the columns are at most 40: the selection of the wait's immediate stands in
    // the body of the column loops until they are unrolled, and with it in them the longer horizons' A, Jr and chunk buffers went to
    // scratch (T = 25: 1072 B, T = 30: 1232 B -- the three arrays' size: their column loops were no longer unrolled in full).
    // Bits: 1 Cholesky, 2 rows of J, 4 z/y dots, 8 Householder update.  HELP: the rows of J are helper 1's, beside the owner's
    // factorisation and not on its path; with the waits there too, <20, false, 1, true> reserved a 20-byte stack that nothing accesses.
    constexpr int CHW = VS ? 0 : HELP ? (JSIM_CHUNK_WAITS & ~2) : JSIM_CHUNK_WAITS;
    // Static LDS (all sizes are compile-time): addresses become instruction immediates.  With a dynamic
    // `extern __shared__` base every one of the ~1000 distinct constant offsets of the unrolled phases was
    // materialised in an SGPR, hoisted out of the tick loop and spilled.
    constexpr int LDC = N + 2, CCH = 16;
    // MFMA tiles -> rows of H (stride LD); then R.  The factor's columns (stride LDC) follow it -- or, when LDS decides how many
    // egos a CU holds (VS), take its place: the rows of H are in registers before the first column is written.
    constexpr bool LCA = VS || (WPE == 2 && T > 13); // the factor's columns on top of H
    constexpr int HLN = LCA ? N * LDC : N * LD + N * LDC;
    constexpr int PREN = PRE ? (int)((sizeof(PreScratch) + 7) / 8) : 0; // the glue's scratch lives here between two solves
    __shared__ __attribute__((aligned(16))) double HL[HLN > PREN ? HLN : PREN];
    double *const Hm = HL;
    constexpr bool HCLR = HELP && !LCA; // the helpers clear R while the owner factors (not where the factor's columns lie on top of H)
    // .. and where H outlives the owner's read of its rows, the factorisation is split by columns: the owner factors [0, NS), helper 2
    // takes the right half of every row from H, applies the owner's columns to it as they are published and factors [NS, N)
    constexpr bool SPLIT = HCLR;
    constexpr int NS = SPLIT ? ((N / 2) & ~1) : N; // even: no 16-byte pair of a column straddles the split
    double *const Lc = HL + (LCA ? 0 : N * LD); // the factor's columns, unscaled (column k at Lc[k*LDC + .])
    static_assert((N * LD) % 2 == 0, "Lc stays 16-byte aligned");
    __shared__ __attribute__((aligned(16))) double gsv[2 * N]; // Givens (c, s) per column pair, identity outside a sweep
    __shared__ __attribute__((aligned(16))) double drow12[2 * NP]; // d = Jhat'n+ : row la of Jhat, then the second row of a steer-rate normal
    double *const drow = drow12, *const drow2 = drow12 + NP;
    __shared__ __attribute__((aligned(16))) double dzv[NP];    // d with the working-set part zeroed (d2)
    __shared__ __attribute__((aligned(16))) double vzv[NP];    // Householder vector v = d2 - rho e1 (zero-padded)
    __shared__ __attribute__((aligned(16))) double rdv[NP];    // diagonal of R (Rm itself keeps zeros on and below its diagonal)
    __shared__ __attribute__((aligned(16))) double UV[VS ? 2 : NR + 5];
    // per-time-step scalars, 1/L[k][k], g, w = L^-1 g -- all dead once the active-set loop starts; VS: the loop's staging
    // area for rows 0, 2, 4, .. of Jhat while a speed row is formed takes their place
    // (in two passes of SPH columns each) -- and the output staging of S5
    constexpr int TQN = (TQ_COUNT * TP + 1) & ~1 /* the vectors behind tq stay 16-byte aligned */;
    constexpr int SPH = (T + 1) & ~1, SPN = VS ? T * SPH : 0;
    static_assert(!VS || (SPN >= NR + 5 || TQN + 3 * NP >= NR + 5), "uvec fits the shared area");
    __shared__ __attribute__((aligned(16))) double SCR[(TQN + 3 * NP > SPN) ? TQN + 3 * NP : SPN];
    double *const tq = SCR, *const invc = SCR + TQN, *const gvc = SCR + TQN + NP, *const wvc = SCR + TQN + 2 * NP;
    double *const spdump = SCR;
    double *const uvec = VS ? SCR : UV;
    __shared__ unsigned maskw[MW + 1];
    // HELP: the owner's mailbox (command, scan inputs) and the helpers' answers (three nearest points per helper)
    __shared__ int hb_cmd, hb_ilen;
    __shared__ int hb_tmo; // a helper's bounded wait for a column ran out in this tick (jsim_spin_published)
    __shared__ __attribute__((aligned(16))) double Jx[HELP ? 64 * (N + 2) : 2];   // rows of the augmented J, helper 1 -> owner
    __shared__ long long hb_s0;
    __shared__ double hb_xy[2], hb_rd[HELP ? 12 : 2];
    __shared__ int hb_ri[HELP ? 12 : 2];
    // NB: the tick boundary's hand-over (HB_NEXT).  Mailbox hb_st: the new speed, then the speed and yaw the step started from (the new
    // position goes in hb_xy).  Helper 1's own: nbz S2's scratch; nbv lane-wise al, be, alp, bep, ccx, ccy, kt, FX, FY (64 each); nbs
    // lane 0's sin and cos of the new yaw (the next plant step's); nbq (VS) the table rows it cannot write in place.
    constexpr bool NB = HELP && !PRE;
    __shared__ double hb_st[NB ? 3 : 1];
    __shared__ __attribute__((aligned(16))) double nbz[NB ? 4 * T : 2];
    __shared__ __attribute__((aligned(16))) double nbv[NB ? 9 * 64 : 2];
    __shared__ double nbs[2];
#ifdef JSIM_STAMPS
    __shared__ int hb_nclk; // (not a length: helper 1's cycles in HB_NEXT, for the owner's clock row)
#endif
    __shared__ __attribute__((aligned(16))) double nbq[(NB && VS) ? TQN : 2];

    const int lane0 = HELP ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int hwave = HELP ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    if (P.pass > 0 && P.status[ego] != JSIM_OK) return; // failed in an earlier pass of this step: the failure stands
    const int it_base = (P.pass > 0 && P.n_iter) ? P.n_iter[ego] : 0;
    int lane = lane0;

    const int pid = P.path_id[ego];
    const long long off = P.poff[pid];
    long long M = P.path_len[ego];
    // PRE: the glue's per-ego loop state
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
        Mfull = (int)(P.poff[pid + 1] - off);
        if (Q.speed_cutoff) pre_cut = Q.cut_io[ego];
    }
    const double speed = P.speed[ego];
    const double dt = P.dt;
    const bool tl = lane < T;
    // controller / plant state carried in registers across ticks
    long long s0 = P.target_ind[ego];
    double sx = P.x0[4 * ego + 0], sy = P.x0[4 * ego + 1], sv = P.x0[4 * ego + 2], syaw = P.x0[4 * ego + 3];
    double wa_t = tl ? P.oa[(size_t)ego * T + lane] : 0.0; // warm start, lane t
    double wd_t = tl ? P.od[(size_t)ego * T + lane] : 0.0;
    double di_prev = K.advance ? K.di_ai[2 * ego] : 0.0;
    double ai_last = K.advance ? K.di_ai[2 * ego + 1] : 0.0;
    int age = K.advance ? K.age[ego] : 0;
    const int hist_base = (K.advance && K.hist) ? *K.tick : 0;
    double2 goal_xy = double2{0.0, 0.0};
    if (K.advance) goal_xy = P.pxy[P.poff[pid + 1] - 1]; // goal = last point of the path given to MPC.__init__

    if (HELP && hwave > 0) { // ---------------------------------------------------------------- the helper wavefronts
        for (;;) {
            __syncthreads();
            const int cmd = __builtin_amdgcn_readfirstlane(hb_cmd);
            if (cmd == HB_EXIT) return;
            // A helper's share of the nearest-index scan: wave W_ of ST_ / 64 takes the points 64 W_ + lane, + ST_, ..; its three nearest
            // (nearest first, ties to the smaller index) go to slots 3 (hwave - 1) .. of hb_rd / hb_ri.  The owner's merge does not
            // depend on how the points were dealt.
#define HB_INSERT_PT(p_, k_)                                                                   \
    {                                                                                          \
        const double dx = (p_).x - hx, dy = (p_).y - hy;                                       \
        const double d = sqrt(dx * dx + dy * dy);                                              \
        if (d < b0) { b2 = b1; i2 = i1; b1 = b0; i1 = i0; b0 = d; i0 = (k_); }                 \
        else if (d < b1) { b2 = b1; i2 = i1; b1 = d; i1 = (k_); }                              \
        else if (d < b2) { b2 = d; i2 = (k_); }                                                \
    }
#define HB_SCAN_WAVE(ST_, W_)                                                                                          \
    {                                                                                                                  \
        const double hx = hb_xy[0], hy = hb_xy[1];                                                                     \
        const int ilen = hb_ilen;                                                                                      \
        const double2 *pp = P.pxy + off + hb_s0;                                                                       \
        double b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;                                                            \
        int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;                                                         \
        int k = (W_) * 64 + lane0;                                                                                     \
        for (; k + 3 * (ST_) < ilen; k += 4 * (ST_)) {                                                                 \
            const double2 p0 = pp[k], p1 = pp[k + (ST_)], p2 = pp[k + 2 * (ST_)], p3 = pp[k + 3 * (ST_)];              \
            HB_INSERT_PT(p0, k) HB_INSERT_PT(p1, k + (ST_)) HB_INSERT_PT(p2, k + 2 * (ST_)) HB_INSERT_PT(p3, k + 3 * (ST_)) \
        }                                                                                                              \
        for (; k < ilen; k += (ST_)) {                                                                                 \
            const double2 p0 = pp[k];                                                                                  \
            HB_INSERT_PT(p0, k)                                                                                        \
        }                                                                                                              \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                                                \
            double v = b0;                                                                                             \
            int id = i0;                                                                                               \
            wargmin_fast(v, id);                                                                                       \
            if (lane0 == 0) { hb_rd[(hwave - 1) * 3 + r] = v; hb_ri[(hwave - 1) * 3 + r] = id; }                       \
            if (i0 == id) { b0 = b1; i0 = i1; b1 = b2; i1 = i2; b2 = INFINITY; i2 = 0x7fffffff; }                      \
        }                                                                                                              \
    }
            if (cmd == HB_SCAN) {
                HB_SCAN_WAVE(192, hwave - 1)
            } else if (NB && cmd == HB_NEXT) {
                if (hwave == 1) {
#ifdef JSIM_STAMPS
                    const long long ht0 = (long long)__builtin_readcyclecounter();
#endif
                    // the next tick's state, rollout and index-free linearisation -- the owner's own texts on the owner's operands
                    const int lane = lane0; // (the shared texts say `lane`)
                    double wa_t = 0.0, wd_t = 0.0;
                    if (tl) { wa_t = uvec[2 * lane]; wd_t = uvec[2 * lane + 1]; }
                    const double wtan = jsim_clamped_tan(wd_t, P.smax);
                    const double sx = hb_xy[0], sy = hb_xy[1], sv = hb_st[0];
                    double syaw = hb_st[NB ? 2 : 0];
                    {
                        double x_ = 0.0, y_ = 0.0, v_ = hb_st[NB ? 1 : 0]; // (the owner posted the new position and speed)
                        jsim_plant_step(x_, y_, v_, syaw, 0.0, 0.0, rdlane(wtan, 0), 0.0, P, dt);
                    }
                    double bx = sx, by = sy, bv = sv, bth = syaw, sn, cs;
                    {
#define JSIM_S2_SCR nbz
#include "mpc_step_reg_s2.inc"
#undef JSIM_S2_SCR
                    }
                    double al = 0, be = 0, alp = 0, bep = 0, ccx = 0, ccy = 0, kt = 0;
                    double PA, PB, PAP, PBP, FX, FY;
                    {
#include "mpc_step_reg_s3a.inc"
                    }
                    double *const rows = VS ? nbq : tq; // (VS: the solution the owner is still reading lies in the table's place)
                    if (lane <= T + 1) {
                        rows[TQ_PA * TP + lane] = PA; rows[TQ_PB * TP + lane] = PB; rows[TQ_PAP * TP + lane] = PAP; rows[TQ_PBP * TP + lane] = PBP;
                        rows[TQ_KT * TP + lane] = kt;
                    }
                    nbv[0 * 64 + lane] = al; nbv[1 * 64 + lane] = be; nbv[2 * 64 + lane] = alp; nbv[3 * 64 + lane] = bep;
                    nbv[4 * 64 + lane] = ccx; nbv[5 * 64 + lane] = ccy; nbv[6 * 64 + lane] = kt; nbv[7 * 64 + lane] = FX; nbv[8 * 64 + lane] = FY;
                    if (lane == 0) { nbs[0] = sn; nbs[1] = cs; }
                    if (lane < 3) { hb_rd[lane] = INFINITY; hb_ri[lane] = 0x7fffffff; } // (no scan of this wave's: the merge takes nine)
                    (void)bx; (void)by;
#ifdef JSIM_STAMPS
                    __builtin_amdgcn_s_waitcnt(0);
                    if (lane == 0) hb_nclk = (int)((long long)__builtin_readcyclecounter() - ht0);
#endif
                } else {
                    HB_SCAN_WAVE(128, hwave - 2)
                }
#undef HB_SCAN_WAVE
#undef HB_INSERT_PT
            } else if (cmd == HB_HBUILD) {
                if (hwave == 1 && NTILE > 1) jsim_h_tile_row<T, 1>(tq, Hm, lane0, dt);
                else if (hwave == 2 && NTILE > 2) jsim_h_tile_row<T, 2>(tq, Hm, lane0, dt);
                else if (hwave == 3 && NTILE > 3) jsim_h_tile_row<T, 3>(tq, Hm, lane0, dt);
                if (hwave == 3) { const double gi = jsim_g_own<T>(tq, lane0, dt); if (lane0 < N) gvc[lane0] = gi; }
            } else if (cmd == HB_JBUILD && hwave == 1) {
                double Jr[N];
                int tmo = 0;
                // (SPLIT: the columns come faster than this wave takes them with a poll -- an LDS round trip -- in front of each: one poll
                //  per two columns, for the odd count ahead; "n columns are published" holds at every call as before)
#define JSIM_J_WAIT(n_) do { if (!SPLIT || (n_) == 1 || !((n_) & 1)) tmo |= jsim_spin_published(&invc[(SPLIT && (n_) + 1 <= N ? (n_) + 1 : (n_)) - 1], tmo); } while (0)
#include "mpc_step_reg_j.inc"
#undef JSIM_J_WAIT
#pragma unroll
                for (int j = 0; j < N; j += 2) *(double2 *)&Jx[lane0 * (N + 2) + j] = double2{Jr[j], Jr[j + 1]};
                if (tmo && lane0 == 0) hb_tmo = 1;
            } else if (cmd == HB_JBUILD && SPLIT && hwave == 2) {
                // the right half of the factorisation.  The lane's row of H, columns [NS, N), with the owner's R / Rd corrections (in LDS
                // before the owner posted the command); H is dead once every lane has its half row -- a wave's LDS operations are
                // performed in order -- and becomes the active-set loop's zeroed R here (the owner passes the phase's closing barrier
                // before the loop).
                if constexpr (SPLIT) { // (discarded elsewhere: N - NS is 0 there)
#ifdef JSIM_STAMPS /* slots 12 .. 14 of the ego's clock row: helper 2 starts, has applied the owner's columns, has factored its own */
#define HSTAMP(i) do { if (P.dbg_clk && lane0 == 0) P.dbg_clk[(size_t)ego * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define HSTAMP(i) do { } while (0)
#endif
                HSTAMP(12);
                double A2[N - NS];
                {
                    const int i = lane0 < N ? lane0 : 0;
#pragma unroll
                    for (int j = NS; j < N; ++j) A2[j - NS] = Hm[i * LD + j];
                    JSIM_STAGE();
                    for (int e = lane0; e < N * LD / 2; e += 64) *(double2 *)&Hm[2 * e] = double2{0.0, 0.0};
                }
                // columns k < NS, as the owner publishes them: A[j] -= (A[k] / c_k) c_j on j >= NS, with the owner's expression for the
                // multiplier on what it published (the lane's own entry of column k, the pivot's reciprocal root).  Lanes < k read an
                // entry nobody wrote: their rows of the factor are not used from column k on.
                int tmo = 0;
                {
                    JSIM_OPAQUE_ZERO(zs_);
                    const double *const LcS = Lc + zs_, *const invS = invc + zs_;
                    const int i = lane0 < N ? lane0 : 0;
                    // two columns per poll (NS is even): the pair (k, k + 1) is read once the pivot of k + 1 is there, the next pair's
                    // poll and reads stand in front of this pair's FMAs
                    double2 cs[2][2][(N - NS) / 2];
                    double own[2][2], invs[2][2];
#define JSIM_S_READ(b_, k_)                                                                                                    \
    {                                                                                                                          \
        tmo |= jsim_spin_published(&invc[(k_) + 1], tmo);                                                                      \
        _Pragma("unroll") for (int c = 0; c < 2; ++c) {                                                                        \
            _Pragma("unroll") for (int j = NS; j < N; j += 2) cs[b_][c][(j - NS) / 2] = *(const double2 *)&LcS[((k_) + c) * LDC + j]; \
            own[b_][c] = LcS[((k_) + c) * LDC + i]; invs[b_][c] = invS[(k_) + c];                                              \
        }                                                                                                                      \
    }
                    JSIM_S_READ(0, 0)
#pragma unroll
                    for (int k = 0; k < NS; k += 2) {
                        if (k + 2 < NS) JSIM_S_READ(((k >> 1) + 1) & 1, k + 2)
                        JSIM_STAGE();
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            const double tk = own[(k >> 1) & 1][c] * (invs[(k >> 1) & 1][c] * invs[(k >> 1) & 1][c]);
#pragma unroll
                            for (int j = NS; j < N; j += 2) {
                                const double2 c2 = cs[(k >> 1) & 1][c][(j - NS) / 2];
                                A2[j - NS] = fma(-tk, c2.x, A2[j - NS]); JSIM_PIN(A2[j - NS]);
                                A2[j + 1 - NS] = fma(-tk, c2.y, A2[j + 1 - NS]); JSIM_PIN(A2[j + 1 - NS]);
                            }
                        }
                        JSIM_STAGE();
                    }
#undef JSIM_S_READ
                }
                if (tmo && lane0 == 0) hb_tmo = 1;
                HSTAMP(13);
#define JSIM_CH_K0 NS
#define JSIM_CH_KE N
#define JSIM_CH_A(j_) A2[(j_) - NS]
#include "mpc_step_reg_chol.inc"
#undef JSIM_CH_K0
#undef JSIM_CH_KE
#undef JSIM_CH_A
                HSTAMP(14);
#undef HSTAMP
                }
            } else if (cmd == HB_JBUILD && HCLR && hwave == 3) {
                // idle in this phase: the active-set loop's identity rotations and zero pads
                if (lane0 < N) { gsv[2 * lane0] = 1.0; gsv[2 * lane0 + 1] = 0.0; }
                if (lane0 < 2) { drow[N + lane0] = 0.0; drow2[N + lane0] = 0.0; dzv[N + lane0] = 0.0; vzv[N + lane0] = 0.0; }
            }
            __syncthreads();
        }
    }
    // tan of the warm start's clamped steer, lane t: what S2 rolls out with.  Evaluated where the warm start is written (here from the
    // loaded one, then in S5 on the new solution, whose lane 0 is also the plant step's) and carried from S5 to S2 only.
    double wtan;
    {
        double dc = (P.smax < wd_t) ? P.smax : wd_t;
        dc = (-P.smax > dc) ? -P.smax : dc;
        wtan = tan(dc);
    }
    bool nb_pending = false, nb_valid = false; // NB: an HB_NEXT pair is open; its results describe the state the next tick starts from
    unsigned it_sum = 0; // active-set iterations of this launch's ticks, both S5 exits: added to K.work / K.iters once, in the last tick
    for (int tk = 0; tk < K.n_ticks; ++tk) {
    // WPE = 2 (256 registers): the state carried from tick to tick is the same in every lane -- say so, and it lives in scalar
    // registers (their overflow goes to single lanes of a spill VGPR, 1/64 of what a uniform value costs in a vector register)
    // instead of vector registers the budget does not have: at T = 20 these went to scratch, written back once per tick.
    if (WPE == 2) {
        sx = uni(sx); sy = uni(sy); sv = uni(sv); syaw = uni(syaw); di_prev = uni(di_prev); ai_last = uni(ai_last);
        goal_xy.x = uni(goal_xy.x); goal_xy.y = uni(goal_xy.y); s0 = uni64(s0); age = uni(age);
    }
    // Re-define `lane` opaquely at every phase boundary: otherwise the hundreds of `lane == k` / `lane < k` exec masks
    // of the unrolled phases are CSE'd across phases / hoisted out of the tick loop, and the register allocator has
    // to spill them (SGPR -> VGPR-lane spills, then VGPR -> AGPR).
#define LANE_FENCE() do { lane = lane0; asm volatile("" : "+v"(lane)); __builtin_assume(lane >= 0 && lane < 64); } while (0)
    LANE_FENCE();
    if (PRE) {
        PreScratch &W = *reinterpret_cast<PreScratch *>(HL);
        PreP pre = Q.pre;
        pre.n_obs = pre_obs.n;
        const PreOut o = jsim_pre_tick_ego(pre, Q.pred_cc_all + ((size_t)tk * Q.pre.n_obs + pre_obs.first) * Q.pre.n_steps * 2,
                                           Q.pred_bc_all + (size_t)tk * Q.pre.n_obs + pre_obs.first, pre_othr, W, lane, ego,
                                           off, Mfull, sx, sy, sv, pre_idx, pre_prev);
        pre_st = o.status;
        if (o.status == JSIM_OK) {
            pre_idx = o.idx; pre_col = o.col;
            if (Q.speed_cutoff) pre_cut = o.path_len; else M = o.path_len;
        }
        pre_prev = Q.speed_cutoff ? Mfull : (int)M; // PreTick.run: this tick's path is the "previous" one of the next
        LDS_SYNC();
        LANE_FENCE();
    }
    double a0n = 0.0, d0n = 0.0; // first control of the new solution
    int status = JSIM_OK;
    int hp = 0;            // HELP: command / barrier pairs passed in this tick (three per tick)
    bool s2_done = false;  // HELP: the rollout ran inside S1
    // the plant step's sin / cos of the tick-start yaw are S2's lane 0 (its bth is syaw + T exact zeros, or syaw itself): kept as
    // uniform values, not in vector registers that would live through the active-set loop
    double p_sn = 0.0, p_cs = 0.0;
    bool p_sc = false;     // S2 ran in this tick
#ifdef JSIM_STAMPS /* slot 15 of the ego's clock row: four stretches of the path across the tick boundary, 16 bits each -- the rollout
                      S2 on the owner (in a tick whose head the helpers ran: helper 1's whole HB_NEXT chain instead), S5's tan, the part
                      of S3 that needs neither the index nor the reference window, the owner's wait at HB_NEXT's closing barrier */
    long long xclk = 0, xt0 = 0;
#define XSTAMP0() do { __builtin_amdgcn_sched_barrier(0); xt0 = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define XSTAMP(k) do { __builtin_amdgcn_sched_barrier(0); xclk |= (((long long)__builtin_readcyclecounter() - xt0) & 0xffff) << (16 * (k)); __builtin_amdgcn_sched_barrier(0); } while (0)
#define XSTAMP_USE(...) asm volatile("" :: __VA_ARGS__)
#else
#define XSTAMP0() do { } while (0)
#define XSTAMP(k) do { } while (0)
#define XSTAMP_USE(...) do { } while (0)
#endif
    do {
    STAMP(0);
    double bx = sx, by = sy, bv = sv, bth = syaw, sn, cs;   // S2's results (declared here: HELP runs S2 inside S1)
    // NB: the previous tick opened an HB_NEXT pair -- it closes here, in front of the merge.  Its results stand unless that tick's tail
    // respawned the ego; then this tick runs whole, as the first tick of a launch does.
    bool nb_use = false;
    if constexpr (NB) if (nb_pending) {
        XSTAMP0();
        __syncthreads();
        XSTAMP(3);
#ifdef JSIM_STAMPS
        xclk |= (long long)hb_nclk & 0xffff;
#endif
        nb_pending = false;
        nb_use = nb_valid;
        if (nb_use) { hp = 1; s2_done = true; sn = nbs[0]; cs = nbs[1]; }
    }
    // ------------------------------------------------------------------ S1: nearest index in direction
    long long tind = s0;
    {
        long long len = M - s0;
        if (len < 0) len = 0;
        if (M < 1) {
            status = 3;
        } else if (len >= 3) {
            double b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
            int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
            const double2 *pp = P.pxy + off + s0;
            const int ilen = (int)len;
#define INSERT_PT(p_, k_)                                                                      \
    {                                                                                          \
        const double dx = (p_).x - sx, dy = (p_).y - sy;                                       \
        const double d = sqrt(dx * dx + dy * dy); /* numpy: sqrt(add.reduce(x*x)) */           \
        if (d < b0) { b2 = b1; i2 = i1; b1 = b0; i1 = i0; b0 = d; i0 = (k_); }                 \
        else if (d < b1) { b2 = b1; i2 = i1; b1 = d; i1 = (k_); }                              \
        else if (d < b2) { b2 = d; i2 = (k_); }                                                \
    }
            if (HELP) {
                // the three helper wavefronts scan (each returns its three nearest points, nearest first); this one rolls out the
                // warm start meanwhile and then merges the nine -- the same three points, in the same order, as one wave's scan finds
                if constexpr (NB) { if (nb_use) goto s1_scanned; } // (scanned and rolled out under the previous tick's tail)
                {
                if (lane == 0) { hb_xy[0] = sx; hb_xy[1] = sy; hb_s0 = s0; hb_ilen = ilen; hb_cmd = HB_SCAN; }
                __syncthreads();
                XSTAMP0();
                {
#define JSIM_S2_SCR tq
#include "mpc_step_reg_s2.inc"
#undef JSIM_S2_SCR
                }
                XSTAMP_USE("v"(bv), "v"(bth), "v"(sn), "v"(cs));
                XSTAMP(0);
                s2_done = true;
                LANE_FENCE();
                __syncthreads();
                }
                s1_scanned:;
                hp = 1;
                if (lane < 9) { b0 = hb_rd[lane]; i0 = hb_ri[lane]; }
                (void)pp;
            } else {
            int k = lane;
            for (; k + 192 < ilen; k += 256) { // four coalesced 1-KiB loads in flight per wave
                const double2 p0 = pp[k], p1 = pp[k + 64], p2 = pp[k + 128], p3 = pp[k + 192];
                INSERT_PT(p0, k) INSERT_PT(p1, k + 64) INSERT_PT(p2, k + 128) INSERT_PT(p3, k + 192)
            }
            for (; k < ilen; k += 64) {
                const double2 p0 = pp[k];
                INSERT_PT(p0, k)
            }
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
    if (status != JSIM_OK) { // the reference raises: nothing of the controller is updated
        if (lane == 0) {
            P.status[ego] = status;
            if (P.n_iter) P.n_iter[ego] = it_base;
        }
        break;
    }

    STAMP(1);
    LANE_FENCE();
    // ------------------------------------------------------------------ S1: travel -> idx -> xref   (lane t <= T)
    const int tl_idx = lane < T ? lane : T;
    double xr, yr, yawr, vr = 0.0;
    double4 ytr = double4{0.0, 0.0, 0.0, 0.0}; // {c1, s1, c2, s2} of S3's weights, from the path table's trig (P.ptrig)
    bool rend;
    long long ik;
    {
        const double vref = (P.vref_min > sv) ? P.vref_min : sv;
        const double cstep = fabs(vref) * dt;
        double trav = cstep;
        if (P.pass == 0) {
#pragma unroll
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + cstep;
        } else { // re-linearisation pass: ov = the previous pass's predicted speeds (mpc.py:232,101)
            const double *ovp = P.ov + (size_t)ego * (T + 1);
            trav = fabs(ovp[0]) * dt;
#pragma unroll
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + fabs(ovp[j]) * dt;
        }
        ik = (long long)rint(trav / P.dl) + tind;
        if (ik > M - 1) ik = M - 1;
        const double2 pr = P.pxy[off + ik];
        xr = pr.x; yr = pr.y; yawr = P.pyaw[off + ik];
        if (P.ptrig) ytr = P.ptrig[off + ik]; // (here, not in S3: it rides the round trip of the two loads above)
        rend = (ik == M - 1);
        if (P.pcv) { // mpc_with_speed variant: xref[2] = cv[idx], cv zeroed from the ego's cut-off index on
            const int cut = (PRE && Q.speed_cutoff) ? pre_cut : (P.cv_cut ? P.cv_cut[ego] : -1);
            vr = (cut < 0 || ik < cut) ? P.pcv[off + ik] : 0.0;
        }
    }
    if (speed - sv < -JSIM_FEAS_TOL || sv - P.vmin < -JSIM_FEAS_TOL) status = JSIM_INFEASIBLE;

    STAMP(2);
    LANE_FENCE();
    // ------------------------------------------------------------------ S2: rollout of the warm start
    if (!(HELP && s2_done)) {
#define JSIM_S2_SCR tq
#include "mpc_step_reg_s2.inc"
#undef JSIM_S2_SCR
    }
    p_sn = rdlane(sn, 0); p_cs = rdlane(cs, 0); p_sc = true;
    if (P.dbg_xbar && lane <= T) {
        double *xb = P.dbg_xbar + (size_t)ego * 4 * (T + 1);
        xb[0 * (T + 1) + lane] = bx; xb[1 * (T + 1) + lane] = by;
        xb[2 * (T + 1) + lane] = bv; xb[3 * (T + 1) + lane] = bth;
    }
    if (P.dbg_idx && lane <= T) P.dbg_idx[(size_t)ego * (T + 1) + lane] = ik;
    if (P.xref && lane <= T) {
        double *xf = P.xref + (size_t)ego * 4 * (T + 1);
        xf[0 * (T + 1) + lane] = xr; xf[1 * (T + 1) + lane] = yr;
        xf[2 * (T + 1) + lane] = vr; xf[3 * (T + 1) + lane] = yawr;
    }
    if (status == JSIM_INFEASIBLE) {
        if (tl) { P.oa[(size_t)ego * T + lane] = 0.0; P.od[(size_t)ego * T + lane] = 0.0; }
        wa_t = 0.0; wd_t = 0.0; wtan = 0.0; s0 = tind;
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = 0u;
        if (lane == 0) {
            P.status[ego] = status;
            P.target_ind[ego] = tind;
            if (P.n_iter) P.n_iter[ego] = it_base;
        }
        break;
    }

    STAMP(3);
    LANE_FENCE();
    // ------------------------------------------------------------------ S3: linearisation coefficients (lane t < T)
    double al = 0, be = 0, alp = 0, bep = 0, ccx = 0, ccy = 0, kt = 0;
    XSTAMP0();
    {
        double PA, PB, PAP, PBP, FX, FY;
        if constexpr (NB) { // (discarded elsewhere: nothing of the hand-over is instantiated in the other kernels)
        if (nb_use) { // helper 1 ran this part under the previous tick's tail: its rows stand in the table, the rest comes over
            al = nbv[0 * 64 + lane]; be = nbv[1 * 64 + lane]; alp = nbv[2 * 64 + lane]; bep = nbv[3 * 64 + lane];
            ccx = nbv[4 * 64 + lane]; ccy = nbv[5 * 64 + lane]; kt = nbv[6 * 64 + lane]; FX = nbv[7 * 64 + lane]; FY = nbv[8 * 64 + lane];
            if (VS && lane <= T + 1) {
                tq[TQ_PA * TP + lane] = nbq[TQ_PA * TP + lane]; tq[TQ_PB * TP + lane] = nbq[TQ_PB * TP + lane];
                tq[TQ_PAP * TP + lane] = nbq[TQ_PAP * TP + lane]; tq[TQ_PBP * TP + lane] = nbq[TQ_PBP * TP + lane];
                tq[TQ_KT * TP + lane] = nbq[TQ_KT * TP + lane];
            }
            PA = PB = PAP = PBP = 0.0;
        } else {
#include "mpc_step_reg_s3a.inc"
        }
        } else {
#include "mpc_step_reg_s3a.inc"
        }
        XSTAMP_USE("v"(PA), "v"(PB), "v"(PAP), "v"(PBP), "v"(FX), "v"(FY), "v"(kt));
        XSTAMP(2);
        double Qxx = 0, Qxy = 0, Qyy = 0, qv = 0, qyaw = 0;
        if (lane >= 1 && lane <= T) {
            if (!rend) {
                double c1 = ytr.x, s1 = ytr.y, c2 = ytr.z, s2 = ytr.w;
                if (!P.ptrig) { // no table (JSIM_PATH_TRIG=0): what path_trig_kernel evaluates, here
                    const double a1 = yawr + 0.5 * M_PI;   // (sincos: one argument reduction per angle; the same values as cos() and sin() -- checked bit for bit)
                    sincos(a1, &s1, &c1); sincos(yawr, &s2, &c2);
                }
                Qxx = (c1 * c1) * P.w_perp + (c2 * c2) * P.w_para;
                Qxy = (c1 * s1) * P.w_perp + (c2 * s2) * P.w_para;
                Qyy = (s1 * s1) * P.w_perp + (s2 * s2) * P.w_para;
                qv = P.Qv; qyaw = P.Qyaw;
            } else {
                Qxx = P.Qf0; Qyy = P.Qf1; qv = P.Qf2; qyaw = P.Qf3;
            }
        }
        const double ex = FX - xr, ey = FY - yr, ev = sv - vr, eyaw = syaw - yawr;
        if (lane <= T + 1) {
            const int t = lane;
            const bool in = lane <= T;
#define JSIM_S3_ROWS() do { tq[TQ_PA * TP + t] = PA; tq[TQ_PB * TP + t] = PB; tq[TQ_PAP * TP + t] = PAP; tq[TQ_PBP * TP + t] = PBP; tq[TQ_KT * TP + t] = kt; } while (0)
            if constexpr (NB) { if (!nb_use) JSIM_S3_ROWS(); } else JSIM_S3_ROWS();
#undef JSIM_S3_ROWS
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
    LDS_SYNC();

    STAMP(4);
    LANE_FENCE();
    // ------------------------------------------------------------------ S4a: H = 2 S'QS (fp64 MFMA), g on the VALU
    // time step outer (its scalars are fetched once), column tiles inner; S_t[:, tile c] serves as the A operand of
    // tile row c and, weighted by Q_t, as the B operand of tile column c.
    double gi_own = 0.0;
    if (HELP) {
        // tile row w of H by wave w (this one: row 0), g by the last helper: the same operations in the same order as below
        if (lane == 0) hb_cmd = HB_HBUILD;
        __syncthreads();
        jsim_h_tile_row<T, 0>(tq, Hm, lane, dt);
        __syncthreads();
        hp = 2;
        gi_own = lane < N ? gvc[lane] : 0.0;   // (helper 3's)
    } else {
        const int kk = lane >> 4, cc = lane & 15;
        // MFMA operands of lane (kk, cc) for column tile c at time t, written so that the four kk cases share ONE formula
        // (selects folded into per-lane table rows and coefficients -- 13 VALU per (t, tile) instead of ~30):
        //   S0 = [t >= thr] c0 (X_t - p0) ,  S1 = [t >= thr] c1 (Y_t - p1) ,  A = (kk == 1 ? S1 : S0) ,  B = fma(W0_t, S0, W1_t S1)
        //   kk < 2 : X/Y = prefix sums of the column's kind (PA/PAP or PB/PBP), c0 = c1 = coef, p = prefix at s+1, thr = s + 2,
        //            (W0, W1) = (Qxx, Qxy) for kk = 0, (Qxy, Qyy) for kk = 1                  -> exactly the x / y rows of S_t, Q_t S_t
        //   kk >= 2: X = the constant-one row, c0 = c23, p0 = 0, c1 = 0, thr = s + 1, (W0, W1) = (q_v or q_yaw, 0)  -> S23, q S23
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
        // own column (lane i < N) for g
        const int so = lane < N ? (lane >> 1) : (T - 1);
        const bool isdo = lane & 1;
        const double kso = tq[TQ_KT * TP + so];
        const double coefo = lane < N ? (isdo ? kso : dt) : 0.0;
        const double pox = isdo ? tq[TQ_PB * TP + so + 1] : tq[TQ_PA * TP + so + 1];
        const double poy = isdo ? tq[TQ_PBP * TP + so + 1] : tq[TQ_PAP * TP + so + 1];
        const int gxrow = (isdo ? TQ_PB : TQ_PA) * TP, gyrow = (isdo ? TQ_PBP : TQ_PAP) * TP;

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
                if (t >= 8 * a + 1) { // S_t has no entry in column tile a before t = 8a + 1
#pragma unroll
                    for (int b = 0; b <= a; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aval[a], bval[b], acc[a][b], 0, 0, 0);
                }
            }
            // g_i += S_t[:, i]' (Q_t e_t)
            if (t > so) {
                gi_own = fma(coefo, isdo ? tq[TQ_QEYAW * TP + t] : tq[TQ_QEV * TP + t], gi_own);
                if (t >= so + 2) {
                    gi_own = fma(coefo * (tq[gxrow + t] - pox), tq[TQ_QEX * TP + t], gi_own);
                    gi_own = fma(coefo * (tq[gyrow + t] - poy), tq[TQ_QEY * TP + t], gi_own);
                }
            }
        }
        gi_own = lane < N ? 2.0 * gi_own : 0.0;
#pragma unroll
        for (int a = 0; a < NTILE; ++a)
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
    LDS_SYNC();
    STAMP(5);
    LANE_FENCE();
    // rows to registers, with the input cost R / R_end (mpc.py:180-183) and difference cost Rd (mpc.py:186) added
    double A[N]; // row i of H, then of L (lower), then row i of R
    {
        // the three entries of row i that the input costs touch are corrected in LDS (the lane's own row: nobody else reads it), then the
        // row comes over as it is -- the same additions as `if (j == i) A[j] += ..; if (j == i + 2 || j + 2 == i) A[j] -= rdc;` on
        // every j, which cost two compares and two selects per entry of the row
        const int i = lane < N ? lane : 0;
        const int t = i >> 1, c = i & 1;
        const double Rt = (tq[TQ_REND * TP + t] != 0.0) ? (c ? P.Re1 : P.Re0) : (c ? P.R1 : P.R0);
        const double rdc = 2.0 * (c ? P.Rd1 : P.Rd0);
        const int nd = (T >= 2) ? ((t == 0 || t == T - 1) ? 1 : 2) : 0;
        if (lane < N) {
            Hm[i * LD + i] += 2.0 * Rt + nd * rdc;
            if (i + 2 < N) Hm[i * LD + i + 2] -= rdc;
            if (i >= 2) Hm[i * LD + i - 2] -= rdc;
        }
        LDS_SYNC();
#pragma unroll
        for (int j = 0; j < NS; ++j) A[j] = Hm[i * LD + j]; // (SPLIT: the right half of the row is helper 2's)
    }
    if (P.dbg_g && lane < N) P.dbg_g[(size_t)ego * N + lane] = gi_own;
    if (P.dbg_H && lane < N) {
        double *Hd = P.dbg_H + (size_t)ego * N * N + (size_t)lane * N;
#pragma unroll
        for (int j = 0; j < N; ++j) Hd[j] = j < NS ? A[j] : Hm[lane * LD + j];
    }
    const double gmax = wmax_dpp(fabs(gi_own));

    if (lane < N) gvc[lane] = gi_own;
    STAMP(6);
    LANE_FENCE();
    // ------------------------------------------------------------------ S4b: Cholesky, right-looking, column by column through LDS
    // (the column loop: mpc_step_reg_chol.inc.)  The same columns then drive the forward substitutions below -- no row broadcasts (two
    // v_readlane per operand), no dump of L.  Measured against the in-register version with v_readlane broadcasts: see DESIGN.md.
    // SPLIT: the owner factors columns [0, NS) of all rows and goes to the phase's closing barrier; helper 2 has the rest.
    if (HELP) { // helper 1 starts the forward substitutions beside this factorisation (SPLIT: helper 2 the factor's right half)
        if (lane < N) invc[lane] = -1.0;     // (invc[k] != -1: column k is published)
        if (lane == 0) { hb_tmo = 0; hb_cmd = HB_JBUILD; }
        __syncthreads();
    }
#define JSIM_CH_K0 0
#define JSIM_CH_KE NS
#define JSIM_CH_A(j_) A[(j_)]
#include "mpc_step_reg_chol.inc"
#undef JSIM_CH_K0
#undef JSIM_CH_KE
#undef JSIM_CH_A
    LDS_SYNC();

    STAMP(7);
    LANE_FENCE();
    // ------------------------------------------------------------------ rows of the augmented J:  L y = rhs, column by column
    //   lane r < N : rhs = e_r                        -> y = row r of J = L^-T
    //   lane N + t : rhs = dt * sum_{s<t} e_{2s}      -> y = dt * sum_{s<t} J[2s][:]   (speed row t)
    //   lane NR    : rhs = g                          -> w = L^-1 g  (u0 = -J w)
    double Jr[N];
    if (!HELP) {
#define JSIM_J_WAIT(n_) do { } while (0)
#include "mpc_step_reg_j.inc"
#undef JSIM_J_WAIT
    } else { // helper 1 has them (and w in wvc): one barrier, then this lane's row from LDS
        __syncthreads();
        hp = 3;
        if (__builtin_amdgcn_readfirstlane(hb_tmo)) { // a helper gave up waiting for a column: neither the factor nor J can be trusted
            status = JSIM_HELPER_TIMEOUT;
            if (lane == 0) {
                P.status[ego] = status;
                if (P.n_iter) P.n_iter[ego] = it_base;
            }
            break;
        }
#pragma unroll
        for (int j = 0; j < N; j += 2) { const double2 v2 = *(const double2 *)&Jx[lane * (N + 2) + j]; Jr[j] = v2.x; Jr[j + 1] = v2.y; }
    }
    LDS_SYNC();

    STAMP(8);
    LANE_FENCE();
    // ------------------------------------------------------------------ unconstrained optimum  val = -Jhat w  (+ v0 on the speed rows)
    double val = 0.0; // lane i < N: u_i ; lane N + t: v_t
    {
        double v0 = 0.0, v1 = 0.0;
        JSIM_OPAQUE_ZERO(zw_);
        const double *const wvW = wvc + zw_;
#pragma unroll
        for (int h = 0; h < N; h += CCH) {
            double2 wb[CCH / 2];
#pragma unroll
            for (int j = h; j < h + CCH && j < N; j += 2) wb[(j - h) / 2] = *(const double2 *)&wvW[j];
            JSIM_STAGE();
#pragma unroll
            for (int j = h; j < h + CCH && j < N; j += 2) {
                v0 = fma(-Jr[j], wb[(j - h) / 2].x, v0);
                v1 = fma(-Jr[j + 1], wb[(j - h) / 2].y, v1);
            }
            JSIM_PIN(v0); JSIM_PIN(v1);
            JSIM_STAGE();
        }
        val = v0 + v1;
        if (!VS && lane >= N && lane < NR) val += sv;
    }
    LDS_SYNC();
    // VS: squared norms of the speed rows (the static weights of the entering rule below), while the factor's area is free:
    // rows 0, 2, 4, .. of Jhat side by side, lane j turns column j into its running sum, lane 2t then reads row t back --
    // 60 cross-lane prefix scans would cost five times as much.
    double spw = 0.0;
    if (VS) {
        const bool evl = lane < N && !(lane & 1);
        if (evl) {
            const int rb = (lane >> 1) * NP;
#pragma unroll
            for (int j = 0; j < N; j += 2) *(double2 *)&HL[rb + j] = double2{Jr[j], Jr[j + 1]};
        }
        LDS_SYNC();
        {
            const int li = lane < N ? lane : N; // lanes >= N work on the padding column
            double a_ = 0.0;
#pragma unroll
            for (int s_ = 0; s_ < T; ++s_) {
                a_ += HL[s_ * NP + li];
                HL[s_ * NP + li] = a_;
            }
        }
        LDS_SYNC();
        {
            const int rb = evl ? (lane >> 1) * NP : 0;
            double n0 = 0.0, n1 = 0.0;
#pragma unroll
            for (int j = 0; j < N; j += 2) {
                const double2 p2 = *(const double2 *)&HL[rb + j];
                n0 = fma(p2.x, p2.x, n0); n1 = fma(p2.y, p2.y, n1);
            }
            spw = (dt * dt) * (n0 + n1);
        }
        LDS_SYNC();
    }
    // From here on Hm holds the STRICT upper triangle of R (row k at Rm[k*LD + ...]); everything on/below the
    // diagonal and every column >= q is kept at exactly 0, the diagonal lives in rdv[] / as 1/R[k][k] in lane k.
    // With that invariant the back substitution needs no masks: steps beyond q and lanes below a row are no-ops.
    // (An explicit R^-1 with r = R^-1 d1 as a lane-parallel product was measured: same cost per add, but every drop
    // then pays a second rotation sweep, which is what the slowest egos -- the ones that set the launch time -- do most.)
    double *const Rm = Hm;
    if (!HCLR) { // (HCLR: helpers 2 and 3 did this beside the factorisation)
        for (int e = lane; e < N * LD; e += 64) Rm[e] = 0.0;
        if (lane < N) { gsv[2 * lane] = 1.0; gsv[2 * lane + 1] = 0.0; } // identity rotations outside a sweep
        if (lane < 2) { drow[N + lane] = 0.0; drow2[N + lane] = 0.0; dzv[N + lane] = 0.0; vzv[N + lane] = 0.0; }
    }
    LDS_SYNC();

    STAMP(9);
    LANE_FENCE();
    // ------------------------------------------------------------------ Goldfarb-Idnani dual active-set iterations
    // per-lane candidate rows (canonical ids) -- lane 2t: AU, AL; lane 2t+1: S+, S-, D+(t), D-(t); lane N+t: VU, VL.
    // Every lane tests  val - ub  (row c0),  lb - val  (row c1)  and, on the steer lanes,  +-(nxt - val) - dmax
    // (rows c2, c3) against its own bounds: no lane-type branches inside the loop.
    int cid0 = -1, cid1 = -1, cid2 = -1, cid3 = -1;
    double ub0 = 0.0, lb1 = 0.0;
    const double dmx = P.dmax;
    double thr0 = 0, thr1 = 0, thr23 = 0;
    double ub2 = dmx, lb3 = -dmx, thr3 = 0; // VS: bounds of the second pair (steer rate on the odd lanes, speed on the even ones)
    if (lane < N) {
        const int t = lane >> 1;
        if ((lane & 1) == 0) {
            cid0 = 4 * T + t; cid1 = 5 * T + t;
            ub0 = P.amax; lb1 = P.amin;
            thr0 = JSIM_VIOL_TOL * (1.0 + fabs(P.amax)); thr1 = JSIM_VIOL_TOL * (1.0 + fabs(P.amin));
            if (VS) { // speed rows of time t + 1
                cid2 = 2 * T - 2 + t + 1; cid3 = 3 * T - 1 + t + 1;
                ub2 = speed; lb3 = P.vmin;
                thr23 = JSIM_VIOL_TOL * (1.0 + fabs(speed - sv)); thr3 = JSIM_VIOL_TOL * (1.0 + fabs(sv - P.vmin));
            }
        } else {
            cid0 = 6 * T + 2 * t; cid1 = cid0 + 1;
            ub0 = P.smax; lb1 = -P.smax;
            thr0 = thr1 = JSIM_VIOL_TOL * (1.0 + P.smax);
            if (t + 1 < T) { cid2 = 2 * t; cid3 = 2 * t + 1; }
            thr23 = thr3 = JSIM_VIOL_TOL * (1.0 + P.dmax);
        }
    } else if (!VS && lane < NR && lane > N) { // t >= 1 (the t = 0 rows are constant)
        const int t = lane - N;
        cid0 = 2 * T - 2 + t; cid1 = 3 * T - 1 + t;
        ub0 = speed; lb1 = P.vmin;
        thr0 = JSIM_VIOL_TOL * (1.0 + fabs(speed - sv)); thr1 = JSIM_VIOL_TOL * (1.0 + fabs(sv - P.vmin));
    }
    // static steepest-edge weights of the entering-row rule: 1 / (n' H^-1 n) = 1 / ||Jhat' n||^2 at the start of the solve.
    // Rows c0, c1 of a lane share ||Jhat[lane]||^2; the steer-rate rows need ||Jhat[lane + 2] - Jhat[lane]||^2.
    double iw01, iw23, w01, w23; // w = ||Jhat'n||^2 = n'H^-1 n: invariant under the orthogonal column updates of Jhat
    {
        double rn0 = 0.0, rn1 = 0.0, dn0 = 0.0, dn1 = 0.0;
        if (HELP) {
            // row lane + 2 straight from the rows helper 1 left in Jx (nothing writes there before the next tick's HB_JBUILD) instead
            // of one cross-lane shuffle per column: the same operands in the same order.  Lanes without a steer-rate row read their own.
            const double *const Jn = Jx + (cid2 >= 0 ? lane + 2 : lane) * (N + 2);
#pragma unroll
            for (int h = 0; h < N; h += CCH) {
                double2 nb[CCH / 2];
#pragma unroll
                for (int j = h; j < h + CCH && j < N; j += 2) nb[(j - h) / 2] = *(const double2 *)&Jn[j];
                JSIM_STAGE();
#pragma unroll
                for (int j = h; j < h + CCH && j < N; j += 2) {
                    rn0 = fma(Jr[j], Jr[j], rn0); rn1 = fma(Jr[j + 1], Jr[j + 1], rn1);
                    const double e0 = nb[(j - h) / 2].x - Jr[j], e1 = nb[(j - h) / 2].y - Jr[j + 1];
                    dn0 = fma(e0, e0, dn0); dn1 = fma(e1, e1, dn1);
                }
                JSIM_STAGE();
            }
        } else {
#pragma unroll
        for (int j = 0; j < N; j += 2) {
            rn0 = fma(Jr[j], Jr[j], rn0); rn1 = fma(Jr[j + 1], Jr[j + 1], rn1);
            const double e0 = __shfl_down(Jr[j], 2) - Jr[j], e1 = __shfl_down(Jr[j + 1], 2) - Jr[j + 1];
            dn0 = fma(e0, e0, dn0); dn1 = fma(e1, e1, dn1);
        }
        }
        const double rn = rn0 + rn1;
        const double dn = (VS && lane < N && !(lane & 1)) ? spw : dn0 + dn1; // even lanes (VS): their speed row
        w01 = rn > 0.0 ? rn : 1.0;
        w23 = dn > 0.0 ? dn : 1.0;
        iw01 = fast_rcp(w01);
        iw23 = fast_rcp(w23);
    }

    int q = 0, iters = 0;
    constexpr int max_iters = 50 * N + 100;
#ifdef JSIM_STAMPS
    long long gclk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gt0 = 0, gt1 = 0;
#define GSTAMP0() do { gt0 = (long long)__builtin_readcyclecounter(); } while (0)
#define GSTAMP(i) do { gt1 = (long long)__builtin_readcyclecounter(); gclk[i] += gt1 - gt0; gt0 = gt1; } while (0)
#else
#define GSTAMP0() do { } while (0)
#define GSTAMP(i) do { } while (0)
#endif
    unsigned abits = 0;  // which of this lane's candidate rows are in the working set
    double lam = 0.0;    // lane k < q: multiplier of working-set position k
    double rdiag = 0.0;  // lane k < q: 1 / R[k][k]
    int actid = -1;      // lane k < q: canonical row id at position k
    // ---- step 1: among the violated rows the one with the largest viol^2 / (n'H^-1 n)  (ties -> lowest canonical index)
    // The two rows of a pair (upper / lower bound of the same quantity) cannot both be violated, so a lane evaluates
    // ONE candidate per pair.  The key keeps its upper 44 bits and carries 511 - row id in the low 9 (jsim_key_pack):
    // positive doubles order like their bit patterns, so one 64-bit max is the whole arg-max, ties included.
    // The search reads only `val` and `abits`: the one for the NEXT entering row is issued right after the step update of an
    // add, ahead of the Householder update of Jhat it does not depend on -- its DPP / readlane chains then run under that
    // update's arithmetic instead of in front of the next publish.
    double s_win, s_violp, s_dd; // winner of the pending search: packed key (0: no violated row), violation, n'H^-1 n
    int s_owner, s_obit;
    double sk_key = 0.0, sk_viol = 0.0, sk_dd = 0.0, sk_red = 0.0; // stages of a search in flight (per lane)
    int sk_bit = 0;
    // stage A: every lane's best candidate (packed key, violation, weight, which of its rows)
#define JSIM_SEARCH_A()                                                                                            \
    {                                                                                                              \
        const double nxt = __shfl_down(val, 2); /* delta_{t+1} for the steer-rate rows */                          \
        const double va = val - ub0, vb = lb1 - val;                                                               \
        const bool up01 = va >= vb;                                                                                \
        const double v01 = up01 ? va : vb;                                                                         \
        const bool ok01 = (cid0 >= 0) & !(abits & (up01 ? 1u : 2u)) & (v01 > (up01 ? thr0 : thr1));                \
        const double k01 = ok01 ? jsim_key_pack(v01 * v01 * iw01, up01 ? cid0 : cid1) : 0.0;                       \
        double e23 = nxt - val;                                                                                    \
        bool up23 = e23 >= 0.0;                                                                                    \
        double v23 = fabs(e23) - dmx;                                                                              \
        bool ok23 = (cid2 >= 0) & !(abits & (up23 ? 4u : 8u)) & (v23 > thr23);                                     \
        if (VS) { /* the even lanes test v_{t+1} = v_0 + dt * (a_0 + .. + a_t) against its two bounds in this slot */ \
            const bool evl = lane < N && !(lane & 1);                                                              \
            const double vsp = fma(dt, wincscan_dpp(evl ? val : 0.0, lane), sv);                                   \
            const double x2 = evl ? vsp : e23;                                                                     \
            const double vu = x2 - ub2, vl = lb3 - x2;                                                             \
            up23 = vu >= vl;                                                                                       \
            v23 = up23 ? vu : vl;                                                                                  \
            ok23 = (cid2 >= 0) & !(abits & (up23 ? 4u : 8u)) & (v23 > (up23 ? thr23 : thr3));                      \
        }                                                                                                          \
        const double k23 = ok23 ? jsim_key_pack(v23 * v23 * iw23, up23 ? cid2 : cid3) : 0.0;                       \
        const bool t23 = k23 > k01;                                                                                \
        sk_key = t23 ? k23 : k01;                                                                                  \
        sk_viol = t23 ? v23 : v01;                                                                                 \
        sk_dd = t23 ? w23 : w01;                                                                                   \
        sk_bit = t23 ? (up23 ? 2 : 3) : (up01 ? 0 : 1);                                                            \
        sk_red = sk_key;                                                                                           \
    }
    // stages B1, B2: the wave maximum of the keys inside every 16-lane row (two DPP steps each)
#define JSIM_SEARCH_B1() { sk_red = vmax_f64(sk_red, dpp_f64<DPP_QP_1032>(sk_red)); sk_red = vmax_f64(sk_red, dpp_f64<DPP_QP_2301>(sk_red)); }
#define JSIM_SEARCH_B2() { sk_red = vmax_f64(sk_red, dpp_f64<DPP_ROW_HALF_MIRROR>(sk_red)); sk_red = vmax_f64(sk_red, dpp_f64<DPP_ROW_MIRROR>(sk_red)); }
    // stage C: across the four rows, then the owner's data (uniform)
#define JSIM_SEARCH_C()                                                                                            \
    {                                                                                                              \
        s_win = fmax(fmax(rdlane(sk_red, 0), rdlane(sk_red, 16)), fmax(rdlane(sk_red, 32), rdlane(sk_red, 48)));  \
        const unsigned long long wb_ = __ballot(sk_key == s_win);                                                  \
        s_owner = wb_ ? __builtin_ctzll(wb_) : 0;                                                                  \
        s_obit = __builtin_amdgcn_readlane(sk_bit, s_owner);                                                       \
        s_violp = rdlane(sk_viol, s_owner);                                                                        \
        s_dd = rdlane(sk_dd, s_owner); /* ||d||^2 = n'H^-1 n does not change while J is updated orthogonally */    \
    }
#define JSIM_SEARCH() { JSIM_SEARCH_A() JSIM_SEARCH_B1() JSIM_SEARCH_B2() JSIM_SEARCH_C() }
    JSIM_SEARCH()
    // WPE = 2 at T = 20: the seven S3 coefficients S5 needs again are not carried through the active-set loop in registers the
    // 256-register budget does not have (they went to scratch: 2.8 GB of HBM writes per 100-tick launch of 4096 egos) but parked in
    // rows of the per-time-step table that are dead by now (the cost weights, read last by the H and g builds); kt is still in its row.
    constexpr bool PARK = (WPE == 2 && !VS && T > 13);
    if (PARK) {
        if (lane <= T) {
            tq[TQ_QXX * TP + lane] = al; tq[TQ_QXY * TP + lane] = be; tq[TQ_QYY * TP + lane] = alp;
            tq[TQ_QV * TP + lane] = bep; tq[TQ_QYAW * TP + lane] = ccx; tq[TQ_QEX * TP + lane] = ccy;
        }
        al = be = alp = bep = ccx = ccy = kt = 0.0;
    }
    for (;;) {
        LANE_FENCE();
        GSTAMP0();
        if (!(s_win > 0.0)) break; // no violated row: optimal
        const int p = 511 - (__double2loint(s_win) & 511);
        double violp = s_violp;
        const int owner = s_owner, obit = s_obit;
        const double dd = s_dd;
        const bool nega = !(obit & 1); // n+ = -G_p' = ca * Jhat[la] (+ cb * Jhat[lb]),  ca = nega ? -1 : +1,  cb = -ca
        const int lb = obit >= 2 ? owner : -1;
        const int la = obit >= 2 ? owner + 2 : owner;
        const bool spd = VS && obit >= 2 && !(owner & 1); // VS: the entering row is a speed row (of time owner / 2 + 1)
#if defined(JSIM_STAMPS) || defined(JSIM_SPAN)
        if (P.dbg_max_gi >= 0 && q >= P.dbg_max_gi) break; // timing experiments only (diagnostic builds)
#endif
        double lplus = 0.0;
        bool failed = false;

        GSTAMP(0);
        for (;;) { // ---- step 2
            if (++iters > max_iters) { failed = true; break; }
            GSTAMP0();
            // d = Jhat' n+ : the owning lane(s) publish their row, every lane j < N then holds d_j
            // (one pass for both rows of a steer-rate normal: the two owners write side by side into the two halves of
            // drow12 -- an LDS write instruction costs ~25 cycles however many lanes take part)
            double dloc;
            if (VS && spd) {
                // a speed row: dt * (Jhat[0] + Jhat[2] + .. + Jhat[owner]) -- the even lanes put their rows side by side,
                // lane j adds up column j (uniform 0/1 factors instead of a trip count: one straight run of reads)
                // (two passes of half the columns each: the staging area is what decides whether a CU holds 3 or 4 egos)
                const int tsel = owner >> 1;
                double acc = 0.0;
#pragma unroll
                for (int hp = 0; hp < 2; ++hp) {
                    const int c0 = hp * SPH, c1 = hp ? N : SPH;
                    if (lane < N && !(lane & 1)) {
                        const int rb = (lane >> 1) * SPH;
#pragma unroll
                        for (int j = c0; j < c1; j += 2) *(double2 *)&spdump[rb + j - c0] = double2{Jr[j], Jr[j + 1]};
                    }
                    LDS_SYNC();
                    const bool mine = lane >= c0 && lane < c1;
                    const int li = mine ? lane - c0 : 0;
                    double a_ = 0.0;
#pragma unroll
                    for (int s_ = 0; s_ < T; ++s_) {
                        const double m_ = s_ <= tsel ? 1.0 : 0.0;
                        a_ = fma(m_, spdump[s_ * SPH + li], a_);
                    }
                    acc = mine ? a_ : acc;
                    LDS_SYNC();
                }
                dloc = lane < N ? dt * acc : 0.0;
                dloc = nega ? -dloc : dloc;
            } else {
            if (lane == la || lane == lb) {
                const int o2 = (lane == lb) ? NP : 0;
#pragma unroll
                for (int j = 0; j < N; j += 2) *(double2 *)&drow12[o2 + j] = double2{Jr[j], Jr[j + 1]};
            }
            LDS_SYNC();
            // (no lane guards: a uniform or exec-skip branch costs ~35 cycles; lanes >= N read the zero padding at [N])
            {
                const int li = lane < N ? lane : N;
                const double da = drow[li], db = drow2[li];
                dloc = lb >= 0 ? da - db : da;
                dloc = nega ? -dloc : dloc;
            }
            }
            GSTAMP(1);
            const double zn = wsum_dpp(lane >= q ? dloc * dloc : 0.0);
            const double dq = rdlane(dloc, q < N ? q : 0);
            const double inrm = fast_rsqrt(zn > 1e-300 ? zn : 1e-300);
            const double nrm = zn * inrm;
            const double sg = dq >= 0.0 ? 1.0 : -1.0;
            {
                const int li = lane < N ? lane : N + 1;            // lanes >= N rewrite the zero at [N + 1]
                const double dzl = (lane >= q && lane < N) ? dloc : 0.0;
                dzv[li] = dzl;
                vzv[li] = lane == q ? dzl + sg * nrm : dzl; // v = d2 + sg*||d2|| e1
            }
            LDS_SYNC();
            GSTAMP(2);
            // z = Jhat2 d2  and  y = Jhat2 v  (y only matters when the row is added)
            double z0 = 0.0, z1 = 0.0, y0 = 0.0, y1 = 0.0;
            // The back substitution behind the dots takes its columns below BSD through the row broadcast (one 16-lane row).  One wave
            // per SIMD: their entries of R from column BSA_LO up are read ahead, under the last chunk of the dots, the lower ones when
            // the steps start -- that round trip passes under the upper steps.  (All sixteen ahead: ~40 more AGPR moves per tick around
            // the loop in the headline kernel, and slower; two waves per SIMD have no registers for any: they read in place.)
            constexpr int BSD = 16, BSA_LO = 8;
            constexpr bool BSA = (WPE == 1);
            const int rl = lane < N ? lane : 0; // this lane's row of R
            double Rr[BSD];
            {
                // chunks of ZC columns, the next chunk's broadcast reads in flight while this one's FMAs issue: the row
                // stays in VGPRs (a 40-column burst buffer pushed half of it into AGPRs, two moves per use)
                constexpr int ZC = JSIM_ZY_CHUNK, NCH = (N + ZC - 1) / ZC;
                double2 dzb[2][ZC / 2], vzb[2][ZC / 2];
#pragma unroll
                for (int j = 0; j < ZC && j < N; j += 2) { dzb[0][j / 2] = *(const double2 *)&dzv[j]; vzb[0][j / 2] = *(const double2 *)&vzv[j]; }
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int h = c * ZC;
                    if (c + 1 < NCH) {
#pragma unroll
                        for (int j = h + ZC; j < h + 2 * ZC && j < N; j += 2) {
                            dzb[(c + 1) & 1][(j - h - ZC) / 2] = *(const double2 *)&dzv[j];
                            vzb[(c + 1) & 1][(j - h - ZC) / 2] = *(const double2 *)&vzv[j];
                        }
                    }
                    if (BSA && c == NCH - 1) { // in flight under this chunk's FMAs
#pragma unroll
                        for (int j = BSA_LO; j < BSD; ++j) Rr[j] = Rm[rl * LD + j];
                    }
                    // (the first chunk was read just above: its waits stay the compiler's, one per pair as the reads come in)
                    if ((CHW & 4) && c > 0) jsim_chunk_wait(c + 1 < NCH ? (h + 2 * ZC < N ? h + 2 * ZC : N) - (h + ZC) : (BSA ? (BSD - BSA_LO) / 2 : 0)); // behind it: the next chunk's d2 and v pairs, or Rr (two entries a read)
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = h; j < h + ZC && j < N; j += 2) {
                        const double2 dz2 = dzb[c & 1][(j - h) / 2], vz2 = vzb[c & 1][(j - h) / 2];
                        z0 = fma(Jr[j], dz2.x, z0); z1 = fma(Jr[j + 1], dz2.y, z1);
                        y0 = fma(Jr[j], vz2.x, y0); y1 = fma(Jr[j + 1], vz2.y, y1);
                    }
                    JSIM_PIN(z0); JSIM_PIN(z1); JSIM_PIN(y0); JSIM_PIN(y1); // consume the chunk HERE (else the FMAs sink to the step update and the whole vector stays live)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const double z = z0 + z1, y = y0 + y1;
            GSTAMP(3);
            // r = R^-1 d1 : back substitution, lane k = row k of R scaled by 1/R[k][k] at load, so one step is
            // r_j = (lane j's running value) ; running -= Rhat[:, j] r_j  -- no masks (zeros below the diagonal / right of
            // column q make the other lanes and steps no-ops).
            //   * columns j >= 16 (blocks 2 and up, entered only while q > 16): two v_readlane bring r_j into a scalar pair, one FMA;
            //   * columns j < 16, always all sixteen: ONE fused FMA whose multiplicand is the running value through the 64-bit
            //     row broadcast (bs_step2 above) -- every 16-lane row receives its own lane j; the consumers of r_j (lanes k < j) sit
            //     in row 0 beside lane j, the lanes of rows 1-3 hold a zero multiplier for these columns (below the diagonal, or
            //     1/R[k][k] = 0 beyond q) and keep their value exactly, as every lane does in a step beyond q.  Same operands in the
            //     same order j = q - 1 .. 0 as the v_readlane form: the same bits.  Their entries of R are on their way or here
            //     (Rr, above), so no LDS round trip stands in front of them, and no branch in front of them either: the compiler
            //     flattens a nest of q > 8k tests into a row of compare-and-branch pairs, ~40 cycles each taken or not, and eight
            //     steps that change nothing cost 20 slots.  (Reading Rr at the top of the iteration and forming the products under
            //     the dots' first reads was measured: 100 cycles less here, 160 more in front of the dots -- DESIGN.md section 6.)
            double rloc = dloc * rdiag;
            {
                constexpr int NB = (N + 7) / 8;
#define BS_BLOCK(blk)                                                                                          \
    {                                                                                                          \
        constexpr int jlo = 8 * (blk), jhi = (8 * (blk) + 7 < N ? 8 * (blk) + 7 : N - 1);                      \
        double Rb[8];                                                                                          \
        _Pragma("unroll") for (int j = jlo; j <= jhi; ++j) Rb[j - jlo] = Rm[rl * LD + j] * rdiag;              \
        _Pragma("unroll") for (int j = jhi; j >= jlo; --j) rloc = fma(-Rb[j - jlo], rdlane(rloc, j), rloc);    \
    }
                // highest block first; a uniform branch costs ~40 cycles taken or not, so the tests are nested
                static_assert(NB > 2 && NB <= 8, "extend the block nest");
                if (q > 16) {
                    if (NB > 3 && q > 24) {
                        if (NB > 4 && q > 32) {
                            if (NB > 5 && q > 40) {
                                if (NB > 6 && q > 48) {
                                    if (NB > 7 && q > 56) BS_BLOCK(7 < NB ? 7 : 0)
                                    BS_BLOCK(6 < NB ? 6 : 0)
                                }
                                BS_BLOCK(5 < NB ? 5 : 0)
                            }
                            BS_BLOCK(4 < NB ? 4 : 0)
                        }
                        BS_BLOCK(3 < NB ? 3 : 0)
                    }
                    BS_BLOCK(2)
                }
#undef BS_BLOCK
                if (BSA) {
#pragma unroll
                    for (int j = 0; j < BSA_LO; ++j) Rr[j] = Rm[rl * LD + j];
                    bs_steps<0, BSD - 1>(rloc, Rr, rdiag);
                } else { // read in place, eight columns at a time
                    double Rb[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) Rb[j] = Rm[rl * LD + 8 + j];
                    bs_steps<8, 7>(rloc, Rb, rdiag);
#pragma unroll
                    for (int j = 0; j < 8; ++j) Rb[j] = Rm[rl * LD + j];
                    bs_steps<0, 7>(rloc, Rb, rdiag);
                }
            }
            GSTAMP(4);
            // dual ratio test: min over the working set of lam_k / r_k (r_k > 0); the step keeps its upper 57 bits and the
            // position k rides in the low 7 (jsim_ratio_pack), so one 64-bit min is the arg-min, ties -> lowest k
            int l;
            double t1;
            {
                double bt = INFINITY;
                {
                    const double tk = jsim_ratio_pack(lam * fast_rcp(rloc), lane); // garbage where rloc <= 0: not selected
                    bt = (lane < q && rloc > 0.0) ? tk : bt;
                }
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
                const double lk = fma(-tstep, rloc, lam);
                lam = lk < 0.0 ? 0.0 : lk;
            }
            lplus += tstep;

            GSTAMP(5);
            if (full) {
                // add p: one Householder reflection on d2; Jhat2 <- Jhat2 (I - beta v v') ; new R column [d1; rho]
                // The search for the NEXT entering row (val and abits are final for this iteration) is dealt out between the
                // chunks of the update, one stage per scheduling region: its DPP / readlane chains wait under the FMAs.
                if (lane == owner) abits |= (1u << obit);
                const double rho = -sg * nrm;
                const double beta = inrm * fast_rcp(nrm + fabs(dq)); // 2 / v'v
                const double w = beta * y;
                if (lane < q) Rm[lane * LD + q] = dloc;
                if (lane == q) { rdv[q] = rho; rdiag = -sg * inrm; actid = p; lam = lplus; }
                {
                    constexpr int ZC = JSIM_ZY_CHUNK, NCH = (N + ZC - 1) / ZC;
                    static_assert(NCH >= 4, "four chunks carry the four stages of the search");
                    constexpr int CB1 = NCH >= 8 ? 2 : 1, CB2 = NCH >= 8 ? 4 : 2, CC_ = NCH >= 8 ? 6 : 3;
                    double2 vzb[2][ZC / 2];
#pragma unroll
                    for (int j = 0; j < ZC && j < N; j += 2) vzb[0][j / 2] = *(const double2 *)&vzv[j];
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const int h = c * ZC;
                        if (c + 1 < NCH) {
#pragma unroll
                            for (int j = h + ZC; j < h + 2 * ZC && j < N; j += 2) vzb[(c + 1) & 1][(j - h - ZC) / 2] = *(const double2 *)&vzv[j];
                        }
                        if ((CHW & 8) && c > 0) jsim_chunk_wait(c + 1 < NCH ? ((h + 2 * ZC < N ? h + 2 * ZC : N) - (h + ZC)) / 2 : 0); // (as in the dots; stage A's two cross-lane reads are in chunk 0)
                        __builtin_amdgcn_sched_barrier(0);
                        if (c == 0) JSIM_SEARCH_A()   // (same scheduling region as this chunk's FMAs)
                        if (c == CB1) JSIM_SEARCH_B1()
                        if (c == CB2) JSIM_SEARCH_B2()
                        if (c == CC_) JSIM_SEARCH_C()
#pragma unroll
                        for (int j = h; j < h + ZC && j < N; j += 2) { // v is zero left of column q
                            Jr[j] = fma(-w, vzb[c & 1][(j - h) / 2].x, Jr[j]);
                            Jr[j + 1] = fma(-w, vzb[c & 1][(j - h) / 2].y, Jr[j + 1]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                ++q;
                LDS_SYNC();
                GSTAMP(6);
            }
            jsim_join_row(Jr); // the drop reads the row as it stands HERE: one register set for J (jsim_mpc.hip; DESIGN.md section 5, fact 7)
            if (full) break;
            // partial step: drop working-set position l (Givens sweep on R in LDS, same rotations on J's columns)
            {
                const int pdrop = __builtin_amdgcn_readlane(actid, l);
                // Rows above l are not rotated, only closed up: columns l + 1 .. q - 1 move one to the left, column q - 1 empties
                // (lane = column offset from l; N <= 62, so one lane per column from l on).
                {
                    const int cA = l + lane;
                    for (int k = 0; k < l; ++k) {
                        const double v = (cA + 1 < q) ? Rm[k * LD + cA + 1] : 0.0;
                        if (cA < q) Rm[k * LD + cA] = v;
                    }
                }
                // Givens sweep, lane = column, row j + 1 of the running sweep carried in registers; every rotated row is written
                // straight to where it ends up, one column to the left (the lane behind the last column writes the zero that
                // empties column q - 1).
                {
                    double x1 = Rm[l * LD + lane];
                    double x2 = (l + 1 < q) ? Rm[(l + 1) * LD + lane] : 0.0;
                    double b = rdv[l + 1 < N ? l + 1 : 0];
                    for (int j = l; j + 1 < q; ++j) {
                        const int jn = (j + 2 < q) ? j + 2 : j + 1;
                        const double x3 = Rm[jn * LD + lane], bn = rdv[jn];
                        const double a = rdlane(x1, j + 1);
                        const double h2 = fma(a, a, b * b);
                        const double ih = fast_rsqrt(h2 > 1e-300 ? h2 : 1e-300);
                        const double hh = h2 * ih;
                        double c = 1.0, s = 0.0;
                        if (hh > 0.0) { c = a * ih; s = b * ih; }
                        const double n1 = fma(c, x1, s * x2);
                        if (lane >= j + 2 && lane <= q) Rm[j * LD + lane - 1] = (lane < q) ? n1 : 0.0;
                        x1 = fma(-s, x1, c * x2);
                        if (lane == 0) { gsv[2 * j] = c; gsv[2 * j + 1] = s; rdv[j] = hh; }
                        x2 = x3; b = bn;
                    }
                    if (lane == 0) Rm[(q - 1) * LD + q - 1] = 0.0;
                    LDS_SYNC();
                }
                // The same rotations on J's columns.  Only rotations l .. q - 2 are not identities: blocks of eight that lie outside
                // are skipped (uniform branch), inside a block identity (c = 1, s = 0) = exact no-op.
#pragma unroll
                for (int h = 0; h + 1 < N; h += 8) {
                    if (h <= q - 2 && h + 7 >= l) {
                        double2 csb[8];
#pragma unroll
                        for (int j = h; j < h + 8 && j + 1 < N; ++j) csb[j - h] = *(const double2 *)&gsv[2 * j];
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int j = h; j < h + 8 && j + 1 < N; ++j) {
                            const double2 cs2 = csb[j - h];
                            const double x1 = Jr[j], x2 = Jr[j + 1];
                            Jr[j] = fma(cs2.x, x1, cs2.y * x2);
                            Jr[j + 1] = fma(-cs2.y, x1, cs2.x * x2);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                {
                    // (a cross-lane read from a lane that EXEC masks off does not return that lane's value: the exchange is pinned
                    // where it stands, with every lane active, ahead of the masked assignment -- cf. compiler fact 4 in DESIGN.md)
                    double lam_n = __shfl_down(lam, 1);
                    int act_n = __shfl_down(actid, 1);
                    asm volatile("" : "+v"(lam_n), "+v"(act_n));
                    if (lane >= l && lane + 1 < q) {
                        lam = lam_n;
                        actid = act_n;
                        rdiag = fast_rcp(rdv[lane]);
                    }
                    if (lane == q - 1) { rdiag = 0.0; lam = 0.0; actid = -1; }
                    JSIM_PIN_WS(lam, rdiag, actid);
                }
                if (lane >= l && lane + 1 < q) { gsv[2 * lane] = 1.0; gsv[2 * lane + 1] = 0.0; }
                --q;
                {
                    int downer, dbit;
                    if (pdrop < 2 * T - 2) { downer = 2 * (pdrop >> 1) + 1; dbit = (pdrop & 1) ? 3 : 2; }
                    else if (pdrop < 3 * T - 1) { downer = VS ? 2 * (pdrop - (2 * T - 2) - 1) : N + pdrop - (2 * T - 2); dbit = VS ? 2 : 0; }
                    else if (pdrop < 4 * T) { downer = VS ? 2 * (pdrop - (3 * T - 1) - 1) : N + pdrop - (3 * T - 1); dbit = VS ? 3 : 1; }
                    else if (pdrop < 5 * T) { downer = 2 * (pdrop - 4 * T); dbit = 0; }
                    else if (pdrop < 6 * T) { downer = 2 * (pdrop - 5 * T); dbit = 1; }
                    else { downer = 2 * ((pdrop - 6 * T) >> 1) + 1; dbit = ((pdrop - 6 * T) & 1) ? 1 : 0; }
                    if (lane == downer) abits &= ~(1u << dbit);
                }
                LDS_SYNC();
                GSTAMP(7);
            }
        }
        if (failed) { status = JSIM_INFEASIBLE; break; }
    }
#undef JSIM_SEARCH
#undef JSIM_SEARCH_A
#undef JSIM_SEARCH_B1
#undef JSIM_SEARCH_B2
#undef JSIM_SEARCH_C

    STAMP(10);
#ifdef JSIM_STAMPS
    if (P.dbg_clk && lane == 0)
        for (int i_ = 0; i_ < 8; ++i_) P.dbg_clk[(size_t)P.B * 16 + (size_t)ego * 8 + i_] = gclk[i_];
#endif
    LANE_FENCE();
    // ------------------------------------------------------------------ S5: outputs
    if (status != JSIM_OK) {
        if (tl) { P.oa[(size_t)ego * T + lane] = 0.0; P.od[(size_t)ego * T + lane] = 0.0; }
        wa_t = 0.0; wd_t = 0.0; wtan = 0.0; s0 = tind;
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = 0u;
        if (lane == 0) {
            P.status[ego] = status;
            P.target_ind[ego] = tind;
            if (P.n_iter) P.n_iter[ego] = it_base + iters;
        }
        it_sum += (unsigned)iters;
        break;
    }
    if (lane < MW) maskw[lane] = 0u;
    if (lane < (VS ? N : NR)) uvec[lane] = val;
    if (VS) { // predicted speeds: v_0 and the prefix sums of the FINAL accelerations
        const bool evl = lane < N && !(lane & 1);
        const double vsp = fma(dt, wincscan_dpp(evl ? val : 0.0, lane), sv);
        if (evl) uvec[N + (lane >> 1) + 1] = vsp;
        if (lane == 0) uvec[N] = sv;
    }
    if constexpr (NB) if (K.advance && tk + 1 < K.n_ticks && P.pass == 0 && !P.dbg_xbar) {
        // The new solution stands in LDS: the helpers start on the next tick (HB_NEXT) under the outputs and the tail below.  The
        // position and speed the plant step will reach need no tan; the yaw does, and helper 1 steps it from what this tick started with.
        double nx = sx, ny = sy, nv = sv, nyaw_ = syaw;
        jsim_plant_step(nx, ny, nv, nyaw_, p_cs, syaw == 0.0 ? syaw : p_sn, 0.0, rdlane(val, 0), P, dt);
        const long long nlen = M - tind;
        if (lane == 0) {
            hb_xy[0] = nx; hb_xy[1] = ny; hb_st[0] = nv; hb_st[NB ? 1 : 0] = sv; hb_st[NB ? 2 : 0] = syaw;
            hb_s0 = tind; hb_ilen = nlen >= 3 ? (int)nlen : 0; hb_cmd = HB_NEXT;
        }
        __syncthreads();
        nb_pending = true; nb_valid = true;
    }
    if (P.dbg_lam)
        for (int e = lane; e < 8 * T; e += 64) P.dbg_lam[(size_t)ego * 8 * T + e] = 0.0;
    LDS_SYNC();
    {
        const double thr = JSIM_ACT_TOL * fmax(1.0, gmax);
        if (lane < q) {
            if (lam > thr) atomicOr(&maskw[actid >> 5], 1u << (actid & 31));
            if (P.dbg_lam) P.dbg_lam[(size_t)ego * 8 * T + actid] = lam;
        }
        LDS_SYNC();
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = maskw[lane];
    }
    {
        double a = 0.0, dl_ = 0.0;
        if (tl) { a = uvec[2 * lane]; dl_ = uvec[2 * lane + 1]; }
        const double vt = lane <= T ? uvec[N + lane] : sv; // tracked speed row = v0 + dt * sum_{s<t} a_s
        if (PARK && lane <= T) {
            al = tq[TQ_QXX * TP + lane]; be = tq[TQ_QXY * TP + lane]; alp = tq[TQ_QYY * TP + lane];
            bep = tq[TQ_QV * TP + lane]; ccx = tq[TQ_QYAW * TP + lane]; ccy = tq[TQ_QEX * TP + lane]; kt = tq[TQ_KT * TP + lane];
        }
        const double yt = syaw + wexscan_dpp(kt * dl_, lane);
        const double xt = sx + wexscan_dpp(fma(al, vt, fma(be, yt, ccx)), lane);
        const double yy = sy + wexscan_dpp(fma(alp, vt, fma(bep, yt, ccy)), lane);
        if (tl) { P.oa[(size_t)ego * T + lane] = a; P.od[(size_t)ego * T + lane] = dl_; }
        wa_t = a; wd_t = dl_; s0 = tind; // next tick's warm start / remembered index
        if (K.advance || tk + 1 < K.n_ticks) { // .. and its tan, for the plant step below (lane 0) and the next tick's S2
            double dc = (P.smax < dl_) ? P.smax : dl_;
            dc = (-P.smax > dc) ? -P.smax : dc;
            XSTAMP_USE("v"(dc));
            XSTAMP0();
            wtan = tan(dc);
            XSTAMP_USE("v"(wtan));
            XSTAMP(1);
        }
        a0n = uvec[0]; d0n = uvec[1];
        if (lane <= T) {
            const size_t o = (size_t)ego * (T + 1) + lane;
            if (P.ox) P.ox[o] = xt;
            if (P.oy) P.oy[o] = yy;
            if (P.ov) P.ov[o] = vt;
            if (P.oyaw) P.oyaw[o] = yt;
        }
    }
    if (lane == 0) {
        P.status[ego] = JSIM_OK;
        P.target_ind[ego] = tind;
        if (P.n_iter) P.n_iter[ego] = it_base + iters;
    }
    it_sum += (unsigned)iters;
    STAMP(11);
#ifdef JSIM_STAMPS
    if (P.dbg_clk && lane == 0) P.dbg_clk[(size_t)ego * 16 + 15] = xclk;
#endif
    } while (0);
    if (HELP) // an early exit left the helpers waiting for this tick's commands
        for (; hp < 3; ++hp) {
            if (lane0 == 0) hb_cmd = HB_SKIP;
            __syncthreads();
            __syncthreads();
        }

    // ---------------------------------------------------------------- rest of the loop body (jsim_loop_advance)
    if (K.advance) {
        double di = di_prev, ai;
        if (status == JSIM_OK) { di = d0n; ai = a0n; }
        else ai = P.amin;                            // MAX_DECEL, main/lib/mpc.py:298-303
        di_prev = di;
        ai_last = ai;
        if (K.hist && lane == 0) {
            const int k = hist_base + tk;
            if (k < K.hist_cap) { K.hist[((size_t)k * P.B + ego) * 2] = di; K.hist[((size_t)k * P.B + ego) * 2 + 1] = ai; }
        }
        // the recorder's xref deviation: the solve's ox[0], oy[0] is the tick-start pose (sx, sy), target_ind is s0
        if (K.rec && lane == 0 && *K.tick + tk < K.rec_cap) // (the counter is read where it is needed: no register holds it)
            jsim_rec_store_dev(K.rec, *K.tick + tk, P.B, ego,
                               status == JSIM_OK ? jsim_xref_deviation(P.pxy[off + s0], P.pyaw[off + s0], sx, sy) : __builtin_nan(""));
        // Simulation.step (main/lib/simulation.py:35-47)
        double dc = (P.smax < di) ? P.smax : di;
        dc = (-P.smax > dc) ? -P.smax : dc;
        double cy_, sy_;
        if (p_sc) { // S2's own; sin keeps the sign of a zero, which the zeros added to lane 0's yaw lose
            sy_ = syaw == 0.0 ? syaw : p_sn; cy_ = p_cs;
        } else {    // the tick left before S2 (no path, nearest-index anomaly)
            sincos(syaw, &sy_, &cy_);
        }
        double tn_;
        if (status == JSIM_OK) tn_ = rdlane(wtan, 0); // di is this solve's delta_0: S5 has tan(dc) in lane 0
        else tn_ = tan(dc);                           // a failed tick steers with the previous di
        // (jsim_plant_step's operations, in the tail's own text: through the function every one-wave kernel's registers were allocated anew)
        const double xd = sv * cy_, yd = sv * sy_, thd = (sv / P.L) * tn_;
        sx += xd * dt; sy += yd * dt; syaw += thd * dt;
        sv += ai * dt;
        sv = (P.vmax_plant < sv) ? P.vmax_plant : sv;
        sv = (P.vmin > sv) ? P.vmin : sv;
        // MPC.is_goal on the new state (main/lib/mpc.py:314-330) / respawn
        bool isgoal = hypot(sx - goal_xy.x, sy - goal_xy.y) <= K.goal_dis;
        long long df = s0 - M;
        if ((df < 0 ? -df : df) >= 5) isgoal = false;
        const bool done = (isgoal && fabs(sv) <= K.stop_speed) || (age + 1 >= K.max_age);
        if (K.rec && lane == 0) { // the History record: the new state ahead of the respawn
            const int k = *K.tick + tk;
            if (k < K.rec_cap)
                jsim_rec_store(K.rec, K.rec_flags, k, P.B, ego, sx, sy, syaw, sv, di, ai,
                               (status == JSIM_OK ? 0 : JSIM_REC_FAILED) | (isgoal && fabs(sv) <= K.stop_speed ? JSIM_REC_GOAL : 0) |
                                   (age + 1 >= K.max_age ? JSIM_REC_AGE : 0));
        }
        if (done) {
            sx = K.x0_spawn[4 * ego]; sy = K.x0_spawn[4 * ego + 1]; sv = K.x0_spawn[4 * ego + 2]; syaw = K.x0_spawn[4 * ego + 3];
            s0 = K.target_spawn[ego];
            wa_t = 0.0; wd_t = 0.0; wtan = 0.0; di_prev = 0.0; ai_last = 0.0; age = 0;
            if constexpr (NB) nb_valid = false; // (NB: what the helpers prepared belongs to the state that ends here)
            if (PRE) { pre_idx = 0; pre_prev = -1; } // a fresh run: no progress index, no previous truncated path
            if (tl) { P.oa[(size_t)ego * T + lane] = 0.0; P.od[(size_t)ego * T + lane] = 0.0; }
            if (lane == 0) {
                P.target_ind[ego] = s0;
                if (K.n_respawn) atomicAdd(K.n_respawn, 1ull);
            }
        } else {
            age += 1;
        }
    }
    LDS_SYNC(); // LDS scratch is reused by the next tick
    // One read-modify-write per launch and counter: in every tick's S5 each put a wait for all outstanding stores on the owner's path.
    // (In the last tick, not behind the loop: there the two pointers stay live across the loop, and the one-wave kernels then keep
    //  their parameters in spill lanes -- 800 v_readlane more in <15, false, 1, false> -- instead of loading them where a tick uses them.)
    if (tk + 1 >= K.n_ticks && lane == 0) {
        if (K.work) K.work[ego] += it_sum;
        if (K.iters) K.iters[ego] += (unsigned long long)it_sum;
    }
    } // tick loop
    if (HELP) {
        if (lane0 == 0) hb_cmd = HB_EXIT;
        __syncthreads();
    }
    if (K.advance && lane == 0) {
        K.x0w[4 * ego] = sx; K.x0w[4 * ego + 1] = sy; K.x0w[4 * ego + 2] = sv; K.x0w[4 * ego + 3] = syaw;
        K.di_ai[2 * ego] = di_prev;
        K.di_ai[2 * ego + 1] = ai_last;
        K.age[ego] = age;
    }
    if (PRE && lane == 0) {
        Q.traj_idx[ego] = pre_idx;
        Q.prev_len[ego] = pre_prev;
        if (Q.speed_cutoff) Q.cut_io[ego] = pre_cut; else Q.path_len_out[ego] = (int)M;
        Q.col_flag[ego] = pre_col;
        Q.pre_status[ego] = pre_st;
    }
}
