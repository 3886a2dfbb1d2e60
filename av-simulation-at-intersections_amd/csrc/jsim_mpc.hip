// jsim_mpc.hip -- MI355X (gfx950 / CDNA4) batched receding-horizon MPC step + the C-ABI of
// include/jsim_mpc.h.  Hand-written HIP, no CUDA-compat layers.  Compile with -ffp-contract=off:
// stages S1-S3 follow numpy's operation order (integer outputs are bit-exact); where a fused
// multiply-add is wanted it is written as fma().
//
// One wavefront (64 lanes) owns one ego for the whole step:
//   S1  reference window      nearest path point (3 smallest distances, wave arg-min), travel -> idx, gather xref
//                             reference: main/lib/mpc.py:89-112, main/lib/trajectories.py:100-126
//   S2  nonlinear rollout     lane t holds time step t; transcendental work lane-parallel, the three
//                             running sums sequential (same order as the reference's python loop)
//                             reference: main/lib/mpc.py:115-129, main/lib/simulation.py:35-47, main/bicycle/main.py:28-41
//   S3  linearisation         A_t,B_t,C_t coefficients per lane (delta_bar == 0 => v, yaw rows are integrators)
//                             reference: main/lib/mpc.py:61-82
//   S4a condense + Hessian    sensitivities generated on the fly from prefix sums; H = 2 S'QS on the fp64
//                             matrix cores (v_mfma_f64_16x16x4_f64, K = the 4 state components of one time
//                             step), block-triangular zero tiles skipped; g, R, Rd terms on the VALU
//                             reference: main/lib/mpc.py:141-186 (cost), :176-178,189 (dynamics eliminated)
//   S4b exact QP solve        Goldfarb-Idnani dual active set (entering row: largest viol^2 / n'H^-1 n); H -> L (Cholesky) -> J = L^-T and the working
//                             set's R factor live in LDS (lane i owns row i); constraints are evaluated from
//                             their structure (boxes, steer-rate differences, speed = prefix sums of accel)
//                             reference: main/lib/mpc.py:187-199 (constraints; cvxpy->ECOS solve replaced)
//   S5  outputs               predicted states of the linearised model, warm start, target_ind, active mask
//                             reference: main/lib/mpc.py:200-205, 293-303
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "jsim_mpc.h"

#define JSIM_VIOL_TOL 1e-10
// Entering-row key: viol^2 / (n'H^-1 n) with its low 20 mantissa bits cleared (keys closer than 2^-32 relative count as
// tied and go to the lowest canonical row id, < 512).  The register kernels store 511 - id in the lowest 9 of them.
// 20 bits: rows that COINCIDE (v_1 <= speed and a_0 <= MAX_ACCEL when v_0 = speed - MAX_ACCEL * dt) have mathematically equal keys
// whose roundings differ by a few ulps; with 9 cleared bits one such pair in ~100 straddled a truncation boundary and the kernel and
// the oracle entered different rows of the pair (same u*, different but equally valid multipliers).
#define JSIM_KEY_MASK 0xFFFFF
__device__ __forceinline__ double jsim_key_trunc(double k)
{
    return __hiloint2double(__double2hiint(k), __double2loint(k) & ~JSIM_KEY_MASK);
}
// Dual ratio test: a step length keeps its upper 57 bits (the low 7 are cleared; the register kernel stores the
// working-set position there), steps closer than 2^-45 relative are ties -> lowest position.
__device__ __forceinline__ double jsim_ratio_trunc(double t)
{
    return __hiloint2double(__double2hiint(t), __double2loint(t) & ~127);
}
__device__ __forceinline__ double jsim_ratio_pack(double t, int k)
{
    return __hiloint2double(__double2hiint(t), (__double2loint(t) & ~127) | k);
}
__device__ __forceinline__ double jsim_key_pack(double k, int id)
{
    return __hiloint2double(__double2hiint(k), (__double2loint(k) & ~JSIM_KEY_MASK) | (511 - id));
}
#define JSIM_DEP_TOL 1e-18
#define JSIM_ACT_TOL 1e-9
#define JSIM_FEAS_TOL 1e-8

typedef double v4d __attribute__((ext_vector_type(4)));

struct KP {
    int T, n, ld, B;
    int pass; // 0: first linearisation; k >= 1: re-linearisation pass k of MAX_ITER (mpc.py:231): skips egos that failed,
              // takes the travel distances from the previous pass's predicted speeds (P.ov) and accumulates n_iter
    double dt, dl, L, w_perp, w_para;
    double R0, R1, Rd0, Rd1, Qv, Qyaw, Qf0, Qf1, Qf2, Qf3, Re0, Re1; // Qf* already multiplied by T
    double dmax, amax, amin, smax, vmax_plant, vmin, vref_min;
    double jerkw; // acceleration-state variant (main/lib/mpc_jerk.py, n = 2T + 1): jerk_penalty_weight
    const double2 *pxy;
    const double *pyaw;
    const double4 *ptrig; // per path point {cos, sin}(yaw + pi/2), {cos, sin}(yaw): S3's weights (jsim_mpc_set_paths), or NULL (S3 evaluates them)
    const double *pcv;   // per-point speed reference of the mpc_with_speed variant, or NULL (xref[2] = 0, mpc.py:107)
    const int *cv_cut;   // [B] index from which that reference is zeroed, or NULL
    const double *pe;    // [B][JSIM_EGO_CFG_DOUBLES] per-ego weights / limits (jsim_mpc_set_ego_config), or NULL
    const long long *poff;
    const double *x0;
    const int *path_id;
    const int *path_len;
    const double *speed;
    long long *target_ind;
    double *oa, *od, *ox, *oy, *ov, *oyaw, *xref;
    unsigned *amask;
    int *status;
    int *n_iter;
    double *dbg_xbar;
    long long *dbg_idx;
    double *dbg_H, *dbg_g, *dbg_lam;
    long long *dbg_clk; // diagnostic build only (-DJSIM_STAMPS): [B][16] s_memtime stamps at phase boundaries
    int dbg_max_gi;     // diagnostic builds only (-DJSIM_STAMPS / -DJSIM_SPAN, env JSIM_DEBUG_MAX_GI): stop the active-set loop after this many
                        // outer iterations (results are then NOT the optimum); -1 = off
};

// per-ego weights / limits over the launch constants (uniform loads: the row depends on the workgroup only)
template <class KPT>
__device__ __forceinline__ void jsim_apply_ego_cfg(KPT &P, const double *pe, int ego, int T, double dt)
{
    const double *w = pe + (size_t)ego * JSIM_EGO_CFG_DOUBLES;
    P.w_perp = w[0]; P.w_para = w[1]; P.R0 = w[2]; P.R1 = w[3]; P.Rd0 = w[4]; P.Rd1 = w[5]; P.Qv = w[6]; P.Qyaw = w[7];
    P.Qf0 = w[8] * T; P.Qf1 = w[9] * T; P.Qf2 = w[10] * T; P.Qf3 = w[11] * T;
    P.dmax = w[12] * dt; P.amax = w[13]; P.amin = w[14];
}

// MPC.get_current_xref_deviation (main/lib/mpc.py:305-312) from the reference point rp = (cx, cy)[target_ind], its yaw and
// (ox[0], oy[0]).  One definition for jsim_mpc_xref_deviation_goal and the recorder: the same operations in the same order (the
// build contracts nothing, -ffp-contract=off), so every kernel that records it gives that entry's value bit for bit.
__device__ __forceinline__ double jsim_xref_deviation(double2 rp, double ryaw, double ox0, double oy0)
{
    const double yp = ryaw + M_PI / 2;
    const double dx = rp.x - ox0, dy = rp.y - oy0;
    const double a = cos(yp) * dx, c = sin(yp) * dy;
    return sqrt(a * a + c * c);
}

// One History record of jsim_loop_set_recorder, written by one lane: slot k (< cap) of ego b, flags = JSIM_REC_* bits.  The
// deviation goes first, before the plant step (the register kernels would otherwise carry it through the step's sin / cos / tan).
template <class DP>
__device__ __forceinline__ void jsim_rec_store_dev(DP rec, int k, int B, int b, double dev)
{
    rec[7 * ((size_t)k * B + b) + 6] = dev;
}
template <class DP, class IP>
__device__ __forceinline__ void jsim_rec_store(DP rec, IP flags, int k, int B, int b, double x, double y, double yaw, double v,
                                               double di, double ai, int fl)
{
    const size_t r = (size_t)k * B + b;
    rec[7 * r] = x; rec[7 * r + 1] = y; rec[7 * r + 2] = yaw; rec[7 * r + 3] = v;
    rec[7 * r + 4] = di; rec[7 * r + 5] = ai;
    flags[r] = fl;
}

// ---------------------------------------------------------------------------------------------------
// wave-level helpers (64 lanes)
// ---------------------------------------------------------------------------------------------------
// Between two phases of a ONE-wave workgroup that hand data from lane to lane through LDS.  The hardware needs nothing -- a wave's LDS
// operations are carried out in program order -- and the compiler only has to keep that order: a wavefront-scope fence.
// __syncthreads() (rounds 1-2) drops its s_barrier in a 64-thread workgroup but keeps `s_waitcnt lgkmcnt(0)`: every hand-over waited
// for its writes to COMPLETE before the reads were even issued.  (-DJSIM_LDS_SYNC_BARRIER: the old form, for A/B runs.)
#ifdef JSIM_LDS_SYNC_BARRIER
#define LDS_SYNC() __syncthreads()
#else
#define LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#endif

#ifdef JSIM_STAMPS
#define STAMP(i) do { if (P.dbg_clk && lane == 0) P.dbg_clk[(size_t)ego * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#elif defined(JSIM_SPAN) /* only the first and the last stamp of a step: two s_memtime per solve, nothing else changes */
#define STAMP(i) do { if (((i) == 0 || (i) == 11) && P.dbg_clk && lane == 0) P.dbg_clk[(size_t)ego * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ double rdlane(double v, int l)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double uni(double v)
{
    int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni64(long long v)
{
    return ((long long)uni((int)(v >> 32)) << 32) | (long long)(unsigned)uni((int)v);
}

__device__ __forceinline__ double wsum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wmax(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// lexicographic arg-min on (v, id): smaller v, ties -> smaller id
__device__ __forceinline__ void wargmin(double &v, int &id)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        double ov = __shfl_xor(v, o);
        int oi = __shfl_xor(id, o);
        bool take = (ov < v) || (ov == v && oi < id);
        v = take ? ov : v;
        id = take ? oi : id;
    }
}
// arg-max on (v, id): larger v, ties -> smaller id
__device__ __forceinline__ void wargmax(double &v, int &id)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        double ov = __shfl_xor(v, o);
        int oi = __shfl_xor(id, o);
        bool take = (ov > v) || (ov == v && oi < id);
        v = take ? ov : v;
        id = take ? oi : id;
    }
}
// exclusive prefix sum over lanes
__device__ __forceinline__ double wexscan(double v, int lane)
{
    double s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        double t = __shfl_up(s, o);
        if (lane >= o) s += t;
    }
    double e = __shfl_up(s, 1);
    return lane == 0 ? 0.0 : e;
}

// ---------------------------------------------------------------------------------------------------
// the step kernel.  RPL = rows of the n x n factors owned by one lane (n <= 64*RPL).
// ---------------------------------------------------------------------------------------------------
enum { TQ_PA = 0, TQ_PB, TQ_PAP, TQ_PBP, TQ_KT, TQ_QXX, TQ_QXY, TQ_QYY, TQ_QV, TQ_QYAW, TQ_QEX, TQ_QEY,
       TQ_QEV, TQ_QEYAW, TQ_REND, TQ_ONE, TQ_ZERO /* constant rows for the register kernels' operand tables */, TQ_COUNT };

// n = 2T decision variables (2T + 1 with the free acc_0 of the acceleration-state variant); ld = row stride of J / R (odd);
// vectors are sized nv = n rounded up to even so that each stays 16-byte aligned
__host__ __device__ static inline int jsim_nvar(int T, int jerk) { return 2 * T + (jerk ? 1 : 0); }
__host__ __device__ static inline int jsim_ld(int n) { return (n + 1) | 1; }
__host__ __device__ static inline size_t jsim_lds_doubles(int T, int jerk)
{
    const size_t n = (size_t)jsim_nvar(T, jerk), ld = (size_t)jsim_ld((int)n), nv = (n + 1) & ~(size_t)1, tp = (size_t)T + 2;
    //      Jm + Rm (even)           dvec uvec      lamv gsv     rdg  ldg  actv(int)   mask                                   tq
    return ((2 * n * ld + 1) & ~(size_t)1) + nv + (nv + 4) + nv + 2 * nv + nv + nv + nv / 2 + 2 + ((8 * (size_t)T + 31) / 32 + 1) / 2 + 1 +
           TQ_COUNT * tp;
}

// JERK: the acceleration-state variant of main/lib/mpc_jerk.py.  Decision vector z = [u0_0, delta_0, .., u0_{T-1}, delta_{T-1}, acc_0]:
// the state [x, y, v, yaw] responds to the EFFECTIVE accelerations  a~_t = acc_t + u0_t = acc_0 + u0_t + dt * sum_{r<t} u0_r
// (v_{t+1} = v_t + dt acc_t + dt u0_t, acc_{t+1} = acc_t + dt u0_t; :67-78) exactly as the stock model responds to a_t, so the
// state-cost Hessian / gradient are the stock ones in (a~, delta) coordinates, carried to z by  a~ = E z  (suffix sums down
// the a-rows and a-columns); the speed rows become  dt * sum_{s<t} A_s  with  A_s = J[acc_0] + J[2s] + dt * sum_{r<s} J[2r].
template <int RPL, bool JERK>
__global__ __launch_bounds__(64) void mpc_step_kernel(const KP Pin)
{
    KP P = Pin;
    if (Pin.pe && (int)blockIdx.x < Pin.B) jsim_apply_ego_cfg(P, Pin.pe, blockIdx.x, Pin.T, Pin.dt);
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int ego = blockIdx.x;
    if (ego >= P.B) return;
    if (P.pass > 0 && P.status[ego] != JSIM_OK) return; // failed in an earlier pass of this step: the failure stands
    const int it_base = (P.pass > 0 && P.n_iter) ? P.n_iter[ego] : 0;
    const int T = P.T, n = P.n, ld = P.ld, tp = T + 2;
    const int nh = 2 * T;             // inputs (u0 / a, delta) x T; n = nh + 1 with the free acc_0 (JERK)
    const int nv = (n + 1) & ~1;
    const int MW = (8 * T + 31) >> 5;

    double *Jm = lds;
    double *Rm = Jm + (size_t)n * ld;
    double *dvec = lds + (((size_t)2 * n * ld + 1) & ~(size_t)1);
    double *uvec = dvec + nv;         // nv + 4
    double *lamv = uvec + nv + 4;     // nv
    double *gsv = lamv + nv;          // 2nv  Givens (c, s)
    double *rdg = gsv + 2 * nv;       // nv   1 / R[k][k]
    double *ldg = rdg + nv;           // nv   1 / L[k][k]
    int *actv = (int *)(ldg + nv);    // n ints
    unsigned *maskw = (unsigned *)(ldg + nv + nv / 2 + 1);
    double *tq = ldg + nv + nv / 2 + 2 + (MW + 1) / 2 + 1;

    // ------------------------------------------------------------------ inputs (wave-uniform)
    const int pid = P.path_id[ego];
    const long long off = P.poff[pid];
    const long long M = P.path_len[ego];
    const long long s0 = P.target_ind[ego];
    const double sx = P.x0[4 * ego + 0], sy = P.x0[4 * ego + 1], sv = P.x0[4 * ego + 2], syaw = P.x0[4 * ego + 3];
    const double speed = P.speed[ego];
    const double dt = P.dt;

    STAMP(0);
    // ------------------------------------------------------------------ S1: nearest index in direction
    long long tind = s0;
    int status = JSIM_OK;
    {
        long long len = M - s0;
        if (len < 0) len = 0;
        if (M < 1) {
            status = 3;
        } else if (len >= 3) {
            double b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
            int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
            const double2 *pp = P.pxy + off + s0;
            for (int k = lane; k < (int)len; k += 64) {
                double2 p = pp[k];
                double dx = p.x - sx, dy = p.y - sy;
                double d = sqrt(dx * dx + dy * dy); // numpy: sqrt(add.reduce(x*x))
                if (d < b0) { b2 = b1; i2 = i1; b1 = b0; i1 = i0; b0 = d; i0 = k; }
                else if (d < b1) { b2 = b1; i2 = i1; b1 = d; i1 = k; }
                else if (d < b2) { b2 = d; i2 = k; }
            }
            int gi[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double dm = b0;
                int im = i0;
                wargmin(dm, im);
                gi[r] = im;
                if (i0 == im) { b0 = b1; i0 = i1; b1 = b2; i1 = i2; b2 = INFINITY; i2 = 0x7fffffff; }
            }
            int g0 = uni(gi[0]), g1 = uni(gi[1]), g2 = uni(gi[2]);
            int d12 = g1 - g2; d12 = d12 < 0 ? -d12 : d12;
            int d01 = g0 - g1; d01 = d01 < 0 ? -d01 : d01;
            if (d12 == 2) tind = g0 + s0;
            else if (d01 == 1) tind = (g0 > g1 ? g0 : g1) + s0;
            else status = JSIM_NEAREST_ANOMALY;
        } else if (len == 2) {
            tind = s0 + 1;
        }
    }
    if (status != JSIM_OK) { // reference raises: nothing is updated
        if (lane == 0) {
            P.status[ego] = status;
            if (P.n_iter) P.n_iter[ego] = it_base;
        }
        return;
    }

    STAMP(1);
    // ------------------------------------------------------------------ S1: travel -> idx -> xref
    const int tl_idx = lane < T ? lane : T; // lanes > T mirror lane T (keeps loads in range)
    double xr, yr, yawr, vr = 0.0;
    bool rend;
    long long ik;
    {
        double vref = (P.vref_min > sv) ? P.vref_min : sv; // python max(state.v, 10/3.6)
        double cstep = fabs(vref) * dt;
        double trav = cstep;
        if (P.pass == 0) {
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + cstep; // np.cumsum: sequential
        } else { // ov = the previous pass's predicted speeds (mpc.py:232,101)
            const double *ovp = P.ov + (size_t)ego * (T + 1);
            trav = fabs(ovp[0]) * dt;
            for (int j = 1; j <= T; ++j)
                if (j <= tl_idx) trav = trav + fabs(ovp[j]) * dt;
        }
        ik = (long long)rint(trav / P.dl) + tind;
        if (ik > M - 1) ik = M - 1;
        double2 pr = P.pxy[off + ik];
        xr = pr.x; yr = pr.y; yawr = P.pyaw[off + ik];
        rend = (ik == M - 1);
        if (P.pcv) { // mpc_with_speed variant: xref[2] = cv[idx], cv zeroed from the ego's cut-off index on
            const int cut = P.cv_cut ? P.cv_cut[ego] : -1;
            vr = (cut < 0 || ik < cut) ? P.pcv[off + ik] : 0.0;
        }
    }

    // infeasible constant rows x[2,0] <= speed, x[2,0] >= MIN_SPEED (ECOS feasibility tolerance)
    if (speed - sv < -JSIM_FEAS_TOL || sv - P.vmin < -JSIM_FEAS_TOL) status = JSIM_INFEASIBLE;

    STAMP(2);
    // ------------------------------------------------------------------ S2: rollout of the warm start
    const bool tl = lane < T;
    double wa_t = tl ? P.oa[(size_t)ego * T + lane] : 0.0;
    double wd_t = tl ? P.od[(size_t)ego * T + lane] : 0.0;
    double bx = sx, by = sy, bv = sv, bth = syaw, sn, cs;
    {
        double dc = (P.smax < wd_t) ? P.smax : wd_t;   // min(delta, MAX_STEER)
        dc = (-P.smax > dc) ? -P.smax : dc;            // max(.., -MAX_STEER)
        double tan_t = tan(dc);
        double vcur = sv;
        for (int j = 0; j < T; ++j) {
            double aj = rdlane(wa_t, j);
            double vn = vcur + aj * dt;
            vn = (P.vmax_plant < vn) ? P.vmax_plant : vn;
            vn = (P.vmin > vn) ? P.vmin : vn;
            vcur = vn;
            if (lane == j + 1) bv = vn;
        }
        double w = ((bv / P.L) * tan_t) * dt;
        double thcur = syaw;
        for (int j = 0; j < T; ++j) {
            thcur = thcur + rdlane(w, j);
            if (lane == j + 1) bth = thcur;
        }
        sincos(bth, &sn, &cs);
        double ix = (bv * cs) * dt, iy = (bv * sn) * dt;
        double xcur = sx, ycur = sy;
        for (int j = 0; j < T; ++j) {
            xcur = xcur + rdlane(ix, j);
            ycur = ycur + rdlane(iy, j);
            if (lane == j + 1) { bx = xcur; by = ycur; }
        }
    }
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
        // reference: solver reports infeasible -> None outputs; target_ind/xref are still stored (mpc.py:293)
        if (tl) { P.oa[(size_t)ego * T + lane] = 0.0; P.od[(size_t)ego * T + lane] = 0.0; }
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = 0u;
        if (lane == 0) {
            P.status[ego] = status;
            P.target_ind[ego] = tind;
            if (P.n_iter) P.n_iter[ego] = it_base;
        }
        return;
    }

    STAMP(3);
    // ------------------------------------------------------------------ S3: linearisation coefficients (lane t < T)
    double al = 0, be = 0, alp = 0, bep = 0, ccx = 0, ccy = 0, kt = 0;
    if (tl) {
        al = dt * cs;                 // A[0,2]
        be = (-dt * bv) * sn;         // A[0,3]
        alp = dt * sn;                // A[1,2]
        bep = (dt * bv) * cs;         // A[1,3]
        ccx = ((dt * bv) * sn) * bth; // C[0]
        ccy = ((-dt * bv) * cs) * bth; // C[1]
        kt = (dt * bv) / P.L;         // B[3,1] with delta_bar = 0
    }
    {
        // exclusive prefix sums over time: x_t = x0 + sum_{r<t}(al_r v_r + be_r yaw_r + ccx_r)
        double PA = wexscan(al, lane), PB = wexscan(be, lane), PAP = wexscan(alp, lane), PBP = wexscan(bep, lane);
        double FX = sx + wexscan(fma(al, sv, fma(be, syaw, ccx)), lane);
        double FY = sy + wexscan(fma(alp, sv, fma(bep, syaw, ccy)), lane);
        double Qxx = 0, Qxy = 0, Qyy = 0, qv = 0, qyaw = 0;
        if (lane >= 1 && lane <= T) {
            if (!rend) {
                double a1 = yawr + 0.5 * M_PI;
                double c1 = cos(a1), s1 = sin(a1), c2 = cos(yawr), s2 = sin(yawr);
                Qxx = (c1 * c1) * P.w_perp + (c2 * c2) * P.w_para;
                Qxy = (c1 * s1) * P.w_perp + (c2 * s2) * P.w_para;
                Qyy = (s1 * s1) * P.w_perp + (s2 * s2) * P.w_para;
                qv = P.Qv; qyaw = P.Qyaw;
            } else {
                Qxx = P.Qf0; Qyy = P.Qf1; qv = P.Qf2; qyaw = P.Qf3;
            }
        }
        double ex = FX - xr, ey = FY - yr, ev = sv - vr, eyaw = syaw - yawr;
        if (lane <= T + 1) {
            const int t = lane;
            bool in = lane <= T;
            tq[TQ_PA * tp + t] = PA; tq[TQ_PB * tp + t] = PB; tq[TQ_PAP * tp + t] = PAP; tq[TQ_PBP * tp + t] = PBP;
            tq[TQ_KT * tp + t] = kt;
            tq[TQ_QXX * tp + t] = in ? Qxx : 0; tq[TQ_QXY * tp + t] = in ? Qxy : 0; tq[TQ_QYY * tp + t] = in ? Qyy : 0;
            tq[TQ_QV * tp + t] = in ? qv : 0; tq[TQ_QYAW * tp + t] = in ? qyaw : 0;
            tq[TQ_QEX * tp + t] = in ? fma(Qxx, ex, Qxy * ey) : 0;
            tq[TQ_QEY * tp + t] = in ? fma(Qxy, ex, Qyy * ey) : 0;
            tq[TQ_QEV * tp + t] = in ? qv * ev : 0;
            tq[TQ_QEYAW * tp + t] = in ? qyaw * eyaw : 0;
            tq[TQ_REND * tp + t] = (in && rend) ? 1.0 : 0.0;
        }
    }
    LDS_SYNC();

    STAMP(4);
    // ------------------------------------------------------------------ S4a: H = 2 S'QS on the fp64 matrix cores
    // v_mfma_f64_16x16x4_f64: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
    // D[row = (lane>>4) + 4*reg][col = lane&15].  k = state component of time step t; tile columns = 8 time steps.
    {
        const int ntile = (nh + 15) >> 4;
        const int kk = lane >> 4, cc = lane & 15;
        for (int ti = 0; ti < ntile; ++ti) {
            const int ca = 16 * ti + cc;
            const bool va = ca < nh;
            const int sa = va ? (ca >> 1) : (T - 1);
            const bool isda = ca & 1;
            const double kta = tq[TQ_KT * tp + sa];
            const double coefa = va ? (isda ? kta : dt) : 0.0;
            const double pax = isda ? tq[TQ_PB * tp + sa + 1] : tq[TQ_PA * tp + sa + 1];
            const double pay = isda ? tq[TQ_PBP * tp + sa + 1] : tq[TQ_PAP * tp + sa + 1];
            const double c23a = !va ? 0.0 : (kk == 2 ? (isda ? 0.0 : dt) : (kk == 3 ? (isda ? kta : 0.0) : 0.0));
            const double *ptxa = isda ? &tq[TQ_PB * tp] : &tq[TQ_PA * tp];
            const double *ptya = isda ? &tq[TQ_PBP * tp] : &tq[TQ_PAP * tp];
            for (int tj = 0; tj <= ti; ++tj) {
                const int cb = 16 * tj + cc;
                const bool vb = cb < nh;
                const int sb = vb ? (cb >> 1) : (T - 1);
                const bool isdb = cb & 1;
                const double ktb = tq[TQ_KT * tp + sb];
                const double coefb = vb ? (isdb ? ktb : dt) : 0.0;
                const double pbx = isdb ? tq[TQ_PB * tp + sb + 1] : tq[TQ_PA * tp + sb + 1];
                const double pby = isdb ? tq[TQ_PBP * tp + sb + 1] : tq[TQ_PAP * tp + sb + 1];
                const double c23b = !vb ? 0.0 : (kk == 2 ? (isdb ? 0.0 : dt) : (kk == 3 ? (isdb ? ktb : 0.0) : 0.0));
                const double *ptxb = isdb ? &tq[TQ_PB * tp] : &tq[TQ_PA * tp];
                const double *ptyb = isdb ? &tq[TQ_PBP * tp] : &tq[TQ_PAP * tp];
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                for (int t = 8 * ti + 1; t <= T; ++t) { // S_t has no entry in tile ti before t = 8*ti + 1
                    double aval;
                    {
                        const bool v1 = t > sa, v2 = t >= sa + 2;
                        double S0 = v2 ? coefa * (ptxa[t] - pax) : 0.0;
                        double S1 = v2 ? coefa * (ptya[t] - pay) : 0.0;
                        double S23 = v1 ? c23a : 0.0;
                        aval = kk == 0 ? S0 : (kk == 1 ? S1 : S23);
                    }
                    double bval;
                    {
                        const bool v1 = t > sb, v2 = t >= sb + 2;
                        double S0 = v2 ? coefb * (ptxb[t] - pbx) : 0.0;
                        double S1 = v2 ? coefb * (ptyb[t] - pby) : 0.0;
                        double S23 = v1 ? c23b : 0.0;
                        double qxx = tq[TQ_QXX * tp + t], qxy = tq[TQ_QXY * tp + t], qyy = tq[TQ_QYY * tp + t];
                        double q23 = kk == 2 ? tq[TQ_QV * tp + t] : tq[TQ_QYAW * tp + t];
                        bval = kk == 0 ? fma(qxx, S0, qxy * S1) : (kk == 1 ? fma(qxy, S0, qyy * S1) : q23 * S23);
                    }
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aval, bval, acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + kk + 4 * r, col = 16 * tj + cc;
                    if (row < nh && col < nh) {
                        double hv = 2.0 * acc[r];
                        Rm[row * ld + col] = hv;
                        if (ti != tj) Rm[col * ld + row] = hv;
                    }
                }
            }
        }
    }
    LDS_SYNC();

    STAMP(5);
    // g = 2 S'Q(f - xref); [JERK: state-cost terms from (a~, delta) to z coordinates;] then the input cost R / R_end
    // (mpc.py:180-183) and the input-difference cost Rd (mpc.py:186) [and the jerk cost, mpc_jerk.py:190]
    double gmax;
    {
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int i = lane + 64 * rr;
            if (i < nh) {
                const int t = i >> 1, c = i & 1;
                // g_i
                const bool isd = c;
                const double ks = tq[TQ_KT * tp + t];
                const double coef = isd ? ks : dt;
                const double px = isd ? tq[TQ_PB * tp + t + 1] : tq[TQ_PA * tp + t + 1];
                const double py = isd ? tq[TQ_PBP * tp + t + 1] : tq[TQ_PAP * tp + t + 1];
                const double *ptx = isd ? &tq[TQ_PB * tp] : &tq[TQ_PA * tp];
                const double *pty = isd ? &tq[TQ_PBP * tp] : &tq[TQ_PAP * tp];
                const double *q23 = isd ? &tq[TQ_QEYAW * tp] : &tq[TQ_QEV * tp];
                double acc = 0.0;
                for (int tt = t + 1; tt <= T; ++tt) {
                    acc = fma(coef, q23[tt], acc);
                    if (tt >= t + 2) {
                        acc = fma(coef * (ptx[tt] - px), tq[TQ_QEX * tp + tt], acc);
                        acc = fma(coef * (pty[tt] - py), tq[TQ_QEY * tp + tt], acc);
                    }
                }
                dvec[i] = 2.0 * acc;
            }
        }
        if (JERK) {
            LDS_SYNC();
            // rows: H <- E'H.  Lane j walks column j upwards: row u0_t = row a~_t + dt * (sum of the rows a~_{t'}, t' > t); the
            // total is the acc_0 row.  (E: a~_t = acc_0 + u0_t + dt * sum_{r<t} u0_r.)
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int j = lane + 64 * rr;
                if (j < nh) {
                    double S = 0.0;
                    for (int t = T - 1; t >= 0; --t) {
                        const double old = Rm[(2 * t) * ld + j];
                        Rm[(2 * t) * ld + j] = fma(dt, S, old);
                        S += old;
                    }
                    Rm[nh * ld + j] = S;
                }
            }
            // g the same way (lane t: suffix sum over the later time steps)
            double gs = 0.0, gt = 0.0;
            if (lane < T) {
                for (int t = T - 1; t > lane; --t) gs += dvec[2 * t];
                gt = gs + dvec[2 * lane]; // lane 0: the total
            }
            LDS_SYNC();
            if (lane < T) dvec[2 * lane] = fma(dt, gs, dvec[2 * lane]);
            if (lane == 0) dvec[nh] = gt;
            // columns: H <- (E'H) E, lane i walks row i (the new acc_0 row included)
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int i = lane + 64 * rr;
                if (i < n) {
                    double S = 0.0;
                    for (int t = T - 1; t >= 0; --t) {
                        const double old = Rm[i * ld + 2 * t];
                        Rm[i * ld + 2 * t] = fma(dt, S, old);
                        S += old;
                    }
                    Rm[i * ld + nh] = S;
                }
            }
            LDS_SYNC();
        }
        double gl = 0.0;
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int i = lane + 64 * rr;
            if (i < nh) {
                const int t = i >> 1, c = i & 1;
                const double Rt = (tq[TQ_REND * tp + t] != 0.0) ? (c ? P.Re1 : P.Re0) : (c ? P.R1 : P.R0);
                const double rdc = 2.0 * (c ? P.Rd1 : P.Rd0);
                const int nd = (T >= 2) ? ((t == 0 || t == T - 1) ? 1 : 2) : 0;
                double dg = 2.0 * Rt + nd * rdc;
                if (JERK && c == 0 && t + 1 < T) dg += 2.0 * P.jerkw * (dt * dt); // (x[4,t+1] - x[4,t])^2 = (dt u0_t)^2
                Rm[i * ld + i] += dg;
                if (t + 1 < T) Rm[i * ld + i + 2] -= rdc;
                if (t >= 1) Rm[i * ld + i - 2] -= rdc;
            }
            if (i < n) {
                const double gi = dvec[i];
                gl = fmax(gl, fabs(gi));
                if (P.dbg_g) P.dbg_g[(size_t)ego * n + i] = gi;
            }
        }
        gmax = uni(wmax(gl));
    }
    LDS_SYNC();
    if (P.dbg_H) {
        double *Hd = P.dbg_H + (size_t)ego * n * n;
        for (int e = lane; e < n * n; e += 64) {
            int r = e / n, c = e - r * n;
            Hd[e] = (c <= r) ? Rm[r * ld + c] : Rm[c * ld + r];
        }
    }

    STAMP(6);
    // ------------------------------------------------------------------ S4b: Cholesky H = L L' (in place, lower), lane = row
    for (int k = 0; k < n; ++k) {
        double s[RPL];
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int i = lane + 64 * rr;
            s[rr] = (i >= k && i < n) ? Rm[i * ld + k] : 0.0;
        }
        for (int j = 0; j < k; ++j) {
            const double lkj = Rm[k * ld + j];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int i = lane + 64 * rr;
                if (i >= k && i < n) s[rr] = fma(-Rm[i * ld + j], lkj, s[rr]);
            }
        }
        double dkk = (RPL == 1 || k < 64) ? rdlane(s[0], k & 63) : rdlane(s[RPL - 1], k & 63);
        if (!(dkk > 0.0)) dkk = 1e-300; // H is SPD by construction (>= 2 min(R) I)
        const double lkk = sqrt(dkk);
        const double inv = 1.0 / lkk;
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int i = lane + 64 * rr;
            if (i == k) { Rm[k * ld + k] = lkk; ldg[k] = inv; }
            else if (i > k && i < n) Rm[i * ld + k] = s[rr] * inv;
        }
        LDS_SYNC();
    }

    STAMP(7);
    // ------------------------------------------------------------------ J = L^-T : lane r owns row r, J[r][i] = (L^-1)[i][r]
    for (int i = 0; i < n; ++i) {
        double s[RPL];
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) s[rr] = (lane + 64 * rr == i) ? 1.0 : 0.0;
        for (int j = 0; j < i; ++j) {
            const double lij = Rm[i * ld + j];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int r = lane + 64 * rr;
                if (r <= j && r < n) s[rr] = fma(-lij, Jm[r * ld + j], s[rr]);
            }
        }
        const double inv = ldg[i];
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int r = lane + 64 * rr;
            if (r < n) Jm[r * ld + i] = (r <= i) ? s[rr] * inv : 0.0;
        }
    }
    LDS_SYNC();

    STAMP(8);
    // ------------------------------------------------------------------ unconstrained optimum u = -J J' g
    double u[RPL];
    {
        double tc[RPL];
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) tc[rr] = 0.0;
        for (int i = 0; i < n; ++i) {
            const double gi = dvec[i];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int j = lane + 64 * rr;
                if (j < n) tc[rr] = fma(Jm[i * ld + j], gi, tc[rr]);
            }
        }
        LDS_SYNC();
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int j = lane + 64 * rr;
            if (j < n) dvec[j] = tc[rr];
        }
        LDS_SYNC();
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) u[rr] = 0.0;
        for (int j = 0; j < n; ++j) {
            const double tj = dvec[j];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int i = lane + 64 * rr;
                if (i < n) u[rr] = fma(Jm[i * ld + j], tj, u[rr]);
            }
        }
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int i = lane + 64 * rr;
            u[rr] = -u[rr];
            if (i < n) uvec[i] = u[rr];
        }
        if (lane < 4) uvec[n + lane] = 0.0;
        if (lane < MW) maskw[lane] = 0u;
    }
    LDS_SYNC();

    STAMP(9);
    // ------------------------------------------------------------------ Goldfarb-Idnani dual active-set iterations
    // static steepest-edge weights of the entering-row rule, per time lane t: 1 / ||J'n||^2 for the rate rows
    // (J[2t+3] - J[2t+1]), the speed rows (dt * sum_{s<t} J[2s]), the accel rows (J[2t]) and the steer rows (J[2t+1]).
    // Rm (L is dead, R not yet started) is the scratch for the cumulative accel rows.
    double iwD = 1.0, iwV = 1.0, iwA = 1.0, iwS = 1.0;
    {
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int j = lane + 64 * rr;
            if (j < n) {
                double c = 0.0, pj = 0.0;
                const double jt = JERK ? Jm[nh * ld + j] : 0.0;
                for (int ss = 0; ss < T; ++ss) {
                    const double a = Jm[(2 * ss) * ld + j];
                    c += JERK ? jt + a + dt * pj : a; // JERK: A_s = J[acc_0] + J[2s] + dt * sum_{r<s} J[2r]
                    pj += a;
                    Rm[(ss + 1) * ld + j] = c;
                }
            }
        }
        LDS_SYNC();
        const int t = lane;
        if (t <= T) {
            double wD = 0.0, wV = 0.0, wA = 0.0, wS = 0.0;
            for (int j = 0; j < n; ++j) {
                if (t >= 1) { const double c = Rm[t * ld + j]; wV = fma(c, c, wV); }
                if (t < T) {
                    const double ja = Jm[(2 * t) * ld + j], js = Jm[(2 * t + 1) * ld + j];
                    wA = fma(ja, ja, wA); wS = fma(js, js, wS);
                    if (t + 1 < T) { const double e = Jm[(2 * t + 3) * ld + j] - js; wD = fma(e, e, wD); }
                }
            }
            wV *= dt * dt;
            iwD = 1.0 / (wD > 0.0 ? wD : 1.0); iwV = 1.0 / (wV > 0.0 ? wV : 1.0);
            iwA = 1.0 / (wA > 0.0 ? wA : 1.0); iwS = 1.0 / (wS > 0.0 ? wS : 1.0);
        }
        LDS_SYNC();
    }
    int q = 0, iters = 0;
    const int max_iters = 50 * n + 100;
    unsigned abits = 0; // lane t: which of the 8 rows of time step t are in the working set
    for (;;) {
        // ---- step 1: among the violated rows the one with the largest viol^2 / (n'H^-1 n) (ties -> lowest canonical index)
        int p;
        double violp;
        {
            const int t = lane;
            double a = 0.0, dl_ = 0.0, dnext = 0.0;
            if (t < T) { double2 ad = *(const double2 *)&uvec[2 * t]; a = ad.x; dl_ = ad.y; dnext = uvec[2 * t + 3]; }
            double aeff = a; // JERK: the effective acceleration a~_t = acc_0 + u0_t + dt * sum_{r<t} u0_r
            if (JERK) aeff = t < T ? uvec[nh] + a + dt * wexscan(a, lane) : 0.0;
            const double vt = sv + dt * wexscan(aeff, lane);
            double best = 0.0, bviol = 0.0;
            int bid = 0x7fffffff;
#define CONSIDER(valid, bit, viol_expr, habs, id_expr, iw)                               \
    if ((valid) && !(abits & (1u << (bit)))) {                                           \
        const double vv = (viol_expr);                                                   \
        const int id_ = (id_expr);                                                       \
        const double key_ = jsim_key_trunc(vv * vv * (iw));                              \
        if (vv > JSIM_VIOL_TOL * (1.0 + (habs)) && (key_ > best || (key_ == best && id_ < bid))) { best = key_; bid = id_; bviol = vv; } \
    }
            CONSIDER(t + 1 < T, 0, (dnext - dl_) - P.dmax, P.dmax, 2 * t, iwD)
            CONSIDER(t + 1 < T, 1, (dl_ - dnext) - P.dmax, P.dmax, 2 * t + 1, iwD)
            CONSIDER(t >= 1 && t <= T, 2, vt - speed, fabs(speed - sv), 2 * T - 2 + t, iwV)
            CONSIDER(t >= 1 && t <= T, 3, P.vmin - vt, fabs(sv - P.vmin), 3 * T - 1 + t, iwV)
            CONSIDER(t < T, 4, a - P.amax, fabs(P.amax), 4 * T + t, iwA)
            CONSIDER(t < T, 5, P.amin - a, fabs(P.amin), 5 * T + t, iwA)
            CONSIDER(t < T, 6, dl_ - P.smax, P.smax, 6 * T + 2 * t, iwS)
            CONSIDER(t < T, 7, -dl_ - P.smax, P.smax, 6 * T + 2 * t + 1, iwS)
#undef CONSIDER
            const int mybid = bid;
            wargmax(best, bid);
            p = uni(bid);
            // the violation of the winner: held by the one lane whose candidate won
            violp = uni(wsum(mybid == p && p != 0x7fffffff ? bviol : 0.0));
        }
        if (p == 0x7fffffff) break; // optimal

        // decode row p
        int kind, tp_, neg = 0;
        if (p < 2 * T - 2) { kind = 0; tp_ = p >> 1; neg = p & 1; }
        else if (p < 3 * T - 1) { kind = 1; tp_ = p - (2 * T - 2); }
        else if (p < 4 * T) { kind = 2; tp_ = p - (3 * T - 1); }
        else if (p < 5 * T) { kind = 3; tp_ = p - 4 * T; }
        else if (p < 6 * T) { kind = 4; tp_ = p - 5 * T; }
        else { kind = 5; tp_ = (p - 6 * T) >> 1; neg = (p - 6 * T) & 1; }
        const unsigned pbit = kind == 0 ? (neg ? 2u : 1u) : kind == 1 ? 4u : kind == 2 ? 8u : kind == 3 ? 16u
                              : kind == 4 ? 32u : (neg ? 128u : 64u);
        double lplus = 0.0;
        bool failed = false;

        for (;;) { // ---- step 2
            if (++iters > max_iters) { failed = true; break; }
            // d = J' n+, n+ = -G_p'   (lane j = column j of J)
            double d[RPL];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int j = lane + 64 * rr;
                double dj = 0.0;
                if (j < n) {
                    if (kind == 0) {
                        double e = Jm[(2 * tp_ + 1) * ld + j] - Jm[(2 * tp_ + 3) * ld + j]; // -(J[d_{t+1}] - J[d_t])
                        dj = neg ? -e : e;
                    } else if (kind == 1 || kind == 2) {
                        double s = 0.0, pj = 0.0;
                        const double jt = JERK ? Jm[nh * ld + j] : 0.0;
                        for (int ss = 0; ss < tp_; ++ss) {
                            const double a = Jm[(2 * ss) * ld + j];
                            s += JERK ? jt + a + dt * pj : a;
                            pj += a;
                        }
                        dj = (kind == 1) ? -dt * s : dt * s;
                    } else if (kind == 3) dj = -Jm[(2 * tp_) * ld + j];
                    else if (kind == 4) dj = Jm[(2 * tp_) * ld + j];
                    else dj = neg ? Jm[(2 * tp_ + 1) * ld + j] : -Jm[(2 * tp_ + 1) * ld + j];
                    dvec[j] = dj;
                }
                d[rr] = dj;
            }
            double dd_l = 0.0, zn_l = 0.0;
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int j = lane + 64 * rr;
                const double sq = d[rr] * d[rr];
                dd_l += sq;
                if (j >= q) zn_l += sq;
            }
            const double dd = uni(wsum(dd_l)), zn = uni(wsum(zn_l));
            LDS_SYNC();
            // z = J2 d2 (lane i = row i)
            double z[RPL];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) z[rr] = 0.0;
            for (int j = q; j < n; ++j) {
                const double dj = dvec[j];
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int i = lane + 64 * rr;
                    if (i < n) z[rr] = fma(Jm[i * ld + j], dj, z[rr]);
                }
            }
            // r = R^-1 d1 (back substitution; lane k = row k of R)
            double r[RPL];
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) r[rr] = d[rr];
            for (int j = q - 1; j >= 0; --j) {
                const double rj = ((RPL == 1 || j < 64) ? rdlane(r[0], j & 63) : rdlane(r[RPL - 1], j & 63)) * rdg[j];
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int i = lane + 64 * rr;
                    if (i == j) r[rr] = rj;
                    else if (i < j) r[rr] = fma(-Rm[i * ld + j], rj, r[rr]);
                }
            }
            // dual ratio test
            int l;
            double t1;
            {
                double bt = INFINITY;
                int bk = 0x7fffffff;
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int k = lane + 64 * rr;
                    if (k < q && r[rr] > 0.0) {
                        double tk = jsim_ratio_trunc(lamv[k] / r[rr]);
                        if (tk < bt) { bt = tk; bk = k; }
                    }
                }
                wargmin(bt, bk);
                t1 = uni(bt);
                l = uni(bk);
            }
            const bool dependent = !(zn > JSIM_DEP_TOL * dd);
            double t2 = dependent ? INFINITY : violp / zn;
            if (t2 < 0.0) t2 = 0.0;
            if (isinf(t1) && isinf(t2)) { failed = true; break; }
            const bool full = (t2 <= t1);
            const double tstep = full ? t2 : t1;
#pragma unroll
            for (int rr = 0; rr < RPL; ++rr) {
                const int i = lane + 64 * rr;
                if (!dependent && i < n) { u[rr] = fma(tstep, z[rr], u[rr]); uvec[i] = u[rr]; }
                if (i < q) {
                    double lk = fma(-tstep, r[rr], lamv[i]);
                    lamv[i] = lk < 0.0 ? 0.0 : lk;
                }
            }
            lplus += tstep;

            if (full) {
                // add p: one Householder reflection on d2; J2 <- J2 P ; new R column [d1; rho]
                const double nrm = sqrt(zn);
                const double dq = (RPL == 1 || q < 64) ? rdlane(d[0], q & 63) : rdlane(d[RPL - 1], q & 63);
                const double sg = dq >= 0.0 ? 1.0 : -1.0;
                const double rho = -sg * nrm;
                const double v0 = dq + sg * nrm;
                const double beta = 1.0 / (nrm * (nrm + fabs(dq)));
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int i = lane + 64 * rr;
                    if (i < n) {
                        const double w = beta * fma(sg * nrm, Jm[i * ld + q], z[rr]);
                        Jm[i * ld + q] = fma(-w, v0, Jm[i * ld + q]);
                        for (int j = q + 1; j < n; ++j) Jm[i * ld + j] = fma(-w, dvec[j], Jm[i * ld + j]);
                    }
                    if (i < q) Rm[i * ld + q] = d[rr];
                    if (i == q) { Rm[q * ld + q] = rho; rdg[q] = 1.0 / rho; actv[q] = p; lamv[q] = lplus; }
                }
                if (lane == tp_) abits |= pbit;
                ++q;
                LDS_SYNC();
                break;
            }
            // partial step: drop working-set position l
            {
                const int pdrop = actv[l];
                // Givens sweep on R (lane k = column k), coefficients kept for the J pass
                for (int j = l; j + 1 < q; ++j) {
                    const double a = Rm[j * ld + j + 1], b = Rm[(j + 1) * ld + j + 1];
                    const double hh = sqrt(a * a + b * b);
                    double c = 1.0, s = 0.0;
                    if (hh > 0.0) { c = a / hh; s = b / hh; }
#pragma unroll
                    for (int rr = 0; rr < RPL; ++rr) {
                        const int k = lane + 64 * rr;
                        if (k >= j + 1 && k < q) {
                            const double x1 = Rm[j * ld + k], x2 = Rm[(j + 1) * ld + k];
                            Rm[j * ld + k] = fma(c, x1, s * x2);
                            Rm[(j + 1) * ld + k] = fma(-s, x1, c * x2);
                        }
                    }
                    if (lane == 0) { gsv[2 * j] = c; gsv[2 * j + 1] = s; }
                    LDS_SYNC();
                }
                // same rotations on the columns of J (lane i = row i, carried column)
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int i = lane + 64 * rr;
                    if (i < n) {
                        double carry = Jm[i * ld + l];
                        for (int j = l; j + 1 < q; ++j) {
                            const double nx = Jm[i * ld + j + 1];
                            const double c = gsv[2 * j], s = gsv[2 * j + 1];
                            Jm[i * ld + j] = fma(c, carry, s * nx);
                            carry = fma(-s, carry, c * nx);
                        }
                        Jm[i * ld + q - 1] = carry;
                    }
                }
                // shift R's columns, the working-set list and the multipliers left
                int an[RPL];
                double ln[RPL];
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int k = lane + 64 * rr;
                    if (k < q) {
                        for (int j = (k > l ? k : l); j + 1 < q; ++j) Rm[k * ld + j] = Rm[k * ld + j + 1];
                    }
                    an[rr] = (k >= l && k + 1 < q) ? actv[k + 1] : 0;
                    ln[rr] = (k >= l && k + 1 < q) ? lamv[k + 1] : 0.0;
                }
                LDS_SYNC();
#pragma unroll
                for (int rr = 0; rr < RPL; ++rr) {
                    const int k = lane + 64 * rr;
                    if (k >= l && k + 1 < q) { actv[k] = an[rr]; lamv[k] = ln[rr]; rdg[k] = 1.0 / Rm[k * ld + k]; }
                }
                --q;
                // clear the dropped row's working-set bit on its time lane
                {
                    int dk, dt_, dneg = 0;
                    if (pdrop < 2 * T - 2) { dk = 0; dt_ = pdrop >> 1; dneg = pdrop & 1; }
                    else if (pdrop < 3 * T - 1) { dk = 1; dt_ = pdrop - (2 * T - 2); }
                    else if (pdrop < 4 * T) { dk = 2; dt_ = pdrop - (3 * T - 1); }
                    else if (pdrop < 5 * T) { dk = 3; dt_ = pdrop - 4 * T; }
                    else if (pdrop < 6 * T) { dk = 4; dt_ = pdrop - 5 * T; }
                    else { dk = 5; dt_ = (pdrop - 6 * T) >> 1; dneg = (pdrop - 6 * T) & 1; }
                    const unsigned dbit = dk == 0 ? (dneg ? 2u : 1u) : dk == 1 ? 4u : dk == 2 ? 8u : dk == 3 ? 16u
                                          : dk == 4 ? 32u : (dneg ? 128u : 64u);
                    if (lane == dt_) abits &= ~dbit;
                }
                LDS_SYNC();
                // violation of p at the new point
                if (kind == 0) {
                    double e = uvec[2 * tp_ + 3] - uvec[2 * tp_ + 1];
                    violp = (neg ? -e : e) - P.dmax;
                } else if (kind == 1 || kind == 2) {
                    double a = (lane < tp_) ? uvec[2 * lane] : 0.0;
                    if (JERK) {
                        const double u0 = lane < T ? uvec[2 * lane] : 0.0;
                        a = (lane < tp_) ? uvec[nh] + u0 + dt * wexscan(u0, lane) : 0.0;
                    }
                    double vt = sv + dt * uni(wsum(a));
                    violp = (kind == 1) ? vt - speed : P.vmin - vt;
                } else if (kind == 3) violp = uvec[2 * tp_] - P.amax;
                else if (kind == 4) violp = P.amin - uvec[2 * tp_];
                else violp = (neg ? -uvec[2 * tp_ + 1] : uvec[2 * tp_ + 1]) - P.smax;
            }
        }
        if (failed) { status = JSIM_INFEASIBLE; break; }
    }

    STAMP(10);
    // ------------------------------------------------------------------ S5: outputs
    if (status != JSIM_OK) {
        if (tl) { P.oa[(size_t)ego * T + lane] = 0.0; P.od[(size_t)ego * T + lane] = 0.0; }
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = 0u;
        if (lane == 0) {
            P.status[ego] = status;
            P.target_ind[ego] = tind;
            if (P.n_iter) P.n_iter[ego] = it_base + iters;
        }
        return;
    }
    {
        const double thr = JSIM_ACT_TOL * fmax(1.0, gmax);
        if (P.dbg_lam) {
            for (int e = lane; e < 8 * T; e += 64) P.dbg_lam[(size_t)ego * 8 * T + e] = 0.0;
            LDS_SYNC(); // drains the zero fill (vmcnt) before other lanes store multipliers to the same words
        }
#pragma unroll
        for (int rr = 0; rr < RPL; ++rr) {
            const int k = lane + 64 * rr;
            if (k < q) {
                const double lk = lamv[k];
                const int id = actv[k];
                if (lk > thr) atomicOr(&maskw[id >> 5], 1u << (id & 31));
                if (P.dbg_lam) P.dbg_lam[(size_t)ego * 8 * T + id] = lk;
            }
        }
        LDS_SYNC();
        if (P.amask && lane < MW) P.amask[(size_t)ego * MW + lane] = maskw[lane];
    }
    {
        double a = 0.0, dl_ = 0.0;
        if (tl) { double2 ad = *(const double2 *)&uvec[2 * lane]; a = ad.x; dl_ = ad.y; }
        // predicted states of the linearised model at u* (= the cvxpy x variable)
        double aeff = a;
        if (JERK) aeff = tl ? uvec[nh] + a + dt * wexscan(a, lane) : 0.0;
        const double vt = sv + dt * wexscan(aeff, lane);
        const double yt = syaw + wexscan(kt * dl_, lane);
        const double xt = sx + wexscan(fma(al, vt, fma(be, yt, ccx)), lane);
        const double yy = sy + wexscan(fma(alp, vt, fma(bep, yt, ccy)), lane);
        if (tl) { P.oa[(size_t)ego * T + lane] = a; P.od[(size_t)ego * T + lane] = dl_; }
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
    STAMP(11);
}

// Both register kernels (mpc_step_reg.inc, mpc_step_reg4.inc) pass a lane's row of J through this where the add of an active-set
// iteration rejoins the path to the drop: the drop then reads THIS value, not the one the iteration started with.  The compiler lays
// the two branches out one behind the other (add ; join ; drop); were the drop to read the start-of-iteration row, that row would
// stay live across the add's FMAs, their results would need a second register set, and the bottom of the loop a copy per column to
// bring them back (compiler fact 7).  One empty asm per column: no instruction.
template <int N>
__device__ __forceinline__ void jsim_join_row(double (&row)[N])
{
#pragma unroll
    for (int j = 0; j < N; ++j) asm volatile("" : "+v"(row[j]));
}

#include "mpc_step_reg.inc"
#include "reg_common.inc"
#include "mpc_step_reg4.inc"

#include "reg_variants.h"

// ---- Split build (build.py's default: one translation unit per horizon, compiled in parallel -- 3 minutes of one core otherwise).
// -DJSIM_KERNEL_TU=<T>: this file up to here plus the explicit instantiations of horizon T's rows of reg_variants.h, nothing else.
// -DJSIM_SPLIT_BUILD  : the rest of the library, with every row declared `extern template` (their host stubs and code objects come
//                       from the kernel translation units).  Neither: everything in one unit.
#define JSIM_REG_KERNEL_1(T, PRE, WPE, HELP) mpc_step_reg_kernel<T, PRE, WPE, HELP>
#define JSIM_REG_KERNEL_4(T, PRE, WPE, HELP) mpc_step_reg4_kernel<T, PRE>
#define JSIM_REG_KERNEL(W, T, PRE, WPE, HELP) JSIM_CAT(JSIM_REG_KERNEL_, W)(T, PRE, WPE, HELP)
#define JSIM_REG_ARGS const KP, const TickP, const PreK
#if defined(JSIM_KERNEL_TU)
#define JSIM_X(w, t, p, e, h) + (t == JSIM_KERNEL_TU)
#if (0 JSIM_REG_VARIANTS(JSIM_X)) == 0
#error "JSIM_KERNEL_TU: not a horizon with a register kernel"
#endif
#undef JSIM_X
#define JSIM_X(w, t, p, e, h) template __global__ void JSIM_REG_KERNEL(w, t, p, e, h)(JSIM_REG_ARGS);
JSIM_CAT(JSIM_REG_ROW_, JSIM_KERNEL_TU)(JSIM_X)
#undef JSIM_X
#else /* !JSIM_KERNEL_TU: the library proper */
#if defined(JSIM_SPLIT_BUILD)
#define JSIM_X(w, t, p, e, h) extern template __global__ void JSIM_REG_KERNEL(w, t, p, e, h)(JSIM_REG_ARGS);
JSIM_REG_VARIANTS(JSIM_X)
#undef JSIM_X
#endif

static int device_cu_count()
{
    static int cus[64];   // per device id, 0 = not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cus[dev];
}

static void launch_reg(int T, int B, hipStream_t s, const KP &P, const TickP &K, const PreK *Q = nullptr)
{
    static const PreK none = {};
    static const int w2_min_b = reg_w2_min_b(getenv("JSIM_W2_MIN_B"));
    static const char *const help_env = getenv("JSIM_HELP_MAX_B");
    const RegVariant v = select_reg_variant(T, B, Q != nullptr, reg_help_max_b(help_env, device_cu_count()), w2_min_b);
#define JSIM_X(w, t, p, e, h)                                                                                                    \
    if (v == RegVariant{w, t, p, e, h}) {                                                                                        \
        hipLaunchKernelGGL((JSIM_REG_KERNEL(w, t, p, e, h)), dim3(B), dim3(v.threads()), 0, s, P, K, Q ? *Q : none);             \
        return;                                                                                                                  \
    }
    JSIM_REG_VARIANTS(JSIM_X)
#undef JSIM_X
}

// ---------------------------------------------------------------------------------------------------
// plant update for the per-vehicle loop (Simulation.step, main/lib/simulation.py:35-47) and the
// controller's (di, ai) selection with the failure path (main/lib/mpc.py:298-303)
// ---------------------------------------------------------------------------------------------------
struct PlantP {
    int B, T;
    double dt, L, smax, vmax, vmin, max_decel;
    const double *pe; // per-ego configuration (MAX_DECEL at [14]) or NULL
};

// The three helpers below are written out once more in the tails of the fused kernels (mpc_step_reg.inc, mpc_step_reg4.inc): keep them in step.
// (di, ai) of ego b: the solve's first controls, or after a failed solve the previous steering and a full brake
__device__ __forceinline__ void select_di_ai(const PlantP &P, int b, const int *status, const double *oa, const double *od,
                                             double *di_ai, double &di, double &ai)
{
    const double max_decel = P.max_decel; // (read here: a choice between its address and the ego's row would put P into scratch)
    di = di_ai[2 * b];
    if (status[b] == JSIM_OK) { di = od[(size_t)b * P.T]; ai = oa[(size_t)b * P.T]; }
    else ai = P.pe ? P.pe[(size_t)b * JSIM_EGO_CFG_DOUBLES + 14] : max_decel;
    di_ai[2 * b] = di;
    di_ai[2 * b + 1] = ai;
}

// Simulation.step
__device__ __forceinline__ void simulation_step(const PlantP &P, double di, double ai, double &x, double &y, double &v, double &th)
{
    double dc = (P.smax < di) ? P.smax : di;
    dc = (-P.smax > dc) ? -P.smax : dc;
    const double xd = v * cos(th), yd = v * sin(th), thd = (v / P.L) * tan(dc);
    x += xd * P.dt; y += yd * P.dt; th += thd * P.dt;
    v += ai * P.dt;
    v = (P.vmax < v) ? P.vmax : v;
    v = (P.vmin > v) ? P.vmin : v;
}

// MPC.is_goal (main/lib/mpc.py:314-330) of the state (x, y, v); the goal is the last point of the path given to MPC.__init__
__device__ __forceinline__ bool mpc_is_goal(const double2 *pxy, const long long *poff, int path, int path_len, long long ti,
                                            double x, double y, double v, double goal_dis, double stop_speed)
{
    const double2 g = pxy[poff[path + 1] - 1];
    bool isgoal = hypot(x - g.x, y - g.y) <= goal_dis;
    const long long df = ti - (long long)path_len;
    if ((df < 0 ? -df : df) >= 5) isgoal = false;
    return isgoal && fabs(v) <= stop_speed;
}

__global__ __launch_bounds__(256) void plant_step_kernel(PlantP P, double *x0, const double *oa, const double *od,
                                                         const int *status, double *di_ai)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    double di, ai;
    select_di_ai(P, b, status, oa, od, di_ai, di, ai);
    double x = x0[4 * b], y = x0[4 * b + 1], v = x0[4 * b + 2], th = x0[4 * b + 3];
    simulation_step(P, di, ai, x, y, v, th);
    x0[4 * b] = x; x0[4 * b + 1] = y; x0[4 * b + 2] = v; x0[4 * b + 3] = th;
}

// Closed-loop bookkeeping of the per-vehicle loop for a batch (main/scenarios/mpc_intersection.py:99-163):
// (di, ai) selection + plant step as above, history record, and replacement of finished egos -- the loop's
// `if mpc.is_goal(state): break` (:101) becomes "respawn at the ego's spawn state with a cold controller".
// The recorder of jsim_loop_set_recorder as the kernels see it: rec == NULL records nothing.  The path yaw is for the deviation.
struct RecP {
    double *rec;   // [cap][B][JSIM_REC_FIELDS]
    int *flags;    // [cap][B]
    int cap;
    const double *pyaw;
};

struct LoopP {
    PlantP plant;
    int max_age;
    double goal_dis, stop_speed;
    const double2 *pxy;
    const long long *poff;
};

__global__ __launch_bounds__(256) void loop_advance_kernel(LoopP P, double *x0, double *oa, double *od,
                                                           const int *status, double *di_ai, long long *target_ind,
                                                           const int *path_id, const int *path_len,
                                                           const double *x0_spawn, const long long *target_spawn,
                                                           int *age, double *hist, int *tick, int hist_cap,
                                                           unsigned long long *n_respawn, RecP R)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int B = P.plant.B, T = P.plant.T;
    if (b >= B) return;
    double di, ai;
    select_di_ai(P.plant, b, status, oa, od, di_ai, di, ai);
    if (hist) {
        const int k = *tick; // device tick counter: bumped by a 1-thread kernel after this one (graph-replay safe)
        if (k < hist_cap) { hist[((size_t)k * B + b) * 2] = di; hist[((size_t)k * B + b) * 2 + 1] = ai; }
    }
    double x = x0[4 * b], y = x0[4 * b + 1], v = x0[4 * b + 2], th = x0[4 * b + 3];
    simulation_step(P.plant, di, ai, x, y, v, th);
    const long long ti = target_ind[b];
    const bool goal = mpc_is_goal(P.pxy, P.poff, path_id[b], path_len[b], ti, x, y, v, P.goal_dis, P.stop_speed); // on the new state
    const bool aged = age[b] + 1 >= P.max_age;
    const bool done = goal || aged;
    if (R.rec) { // the History record: state after the plant step, ahead of the respawn; the solve's ox[0], oy[0] is x0's pose
        const int k = *tick;
        if (k < R.cap) {
            const bool ok = status[b] == JSIM_OK;
            const long long off = P.poff[path_id[b]];
            jsim_rec_store_dev(R.rec, k, B, b,
                               ok ? jsim_xref_deviation(P.pxy[off + ti], R.pyaw[off + ti], x0[4 * b], x0[4 * b + 1]) : __builtin_nan(""));
            jsim_rec_store(R.rec, R.flags, k, B, b, x, y, th, v, di, ai,
                           (ok ? 0 : JSIM_REC_FAILED) | (goal ? JSIM_REC_GOAL : 0) | (aged ? JSIM_REC_AGE : 0));
        }
    }
    if (done) {
        x = x0_spawn[4 * b]; y = x0_spawn[4 * b + 1]; v = x0_spawn[4 * b + 2]; th = x0_spawn[4 * b + 3];
        target_ind[b] = target_spawn[b];
        for (int t = 0; t < T; ++t) { oa[(size_t)b * T + t] = 0.0; od[(size_t)b * T + t] = 0.0; }
        di_ai[2 * b] = 0.0; di_ai[2 * b + 1] = 0.0;
        age[b] = 0;
        if (n_respawn) atomicAdd(n_respawn, 1ull);
    } else {
        age[b] += 1;
    }
    x0[4 * b] = x; x0[4 * b + 1] = y; x0[4 * b + 2] = v; x0[4 * b + 3] = th;
}

__global__ void tick_increment_kernel(int *tick) { *tick += 1; }
__global__ void tick_add_kernel(int *tick, int n) { *tick += n; }

// host ticks: this tick's active-set iterations (summed over the linearisation passes) onto the running totals
__global__ __launch_bounds__(256) void iters_add_kernel(int B, const int *n_iter, unsigned long long *iters)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) iters[b] += (unsigned long long)n_iter[b];
}

struct GoalP {
    int B, T;
    double goal_dis, stop_speed;
    const double2 *pxy;
    const double *pyaw;
    const long long *poff;
};

// MPC.get_current_xref_deviation (main/lib/mpc.py:305-312) and MPC.is_goal (:314-330)
__global__ __launch_bounds__(256) void deviation_goal_kernel(GoalP P, const double *x0, const int *path_id,
                                                             const int *path_len, const long long *target_ind,
                                                             const double *ox, const double *oy, double *deviation,
                                                             int *is_goal)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const long long off = P.poff[path_id[b]];
    const long long ti = target_ind[b];
    if (deviation)
        deviation[b] = jsim_xref_deviation(P.pxy[off + ti], P.pyaw[off + ti], ox[(size_t)b * (P.T + 1)], oy[(size_t)b * (P.T + 1)]);
    if (is_goal)
        is_goal[b] = mpc_is_goal(P.pxy, P.poff, path_id[b], path_len[b], ti, x0[4 * b], x0[4 * b + 1], x0[4 * b + 2], P.goal_dis,
                                 P.stop_speed) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------
// A device array the context owns: reserve() only ever grows it (dropping the old contents when it does); freed with the context.
template <class T> struct DevArray {
    T *p = nullptr;
    size_t cap = 0; // elements
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    ~DevArray() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t n, bool *grew = nullptr)
    {
        if (grew) *grew = n > cap;
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, sizeof(T) * n);
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
};

struct jsim_ctx {
    jsim_cfg cfg{};
    int device = 0;
    DevArray<double2> d_pxy;
    DevArray<double> d_pyaw;
    DevArray<double4> d_ptrig;     // [n_points] the path yaws' trig (path_trig_kernel); unallocated under JSIM_PATH_TRIG=0
    DevArray<long long> d_poff;
    int n_paths = 0;
    long long n_points = 0;
    // per-vehicle loop glue (row f1): host copy of the paths, car circle geometry, per-point circle centres, predictions
    double *h_cx = nullptr, *h_cy = nullptr, *h_cyaw = nullptr;
    int have_geom = 0;
    double cc0 = 0, cc1 = 0, col_radius = 0;
    DevArray<double> d_get_all;    // [ticks][n_obs][6]  obstacle get() tuples of a fused scenario run
    DevArray<double2> d_pred_all;  // [ticks][n_obs][n_steps][2]
    DevArray<double4> d_bc_all;    // [ticks][n_obs] bounding circles of the predictions
    DevArray<double4> d_pred_bc;   // [JSIM_MAX_OBS] of the current single-tick prediction
    double occ0 = 0, occ1 = 0, ocol_radius = 0, oL = 0; // the obstacles' circles / wheelbase (jsim_loop_set_obstacle_geometry); default: the ego's
    int have_ogeom = 0;
    // per-vehicle shapes (jsim_loop_set_vehicle_shapes): (cc0, cc1, radius, L) of each scripted vehicle and its (thr, thr_sq)
    // against the egos' radius; n_shapes = 0: none, the global obstacle geometry above holds for all
    DevArray<double4> d_shapes;    // [n_shapes]
    DevArray<double2> d_othr;      // [n_shapes]
    std::vector<double> h_shapes;  // host copy [n_shapes][4] (the thresholds follow jsim_loop_set_geometry)
    int n_shapes = 0;
    // route vehicles (jsim_loop_set_traffic_routes): the table as the obstacle kernels read it; n_routes = 0: none
    DevArray<double4> d_route_pt;  // [points] (x, y, yaw, S)
    DevArray<int> d_route_off;     // [n_routes + 1]
    DevArray<double> d_route_in;   // [3][points] the uploaded x, y, yaw (route_arclen_kernel's input)
    int n_routes = 0;
    DevArray<double4> d_conflict_rows; // [n_obs] (cc_front, cc_rear, thr, thr_sq) of jsim_loop_eval_conflicts' last call with a table
    DevArray<double4> d_gap_rows;      // the same of jsim_loop_eval_gaps' last call with a table
    DevArray<double4> d_headway_rows;  // [n_obs] (cc_front, cc_rear, radius, thr) of jsim_loop_eval_headway's last call with a table
    DevArray<double> d_static_rows;    // [n_rows][JSIM_STATIC_ROW] and
    DevArray<int> d_static_off;        // [n_sets + 1] of jsim_loop_eval_static's last call
    DevArray<double2> d_pcc;
    DevArray<double2> d_pred_cc;
    int pred_n_obs = 0, pred_n_steps = 0;
    // interacting egos (jsim_loop_set_groups, jsim_loop_run_interacting): groups and the egos' own predictions
    DevArray<int> d_group_of, d_group_off; // [group_B], [n_groups + 1]
    std::vector<int> h_group_off;          // host copy (the traffic checks of jsim_loop_run_interacting)
    int group_B = 0, n_groups = 0, group_max = 0;
    int mate_prediction = JSIM_MATE_CONSTANT; // how jsim_loop_run_interacting predicts the group mates (jsim_loop_set_mate_prediction)
    // traffic sets (jsim_loop_set_traffic): ego -> set, set -> its vehicles in the [total] obstacle tables; host copies to validate
    DevArray<int> d_set_of, d_obs_off;     // [traffic_B], [n_sets + 1]
    std::vector<int> h_set_of, h_obs_off;
    int traffic_B = 0, n_sets = 0, traffic_chunk = 0; // traffic_chunk: ticks per fused launch, 0 = from JSIM_TRAFFIC_BUDGET
    // the History recorder (jsim_loop_set_recorder): caller-owned device buffers, rec_cap = 0: none
    double *rec = nullptr, *rec_obs = nullptr;
    int32_t *rec_flags = nullptr;
    int rec_B = 0, rec_cap = 0, rec_n_obs = 0;
    // the plan recorder (jsim_loop_set_plan_recorder): caller-owned device buffers of the recorder's B and cap, plan_oa = NULL: none
    double *plan_oa = nullptr, *plan_od = nullptr;
    int32_t *plan_status = nullptr;
    DevArray<double2> d_ego_cc;   // [B][n_steps][2]
    DevArray<double4> d_ego_bc;    // [B]
    // jsim_loop_eval_cutoffs: the egos' path ids as the glue last took them (caller-owned device array [B], NULL: no glue call yet),
    // the interacting egos' tick-start states and last steering of a chunk, and the carry of a call without one
    const int32_t *glue_path_id = nullptr;
    int glue_B = 0;
    DevArray<double> d_cut_x0, d_cut_di;   // [chunk][B][4], [chunk][B][2]
    DevArray<int> d_cut_carry;             // [B][3]
    DevArray<int> d_fork_rows, d_fork_ticks; // [2][n_rows] (ego, at) of jsim_loop_fork_state's, [n_obs] of jsim_loop_obstacles_at's last call
    DevArray<int> d_ckpt_rows;     // (ego, slot) [2][n_rows], then (vehicle, slot) [2][n_veh] of jsim_loop_checkpoint_load's last call
    DevArray<double> d_pcv;        // speed reference per path point (mpc_with_speed variant) or NULL
    const int *cv_cut = nullptr;   // caller-owned device array [B] or NULL
    size_t lds_bytes = 0;
    const double *d_pe = nullptr;  // per-ego weights / limits (caller-owned device array) or NULL
    void *comm = nullptr;          // ncclComm_t of jsim_comm_init (RCCL), or NULL
    DevArray<int> d_order;         // launch order of the fused closed-loop launches (prepare_launch_order) ..
    DevArray<unsigned> d_work;     // .. and the per-ego iteration count of the previous launch it is derived from
    DevArray<unsigned long long> d_iters; // per-ego running totals of active-set iterations over the closed-loop ticks (jsim_mpc_iter_totals)
    DevArray<int32_t> d_n_iter;           // host ticks without a caller's n_iter: the tick's counts for d_iters
    int order_mode = 0;      // 0: from the environment (default on), 1: on, -1: off (jsim_mpc_set_launch_order)
    int use_reg_kernel = 0;  // 1: register-resident fast path available for this T (and not disabled)
    int dbg_max_gi = 0;
    long long *dbg_clk = nullptr; // diagnostic builds only
    char err[512] = "";
};

static thread_local char g_err[512] = "";

static int fail(jsim_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof(g_err), "%s", buf);
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", buf);
    return code;
}

#define HIP_TRY(ctx, call)                                                                                     \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) return fail(ctx, -5, "%s failed: %s", #call, hipGetErrorString(e_));             \
    } while (0)

// Every entry point that launches, allocates or copies runs on the context's device and leaves the caller's current device
// as it found it (two contexts on different GPUs in one process; a caller whose current device is another one).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess; // a failed hipGetDevice / hipSetDevice: the entry point must not carry on on the caller's device
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
        }
    }
    bool ok() const { return err == hipSuccess; }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

#define JSIM_GUARD_OK(ctx_)                                                                                   \
    do {                                                                                                       \
        if (!dev_guard.ok()) return fail(ctx_, -5, "switching to the context's device failed: %s", hipGetErrorString(dev_guard.err)); \
    } while (0)

// The one-shot calls (route planner, trajectory scoring) take a device id, not a context: it must name a device, and the call
// runs on it under a DeviceGuard
#define JSIM_ON_DEVICE_ID(who_, id_)                                                                           \
    int ndev = 0;                                                                                             \
    HIP_TRY(nullptr, hipGetDeviceCount(&ndev));                                                               \
    if ((id_) < 0 || (id_) >= ndev) return fail(nullptr, -19, "%s: device %d of %d", who_, id_, ndev);       \
    DeviceGuard dev_guard(id_);                                                                                \
    JSIM_GUARD_OK(nullptr)

// The device buffers of a one-shot call: allocated and filled inside the call, freed when it returns, whichever way.  The first
// error is kept and turns every later step into a no-op; result() tells a failed allocation / upload from what came after.
struct DeviceScratch {
    std::vector<void *> owned;
    hipError_t err = hipSuccess;
    bool setup_failed = false; // err comes from alloc() / upload()
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { for (void *q : owned) (void)hipFree(q); }
    bool ok() const { return err == hipSuccess; }
    template <class T> T *alloc(size_t n) // (n = 0: still a valid pointer)
    {
        void *q = nullptr;
        if (!ok()) return nullptr;
        err = hipMalloc(&q, n ? sizeof(T) * n : 8);
        if (!ok()) { setup_failed = true; return nullptr; }
        owned.push_back(q);
        return (T *)q;
    }
    template <class T> const T *upload(const T *host, size_t n)
    {
        T *q = alloc<T>(n);
        if (q && n) { err = hipMemcpy(q, host, sizeof(T) * n, hipMemcpyHostToDevice); setup_failed = !ok(); }
        return ok() ? q : nullptr;
    }
    template <class T> void fill(T *dev, int byte, size_t n) { if (ok() && n) err = hipMemset(dev, byte, sizeof(T) * n); }
    template <class T> void download(T *host, const T *dev, size_t n) { if (ok() && n) err = hipMemcpy(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost); }
    int result(const char *who) const
    {
        if (ok()) return 0;
        if (setup_failed) return fail(nullptr, -12, "%s: device allocation / upload failed", who);
        return fail(nullptr, -5, "%s: %s", who, hipGetErrorString(err));
    }
};

extern "C" int jsim_abi_version(void) { return JSIM_ABI_VERSION; }

extern "C" const char *jsim_last_error(const jsim_ctx *ctx) { return ctx ? ctx->err : g_err; }

extern "C" int jsim_mpc_create(const jsim_cfg *cfg, int device_id, jsim_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, -22, "jsim_mpc_create: null argument");
    if (cfg->T < 1 || cfg->T > JSIM_MAX_T) return fail(nullptr, -22, "jsim_mpc_create: T=%d outside [1, %d]", cfg->T, JSIM_MAX_T);
    if (cfg->max_iter < 1 || cfg->max_iter > 16) return fail(nullptr, -22, "jsim_mpc_create: MAX_ITER=%d (1..16)", cfg->max_iter);
    if (!(cfg->dt > 0) || !(cfg->dl > 0) || !(cfg->L > 0)) return fail(nullptr, -22, "jsim_mpc_create: dt, dl, L must be positive");
    if (!(cfg->R[0] > 0) || !(cfg->R[1] > 0) || !(cfg->R_end[0] > 0) || !(cfg->R_end[1] > 0))
        return fail(nullptr, -22, "jsim_mpc_create: R / R_end must be positive (strict convexity)");
    if (cfg->nx != 4 && cfg->nx != 5) return fail(nullptr, -22, "jsim_mpc_create: NX=%d (4: lib/mpc.py, 5: lib/mpc_jerk.py)", cfg->nx);
    if (cfg->nx == 5 && !(cfg->jerk_weight >= 0)) return fail(nullptr, -22, "jsim_mpc_create: jerk_weight must be >= 0");
    int ndev = 0;
    HIP_TRY(nullptr, hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(nullptr, -19, "jsim_mpc_create: no HIP device");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, -22, "jsim_mpc_create: device %d of %d", device_id, ndev);
    const size_t lds_bytes = jsim_lds_doubles(cfg->T, cfg->nx == 5) * sizeof(double);
    if (lds_bytes > 160 * 1024) return fail(nullptr, -22, "jsim_mpc_create: T=%d needs %zu B of LDS (> 160 KiB)", cfg->T, lds_bytes);
    DeviceGuard dev_guard(device_id);   // the caller's current device is left as it was
    JSIM_GUARD_OK(nullptr);
    // dynamic LDS above the 64 KiB default has to be granted per kernel; done once here so that the step call
    // itself is pure launches (it may be captured into a hipGraph)
    HIP_TRY(nullptr, hipFuncSetAttribute((const void *)mpc_step_kernel<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(nullptr, hipFuncSetAttribute((const void *)mpc_step_kernel<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(nullptr, hipFuncSetAttribute((const void *)mpc_step_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_TRY(nullptr, hipFuncSetAttribute((const void *)mpc_step_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    jsim_ctx *c = new (std::nothrow) jsim_ctx();
    if (!c) return fail(nullptr, -12, "jsim_mpc_create: out of memory");
    c->cfg = *cfg;
    c->device = device_id;
    c->lds_bytes = lds_bytes;
    // register-resident fast path: instantiated for the stock horizon (13) and the benchmark horizon (20);
    // JSIM_FORCE_LDS_KERNEL=1 routes those through the generic LDS-resident kernel too (used by the tests to
    // cover both kernels on the same inputs)
    const char *force = getenv("JSIM_FORCE_LDS_KERNEL");
    c->use_reg_kernel = cfg->nx == 4 && has_reg_kernel(cfg->T) && !(force && force[0] == '1');
    const char *mg = getenv("JSIM_DEBUG_MAX_GI");
    c->dbg_max_gi = mg ? atoi(mg) : -1;
    *out = c;
    return 0;
}

static void free_paths(jsim_ctx *c)
{
    c->d_pxy.release(); c->d_pyaw.release(); c->d_ptrig.release(); c->d_poff.release(); c->d_pcc.release(); c->d_pcv.release();
    delete[] c->h_cx; delete[] c->h_cy; delete[] c->h_cyaw;
    c->h_cx = c->h_cy = c->h_cyaw = nullptr;
    c->n_paths = 0; c->n_points = 0;
}

extern "C" void jsim_mpc_destroy(jsim_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->comm) (void)jsim_comm_destroy(ctx);
    DeviceGuard dev_guard(ctx->device);   // (a failed switch still frees: hipFree takes the pointers' own device)
    free_paths(ctx);
    delete ctx;                           // the device arrays, while the guard still holds the context's device
}

// circle centres of every path point (lib/trajectories.py:11-55 with the two body-axis circles of
// lib/car_dimensions.py:66-79): (cos(yaw) * x_off - sin(yaw) * 0.0) + x, (sin(yaw) * x_off + cos(yaw) * 0.0) + y
static int upload_circle_centres(jsim_ctx *ctx)
{
    const long long N = ctx->n_points;
    if (N <= 0 || !ctx->h_cx) return 0;
    std::vector<double2> h((size_t)2 * N);
    for (long long i = 0; i < N; ++i) {
        const double c = std::cos(ctx->h_cyaw[i]), s = std::sin(ctx->h_cyaw[i]);
        h[2 * i].x = c * ctx->cc0 - s * 0.0 + ctx->h_cx[i];     h[2 * i].y = s * ctx->cc0 + c * 0.0 + ctx->h_cy[i];
        h[2 * i + 1].x = c * ctx->cc1 - s * 0.0 + ctx->h_cx[i]; h[2 * i + 1].y = s * ctx->cc1 + c * 0.0 + ctx->h_cy[i];
    }
    ctx->d_pcc.release();
    HIP_TRY(ctx, ctx->d_pcc.reserve(2 * N));
    HIP_TRY(ctx, hipMemcpy(ctx->d_pcc, h.data(), sizeof(double2) * 2 * N, hipMemcpyHostToDevice));
    return 0;
}

// The trig of S3's tracking weights, once per path table instead of once per tick and lane: the same two sincos calls on the same
// expressions as the register kernels' own (their ptrig == NULL branch), so the table holds their values bit for bit.
__global__ __launch_bounds__(256) void path_trig_kernel(const double *pyaw, double4 *ptrig, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double yawr = pyaw[i];
    const double a1 = yawr + 0.5 * M_PI;
    double c1, s1, c2, s2;
    sincos(a1, &s1, &c1); sincos(yawr, &s2, &c2);
    ptrig[i] = double4{c1, s1, c2, s2};
}

extern "C" int jsim_mpc_set_paths(jsim_ctx *ctx, const double *cx, const double *cy, const double *cyaw,
                                  const int64_t *path_off, int32_t n_paths)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_set_paths: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!cx || !cy || !cyaw || !path_off || n_paths < 1) return fail(ctx, -22, "jsim_mpc_set_paths: bad argument");
    if (path_off[0] != 0) return fail(ctx, -22, "jsim_mpc_set_paths: path_off[0] must be 0");
    for (int i = 0; i < n_paths; ++i)
        if (path_off[i + 1] <= path_off[i]) return fail(ctx, -22, "jsim_mpc_set_paths: path %d is empty", i);
    const long long N = path_off[n_paths];
    free_paths(ctx);
    // resident path table: xy interleaved (one 16-byte load per point in the nearest-index scan) + yaw
    double2 *h = new (std::nothrow) double2[N];
    if (!h) return fail(ctx, -12, "jsim_mpc_set_paths: out of host memory");
    for (long long i = 0; i < N; ++i) { h[i].x = cx[i]; h[i].y = cy[i]; }
    hipError_t e = ctx->d_pxy.reserve(N);
    if (e == hipSuccess) e = ctx->d_pyaw.reserve(N);
    if (e == hipSuccess) e = ctx->d_poff.reserve(n_paths + 1);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_pxy, h, sizeof(double2) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_pyaw, cyaw, sizeof(double) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_poff, path_off, sizeof(long long) * (n_paths + 1), hipMemcpyHostToDevice);
    delete[] h;
    const char *pt = getenv("JSIM_PATH_TRIG");   // "0": no table, the kernels evaluate the trig themselves (A/B and test switch)
    if (e == hipSuccess && !(pt && pt[0] == '0')) {
        e = ctx->d_ptrig.reserve(N);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(path_trig_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, ctx->d_pyaw.p, ctx->d_ptrig.p, N);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
    }
    if (e != hipSuccess) { free_paths(ctx); return fail(ctx, -5, "jsim_mpc_set_paths: %s", hipGetErrorString(e)); }
    ctx->n_paths = n_paths;
    ctx->n_points = N;
    ctx->h_cx = new (std::nothrow) double[N]; ctx->h_cy = new (std::nothrow) double[N]; ctx->h_cyaw = new (std::nothrow) double[N];
    if (!ctx->h_cx || !ctx->h_cy || !ctx->h_cyaw) return fail(ctx, -12, "jsim_mpc_set_paths: out of host memory");
    memcpy(ctx->h_cx, cx, sizeof(double) * N); memcpy(ctx->h_cy, cy, sizeof(double) * N); memcpy(ctx->h_cyaw, cyaw, sizeof(double) * N);
    if (ctx->have_geom) return upload_circle_centres(ctx);
    return 0;
}

// The closed-loop entry points' arguments, packed once per call: jsim_mpc_step's buffers (x0 is written by the advance only,
// path_len by the glue only), jsim_loop_advance's own, and those of the glue and the scripted obstacles (jsim_loop_run_scenario).
struct StepBufs {
    double *x0; const int32_t *path_id, *path_len; const double *speed; int64_t *target_ind;
    double *oa, *od, *ox, *oy, *ov, *oyaw, *xref; uint32_t *active_mask; int32_t *status, *n_iter;
};
struct AdvanceBufs {
    double *di_ai; const double *x0_spawn; const int64_t *target_spawn; int32_t *age, max_age;
    double *hist; int32_t *tick, hist_cap; uint64_t *n_respawn;
};
struct GlueBufs {
    int64_t *traj_idx; int32_t *prev_path_len, *col_flag, *pre_status, frame_window, margin, n_obs;
    double *obs_state; const double *obs_param; double *obs_get; int32_t n_steps, speed_cutoff;
};

static int check_step(jsim_ctx *ctx, const char *fn, const StepBufs &S)
{
    if (!S.x0 || !S.path_id || !S.path_len || !S.speed || !S.target_ind || !S.oa || !S.od || !S.status)
        return fail(ctx, -22, "%s: a required device pointer is null", fn);
    if (!ctx->d_pxy) return fail(ctx, -22, "%s: jsim_mpc_set_paths has not been called", fn);
    if (ctx->cfg.max_iter > 1 && !S.ov)
        return fail(ctx, -22, "%s: MAX_ITER=%d needs the ov buffer (the next pass's travel distances)", fn, ctx->cfg.max_iter);
    return 0;
}

static int check_advance(jsim_ctx *ctx, const char *fn, const AdvanceBufs &A)
{
    if (!A.di_ai || !A.x0_spawn || !A.target_spawn || !A.age) return fail(ctx, -22, "%s: a required device pointer is null", fn);
    if (A.hist && !A.tick) return fail(ctx, -22, "%s: hist needs a device tick counter", fn);
    return 0;
}

// A registered recorder must be the run's: the same B and a device tick counter (its slots); n_obs >= 0: the run's scripted
// vehicles, which a recorder of obstacle tuples must hold
static int check_recorder(jsim_ctx *ctx, const char *fn, int B, const int32_t *tick, int n_obs)
{
    if (!ctx->rec) return 0;
    if (ctx->rec_B != B) return fail(ctx, -22, "%s: the recorder (jsim_loop_set_recorder) is for B=%d, not B=%d", fn, ctx->rec_B, B);
    if (!tick) return fail(ctx, -22, "%s: the recorder needs a device tick counter", fn);
    if (n_obs >= 0 && ctx->rec_obs && ctx->rec_n_obs != n_obs)
        return fail(ctx, -22, "%s: the recorder holds %d vehicles, the run has n_obs=%d", fn, ctx->rec_n_obs, n_obs);
    return 0;
}

static int check_glue(jsim_ctx *ctx, const char *fn, const GlueBufs &G)
{
    if (!G.traj_idx || !G.prev_path_len || !G.col_flag || !G.pre_status) return fail(ctx, -22, "%s: a required device pointer is null", fn);
    if (G.n_obs > 0 && (!G.obs_state || !G.obs_param || !G.obs_get)) return fail(ctx, -22, "%s: null obstacle pointer", fn);
    if (!ctx->d_pxy || !ctx->d_pcc || !ctx->have_geom) return fail(ctx, -22, "%s: paths / geometry not set", fn);
    return 0;
}

static KP fill_kp(const jsim_ctx *ctx, int32_t B, const StepBufs &S)
{
    const jsim_cfg &c = ctx->cfg;
    KP P;
    memset(&P, 0, sizeof(P));
    P.T = c.T; P.n = jsim_nvar(c.T, c.nx == 5); P.ld = jsim_ld(P.n); P.B = B;
    P.jerkw = c.jerk_weight;
    P.dt = c.dt; P.dl = c.dl; P.L = c.L; P.w_perp = c.w_perp; P.w_para = c.w_para;
    P.R0 = c.R[0]; P.R1 = c.R[1]; P.Rd0 = c.Rd[0]; P.Rd1 = c.Rd[1]; P.Qv = c.Q_v_yaw[0]; P.Qyaw = c.Q_v_yaw[1];
    P.Qf0 = c.Qf[0] * c.T; P.Qf1 = c.Qf[1] * c.T; P.Qf2 = c.Qf[2] * c.T; P.Qf3 = c.Qf[3] * c.T; // mpc.py:28
    P.Re0 = c.R_end[0]; P.Re1 = c.R_end[1];
    P.dmax = c.max_dsteer * c.dt; P.amax = c.max_accel; P.amin = c.max_decel; P.smax = c.max_steer;
    P.vmax_plant = c.max_speed; P.vmin = c.min_speed; P.vref_min = c.min_ref_speed;
    P.pxy = ctx->d_pxy; P.pyaw = ctx->d_pyaw; P.ptrig = ctx->d_ptrig; P.poff = ctx->d_poff;
    P.pcv = ctx->d_pcv; P.cv_cut = ctx->cv_cut; P.pe = ctx->d_pe;
    P.x0 = S.x0; P.path_id = S.path_id; P.path_len = S.path_len; P.speed = S.speed;
    P.target_ind = (long long *)S.target_ind; P.oa = S.oa; P.od = S.od; P.ox = S.ox; P.oy = S.oy; P.ov = S.ov; P.oyaw = S.oyaw;
    P.xref = S.xref; P.amask = S.active_mask; P.status = S.status; P.n_iter = S.n_iter;
    P.dbg_clk = ctx->dbg_clk; P.dbg_max_gi = ctx->dbg_max_gi;
    return P;
}

// the largest double x with sqrt(x) <= thr (IEEE sqrt is correctly rounded and monotone): comparing a squared distance with it
// decides exactly what comparing its square root with thr decides
static double jsim_sqrt_threshold(double thr)
{
    double x = thr * thr;
    while (std::sqrt(x) > thr) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= thr) x = std::nextafter(x, INFINITY);
    return x;
}

// the glue's launch constants and the context's tables and single-tick predictions; the per-ego pointers are the caller's
static PreP fill_prep(const jsim_ctx *ctx, int B, int n_obs, int n_steps, int frame_window, int margin)
{
    const jsim_cfg &c = ctx->cfg;
    PreP P;
    memset(&P, 0, sizeof(P));
    P.B = B; P.n_obs = n_obs; P.n_steps = n_steps; P.frame_window = frame_window; P.margin = margin;
    P.dt = c.dt; P.max_accel = c.max_accel; P.max_speed = c.max_speed; P.thr = ctx->col_radius + ctx->ocol_radius; // min_distance: 2 * radius, or car radius + bicycle radius
    P.thr_sq = jsim_sqrt_threshold(P.thr);
    P.pxy = ctx->d_pxy; P.pcc = ctx->d_pcc; P.poff = ctx->d_poff; P.pred_cc = ctx->d_pred_cc; P.pred_bc = ctx->d_pred_bc;
    P.othr = ctx->n_shapes > 0 ? ctx->d_othr.p : nullptr;
    return P;
}

// ---------------------------------------------------------------------------------------------------
// Launch order of the fused closed-loop launches.  A launch ends when its slowest ego does, and with more egos than
// the chip holds at once (1024 one-wave egos at T = 13 / 20 / 30, 512 four-wave egos at T = 40) the workgroups of the
// second round start when a slot frees up: an ego far from its path -- four to five times the mean number of active-set
// iterations per tick, tick after tick -- that starts late ends the launch late.  Workgroups are dispatched in blockIdx
// order, so workgroup b is given ego order[b], the egos ranked by the iterations they needed in the PREVIOUS launch, most
// first (longest-processing-time-first list scheduling).  Egos are independent: the order changes when an ego is solved,
// never what is computed for it.  JSIM_LAUNCH_ORDER=0 in the environment keeps the identity order (A/B runs).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void launch_order_kernel(const unsigned *work, int B, int *order)
{
    __shared__ unsigned tile[1024];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned wi = i < B ? work[i] : 0u;
    int rank = 0; // egos ahead of ego i: more work, or the same work and a lower index (a permutation whatever the values)
    for (int base = 0; base < B; base += 1024) {
        __syncthreads();
        for (int j = threadIdx.x; j < 1024; j += 256) tile[j] = base + j < B ? work[base + j] : 0u;
        __syncthreads();
        const int n = B - base < 1024 ? B - base : 1024;
        for (int j = 0; j < n; ++j) {
            const unsigned wj = tile[j];
            rank += (wj > wi || (wj == wi && base + j < i)) ? 1 : 0;
        }
    }
    if (i < B) order[rank] = i;
}

static int prepare_launch_order(jsim_ctx *ctx, int B, hipStream_t s, TickP &K)
{
    static const int enabled = [] { const char *e = getenv("JSIM_LAUNCH_ORDER"); return !(e && e[0] == '0'); }();
    K.order = nullptr; K.work = nullptr;
    const bool on = ctx->order_mode ? ctx->order_mode > 0 : (bool)enabled;
    if (!on || B < 512 || B > 65536) return 0; // fewer egos than slots: all start at once; beyond: O(B^2) ranking not worth it
    bool grew;
    HIP_TRY(ctx, ctx->d_order.reserve(B));
    HIP_TRY(ctx, ctx->d_work.reserve(B, &grew));
    if (grew) HIP_TRY(ctx, hipMemsetAsync(ctx->d_work, 0, sizeof(unsigned) * (size_t)B, s));
    hipLaunchKernelGGL(launch_order_kernel, dim3((B + 255) / 256), dim3(256), 0, s, ctx->d_work, B, ctx->d_order);
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_work, 0, sizeof(unsigned) * (size_t)B, s));
    K.order = ctx->d_order; K.work = ctx->d_work;
    return 0;
}

// Per-ego running totals of active-set iterations, added to by every closed-loop tick: inside the fused launches (one 8-byte update
// per ego and tick), after each MPC step of run_host_ticks.  Sized on first use, cleared when they grow.
static int prepare_iter_totals(jsim_ctx *ctx, int B, hipStream_t s)
{
    bool grew;
    HIP_TRY(ctx, ctx->d_iters.reserve(B, &grew));
    if (grew) HIP_TRY(ctx, hipMemsetAsync(ctx->d_iters, 0, sizeof(unsigned long long) * (size_t)B, s));
    return 0;
}

extern "C" int jsim_mpc_iter_totals(jsim_ctx *ctx, int32_t B, uint64_t *totals, int32_t reset)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_iter_totals: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B <= 0 || (size_t)B > ctx->d_iters.cap) return fail(ctx, -22, "jsim_mpc_iter_totals: B=%d, but the closed-loop runs of this context had at most %d egos", B, (int)ctx->d_iters.cap);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (totals) HIP_TRY(ctx, hipMemcpy(totals, ctx->d_iters, sizeof(uint64_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(ctx, hipMemset(ctx->d_iters, 0, sizeof(unsigned long long) * ctx->d_iters.cap));
    return 0;
}

extern "C" int jsim_mpc_set_launch_order(jsim_ctx *ctx, int32_t enabled)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_set_launch_order: null ctx");
    ctx->order_mode = enabled ? 1 : -1;
    return 0;
}

extern "C" int jsim_mpc_get_launch_order(jsim_ctx *ctx, int32_t B, int32_t *order, uint32_t *work)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_get_launch_order: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B <= 0 || (size_t)B > ctx->d_work.cap) // (d_work is reserved after d_order)
        return fail(ctx, -22, "jsim_mpc_get_launch_order: B=%d, but the last ordered launch had %d egos", B, (int)ctx->d_work.cap);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (order) HIP_TRY(ctx, hipMemcpy(order, ctx->d_order, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    if (work) HIP_TRY(ctx, hipMemcpy(work, ctx->d_work, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return 0;
}

// MPC.step for the batch: one launch per linearisation pass (_iterative_linear_mpc_control, main/lib/mpc.py:231-236)
static void launch_step(const jsim_ctx *ctx, KP &P, hipStream_t s)
{
    const jsim_cfg &c = ctx->cfg;
    TickP K;
    memset(&K, 0, sizeof(K));
    K.n_ticks = 1; // plain MPC.step: one tick, no plant/bookkeeping
    for (int pass = 0; pass < c.max_iter; ++pass) {
        P.pass = pass;
        if (ctx->use_reg_kernel) launch_reg(c.T, P.B, s, P, K);
        else if (c.nx == 5) {
            if (P.n <= 64) hipLaunchKernelGGL((mpc_step_kernel<1, true>), dim3(P.B), dim3(64), ctx->lds_bytes, s, P);
            else hipLaunchKernelGGL((mpc_step_kernel<2, true>), dim3(P.B), dim3(64), ctx->lds_bytes, s, P);
        } else if (P.n <= 64) hipLaunchKernelGGL((mpc_step_kernel<1, false>), dim3(P.B), dim3(64), ctx->lds_bytes, s, P);
        else hipLaunchKernelGGL((mpc_step_kernel<2, false>), dim3(P.B), dim3(64), ctx->lds_bytes, s, P);
    }
}

extern "C" int jsim_mpc_step(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                             const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa,
                             double *od, double *ox, double *oy, double *ov, double *oyaw, double *xref,
                             uint32_t *active_mask, int32_t *status, int32_t *n_iter, void *stream)
{
    return jsim_mpc_step_debug(ctx, B, x0, path_id, path_len, speed, target_ind, oa, od, ox, oy, ov, oyaw, xref, active_mask,
                               status, n_iter, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int jsim_mpc_step_debug(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                                   const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa,
                                   double *od, double *ox, double *oy, double *ov, double *oyaw, double *xref,
                                   uint32_t *active_mask, int32_t *status, int32_t *n_iter, double *xbar,
                                   int64_t *ref_idx, double *H, double *g, double *lam, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_step: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0) return fail(ctx, -22, "jsim_mpc_step: B=%d", B);
    if (B == 0) return 0;
    const StepBufs S = {const_cast<double *>(x0), path_id, path_len, speed, target_ind, oa, od, ox, oy, ov, oyaw, xref,
                        active_mask, status, n_iter};
    if (int rc = check_step(ctx, "jsim_mpc_step", S)) return rc;
    KP P = fill_kp(ctx, B, S);
    P.dbg_xbar = xbar; P.dbg_idx = (long long *)ref_idx; P.dbg_H = H; P.dbg_g = g; P.dbg_lam = lam;
    launch_step(ctx, P, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

static PlantP plant_p(const jsim_ctx *ctx, int B)
{
    const jsim_cfg &c = ctx->cfg;
    return PlantP{B, c.T, c.dt, c.L, c.max_steer, c.max_speed, c.min_speed, c.max_decel, ctx->d_pe};
}

extern "C" int jsim_plant_step(jsim_ctx *ctx, int32_t B, double *x0, const double *oa, const double *od,
                               const int32_t *status, double *di_ai, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_plant_step: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0) return fail(ctx, -22, "jsim_plant_step: B=%d", B);
    if (B == 0) return 0;
    if (!x0 || !oa || !od || !status || !di_ai) return fail(ctx, -22, "jsim_plant_step: null device pointer");
    hipLaunchKernelGGL(plant_step_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, plant_p(ctx, B), x0, oa, od,
                       status, di_ai);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int jsim_mpc_xref_deviation_goal(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id,
                                            const int32_t *path_len, const int64_t *target_ind, const double *ox,
                                            const double *oy, double *deviation, int32_t *is_goal, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_xref_deviation_goal: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0) return fail(ctx, -22, "jsim_mpc_xref_deviation_goal: B=%d", B);
    if (B == 0) return 0;
    if (!x0 || !path_id || !path_len || !target_ind || (deviation && (!ox || !oy)))
        return fail(ctx, -22, "jsim_mpc_xref_deviation_goal: null device pointer");
    if (!ctx->d_pxy) return fail(ctx, -22, "jsim_mpc_xref_deviation_goal: no paths set");
    const jsim_cfg &c = ctx->cfg;
    GoalP P = {B, c.T, c.goal_dis, c.stop_speed, ctx->d_pxy, ctx->d_pyaw, ctx->d_poff};
    hipLaunchKernelGGL(deviation_goal_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, x0, path_id,
                       path_len, (const long long *)target_ind, ox, oy, deviation, is_goal);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// plant, history, goal / respawn, then the device tick counter
static void launch_advance(const jsim_ctx *ctx, int B, const StepBufs &S, const AdvanceBufs &A, hipStream_t s)
{
    const jsim_cfg &c = ctx->cfg;
    LoopP P = {plant_p(ctx, B), A.max_age > 0 ? A.max_age : 0x7fffffff, c.goal_dis, c.stop_speed, ctx->d_pxy, ctx->d_poff};
    const RecP R = {ctx->rec, ctx->rec_flags, ctx->rec_cap, ctx->d_pyaw};
    hipLaunchKernelGGL(loop_advance_kernel, dim3((B + 255) / 256), dim3(256), 0, s, P, S.x0, S.oa, S.od, S.status, A.di_ai,
                       (long long *)S.target_ind, S.path_id, S.path_len, A.x0_spawn, (const long long *)A.target_spawn, A.age,
                       A.hist, A.tick, A.hist_cap, (unsigned long long *)A.n_respawn, R);
    if (A.tick) hipLaunchKernelGGL(tick_increment_kernel, dim3(1), dim3(1), 0, s, A.tick);
}

extern "C" int jsim_loop_advance(jsim_ctx *ctx, int32_t B, double *x0, double *oa, double *od, const int32_t *status,
                                 double *di_ai, int64_t *target_ind, const int32_t *path_id, const int32_t *path_len,
                                 const double *x0_spawn, const int64_t *target_spawn, int32_t *age, int32_t max_age,
                                 double *hist, int32_t *tick, int32_t hist_cap, uint64_t *n_respawn, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_advance: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0) return fail(ctx, -22, "jsim_loop_advance: B=%d", B);
    if (B == 0) return 0;
    if (!x0 || !oa || !od || !status || !target_ind || !path_id || !path_len)
        return fail(ctx, -22, "jsim_loop_advance: a required device pointer is null");
    const AdvanceBufs A = {di_ai, x0_spawn, target_spawn, age, max_age, hist, tick, hist_cap, n_respawn};
    if (int rc = check_advance(ctx, "jsim_loop_advance", A)) return rc;
    if (int rc = check_recorder(ctx, "jsim_loop_advance", B, tick, -1)) return rc;
    if (!ctx->d_pxy) return fail(ctx, -22, "jsim_loop_advance: no paths set");
    StepBufs S = {}; // (the advance reads status)
    S.x0 = x0; S.path_id = path_id; S.path_len = path_len; S.target_ind = target_ind; S.oa = oa; S.od = od;
    S.status = const_cast<int32_t *>(status);
    launch_advance(ctx, B, S, A, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

#if defined(JSIM_STAMPS) || defined(JSIM_SPAN)
// diagnostic build only (not declared in include/jsim_mpc.h, not built into libjsim_mpc.so)
extern "C" int jsim_debug_set_clock_buffer(jsim_ctx *ctx, long long *dev_buf)
{
    if (!ctx) return -22;
    ctx->dbg_clk = dev_buf;
    return 0;
}
#endif

// ---------------------------------------------------------------------------------------------------
// The job's one exchange: all-gather of the per-rank result blocks over RCCL (xGMI).  Egos are independent
// (main/lib/mpc.py:141-211 couples nothing), so nothing is exchanged on the solve path; this is the final trajectory gather.
// librccl is loaded on first use -- the library itself links only libamdhip64 and single-GPU users never touch RCCL.
// ---------------------------------------------------------------------------------------------------
struct JsimNcclId { char internal[128]; }; // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed by value like the original
namespace {
struct RcclApi {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, JsimNcclId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
}
static RcclApi g_rccl;

static int rccl_load(jsim_ctx *ctx)
{
    if (g_rccl.h) return 0;
    const char *names[] = {getenv("JSIM_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names)
        if (n && n[0] && (h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(ctx, -2, "RCCL not found (librccl.so.1; set JSIM_RCCL_LIB): %s", dlerror());
    RcclApi a;
    a.h = h;
    a.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void **, int, JsimNcclId, int))dlsym(h, "ncclCommInitRank");
    a.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(h, "ncclAllGather");
    a.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    a.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString)
        return fail(ctx, -2, "RCCL library lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy");
    g_rccl = a;
    return 0;
}

extern "C" int jsim_comm_unique_id(void *id128)
{
    if (!id128) return fail(nullptr, -22, "jsim_comm_unique_id: null argument");
    if (int rc = rccl_load(nullptr)) return rc;
    const int r = g_rccl.GetUniqueId(id128);
    if (r) return fail(nullptr, -5, "ncclGetUniqueId: %s", g_rccl.GetErrorString(r));
    return 0;
}

extern "C" int jsim_comm_init(jsim_ctx *ctx, const void *id128, int32_t n_ranks, int32_t rank)
{
    if (!ctx) return fail(nullptr, -22, "jsim_comm_init: null ctx");
    if (!id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(ctx, -22, "jsim_comm_init: bad argument (rank %d of %d)", rank, n_ranks);
    if (ctx->comm) return fail(ctx, -17, "jsim_comm_init: this context already has a communicator");
    if (int rc = rccl_load(ctx)) return rc;
    DeviceGuard dev_guard(ctx->device); // ncclCommInitRank binds the communicator to the current device
    JSIM_GUARD_OK(ctx);
    JsimNcclId id;
    memcpy(&id, id128, sizeof(id));
    void *comm = nullptr;
    const int r = g_rccl.CommInitRank(&comm, n_ranks, id, rank);
    if (r) return fail(ctx, -5, "ncclCommInitRank(rank %d of %d): %s", rank, n_ranks, g_rccl.GetErrorString(r));
    ctx->comm = comm;
    return 0;
}

extern "C" int jsim_mpc_gather(jsim_ctx *ctx, void *comm, const void *local, void *out, size_t bytes_per_rank, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_gather: null ctx");
    void *c = comm ? comm : ctx->comm;
    if (!c) return fail(ctx, -22, "jsim_mpc_gather: no communicator (jsim_comm_init, or pass an ncclComm_t)");
    if (bytes_per_rank == 0) return 0;
    if (!local || !out) return fail(ctx, -22, "jsim_mpc_gather: null device pointer");
    if (int rc = rccl_load(ctx)) return rc;
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    const int r = g_rccl.AllGather(local, out, bytes_per_rank, /* ncclChar */ 0, c, (hipStream_t)stream);
    if (r) return fail(ctx, -5, "ncclAllGather: %s", g_rccl.GetErrorString(r));
    return 0;
}

extern "C" int jsim_comm_destroy(jsim_ctx *ctx)
{
    if (!ctx) return fail(nullptr, -22, "jsim_comm_destroy: null ctx");
    if (!ctx->comm) return 0;
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    const int r = g_rccl.h ? g_rccl.CommDestroy(ctx->comm) : 0;
    ctx->comm = nullptr;
    if (r) return fail(ctx, -5, "ncclCommDestroy: %s", g_rccl.GetErrorString(r));
    return 0;
}

#include "planner.inc"

// Route planner: HOST pointers in and out -- a one-time precompute whose (M, 3) output is what
// jsim_mpc_set_paths takes; device buffers are allocated, filled, searched (one wavefront per route) and read back inside the call.
// Both entry points below end here: wh [R][5], wc [R][4] and form [R] are per-route tables; `who` names the caller in the messages.
static int plan_routes_tables(const char *who, int device_id, int32_t n_routes, const double *start, const double *goal, const double *goal_box,
                              const double *tol, const double *hp, const int32_t *hp_off, int32_t n_obs_total,
                              const int32_t *route_obs_off, const double *mp_pts, const double *mp_len, int32_t n_prim,
                              int32_t n_pts, const double *cc_pts, const int32_t *cc_off, const double *wh, const double *wc,
                              const int32_t *form, int32_t max_path, int32_t node_cap, int32_t *status, double *cost, int32_t *n_prims,
                              int32_t *prims, double *nodes, double *traj, int32_t *n_expanded)
{
    if (n_routes < 0 || n_prim < 1 || n_prim > JPL_MAX_PRIM || n_pts < 2 || max_path < 1 || n_obs_total < 0 || node_cap < 64 || node_cap > (1 << 24))
        return fail(nullptr, -22, "%s: bad sizes (routes %d, primitives %d (max %d), points %d, max_path %d)", who, n_routes, n_prim,
                    JPL_MAX_PRIM, n_pts, max_path);
    if (n_routes == 0) return 0;
    if (!start || !goal || !goal_box || !tol || !hp_off || !route_obs_off || !mp_pts || !mp_len || !cc_pts || !cc_off || !wh || !wc || !form ||
        !status || !cost || !n_prims || !prims || !nodes || !traj || !n_expanded || (n_obs_total > 0 && !hp))
        return fail(nullptr, -22, "%s: null argument", who);
    // the offset tables index device arrays from inside the kernel: they must be what they claim to be
    for (int k = 0; k < n_obs_total; ++k)
        if (hp_off[k] < 0 || hp_off[k + 1] < hp_off[k]) return fail(nullptr, -22, "%s: hp_off is not non-decreasing at %d", who, k);
    if (hp_off[0] != 0) return fail(nullptr, -22, "%s: hp_off[0] = %d", who, hp_off[0]);
    for (int k = 0; k < n_routes; ++k)
        if (route_obs_off[k] < 0 || route_obs_off[k + 1] < route_obs_off[k] || route_obs_off[k + 1] > n_obs_total)
            return fail(nullptr, -22, "%s: route_obs_off[%d..%d] = %d, %d with %d obstacles", who, k, k + 1, route_obs_off[k], route_obs_off[k + 1], n_obs_total);
    for (int k = 0; k < n_prim; ++k)
        if (cc_off[k] < 0 || cc_off[k + 1] < cc_off[k]) return fail(nullptr, -22, "%s: cc_off is not non-decreasing at %d", who, k);
    for (int k = 0; k < n_routes; ++k) {
        if (form[k] != JPL_FORM_GENERIC && form[k] != JPL_FORM_MULTI)
            return fail(nullptr, -22, "%s: form[%d] = %d (0: mp_search_ww_generic, 1: multi_trajectory_planner)", who, k, form[k]);
        for (int j = 0; j < 9; ++j) {
            const double w = j < 5 ? wh[5 * (size_t)k + j] : wc[4 * (size_t)k + j - 5];
            if (!std::isfinite(w)) return fail(nullptr, -22, "%s: route %d: %s[%d] is not finite", who, k, j < 5 ? "wh" : "wc", j < 5 ? j : j - 5);
        }
    }
    JSIM_ON_DEVICE_ID(who, device_id);
    const int R = n_routes, cap = node_cap, seg = n_pts - 1;
    // sizes in 64 bits BEFORE anything is allocated: per route ~84 B per node slot (+ the hash table) and the output arrays
    if (max_path > 4096 || n_pts > 4096) return fail(nullptr, -22, "%s: max_path %d / points per primitive %d above 4096", who, max_path, n_pts);
    {
        const unsigned long long per_route = 84ull * (unsigned long long)cap * 3ull + 8ull * 3ull * (unsigned long long)max_path * (unsigned long long)seg;
        if ((unsigned long long)R * per_route > (64ull << 30))
            return fail(nullptr, -12, "%s: %d routes x node_cap %d x max_path %d would need more than 64 GiB of device memory", who, R, cap, max_path);
    }
    int hash_cap = 128;
    while (hash_cap < 2 * cap) hash_cap <<= 1;
    // a circle around every obstacle (the kernel's exact pruning of the collision test): vertices = the pairwise intersections of its
    // half-plane boundaries that satisfy all the others; bounded iff the largest angular gap between consecutive normals is below pi
    std::vector<double> obc((size_t)(n_obs_total > 0 ? n_obs_total : 1) * 3, 0.0);
    std::vector<double> vx, vy;                                       // (at most 64 * 63 / 2 vertices per obstacle)
    for (int o = 0; o < n_obs_total; ++o) {
        const double *q = hp + (size_t)hp_off[o] * 3;
        const int n = hp_off[o + 1] - hp_off[o];
        double *c = &obc[(size_t)o * 3];
        c[0] = 0.0; c[1] = 0.0; c[2] = INFINITY;
        if (n < 3 || n > 64) continue;
        double ang[64];
        for (int i = 0; i < n; ++i) ang[i] = atan2(q[3 * i + 1], q[3 * i]);
        std::sort(ang, ang + n);
        double gap = ang[0] + 2.0 * M_PI - ang[n - 1];
        for (int i = 1; i < n; ++i) gap = std::max(gap, ang[i] - ang[i - 1]);
        if (!(gap < M_PI - 1e-9)) continue;                       // unbounded (or degenerate): no circle, never pruned
        // EVERY such vertex counts: rows listed more than once give the same vertex many times over (a 16-gon with each row four
        // times: 16 x 16 of them), and a circle around only the first few of the list does not contain the obstacle
        double sx = 0.0, sy = 0.0;
        vx.clear(); vy.clear();
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) {
                const double a1 = q[3 * i], b1 = q[3 * i + 1], c1 = q[3 * i + 2], a2 = q[3 * j], b2 = q[3 * j + 1], c2 = q[3 * j + 2];
                const double det = a1 * b2 - a2 * b1;
                if (fabs(det) <= 1e-12 * (fabs(a1) + fabs(b1)) * (fabs(a2) + fabs(b2))) continue;
                const double px = (b1 * c2 - b2 * c1) / det, py = (a2 * c1 - a1 * c2) / det;
                bool in = std::isfinite(px) && std::isfinite(py);
                for (int k = 0; k < n && in; ++k) {
                    const double v = q[3 * k] * px + q[3 * k + 1] * py + q[3 * k + 2];
                    in = v <= 1e-9 * (1.0 + fabs(q[3 * k + 2]) + (fabs(q[3 * k]) + fabs(q[3 * k + 1])) * (fabs(px) + fabs(py)));
                }
                if (in) { vx.push_back(px); vy.push_back(py); sx += px; sy += py; }
            }
        const int nv = (int)vx.size();
        if (nv < 3) continue;                                    // (an empty or degenerate set: left to the exact test)
        const double mx = sx / nv, my = sy / nv;
        double rr = 0.0;
        for (int i = 0; i < nv; ++i) rr = std::max(rr, hypot(vx[i] - mx, vy[i] - my));
        c[0] = mx; c[1] = my; c[2] = rr * (1.0 + 1e-9) + 1e-9;
    }
    const size_t n_hp = (size_t)hp_off[n_obs_total], n_cc = (size_t)cc_off[n_prim];
    const size_t Rn = (size_t)R * cap, n_prims_out = (size_t)R * max_path, n_nodes = (size_t)R * (max_path + 1) * 3, n_traj = n_prims_out * seg * 3;
    DeviceScratch D;
    PlanP P;
    memset(&P, 0, sizeof(P));
    P.n_routes = R; P.n_prim = n_prim; P.n_pts = n_pts; P.max_path = max_path; P.node_cap = cap; P.hash_cap = hash_cap;
    P.wh = D.upload(wh, 5 * (size_t)R); P.wc = D.upload(wc, 4 * (size_t)R); P.form = D.upload(form, R);
    P.start = D.upload(start, 3 * (size_t)R); P.goal = D.upload(goal, 3 * (size_t)R);
    P.goal_box = D.upload(goal_box, 4 * (size_t)R); P.tol = D.upload(tol, R);
    P.hp = D.upload(hp, 3 * n_hp); P.hp_off = D.upload(hp_off, n_obs_total + 1); P.route_obs_off = D.upload(route_obs_off, R + 1);
    P.obc = D.upload(obc.data(), obc.size());
    P.mp_pts = D.upload(mp_pts, 3 * (size_t)n_prim * n_pts); P.mp_len = D.upload(mp_len, n_prim);
    P.cc_pts = D.upload(cc_pts, 2 * n_cc); P.cc_off = D.upload(cc_off, n_prim + 1);
    P.nx = D.alloc<double>(Rn); P.ny = D.alloc<double>(Rn); P.nth = D.alloc<double>(Rn); P.ng = D.alloc<double>(Rn);
    P.nparent = D.alloc<int>(Rn); P.nprim = D.alloc<int>(Rn); P.htab = D.alloc<int>((size_t)R * hash_cap);
    P.ov_gh = D.alloc<double>(Rn); P.ov_g = D.alloc<double>(Rn); P.ov_id = D.alloc<int>(Rn);
    P.status = D.alloc<int>(R); P.n_prims = D.alloc<int>(R); P.n_expanded = D.alloc<int>(R);
    P.prims = D.alloc<int>(n_prims_out); P.cost = D.alloc<double>(R);
    P.nodes = D.alloc<double>(n_nodes); P.traj = D.alloc<double>(n_traj);
    if (!D.ok()) return D.result(who);
    D.fill(P.cost, 0, R); D.fill(P.htab, 0xff, (size_t)R * hash_cap); D.fill(P.traj, 0, n_traj); D.fill(P.nodes, 0, n_nodes);
    D.fill(P.prims, 0xff, n_prims_out);
    if (D.ok()) {
        hipLaunchKernelGGL(plan_astar_kernel, dim3(R), dim3(64), 0, 0, P);
        D.err = hipGetLastError();
    }
    if (D.ok()) D.err = hipDeviceSynchronize();
#ifdef JPL_STAMPS
    {
        static long long clk[64][32];
        (void)hipMemcpyFromSymbol(clk, HIP_SYMBOL(jpl_clk), sizeof(clk));
        for (int r_ = 0; r_ < R && r_ < 64; ++r_)
            if (clk[r_][7] > 1000) {
                fprintf(stderr, "jpl route %d: %lld expansions, %lld nodes, %lld open at the end; per expansion:", r_, clk[r_][7], clk[r_][13], clk[r_][14]);
                for (int k = 0; k < 32; ++k) if (k != 7 && k != 13 && k != 14) fprintf(stderr, " [%d] %.2f", k, (double)clk[r_][k] / clk[r_][7]);
                fprintf(stderr, "\n");
            }
    }
#endif
    D.download(status, P.status, R); D.download(cost, P.cost, R); D.download(n_prims, P.n_prims, R); D.download(n_expanded, P.n_expanded, R);
    D.download(prims, P.prims, n_prims_out); D.download(nodes, P.nodes, n_nodes); D.download(traj, P.traj, n_traj);
    return D.result(who);
}

// One launch-wide weight set, the generic form (mp_search_ww_generic.py): its row repeated for every route.
extern "C" int jsim_plan_routes(int device_id, int32_t n_routes, const double *start, const double *goal, const double *goal_box,
                                const double *tol, const double *hp, const int32_t *hp_off, int32_t n_obs_total,
                                const int32_t *route_obs_off, const double *mp_pts, const double *mp_len, int32_t n_prim,
                                int32_t n_pts, const double *cc_pts, const int32_t *cc_off, const double *wh, const double *wc,
                                int32_t max_path, int32_t node_cap, int32_t *status, double *cost, int32_t *n_prims, int32_t *prims,
                                double *nodes, double *traj, int32_t *n_expanded)
{
    if (n_routes > (1 << 24))   // (at >= 16 KiB of workspace per route: beyond the 64 GiB the shared part allows)
        return fail(nullptr, -12, "jsim_plan_routes: %d routes would need more than 64 GiB of device memory", n_routes);
    const size_t R = n_routes > 0 ? (size_t)n_routes : 0;
    const bool tables = wh && wc;   // (a null pointer is reported by the shared part, after the sizes)
    std::vector<double> wht(5 * R), wct(4 * R);
    std::vector<int32_t> formt(R + 1, JPL_FORM_GENERIC);
    for (size_t k = 0; tables && k < R; ++k) {
        for (int j = 0; j < 5; ++j) wht[5 * k + j] = wh[j];
        for (int j = 0; j < 4; ++j) wct[4 * k + j] = wc[j];
    }
    return plan_routes_tables("jsim_plan_routes", device_id, n_routes, start, goal, goal_box, tol, hp, hp_off, n_obs_total, route_obs_off, mp_pts,
                              mp_len, n_prim, n_pts, cc_pts, cc_off, tables ? wht.data() : nullptr, tables ? wct.data() : nullptr, formt.data(),
                              max_path, node_cap, status, cost, n_prims, prims, nodes, traj, n_expanded);
}

// Per-route weights and cost form: a weight sweep of one scenario (Planner_Sensitivity_*.py, one planner run per set) or the candidate
// set of the multi-trajectory planner (multi_trajectory_planner.py:242-269 run_all, one A* per (e, p, o)) as ONE launch.
extern "C" int jsim_plan_routes_weighted(int device_id, int32_t n_routes, const double *start, const double *goal, const double *goal_box,
                                         const double *tol, const double *hp, const int32_t *hp_off, int32_t n_obs_total,
                                         const int32_t *route_obs_off, const double *mp_pts, const double *mp_len, int32_t n_prim,
                                         int32_t n_pts, const double *cc_pts, const int32_t *cc_off, const double *wh, const double *wc,
                                         const int32_t *form, int32_t max_path, int32_t node_cap, int32_t *status, double *cost,
                                         int32_t *n_prims, int32_t *prims, double *nodes, double *traj, int32_t *n_expanded)
{
    return plan_routes_tables("jsim_plan_routes_weighted", device_id, n_routes, start, goal, goal_box, tol, hp, hp_off, n_obs_total, route_obs_off,
                              mp_pts, mp_len, n_prim, n_pts, cc_pts, cc_off, wh, wc, form, max_path, node_cap, status, cost, n_prims, prims,
                              nodes, traj, n_expanded);
}

#include "reasons.inc"

// Stakeholder reasons: HOST pointers in and out -- a replan is an event, not a tick; device buffers are
// allocated, filled, scored (one workgroup per situation, one wavefront per candidate) and read back inside the call.
extern "C" int jsim_score_trajectories(int device_id, int32_t n_sit, const int32_t *cand_off, const int32_t *pt_off, const double *pts,
                                       const int32_t *mode, const int32_t *time_from, const double *ego, const double *cyc, const double *now,
                                       const double *par, int32_t n_w, const double *w, const int32_t *form, const double *ideal,
                                       int32_t *status, int32_t *n_samples, double *ct, double *avg, double *scores, int32_t *best,
                                       double *detail, double *resampled)
{
    const char *who = "jsim_score_trajectories";
    if (n_sit < 0 || n_w < 0 || n_sit > (1 << 20) || n_w > (1 << 24)) return fail(nullptr, -22, "%s: bad sizes (situations %d, weight rows %d)", who, n_sit, n_w);
    if (n_sit == 0) return 0;
    if (!cand_off || !pt_off || !mode || !time_from || !ego || !cyc || !now || !par || !ideal || !status || !n_samples || !ct || !avg ||
        (n_w > 0 && (!w || !form || !scores || !best)))
        return fail(nullptr, -22, "%s: null argument", who);
    if (cand_off[0] != 0) return fail(nullptr, -22, "%s: cand_off[0] = %d", who, cand_off[0]);
    for (int s = 0; s < n_sit; ++s) {
        if (cand_off[s + 1] < cand_off[s]) return fail(nullptr, -22, "%s: cand_off decreases at %d", who, s);
        if (cand_off[s + 1] - cand_off[s] > JSIM_MAX_CAND)
            return fail(nullptr, -22, "%s: situation %d has %d candidates (at most %d)", who, s, cand_off[s + 1] - cand_off[s], (int)JSIM_MAX_CAND);
    }
    const int ctot = cand_off[n_sit];
    if (pt_off[0] != 0) return fail(nullptr, -22, "%s: pt_off[0] = %d", who, pt_off[0]);
    for (int c = 0; c < ctot; ++c)
        if (pt_off[c + 1] < pt_off[c]) return fail(nullptr, -22, "%s: pt_off decreases at %d", who, c);
    const size_t n_pts = ctot > 0 ? (size_t)pt_off[ctot] : 0;
    if (n_pts > 0 && !pts) return fail(nullptr, -22, "%s: null argument", who);
    for (int s = 0; s < n_sit; ++s) {
        const int c0 = cand_off[s], C = cand_off[s + 1] - c0;
        for (int c = 0; c < C; ++c) {
            if (mode[c0 + c] != 0 && mode[c0 + c] != 1) return fail(nullptr, -22, "%s: mode[%d] = %d (0: planned, 1: following)", who, c0 + c, mode[c0 + c]);
            const int d = time_from[c0 + c];
            if (d < 0 || d >= C) return fail(nullptr, -22, "%s: time_from[%d] = %d outside its situation of %d", who, c0 + c, d, C);
            if (time_from[c0 + d] != d) return fail(nullptr, -22, "%s: time_from[%d] = %d names a candidate that names another", who, c0 + c, d);
        }
    }
    auto finite = [](const double *a, size_t n) { for (size_t k = 0; k < n; ++k) if (!std::isfinite(a[k])) return false; return true; };
    if (!finite(pts, 3 * n_pts) || !finite(ego, 4 * (size_t)n_sit) || !finite(cyc, 6 * (size_t)n_sit) || !finite(now, 5 * (size_t)n_sit) ||
        !finite(par, JSIM_REASON_NPAR * (size_t)n_sit) || !finite(w, 3 * (size_t)n_w) || !finite(ideal, 3))
        return fail(nullptr, -22, "%s: a number that is not finite", who);
    for (int s = 0; s < n_sit; ++s)
        if (!(par[JSIM_REASON_NPAR * (size_t)s + JSIM_REASON_DT] > 0.0)) return fail(nullptr, -22, "%s: situation %d: DT <= 0", who, s);
    for (int k = 0; k < n_w; ++k)
        if (form[k] != 0 && form[k] != 1) return fail(nullptr, -22, "%s: form[%d] = %d (0: for_reasons, 1: with_weights)", who, k, form[k]);
    for (int k = 0; k < 3; ++k)   // balance_function divides by each ideal weight (the reference raises ZeroDivisionError on a zero)
        if (!(ideal[k] > 0.0)) return fail(nullptr, -22, "%s: ideal[%d] <= 0", who, k);
    JSIM_ON_DEVICE_ID(who, device_id);
    const size_t S = (size_t)n_sit, W = (size_t)n_w, Ct = (size_t)ctot;
    if (W * (Ct + S) * 8ull > (16ull << 30)) return fail(nullptr, -12, "%s: %d weight rows x %d candidates would need more than 16 GiB", who, n_w, ctot);
    const size_t n_detail = Ct * 5 * JSIM_MAX_RES, n_res = Ct * JSIM_MAX_RES * 3;
    DeviceScratch D;
    ReasonP P;
    memset(&P, 0, sizeof(P));
    P.n_sit = n_sit; P.n_w = n_w; P.ctot = ctot;
    P.ideal[0] = ideal[0]; P.ideal[1] = ideal[1]; P.ideal[2] = ideal[2];
    P.cand_off = D.upload(cand_off, S + 1); P.pt_off = D.upload(pt_off, Ct + 1); P.pts = D.upload(pts, 3 * n_pts);
    P.mode = D.upload(mode, Ct); P.time_from = D.upload(time_from, Ct);
    P.ego = D.upload(ego, 4 * S); P.cyc = D.upload(cyc, 6 * S); P.now = D.upload(now, 5 * S); P.par = D.upload(par, JSIM_REASON_NPAR * S);
    P.w = D.upload(w, 3 * W); P.form = D.upload(form, W);
    P.status = D.alloc<int>(Ct); P.n_samples = D.alloc<int>(Ct); P.ct = D.alloc<double>(Ct); P.avg = D.alloc<double>(4 * Ct);
    P.scores = D.alloc<double>(W * Ct); P.best = D.alloc<int>(W * S);
    if (detail) P.detail = D.alloc<double>(n_detail);
    if (resampled) P.resampled = D.alloc<double>(n_res);
    if (!D.ok()) return D.result(who);
    // every real output starts as NaN (all bits set): what the kernel does not write -- a candidate with a status, the rows behind a
    // candidate's samples -- stays NaN
    D.fill(P.ct, 0xff, Ct); D.fill(P.avg, 0xff, 4 * Ct); D.fill(P.scores, 0xff, W * Ct);
    if (detail) D.fill(P.detail, 0xff, n_detail);
    if (resampled) D.fill(P.resampled, 0xff, n_res);
    if (D.ok()) {
        hipLaunchKernelGGL(score_trajectories_kernel, dim3(n_sit), dim3(64 * JSIM_MAX_CAND), 0, 0, P);
        D.err = hipGetLastError();
    }
    if (D.ok()) D.err = hipDeviceSynchronize();
    D.download(status, P.status, Ct); D.download(n_samples, P.n_samples, Ct); D.download(ct, P.ct, Ct); D.download(avg, P.avg, 4 * Ct);
    D.download(scores, P.scores, W * Ct); D.download(best, P.best, W * S);
    if (detail) D.download(detail, P.detail, n_detail);
    if (resampled) D.download(resampled, P.resampled, n_res);
    return D.result(who);
}

#include "recorder_walk.inc"
#include "reasons_ticks.inc"

// ---- what the four calls that read the History recorder share around their launches ----
// The end of such a call's checks (they need no context and no device, so a null ctx is refused last) and the start of its device
// work: with nothing to do (`nothing_`) it returns, else it runs on the context's device
#define JSIM_RECORDER_CALL(nothing_)                                                                           \
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);                                                   \
    if (nothing_) return 0;                                                                                   \
    DeviceGuard dev_guard(ctx->device);                                                                        \
    JSIM_GUARD_OK(ctx)

// ego_shape = the egos' (cc_front, cc_rear, radius), a HOST pointer
static int check_ego_shape(jsim_ctx *ctx, const char *F, const double *s)
{
    if (!std::isfinite(s[0]) || !std::isfinite(s[1])) return fail(ctx, -22, "%s: ego_shape: a circle offset that is not finite", F);
    if (!(s[2] > 0.0) || !std::isfinite(s[2])) return fail(ctx, -22, "%s: ego_shape: radius %g is not positive and finite", F, s[2]);
    return 0;
}
// Replace one of the context's tables with n host entries; sync = false: behind another replacement, with no launch in between
template <class T> static int replace_table(jsim_ctx *ctx, DevArray<T> &table, const T *host, size_t n, bool sync = true)
{
    if (sync) HIP_TRY(ctx, hipDeviceSynchronize()); // an earlier call's launch may still read the table that is replaced
    HIP_TRY(ctx, table.reserve(n));
    HIP_TRY(ctx, hipMemcpy(table, host, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}
// One wavefront per ego on `stream`
template <class PT> static int launch_per_ego(jsim_ctx *ctx, void (*kernel)(const PT), int B, void *stream, const PT &P)
{
    hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// Stakeholder reasons per recorded tick and the replan trigger: DEVICE pointers, the recorder's buffers as
// they are; one launch on `stream`, one wavefront per ego.
extern "C" int jsim_loop_eval_reasons(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                      const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_of,
                                      const double *par, const double *threshold, double *carry, double *val, double *timers,
                                      int32_t *trig, int32_t *first, void *stream)
{
    const char *const F = "jsim_loop_eval_reasons";
    if (B < 0 || n_ticks < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d", F, B, n_ticks);
    if (obs_rec && n_obs < 1) return fail(ctx, -22, "%s: obs_rec given with n_obs=%d", F, n_obs);
    if (!rec || !flags || !x_first || !x_spawn || !veh_of || !par || !threshold || !carry || !val || !timers || !trig || !first)
        return fail(ctx, -22, "%s: null device pointer", F);
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    const ReasonTickP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), obs_rec ? n_obs : 0, obs_rec, veh_of, par, threshold,
                           carry, val, timers, trig, first};
    return launch_per_ego(ctx, reason_ticks_kernel, B, stream, P);
}

#include "conflicts.inc"

// ---- the vehicle-list arguments of the conflicts, gaps and headway entry points ----
// DEVICE pointers but for shapes [n_obs][4] = the rows of jsim_loop_set_vehicle_shapes and ego_shape = the egos' (cc_front, cc_rear,
// radius), which are HOST pointers: the device rows are made here
struct VehicleArgs {
    int n_obs;
    const double *obs_rec;
    const int *veh_range, *mate_range;
    const double *shapes, *ego_shape;
};
// The checks, ahead of JSIM_RECORDER_CALL
static int check_vehicle_list(jsim_ctx *ctx, const char *F, const VehicleArgs &A)
{
    if (!A.obs_rec && A.n_obs > 0) return fail(ctx, -22, "%s: null obs_rec with n_obs=%d", F, A.n_obs);
    if (!A.ego_shape) return fail(ctx, -22, "%s: null ego_shape", F);
    if (int rc = check_ego_shape(ctx, F, A.ego_shape)) return rc;
    for (int i = 0; A.shapes && i < A.n_obs; ++i) {
        const double *s = A.shapes + 4 * (size_t)i;
        if (!std::isfinite(s[0]) || !std::isfinite(s[1]) || !(s[2] > 0.0) || !std::isfinite(s[2]))
            return fail(ctx, -22, "%s: shapes row %d needs finite circle offsets and a positive, finite radius", F, i);
    }
    return 0;
}
// A row of a vehicle of radius r: min_distance thr = the egos' radius + its own; (thr, thr_sq: the squared form the distances are
// compared with) for conflicts and gaps, (radius, thr) for headway
static double4 vehicle_row(bool radius_thr, double cc_f, double cc_r, double r, double r_ego)
{
    const double thr = r_ego + r;
    return radius_thr ? double4{cc_f, cc_r, r, thr} : double4{cc_f, cc_r, thr, jsim_sqrt_threshold(thr)};
}
// The device work, behind JSIM_RECORDER_CALL: the rows of `shapes` replace `table`, the call's own (a launch of another call may
// still read that call's table), and V is the kernel's argument
static int upload_vehicle_list(jsim_ctx *ctx, DevArray<double4> &table, const RecorderBuf &R, const VehicleArgs &A, bool radius_thr,
                               VehicleListP &V)
{
    const double *e = A.ego_shape;
    const bool rows = A.shapes && A.n_obs > 0;
    if (rows) {
        std::vector<double4> host((size_t)A.n_obs);
        for (int i = 0; i < A.n_obs; ++i) {
            const double *s = A.shapes + 4 * (size_t)i;
            host[i] = vehicle_row(radius_thr, s[0], s[1], s[2], e[2]);
        }
        if (int rc = replace_table(ctx, table, host.data(), (size_t)A.n_obs)) return rc;
    }
    V = VehicleListP{R, A.n_obs, A.n_obs > 0 ? A.obs_rec : nullptr, A.veh_range, A.mate_range, rows ? table.p : nullptr, e[0], e[1],
                     vehicle_row(radius_thr, e[0], e[1], e[2], e[2])};
    return 0;
}

// Clearance and first contact per recorded tick: DEVICE pointers for the recorder's buffers, the ranges and
// the outputs, HOST pointers for `shapes` and `ego_shape` (the thresholds are made here, on the host); one launch on `stream`, one
// wavefront per ego.
extern "C" int jsim_loop_eval_conflicts(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                        const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                                        const int32_t *mate_range, const double *shapes, const double *ego_shape, int32_t frame_window,
                                        double *clear, int32_t *who, int32_t *row, int32_t *hit_tick, int32_t *hit_frame,
                                        double *hit_xy, void *stream)
{
    const char *const F = "jsim_loop_eval_conflicts";
    if (B < 0 || n_ticks < 0 || n_obs < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d n_obs=%d", F, B, n_ticks, n_obs);
    if (frame_window < 0 || frame_window > 20) return fail(ctx, -22, "%s: frame_window=%d outside [0, 20]", F, frame_window);
    if (!rec || !flags || !x_first || !x_spawn || !veh_range || !mate_range || !clear || !who || !row || !hit_tick || !hit_frame || !hit_xy)
        return fail(ctx, -22, "%s: null device pointer", F);
    const VehicleArgs A = {n_obs, obs_rec, veh_range, mate_range, shapes, ego_shape};
    if (int rc = check_vehicle_list(ctx, F, A)) return rc;
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    ConflictP P = {{}, frame_window, clear, who, row, hit_tick, hit_frame, hit_xy};
    if (int rc = upload_vehicle_list(ctx, ctx->d_conflict_rows, recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), A, false, P.V)) return rc;
    return launch_per_ego(ctx, conflict_ticks_kernel, B, stream, P);
}

#include "gaps.inc"

// The time gap between an ego and each vehicle per recorded tick: pointers as jsim_loop_eval_conflicts has
// them; one launch on `stream`, one wavefront per ego, its LDS sized from the window and the longest list the tables allow.
extern "C" int jsim_loop_eval_gaps(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                   const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                                   const int32_t *mate_range, const double *shapes, const double *ego_shape, int32_t window, int32_t within,
                                   int8_t *off, int32_t *ep_gap, int32_t *ep_tick, int32_t *ep_who, int32_t *ep_off, void *stream)
{
    const char *const F = "jsim_loop_eval_gaps";
    if (B < 0 || n_ticks < 0 || n_obs < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d n_obs=%d", F, B, n_ticks, n_obs);
    if (window < 0 || window > JSIM_GAP_MAX_WINDOW) return fail(ctx, -22, "%s: window=%d outside [0, %d]", F, window, JSIM_GAP_MAX_WINDOW);
    if (within != 0 && within != 1) return fail(ctx, -22, "%s: within=%d is neither 0 (episode) nor 1 (record)", F, within);
    if (!rec || !flags || !x_first || !x_spawn || !veh_range || !mate_range) return fail(ctx, -22, "%s: null device pointer", F);
    const void *const outs[] = {off, ep_gap, ep_tick, ep_who, ep_off};
    const char *const out_names[] = {"off", "ep_gap", "ep_tick", "ep_who", "ep_off"};
    for (int i = 0; i < 5; ++i)
        if (!outs[i]) return fail(ctx, -22, "%s: null output %s", F, out_names[i]);
    const VehicleArgs A = {n_obs, obs_rec, veh_range, mate_range, shapes, ego_shape};
    if (int rc = check_vehicle_list(ctx, F, A)) return rc;
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    GapP P = {{}, window, within, reinterpret_cast<unsigned long long *>(off), ep_gap, ep_tick, ep_who, ep_off};
    if (int rc = upload_vehicle_list(ctx, ctx->d_gap_rows, recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), A, false, P.V)) return rc;
    // no list is longer than the recorded vehicles plus the other egos, or than JSIM_MAX_OBS (jcf_list clamps to both)
    const int longest = std::min<long long>(JSIM_MAX_OBS, (long long)n_obs + B - 1);
    const size_t lds = sizeof(double2) * 2 * (size_t)std::max(longest, 1) * (size_t)(64 + 2 * window);
    hipLaunchKernelGGL(gap_ticks_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

#include "static_conflicts.inc"

// Static-obstacle clearance and contact per recorded tick: DEVICE pointers for the recorder's buffers, set_of
// and the outputs, HOST pointers for `set_off`, `rows` and `ego_shape` (checked here, copied to the device inside the call); one
// launch on `stream`, one wavefront per ego.
extern "C" int jsim_loop_eval_static(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, const double *x_first,
                                     const double *x_spawn, const int32_t *set_of, int32_t n_sets, const int32_t *set_off, int32_t n_rows,
                                     const double *rows, const double *ego_shape, int32_t include_hidden, double *clear, int32_t *who,
                                     int32_t *hit, int32_t *off_tick, void *stream)
{
    const char *const F = "jsim_loop_eval_static";
    if (B < 0 || n_ticks < 0 || n_sets < 0 || n_rows < 0)
        return fail(ctx, -22, "%s: B=%d n_ticks=%d n_sets=%d n_rows=%d", F, B, n_ticks, n_sets, n_rows);
    if (include_hidden != 0 && include_hidden != 1) return fail(ctx, -22, "%s: include_hidden=%d is neither 0 nor 1", F, include_hidden);
    if (!ego_shape) return fail(ctx, -22, "%s: null ego_shape", F);
    if (!set_off && n_sets > 0) return fail(ctx, -22, "%s: null set_off with n_sets=%d", F, n_sets);
    if (!rows && (n_sets > 0 || n_rows > 0)) return fail(ctx, -22, "%s: null rows with n_sets=%d n_rows=%d", F, n_sets, n_rows);
    if (!rec || !flags || !x_first || !x_spawn || !set_of || !clear || !who || !hit || !off_tick)
        return fail(ctx, -22, "%s: null device pointer", F);
    if (int rc = check_ego_shape(ctx, F, ego_shape)) return rc;
    const double cc_f = ego_shape[0], cc_r = ego_shape[1], r_ego = ego_shape[2];
    if (set_off) {
        if (set_off[0] != 0) return fail(ctx, -22, "%s: set_off[0]=%d, not 0", F, set_off[0]);
        for (int s = 0; s < n_sets; ++s)
            if (set_off[s + 1] < set_off[s]) return fail(ctx, -22, "%s: set_off decreases at set %d", F, s);
    }
    if ((set_off ? set_off[n_sets] : 0) != n_rows)
        return fail(ctx, -22, "%s: set_off ends at %d, not at n_rows=%d", F, set_off ? set_off[n_sets] : 0, n_rows);
    for (int i = 0; i < n_rows; ++i) {
        const double *r = rows + JSIM_STATIC_ROW * (size_t)i;
        if (r[0] != 0.0 && r[0] != 1.0) return fail(ctx, -22, "%s: rows[%d]: kind %g is neither 0 (box) nor 1 (circle)", F, i, r[0]);
        if (r[1] != 0.0 && r[1] != 1.0) return fail(ctx, -22, "%s: rows[%d]: hidden %g is neither 0 nor 1", F, i, r[1]);
        if (!(r[2] >= 1.0 && r[2] <= 8.0) || r[2] != std::floor(r[2])) return fail(ctx, -22, "%s: rows[%d]: n_hp %g outside 1..8", F, i, r[2]);
        for (int j = 3; j < 7; ++j)
            if (!std::isfinite(r[j])) return fail(ctx, -22, "%s: rows[%d]: geometry entry %d is not finite", F, i, j);
        for (int j = 8; j < 8 + 3 * (int)r[2]; ++j)
            if (!std::isfinite(r[j])) return fail(ctx, -22, "%s: rows[%d]: half-plane entry %d is not finite", F, i, j);
        if (r[0] == 1.0 && !(r[5] > 0.0)) return fail(ctx, -22, "%s: rows[%d]: circle radius %g is not positive", F, i, r[5]);
        if (r[0] == 0.0 && (r[3] > r[5] || r[4] > r[6])) return fail(ctx, -22, "%s: rows[%d]: box with x1 > x2 or y1 > y2", F, i);
    }
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    if (n_sets > 0) {
        if (int rc = replace_table(ctx, ctx->d_static_off, set_off, (size_t)n_sets + 1)) return rc;
        if (n_rows > 0)
            if (int rc = replace_table(ctx, ctx->d_static_rows, rows, (size_t)n_rows * JSIM_STATIC_ROW, false)) return rc;
    }
    const StaticP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), n_sets, include_hidden, set_of,
                       n_sets > 0 ? ctx->d_static_off.p : nullptr, n_rows > 0 ? ctx->d_static_rows.p : nullptr, cc_f, cc_r, r_ego,
                       clear, who, hit, off_tick};
    return launch_per_ego(ctx, static_ticks_kernel, B, stream, P);
}

#include "episodes.inc"

// One row per recorded episode: DEVICE pointers throughout -- the recorder's buffers, the per-tick outputs of
// the three calls above (each group NULL or whole) and the table; three launches on `stream` (count, scan, summary).
extern "C" int jsim_loop_summarise_episodes(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                                            const double *x_first, const double *x_spawn, const double *veh_clear, const int32_t *veh_who,
                                            const int32_t *veh_hit_tick, const int32_t *veh_hit_frame, const double *veh_hit_xy,
                                            const double *st_clear, const int32_t *st_who, const int32_t *st_hit,
                                            const int32_t *st_off_tick, const double *rs_val, const int32_t *rs_trig, int32_t ep_cap,
                                            int64_t *ep_off, int32_t *ep_i, double *ep_d, void *stream)
{
    const char *const F = "jsim_loop_summarise_episodes";
    if (B < 0 || n_ticks < 0 || ep_cap < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d ep_cap=%d", F, B, n_ticks, ep_cap);
    const int n_veh = !!veh_clear + !!veh_who + !!veh_hit_tick + !!veh_hit_frame + !!veh_hit_xy;
    if (n_veh != 0 && n_veh != 5)
        return fail(ctx, -22, "%s: the veh_ group (veh_clear, veh_who, veh_hit_tick, veh_hit_frame, veh_hit_xy) is given in part", F);
    const int n_st = !!st_clear + !!st_who + !!st_hit + !!st_off_tick;
    if (n_st != 0 && n_st != 4) return fail(ctx, -22, "%s: the st_ group (st_clear, st_who, st_hit, st_off_tick) is given in part", F);
    if (!rs_val != !rs_trig) return fail(ctx, -22, "%s: the rs_ group (rs_val, rs_trig) is given in part", F);
    if (!rec || !flags || !x_first || !x_spawn || !ep_off || !ep_i || !ep_d) return fail(ctx, -22, "%s: null device pointer", F);
    JSIM_RECORDER_CALL(false);     // (no ego, no tick: the scan still writes the offsets)
    const EpisodeP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), ep_cap, veh_clear, veh_who, veh_hit_tick, veh_hit_frame, veh_hit_xy,
                        st_clear, st_who, st_hit, st_off_tick, rs_val, rs_trig, (long long *)ep_off, ep_i, ep_d};
    if (B > 0)
        if (int rc = launch_per_ego(ctx, episode_count_kernel, B, stream, P)) return rc;
    hipLaunchKernelGGL(episode_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return B > 0 ? launch_per_ego(ctx, episode_summary_kernel, B, stream, P) : 0;
}

#include "path_project.inc"
#include "tracking.inc"

// The call's own path table as the tracking and headway entry points take it, behind their null-pointer loops: DEVICE pointers with
// HOST counts (n_pts, n_paths >= 0 checked with the call's other counts)
static int path_table(jsim_ctx *ctx, const char *F, int B, const int32_t *path_id, int n_pts, const double *px, const double *py,
                      const double *pyaw, int n_paths, const int64_t *path_off, const double *arc, PathTableP &T)
{
    if (n_paths == 0 && B > 0) return fail(ctx, -22, "%s: n_paths=0 with B=%d", F, B);
    T = PathTableP{path_id, n_pts, n_paths, px, py, pyaw, arc, (const long long *)path_off};
    return 0;
}

// Every recorded pose projected onto a path: DEVICE pointers throughout -- the recorder's buffers, path_id,
// the call's own path table and the outputs -- with HOST counts; one launch on `stream`, one wavefront per ego.
extern "C" int jsim_loop_eval_tracking(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                                       const int32_t *path_id, int32_t n_pts, const double *px, const double *py, const double *pyaw,
                                       int32_t n_paths, const int64_t *path_off, const double *arc, int32_t *idx, int32_t *seg, double *s,
                                       double *d, double *e_yaw, int32_t *ep_i, double *ep_d, void *stream)
{
    const char *const F = "jsim_loop_eval_tracking";
    if (B < 0 || n_ticks < 0 || n_pts < 0 || n_paths < 0)
        return fail(ctx, -22, "%s: B=%d n_ticks=%d n_pts=%d n_paths=%d", F, B, n_ticks, n_pts, n_paths);
    const void *const ptrs[] = {rec, flags, path_id, px, py, pyaw, path_off, arc, idx, seg, s, d, e_yaw, ep_i, ep_d};
    const char *const names[] = {"rec", "flags", "path_id", "px", "py", "pyaw", "path_off", "arc", "idx", "seg", "s", "d", "e_yaw", "ep_i", "ep_d"};
    for (int i = 0; i < 15; ++i)
        if (!ptrs[i]) return fail(ctx, -22, "%s: null pointer %s", F, names[i]);
    TrackP P = {B, n_ticks, rec, flags, {}, idx, seg, s, d, e_yaw, ep_i, ep_d};
    if (int rc = path_table(ctx, F, B, path_id, n_pts, px, py, pyaw, n_paths, path_off, arc, P.T)) return rc;
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    return launch_per_ego(ctx, tracking_ticks_kernel, B, stream, P);
}

#include "headway.inc"

// Every recorded vehicle projected onto the ego's path: DEVICE pointers for the recorder's buffers, the
// ranges, path_id, the call's own path table and the outputs, HOST pointers for `shapes` and `ego_shape` (radii and thresholds are
// made here, on the host) with HOST counts and margin; one launch on `stream`, one wavefront per ego.
extern "C" int jsim_loop_eval_headway(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                      const double *obs_rec, const double *x_first, const double *x_spawn, const int32_t *veh_range,
                                      const int32_t *mate_range, const double *shapes, const double *ego_shape, const int32_t *path_id,
                                      int32_t n_pts, const double *px, const double *py, const double *pyaw, int32_t n_paths,
                                      const int64_t *path_off, const double *arc, double margin, int32_t *lead, double *lead_gap,
                                      double *thw, double *ttc, int32_t *ttc_who, double *u_ego, int32_t *ep_i, double *ep_d, double *gap,
                                      double *lat, double *rate, void *stream)
{
    const char *const F = "jsim_loop_eval_headway";
    if (B < 0 || n_ticks < 0 || n_obs < 0 || n_pts < 0 || n_paths < 0)
        return fail(ctx, -22, "%s: B=%d n_ticks=%d n_obs=%d n_pts=%d n_paths=%d", F, B, n_ticks, n_obs, n_pts, n_paths);
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(ctx, -22, "%s: margin %g is not finite and >= 0", F, margin);
    const void *const ptrs[] = {rec, flags, x_first, x_spawn, veh_range, mate_range, ego_shape, path_id, px, py, pyaw, path_off, arc,
                                lead, lead_gap, thw, ttc, ttc_who, u_ego, ep_i, ep_d};
    const char *const names[] = {"rec", "flags", "x_first", "x_spawn", "veh_range", "mate_range", "ego_shape", "path_id", "px", "py", "pyaw",
                                 "path_off", "arc", "lead", "lead_gap", "thw", "ttc", "ttc_who", "u_ego", "ep_i", "ep_d"};
    for (int i = 0; i < 21; ++i)
        if (!ptrs[i]) return fail(ctx, -22, "%s: null pointer %s", F, names[i]);
    const int n_places = !!gap + !!lat + !!rate;
    if (n_places != 0 && n_places != 3) return fail(ctx, -22, "%s: the per-place outputs (gap, lat, rate) are given in part", F);
    const VehicleArgs A = {n_obs, obs_rec, veh_range, mate_range, shapes, ego_shape};
    HeadwayP P = {{}, {}, ego_shape[2], margin, lead, lead_gap, thw, ttc, ttc_who, u_ego, ep_i, ep_d, gap, lat, rate};
    if (int rc = path_table(ctx, F, B, path_id, n_pts, px, py, pyaw, n_paths, path_off, arc, P.T)) return rc;
    if (int rc = check_vehicle_list(ctx, F, A)) return rc;
    JSIM_RECORDER_CALL(B == 0 || n_ticks == 0);
    if (int rc = upload_vehicle_list(ctx, ctx->d_headway_rows, recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), A, true, P.V)) return rc;
    return launch_per_ego(ctx, headway_ticks_kernel, B, stream, P);
}

// the shape table's (thr, thr_sq) rows: check_collision_moving_bicycle's min_distance = the egos' radius + the vehicle's own
static int upload_shape_thresholds(jsim_ctx *ctx)
{
    if (ctx->n_shapes == 0) return 0;
    std::vector<double2> th((size_t)ctx->n_shapes);
    for (int i = 0; i < ctx->n_shapes; ++i) {
        const double thr = ctx->col_radius + ctx->h_shapes[4 * (size_t)i + 2];
        th[i] = double2{thr, jsim_sqrt_threshold(thr)};
    }
    HIP_TRY(ctx, hipDeviceSynchronize()); // launches in flight on any stream may still read the table that is replaced
    HIP_TRY(ctx, ctx->d_othr.reserve(ctx->n_shapes));
    HIP_TRY(ctx, hipMemcpy(ctx->d_othr, th.data(), sizeof(double2) * ctx->n_shapes, hipMemcpyHostToDevice));
    return 0;
}

// A registered shape table must be the call's: one row per scripted vehicle (a call without vehicles passes)
static int check_shapes(jsim_ctx *ctx, const char *fn, int n_obs)
{
    if (ctx->n_shapes > 0 && n_obs > 0 && n_obs != ctx->n_shapes)
        return fail(ctx, -22, "%s: n_obs=%d, but the shape table (jsim_loop_set_vehicle_shapes) holds %d vehicles", fn, n_obs,
                    ctx->n_shapes);
    return 0;
}

extern "C" int jsim_loop_set_geometry(jsim_ctx *ctx, double cc_front, double cc_rear, double radius)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_set_geometry: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!(radius > 0)) return fail(ctx, -22, "jsim_loop_set_geometry: radius must be positive");
    ctx->cc0 = cc_front; ctx->cc1 = cc_rear; ctx->col_radius = radius; ctx->have_geom = 1;
    if (!ctx->have_ogeom) { ctx->occ0 = cc_front; ctx->occ1 = cc_rear; ctx->ocol_radius = radius; ctx->oL = ctx->cfg.L; }
    HIP_TRY(ctx, ctx->d_pred_cc.reserve(JSIM_MAX_OBS * JSIM_MAX_PRED * 2));
    HIP_TRY(ctx, ctx->d_pred_bc.reserve(JSIM_MAX_OBS));
    if (int rc = upload_shape_thresholds(ctx)) return rc;
    return upload_circle_centres(ctx);
}

extern "C" int jsim_loop_set_obstacle_geometry(jsim_ctx *ctx, double cc_front, double cc_rear, double radius, double wheelbase)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_set_obstacle_geometry: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!(radius > 0) || !(wheelbase > 0)) return fail(ctx, -22, "jsim_loop_set_obstacle_geometry: radius and wheelbase must be positive");
    ctx->occ0 = cc_front; ctx->occ1 = cc_rear; ctx->ocol_radius = radius; ctx->oL = wheelbase; ctx->have_ogeom = 1;
    return 0;
}

// ---- Per-vehicle shapes: each scripted vehicle is predicted, stepped and tested with its own circles and wheelbase ----
extern "C" int jsim_loop_set_vehicle_shapes(jsim_ctx *ctx, int32_t n, const double *shapes)
{
    const char *const F = "jsim_loop_set_vehicle_shapes";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (n < 0) return fail(ctx, -22, "%s: n=%d", F, n);
    if (n > 0) {
        if (!shapes) return fail(ctx, -22, "%s: null shapes", F);
        if (!ctx->have_geom) return fail(ctx, -22, "%s: jsim_loop_set_geometry has not been called", F);
        for (int i = 0; i < n; ++i)
            if (!(shapes[4 * (size_t)i + 2] > 0) || !(shapes[4 * (size_t)i + 3] > 0) || !std::isfinite(shapes[4 * (size_t)i]) ||
                !std::isfinite(shapes[4 * (size_t)i + 1]))
                return fail(ctx, -22, "%s: vehicle %d: radius and wheelbase must be positive, the circle offsets finite", F, i);
    }
    if (n == 0) { ctx->n_shapes = 0; ctx->h_shapes.clear(); return 0; }
    // (the device copies are written before the table is switched: a failed upload leaves the context without one; launches
    // in flight on any stream may still read the table that is replaced: they finish first)
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->n_shapes = 0;
    static_assert(sizeof(double4) == 4 * sizeof(double), "a shape row is one double4");
    HIP_TRY(ctx, ctx->d_shapes.reserve(n));
    HIP_TRY(ctx, hipMemcpy(ctx->d_shapes, shapes, sizeof(double4) * n, hipMemcpyHostToDevice));
    ctx->h_shapes.assign(shapes, shapes + 4 * (size_t)n);
    ctx->n_shapes = n;
    if (int rc = upload_shape_thresholds(ctx)) { ctx->n_shapes = 0; return rc; }
    return 0;
}

static const double4 *shapes_p(const jsim_ctx *ctx) { return ctx->n_shapes > 0 ? ctx->d_shapes.p : nullptr; }

// ---- Route vehicles: the table of polylines that kind-3 rows of the obstacle tables follow (the rule: include/jsim_mpc.h) ----
extern "C" int jsim_loop_set_traffic_routes(jsim_ctx *ctx, int32_t n_routes, const double *x, const double *y, const double *yaw,
                                            const int32_t *off)
{
    const char *const F = "jsim_loop_set_traffic_routes";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (n_routes < 0) return fail(ctx, -22, "%s: n_routes=%d", F, n_routes);
    if (n_routes == 0) {
        HIP_TRY(ctx, hipDeviceSynchronize()); // launches in flight keep the table they were given
        ctx->n_routes = 0;
        return 0;
    }
    if (!x || !y || !yaw || !off) return fail(ctx, -22, "%s: null array", F);
    if (off[0] != 0) return fail(ctx, -22, "%s: off[0]=%d, not 0", F, off[0]);
    for (int r = 0; r < n_routes; ++r)
        if (off[r + 1] < off[r]) return fail(ctx, -22, "%s: offsets decrease at route %d (%d after %d)", F, r, off[r + 1], off[r]);
    const size_t n = (size_t)off[n_routes];
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i]) || !std::isfinite(yaw[i]))
            return fail(ctx, -22, "%s: point %zu is not finite", F, i);
    // (launches in flight on any stream may still read the table that is replaced: they finish first; a failed upload leaves the
    // context without a table)
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->n_routes = 0;
    HIP_TRY(ctx, ctx->d_route_off.reserve((size_t)n_routes + 1));
    HIP_TRY(ctx, ctx->d_route_pt.reserve(n > 0 ? n : 1));
    HIP_TRY(ctx, ctx->d_route_in.reserve(n > 0 ? 3 * n : 1));
    HIP_TRY(ctx, hipMemcpy(ctx->d_route_off, off, sizeof(int) * ((size_t)n_routes + 1), hipMemcpyHostToDevice));
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpy(ctx->d_route_in.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_route_in.p + n, y, sizeof(double) * n, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_route_in.p + 2 * n, yaw, sizeof(double) * n, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(route_arclen_kernel, dim3((n_routes + 63) / 64), dim3(64), 0, (hipStream_t)0, n_routes, ctx->d_route_off.p,
                       ctx->d_route_in.p, ctx->d_route_in.p + n, ctx->d_route_in.p + 2 * n, ctx->d_route_pt.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize()); // the table is whole before any stream's next launch reads it
    ctx->n_routes = n_routes;
    return 0;
}

// obstacle_predict_kernel on n_ticks consecutive ticks' get() tuples of n_obs > 0 vehicles
static void launch_obstacle_predict(const jsim_ctx *ctx, int n_obs, int n_steps, const double *get, double *pred, double2 *pred_cc,
                                    double4 *pred_bc, int n_ticks, hipStream_t s)
{
    const ObsP P = {n_obs, n_steps, ctx->cfg.dt, ctx->oL, ctx->occ0, ctx->occ1, get, pred, pred_cc, pred_bc, shapes_p(ctx)};
    hipLaunchKernelGGL(obstacle_predict_kernel, dim3((n_obs + 63) / 64, n_ticks), dim3(64), 0, s, P);
}

// one get(), or get() + step(), of O.n_obs > 0 vehicles
static void launch_obstacle_step(const ObsStepP &O, hipStream_t s)
{
    hipLaunchKernelGGL(obstacle_step_kernel, dim3((O.n_obs + 63) / 64), dim3(64), 0, s, O);
}

// n_ticks ticks of them, every tick's get() tuples to get_all
static void launch_obstacle_rollout(const ObsStepP &O, int n_ticks, double *get_all, hipStream_t s)
{
    hipLaunchKernelGGL(obstacle_rollout_kernel, dim3((O.n_obs + 63) / 64), dim3(64), 0, s, O, n_ticks, get_all);
}

// the registered traffic layout as the glue kernels take it (both NULL without one)
static TrafficP traffic_p(const jsim_ctx *ctx)
{
    if (ctx->n_sets == 0) return TrafficP{nullptr, nullptr};
    return TrafficP{ctx->d_set_of, ctx->d_obs_off};
}

static ObsStepP obstacle_step_p(const jsim_ctx *ctx, int n_obs, int do_step, double *state, const double *param, double *get)
{
    return ObsStepP{n_obs, do_step, ctx->have_ogeom ? ctx->oL : ctx->cfg.L, state, param, get, nullptr, nullptr, 0, shapes_p(ctx),
                    ctx->n_routes > 0 ? ctx->d_route_pt.p : nullptr, ctx->n_routes > 0 ? ctx->d_route_off.p : nullptr, ctx->n_routes};
}

// the same, with the recorder's obstacle tuples (when one is registered) at the slots of the device tick counter
static ObsStepP obstacle_step_rec_p(const jsim_ctx *ctx, int n_obs, int do_step, double *state, const double *param, double *get,
                                    const int32_t *tick)
{
    ObsStepP O = obstacle_step_p(ctx, n_obs, do_step, state, param, get);
    if (ctx->rec_obs) { O.rec = ctx->rec_obs; O.tick = tick; O.rec_cap = ctx->rec_cap; }
    return O;
}

extern "C" int jsim_loop_predict_obstacles(jsim_ctx *ctx, int32_t n_obs, const double *obst, int32_t n_steps, double *pred,
                                           void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_predict_obstacles: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!ctx->have_geom) return fail(ctx, -22, "jsim_loop_predict_obstacles: jsim_loop_set_geometry has not been called");
    if (n_obs < 0 || n_obs > JSIM_MAX_OBS || n_steps < 1 || n_steps > JSIM_MAX_PRED)
        return fail(ctx, -22, "jsim_loop_predict_obstacles: n_obs=%d (max %d), n_steps=%d (max %d)", n_obs, JSIM_MAX_OBS, n_steps, JSIM_MAX_PRED);
    if (int rc = check_shapes(ctx, "jsim_loop_predict_obstacles", n_obs)) return rc;
    ctx->pred_n_obs = n_obs; ctx->pred_n_steps = n_steps;
    if (n_obs == 0) return 0;
    if (!obst || !pred) return fail(ctx, -22, "jsim_loop_predict_obstacles: null device pointer");
    launch_obstacle_predict(ctx, n_obs, n_steps, obst, pred, ctx->d_pred_cc, ctx->d_pred_bc, 1, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int jsim_loop_pre_tick(jsim_ctx *ctx, int32_t B, const double *x0, const int32_t *path_id, int64_t *traj_idx,
                                  const int32_t *prev_path_len, int32_t *path_len, int32_t *col_flag, double *col_xy,
                                  int32_t *first_idx, int32_t *status, int32_t frame_window, int32_t margin,
                                  int32_t *dbg_res_idx, int32_t *dbg_n_res, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_pre_tick: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0 || frame_window < 0 || frame_window > 32 || margin < 0) return fail(ctx, -22, "jsim_loop_pre_tick: bad argument");
    if (B == 0) return 0;
    if (!x0 || !path_id || !traj_idx || !prev_path_len || !path_len || !col_flag || !status)
        return fail(ctx, -22, "jsim_loop_pre_tick: null device pointer");
    if (!ctx->d_pxy || !ctx->d_pcc) return fail(ctx, -22, "jsim_loop_pre_tick: paths / geometry not set");
    if (dbg_res_idx && !dbg_n_res) return fail(ctx, -22, "jsim_loop_pre_tick: dbg_res_idx needs dbg_n_res");
    if (int rc = check_shapes(ctx, "jsim_loop_pre_tick", ctx->pred_n_obs)) return rc;
    ctx->glue_path_id = path_id; ctx->glue_B = B;
    PreP P = fill_prep(ctx, B, ctx->pred_n_obs, ctx->pred_n_steps, frame_window, margin);
    P.x0 = x0; P.path_id = path_id; P.traj_idx = (long long *)traj_idx; P.prev_path_len = prev_path_len; P.path_len = path_len;
    P.col_flag = col_flag; P.col_xy = col_xy; P.first_idx = first_idx; P.status = status;
    P.dbg_res_idx = dbg_res_idx; P.dbg_n_res = dbg_n_res;
    hipLaunchKernelGGL(loop_pre_tick_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, P, TrafficP{});
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ---- MPC variants of the reference that differ from main/lib/mpc.py only in data ----
extern "C" int jsim_mpc_set_path_speed(jsim_ctx *ctx, const double *cv)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_set_path_speed: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    ctx->d_pcv.release();
    if (!cv) return 0; // back to the plain controller (no speed reference)
    if (ctx->n_points <= 0) return fail(ctx, -22, "jsim_mpc_set_path_speed: call jsim_mpc_set_paths first");
    HIP_TRY(ctx, ctx->d_pcv.reserve(ctx->n_points));
    HIP_TRY(ctx, hipMemcpy(ctx->d_pcv, cv, sizeof(double) * ctx->n_points, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int jsim_mpc_set_speed_cutoff(jsim_ctx *ctx, const int32_t *cv_cut)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_set_speed_cutoff: null ctx");
    ctx->cv_cut = cv_cut;
    return 0;
}

extern "C" int jsim_mpc_update_cfg(jsim_ctx *ctx, const jsim_cfg *cfg)
{
    if (!ctx || !cfg) return fail(ctx, -22, "jsim_mpc_update_cfg: null argument");
    if (cfg->T != ctx->cfg.T) return fail(ctx, -22, "jsim_mpc_update_cfg: the horizon cannot change (T=%d -> %d)", ctx->cfg.T, cfg->T);
    if (cfg->nx != ctx->cfg.nx) return fail(ctx, -22, "jsim_mpc_update_cfg: NX cannot change (%d -> %d)", ctx->cfg.nx, cfg->nx);
    if (cfg->max_iter < 1 || cfg->max_iter > 16) return fail(ctx, -22, "jsim_mpc_update_cfg: MAX_ITER=%d (1..16)", cfg->max_iter);
    if (!(cfg->dt > 0) || !(cfg->dl > 0) || !(cfg->L > 0) || !(cfg->R[0] > 0) || !(cfg->R[1] > 0) || !(cfg->R_end[0] > 0) ||
        !(cfg->R_end[1] > 0))
        return fail(ctx, -22, "jsim_mpc_update_cfg: dt, dl, L, R, R_end must be positive");
    ctx->cfg = *cfg;
    return 0;
}

extern "C" int jsim_mpc_set_ego_config(jsim_ctx *ctx, const double *cfg)
{
    if (!ctx) return fail(nullptr, -22, "jsim_mpc_set_ego_config: null ctx");
    ctx->d_pe = cfg;
    return 0;
}

extern "C" int jsim_loop_obstacles(jsim_ctx *ctx, int32_t n_obs, double *state, const double *param, double *get, int32_t do_step,
                                   void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_obstacles: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (n_obs < 0 || n_obs > JSIM_MAX_OBS) return fail(ctx, -22, "jsim_loop_obstacles: n_obs=%d (max %d)", n_obs, JSIM_MAX_OBS);
    if (n_obs == 0) return 0;
    if (int rc = check_shapes(ctx, "jsim_loop_obstacles", n_obs)) return rc;
    if (!state || !param) return fail(ctx, -22, "jsim_loop_obstacles: null device pointer");
    launch_obstacle_step(obstacle_step_p(ctx, n_obs, do_step ? 1 : 0, state, param, get), (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// an ego that was just respawned (age == 0 after the advance) starts its run like a new one: progress index 0, no previous path
__global__ __launch_bounds__(256) void glue_reset_kernel(int B, const int *age, long long *traj_idx, int *prev_len)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && age[b] == 0) { traj_idx[b] = 0; prev_len[b] = -1; }
}

// the egos' predictions (circle centres, bounding circles), sized on first use
static int ensure_ego_pred(jsim_ctx *ctx, int B, int n_steps)
{
    HIP_TRY(ctx, ctx->d_ego_cc.reserve((size_t)B * n_steps * 2));
    HIP_TRY(ctx, ctx->d_ego_bc.reserve(B));
    return 0;
}

static void launch_ego_predict(jsim_ctx *ctx, int B, const double *x0, const double *di_ai, int n_steps, double *pred, hipStream_t s)
{
    EgoPredP P = {B, n_steps, ctx->cfg.dt, ctx->cfg.L, ctx->cc0, ctx->cc1, x0, di_ai, pred, ctx->d_ego_cc, ctx->d_ego_bc};
    hipLaunchKernelGGL(ego_predict_kernel, dim3((B + 63) / 64), dim3(64), 0, s, P);   // one wave per block: spread over the CUs
}

// where the glue's cut-off index goes: the controller's speed cut-off (jsim_mpc_set_speed_cutoff), or the path length
static int32_t *glue_out(const jsim_ctx *ctx, const StepBufs &S, const GlueBufs &G)
{
    return const_cast<int32_t *>(G.speed_cutoff ? ctx->cv_cut : S.path_len);
}

// the egos' predictions under the plan rule (JSIM_MATE_PLAN): one wavefront per ego, wheelbase and clamps as plant_p's
static void launch_ego_plan_predict(jsim_ctx *ctx, int B, const double *x0, const double *oa, const double *od, const int32_t *status,
                                    const double *di_ai, int n_steps, double *pred, hipStream_t s)
{
    const jsim_cfg &c = ctx->cfg;
    EgoPlanP P = {B, n_steps, c.T, c.dt, c.L, c.max_steer, c.max_speed, c.min_speed, ctx->cc0, ctx->cc1, x0, oa, od, status, di_ai,
                  pred, ctx->d_ego_cc, ctx->d_ego_bc};
    hipLaunchKernelGGL(ego_plan_predict_kernel, dim3(B), dim3(64), 0, s, P);
}

#include "plan_predictions.inc" // the plan recorder's and the plan scorer's parameters; their kernels are jsim_plan.hip's

enum class Glue { none, scripted, interacting };

// n_ticks ticks as separate launches, the calls the tick() methods of closed_loop.py make.  With a glue (G): scripted obstacles
// get() -> their prediction -> [interacting: every ego's prediction from the tick-start states ->] glue per ego against the
// scripted obstacles [, then its group mates] -> previous path length -> MPC.step -> plant, history, goal / respawn -> glue reset
// of respawned egos -> obstacles step().  Without one: MPC.step -> plant, history, goal / respawn.
static int run_host_ticks(jsim_ctx *ctx, int B, int n_ticks, const StepBufs &S, const AdvanceBufs &A, const GlueBufs *G,
                          Glue kind, hipStream_t s)
{
    KP P = fill_kp(ctx, B, S);
    PreP Q = {};
    GroupP GP = {};
    const TrafficP X = G ? traffic_p(ctx) : TrafficP{};
    const bool traffic = X.set_of != nullptr; // traffic sets: the predictions of all sets' vehicles do not fit the single-tick tables
    if (traffic) {
        HIP_TRY(ctx, ctx->d_pred_all.reserve((size_t)std::max(G->n_obs, 1) * G->n_steps * 2));
        HIP_TRY(ctx, ctx->d_bc_all.reserve(std::max(G->n_obs, 1)));
    }
    double2 *const pred_cc = traffic ? ctx->d_pred_all : ctx->d_pred_cc;
    double4 *const pred_bc = traffic ? ctx->d_bc_all : ctx->d_pred_bc;
    if (G) {
        Q = fill_prep(ctx, B, G->n_obs, G->n_steps, G->frame_window, G->margin);
        Q.x0 = S.x0; Q.path_id = S.path_id; Q.traj_idx = (long long *)G->traj_idx; Q.prev_path_len = G->prev_path_len;
        Q.path_len = glue_out(ctx, S, *G); Q.col_flag = G->col_flag; Q.status = G->pre_status;
        Q.pred_cc = pred_cc; Q.pred_bc = pred_bc;
        const double mate_thr = 2.0 * ctx->col_radius; // check_collision_moving_cars between two egos
        GP = GroupP{ctx->d_group_of, ctx->d_group_off, ctx->d_ego_cc, ctx->d_ego_bc, G->n_obs, mate_thr, jsim_sqrt_threshold(mate_thr)};
    }
    auto obstacles = [&](int do_step) { // get(), or get() then step()
        if (G->n_obs == 0) return;
        launch_obstacle_step(obstacle_step_rec_p(ctx, G->n_obs, do_step, G->obs_state, G->obs_param, G->obs_get, A.tick), s);
    };
    // every tick's iteration counts go onto the totals (jsim_mpc_iter_totals): the caller's n_iter, or the context's own
    if (int rc = prepare_iter_totals(ctx, B, s)) return rc;
    if (!P.n_iter) {
        HIP_TRY(ctx, ctx->d_n_iter.reserve(B));
        P.n_iter = ctx->d_n_iter;
    }
    for (int k = 0; k < n_ticks; ++k) {
        if (G) {
            obstacles(0);
            // (traffic sets: no single-tick prediction of at most JSIM_MAX_OBS obstacles is left for jsim_loop_pre_tick)
            ctx->pred_n_obs = traffic ? 0 : G->n_obs; ctx->pred_n_steps = G->n_steps;
            if (G->n_obs > 0) launch_obstacle_predict(ctx, G->n_obs, G->n_steps, G->obs_get, nullptr, pred_cc, pred_bc, 1, s);
            if (kind == Glue::interacting) {
                if (ctx->plan_oa) {
                    const PlanRecP PR = {B, ctx->cfg.T, ctx->rec_cap, A.tick, S.oa, S.od, S.status, ctx->plan_oa, ctx->plan_od,
                                         ctx->plan_status};
                    hipLaunchKernelGGL(plan_record_kernel, dim3((unsigned)(((size_t)B * ctx->cfg.T + 255) / 256)), dim3(256), 0, s, PR);
                }
                if (ctx->mate_prediction == JSIM_MATE_PLAN)
                    launch_ego_plan_predict(ctx, B, S.x0, S.oa, S.od, S.status, A.di_ai, G->n_steps, nullptr, s);
                else
                    launch_ego_predict(ctx, B, S.x0, A.di_ai, G->n_steps, nullptr, s);
                hipLaunchKernelGGL(group_pre_tick_kernel, dim3(B), dim3(64), 0, s, Q, GP, X);
            } else {
                hipLaunchKernelGGL(loop_pre_tick_kernel, dim3(B), dim3(64), 0, s, Q, X);
            }
            // the previous tmp_trajectory: the truncated path, or always the full one (mpc_intersection_new_ref.py:131)
            HIP_TRY(ctx, hipMemcpyAsync(G->prev_path_len, S.path_len, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
        }
        launch_step(ctx, P, s);
        hipLaunchKernelGGL(iters_add_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, P.n_iter, ctx->d_iters.p);
        launch_advance(ctx, B, S, A, s);
        if (G) {
            hipLaunchKernelGGL(glue_reset_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, A.age, (long long *)G->traj_idx,
                               G->prev_path_len);
            obstacles(1);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// The fused K-tick register kernel runs the ticks when the horizon has one, MAX_ITER is 1, and a registered speed cut-off is
// the glue's own output; otherwise run_host_ticks does.
static bool fused_ticks(const jsim_ctx *ctx, const GlueBufs *G)
{
    return ctx->use_reg_kernel && ctx->cfg.max_iter == 1 && !(G && ctx->cv_cut && !G->speed_cutoff);
}

// One fused launch of n_ticks ticks: each ego's wavefront runs [glue (Q) ->] MPC.step -> plant, history, goal / respawn.
static int launch_fused(jsim_ctx *ctx, int B, int n_ticks, const StepBufs &S, const AdvanceBufs &A, const PreK *Q, hipStream_t s)
{
    const jsim_cfg &c = ctx->cfg;
    KP P = fill_kp(ctx, B, S);
#ifndef JSIM_STAMPS /* (a stamped build keeps its clock rows in the fused launch: they then hold the launch's last tick) */
    P.dbg_clk = nullptr;
#endif
    TickP K;
    memset(&K, 0, sizeof(K));
    K.n_ticks = n_ticks; K.advance = 1; K.max_age = A.max_age > 0 ? A.max_age : 0x7fffffff; K.hist_cap = A.hist_cap;
    K.max_decel = c.max_decel; K.goal_dis = c.goal_dis; K.stop_speed = c.stop_speed;
    K.x0w = S.x0; K.di_ai = A.di_ai; K.x0_spawn = A.x0_spawn; K.target_spawn = (const long long *)A.target_spawn; K.age = A.age;
    K.hist = A.hist; K.tick = A.tick; K.n_respawn = (unsigned long long *)A.n_respawn;
    K.rec = ctx->rec; K.rec_flags = ctx->rec_flags; K.rec_cap = ctx->rec_cap;
    if (int rc = prepare_launch_order(ctx, B, s, K)) return rc;
    if (int rc = prepare_iter_totals(ctx, B, s)) return rc;
    K.iters = ctx->d_iters;
    launch_reg(c.T, B, s, P, K, Q);
    if (A.tick) hipLaunchKernelGGL(tick_add_kernel, dim3(1), dim3(1), 0, s, A.tick, n_ticks);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int jsim_mpc_run_ticks(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id,
                                  const int32_t *path_len, const double *speed, int64_t *target_ind, double *oa,
                                  double *od, double *ox, double *oy, double *ov, double *oyaw, double *xref,
                                  uint32_t *active_mask, int32_t *status, int32_t *n_iter, double *di_ai,
                                  const double *x0_spawn, const int64_t *target_spawn, int32_t *age, int32_t max_age,
                                  double *hist, int32_t *tick, int32_t hist_cap, uint64_t *n_respawn, void *stream)
{
    const char *const F = "jsim_mpc_run_ticks";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0 || n_ticks < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d", F, B, n_ticks);
    if (B == 0 || n_ticks == 0) return 0;
    const StepBufs S = {x0, path_id, path_len, speed, target_ind, oa, od, ox, oy, ov, oyaw, xref, active_mask, status, n_iter};
    const AdvanceBufs A = {di_ai, x0_spawn, target_spawn, age, max_age, hist, tick, hist_cap, n_respawn};
    if (int rc = check_step(ctx, F, S)) return rc;
    if (int rc = check_advance(ctx, F, A)) return rc;
    if (int rc = check_recorder(ctx, F, B, tick, -1)) return rc;
    if (!fused_ticks(ctx, nullptr)) return run_host_ticks(ctx, B, n_ticks, S, A, nullptr, Glue::none, (hipStream_t)stream);
    return launch_fused(ctx, B, n_ticks, S, A, nullptr, (hipStream_t)stream);
}

// Traffic sets: the fused scenario run lays out every tick's predictions of all sets' vehicles up front, total x n_steps x 32 B
// per tick (plus 80 B per vehicle of get() tuples and bounding circles) -- 4096 egos x 4 vehicles x 35 steps: 19 MB a tick.  It
// splits n_ticks into fused launches of at most this many bytes of tables each, unless jsim_loop_set_traffic forced a chunk.
#define JSIM_TRAFFIC_BUDGET (512ull << 20)

static int traffic_chunk_ticks(const jsim_ctx *ctx, int n_obs, int n_steps, int n_ticks)
{
    if (ctx->traffic_chunk > 0) return std::min(ctx->traffic_chunk, n_ticks);
    const unsigned long long per_tick = (unsigned long long)std::max(n_obs, 1) * ((unsigned long long)n_steps * 32 + 32 + 48);
    return (int)std::max(1ull, std::min((unsigned long long)n_ticks, JSIM_TRAFFIC_BUDGET / per_tick));
}

// A registered traffic layout must be the run's: the same B, and n_obs = all sets' vehicles
static int check_traffic(jsim_ctx *ctx, const char *fn, int B, int n_obs)
{
    if (ctx->traffic_B != B)
        return fail(ctx, -22, "%s: the traffic layout (jsim_loop_set_traffic) is for B=%d, not B=%d", fn, ctx->traffic_B, B);
    if (n_obs != ctx->h_obs_off[ctx->n_sets])
        return fail(ctx, -22, "%s: n_obs=%d, but the traffic sets hold %d vehicles", fn, n_obs, ctx->h_obs_off[ctx->n_sets]);
    return 0;
}

// The whole scenario loop (main/scenarios/mpc_intersection.py:99-163) for n_ticks ticks.  With a one-wave register kernel and
// one linearisation pass it is THREE launches: the scripted obstacles rolled forward n_ticks ticks (they do not depend on the
// egos), their predictions for every tick, and the fused K-tick kernel with the loop glue inside each ego's tick loop.  With
// traffic sets, the same three per chunk of traffic_chunk_ticks ticks.
// Otherwise the same ticks as the separate calls a host loop would make.
extern "C" int jsim_loop_run_scenario(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id,
                                      int32_t *path_len, const double *speed, int64_t *target_ind, double *oa, double *od,
                                      double *ox, double *oy, double *ov, double *oyaw, double *xref, uint32_t *active_mask,
                                      int32_t *status, int32_t *n_iter, double *di_ai, const double *x0_spawn,
                                      const int64_t *target_spawn, int32_t *age, int32_t max_age, double *hist, int32_t *tick,
                                      int32_t hist_cap, uint64_t *n_respawn, int64_t *traj_idx, int32_t *prev_path_len,
                                      int32_t *col_flag, int32_t *pre_status, int32_t frame_window, int32_t margin,
                                      int32_t n_obs, double *obs_state, const double *obs_param, double *obs_get,
                                      int32_t n_steps, int32_t speed_cutoff, void *stream)
{
    const char *const F = "jsim_loop_run_scenario";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0 || n_ticks < 0 || frame_window < 0 || frame_window > 32 || margin < 0) return fail(ctx, -22, "%s: bad argument", F);
    if (B == 0 || n_ticks == 0) return 0;
    const StepBufs S = {x0, path_id, path_len, speed, target_ind, oa, od, ox, oy, ov, oyaw, xref, active_mask, status, n_iter};
    const AdvanceBufs A = {di_ai, x0_spawn, target_spawn, age, max_age, hist, tick, hist_cap, n_respawn};
    const GlueBufs G = {traj_idx, prev_path_len, col_flag, pre_status, frame_window, margin, n_obs, obs_state, obs_param, obs_get,
                        n_steps, speed_cutoff};
    if (int rc = check_step(ctx, F, S)) return rc;
    if (int rc = check_advance(ctx, F, A)) return rc;
    if (int rc = check_recorder(ctx, F, B, tick, n_obs)) return rc;
    const bool traffic = ctx->n_sets > 0;
    if (n_steps < 1 || n_steps > JSIM_MAX_PRED || (traffic ? n_obs < 0 : (n_obs < 0 || n_obs > JSIM_MAX_OBS)))
        return fail(ctx, -22, "%s: n_obs=%d (max %d), n_steps=%d (max %d)", F, n_obs, JSIM_MAX_OBS, n_steps, JSIM_MAX_PRED);
    if (traffic)
        if (int rc = check_traffic(ctx, F, B, n_obs)) return rc;
    if (int rc = check_shapes(ctx, F, n_obs)) return rc;
    if (int rc = check_glue(ctx, F, G)) return rc;
    if (speed_cutoff && !ctx->cv_cut) return fail(ctx, -22, "%s: the speed-cut-off glue needs jsim_mpc_set_speed_cutoff first", F);
    ctx->glue_path_id = path_id; ctx->glue_B = B;
    hipStream_t s = (hipStream_t)stream;
    if (!fused_ticks(ctx, &G)) return run_host_ticks(ctx, B, n_ticks, S, A, &G, Glue::scripted, s);
    // obstacles: a chunk's ticks of get() tuples, then every tick's prediction, then the chunk's fused launch; the obstacle
    // state and obs_get carry over from chunk to chunk (without traffic sets: one chunk)
    const int chunk = traffic ? traffic_chunk_ticks(ctx, n_obs, n_steps, n_ticks) : n_ticks;
    const size_t obs_ticks = (size_t)chunk * (n_obs > 0 ? n_obs : 1);
    HIP_TRY(ctx, ctx->d_get_all.reserve(obs_ticks * 6));
    HIP_TRY(ctx, ctx->d_pred_all.reserve(obs_ticks * n_steps * 2));
    HIP_TRY(ctx, ctx->d_bc_all.reserve(obs_ticks));
    ctx->pred_n_obs = traffic ? 0 : n_obs; ctx->pred_n_steps = n_steps;
    PreK Q;
    memset(&Q, 0, sizeof(Q));
    Q.pre = fill_prep(ctx, B, n_obs, n_steps, frame_window, margin);
    Q.pred_cc_all = ctx->d_pred_all; Q.pred_bc_all = ctx->d_bc_all; Q.traj_idx = (long long *)traj_idx; Q.prev_len = prev_path_len; Q.path_len_out = path_len;
    Q.col_flag = col_flag; Q.pre_status = pre_status;
    Q.speed_cutoff = speed_cutoff ? 1 : 0; Q.cut_io = glue_out(ctx, S, G);
    Q.traffic = traffic_p(ctx);
    for (int k0 = 0; k0 < n_ticks; k0 += chunk) {
        const int nk = std::min(chunk, n_ticks - k0);
        if (n_obs > 0) {
            launch_obstacle_rollout(obstacle_step_rec_p(ctx, n_obs, 1, obs_state, obs_param, nullptr, tick), nk, ctx->d_get_all, s);
            launch_obstacle_predict(ctx, n_obs, n_steps, ctx->d_get_all, nullptr, ctx->d_pred_all, ctx->d_bc_all, nk, s);
            // the last get() tuples, as after nk host ticks
            HIP_TRY(ctx, hipMemcpyAsync(obs_get, ctx->d_get_all + (size_t)(nk - 1) * n_obs * 6, sizeof(double) * n_obs * 6,
                                        hipMemcpyDeviceToDevice, s));
        }
        if (int rc = launch_fused(ctx, B, nk, S, A, &Q, s)) return rc;
    }
    return 0;
}

// ---- Interacting egos: the obstacles of an ego are the scripted vehicles and the other egos of its group ----
extern "C" int jsim_loop_set_groups(jsim_ctx *ctx, int32_t B, int32_t n_groups, const int32_t *group_off)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_set_groups: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (n_groups < 0 || B < 0) return fail(ctx, -22, "jsim_loop_set_groups: B=%d n_groups=%d", B, n_groups);
    if (n_groups > 0) {
        if (!group_off) return fail(ctx, -22, "jsim_loop_set_groups: null group_off");
        if (group_off[0] != 0 || group_off[n_groups] != B)
            return fail(ctx, -22, "jsim_loop_set_groups: group_off must run from 0 to B=%d (got %d .. %d)", B, group_off[0],
                        group_off[n_groups]);
        for (int g = 0; g < n_groups; ++g) {
            const int n = group_off[g + 1] - group_off[g];
            if (n < 1 || n > JSIM_MAX_OBS)
                return fail(ctx, -22, "jsim_loop_set_groups: group %d has %d egos (1..%d)", g, n, JSIM_MAX_OBS);
        }
    }
    ctx->d_group_of.release(); ctx->d_group_off.release(); ctx->h_group_off.clear();
    ctx->group_B = 0; ctx->n_groups = 0; ctx->group_max = 0;
    if (n_groups == 0) return 0;
    std::vector<int> of((size_t)B);
    int gmax = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int b = group_off[g]; b < group_off[g + 1]; ++b) of[b] = g;
        gmax = std::max(gmax, group_off[g + 1] - group_off[g]);
    }
    HIP_TRY(ctx, ctx->d_group_of.reserve(B));
    HIP_TRY(ctx, ctx->d_group_off.reserve(n_groups + 1));
    HIP_TRY(ctx, hipMemcpy(ctx->d_group_of, of.data(), sizeof(int) * B, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_group_off, group_off, sizeof(int) * (n_groups + 1), hipMemcpyHostToDevice));
    ctx->h_group_off.assign(group_off, group_off + n_groups + 1);
    ctx->group_B = B; ctx->n_groups = n_groups; ctx->group_max = gmax;
    return 0;
}

// ---- Traffic sets: each ego meets the scripted vehicles of its own set ----
extern "C" int jsim_loop_set_traffic(jsim_ctx *ctx, int32_t B, int32_t n_sets, const int32_t *set_of, const int32_t *obs_off,
                                     int32_t chunk_ticks)
{
    const char *const F = "jsim_loop_set_traffic";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0 || n_sets < 0 || chunk_ticks < 0) return fail(ctx, -22, "%s: B=%d n_sets=%d chunk_ticks=%d", F, B, n_sets, chunk_ticks);
    if (n_sets > 0) {
        if (!obs_off || (B > 0 && !set_of)) return fail(ctx, -22, "%s: null set_of / obs_off", F);
        if (obs_off[0] != 0) return fail(ctx, -22, "%s: obs_off must start at 0 (got %d)", F, obs_off[0]);
        for (int k = 0; k < n_sets; ++k) {
            const long long n = (long long)obs_off[k + 1] - obs_off[k];
            if (n < 0) return fail(ctx, -22, "%s: obs_off decreases at set %d (%d -> %d)", F, k, obs_off[k], obs_off[k + 1]);
            if (n > JSIM_MAX_OBS) return fail(ctx, -22, "%s: set %d has %lld vehicles (max %d)", F, k, n, JSIM_MAX_OBS);
        }
        for (int b = 0; b < B; ++b)
            if (set_of[b] < 0 || set_of[b] >= n_sets)
                return fail(ctx, -22, "%s: set_of[%d] = %d is not a set (0..%d)", F, b, set_of[b], n_sets - 1);
    }
    ctx->d_set_of.release(); ctx->d_obs_off.release(); ctx->h_set_of.clear(); ctx->h_obs_off.clear();
    ctx->traffic_B = 0; ctx->n_sets = 0; ctx->traffic_chunk = 0;
    if (n_sets == 0) return 0;
    HIP_TRY(ctx, ctx->d_set_of.reserve(std::max(B, 1)));
    HIP_TRY(ctx, ctx->d_obs_off.reserve(n_sets + 1));
    if (B > 0) HIP_TRY(ctx, hipMemcpy(ctx->d_set_of, set_of, sizeof(int) * B, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_obs_off, obs_off, sizeof(int) * (n_sets + 1), hipMemcpyHostToDevice));
    ctx->h_set_of.assign(set_of, set_of + B);
    ctx->h_obs_off.assign(obs_off, obs_off + n_sets + 1);
    ctx->traffic_B = B; ctx->n_sets = n_sets; ctx->traffic_chunk = chunk_ticks;
    return 0;
}

// ---- The History recorder: the loop entry points write each ego's per-tick record where the state lives ----
extern "C" int jsim_loop_set_recorder(jsim_ctx *ctx, int32_t B, int32_t cap, double *rec, int32_t *flags, int32_t n_obs,
                                      double *obs_rec)
{
    const char *const F = "jsim_loop_set_recorder";
    // (the argument checks come first: they need no context and no device)
    if (B < 0 || cap < 0 || n_obs < 0) return fail(ctx, -22, "%s: B=%d cap=%d n_obs=%d", F, B, cap, n_obs);
    if (cap > 0 && (!rec || !flags)) return fail(ctx, -22, "%s: cap=%d needs the rec and flags buffers", F, cap);
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    if (n_obs == 0) obs_rec = nullptr; // (no vehicles recorded)
    if (cap > 0 && obs_rec && ctx->n_sets > 0 && n_obs != ctx->h_obs_off[ctx->n_sets])
        return fail(ctx, -22, "%s: n_obs=%d, but the traffic sets hold %d vehicles", F, n_obs, ctx->h_obs_off[ctx->n_sets]);
    ctx->rec = nullptr; ctx->rec_flags = nullptr; ctx->rec_obs = nullptr;
    ctx->rec_B = 0; ctx->rec_cap = 0; ctx->rec_n_obs = 0;
    ctx->plan_oa = nullptr; ctx->plan_od = nullptr; ctx->plan_status = nullptr; // (a plan recorder goes with the recorder it was sized by)
    if (cap == 0) return 0;
    ctx->rec = rec; ctx->rec_flags = flags; ctx->rec_cap = cap; ctx->rec_B = B;
    if (obs_rec) { ctx->rec_obs = obs_rec; ctx->rec_n_obs = n_obs; }
    return 0;
}

// ---- The plan recorder: jsim_loop_run_interacting keeps every tick's shared plans beside the History ----
extern "C" int jsim_loop_set_plan_recorder(jsim_ctx *ctx, int32_t B, int32_t cap, double *plan_oa, double *plan_od, int32_t *plan_status)
{
    const char *const F = "jsim_loop_set_plan_recorder";
    if (B < 0 || cap < 0) return fail(ctx, -22, "%s: B=%d cap=%d", F, B, cap);
    if (cap > 0 && (!plan_oa || !plan_od || !plan_status)) return fail(ctx, -22, "%s: cap=%d needs the plan_oa, plan_od and plan_status buffers", F, cap);
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    if (cap > 0 && (!ctx->rec || ctx->rec_B != B || ctx->rec_cap != cap))
        return fail(ctx, -22, "%s: B=%d cap=%d, but the registered recorder (jsim_loop_set_recorder) has B=%d cap=%d", F, B, cap, ctx->rec_B,
                    ctx->rec_cap);
    ctx->plan_oa = nullptr; ctx->plan_od = nullptr; ctx->plan_status = nullptr;
    if (cap == 0) return 0;
    ctx->plan_oa = plan_oa; ctx->plan_od = plan_od; ctx->plan_status = plan_status;
    return 0;
}

extern "C" int jsim_loop_predict_egos(jsim_ctx *ctx, int32_t B, const double *x0, const double *di_ai, int32_t n_steps,
                                      double *pred, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_predict_egos: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!ctx->have_geom) return fail(ctx, -22, "jsim_loop_predict_egos: jsim_loop_set_geometry has not been called");
    if (B < 0 || n_steps < 1 || n_steps > JSIM_MAX_PRED)
        return fail(ctx, -22, "jsim_loop_predict_egos: B=%d, n_steps=%d (max %d)", B, n_steps, JSIM_MAX_PRED);
    if (B == 0) return 0;
    if (!x0 || !di_ai) return fail(ctx, -22, "jsim_loop_predict_egos: null device pointer");
    if (int rc = ensure_ego_pred(ctx, B, n_steps)) return rc;
    launch_ego_predict(ctx, B, x0, di_ai, n_steps, pred, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int jsim_loop_set_mate_prediction(jsim_ctx *ctx, int32_t mode)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_set_mate_prediction: null ctx");
    if (mode != JSIM_MATE_CONSTANT && mode != JSIM_MATE_PLAN)
        return fail(ctx, -22, "jsim_loop_set_mate_prediction: mode=%d (JSIM_MATE_CONSTANT %d or JSIM_MATE_PLAN %d)", mode,
                    JSIM_MATE_CONSTANT, JSIM_MATE_PLAN);
    ctx->mate_prediction = mode;
    return 0;
}

extern "C" int jsim_loop_predict_egos_plan(jsim_ctx *ctx, int32_t B, const double *x0, const double *oa, const double *od,
                                           const int32_t *status, const double *di_ai, int32_t n_steps, double *pred, void *stream)
{
    if (!ctx) return fail(nullptr, -22, "jsim_loop_predict_egos_plan: null ctx");
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (!ctx->have_geom) return fail(ctx, -22, "jsim_loop_predict_egos_plan: jsim_loop_set_geometry has not been called");
    if (B < 0 || n_steps < 1 || n_steps > JSIM_MAX_PRED)
        return fail(ctx, -22, "jsim_loop_predict_egos_plan: B=%d, n_steps=%d (max %d)", B, n_steps, JSIM_MAX_PRED);
    if (B == 0) return 0;
    if (!x0 || !oa || !od || !status || !di_ai) return fail(ctx, -22, "jsim_loop_predict_egos_plan: null device pointer");
    if (int rc = ensure_ego_pred(ctx, B, n_steps)) return rc;
    launch_ego_plan_predict(ctx, B, x0, oa, od, status, di_ai, n_steps, pred, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// What a glue over interacting egos needs of the context: registered groups for this B, scripted vehicles of the egos' shape or
// with a shape table, and room in the glue's obstacle table for every ego's vehicles and group mates
static int check_groups(jsim_ctx *ctx, const char *F, int B, int n_obs, int n_steps)
{
    if (ctx->have_ogeom && ctx->n_shapes == 0) // (a shape table gives the scripted vehicles their own thresholds beside the mates')
        return fail(ctx, -22, "%s: egos cannot be mixed with obstacles of another shape (jsim_loop_set_obstacle_geometry has been called)", F);
    if (ctx->n_groups == 0 || ctx->group_B != B) return fail(ctx, -22, "%s: no groups set for B=%d (jsim_loop_set_groups)", F, B);
    const bool traffic = ctx->n_sets > 0;
    if (n_obs < 0 || n_steps < 1 || n_steps > JSIM_MAX_PRED || (!traffic && n_obs + ctx->group_max - 1 > JSIM_MAX_OBS))
        return fail(ctx, -22, "%s: n_obs=%d + largest group %d - 1 > %d, or n_steps=%d (max %d)", F, n_obs, ctx->group_max,
                    JSIM_MAX_OBS, n_steps, JSIM_MAX_PRED);
    if (traffic) { // one set per group, and its vehicles + the group mates fit the glue's obstacle table
        if (int rc = check_traffic(ctx, F, B, n_obs)) return rc;
        for (int g = 0; g < ctx->n_groups; ++g) {
            const int b0 = ctx->h_group_off[g], b1 = ctx->h_group_off[g + 1], set = ctx->h_set_of[b0];
            for (int b = b0 + 1; b < b1; ++b)
                if (ctx->h_set_of[b] != set)
                    return fail(ctx, -22, "%s: group %d mixes traffic sets (ego %d: set %d, ego %d: set %d)", F, g, b0, set, b,
                                ctx->h_set_of[b]);
            const int n = ctx->h_obs_off[set + 1] - ctx->h_obs_off[set];
            if (n + (b1 - b0) - 1 > JSIM_MAX_OBS)
                return fail(ctx, -22, "%s: group %d: %d vehicles of set %d + %d group mates > %d", F, g, n, set, b1 - b0 - 1,
                            JSIM_MAX_OBS);
        }
    }
    return 0;
}

// n_ticks Jacobi ticks of interacting egos (main/scenarios/interactive_mpc.py:117-190), each as separate launches
// (run_host_ticks).  Arguments as jsim_loop_run_scenario; groups from jsim_loop_set_groups.
extern "C" int jsim_loop_run_interacting(jsim_ctx *ctx, int32_t B, int32_t n_ticks, double *x0, const int32_t *path_id,
                                         int32_t *path_len, const double *speed, int64_t *target_ind, double *oa, double *od,
                                         double *ox, double *oy, double *ov, double *oyaw, double *xref, uint32_t *active_mask,
                                         int32_t *status, int32_t *n_iter, double *di_ai, const double *x0_spawn,
                                         const int64_t *target_spawn, int32_t *age, int32_t max_age, double *hist, int32_t *tick,
                                         int32_t hist_cap, uint64_t *n_respawn, int64_t *traj_idx, int32_t *prev_path_len,
                                         int32_t *col_flag, int32_t *pre_status, int32_t frame_window, int32_t margin,
                                         int32_t n_obs, double *obs_state, const double *obs_param, double *obs_get,
                                         int32_t n_steps, int32_t speed_cutoff, void *stream)
{
    const char *const F = "jsim_loop_run_interacting";
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    if (B < 0 || n_ticks < 0 || frame_window < 0 || frame_window > 32 || margin < 0) return fail(ctx, -22, "%s: bad argument", F);
    if (speed_cutoff) return fail(ctx, -22, "%s: only the truncate glue is supported (speed_cutoff = 1)", F);
    if (int rc = check_groups(ctx, F, B, n_obs, n_steps)) return rc;
    if (int rc = check_shapes(ctx, F, n_obs)) return rc;
    if (B == 0 || n_ticks == 0) return 0;
    const StepBufs S = {x0, path_id, path_len, speed, target_ind, oa, od, ox, oy, ov, oyaw, xref, active_mask, status, n_iter};
    const AdvanceBufs A = {di_ai, x0_spawn, target_spawn, age, max_age, hist, tick, hist_cap, n_respawn};
    const GlueBufs G = {traj_idx, prev_path_len, col_flag, pre_status, frame_window, margin, n_obs, obs_state, obs_param, obs_get,
                        n_steps, speed_cutoff};
    if (int rc = check_step(ctx, F, S)) return rc;
    if (int rc = check_advance(ctx, F, A)) return rc;
    if (int rc = check_recorder(ctx, F, B, tick, n_obs)) return rc;
    if (int rc = check_glue(ctx, F, G)) return rc;
    ctx->glue_path_id = path_id; ctx->glue_B = B;
    if (int rc = ensure_ego_pred(ctx, B, n_steps)) return rc;
    return run_host_ticks(ctx, B, n_ticks, S, A, &G, Glue::interacting, (hipStream_t)stream);
}

#include "cutoff_ticks.inc"

// The collision cut-off of every recorded tick: DEVICE pointers, the recorder's buffers as they are; per
// chunk of ticks the vehicles' predictions, for interacting egos the mates' states and predictions, and one launch of one wavefront
// per ego that walks the chunk's ticks in order; all on `stream`.
// plan: the group mates are predicted under the plan rule from the recorded plans (jsim_loop_eval_cutoffs_plan), not the constant one
static int eval_cutoffs(const char *F, bool plan, jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                        int32_t n_obs, const double *obs_rec, const double *x_first, const double *x_spawn, int32_t frame_window,
                        int32_t margin, int32_t n_steps, int32_t speed_cutoff, int32_t interacting, int32_t chunk_ticks,
                        int32_t first_tick, int32_t *carry, int32_t *status, int32_t *idx, int32_t *cut, int32_t *hit, int32_t *first,
                        double *col_xy, const double *plan_oa, const double *plan_od, const int32_t *plan_status, void *stream)
{
    if (B < 0 || n_ticks < 0 || n_obs < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d n_obs=%d", F, B, n_ticks, n_obs);
    if (margin < 0 || chunk_ticks < 0) return fail(ctx, -22, "%s: margin=%d chunk_ticks=%d", F, margin, chunk_ticks);
    if (first_tick < 0 || first_tick > n_ticks) return fail(ctx, -22, "%s: first_tick=%d outside [0, n_ticks=%d]", F, first_tick, n_ticks);
    if (!obs_rec && n_obs > 0) return fail(ctx, -22, "%s: null obs_rec with n_obs=%d", F, n_obs);
    if (n_steps < 1 || n_steps > JSIM_MAX_PRED) return fail(ctx, -22, "%s: n_steps=%d outside [1, %d]", F, n_steps, JSIM_MAX_PRED);
    if (frame_window < 0 || frame_window > 32) return fail(ctx, -22, "%s: frame_window=%d outside [0, 32]", F, frame_window);
    if ((speed_cutoff != 0 && speed_cutoff != 1) || (interacting != 0 && interacting != 1))
        return fail(ctx, -22, "%s: speed_cutoff=%d interacting=%d (each 0 or 1)", F, speed_cutoff, interacting);
    if (speed_cutoff && interacting) return fail(ctx, -22, "%s: interacting egos have the truncate glue only (speed_cutoff=1)", F);
    if (!rec || !flags || !x_first || !x_spawn || !status || !idx || !cut || !hit || !first || !col_xy)
        return fail(ctx, -22, "%s: null device pointer", F);
    if (plan && (!plan_oa || !plan_od || !plan_status)) return fail(ctx, -22, "%s: null plan_oa / plan_od / plan_status", F);
    if (plan && !interacting) return fail(ctx, -22, "%s: interacting=0 (only interacting egos share plans)", F);
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    // the context's tables must be those of the loop that made the recording
    if (!ctx->d_pxy || !ctx->d_pcc || !ctx->have_geom) return fail(ctx, -22, "%s: paths / geometry not set", F);
    const bool traffic = ctx->n_sets > 0;
    if (traffic) {
        if (int rc = check_traffic(ctx, F, B, n_obs)) return rc;
    } else if (n_obs > JSIM_MAX_OBS) {
        return fail(ctx, -22, "%s: n_obs=%d (max %d without traffic sets)", F, n_obs, JSIM_MAX_OBS);
    }
    if (interacting)
        if (int rc = check_groups(ctx, F, B, n_obs, n_steps)) return rc;
    if (speed_cutoff && !ctx->cv_cut) return fail(ctx, -22, "%s: speed_cutoff=1 without a registered speed cut-off (jsim_mpc_set_speed_cutoff)", F);
    if (int rc = check_shapes(ctx, F, n_obs)) return rc;
    if (B == 0 || first_tick == n_ticks) return 0;
    if (!ctx->glue_path_id || ctx->glue_B != B) // (ticks, but no run of B egos: not this context's)
        return fail(ctx, -22, "%s: no glue call has bound the path ids of B=%d egos yet", F, B);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    hipStream_t s = (hipStream_t)stream;
    // ticks per chunk: the vehicles' predictions (as the fused run's chunks count them) and, interacting, every ego's own
    const unsigned long long per_tick = (unsigned long long)std::max(n_obs, 1) * ((unsigned long long)n_steps * 32 + 32) +
                                        (interacting ? (unsigned long long)B * ((unsigned long long)n_steps * 32 + 32 + 48) : 0ull);
    unsigned long long chunk = chunk_ticks > 0 ? (unsigned long long)chunk_ticks : std::max(1ull, JSIM_TRAFFIC_BUDGET / per_tick);
    chunk = std::min({chunk, (unsigned long long)(n_ticks - first_tick), 65535ull, std::max(1ull, (1ull << 30) / (unsigned long long)B)}); // (grid.y; rows as int)
    const int C = (int)chunk;
    const size_t obs_ticks = (size_t)C * std::max(n_obs, 1);
    HIP_TRY(ctx, ctx->d_pred_all.reserve(obs_ticks * n_steps * 2));
    HIP_TRY(ctx, ctx->d_bc_all.reserve(obs_ticks));
    if (interacting) {
        if (int rc = ensure_ego_pred(ctx, C * B, n_steps)) return rc;
        HIP_TRY(ctx, ctx->d_cut_x0.reserve((size_t)C * B * 4));
        HIP_TRY(ctx, ctx->d_cut_di.reserve((size_t)C * B * 2));
    }
    if (!carry) {
        HIP_TRY(ctx, ctx->d_cut_carry.reserve((size_t)B * JSIM_CUT_CARRY));
        hipLaunchKernelGGL(cutoff_carry_init_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, ctx->glue_path_id, ctx->d_poff.p,
                           ctx->d_cut_carry.p);
        carry = ctx->d_cut_carry;
    }
    CutoffP P;
    memset(&P, 0, sizeof(P));
    P.R = recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn);
    P.pre = fill_prep(ctx, B, n_obs, n_steps, frame_window, margin);
    P.pre.path_id = ctx->glue_path_id;
    P.X = traffic_p(ctx);
    const double mate_thr = 2.0 * ctx->col_radius;
    if (interacting)
        P.G = GroupP{ctx->d_group_of, ctx->d_group_off, ctx->d_ego_cc, ctx->d_ego_bc, n_obs, mate_thr, jsim_sqrt_threshold(mate_thr)};
    P.speed_cutoff = speed_cutoff; P.interacting = interacting;
    P.pred_cc = ctx->d_pred_all; P.pred_bc = ctx->d_bc_all;
    P.carry = carry; P.status = status; P.idx = idx; P.cut = cut; P.hit = hit; P.first = first; P.col_xy = col_xy;
    for (int k0 = first_tick; k0 < n_ticks; k0 += C) {
        const int nk = std::min(C, n_ticks - k0);
        if (n_obs > 0)
            launch_obstacle_predict(ctx, n_obs, n_steps, obs_rec + (size_t)k0 * n_obs * 6, nullptr, ctx->d_pred_all, ctx->d_bc_all, nk, s);
        if (interacting) {
            hipLaunchKernelGGL(cutoff_mate_state_kernel, dim3((unsigned)(((size_t)nk * B + 255) / 256)), dim3(256), 0, s, P.R, k0, nk,
                               ctx->d_cut_x0.p, ctx->d_cut_di.p);
            if (plan) // the chunk's slab of the plan record is a [nk * B][T] batch, row = tick * B + ego as the states'
                launch_ego_plan_predict(ctx, nk * B, ctx->d_cut_x0, plan_oa + (size_t)k0 * B * ctx->cfg.T, plan_od + (size_t)k0 * B * ctx->cfg.T,
                                        plan_status + (size_t)k0 * B, ctx->d_cut_di, n_steps, nullptr, s);
            else
                launch_ego_predict(ctx, nk * B, ctx->d_cut_x0, ctx->d_cut_di, n_steps, nullptr, s);
        }
        P.k0 = k0; P.C = nk;
        if (int rc = launch_per_ego(ctx, cutoff_ticks_kernel, B, stream, P)) return rc;
    }
    return 0;
}

extern "C" int jsim_loop_eval_cutoffs(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                      const double *obs_rec, const double *x_first, const double *x_spawn, int32_t frame_window,
                                      int32_t margin, int32_t n_steps, int32_t speed_cutoff, int32_t interacting, int32_t chunk_ticks,
                                      int32_t first_tick, int32_t *carry, int32_t *status, int32_t *idx, int32_t *cut, int32_t *hit, int32_t *first,
                                      double *col_xy, void *stream)
{
    return eval_cutoffs("jsim_loop_eval_cutoffs", false, ctx, B, n_ticks, rec, flags, n_obs, obs_rec, x_first, x_spawn, frame_window, margin,
                        n_steps, speed_cutoff, interacting, chunk_ticks, first_tick, carry, status, idx, cut, hit, first, col_xy, nullptr,
                        nullptr, nullptr, stream);
}

// The same for a recording of JSIM_MATE_PLAN: the mates' predictions are made again from the plan record
// (jsim_loop_set_plan_recorder's buffers [n_ticks][B][T], [n_ticks][B]) by ego_plan_predict_kernel, the kernel the loop ran.
extern "C" int jsim_loop_eval_cutoffs_plan(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                           const double *obs_rec, const double *x_first, const double *x_spawn, int32_t frame_window,
                                           int32_t margin, int32_t n_steps, int32_t speed_cutoff, int32_t interacting, int32_t chunk_ticks,
                                           int32_t first_tick, int32_t *carry, int32_t *status, int32_t *idx, int32_t *cut, int32_t *hit,
                                           int32_t *first, double *col_xy, const double *plan_oa, const double *plan_od,
                                           const int32_t *plan_status, void *stream)
{
    return eval_cutoffs("jsim_loop_eval_cutoffs_plan", true, ctx, B, n_ticks, rec, flags, n_obs, obs_rec, x_first, x_spawn, frame_window,
                        margin, n_steps, speed_cutoff, interacting, chunk_ticks, first_tick, carry, status, idx, cut, hit, first, col_xy,
                        plan_oa, plan_od, plan_status, stream);
}

#include "predictions.inc"

// Every recorded prediction against what the vehicle then did: DEVICE pointers throughout, the recorder's
// buffers as they are; one launch on `stream`, one wavefront per row (the recorded vehicles, then, with egos = 1, the egos).
extern "C" int jsim_loop_score_predictions(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, int32_t n_obs,
                                           const double *obs_rec, const double *x_first, const double *x_spawn, int32_t egos,
                                           int32_t n_steps, double tol, int32_t *pt_i, double *pt_d, double *step_sum, int32_t *step_cnt,
                                           double *err, void *stream)
{
    const char *const F = "jsim_loop_score_predictions";
    if (B < 0 || n_ticks < 0 || n_obs < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d n_obs=%d", F, B, n_ticks, n_obs);
    if (n_steps < 1 || n_steps > JSIM_MAX_PRED) return fail(ctx, -22, "%s: n_steps=%d outside [1, %d]", F, n_steps, JSIM_MAX_PRED);
    if (egos != 0 && egos != 1) return fail(ctx, -22, "%s: egos=%d (0 or 1)", F, egos);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, -22, "%s: tol %g is not finite and >= 0", F, tol);
    if (!obs_rec && n_obs > 0) return fail(ctx, -22, "%s: null obs_rec with n_obs=%d", F, n_obs);
    const void *const ptrs[] = {rec, flags, x_first, x_spawn, pt_i, pt_d, step_sum, step_cnt};
    const char *const names[] = {"rec", "flags", "x_first", "x_spawn", "pt_i", "pt_d", "step_sum", "step_cnt"};
    for (int i = 0; i < 8; ++i)
        if (!ptrs[i]) return fail(ctx, -22, "%s: null pointer %s", F, names[i]);
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    if (ctx->n_sets > 0)
        if (int rc = check_traffic(ctx, F, B, n_obs)) return rc;
    if (int rc = check_shapes(ctx, F, n_obs)) return rc;
    const long long V = (long long)n_obs + (egos ? B : 0);
    if (V == 0 || n_ticks == 0) return 0;
    if (V > 0x7fffffffll) return fail(ctx, -22, "%s: %lld rows", F, V);
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    const PredScoreP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), n_obs, egos, n_steps, ctx->cfg.dt,
                          ctx->have_ogeom ? ctx->oL : ctx->cfg.L, ctx->cfg.L, tol, obs_rec, n_obs > 0 ? shapes_p(ctx) : nullptr,
                          pt_i, pt_d, step_sum, step_cnt, err};
    return launch_per_ego(ctx, prediction_score_kernel, (int)V, stream, P);
}

static_assert(JPP_SLOTS == JPS_SLOTS, "plan_predictions.inc stages prediction_score_kernel's truth slots");

// Every recorded plan-rule prediction against what the ego then did: DEVICE pointers throughout, the
// recorder's and the plan recorder's buffers as they are; one launch on `stream`, one wavefront per ego.
extern "C" int jsim_loop_score_plan_predictions(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags,
                                                const double *x_first, const double *x_spawn, const double *plan_oa, const double *plan_od,
                                                const int32_t *plan_status, int32_t n_steps, double tol, int32_t *pt_i, double *pt_d,
                                                double *step_sum, int32_t *step_cnt, double *err, void *stream)
{
    const char *const F = "jsim_loop_score_plan_predictions";
    if (B < 0 || n_ticks < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d", F, B, n_ticks);
    if (n_steps < 1 || n_steps > JSIM_MAX_PRED) return fail(ctx, -22, "%s: n_steps=%d outside [1, %d]", F, n_steps, JSIM_MAX_PRED);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, -22, "%s: tol %g is not finite and >= 0", F, tol);
    const void *const ptrs[] = {rec, flags, x_first, x_spawn, plan_oa, plan_od, plan_status, pt_i, pt_d, step_sum, step_cnt};
    const char *const names[] = {"rec", "flags", "x_first", "x_spawn", "plan_oa", "plan_od", "plan_status", "pt_i", "pt_d", "step_sum", "step_cnt"};
    for (int i = 0; i < 11; ++i)
        if (!ptrs[i]) return fail(ctx, -22, "%s: null pointer %s", F, names[i]);
    if (!ctx) return fail(nullptr, -22, "%s: null ctx", F);
    const jsim_cfg &c = ctx->cfg; // (T <= JSIM_MAX_T, the tile's width, since jsim_mpc_create)
    if (B == 0 || n_ticks == 0) return 0;
    DeviceGuard dev_guard(ctx->device);
    JSIM_GUARD_OK(ctx);
    const PlanScoreP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), n_steps, c.T, c.dt, c.L, c.max_steer, c.max_speed,
                          c.min_speed, tol, plan_oa, plan_od, plan_status, pt_i, pt_d, step_sum, step_cnt, err};
    return launch_per_ego(ctx, plan_prediction_score_kernel, B, stream, P);
}

#include "fork.inc"

// The start of a loop forked off a recorded run: row r's ego state at the start of tick at[r] of ego ego[r]
// and the first tick of that tick's episode.  DEVICE pointers: the recorder's buffers and the two outputs; ego and at are HOST
// arrays, checked here and copied to the context's table; one launch on `stream`, one wavefront per row.
extern "C" int jsim_loop_fork_state(jsim_ctx *ctx, int32_t B, int32_t n_ticks, const double *rec, const int32_t *flags, const double *x_first,
                                    const double *x_spawn, int32_t n_rows, const int32_t *ego, const int32_t *at, double *x0, int32_t *k0,
                                    void *stream)
{
    const char *const F = "jsim_loop_fork_state";
    if (B < 0 || n_ticks < 0 || n_rows < 0) return fail(ctx, -22, "%s: B=%d n_ticks=%d n_rows=%d", F, B, n_ticks, n_rows);
    if (n_rows > 0 && (!rec || !flags || !x_first || !x_spawn || !ego || !at || !x0 || !k0)) return fail(ctx, -22, "%s: null pointer", F);
    for (int r = 0; r < n_rows; ++r) {
        if (ego[r] < 0 || ego[r] >= B) return fail(ctx, -22, "%s: row %d: ego=%d outside [0, B=%d)", F, r, ego[r], B);
        if (at[r] < 0 || at[r] > n_ticks) return fail(ctx, -22, "%s: row %d: at=%d outside [0, n_ticks=%d]", F, r, at[r], n_ticks);
    }
    JSIM_RECORDER_CALL(n_rows == 0);
    std::vector<int> rows((size_t)2 * n_rows);
    std::copy(ego, ego + n_rows, rows.begin());
    std::copy(at, at + n_rows, rows.begin() + n_rows);
    if (int rc = replace_table(ctx, ctx->d_fork_rows, rows.data(), rows.size())) return rc;
    const ForkStateP P = {recorder_buf(B, n_ticks, rec, flags, x_first, x_spawn), n_rows, ctx->d_fork_rows.p, ctx->d_fork_rows.p + n_rows, x0, k0};
    return launch_per_ego(ctx, fork_state_kernel, n_rows, stream, P);
}

// The scripted vehicles at their own ticks: DEVICE pointers state0, param, wheelbase (NULL: the wheelbase
// jsim_loop_obstacles steps with) and state; ticks is a HOST array; one launch on `stream`, one thread per vehicle.
extern "C" int jsim_loop_obstacles_at(jsim_ctx *ctx, int32_t n_obs, const double *state0, const double *param, const double *wheelbase,
                                      const int32_t *ticks, double *state, void *stream)
{
    const char *const F = "jsim_loop_obstacles_at";
    if (n_obs < 0) return fail(ctx, -22, "%s: n_obs=%d", F, n_obs);
    if (n_obs > 0 && (!state0 || !param || !ticks || !state)) return fail(ctx, -22, "%s: null pointer", F);
    for (int o = 0; o < n_obs; ++o)
        if (ticks[o] < 0) return fail(ctx, -22, "%s: vehicle %d: ticks=%d", F, o, ticks[o]);
    JSIM_RECORDER_CALL(n_obs == 0);
    if (int rc = replace_table(ctx, ctx->d_fork_ticks, ticks, (size_t)n_obs)) return rc;
    const ObsAtP P = {n_obs, ctx->have_ogeom ? ctx->oL : ctx->cfg.L, state0, param, wheelbase, ctx->d_fork_ticks.p, state,
                      ctx->n_routes > 0 ? ctx->d_route_pt.p : nullptr, ctx->n_routes > 0 ? ctx->d_route_off.p : nullptr, ctx->n_routes};
    hipLaunchKernelGGL(obstacles_at_kernel, dim3((n_obs + 63) / 64), dim3(64), 0, (hipStream_t)stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

#include "checkpoint.inc" // the checkpoint kernels' parameters; the kernels themselves are jsim_plan.hip's

static bool ckpt_aligned(const void *p) { return ((uintptr_t)p & 3u) == 0; }

// One slot of a loop's checkpoint slabs written, or read back: n_arrays copies of bytes[i] bytes from src[i] to
// dst[i] in ONE launch on `stream`.  src, dst and bytes are HOST arrays of DEVICE pointers and sizes; the table travels in the
// kernel's arguments, so the call neither allocates nor synchronises.
extern "C" int jsim_loop_checkpoint_save(jsim_ctx *ctx, int32_t n_arrays, const void *const *src, void *const *dst, const int64_t *bytes,
                                         void *stream)
{
    const char *const F = "jsim_loop_checkpoint_save";
    if (n_arrays < 0 || n_arrays > JSIM_CKPT_MAX_ARRAYS) return fail(ctx, -22, "%s: n_arrays=%d (0..%d)", F, n_arrays, JSIM_CKPT_MAX_ARRAYS);
    if (n_arrays > 0 && (!src || !dst || !bytes)) return fail(ctx, -22, "%s: null pointer", F);
    long long most = 0;
    for (int i = 0; i < n_arrays; ++i) {
        if (!src[i] || !dst[i]) return fail(ctx, -22, "%s: array %d: null pointer", F, i);
        if (bytes[i] < 0 || (bytes[i] & 3) || !ckpt_aligned(src[i]) || !ckpt_aligned(dst[i]))
            return fail(ctx, -22, "%s: array %d: bytes=%lld and both pointers must be multiples of 4", F, i, (long long)bytes[i]);
        most = std::max(most, (long long)bytes[i]);
    }
    JSIM_RECORDER_CALL(n_arrays == 0 || most == 0);
    CkptCopyP P;
    memset(&P, 0, sizeof(P));
    P.n = n_arrays;
    for (int i = 0; i < n_arrays; ++i) P.e[i] = CkptCopy{src[i], dst[i], (long long)bytes[i]};
    // the largest array in 16-byte words, one per thread, up to 64 blocks; the threads stride beyond that
    const unsigned gx = (unsigned)std::min<long long>(64, std::max<long long>(1, (most / 16 + 255) / 256));
    hipLaunchKernelGGL(checkpoint_copy_kernel, dim3(gx, (unsigned)n_arrays), dim3(256), 0, (hipStream_t)stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// Rows of written slots gathered into a new loop's buffers.  ctx is the NEW loop's context; B, n_slots and
// n_obs describe the slabs.  HOST arrays: written [n_slots], ego, slot [n_rows], slab, dst, row_bytes [n_fields] (DEVICE pointers
// and sizes), veh_src, veh_slot [n_veh].  DEVICE: what slab[i] and dst[i] point to, obs_slab, obs_state.  Two launches on `stream`.
extern "C" int jsim_loop_checkpoint_load(jsim_ctx *ctx, int32_t B, int32_t n_slots, const int32_t *written, int32_t n_rows, const int32_t *ego,
                                         const int32_t *slot, int32_t n_fields, const void *const *slab, void *const *dst,
                                         const int64_t *row_bytes, int32_t n_obs, const double *obs_slab, int32_t n_veh,
                                         const int32_t *veh_src, const int32_t *veh_slot, double *obs_state, void *stream)
{
    const char *const F = "jsim_loop_checkpoint_load";
    if (B < 0 || n_slots < 0 || n_rows < 0 || n_obs < 0 || n_veh < 0 || n_fields < 0 || n_fields > JSIM_CKPT_MAX_ARRAYS)
        return fail(ctx, -22, "%s: B=%d n_slots=%d n_rows=%d n_fields=%d (max %d) n_obs=%d n_veh=%d", F, B, n_slots, n_rows, n_fields,
                    JSIM_CKPT_MAX_ARRAYS, n_obs, n_veh);
    if ((n_slots > 0 && !written) || (n_rows > 0 && (!ego || !slot)) || (n_fields > 0 && (!slab || !dst || !row_bytes)) ||
        (n_veh > 0 && (!veh_src || !veh_slot || !obs_slab || !obs_state)))
        return fail(ctx, -22, "%s: null pointer", F);
    for (int i = 0; i < n_fields; ++i) {
        if (!slab[i] || !dst[i]) return fail(ctx, -22, "%s: field %d: null pointer", F, i);
        if (row_bytes[i] <= 0 || (row_bytes[i] & 3) || !ckpt_aligned(slab[i]) || !ckpt_aligned(dst[i]))
            return fail(ctx, -22, "%s: field %d: row_bytes=%lld and both pointers must be multiples of 4", F, i, (long long)row_bytes[i]);
    }
    auto is_written = [&](int s) { return s >= 0 && s < n_slots && written[s] != 0; };
    for (int r = 0; r < n_rows; ++r) {
        if (ego[r] < 0 || ego[r] >= B) return fail(ctx, -22, "%s: row %d: ego=%d outside [0, B=%d)", F, r, ego[r], B);
        if (!is_written(slot[r])) return fail(ctx, -22, "%s: row %d: slot=%d is not a written slot (n_slots=%d)", F, r, slot[r], n_slots);
    }
    for (int o = 0; o < n_veh; ++o) {
        if (veh_src[o] < 0 || veh_src[o] >= n_obs) return fail(ctx, -22, "%s: vehicle %d: source=%d outside [0, n_obs=%d)", F, o, veh_src[o], n_obs);
        if (!is_written(veh_slot[o])) return fail(ctx, -22, "%s: vehicle %d: slot=%d is not a written slot (n_slots=%d)", F, o, veh_slot[o], n_slots);
    }
    JSIM_RECORDER_CALL((n_rows == 0 || n_fields == 0) && n_veh == 0);
    std::vector<int> rows((size_t)2 * n_rows + (size_t)2 * n_veh);
    int *const h = rows.data();
    std::copy(ego, ego + n_rows, h);
    std::copy(slot, slot + n_rows, h + n_rows);
    std::copy(veh_src, veh_src + n_veh, h + 2 * (size_t)n_rows);
    std::copy(veh_slot, veh_slot + n_veh, h + 2 * (size_t)n_rows + n_veh);
    if (int rc = replace_table(ctx, ctx->d_ckpt_rows, rows.data(), rows.size())) return rc;
    const int *const d = ctx->d_ckpt_rows.p;
    if (n_rows > 0 && n_fields > 0) {
        CkptLoadP P;
        memset(&P, 0, sizeof(P));
        P.B = B; P.n_rows = n_rows; P.n_fields = n_fields; P.ego = d; P.slot = d + n_rows;
        for (int i = 0; i < n_fields; ++i) P.f[i] = CkptField{(const char *)slab[i], (char *)dst[i], (long long)row_bytes[i]};
        hipLaunchKernelGGL(checkpoint_load_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, P);
    }
    if (n_veh > 0) {
        const CkptVehP V = {n_veh, n_obs, d + 2 * (size_t)n_rows, d + 2 * (size_t)n_rows + n_veh, obs_slab, obs_state};
        hipLaunchKernelGGL(checkpoint_vehicles_kernel, dim3((unsigned)(((size_t)n_veh * 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
#endif /* !JSIM_KERNEL_TU */
