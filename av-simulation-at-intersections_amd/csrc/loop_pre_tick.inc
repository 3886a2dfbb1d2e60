// loop_pre_tick.inc -- the part of the per-vehicle loop that PRODUCES the truncated path for the MPC
// (SURVEY.md 8 row f1; included by jsim_mpc.hip).  One wavefront per ego.
//
//   main/scenarios/mpc_intersection.py:104-109   progress index on the full path (nearest index in direction)
//   :111-120  + lib/trajectories.py:58-86        ego path resampled as if accelerating at MAX_ACCEL up to MAX_SPEED
//   :122-126  + lib/moving_obstacles_prediction.py:21-47   obstacle prediction (obstacle_predict_kernel, once per tick)
//   :129      + lib/collision_avoidance.py:68-124 first colliding (frame, ego circle, obstacle copy, obstacle circle) row,
//                                                then first path point whose circle touches that obstacle circle
//   :133-140  + lib/collision_avoidance.py:168-180 first path index within 1 mm of the hit, minus margin, max(idx+1, .)
//
// All outputs are indices: the arithmetic follows numpy's operation order (sequential cumsum, unfused
// sqrt(dx*dx+dy*dy), floor of an IEEE division).  Circle centres of every path point are precomputed once on the
// host (jsim_loop_set_geometry) -- the path is static -- so the kernel evaluates no transcendental for the ego.

#define JSIM_MAX_RES 320   // kept points of a resampled ego path (<= ~150 for 720-point routes)

struct ObsP {
    int n_obs, n_steps;
    double dt, L, cc0, cc1;
    const double *obst; // [n_obs][6] (x, y, v, yaw, a, steer)  -- MovingObstacle*.get()
    double *pred;       // [n_obs][n_steps][3]  (x, y, yaw); may be NULL
    double2 *pred_cc;   // [n_obs][n_steps][2]  circle centres
    double4 *pred_bc;   // [n_obs] (x, y, r, -): a circle around ALL predicted circle centres of the obstacle (inflated beyond
                        // rounding): an ego whose own circles stay clear of it skips the obstacle's collision rows
    // blockIdx.y = tick of a K-tick batch: obst, pred_cc and pred_bc advance by one tick's worth per tick (pred is per call only)
    const double4 *shape; // [n_obs] (cc0, cc1, radius, L) of each vehicle (jsim_loop_set_vehicle_shapes), NULL: L, cc0, cc1 above for all
};

// lib/moving_obstacles_prediction.py:21-47 (yaw uses the UPDATED speed), circle centres lib/trajectories.py:11-37.  Obstacle o
// of tick t: obst, pred_cc and pred_bc advance by one tick's worth (P.n_obs obstacles) per tick, pred is per call only.
__device__ __forceinline__ void obstacle_predict_one(const ObsP &P, int o, int t)
{
    const double *ob = P.obst + (size_t)t * P.n_obs * 6;
    double2 *pcc = P.pred_cc + (size_t)t * P.n_obs * P.n_steps * 2;
    double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
    double x = ob[6 * o], y = ob[6 * o + 1], v = ob[6 * o + 2], yaw = ob[6 * o + 3];
    const double a = ob[6 * o + 4], st = ob[6 * o + 5];
    const double tn = tan(st);
    // the vehicle's own wheelbase and circle offsets, or the launch's for all
    double L = P.L, cc0 = P.cc0, cc1 = P.cc1;
    if (P.shape) { const double4 sh = P.shape[o]; cc0 = sh.x; cc1 = sh.y; L = sh.w; }
    for (int i = 0; i < P.n_steps; ++i) {
        x += v * cos(yaw) * P.dt;
        y += v * sin(yaw) * P.dt;
        v += a * P.dt;
        yaw += (v / L) * tn * P.dt;
        const size_t k = (size_t)o * P.n_steps + i;
        if (P.pred) { P.pred[3 * k] = x; P.pred[3 * k + 1] = y; P.pred[3 * k + 2] = yaw; }
        const double c = cos(yaw), s = sin(yaw);
        pcc[2 * k] = double2{c * cc0 - s * 0.0 + x, s * cc0 + c * 0.0 + y};
        pcc[2 * k + 1] = double2{c * cc1 - s * 0.0 + x, s * cc1 + c * 0.0 + y};
        for (int b = 0; b < 2; ++b) {
            const double2 q = pcc[2 * k + b];
            bx0 = fmin(bx0, q.x); bx1 = fmax(bx1, q.x); by0 = fmin(by0, q.y); by1 = fmax(by1, q.y);
        }
    }
    if (P.pred_bc) {
        const double mx = 0.5 * (bx0 + bx1), my = 0.5 * (by0 + by1);
        double r = 0.0;
        for (int i = 0; i < 2 * P.n_steps; ++i) {
            const double2 q = pcc[(size_t)o * P.n_steps * 2 + i];
            const double dx = q.x - mx, dy = q.y - my;
            r = fmax(r, sqrt(dx * dx + dy * dy));
        }
        P.pred_bc[(size_t)t * P.n_obs + o] = double4{mx, my, r * (1.0 + 1e-9) + 1e-9, 0.0};
    }
}

#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
// Grid (ceil(n_obs / 64), ticks), one thread per (tick, vehicle): one block per tick for the n_obs <= JSIM_MAX_OBS vehicles of a
// run without traffic sets, many for the vehicles of all sets (jsim_loop_set_traffic, P.n_obs = their total).  Each thread is a
// serial chain of n_steps fp64 sin / cos, like ego_predict_kernel: one wave per block.
__global__ __launch_bounds__(64) void obstacle_predict_kernel(ObsP P)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n_obs) return;
    obstacle_predict_one(P, o, blockIdx.y);
}
#endif

// Traffic sets (jsim_loop_set_traffic): the scripted vehicles of all sets sit in one [total] table, set s at obs_off[s] ..
// obs_off[s + 1]; each ego reads its own set's slice.  set_of == NULL: no layout, every ego reads all n_obs vehicles.
struct TrafficP {
    const int *set_of;  // [B] traffic set of each ego
    const int *obs_off; // [n_sets + 1]
};

struct ObsSlice { int first, n; };

__device__ __forceinline__ ObsSlice traffic_slice(const TrafficP &X, int ego, int n_obs)
{
    if (!X.set_of) return ObsSlice{0, n_obs};
    const int s = X.set_of[ego];
    const int o0 = X.obs_off[s];
    return ObsSlice{o0, X.obs_off[s + 1] - o0};
}

struct PreP {
    int B, n_obs, n_steps, frame_window, margin;
    double dt, max_accel, max_speed, thr; // thr = min_distance (2 * radius, or car radius + obstacle radius)
    double thr_sq; // the largest double whose correctly rounded square root is <= thr: sqrt(d2) <= thr  <=>  d2 <= thr_sq, exactly
    const double2 *pxy;
    const double2 *pcc; // [point][2]
    const long long *poff;
    const double2 *pred_cc;
    const double4 *pred_bc;   // [n_obs] bounding circles of the predictions (obstacle_predict_kernel)
    const double *x0;
    const int *path_id;
    long long *traj_idx;      // in/out
    const int *prev_path_len; // in (-1 = no previous truncated path)
    int *path_len;            // out
    int *col_flag;            // out: 1 = collision found
    double *col_xy;           // out [B][2] (may be NULL)
    int *first_idx;           // out: index of the hit on the detailed path (may be NULL)
    int *status;              // out
    int *dbg_res_idx;         // [B][JSIM_MAX_RES] kept indices (may be NULL)
    int *dbg_n_res;           // [B]
    // per-vehicle shapes (jsim_loop_set_vehicle_shapes): (thr, thr_sq) of each of the n_obs vehicles -- ego radius + its own
    // radius -- in the order of pred_cc / pred_bc; NULL: thr / thr_sq above for all
    const double2 *othr;
};

// What one tick of the glue decides for one ego.  status != JSIM_OK: nothing else is valid (the reference raised / the
// resampled path outgrew the table) and the caller leaves the ego's loop state alone.
struct PreOut {
    int status, idx, path_len, col, first;
    double cx, cy;
};

// LDS scratch of one wavefront (one ego)
struct PreScratch {
    int res_idx[JSIM_MAX_RES];
    double2 ecc[JSIM_MAX_RES][2];
    double2 occ[JSIM_MAX_OBS * JSIM_MAX_PRED * 2];
    double stepbuf[128]; // [0, 64): zeros; [64, 128): the point-to-point distances of the current chunk
    int olist[JSIM_MAX_OBS]; // the obstacles whose bounding circle comes within reach of the ego's resampled path
    double2 othr[JSIM_MAX_OBS]; // (thr, thr_sq) of each of the ego's obstacles: its slice of PreP.othr, or PreP.thr / thr_sq
};

// One wavefront = one ego.  pred_cc: this tick's obstacle circle centres [n_obs][n_steps][2]; (sx, sy, sv): the ego's pose;
// idx0 / prev: its progress index and the length of its previous (truncated) path.  Called by loop_pre_tick_kernel (one
// launch per tick) and from inside the fused K-tick kernel (mpc_step_reg.inc, PRE).
// BLOCK: the caller's workgroup has several wavefronts that all run this function on the same scratch (the four-wave T = 40 kernel):
// its phases are separated by workgroup barriers.  Otherwise ONE wavefront runs it -- alone in its workgroup or beside helper
// wavefronts that must not be woken -- and what it hands from lane to lane through LDS only needs the compiler's order kept.
// OCC_READY: the caller has already put the P.n_obs obstacles' circle centres into W.occ and their thresholds into W.othr
// (group_pre_tick_kernel gathers scripted obstacles and group mates there); pred_cc and othr are not read.
// othr: the ego's slice of P.othr (its obstacles' own thresholds), or NULL: P.thr / P.thr_sq for every obstacle.
#define JSIM_PRE_SYNC() do { if (BLOCK) __syncthreads(); else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } } while (0)
template <bool BLOCK = false, bool OCC_READY = false>
__device__ __forceinline__ PreOut jsim_pre_tick_ego(const PreP &P, const double2 *pred_cc, const double4 *pred_bc, const double2 *othr_g, PreScratch &W, int lane, int ego,
                                                    long long off, int M, double sx, double sy, double sv, long long idx0,
                                                    int prev)
{
    int *const res_idx = W.res_idx;
    double2 (*const ecc)[2] = W.ecc;
    double2 *const occ = W.occ;
    double *const stepbuf = W.stepbuf;
    const int *const olist = W.olist;
    const double2 *const othr = W.othr;
    PreOut out;
    out.status = JSIM_OK; out.idx = (int)idx0; out.path_len = M; out.col = 0; out.first = -1; out.cx = 0.0; out.cy = 0.0;
    int status = JSIM_OK;

    // obstacle circle centres and thresholds -> LDS
    if (!OCC_READY) {
        for (int e = lane; e < P.n_obs * P.n_steps * 2; e += 64) occ[e] = pred_cc[e];
        if (lane < P.n_obs) W.othr[lane] = othr_g ? othr_g[lane] : double2{P.thr, P.thr_sq};
    }
    stepbuf[lane] = 0.0;

    // ---- progress index (mpc_intersection.py:106-109): nearest index in direction on the FULL path
    if (prev < 0 || idx0 != (long long)prev - 1) {
        long long len = (long long)M - idx0;
        if (len < 0) len = 0;
        if (len >= 3) {
            double b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
            int i0 = 0x7fffffff, i1 = 0x7fffffff, i2 = 0x7fffffff;
            const double2 *pp = P.pxy + off + idx0;
            for (int k = lane; k < (int)len; k += 64) {
                const double2 p = pp[k];
                const double dx = p.x - sx, dy = p.y - sy;
                const double d = sqrt(dx * dx + dy * dy);
                if (d < b0) { b2 = b1; i2 = i1; b1 = b0; i1 = i0; b0 = d; i0 = k; }
                else if (d < b1) { b2 = b1; i2 = i1; b1 = d; i1 = k; }
                else if (d < b2) { b2 = d; i2 = k; }
            }
            int gi[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double v = b0;
                int id = i0;
                wargmin_dpp(v, id);
                gi[r] = id;
                if (i0 == id) { b0 = b1; i0 = i1; b1 = b2; i1 = i2; b2 = INFINITY; i2 = 0x7fffffff; }
            }
            int d12 = gi[1] - gi[2]; d12 = d12 < 0 ? -d12 : d12;
            int d01 = gi[0] - gi[1]; d01 = d01 < 0 ? -d01 : d01;
            if (d12 == 2) idx0 += gi[0];
            else if (d01 == 1) idx0 += (gi[0] > gi[1] ? gi[0] : gi[1]);
            else status = JSIM_NEAREST_ANOMALY;
        } else if (len == 2) {
            idx0 += 1;
        }
    }
    if (status != JSIM_OK) { out.status = status; return out; }
    const int idx = (int)idx0;
    const int n = M - idx; // detailed path = full[idx:], n >= 1
    const double2 *dp = P.pxy + off + idx;
    const double2 *dcc = P.pcc + 2 * (off + idx);

    // ---- resample_curve(detailed, dl_i) (lib/trajectories.py:58-86): sequential cumulative distance, keep where
    //      floor(cum_i / dl_i) steps up; dl_i = DT * min((i + 1) * MAX_ACCEL + v, MAX_SPEED)   (mpc_intersection.py:113-120)
    int n_res = 0;
    {
        double cum = 0.0;        // running sum (uniform)
        long long kprev = 0;     // floor(cum_{i-1} / dl_{i-1})
        const bool accel = sv < P.max_speed;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            double step = 0.0;
            if (i >= 1 && i < n) {
                const double2 a = dp[i], b = dp[i - 1];
                const double dx = a.x - b.x, dy = a.y - b.y;
                step = sqrt(dx * dx + dy * dy);
            }
            // exact sequential accumulate (np.cumsum order), all 64 prefixes at once: the chunk's steps sit behind 64 zeros in
            // LDS and lane L adds stepbuf[1 + L], .., stepbuf[64 + L] to the carry -- 63 - L exact no-ops (+ 0.0), then
            // step_0, .., step_L in order.  One conflict-free ds_read with an immediate offset and one add per element
            // (two v_readlane, an add, a compare and two selects before).
            const int cnt = (n - base) < 64 ? (n - base) : 64;
            stepbuf[64 + lane] = step;
            JSIM_PRE_SYNC();
            double mycum = cum;
#pragma unroll
            for (int t = 0; t < 64; ++t) mycum += stepbuf[1 + t + lane];
            cum = rdlane(mycum, cnt - 1);
            JSIM_PRE_SYNC();
            bool keep = false;
            long long ki = 0;
            if (i < n) {
                double dli;
                if (accel) {
                    double acc = (double)(i + 1) * P.max_accel + sv; // cumsum of MAX_ACCEL is exact
                    dli = P.dt * (acc < P.max_speed ? acc : P.max_speed);
                } else dli = P.dt * P.max_speed;
                ki = (long long)floor(mycum / dli);
            }
            // k of the previous point: lane-1, or the carry from the previous chunk
            long long kp = __shfl_up(ki, 1);
            if (lane == 0) kp = kprev;
            if (i < n) keep = (i == 0) || (i == n - 1) || (ki - kp >= 1);
            kprev = __shfl(ki, cnt - 1);
            const unsigned long long bal = __ballot(keep);
            const int slot = n_res + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && slot < JSIM_MAX_RES) {
                res_idx[slot] = i;
                ecc[slot][0] = dcc[2 * i];
                ecc[slot][1] = dcc[2 * i + 1];
            }
            n_res += __popcll(bal);
        }
    }
    if (n_res > JSIM_MAX_RES) { out.status = 4; return out; } // resampled path longer than the kernel's table
    JSIM_PRE_SYNC();
    if (P.dbg_res_idx) {
        for (int e = lane; e < n_res; e += 64) P.dbg_res_idx[(size_t)ego * JSIM_MAX_RES + e] = res_idx[e];
        if (lane == 0) P.dbg_n_res[ego] = n_res;
    }

    // ---- first colliding row (collision_avoidance.py:85-103).  Row order: frame, ego circle a, obstacle o, frame
    //      offset -w..w, obstacle circle b.  Copy (o, off) shows sample clamp(min(f, Pn-1) - off, 0, Pn-1) at frame f.
    int hit_o = -1, hit_j = 0, hit_b = 0;
    bool any_hit = false;
    // Obstacles that cannot touch the ego at all are left out of the pair table: a circle around the ego's resampled circle
    // centres against the circle around each obstacle's predicted ones (both inflated beyond rounding).  Rows of the
    // remaining obstacles keep their order, so the first hit is the reference's.
    int na = 0;
    if (P.n_obs > 0) {
        double ex0 = INFINITY, ex1 = -INFINITY, ey0 = INFINITY, ey1 = -INFINITY;
        for (int e = lane; e < 2 * n_res; e += 64) {
            const double2 q = ecc[e >> 1][e & 1];
            ex0 = fmin(ex0, q.x); ex1 = fmax(ex1, q.x); ey0 = fmin(ey0, q.y); ey1 = fmax(ey1, q.y);
        }
        ex0 = wmin_dpp(ex0); ex1 = wmax_dpp(ex1); ey0 = wmin_dpp(ey0); ey1 = wmax_dpp(ey1);
        const double emx = 0.5 * (ex0 + ex1), emy = 0.5 * (ey0 + ey1);
        double er = 0.0;
        for (int e = lane; e < 2 * n_res; e += 64) {
            const double2 q = ecc[e >> 1][e & 1];
            const double dx = q.x - emx, dy = q.y - emy;
            er = fmax(er, sqrt(dx * dx + dy * dy));
        }
        er = wmax_dpp(er) * (1.0 + 1e-9) + 1e-9;
        bool near = false;
        if (lane < P.n_obs) {
            const double4 bc = pred_bc[lane];
            const double dx = bc.x - emx, dy = bc.y - emy;
            near = sqrt(dx * dx + dy * dy) - bc.z - er <= othr[lane].x;
        }
        const unsigned long long nm = __ballot(near);
        na = __popcll(nm);
        if (lane < P.n_obs && near) W.olist[__popcll(nm & ((1ull << lane) - 1ull))] = lane;
        JSIM_PRE_SYNC();
    }
    if (na > 0) {
        const int Pn = P.n_steps, w = P.frame_window, W = 2 * w + 1;
        const int R = 2 * na * W * 2;            // rows per frame (of the obstacles within reach)
        const int F = n_res > Pn ? n_res : Pn;
        const int FB = 8;                         // frames per block
        for (int f0 = 0; f0 < F && !any_hit; f0 += FB) {
            const int fcnt = (F - f0) < FB ? (F - f0) : FB;
            long long best = 0x7fffffffffffffffll;
            // A lane takes rows rr = lane, lane + 64, .. of EVERY frame of the block: (a, o, offset, b) is decoded once per
            // row slot by stepping a mixed-radix counter (three integer divisions per test cost five times the test), the
            // frames of the block are the inner loop.  The smallest key = the first row in row order, as before.
            const int b = lane & 1;
            int ao = (lane >> 1) / W;            // a * n_obs + o   (one division per block)
            int kk = (lane >> 1) - ao * W;       // offset + w
            for (int rr = lane; rr < R; rr += 64) {
                const int a = ao >= na ? 1 : 0;
                const int o = olist[ao - a * na];
                const int offk = kk - w;
                const double2 *oc = &occ[(size_t)o * Pn * 2 + b];
                const double thr_sq = othr[o].y;  // the obstacle's own threshold: one LDS read per row slot
                for (int fl = 0; fl < fcnt; ++fl) {
                    const int f = f0 + fl;
                    const int fa = f < n_res - 1 ? f : n_res - 1;
                    const int fo = f < Pn - 1 ? f : Pn - 1;
                    int j = fo - offk;
                    j = j < 0 ? 0 : (j > Pn - 1 ? Pn - 1 : j);
                    const double2 pa = ecc[fa][a];
                    const double2 po = oc[2 * j];
                    const double dx = pa.x - po.x, dy = pa.y - po.y;
                    if (dx * dx + dy * dy <= thr_sq) { // == (sqrt(dx*dx + dy*dy) <= thr), without the square root
                        const long long key = ((long long)(fl * R + rr) << 32) | ((long long)o << 16) | ((long long)j << 1) | b;
                        if (key < best) best = key;
                    }
                }
                kk += 32;                        // 64 rows = 32 (offset, b) pairs further
                while (kk >= W) { kk -= W; ++ao; }
            }
            // wave minimum of the 64-bit key (row index in the high word)
            double bd = (double)(best >> 32);
            int bl = (best == 0x7fffffffffffffffll) ? 0x7fffffff : lane;
            if (best == 0x7fffffffffffffffll) bd = INFINITY;
            wargmin_dpp(bd, bl);
            if (bl != 0x7fffffff) {
                const long long kb = __shfl(best, bl);
                any_hit = true;
                hit_o = (int)((kb >> 16) & 0xffff);
                hit_j = (int)((kb >> 1) & 0x7fff);
                hit_b = (int)(kb & 1);
            }
        }
    }
    out.idx = idx;
    if (!any_hit) return out;
    // ---- first point of the detailed path whose front (then rear) circle touches that obstacle circle (:111-118)
    const double2 hp = occ[((size_t)hit_o * P.n_steps + hit_j) * 2 + hit_b];
    const double hthr = othr[hit_o].x;
    int first = 0;
    {
        bool found = false;
        for (int a = 0; a < 2 && !found; ++a) {
            int bi = 0x7fffffff;
            for (int i = lane; i < n; i += 64) {
                const double2 c = dcc[2 * i + a];
                const double dx = hp.x - c.x, dy = hp.y - c.y;
                if (sqrt(dx * dx + dy * dy) <= hthr && i < bi) bi = i;
            }
            double bd = (double)bi;
            int dummy = lane;
            wargmin_dpp(bd, dummy);
            if (bd < 2.0e9) { first = (int)bd; found = true; }
        }
    }
    const double2 cp = dp[first]; // collision point on the path
    // ---- cut-off (collision_avoidance.py:168-180): first index of the FULL path within 1 mm of that point
    int cidx;
    {
        int bi = 0x7fffffff;
        const double2 *fp = P.pxy + off;
        for (int i = lane; i < M; i += 64) {
            const double2 q = fp[i];
            const double dx = q.x - cp.x, dy = q.y - cp.y;
            if (sqrt(dx * dx + dy * dy) <= 0.001 && i < bi) bi = i;
        }
        double bd = (double)bi;
        int dummy = lane;
        wargmin_dpp(bd, dummy);
        cidx = (int)bd;
    }
    int cut = cidx - P.margin;
    if (cut < idx + 1) cut = idx + 1;
    out.path_len = cut; out.col = 1; out.first = first; out.cx = cp.x; out.cy = cp.y;
    return out;
}

#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
// X: the ego reads its traffic set's slice of P.pred_cc / P.pred_bc (P.n_obs = all sets' vehicles), or all of them
__global__ __launch_bounds__(64) void loop_pre_tick_kernel(PreP P, TrafficP X)
{
    __shared__ PreScratch W;
    const int lane = threadIdx.x;
    const int ego = blockIdx.x;
    if (ego >= P.B) return;
    const int pid = P.path_id[ego];
    const long long off = P.poff[pid];
    const int M = (int)(P.poff[pid + 1] - off);
    const ObsSlice sl = traffic_slice(X, ego, P.n_obs);
    PreP Q = P;
    Q.n_obs = sl.n;
    const PreOut o = jsim_pre_tick_ego(Q, P.pred_cc + (size_t)sl.first * P.n_steps * 2, P.pred_bc + sl.first,
                                       P.othr ? P.othr + sl.first : nullptr, W, lane, ego, off, M,
                                       P.x0[4 * ego], P.x0[4 * ego + 1], P.x0[4 * ego + 2], P.traj_idx[ego], P.prev_path_len[ego]);
    if (lane != 0) return;
    P.status[ego] = o.status;
    if (o.status != JSIM_OK) return; // the reference raised: the ego's loop state stays as it was
    P.traj_idx[ego] = o.idx;
    P.path_len[ego] = o.path_len;
    P.col_flag[ego] = o.col;
    if (o.col && P.col_xy) { P.col_xy[2 * ego] = o.cx; P.col_xy[2 * ego + 1] = o.cy; }
    if (P.first_idx) P.first_idx[ego] = o.first;
}
#endif

// ---- Interacting egos (main/scenarios/interactive_mpc.py:117-190): the obstacles of an ego are the scripted vehicles and
//      the OTHER egos of its group (contiguous batch range group_off[g] .. group_off[g + 1]), every ego predicted like an
//      obstacle from its tick-start state: MovingObstaclesPrediction(x, y, v, yaw, a = 0, steering = the delta it applied
//      last tick).
struct EgoPredP {
    int B, n_steps;
    double dt, L, cc0, cc1;
    const double *x0;    // [B][4] (x, y, v, yaw)
    const double *di_ai; // [B][2] (delta, a) applied last tick (0 before the first step and after a respawn)
    double *pred;        // [B][n_steps][3] (x, y, yaw); may be NULL
    double2 *pred_cc;    // [B][n_steps][2] circle centres
    double4 *pred_bc;    // [B] bounding circles, as obstacle_predict_kernel
};

// One thread per ego over the whole batch, 64 per block (each thread is a serial chain of n_steps fp64 sin / cos: one wave per
// CU rather than four to a block).  The arithmetic is obstacle_predict_kernel's, operation for operation, so an ego
// predicted here equals its (x, y, v, yaw, 0, delta) tuple run through that kernel bit for bit.
#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
__global__ __launch_bounds__(64) void ego_predict_kernel(EgoPredP P)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= P.B) return;
    double2 *pcc = P.pred_cc;
    double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
    double x = P.x0[4 * o], y = P.x0[4 * o + 1], v = P.x0[4 * o + 2], yaw = P.x0[4 * o + 3];
    const double a = 0.0, st = P.di_ai[2 * o];
    const double tn = tan(st);
    for (int i = 0; i < P.n_steps; ++i) {
        x += v * cos(yaw) * P.dt;
        y += v * sin(yaw) * P.dt;
        v += a * P.dt;
        yaw += (v / P.L) * tn * P.dt;
        const size_t k = (size_t)o * P.n_steps + i;
        if (P.pred) { P.pred[3 * k] = x; P.pred[3 * k + 1] = y; P.pred[3 * k + 2] = yaw; }
        const double c = cos(yaw), s = sin(yaw);
        pcc[2 * k] = double2{c * P.cc0 - s * 0.0 + x, s * P.cc0 + c * 0.0 + y};
        pcc[2 * k + 1] = double2{c * P.cc1 - s * 0.0 + x, s * P.cc1 + c * 0.0 + y};
        for (int b = 0; b < 2; ++b) {
            const double2 q = pcc[2 * k + b];
            bx0 = fmin(bx0, q.x); bx1 = fmax(bx1, q.x); by0 = fmin(by0, q.y); by1 = fmax(by1, q.y);
        }
    }
    const double mx = 0.5 * (bx0 + bx1), my = 0.5 * (by0 + by1);
    double r = 0.0;
    for (int i = 0; i < 2 * P.n_steps; ++i) {
        const double2 q = pcc[(size_t)o * P.n_steps * 2 + i];
        const double dx = q.x - mx, dy = q.y - my;
        r = fmax(r, sqrt(dx * dx + dy * dy));
    }
    P.pred_bc[o] = double4{mx, my, r * (1.0 + 1e-9) + 1e-9, 0.0};
}
#endif

// ---- Egos that share their MPC plans (JSIM_MATE_PLAN, include/jsim_mpc.h, DESIGN.md section 27): ego m is predicted by rolling
//      the controls its controller holds at the start of the tick -- oa[m][0..T-1], od[m][0..T-1] of its last solve, element 0
//      the input it applied last tick (every kernel stores them unshifted) -- through the plant's own step (simulation_step).
//      Input of prediction step i, with j = i + 1:  status[m] == JSIM_OK: (oa[m][j], od[m][j]) while j <= T - 1, then
//      (0, od[m][T - 1]);  any other status: (0, the delta applied last tick) for every step.
struct EgoPlanP {
    int B, n_steps, T;
    double dt, L, smax, vmax, vmin, cc0, cc1; // wheelbase and clamps: the plant's (PlantP)
    const double *x0;    // [B][4] (x, y, v, yaw)
    const double *oa;    // [B][T] accelerations of the last solve (zeros before the first one and after a respawn)
    const double *od;    // [B][T] steering angles of the last solve
    const int *status;   // [B] status of the last solve
    const double *di_ai; // [B][2] (delta, a) applied last tick
    double *pred;        // [B][n_steps][3] (x, y, yaw); may be NULL
    double2 *pred_cc;    // [B][n_steps][2] circle centres
    double4 *pred_bc;    // [B] bounding circles, as ego_predict_kernel
};

#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
// The running value of s += inc[0], s += inc[1], .. in step order, every lane adding the broadcast of lane i's increment to the
// same s: lane i is left with s after step i (lanes from n on with s0).  The sums are the serial loop's, add for add.
__device__ __forceinline__ double plan_running_sum(double s0, double inc, int n, int lane)
{
    double s = s0, after = s0;
    for (int i = 0; i < n; ++i) {
        s += rdlane(inc, i);
        after = lane == i ? s : after;
    }
    return after;
}

// Grid B, one wavefront per ego, lane i owns prediction step i (n_steps <= JSIM_MAX_PRED = 64).  What costs -- tan of the
// clamped steering, sin / cos of every heading, the circle centres -- is evaluated once per step across the lanes; what is
// serial -- v with its clamps, then yaw, then x and y -- is a loop of fp64 adds on values broadcast with v_readlane.  cos / sin of
// a heading serve the circle centres of its own sample and the position increment of the next step: the next lane fetches them.
// All 64 lanes stay active to the end (the DPP reductions read every lane); lanes from n_steps on hold neutral values and
// store nothing.  No LDS.
__global__ __launch_bounds__(64) void ego_plan_predict_kernel(EgoPlanP P)
{
    const int o = blockIdx.x, lane = threadIdx.x;
    if (o >= P.B) return;
    const int n = P.n_steps, T = P.T;
    const bool mine = lane < n;
    // the input of step `lane`: every index stays inside the ego's row, for the idle lanes too
    const int j = lane + 1, jc = j < T ? j : T - 1;
    const bool ok = P.status[o] == JSIM_OK;
    const double a_plan = P.oa[(size_t)o * T + jc], d_plan = P.od[(size_t)o * T + jc];
    const double ai = (ok && j < T) ? a_plan : 0.0;
    const double di = ok ? d_plan : P.di_ai[2 * o];
    double dc = (P.smax < di) ? P.smax : di;
    dc = (-P.smax > dc) ? -P.smax : dc;
    const double tn = tan(dc);
    const double x0 = P.x0[4 * o], y0 = P.x0[4 * o + 1], v0 = P.x0[4 * o + 2], th0 = P.x0[4 * o + 3];
    const double c0 = cos(th0), s0 = sin(th0);
    // v: lane i keeps the speed BEFORE step i, which both the position and the heading increment of the step use
    double vb = v0;
    {
        const double adt = ai * P.dt;
        double v = v0;
        for (int i = 0; i < n; ++i) {
            vb = lane == i ? v : vb;
            v += rdlane(adt, i);
            v = (P.vmax < v) ? P.vmax : v;
            v = (P.vmin > v) ? P.vmin : v;
        }
    }
    // yaw after the lane's step; its cos / sin, and the previous heading's from the lane below (lane 0: the start heading's)
    const double yaw = plan_running_sum(th0, (vb / P.L) * tn * P.dt, n, lane);
    const double c = cos(yaw), s = sin(yaw);
    double cp = __shfl_up(c, 1), sp = __shfl_up(s, 1);
    if (lane == 0) { cp = c0; sp = s0; }
    const double x = plan_running_sum(x0, vb * cp * P.dt, n, lane);
    const double y = plan_running_sum(y0, vb * sp * P.dt, n, lane);
    const double2 q0 = double2{c * P.cc0 - s * 0.0 + x, s * P.cc0 + c * 0.0 + y};
    const double2 q1 = double2{c * P.cc1 - s * 0.0 + x, s * P.cc1 + c * 0.0 + y};
    if (mine) {
        const size_t k = (size_t)o * n + lane;
        if (P.pred) { P.pred[3 * k] = x; P.pred[3 * k + 1] = y; P.pred[3 * k + 2] = yaw; }
        P.pred_cc[2 * k] = q0;
        P.pred_cc[2 * k + 1] = q1;
    }
    // the circle around all circle centres, as ego_predict_kernel (min / max do not depend on the order)
    const double bx0 = wmin_dpp(mine ? fmin(q0.x, q1.x) : INFINITY), bx1 = wmax_dpp(mine ? fmax(q0.x, q1.x) : -INFINITY);
    const double by0 = wmin_dpp(mine ? fmin(q0.y, q1.y) : INFINITY), by1 = wmax_dpp(mine ? fmax(q0.y, q1.y) : -INFINITY);
    const double mx = 0.5 * (bx0 + bx1), my = 0.5 * (by0 + by1);
    const double dx0 = q0.x - mx, dy0 = q0.y - my, dx1 = q1.x - mx, dy1 = q1.y - my;
    const double r = wmax_dpp(mine ? fmax(sqrt(dx0 * dx0 + dy0 * dy0), sqrt(dx1 * dx1 + dy1 * dy1)) : 0.0);
    if (lane == 0) P.pred_bc[o] = double4{mx, my, r * (1.0 + 1e-9) + 1e-9, 0.0};
}
#endif

struct GroupP {
    const int *group_of;     // [B] group of each ego
    const int *group_off;    // [n_groups + 1]
    const double2 *ego_cc;   // [B][n_steps][2] (ego_predict_kernel)
    const double4 *ego_bc;   // [B]
    int n_scripted;          // scripted obstacles in P.pred_cc / P.pred_bc (P.n_obs is ignored); with traffic sets: all sets' vehicles
    double mate_thr, mate_thr_sq; // the ego / ego threshold (2 * the egos' radius) of the group mates' rows
};

// loop_pre_tick_kernel for interacting egos: one wavefront per ego gathers the scripted predictions, then those of its group
// mates in ascending batch index (skipping itself), into the LDS view jsim_pre_tick_ego reads, and runs the same glue.  The
// scripted ones are its traffic set's (X), or all G.n_scripted without a layout; their thresholds are the shape table's
// (P.othr) or P.thr, the mates' the ego / ego one.
#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
// The gather, for group_pre_tick_kernel and the replay of recorded ticks (cutoff_ticks.inc): the ego's obstacles -> W.occ / W.othr
// and their bounding circles -> bc [JSIM_MAX_OBS] (LDS); returns how many they are.  Ends behind the wavefront's fence.
__device__ __forceinline__ int group_gather_obstacles(const PreP &P, const GroupP &G, const TrafficP &X, int ego, int lane,
                                                      PreScratch &W, double4 *bc)
{
    constexpr bool BLOCK = false;
    const int g = G.group_of[ego];
    const int g0 = G.group_off[g], n_mates = G.group_off[g + 1] - g0 - 1;
    const ObsSlice sl = traffic_slice(X, ego, G.n_scripted);
    const int ns = sl.n, per = P.n_steps * 2;
    const double2 *scc = P.pred_cc + (size_t)sl.first * per;
    for (int e = lane; e < ns * per; e += 64) W.occ[e] = scc[e];
    for (int m = 0; m < n_mates; ++m) {
        const int j = g0 + m + (g0 + m >= ego ? 1 : 0);
        const double2 *src = G.ego_cc + (size_t)j * per;
        double2 *dst = W.occ + (size_t)(ns + m) * per;
        for (int e = lane; e < per; e += 64) dst[e] = src[e];
    }
    if (lane < ns) {
        bc[lane] = P.pred_bc[sl.first + lane];
        W.othr[lane] = P.othr ? P.othr[sl.first + lane] : double2{P.thr, P.thr_sq};
    } else if (lane < ns + n_mates) {
        const int m = lane - ns;
        bc[lane] = G.ego_bc[g0 + m + (g0 + m >= ego ? 1 : 0)];
        W.othr[lane] = double2{G.mate_thr, G.mate_thr_sq};
    }
    JSIM_PRE_SYNC();
    return ns + n_mates;
}

__global__ __launch_bounds__(64) void group_pre_tick_kernel(PreP P, GroupP G, TrafficP X)
{
    __shared__ PreScratch W;
    __shared__ double4 bc[JSIM_MAX_OBS];
    const int lane = threadIdx.x;
    const int ego = blockIdx.x;
    if (ego >= P.B) return;
    PreP Q = P;
    Q.n_obs = group_gather_obstacles(P, G, X, ego, lane, W, bc);
    const int pid = P.path_id[ego];
    const long long off = P.poff[pid];
    const int M = (int)(P.poff[pid + 1] - off);
    const PreOut o = jsim_pre_tick_ego<false, true>(Q, nullptr, bc, nullptr, W, lane, ego, off, M, P.x0[4 * ego], P.x0[4 * ego + 1],
                                                     P.x0[4 * ego + 2], P.traj_idx[ego], P.prev_path_len[ego]);
    if (lane != 0) return;
    P.status[ego] = o.status;
    if (o.status != JSIM_OK) return; // the ego's loop state stays as it was
    P.traj_idx[ego] = o.idx;
    P.path_len[ego] = o.path_len;
    P.col_flag[ego] = o.col;
    if (o.col && P.col_xy) { P.col_xy[2 * ego] = o.cx; P.col_xy[2 * ego + 1] = o.cy; }
    if (P.first_idx) P.first_idx[ego] = o.first;
}
#endif


#include "traffic_routes.inc" // route vehicles (kind 3): the route table's kernel and route_pose

// Scripted obstacle vehicles of the reference scenarios (main/lib/moving_obstacles.py): MovingObstacleTIntersection (:166-232,
// kind 0), MovingObstacleRoundabout (:28-124, kind 1) and MovingObstacleArterial (:126-164, kind 2).  State (xc, yc, theta,
// counter) advanced by Bicycle.step with the scripted steering / start-delay rules; the `get()` tuple (x, y, v, yaw, a = 0,
// steer) is written for the prediction kernel.  One thread per obstacle over ceil(n_obs / 64) blocks: one block without traffic
// sets (n_obs <= JSIM_MAX_OBS), many for the vehicles of all sets (P.n_obs = their total, tens of thousands).
// Kind 3, a vehicle on a route of the table below, is not the reference's: include/jsim_mpc.h states its rule.
struct ObsStepP {
    int n_obs, do_step;
    double L;             // wheelbase of every vehicle without a shape table
    double *state;        // [n_obs][4]  xc, yc, theta, counter
    const double *param;  // [n_obs][8]  direction (+-1), turning (0/1), speed, offset (<= 0: none), x_turn, dt, kind, initial_speed
    double *get;          // [n_obs][6]  x, y, v, yaw, a, steer  (state BEFORE the step, like o.get() ahead of o.step())
    // the recorder (jsim_loop_set_recorder), NULL: none -- the get() tuples ahead of each step() go to rec [rec_cap][n_obs][6],
    // slot = the device tick counter (+ the tick of a rollout), as the scripts' obstacles_positions keep them
    double *rec;
    const int *tick;
    int rec_cap;
    const double4 *shape; // [n_obs] (cc0, cc1, radius, L) of each vehicle (jsim_loop_set_vehicle_shapes), NULL: L above for all
    // the route table (jsim_loop_set_traffic_routes), NULL: none -- a kind-3 row is then stepped as kind 0
    const double4 *route_pt; // [points] (x, y, yaw, S)
    const int *route_off;    // [n_routes + 1]
    int n_routes;
};

__device__ __forceinline__ double obstacle_steer(double dir, double turning, double xc, double theta, double x_turn)
{
    if (turning == 0.0) return 0.0;
    if (dir > 0.0) return (xc >= x_turn && theta > (-M_PI / 2)) ? -0.38 : 0.0; // steering angle right (short turn)
    return (xc <= x_turn && theta < (3 * M_PI / 2)) ? 0.19 : 0.0;               // steering angle left (long turn)
}

// MovingObstacleRoundabout.steering_angle (:66-108): a chain of overriding ifs; its last rule also REWRITES the heading
// (a side effect of the property, so it happens on every evaluation -- in get() and in step())
__device__ __forceinline__ double roundabout_steer(double dir, double turning, double xc, double yc, double &theta)
{
    double s = 0.0;
    if (turning == 0.0) return s;
    const double A = atan((1.0 / 5.0) * 2.86); // calculate_steering_angle_for_radius(5), :15-25
    if (dir > 0.0) {
        if (-7.0 <= xc && xc <= -4.0 && yc < 0.0) s = -A;
        if (-3.0 < xc) s = A;
        if (yc > 0.0 && -5.0 <= xc && xc <= -3.0) s = -A;
        if (xc <= -3.0 && yc > 0.0) { theta = -M_PI; s = 0.0; }
    } else {
        if (4.0 <= xc && xc <= 7.0 && yc > 0.0) s = -A;
        if (xc < 3.0) s = A;
        if (yc < 0.0 && 3.0 <= xc && xc <= 5.0) s = -A;
        if (3.0 <= xc && yc < 0.0) { theta = 0.0; s = 0.0; }
    }
    return s;
}

// A route vehicle (kind 3; include/jsim_mpc.h states the rule): get() is the pose of the counter, step() the counter + 1 and its
// pose; the state's pose slots are outputs
__device__ __forceinline__ void route_vehicle_one(const ObsStepP &P, int o, int &hint)
{
    const double *pr = P.param + 8 * o;
    const double L = P.shape ? P.shape[o].w : P.L;
    double cnt = P.state[4 * o + 3], x, y, yaw, v, steer;
    route_pose(P.route_pt, P.route_off, P.n_routes, pr, L, cnt, hint, x, y, yaw, v, steer);
    if (P.get) {
        P.get[6 * o] = x; P.get[6 * o + 1] = y; P.get[6 * o + 2] = v; P.get[6 * o + 3] = yaw; P.get[6 * o + 4] = 0.0;
        P.get[6 * o + 5] = steer;
    }
    if (P.do_step) {
        cnt += 1.0;
        route_pose(P.route_pt, P.route_off, P.n_routes, pr, L, cnt, hint, x, y, yaw, v, steer);
    }
    P.state[4 * o] = x; P.state[4 * o + 1] = y; P.state[4 * o + 2] = yaw; P.state[4 * o + 3] = cnt;
}

// hint: a caller that steps one vehicle through many ticks carries the route vehicles' segment index here (route_segment)
__device__ __forceinline__ void obstacle_step_one(const ObsStepP &P, int o, int *hint = nullptr)
{
    if (P.route_pt && (int)P.param[8 * o + 6] == 3) {
        int h = hint ? *hint : -1;
        route_vehicle_one(P, o, h);
        if (hint) *hint = h;
        return;
    }
    double xc = P.state[4 * o], yc = P.state[4 * o + 1], th = P.state[4 * o + 2], cnt = P.state[4 * o + 3];
    const double *pr = P.param + 8 * o;
    const double dir = pr[0], turning = pr[1], speed = pr[2], offs = pr[3], x_turn = pr[4], dt = pr[5];
    const int kind = (int)pr[6];
    const double v0 = pr[7];
    const double th_get = th; // get() reads the heading before it evaluates the steering property
    double steer, v;
    if (kind == 1) {
        steer = roundabout_steer(dir, turning, xc, yc, th);
        v = (!(offs > 0.0) || cnt > (offs / 0.2)) ? speed : 0.0;   // self.dt = dt = 0.2 for the start delay (:47)
    } else if (kind == 2) {
        steer = 0.0;
        v = (!(offs > 0.0) || cnt > (offs / dt)) ? speed : v0;     // initial_speed before the offset (:151-156)
    } else {
        steer = obstacle_steer(dir, turning, xc, th, x_turn);
        v = (!(offs > 0.0) || cnt > (offs / dt)) ? speed : 0.0;    // forward_velocity
    }
    if (P.get) {
        P.get[6 * o] = xc; P.get[6 * o + 1] = yc; P.get[6 * o + 2] = v; P.get[6 * o + 3] = th_get; P.get[6 * o + 4] = 0.0;
        P.get[6 * o + 5] = steer;
    }
    if (P.do_step) { // Bicycle.step (main/bicycle/main.py:28-41), then counter += 1
        const double L = P.shape ? P.shape[o].w : P.L;
        const double xd = v * cos(th), yd = v * sin(th), thd = (v / L) * tan(steer);
        xc += xd * dt; yc += yd * dt; th += thd * dt;
        P.state[4 * o] = xc; P.state[4 * o + 1] = yc; P.state[4 * o + 3] = cnt + 1.0;
    }
    P.state[4 * o + 2] = th; // also without a step: the roundabout rule may have rewritten the heading
}

// The recorder's slot of the tick dk ticks after the counter's, or NULL (no recorder, or beyond its capacity)
__device__ __forceinline__ double *obstacle_rec_slot(const ObsStepP &P, int dk)
{
    if (!P.rec) return nullptr;
    const int k = *P.tick + dk;
    return (k >= 0 && k < P.rec_cap) ? P.rec + (size_t)k * P.n_obs * 6 : nullptr;
}

// a host tick's get() + step() call, the last launch of the tick: its get() tuple to the recorder's slot of the tick (the
// advance has already counted it)
__device__ __forceinline__ void obstacle_record(const ObsStepP &P, int o)
{
    if (!P.do_step || !P.get) return;
    double *r = obstacle_rec_slot(P, -1);
    if (r)
        for (int j = 0; j < 6; ++j) r[6 * o + j] = P.get[6 * o + j];
}

#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
__global__ __launch_bounds__(64) void obstacle_step_kernel(ObsStepP P)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n_obs) return;
    obstacle_step_one(P, o);
    obstacle_record(P, o);
}

// n_ticks ticks of the loop's two calls per tick -- get() ahead of the prediction, then get() + step() (ScenarioLoop.tick) --
// for scripted obstacles, which do not depend on the egos: the get() tuples of every tick go to get_all [n_ticks][n_obs][6].
__global__ __launch_bounds__(64) void obstacle_rollout_kernel(ObsStepP P, int n_ticks, double *get_all)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n_obs) return;
    int hint = -1;
    for (int k = 0; k < n_ticks; ++k) {
        ObsStepP Q = P;
        Q.do_step = 0; Q.get = get_all + (size_t)k * P.n_obs * 6;
        obstacle_step_one(Q, o, &hint);
        Q.do_step = 1; Q.get = obstacle_rec_slot(P, k);
        obstacle_step_one(Q, o, &hint);
    }
}
#endif
