// Clearance and first contact per recorded tick (DESIGN.md section 17): what check_collision_moving_cars and
// check_collision_moving_bicycle of main/lib/collision_avoidance.py (:85-166) answer when they are handed an episode's realised
// poses (main/planner/moving_obstacle_avoidance.py:44-76) -- the ego's History against the vehicles' recorded get() tuples and its
// group mates' Histories -- as one pass over the History recorder's buffers (jsim_loop_set_recorder), walked as recorder_walk.inc
// says: one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t.
//
// Lane-parallel: the poses, the circle centres, the reference's pair table of the tick's frame (every row of it), `clear`, `who`
// and `row`.  Per episode, in two forward sweeps of the same wavefront: sweep 1 notes at the slot of the episode's first tick the
// tick of its first touching frame and that row's vehicle circle (its position and whose it is); sweep 2 carries that position and
// the vehicle's threshold through the episode as uniform values and keeps the earliest frame at which the ego's front circle, and
// the earliest at which its rear circle, touches it -- the reference's `np.argmax(mask) % len` over front ++ rear.

// The ego's vehicle list as every call that meets it takes it (conflicts, gaps, headway): the recorder's buffers, the recorded
// vehicles, the ego's slice of them and of its group mates, and the shapes.  What .z and .w of a row of `shapes` and of ego_row mean
// is the caller's: conflicts and gaps pass (thr, thr_sq), headway passes (radius, thr)
struct VehicleListP {
    RecorderBuf R;
    int n_obs;
    const double *obs_rec;    // [n][n_obs][6] or NULL (n_obs = 0)
    const int *veh_range;     // [B][2] the ego's vehicles [lo, hi) among the n_obs recorded ones
    const int *mate_range;    // [B][2] the batch range [mlo, mhi) of its group mates (itself skipped)
    const double4 *shapes;    // [n_obs] (cc_front, cc_rear, .z, .w) or NULL: every vehicle has the ego's shape
    double cc_f, cc_r;        // the ego's circle offsets
    double4 ego_row;          // (cc_front, cc_rear, .z, .w) of a vehicle with the ego's shape: a mate, or any vehicle without a table
};

struct ConflictP {
    VehicleListP V;           // rows: (cc_front, cc_rear, thr, thr_sq)
    int w;
    double *clear;            // [n][B]
    int *who, *row;           // [n][B]
    int *hit_tick, *hit_frame; // [n][B], at an episode's first slot
    double *hit_xy;           // [n][B][2]
};

// The ego's vehicle list: ns scripted vehicles from lo on, then nm mates from mlo on with the ego itself skipped; clamped to the
// tables and to JSIM_MAX_OBS in total (the Python surface refuses what is clamped here)
struct ConflictList { int lo, ns, mlo, nm, skip; };
__device__ __forceinline__ ConflictList jcf_list(const VehicleListP &V, int b)
{
    ConflictList L;
    int lo = V.veh_range[2 * b], hi = V.veh_range[2 * b + 1];
    lo = lo < 0 ? 0 : lo; hi = hi > V.n_obs ? V.n_obs : hi;
    L.lo = lo; L.ns = hi > lo ? hi - lo : 0;
    if (L.ns > JSIM_MAX_OBS) L.ns = JSIM_MAX_OBS;
    int mlo = V.mate_range[2 * b], mhi = V.mate_range[2 * b + 1];
    mlo = mlo < 0 ? 0 : mlo; mhi = mhi > V.R.B ? V.R.B : mhi;
    L.mlo = mlo;
    L.skip = (b >= mlo && b < mhi) ? b : V.R.B;      // the batch index the enumeration steps over
    L.nm = mhi > mlo ? mhi - mlo - (L.skip < V.R.B ? 1 : 0) : 0;
    if (L.ns + L.nm > JSIM_MAX_OBS) L.nm = JSIM_MAX_OBS - L.ns;
    return L;
}

// Vehicle i of the list: its row; a scripted vehicle's (i < L.ns) record of tick k, its get() tuple x, y, v, yaw, ..; the batch index
// of the mate that holds place i >= L.ns, the ego's own stepped over; and the pose either has at the start of tick k
__device__ __forceinline__ double4 jcf_vehicle_row(const VehicleListP &V, const ConflictList &L, int i)
{
    return (i < L.ns && V.shapes) ? V.shapes[L.lo + i] : V.ego_row;
}
__device__ __forceinline__ const double *jcf_scripted(const VehicleListP &V, const ConflictList &L, int i, int k)
{
    return V.obs_rec + 6 * ((size_t)k * V.n_obs + (L.lo + i));
}
__device__ __forceinline__ int jcf_mate(const ConflictList &L, int i)
{
    int m = L.mlo + (i - L.ns);
    if (m >= L.skip) ++m;
    return m;
}
__device__ __forceinline__ void jcf_vehicle_pose(const VehicleListP &V, const ConflictList &L, int i, int k, double &x, double &y, double &yaw)
{
    if (i < L.ns) {
        const double *c = jcf_scripted(V, L, i, k);
        x = c[0]; y = c[1]; yaw = c[3];
    } else {
        jrw_pose(V.R, jcf_mate(L, i), k, x, y, yaw);
    }
}

__global__ __launch_bounds__(64) void conflict_ticks_kernel(const ConflictP P)
{
    const VehicleListP &V = P.V;
    const RecorderBuf &R = V.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks, w = P.w, nw = 2 * P.w + 1;
    const ConflictList L = jcf_list(V, b);
    const int n_veh = L.ns + L.nm;
    const unsigned long long upto = ~0ull >> (63 - lane), from = ~0ull << lane;   // bits 0 .. lane, bits lane .. 63

    // ---- sweep 1: the frame of every tick; per episode the first touching frame's tick, vehicle and vehicle circle ----
    RecChunk C = {};
    unsigned long long e_next = jrw_end_mask(R, lane, jrw_flag(R, b, lane), true);
    int ep_k0 = 0, ep_tick = -1, ep_i = -1;
    double ep_px = NAN, ep_py = NAN;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        // the next chunk's ends ahead of the body: the frame offsets reach into it
        jrw_enter(C, R, k0c, e_next, true);
        e_next = jrw_end_mask(R, k + 64, jrw_flag(R, b, k + 64), true);
        const unsigned long long e_prev = C.e_prev, e_cur = C.e_cur, s_cur = C.s_cur;
        const unsigned long long s_prev = k0c == 0 ? 0ull : ((e_prev << 1) | 1ull);   // (bit 0: at or before the chunk's first tick)
        // the episode's own first and last tick where an offset can reach them: within the neighbouring chunks, else a bound that
        // is more than 20 ticks away in any case
        const unsigned long long sb = s_cur & upto, eb = e_cur & from;
        const int ks = sb ? k0c + 63 - __builtin_clzll(sb) : (s_prev ? k0c - 1 - __builtin_clzll(s_prev) : k0c - 64);
        const int ke = eb ? k0c + __builtin_ctzll(eb) : (e_next ? k0c + 64 + __builtin_ctzll(e_next) : k0c + 127);

        double clear = NAN, hpx = NAN, hpy = NAN;
        int who = -1, crow = 0x7fffffff, row = 0x7fffffff, hi = -1;
        if (valid && n_veh > 0) {
            double ex, ey, eyaw, es, ec;
            jrw_pose(R, b, k, ex, ey, eyaw);
            sincos(eyaw, &es, &ec);
            const double ecx[2] = {ex + ec * V.cc_f, ex + ec * V.cc_r}, ecy[2] = {ey + es * V.cc_f, ey + es * V.cc_r};
            for (int i = 0; i < n_veh; ++i) {
                const double4 sh = jcf_vehicle_row(V, L, i);
                for (int off = -w; off <= w; ++off) {
                    int kc = k - off;
                    kc = kc < ks ? ks : kc; kc = kc > ke ? ke : kc;
                    double vx, vy, vyaw, vs, vc;
                    jcf_vehicle_pose(V, L, i, kc, vx, vy, vyaw);
                    sincos(vyaw, &vs, &vc);
                    for (int c = 0; c < 2; ++c) {
                        const double cc = c ? sh.y : sh.x;
                        const double px = vx + vc * cc, py = vy + vs * cc;
                        for (int a = 0; a < 2; ++a) {
                            const double dx = ecx[a] - px, dy = ecy[a] - py;
                            const double d2 = dx * dx + dy * dy;
                            const int r = ((a * n_veh + i) * nw + (off + w)) * 2 + c;
                            if (d2 <= sh.w && r < row) { row = r; hpx = px; hpy = py; hi = i; }
                            if (off == 0) {
                                const double cl = sqrt(d2) - sh.z;
                                if (crow == 0x7fffffff || cl < clear || (cl == clear && r < crow)) { clear = cl; who = i; crow = r; }
                            }
                        }
                    }
                }
            }
        }
        if (row == 0x7fffffff) row = -1;
        const unsigned long long touch = __ballot(valid && row >= 0);

        if (valid) {
            const size_t q = (size_t)k * B + b;
            P.clear[q] = clear; P.who[q] = who; P.row[q] = row;
            if (!((s_cur >> lane) & 1ull)) {   // not an episode's first tick: no episode outputs
                P.hit_tick[q] = -1; P.hit_frame[q] = -1; P.hit_xy[2 * q] = NAN; P.hit_xy[2 * q + 1] = NAN;
            }
        }
        // the episodes of this chunk, one after the other (every branch is uniform: the masks are ballots)
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) { ep_k0 = k0c + pos; ep_tick = -1; ep_i = -1; ep_px = NAN; ep_py = NAN; }
            const unsigned long long h = touch & jrw_lanes(pos, e);
            if (ep_tick < 0 && h != 0ull) {
                const int t = (int)__builtin_ctzll(h);
                ep_tick = k0c + t;
                ep_i = __shfl(hi, t); ep_px = __shfl(hpx, t); ep_py = __shfl(hpy, t);
            }
            if (ends && lane == 0) {           // the episode ends here: its slot, written once in this sweep
                const size_t q = (size_t)ep_k0 * B + b;
                P.hit_tick[q] = ep_tick; P.hit_frame[q] = ep_i; P.hit_xy[2 * q] = ep_px; P.hit_xy[2 * q + 1] = ep_py;
            }
        });
    }
    if (n_veh == 0) return;        // every episode slot holds -1 / -1 / NaN already
    __threadfence();               // sweep 2 reads, in other lanes, what lane 0 wrote

    // ---- sweep 2: per episode with a touching row, the earliest frame at which each ego circle touches that vehicle circle ----
    int s_k0 = 0, s_tick = -1, bf = -1, br = -1;
    double s_px = NAN, s_py = NAN, s_thr_sq = 0.0;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        jrw_enter(C, R, k0c, jrw_end_mask(R, k, jrw_flag(R, b, k), true), true);
        double fx = NAN, fy = NAN, rx = NAN, ry = NAN;
        if (valid) {
            double ex, ey, eyaw, es, ec;
            jrw_pose(R, b, k, ex, ey, eyaw);
            sincos(eyaw, &es, &ec);
            fx = ex + ec * V.cc_f; fy = ey + es * V.cc_f; rx = ex + ec * V.cc_r; ry = ey + es * V.cc_r;
        }
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) {
                s_k0 = k0c + pos; bf = -1; br = -1;
                const size_t q = (size_t)s_k0 * B + b;
                s_tick = P.hit_tick[q];
                if (s_tick >= 0) {
                    s_px = P.hit_xy[2 * q]; s_py = P.hit_xy[2 * q + 1];
                    int i = P.hit_frame[q];
                    i = i < 0 ? 0 : (i >= n_veh ? n_veh - 1 : i);
                    s_thr_sq = jcf_vehicle_row(V, L, i).w;
                }
            }
            if (s_tick >= 0) {
                const bool in = valid && lane >= pos && lane <= e;
                const double dfx = s_px - fx, dfy = s_py - fy, drx = s_px - rx, dry = s_py - ry;
                const unsigned long long tf = __ballot(in && dfx * dfx + dfy * dfy <= s_thr_sq);
                const unsigned long long tr = __ballot(in && drx * drx + dry * dry <= s_thr_sq);
                if (bf < 0 && tf != 0ull) bf = k0c + (int)__builtin_ctzll(tf);
                if (br < 0 && tr != 0ull) br = k0c + (int)__builtin_ctzll(tr);
                if (ends) {                    // the episode ends here: front ++ rear, the first hit's index modulo the length
                    const int fr = bf >= 0 ? bf : br;
                    if (fr >= 0) {
                        double hx, hy, hyaw;
                        jrw_pose(R, b, fr, hx, hy, hyaw);
                        if (lane == 0) {
                            const size_t q = (size_t)s_k0 * B + b;
                            P.hit_frame[q] = fr - s_k0; P.hit_xy[2 * q] = hx; P.hit_xy[2 * q + 1] = hy;
                        }
                    }
                }
            }
        });
    }
}
