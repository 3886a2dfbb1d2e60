// Static-obstacle clearance and contact per recorded tick (DESIGN.md section 18): what check_collision of main/lib/obstacles.py
// (:157-176) on Obstacle.to_convex(margin) -- the planner's collision test, main/lib/mp_search_ww_generic.py:199-215 -- and
// BoxObstacle / CircleObstacle.distance_to_point (:95-103, :150-154) answer when they are handed the driven poses' two collision
// circle centres (main/lib/trajectories.py:11-55), as one pass over the History recorder's buffers, walked as recorder_walk.inc says:
// one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t.
//
// Lane-parallel: the pose, one sincos, the two circle centres, `clear`, `who` and `hit`.  An obstacle row is the same for every lane
// of the wavefront: its address depends on the ego's set and the loop counter alone, so the row is read as wave-uniform values.
// Per episode, from ballots: the first touching tick, written at the slot of the episode's first tick by lane 0.

struct StaticP {
    RecorderBuf R;
    int n_sets, include_hidden;
    const int *set_of;        // [B] the ego's obstacle set; outside [0, n_sets): an empty set
    const int *set_off;       // [n_sets + 1] a set's rows are [set_off[s], set_off[s + 1])
    const double *rows;       // [n_rows][JSIM_STATIC_ROW]
    double cc_f, cc_r, radius; // the ego's circle offsets and radius
    double *clear;            // [n][B]
    int *who, *hit, *off_tick; // [n][B]; off_tick at an episode's first slot
};

// BoxObstacle.distance_to_point / CircleObstacle.distance_to_point of one centre; g = the row's geometry entries
__device__ __forceinline__ double jsf_distance(bool circle, double g0, double g1, double g2, double g3, double x, double y)
{
    if (circle) {
        const double dx = g0 - x, dy = g1 - y;
        return fmax(0.0, sqrt(dx * dx + dy * dy) - g2);
    }
    const double dx = fmax(fmax(g0 - x, 0.0), x - g2), dy = fmax(fmax(g1 - y, 0.0), y - g3);
    return sqrt(dx * dx + dy * dy);
}

// The kernel's body.  `rows` (= P.rows) is restrict-qualified: a row's address is the same in every lane, and with the stores of
// this body known not to alias the table its loads are scalar loads, the row's entries wave-uniform operands.
__device__ __forceinline__ void jsf_ticks(const StaticP &P, const double *__restrict__ rows)
{
    const RecorderBuf &R = P.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks;
    const int s = P.set_of[b];
    int lo = 0, hi = 0;
    if (s >= 0 && s < P.n_sets) { lo = P.set_off[s]; hi = P.set_off[s + 1]; }

    RecChunk C = {};
    int ep_k0 = 0, ep_tick = -1;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        jrw_enter(C, R, k0c, jrw_end_mask(R, k, jrw_flag(R, b, k), true), true);

        double clear = NAN;
        int who = -1, hit = -1;
        if (valid) {
            double ex, ey, eyaw, es, ec;
            jrw_pose(R, b, k, ex, ey, eyaw);
            sincos(eyaw, &es, &ec);
            const double fx = ex + ec * P.cc_f, fy = ey + es * P.cc_f, rx = ex + ec * P.cc_r, ry = ey + es * P.cc_r;
            for (int o = lo; o < hi; ++o) {
                const double *r = rows + JSIM_STATIC_ROW * (size_t)o;
                if (!P.include_hidden && r[1] != 0.0) continue;
                const bool circle = r[0] != 0.0;
                const double df = jsf_distance(circle, r[3], r[4], r[5], r[6], fx, fy);
                const double dr = jsf_distance(circle, r[3], r[4], r[5], r[6], rx, ry);
                const double cl = fmin(df, dr) - P.radius;
                if (who < 0 || cl < clear) { clear = cl; who = o - lo; }
                // inside every half-plane of to_convex(margin), for at least one of the two centres
                const int n_hp = (int)r[2];
                bool tf = true, tr = true;
                for (int h = 0; h < n_hp; ++h) {
                    const double ha = r[8 + 3 * h], hb = r[9 + 3 * h], hc = r[10 + 3 * h];
                    tf = tf && (ha * fx + hb * fy) + hc <= 0.0;
                    tr = tr && (ha * rx + hb * ry) + hc <= 0.0;
                }
                if (hit < 0 && (tf || tr)) hit = o - lo;
            }
        }
        const unsigned long long touch = __ballot(valid && hit >= 0);

        if (valid) {
            const size_t q = (size_t)k * B + b;
            P.clear[q] = clear; P.who[q] = who; P.hit[q] = hit;
            if (!((C.s_cur >> lane) & 1ull)) P.off_tick[q] = -1;    // not an episode's first tick
        }
        // the episodes of this chunk, one after the other (every branch is uniform: the masks are ballots)
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) { ep_k0 = k0c + pos; ep_tick = -1; }
            const unsigned long long h = touch & jrw_lanes(pos, e);
            if (ep_tick < 0 && h != 0ull) ep_tick = k0c + (int)__builtin_ctzll(h);
            if (ends && lane == 0) P.off_tick[(size_t)ep_k0 * B + b] = ep_tick;   // the episode ends here: its slot, written once
        });
    }
}

__global__ __launch_bounds__(64) void static_ticks_kernel(const StaticP P)
{
    jsf_ticks(P, P.rows);
}
