// The time gap between an ego and each vehicle per recorded tick (DESIGN.md section 23): for ego b, tick k and vehicle i of its list
// (conflicts.inc's VehicleListP: its list, shapes, thresholds and circle-centre arithmetic, operation for operation), the offset
// `off` of smallest |off| <= W at which one of the four circle pairs of (ego at tick k, vehicle i at tick k - off) touches -- off > 0: the vehicle
// stood here first, off < 0: the ego did; -o in front of +o.  The least frame_window at which check_collision_moving_cars /
// check_collision_moving_bicycle (main/lib/collision_avoidance.py:68-166) report a hit on an episode is the smallest |off| of its
// ticks.  One pass over the History recorder's buffers, walked as recorder_walk.inc says: one wavefront per ego, ticks 64 at a time,
// lane t owns tick k0c + t.
//
// The 64 lanes of a chunk share the vehicle ticks k0c - W .. k0c + 63 + W: their circle centres are made once per chunk -- one pose
// load and one sincos per (vehicle, vehicle tick) -- and kept in LDS as double2, [circle][vehicle][64 + 2W]; lane t reads offset off
// at entry t + W - off, consecutive lanes consecutive 16-byte slots.  Per episode the smallest |off|, its first tick, the lowest
// place that has it there and that place's signed offset, by a wavefront minimum over (gap, lane) per segment, written at the slot
// of the episode's first tick when the episode ends (the last record closes the running one, as in conflicts.inc).

struct GapP {
    VehicleListP V;           // rows: (cc_front, cc_rear, thr, thr_sq), as conflict_ticks_kernel takes them
    int W, within;            // the window 0 .. JSIM_GAP_MAX_WINDOW; 0: vehicle ticks of the ego's own episode only, 1: every recorded tick
    unsigned long long *off;  // [n][B] eight int8, place i in byte i
    int *ep_gap, *ep_tick, *ep_who, *ep_off; // [n][B], at an episode's first slot
};

__global__ __launch_bounds__(64) void gap_ticks_kernel(const GapP G)
{
    extern __shared__ double2 jgp_centres[];         // [2][n_veh][64 + 2W]: (x, y) of circle c of vehicle i at tick k0c - W + s
    const VehicleListP &V = G.V;
    const RecorderBuf &R = V.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks, W = G.W, span = 64 + 2 * G.W;
    const ConflictList L = jcf_list(V, b);
    const int n_veh = L.ns + L.nm;
    const unsigned long long upto = ~0ull >> (63 - lane), from = ~0ull << lane;   // bits 0 .. lane, bits lane .. 63
    const unsigned long long none8 = 0x8080808080808080ull;                        // JSIM_GAP_NONE in every place

    RecChunk C = {};
    unsigned long long e_next = jrw_end_mask(R, lane, jrw_flag(R, b, lane), true);
    int ep_k0 = 0, ep_gap = -1, ep_tick = -1, ep_who = -1, ep_off = JSIM_GAP_NONE;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        // the next chunk's ends ahead of the body: the offsets reach into it
        jrw_enter(C, R, k0c, e_next, true);
        e_next = jrw_end_mask(R, k + 64, jrw_flag(R, b, k + 64), true);
        const unsigned long long e_prev = C.e_prev, e_cur = C.e_cur, s_cur = C.s_cur;
        const unsigned long long s_prev = k0c == 0 ? 0ull : ((e_prev << 1) | 1ull);   // (bit 0: at or before the chunk's first tick)
        // the episode's own first and last tick where an offset can reach them: within the neighbouring chunks, else a bound that is
        // more than 63 ticks away in any case; under within = 1 the record's own
        // (the bounds outside the chunk are the wavefront's, the ones inside it each lane's)
        const int ks_out = G.within ? 0 : (s_prev ? k0c - 1 - __builtin_clzll(s_prev) : k0c - 64);
        const int ke_out = G.within ? n - 1 : (e_next ? k0c + 64 + __builtin_ctzll(e_next) : k0c + 127);
        const unsigned long long sb = G.within ? 0ull : (s_cur & upto), eb = G.within ? 0ull : (e_cur & from);
        const int ks = sb ? k0c + 63 - __builtin_clzll(sb) : ks_out;
        const int ke = eb ? k0c + __builtin_ctzll(eb) : ke_out;

        // the circle centres of the vehicle ticks this chunk can reach, once
        for (int i = 0; i < n_veh; ++i) {
            const double4 sh = jcf_vehicle_row(V, L, i);
            for (int s = lane; s < span; s += 64) {
                const int kv = k0c - W + s;
                if (kv >= 0 && kv < n) {
                    double vx, vy, vyaw, vs, vc;
                    jcf_vehicle_pose(V, L, i, kv, vx, vy, vyaw);
                    sincos(vyaw, &vs, &vc);
                    jgp_centres[i * span + s] = double2{vx + vc * sh.x, vy + vs * sh.x};
                    jgp_centres[(n_veh + i) * span + s] = double2{vx + vc * sh.y, vy + vs * sh.y};
                }
            }
        }
        __syncthreads();

        unsigned long long offs = none8;
        int gap = 0x7fffffff, who = -1, soff = JSIM_GAP_NONE;
        if (valid && n_veh > 0) {
            double ex, ey, eyaw, es, ec;
            jrw_pose(R, b, k, ex, ey, eyaw);
            sincos(eyaw, &es, &ec);
            const double ecx[2] = {ex + ec * V.cc_f, ex + ec * V.cc_r}, ecy[2] = {ey + es * V.cc_f, ey + es * V.cc_r};
            for (int i = 0; i < n_veh; ++i) {
                const double thr_sq = jcf_vehicle_row(V, L, i).w;
                const double2 *front = jgp_centres + i * span + (lane + W), *rear = jgp_centres + (n_veh + i) * span + (lane + W);
                // the vehicle at tick k - off against the ego at tick k: any of the four circle pairs
                auto touches = [&](int off) {
                    const double2 pc[2] = {front[-off], rear[-off]};
                    bool t = false;
                    for (int c = 0; c < 2; ++c)
                        for (int a = 0; a < 2; ++a) {
                            const double dx = ecx[a] - pc[c].x, dy = ecy[a] - pc[c].y;
                            const double d2 = dx * dx + dy * dy;
                            t = t || d2 <= thr_sq;
                        }
                    return t;
                };
                int found = JSIM_GAP_NONE;
                for (int o = 0; o <= W && found == JSIM_GAP_NONE; ++o) {   // by ascending |off|, -o in front of +o
                    if (k + o <= ke && touches(-o)) found = -o;
                    else if (o > 0 && k - o >= ks && touches(o)) found = o;
                }
                if (found != JSIM_GAP_NONE) {
                    offs = (offs & ~(0xffull << (8 * i))) | ((unsigned long long)(unsigned char)found << (8 * i));
                    const int g = found < 0 ? -found : found;
                    if (g < gap) { gap = g; who = i; soff = found; }
                }
            }
        }
        __syncthreads();                       // the next chunk's centres replace these

        if (valid) {
            const size_t q = (size_t)k * B + b;
            G.off[q] = offs;
            if (!((s_cur >> lane) & 1ull)) {   // not an episode's first tick: no episode outputs
                G.ep_gap[q] = -1; G.ep_tick[q] = -1; G.ep_who[q] = -1; G.ep_off[q] = JSIM_GAP_NONE;
            }
        }
        // the episodes of this chunk, one after the other (every branch is uniform: the masks are ballots, the minimum is the wave's)
        const int key = who >= 0 ? gap * 64 + lane : 0x7fffffff;   // the smallest gap, then the earliest tick
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) { ep_k0 = k0c + pos; ep_gap = -1; ep_tick = -1; ep_who = -1; ep_off = JSIM_GAP_NONE; }
            int best = (lane >= pos && lane <= e) ? key : 0x7fffffff;
            for (int m = 32; m > 0; m >>= 1) {
                const int other = __shfl_xor(best, m);
                best = other < best ? other : best;
            }
            if (best != 0x7fffffff && (ep_gap < 0 || (best >> 6) < ep_gap)) {
                const int t = best & 63;
                ep_gap = best >> 6; ep_tick = k0c + t;
                ep_who = __shfl(who, t); ep_off = __shfl(soff, t);
            }
            if (ends && lane == 0) {           // the episode ends here: its slot, written once
                const size_t q = (size_t)ep_k0 * B + b;
                G.ep_gap[q] = ep_gap; G.ep_tick[q] = ep_tick; G.ep_who[q] = ep_who; G.ep_off[q] = ep_off;
            }
        });
    }
}
