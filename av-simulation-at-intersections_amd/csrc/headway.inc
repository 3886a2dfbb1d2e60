// Every recorded vehicle projected onto the ego's path (DESIGN.md section 25): for ego b, tick k and place i of its vehicle list
// (conflicts.inc's VehicleListP, list and circle-centre arithmetic, operation for operation), the road between the two along path
// path_id[b] of a path table that is the call's own (path_project.inc's table, clamp, search and projection rule, the text that
// tracking.inc runs): the space headway `gap` of the two circle-pair intervals, the lateral offset `lat` of the vehicle's nearer
// centre, the closing speed `rate` along the path and the time to collision; per tick the leader, its gap, the time headway and the
// smallest TTC.  Everything is taken at the start of tick k.  One pass over the History recorder's buffers, walked as
// recorder_walk.inc says: one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t.
//
// The search is the hot part: a lane has 2 + 2 * n_veh query points (front and rear circle centre of the ego and of each vehicle)
// and every one is searched over the same path.  A path point's address is the same in every lane, so jpp_search<Q> reads px / py
// as scalar loads, four points to a step, and one loaded point serves every query of the group that is held in registers: each
// query keeps its own smallest squared distance and index and replaces them on strict < in ascending order
// (calc_nearest_index(state, cx, cy, 0) of main/lib/trajectories.py:89-97).  The groups: the ego's two centres, then the vehicles
// JSIM_HW_GROUP = 4 places (8 queries) to a pass and the rest in groups of 2 and 1 places after the binary digits of n_veh
// (wave-uniform), so that no pass carries an absent query: two passes over the path for four vehicles, three for eight, four at the
// most (seven).  Eight places to a pass fit without scratch too, but at 282 VGPRs -- one wavefront per SIMD; with four the kernel
// takes 185 and two wavefronts share a SIMD (DESIGN.md section 25).  After a search each lane gathers the at most three points around
// each index with vector loads (jpp_project).  Per episode, by butterflies over the segment's lanes and a wave-uniform carry
// (episodes.inc), written by lane 0 at the slot of the episode's first tick when the episode ends (the last record closes the
// running one, as in conflicts.inc).

#ifndef JSIM_HW_GROUP
#define JSIM_HW_GROUP 4       // places to a pass: 4 or 8 (a diagnostic build's -DJSIM_HW_GROUP=8)
#endif

struct HeadwayP {
    VehicleListP V;           // rows: (cc_front, cc_rear, radius, thr = the ego's radius + its own)
    PathTableP T;
    double r_ego, margin;
    int *lead;                // [n][B]
    double *lead_gap, *thw, *ttc;
    int *ttc_who;
    double *u_ego;
    int *ep_i;                // [n][B][JSIM_HW_NI], at an episode's first slot
    double *ep_d;             // [n][B][JSIM_HW_ND]
    double *gap, *lat, *rate; // [n][B][JSIM_MAX_OBS] or NULL: not written
};

// Pose and speed at the start of tick k: an ego's by jrw_pose's rule, a scripted vehicle's its record of the tick
struct HwState { double x, y, yaw, v; };
__device__ __forceinline__ bool jhw_finite(const HwState &S) { return isfinite(S.x) && isfinite(S.y) && isfinite(S.yaw) && isfinite(S.v); }
__device__ __forceinline__ HwState jhw_ego_state(const RecorderBuf &R, int e, int k)
{
    if (k == 0 || jrw_is_end(R.flags[(size_t)(k - 1) * R.B + e])) {
        const double *p = (k == 0 ? R.x_first : R.x_spawn) + 4 * (size_t)e;
        return HwState{p[0], p[1], p[3], p[2]};
    }
    const double *p = R.rec + JSIM_REC_FIELDS * ((size_t)(k - 1) * R.B + e);
    return HwState{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ HwState jhw_vehicle_state(const VehicleListP &V, const ConflictList &L, int i, int k)
{
    if (i < L.ns) {
        const double *c = jcf_scripted(V, L, i, k);
        return HwState{c[0], c[1], c[3], c[2]};
    }
    return jhw_ego_state(V.R, jcf_mate(L, i), k);
}

// What a tick keeps of its places: the leader and the smallest time to collision, places in ascending order, replaced on strict <
struct HwTick { int lead, ttc_who; double lead_gap, ttc; };

// The places [g0, g0 + VG) of the list: their 2 * VG circle centres in one pass over the path.  `live`: the lane has a tick and its
// ego a finite pose (else every place is NaN); e_lo, e_hi, u_e: the ego's interval and speed along the path
template <int VG>
__device__ __forceinline__ void jhw_group(const HeadwayP &P, const double *__restrict__ px, const double *__restrict__ py,
                                          const ConflictList &L, int lo, int np, int g0, int k, bool valid, bool live, double e_lo,
                                          double e_hi, double u_e, size_t q, HwTick &T)
{
    HwState S[VG];
    double4 sh[VG];
    double x[2 * VG], y[2 * VG];
    int bi[2 * VG];
#pragma unroll
    for (int j = 0; j < VG; ++j) {
        sh[j] = jcf_vehicle_row(P.V, L, g0 + j);
        S[j] = HwState{NAN, NAN, NAN, NAN};
        if (live) S[j] = jhw_vehicle_state(P.V, L, g0 + j, k);
        double vs, vc;
        sincos(S[j].yaw, &vs, &vc);
        x[2 * j] = S[j].x + vc * sh[j].x; y[2 * j] = S[j].y + vs * sh[j].x;
        x[2 * j + 1] = S[j].x + vc * sh[j].y; y[2 * j + 1] = S[j].y + vs * sh[j].y;
    }
    jpp_search<2 * VG>(px + lo, py + lo, np, x, y, bi);
#pragma unroll
    for (int j = 0; j < VG; ++j) {
        const int i = g0 + j;
        double gap = NAN, lat = NAN, rate = NAN, ttc = NAN;
        bool on = false;
        if (live && jhw_finite(S[j])) {
            const PathProj F = jpp_project(P.T, px, py, lo, np, bi[2 * j], x[2 * j], y[2 * j]);
            const PathProj R = jpp_project(P.T, px, py, lo, np, bi[2 * j + 1], x[2 * j + 1], y[2 * j + 1]);
            const double v_lo = fmin(F.s, R.s) - sh[j].z, v_hi = fmax(F.s, R.s) + sh[j].z;
            const double ahead = v_lo - e_hi, behind = v_hi - e_lo;
            gap = ahead > 0.0 ? ahead : (behind < 0.0 ? behind : 0.0);
            lat = fabs(R.d) < fabs(F.d) ? R.d : F.d;          // the front centre on a tie
            rate = S[j].v * cos(S[j].yaw - F.ref) - u_e;
            on = fabs(lat) <= sh[j].w + P.margin;
            if (on) {
                if (gap == 0.0) ttc = 0.0;
                else if (gap > 0.0) ttc = rate < 0.0 ? gap / -rate : INFINITY;
                else ttc = rate > 0.0 ? -gap / rate : INFINITY;
            }
        }
        if (P.gap && valid) {
            P.gap[JSIM_MAX_OBS * q + i] = gap; P.lat[JSIM_MAX_OBS * q + i] = lat; P.rate[JSIM_MAX_OBS * q + i] = rate;
        }
        if (on && gap >= 0.0 && (T.lead < 0 || gap < T.lead_gap)) { T.lead = i; T.lead_gap = gap; }
        if (ttc == ttc && (T.ttc_who < 0 || ttc < T.ttc)) { T.ttc_who = i; T.ttc = ttc; }
    }
}

// The kernel's body.  `px`, `py` (= P.T.px, P.T.py) are restrict-qualified: the stores of this body are known not to alias the table
// that path_project.inc's search and gather read.
__device__ __forceinline__ void jhw_ticks(const HeadwayP &P, const double *__restrict__ px, const double *__restrict__ py)
{
    const RecorderBuf &R = P.V.R;
    const int lane = threadIdx.x, b = blockIdx.x, B = R.B, n = R.n_ticks;
    const ConflictList L = jcf_list(P.V, b);
    const int n_veh = L.ns + L.nm;
    const PathRange pr = jpp_path(P.T, b);
    const int lo = pr.lo, np = pr.np;
    const bool any = n_veh > 0 && np > 0;                     // (uniform: the list and the path are the wavefront's)

    RecChunk C = {};
    int ep_k0 = 0, ep_n = 0, ep_lead = 0, ep_nf = 0, ep_gap_who = -1, ep_ttc_who = -1;
    EpisodeExt ep_gap = {NAN, -1}, ep_thw = {NAN, -1}, ep_ttc = {NAN, -1};
    double ep_sum = 0.0;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        const size_t q = (size_t)k * B + b;
        jrw_enter(C, R, k0c, jrw_end_mask(R, k, jrw_flag(R, b, k), true), true);

        HwTick T = {-1, -1, NAN, NAN};
        double thw = NAN, u_e = NAN;
        if (any) {
            HwState E = {NAN, NAN, NAN, NAN};
            if (valid) E = jhw_ego_state(R, b, k);
            const bool live = valid && jhw_finite(E);
            double es, ec;
            sincos(E.yaw, &es, &ec);
            const double ex[2] = {E.x + ec * P.V.cc_f, E.x + ec * P.V.cc_r}, ey[2] = {E.y + es * P.V.cc_f, E.y + es * P.V.cc_r};
            int ei[2];
            jpp_search<2>(px + lo, py + lo, np, ex, ey, ei);
            double e_lo = NAN, e_hi = NAN;
            if (live) {
                const PathProj F = jpp_project(P.T, px, py, lo, np, ei[0], ex[0], ey[0]);
                const PathProj Rr = jpp_project(P.T, px, py, lo, np, ei[1], ex[1], ey[1]);
                e_lo = fmin(F.s, Rr.s) - P.r_ego; e_hi = fmax(F.s, Rr.s) + P.r_ego;
                u_e = E.v * cos(E.yaw - F.ref);
            }
            int g0 = 0;
            for (; n_veh - g0 >= JSIM_HW_GROUP; g0 += JSIM_HW_GROUP)
                jhw_group<JSIM_HW_GROUP>(P, px, py, L, lo, np, g0, k, valid, live, e_lo, e_hi, u_e, q, T);
            if (JSIM_HW_GROUP > 4 && (n_veh & 4)) { jhw_group<4>(P, px, py, L, lo, np, g0, k, valid, live, e_lo, e_hi, u_e, q, T); g0 += 4; }
            if (n_veh & 2) { jhw_group<2>(P, px, py, L, lo, np, g0, k, valid, live, e_lo, e_hi, u_e, q, T); g0 += 2; }
            if (n_veh & 1) { jhw_group<1>(P, px, py, L, lo, np, g0, k, valid, live, e_lo, e_hi, u_e, q, T); }
            if (T.lead >= 0) thw = T.lead_gap == 0.0 ? 0.0 : (u_e > 0.0 ? T.lead_gap / u_e : INFINITY);
        }

        if (valid) {
            P.lead[q] = T.lead; P.lead_gap[q] = T.lead_gap; P.thw[q] = thw; P.ttc[q] = T.ttc; P.ttc_who[q] = T.ttc_who; P.u_ego[q] = u_e;
            if (P.gap)                                        // the places nobody holds
                for (int i = any ? n_veh : 0; i < JSIM_MAX_OBS; ++i) {
                    P.gap[JSIM_MAX_OBS * q + i] = NAN; P.lat[JSIM_MAX_OBS * q + i] = NAN; P.rate[JSIM_MAX_OBS * q + i] = NAN;
                }
            jrw_blank_slot(C, lane, q, P.ep_i, JSIM_HW_NI, P.ep_d, JSIM_HW_ND);
        }
        // the episodes of this chunk, one after the other (every branch is uniform: the masks are ballots, the extremes the wave's)
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) {
                ep_k0 = k0c + pos; ep_n = 0; ep_lead = 0; ep_nf = 0; ep_gap_who = -1; ep_ttc_who = -1; ep_sum = 0.0;
                ep_gap = EpisodeExt{NAN, -1}; ep_thw = EpisodeExt{NAN, -1}; ep_ttc = EpisodeExt{NAN, -1};
            }
            const bool in = lane >= pos && lane <= e;
            const bool fin = in && isfinite(thw);
            int at = 0;
            ep_n += e - pos + 1;
            ep_lead += __popcll(__ballot(in && T.lead >= 0));
            ep_nf += __popcll(__ballot(fin));
            ep_sum += jep_sum(fin ? thw : 0.0);
            if (jep_extreme(ep_gap, in ? T.lead_gap : NAN, true, k0c, at)) ep_gap_who = __shfl(T.lead, at);
            jep_extreme(ep_thw, in ? thw : NAN, true, k0c, at);
            if (jep_extreme(ep_ttc, in ? T.ttc : NAN, true, k0c, at)) ep_ttc_who = __shfl(T.ttc_who, at);
            if (ends && lane == 0) {                          // the episode ends here: its slot, written once
                const size_t s = (size_t)ep_k0 * B + b;
                int *I = P.ep_i + JSIM_HW_NI * s;
                double *D = P.ep_d + JSIM_HW_ND * s;
                I[JSIM_HW_TICKS] = ep_n; I[JSIM_HW_LEAD_TICKS] = ep_lead; I[JSIM_HW_GAP_TICK] = ep_gap.tick; I[JSIM_HW_GAP_WHO] = ep_gap_who;
                I[JSIM_HW_THW_TICK] = ep_thw.tick; I[JSIM_HW_TTC_TICK] = ep_ttc.tick; I[JSIM_HW_TTC_WHO] = ep_ttc_who;
                D[JSIM_HW_GAP_MIN] = ep_gap.v; D[JSIM_HW_THW_MIN] = ep_thw.v; D[JSIM_HW_TTC_MIN] = ep_ttc.v;
                D[JSIM_HW_THW_MEAN] = ep_nf > 0 ? ep_sum / (double)ep_nf : NAN;
            }
        });
    }
}

__global__ __launch_bounds__(64) void headway_ticks_kernel(const HeadwayP P)
{
    jhw_ticks(P, P.T.px, P.T.py);
}
