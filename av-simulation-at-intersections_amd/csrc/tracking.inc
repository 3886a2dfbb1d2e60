// Every recorded pose projected onto a path (DESIGN.md section 24): for ego b and tick k the pose rec[k] -- History.x[k], .y[k],
// .yaw[k], the state after the plant step -- against path path_id[b] of a path table that is the call's own: idx =
// calc_nearest_index(state, cx, cy, 0) of main/lib/trajectories.py:89-97, the segment beside it that holds the foot of the
// perpendicular, the arc length s of the foot, the signed lateral offset d (left of the direction of travel is positive) and the
// heading error e_yaw against the path's yaw at the foot -- what plot_trajectories_comparison of
// main/scenarios/mpc_sensitivity_analysis*.py draws and never measures.  One pass over the History recorder's buffers, walked as
// recorder_walk.inc says: one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t.
//
// The path table, the clamp of the ego's path, the search (one query a lane: jpp_search<1>) and the segment rule are
// path_project.inc's, which headway.inc shares; this file's own are the pose it projects, e_yaw from the rule's reference yaw and the
// episode outputs.  Per episode, by butterflies over the segment's lanes and a wave-uniform carry (episodes.inc): the ticks, the
// largest |d| and its first tick, the mean of d * d, the largest |e_yaw|, s at the first and the last tick; written by lane 0 at
// the slot of the episode's first tick when the episode ends (the last record closes the running one, as in conflicts.inc).

struct TrackP {
    int B, n_ticks;
    const double *rec;        // [n][B][JSIM_REC_FIELDS]
    const int *flags;         // [n][B]
    PathTableP T;
    int *idx, *seg;           // [n][B]
    double *s, *d, *e_yaw;    // [n][B]
    int *ep_i;                // [n][B][JSIM_TRK_NI], at an episode's first slot
    double *ep_d;             // [n][B][JSIM_TRK_ND]
};

// The kernel's body.  `px`, `py` (= P.T.px, P.T.py) are restrict-qualified: the stores of this body are known not to alias the table
// that path_project.inc's search and gather read.
__device__ __forceinline__ void jtk_ticks(const TrackP &P, const double *__restrict__ px, const double *__restrict__ py)
{
    const int lane = threadIdx.x, b = blockIdx.x, B = P.B, n = P.n_ticks;
    const RecorderBuf R = {B, n, P.rec, P.flags, nullptr, nullptr};
    const PathRange pr = jpp_path(P.T, b);
    const int lo = pr.lo, np = pr.np;

    RecChunk C = {};
    int ep_k0 = 0, ep_n = 0, ep_nd = 0;
    EpisodeExt ep_dmax = {NAN, -1};
    double ep_sum = 0.0, ep_yaw = NAN, ep_s0 = NAN, ep_s1 = NAN;
    for (int k0c = 0; k0c < n; k0c += 64) {
        const int k = k0c + lane;
        const bool valid = k < n;
        jrw_enter(C, R, k0c, jrw_end_mask(R, k, jrw_flag(R, b, k), true), true);

        double x = NAN, y = NAN, yaw = NAN;
        if (valid) {
            const double *r = P.rec + JSIM_REC_FIELDS * ((size_t)k * B + b);
            x = r[0]; y = r[1]; yaw = r[2];
        }
        const bool ok = np > 0 && isfinite(x) && isfinite(y) && isfinite(yaw);
        int idx = -1, seg = -1;
        double s = NAN, d = NAN, e_yaw = NAN;
        if (np > 0) {                                         // (uniform: the ego's path is the wavefront's)
            const double qx[1] = {x}, qy[1] = {y};
            int best_i[1];
            jpp_search<1>(px + lo, py + lo, np, qx, qy, best_i);
            if (ok) {
                idx = best_i[0];
                const PathProj F = jpp_project(P.T, px, py, lo, np, idx, x, y);
                seg = F.seg; s = F.s; d = F.d;
                e_yaw = jpl_pymod((yaw - F.ref) + 3.141592653589793, 6.283185307179586) - 3.141592653589793;
            }
        }

        if (valid) {
            const size_t q = (size_t)k * B + b;
            P.idx[q] = idx; P.seg[q] = seg; P.s[q] = s; P.d[q] = d; P.e_yaw[q] = e_yaw;
            jrw_blank_slot(C, lane, q, P.ep_i, JSIM_TRK_NI, P.ep_d, JSIM_TRK_ND);
        }
        // the episodes of this chunk, one after the other (every branch is uniform: the masks are ballots, the extremes the wave's)
        const double ad = fabs(d), ay = fabs(e_yaw);
        jrw_segments(C, [&](int pos, int e, bool starts, bool ends) {
            if (starts) {
                ep_k0 = k0c + pos; ep_n = 0; ep_nd = 0; ep_dmax = EpisodeExt{NAN, -1};
                ep_sum = 0.0; ep_yaw = NAN; ep_s0 = __shfl(s, pos);
            }
            const bool in = lane >= pos && lane <= e;
            const bool has = in && d == d;
            int at = 0;
            ep_n += e - pos + 1;
            ep_nd += __popcll(__ballot(has));
            ep_sum += jep_sum(has ? d * d : 0.0);
            jep_extreme(ep_dmax, in ? ad : NAN, false, k0c, at);
            ep_yaw = fmax(ep_yaw, jep_max(in ? ay : NAN));
            ep_s1 = __shfl(s, e);
            if (ends && lane == 0) {                          // the episode ends here: its slot, written once
                const size_t q = (size_t)ep_k0 * B + b;
                int *I = P.ep_i + JSIM_TRK_NI * q;
                double *D = P.ep_d + JSIM_TRK_ND * q;
                I[JSIM_TRK_TICKS] = ep_n; I[JSIM_TRK_D_TICK] = ep_dmax.tick;
                D[JSIM_TRK_D_MAX] = ep_dmax.v; D[JSIM_TRK_D2_MEAN] = ep_nd > 0 ? ep_sum / (double)ep_nd : NAN;
                D[JSIM_TRK_YAW_MAX] = ep_yaw; D[JSIM_TRK_S_FIRST] = ep_s0; D[JSIM_TRK_S_LAST] = ep_s1;
            }
        });
    }
}

__global__ __launch_bounds__(64) void tracking_ticks_kernel(const TrackP P)
{
    jtk_ticks(P, P.T.px, P.T.py);
}
