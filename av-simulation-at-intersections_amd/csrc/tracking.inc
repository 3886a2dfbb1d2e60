// Every recorded pose projected onto a path (DESIGN.md section 24): for ego b and tick k the pose rec[k] -- History.x[k], .y[k],
// .yaw[k], the state after the plant step -- against path path_id[b] of a path table that is the call's own: idx =
// calc_nearest_index(state, cx, cy, 0) of main/lib/trajectories.py:89-97, the segment beside it that holds the foot of the
// perpendicular, the arc length s of the foot, the signed lateral offset d (left of the direction of travel is positive) and the
// heading error e_yaw against the path's yaw at the foot -- what plot_trajectories_comparison of
// main/scenarios/mpc_sensitivity_analysis*.py draws and never measures.  One pass over the History recorder's buffers, walked as
// recorder_walk.inc says: one wavefront per ego, ticks 64 at a time, lane t owns tick k0c + t.
//
// The search: the path point of step i has the same address in every lane, so px / py are read through restrict-qualified pointers
// as scalar loads, four points to a step; each lane keeps its own smallest squared distance and replaces it on strict < in
// ascending order (np.argmin's first occurrence).  After it each lane gathers the at most three points around its own idx with
// vector loads.  Per episode, by butterflies over the segment's lanes and a wave-uniform carry (episodes.inc): the ticks, the
// largest |d| and its first tick, the mean of d * d, the largest |e_yaw|, s at the first and the last tick; written by lane 0 at
// the slot of the episode's first tick when the episode ends (the last record closes the running one, as in conflicts.inc).

struct TrackP {
    int B, n_ticks;
    const double *rec;        // [n][B][JSIM_REC_FIELDS]
    const int *flags;         // [n][B]
    const int *path_id;       // [B]
    int n_pts, n_paths;
    const double *px, *py, *pyaw, *arc; // [n_pts]
    const long long *path_off; // [n_paths + 1]
    int *idx, *seg;           // [n][B]
    double *s, *d, *e_yaw;    // [n][B]
    int *ep_i;                // [n][B][JSIM_TRK_NI], at an episode's first slot
    double *ep_d;             // [n][B][JSIM_TRK_ND]
};

// One candidate segment A -> B against the pose (x, y): the clamped parameter of the foot and the squared residual
struct TrackFoot { double t, q, ux, uy; };
__device__ __forceinline__ TrackFoot jtk_foot(double ax, double ay, double bx, double by, double x, double y)
{
    TrackFoot F;
    F.ux = bx - ax; F.uy = by - ay;
    const double L2 = F.ux * F.ux + F.uy * F.uy;
    double t = 0.0;
    if (L2 != 0.0) {
        t = ((x - ax) * F.ux + (y - ay) * F.uy) / L2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double rx = x - (ax + t * F.ux), ry = y - (ay + t * F.uy);
    F.t = t; F.q = rx * rx + ry * ry;
    return F;
}

// The kernel's body.  `px`, `py` (= P.px, P.py) are restrict-qualified: a search step's address is the same in every lane, and with
// the stores of this body known not to alias the table its loads are scalar loads, the points wave-uniform operands.
__device__ __forceinline__ void jtk_ticks(const TrackP &P, const double *__restrict__ px, const double *__restrict__ py)
{
    const int lane = threadIdx.x, b = blockIdx.x, B = P.B, n = P.n_ticks;
    const RecorderBuf R = {B, n, P.rec, P.flags, nullptr, nullptr};
    // the ego's path, clamped to the table: [lo, lo + np)
    const int p = P.path_id[b];
    long long lo64 = 0, hi64 = 0;
    if (p >= 0 && p < P.n_paths) { lo64 = P.path_off[p]; hi64 = P.path_off[p + 1]; }
    lo64 = lo64 < 0 ? 0 : (lo64 > P.n_pts ? P.n_pts : lo64);
    hi64 = hi64 < lo64 ? lo64 : (hi64 > P.n_pts ? P.n_pts : hi64);
    const int lo = (int)lo64, np = (int)(hi64 - lo64);

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
            // calc_nearest_index(state, cx, cy, 0): ascending, replaced on strict <
            const double *qx = px + lo, *qy = py + lo;
            int best_i = 0;
            double best;
            {
                const double dx = qx[0] - x, dy = qy[0] - y;
                best = dx * dx + dy * dy;
            }
            int i = 1;
            for (; i + 4 <= np; i += 4) {
                double d2[4];
                for (int j = 0; j < 4; ++j) {
                    const double dx = qx[i + j] - x, dy = qy[i + j] - y;
                    d2[j] = dx * dx + dy * dy;
                }
                for (int j = 0; j < 4; ++j)
                    if (d2[j] < best) { best = d2[j]; best_i = i + j; }
            }
            for (; i < np; ++i) {
                const double dx = qx[i] - x, dy = qy[i] - y;
                const double d2 = dx * dx + dy * dy;
                if (d2 < best) { best = d2; best_i = i; }
            }
            if (ok) {
                idx = best_i;
                // this lane's own points: idx - 1, idx, idx + 1, clamped to the path
                const int ia = lo + (idx > 0 ? idx - 1 : 0), ib = lo + idx, ic = lo + (idx + 1 < np ? idx + 1 : np - 1);
                const double bx = px[ib], by = py[ib];
                double t = 0.0, q, cross = 0.0;
                int other = ib;                               // the segment's far point, as a table index
                seg = 0;
                {
                    const double rx = x - bx, ry = y - by;
                    q = rx * rx + ry * ry;                    // n = 1: the point itself
                }
                const bool has_a = idx >= 1, has_b = idx + 1 < np;   // segments idx - 1 and idx within [0, n - 2]
                TrackFoot Fa = {}, Fb = {};
                if (has_a) Fa = jtk_foot(px[ia], py[ia], bx, by, x, y);
                if (has_b) Fb = jtk_foot(bx, by, px[ic], py[ic], x, y);
                if (has_a && (!has_b || !(Fb.q < Fa.q))) {    // the lower segment on a tie
                    seg = idx - 1; t = Fa.t; q = Fa.q; other = ib;
                    cross = Fa.ux * (y - py[ia]) - Fa.uy * (x - px[ia]);
                } else if (has_b) {
                    seg = idx; t = Fb.t; q = Fb.q; other = ic;
                    cross = Fb.ux * (y - by) - Fb.uy * (x - bx);
                }
                const int first = lo + seg;
                const double a0 = P.arc[first], y0 = P.pyaw[first];
                s = np > 1 ? a0 + t * (P.arc[other] - a0) : 0.0;
                const double root = sqrt(q);
                d = cross >= 0.0 ? root : -root;
                const double ref = np > 1 ? y0 + t * (P.pyaw[other] - y0) : y0;
                e_yaw = jpl_pymod((yaw - ref) + 3.141592653589793, 6.283185307179586) - 3.141592653589793;
            }
        }

        if (valid) {
            const size_t q = (size_t)k * B + b;
            P.idx[q] = idx; P.seg[q] = seg; P.s[q] = s; P.d[q] = d; P.e_yaw[q] = e_yaw;
            if (!((C.s_cur >> lane) & 1ull)) {                // not an episode's first tick: no episode outputs
                for (int j = 0; j < JSIM_TRK_NI; ++j) P.ep_i[JSIM_TRK_NI * q + j] = -1;
                for (int j = 0; j < JSIM_TRK_ND; ++j) P.ep_d[JSIM_TRK_ND * q + j] = NAN;
            }
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
    jtk_ticks(P, P.px, P.py);
}
