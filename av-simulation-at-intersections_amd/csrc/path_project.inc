// A point projected onto a path of a call's own path table, stated once for tracking_ticks_kernel and headway_ticks_kernel (DESIGN.md
// section 24 is the contract): idx = calc_nearest_index(state, cx, cy, 0) of main/lib/trajectories.py:89-97, the segment beside it
// that holds the foot of the perpendicular, the arc length s of the foot, the signed lateral offset d (left of the direction of
// travel is positive) and the path's yaw at the foot.
//
// The search: the path point of step i has the same address in every lane, so the points are scalar loads, four to a step, and
// wave-uniform operands of every query's distance; each query keeps its own smallest squared distance and replaces it on strict < in
// ascending order (np.argmin's first occurrence).  After it each lane gathers the at most three points around its own idx with
// vector loads through the kernel body's restrict-qualified px / py.

struct PathTableP {
    const int *path_id;       // [B]
    int n_pts, n_paths;
    const double *px, *py, *pyaw, *arc; // [n_pts]
    const long long *path_off; // [n_paths + 1]
};

// Ego b's path, clamped to the table: [lo, lo + np)
struct PathRange { int lo, np; };
__device__ __forceinline__ PathRange jpp_path(const PathTableP &T, int b)
{
    const int p = T.path_id[b];
    long long lo64 = 0, hi64 = 0;
    if (p >= 0 && p < T.n_paths) { lo64 = T.path_off[p]; hi64 = T.path_off[p + 1]; }
    lo64 = lo64 < 0 ? 0 : (lo64 > T.n_pts ? T.n_pts : lo64);
    hi64 = hi64 < lo64 ? lo64 : (hi64 > T.n_pts ? T.n_pts : hi64);
    return PathRange{(int)lo64, (int)(hi64 - lo64)};
}

// Q queries against the np >= 1 points of one path: a loaded point serves every query.  The table is read through the constant
// address space: nothing writes it while a kernel runs and its addresses are the wavefront's.  headway_ticks_kernel has more stores
// (three a place) than the compiler's search for a clobbering store follows, and through the restrict-qualified pointers alone its
// loads come out as vector loads of one address in every lane; tracking_ticks_kernel's are scalar loads either way.
typedef const __attribute__((address_space(4))) double *jpp_table;
template <int Q>
__device__ __forceinline__ void jpp_search(const double *__restrict__ px, const double *__restrict__ py, int np, const double (&x)[Q],
                                           const double (&y)[Q], int (&best_i)[Q])
{
    const jpp_table qx = (jpp_table)px, qy = (jpp_table)py;
    double best[Q];
    {
        const double ax = qx[0], ay = qy[0];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const double dx = ax - x[j], dy = ay - y[j];
            best[j] = dx * dx + dy * dy;
            best_i[j] = 0;
        }
    }
    int i = 1;
    for (; i + 4 <= np; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double ax = qx[i + u], ay = qy[i + u];
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const double dx = ax - x[j], dy = ay - y[j];
                const double d2 = dx * dx + dy * dy;
                if (d2 < best[j]) { best[j] = d2; best_i[j] = i + u; }
            }
        }
    }
    for (; i < np; ++i) {
        const double ax = qx[i], ay = qy[i];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const double dx = ax - x[j], dy = ay - y[j];
            const double d2 = dx * dx + dy * dy;
            if (d2 < best[j]) { best[j] = d2; best_i[j] = i; }
        }
    }
}

// One candidate segment A -> B against the point (x, y): the clamped parameter of the foot and the squared residual
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

// The point (x, y) on the path [lo, lo + np) from its nearest index idx: of the segments idx - 1 and idx (within [0, np - 2]) the
// one with the smaller residual, the foot clamped -- and from it the segment, the arc length, the signed offset and the path's yaw
// at the foot.  This lane's own points are idx - 1, idx, idx + 1, clamped to the path.
struct PathProj { int seg; double s, d, ref; };
__device__ __forceinline__ PathProj jpp_project(const PathTableP &T, const double *__restrict__ px, const double *__restrict__ py, int lo,
                                                int np, int idx, double x, double y)
{
    const int ia = lo + (idx > 0 ? idx - 1 : 0), ib = lo + idx, ic = lo + (idx + 1 < np ? idx + 1 : np - 1);
    const double bx = px[ib], by = py[ib];
    double t = 0.0, q, cross = 0.0;
    int other = ib, seg = 0;                                  // other: the segment's far point, as a table index
    {
        const double rx = x - bx, ry = y - by;
        q = rx * rx + ry * ry;                                // np = 1: the point itself
    }
    const bool has_a = idx >= 1, has_b = idx + 1 < np;
    TrackFoot Fa = {}, Fb = {};
    if (has_a) Fa = jtk_foot(px[ia], py[ia], bx, by, x, y);
    if (has_b) Fb = jtk_foot(bx, by, px[ic], py[ic], x, y);
    if (has_a && (!has_b || !(Fb.q < Fa.q))) {                // the lower segment on a tie
        seg = idx - 1; t = Fa.t; q = Fa.q; other = ib;
        cross = Fa.ux * (y - py[ia]) - Fa.uy * (x - px[ia]);
    } else if (has_b) {
        seg = idx; t = Fb.t; q = Fb.q; other = ic;
        cross = Fb.ux * (y - by) - Fb.uy * (x - bx);
    }
    const int first = lo + seg;
    const double a0 = T.arc[first], y0 = T.pyaw[first];
    const double root = sqrt(q);
    PathProj R;
    R.seg = seg;
    R.s = np > 1 ? a0 + t * (T.arc[other] - a0) : 0.0;
    R.d = cross >= 0.0 ? root : -root;
    R.ref = np > 1 ? y0 + t * (T.pyaw[other] - y0) : y0;
    return R;
}
