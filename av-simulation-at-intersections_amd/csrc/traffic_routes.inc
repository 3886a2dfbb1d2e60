// Route vehicles (kind 3 of the scripted obstacle tables; DESIGN.md section 32): a vehicle that follows a polyline of the route
// table (jsim_loop_set_traffic_routes) at a scripted speed.  The rule is stated once, in include/jsim_mpc.h above
// jsim_loop_set_traffic_routes; the numbers in the comments below are its items.  The table is one double4 per point, (x, y, yaw,
// S) with S the arc length from the route's first point, so a segment's two ends are two 32-byte loads.

// The table from the uploaded coordinates: one thread per route sums S in index order (a cold path that runs once per table)
#ifndef JSIM_KERNEL_TU /* (a kernel translation unit of the split build holds the register kernels only) */
__global__ __launch_bounds__(64) void route_arclen_kernel(int n_routes, const int *off, const double *x, const double *y,
                                                          const double *yaw, double4 *pt)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_routes) return;
    const int b = off[r], e = off[r + 1];
    double S = 0.0;
    for (int j = b; j < e; ++j) {
        if (j > b) {
            const double dx = x[j] - x[j - 1], dy = y[j] - y[j - 1];
            S = S + __dsqrt_rn(dx * dx + dy * dy); // (correctly rounded: S is the host's sum to the bit)
        }
        pt[j] = double4{x[j], y[j], yaw[j], S};
    }
}
#endif

// Item 5's j: the largest index with S[j] <= s and j <= n - 2 (n >= 2).  From a hint that is still behind s -- the segment of the
// vehicle's previous pose: s never decreases between two wraps -- the walk forward ends at that very index, S being
// non-decreasing; without one (hint < 0, or s has wrapped back behind it) the index is bisected.
__device__ __forceinline__ int route_segment(const double4 *p, int n, double s, int hint)
{
    if (hint >= 0 && hint <= n - 2 && p[hint].w <= s) {
        int j = hint;
        while (j + 1 <= n - 2 && p[j + 1].w <= s) ++j;
        return j;
    }
    int lo = 0, hi = n - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p[mid].w <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The pose at counter cnt of the vehicle with param row pr and wheelbase L; hint: route_segment's, updated
__device__ __forceinline__ void route_pose(const double4 *pt, const int *off, int n_routes, const double *pr, double L, double cnt,
                                           int &hint, double &x, double &y, double &yaw, double &v, double &steer)
{
    int r = (int)pr[0];
    r = r < 0 ? 0 : (r > n_routes - 1 ? n_routes - 1 : r);                  // 8
    const int b = off[r], n = off[r + 1] - b;
    const double4 *p = pt + b;
    const int end = (int)pr[1], per = (int)pr[7];
    const double speed = pr[2], offs = pr[3], s0 = pr[4], dt = pr[5];
    int c = (int)cnt;
    if (per >= 1) c %= per;                                                 // 1
    const int n0 = offs > 0.0 ? (int)floor(offs / dt) + 1 : 0;              // 2
    const int m = c - n0 > 0 ? c - n0 : 0;                                  // 3
    const double s = s0 + (double)m * (speed * dt);                         // 4
    v = 0.0; steer = 0.0;
    if (n < 2) {                                                            // 7
        x = n == 1 ? p[0].x : 0.0; y = n == 1 ? p[0].y : 0.0; yaw = n == 1 ? p[0].z : 0.0;
        return;
    }
    const double4 last = p[n - 1];
    if (s < last.w) {                                                       // 5
        int j = route_segment(p, n, s, hint);
        hint = j;
        if (j + 1 <= n - 2 && p[j + 1].w - s <= 1e-9) ++j;
        const double4 a = p[j], q = p[j + 1];
        const double ds = q.w - a.w;
        const double f = ds > 0.0 ? (s - a.w) / ds : 0.0;
        x = a.x + f * (q.x - a.x); y = a.y + f * (q.y - a.y); yaw = a.z + f * (q.z - a.z);
        if (c >= n0) v = speed;
        if (ds > 0.0) steer = atan((L * (q.z - a.z)) / ds);
    } else if (end == 1) {                                                  // 6
        x = last.x; y = last.y; yaw = last.z;
    } else {
        x = (double)JSIM_ROUTE_PARK; y = (double)JSIM_ROUTE_PARK; yaw = 0.0;
    }
}
