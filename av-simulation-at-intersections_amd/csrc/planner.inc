// planner.inc -- the route planner (SURVEY.md 8 row f4): A* over motion primitives, one wavefront per route query.
// (included by jsim_mpc.hip)
//
// Replaces, for a BATCH of queries at once (the reference plans one route per script run, 20-430 ms of Python each):
//   main/lib/mp_search_ww_generic.py:136-140  MotionPrimitiveSearch.run      :202-243  neighbor_function (collision test of every
//   primitive against every obstacle's half-planes, edge cost)              :166-190  distance_to_goal (heuristic)
//   :150-155 is_goal      :245-257 path_to_full_trajectory
//   main/lib/a_star.py:31-78  AStar.run: heap of (g + h, g, node, predecessor), dict of best predecessors keyed by the exact node
//   main/lib/obstacles.py:157-176 check_collision ; main/lib/linalg.py:4-57 ; main/lib/maths.py:4-10
// and, per route (weights wh / wc and a cost form from tables, one row per route: a weight sweep or the candidate set of the
// multi-trajectory planner is ONE launch), the cost terms of main/planner/multi_trajectory_planner.py:112-201 (JPL_FORM_MULTI):
//   :185-201 distance_to_goal = e hypot + p |wrapped heading difference| + o steering proxy ; :137-141 the edge's obstacle term
//   guarded by wc_obstacle, 1 / d for d > 0
//
// Most searches are small (13-208 expansions, open list <= 565 entries on the 18 reference routes), a few lane-changing routes of
// the two-lane scenario are not (up to 23k expansions, 62k open entries -- 48 s of the reference's Python).  The open list is a
// 64-ary heap keyed like the reference's tuples (g + h, then g, then the node's x, y, theta: a strict total order, so the pop
// sequence does not depend on the heap's shape): its levels 0-2 (4161 entries) sit in LDS, the rest in the route's global
// workspace, and the WAVE makes its moves -- a sink reads the 64 children of a slot one per lane and takes their minimum by DPP
// (three levels hold 266k entries); an A* successor's key is close to the current minimum, so the hole the pop leaves at the root
// is filled with the SMALLEST successor of the expansion, which sinks a level or two (only a dead end or a stale entry moves the
// last entry to the root), and the other successors are appended by their own lanes, which look at their parents themselves:
// few ever climb.  Node records and the best-predecessor dict (an open-addressing table over the exact bits of (x, y, theta))
// live in that workspace too, sized by the caller (node_cap).  One expansion is 9 primitives x ~10 collision points x the
// obstacles in reach x 4-8 half-planes, and the lanes share it: lane = (primitive, collision point); lane k prices neighbour k
// (pose, edge cost, heuristic, dict look-up).  Memory: one wavefront sees its own writes in program order, so the search loop has
// no barrier and no wait; everything an expansion stores (records, entries beyond LDS, the dict entry) leaves at its END, behind
// the loads the next pop needs -- gfx9 counts loads and stores in one counter, and a wait for a load right after a store costs the
// store's round trip.  The trajectory of the found path is written by all lanes.
// Expression order follows the Python source term by term (left-to-right sums, Python's float %), every product an explicit
// operation (the file is compiled -ffp-contract=off).

#define JPL_HEAP_CAP 4161   /* open-list entries held in LDS: levels 0-2 of the 64-ary heap (1 + 64 + 4096) */
#define JPL_MAX_PRIM 16
#define JPL_MAX_CC 16     /* collision points per primitive */
#define JPL_MAX_HP 512    /* half-planes of one query's obstacle set */
#define JPL_MAX_OBS 64
#define JPL_D 64          /* arity of the open list's heap: one child per lane */
#define JPL_FORM_GENERIC 0   /* main/lib/mp_search_ww_generic.py: heuristic :166-190, edge cost :202-243 */
#define JPL_FORM_MULTI 1     /* main/planner/multi_trajectory_planner.py: heuristic :185-201, edge cost :112-153 */
#define JPL_PASSES ((JPL_MAX_PRIM * JPL_MAX_CC + 63) / 64)   /* (primitive, collision point) pairs per lane */
// One wavefront per route: what one lane writes -- to LDS or to memory -- the others see in program order, with no wait and no barrier
// instruction (LLVM's AMDGPU memory model: a wavefront-scope fence needs no code on gfx942 / gfx950); the fence keeps the COMPILER
// from moving memory operations across it.  (__syncthreads() here waited for every store in flight: vmcnt counts stores on gfx9.)
#define JPL_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

struct PlanP {
    int n_routes, n_prim, n_pts, max_path, node_cap;
    const double *wh, *wc;                         // [R][5] (dist, theta, steering, obstacle, center), [R][4] (dist, steering, obstacle, center)
    const int *form;                               // [R] 0: mp_search_ww_generic.py, 1: multi_trajectory_planner.py (JPL_FORM_*)
    const double *start, *goal, *goal_box, *tol;   // [R][3], [R][3], [R][4] (x1, y1, x2, y2), [R]
    const double *hp;                              // [.][3] half-planes a x + b y + c <= 0 (inside)
    const int *hp_off;                             // per obstacle: [first, last) into hp
    const int *route_obs_off;                      // [R + 1] per route: [first, last) obstacle
    const double *obc;                             // [.][3] per obstacle: a circle (x, y, r) that contains it; r = inf: none known (unbounded)
    const double *mp_pts;                          // [P][n_pts][3]
    const double *mp_len;                          // [P]
    const double *cc_pts;                          // [.][2] collision points (xy, primitive frame)
    const int *cc_off;                             // [P + 1]
    // per-route node records (global workspace) and outputs
    double *nx, *ny, *nth, *ng;                    // [R][node_cap]
    int *nparent, *nprim;                          // [R][node_cap]
    int *htab; int hash_cap;                       // [R][hash_cap] (a power of two >= 2 node_cap): the dict, node id per slot or -1
    double *ov_gh, *ov_g; int *ov_id;              // [R][node_cap] the open list beyond its first JPL_HEAP_CAP entries (those sit in LDS)
    int *status, *n_prims, *prims, *n_expanded;    // [R], [R], [R][max_path], [R]
    double *cost, *nodes, *traj;                   // [R], [R][max_path + 1][3], [R][max_path * (n_pts - 1)][3]
};

#include "pymod.inc" // jpl_pymod
__device__ __forceinline__ double jpl_normalize_angle(double th) // main/lib/maths.py:4-10
{
    th = jpl_pymod(th, 6.283185307179586);
    if (th >= 3.141592653589793) th -= 6.283185307179586;
    return th;
}
__device__ __forceinline__ double jpl_steer_change(double th_a, double th_b) // mp_search_ww_generic.py:60-82
{
    double d = th_b - th_a;
    d = jpl_pymod(d + 3.141592653589793, 2 * 3.141592653589793) - 3.141592653589793;
    return fabs(d) * 1.0;
}
__device__ __forceinline__ unsigned jpl_hash(double x, double y, double th, unsigned mask)
{
    unsigned long long h = (unsigned long long)__double_as_longlong(x) * 0x9E3779B97F4A7C15ull;
    h ^= ((unsigned long long)__double_as_longlong(y) + 0x7F4A7C159E3779B9ull) * 0xC2B2AE3D27D4EB4Full;
    h ^= ((unsigned long long)__double_as_longlong(th) + 0x165667B19E3779F9ull) * 0x27D4EB2F165667C5ull;
    h ^= h >> 29;
    return (unsigned)h & mask;
}

#ifdef JPL_STAMPS /* development builds: the wave's clock per phase of the search loop, summed per route; jsim_plan_routes prints them
   per expansion for routes above 1000 expansions.  Times: [0] pop + dict check, [6] cos / sin, neighbour poses + first dict probe, obstacles
   in reach, [1] collision test, [2] neighbours, [3] new poses to LDS, [5] smallest successor + its sink from the root, [10] appends,
   [18] [16] [19] [22] [23] [25] the climbs, [26] the refill after a dead end, [4] the expansion's stores + the next root, [15] refill after
   a stale pop.  Counts: [8] sink levels, [9] climb steps, [20] climb iterations, [17] expansions with a climber, [11] obstacles in reach,
   [12] stale pops, [21] ties decided by the poses */
__device__ long long jpl_clk[64][32];
#define JPL_T(k) do { const long long t_ = __builtin_readcyclecounter(); jpl_acc[k] += t_ - jpl_t0; jpl_t0 = t_; } while (0)
#define JPL_CNT(k) do { ++jpl_acc[k]; } while (0)
#else
#define JPL_T(k) do { } while (0)
#define JPL_CNT(k) do { } while (0)
#endif

__global__ __launch_bounds__(64) void plan_astar_kernel(const PlanP P)
{
    __shared__ double hk_gh[JPL_HEAP_CAP], hk_g[JPL_HEAP_CAP];
    __shared__ int hk_id[JPL_HEAP_CAP];
    __shared__ double hpl[JPL_MAX_HP * 3];
    __shared__ int hpo[JPL_MAX_OBS + 1];
    __shared__ double obl[JPL_MAX_OBS * 3];
    __shared__ double ccl[JPL_MAX_PRIM * JPL_MAX_CC * 2];
    __shared__ int cco[JPL_MAX_PRIM + 1];
    __shared__ double nw_x[JPL_MAX_PRIM], nw_y[JPL_MAX_PRIM], nw_th[JPL_MAX_PRIM];   // poses of the expansion's new nodes, by rank
    __shared__ int nb_ok[JPL_MAX_PRIM];
    __shared__ int sh_i[8];
    __shared__ double sh_d[8];

    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= P.n_routes) return;
    const int NP = P.n_prim, cap = P.node_cap;
    double *nx = P.nx + (size_t)r * cap, *ny = P.ny + (size_t)r * cap, *nth = P.nth + (size_t)r * cap, *ng = P.ng + (size_t)r * cap;
    int *npar = P.nparent + (size_t)r * cap, *nprm = P.nprim + (size_t)r * cap;
    const double gx = P.goal[3 * r], gy = P.goal[3 * r + 1], gth = P.goal[3 * r + 2];
    const double bx1 = P.goal_box[4 * r], by1 = P.goal_box[4 * r + 1], bx2 = P.goal_box[4 * r + 2], by2 = P.goal_box[4 * r + 3];
    const double tol = P.tol[r];
    // The route's own weights and cost form (jsim_plan_routes_weighted): one row per route, the same for all its lanes -- read once,
    // here, and marked uniform: scalar registers throughout the search, and the form a scalar branch (one side's code is run)
    const double wh_dist = uni(P.wh[5 * r]), wh_theta = uni(P.wh[5 * r + 1]), wh_steer = uni(P.wh[5 * r + 2]), wh_obst = uni(P.wh[5 * r + 3]);
    const double wh_center = uni(P.wh[5 * r + 4]);
    const double wc_dist = uni(P.wc[4 * r]), wc_steer = uni(P.wc[4 * r + 1]), wc_obst = uni(P.wc[4 * r + 2]), wc_center = uni(P.wc[4 * r + 3]);
    const bool multi = uni(P.form[r]) == JPL_FORM_MULTI;
    // the edge's obstacle term: guarded by the HEURISTIC's weight in the generic file (sic, mp_search_ww_generic.py:230), by the
    // edge's own in the multi-trajectory planner (multi_trajectory_planner.py:139)
    const bool edge_obst = multi ? wc_obst != 0.0 : wh_obst != 0.0;
    const int o0 = P.route_obs_off[r], o1 = P.route_obs_off[r + 1], n_obs = o1 - o0;
    const int h0 = P.hp_off[o0], n_hp = P.hp_off[o1] - h0;
    bool bad = n_obs > JPL_MAX_OBS || n_hp > JPL_MAX_HP || NP > JPL_MAX_PRIM;
    for (int k = 0; k < NP && !bad; ++k) bad = (P.cc_off[k + 1] - P.cc_off[k]) > JPL_MAX_CC;
    if (bad) { if (lane == 0) { P.status[r] = 5; P.n_prims[r] = 0; P.n_expanded[r] = 0; } return; }
    int *const htab = P.htab + (size_t)r * P.hash_cap;   // (filled with -1 by the host)
    const unsigned hmask = (unsigned)P.hash_cap - 1u;
    double *const ov_gh = P.ov_gh + (size_t)r * cap, *const ov_g = P.ov_g + (size_t)r * cap;
    int *const ov_id = P.ov_id + (size_t)r * cap;
    for (int e = lane; e < n_hp * 3; e += 64) hpl[e] = P.hp[(size_t)h0 * 3 + e];
    for (int e = lane; e <= n_obs; e += 64) hpo[e] = P.hp_off[o0 + e] - h0;
    for (int e = lane; e < n_obs * 3; e += 64) obl[e] = P.obc[(size_t)o0 * 3 + e];
    for (int k = lane; k <= NP; k += 64) cco[k] = P.cc_off[k] - P.cc_off[0];
    __syncthreads();
    for (int k = 0; k < NP; ++k)
        for (int e = lane; e < (cco[k + 1] - cco[k]) * 2; e += 64) ccl[(k * JPL_MAX_CC) * 2 + e] = P.cc_pts[(size_t)(P.cc_off[0] + cco[k]) * 2 + e];
    // which (primitive, collision point) pairs this lane tests: pair p = lane, lane + 64, ...
    int n_pairs = cco[NP];
    // Exact pruning of the collision test (round 3): every collision point of every primitive placed at a node lies within rmax of the
    // node's position (a rotation keeps |p|), and obstacle o lies inside the circle (x_o, y_o, r_o) the host derived from its
    // half-planes -- so an obstacle whose circle centre is further than rmax + r_o from the node cannot contain any of the points and
    // is left out of this expansion's walk (typically 2-6 of the 24 obstacles of an intersection are in reach of a 5 m primitive).
    __syncthreads();
    double rmax = 0.0;
    for (int k = 0; k < NP; ++k)
        for (int j = lane; j < cco[k + 1] - cco[k]; j += 64) {
            const double px = ccl[(k * JPL_MAX_CC + j) * 2], py = ccl[(k * JPL_MAX_CC + j) * 2 + 1];
            rmax = fmax(rmax, sqrt(px * px + py * py));
        }
    for (int o = 32; o >= 1; o >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, o));
    rmax = rmax * (1.0 + 1e-9) + 1e-9;
    // this lane's (primitive, collision point) pairs -- pair p = lane, lane + 64, ... -- do not change from expansion to expansion
    int pk[JPL_PASSES];
    double ppx[JPL_PASSES], ppy[JPL_PASSES];
#pragma unroll
    for (int q = 0; q < JPL_PASSES; ++q) {
        const int p = lane + 64 * q;
        pk[q] = -1; ppx[q] = 0.0; ppy[q] = 0.0;
        if (p < n_pairs) {
            int k = 0;
            while (p >= cco[k + 1]) ++k;
            pk[q] = k; ppx[q] = ccl[(k * JPL_MAX_CC + p - cco[k]) * 2]; ppy[q] = ccl[(k * JPL_MAX_CC + p - cco[k]) * 2 + 1];
        }
    }
#ifdef JPL_STAMPS
    long long jpl_acc[32] = {0}, jpl_t0 = 0;
#endif
    // this lane's obstacle circle (lane o tests obstacle o: n_obs <= 64) and, for lane k < NP, primitive k's end pose and length
    const double ocx = lane < n_obs ? obl[3 * lane] : 0.0, ocy = lane < n_obs ? obl[3 * lane + 1] : 0.0, ocr = lane < n_obs ? obl[3 * lane + 2] : 0.0;
    const double *const lp_ = P.mp_pts + ((size_t)(lane < NP ? lane : 0) * P.n_pts + (P.n_pts - 1)) * 3;
    const double lpx = lp_[0], lpy = lp_[1], lpth = lp_[2], lplen = P.mp_len[lane < NP ? lane : 0];
    // heap of node ids ordered by (g + h, g, x, y, theta) -- the reference's tuple order (a_star.py:34)
    // (the nodes made by the expansion under way have their poses in LDS, by rank: their records are stored at its end)
    int n_heap = 0, n_nodes = 0, n_exp = 0, status = -1, goal_id = -1;   // n_heap counts the root even while it is vacant (after a pop)
    auto less_pose = [&](int ia, int ib) -> bool {
        JPL_CNT(21);
        const double xa = ia >= n_nodes ? nw_x[ia - n_nodes] : nx[ia], xb = ib >= n_nodes ? nw_x[ib - n_nodes] : nx[ib];
        if (xa != xb) return xa < xb;
        const double ya = ia >= n_nodes ? nw_y[ia - n_nodes] : ny[ia], yb = ib >= n_nodes ? nw_y[ib - n_nodes] : ny[ib];
        if (ya != yb) return ya < yb;
        const double ta = ia >= n_nodes ? nw_th[ia - n_nodes] : nth[ia], tb = ib >= n_nodes ? nw_th[ib - n_nodes] : nth[ib];
        return ta < tb;
    };
    auto less = [&](double gha, double ga, int ia, double ghb, double gb, int ib) -> bool {
        if (gha != ghb) return gha < ghb;
        if (ga != gb) return ga < gb;
        return less_pose(ia, ib);
    };
    // the same with uniform operands, the outcome marked uniform (a scalar branch: what the wave does next does not fall through
    // the other side's code and its wait states)
    auto less_u = [&](double gha, double ga, int ia, double ghb, double gb, int ib) -> bool {
        if (gha != ghb) return gha < ghb;
        if (ga != gb) return ga < gb;
        return uni((int)less_pose(ia, ib)) != 0;
    };
    // open-list entry i: LDS for i < JPL_HEAP_CAP, the route's global overflow arrays beyond
    // (one branch, three independent loads: as three separate selects every field paid its own memory round trip)
    // (the id pinned per branch: merged into one load through a generic pointer -- flat_load -- it made every look-up wait for all
    // memory operations in flight, the stores of the entries just appended among them)
    auto hget = [&](int i, double &a, double &b, int &c) {
        if (i < JPL_HEAP_CAP) { a = hk_gh[i]; b = hk_g[i]; c = hk_id[i]; asm volatile("" : "+v"(c)); }
        else { const int j = i - JPL_HEAP_CAP; a = ov_gh[j]; b = ov_g[j]; c = ov_id[j]; asm volatile("" : "+v"(c)); }
    };
    auto hset = [&](int i, double a, double b, int c) {
        if (i < JPL_HEAP_CAP) { hk_gh[i] = a; hk_g[i] = b; hk_id[i] = c; }
        else { ov_gh[i - JPL_HEAP_CAP] = a; ov_g[i - JPL_HEAP_CAP] = b; ov_id[i - JPL_HEAP_CAP] = c; }
    };
    // The heap's moves are made by the WAVE (round 3; lane 0 alone, one key after the other, spent 3k cycles per level of a binary or
    // 16-ary sink and 1.7k per push).  Called by all lanes, in uniform control flow, with uniform arguments.
    // wave_min: the smallest of the 64 lanes' entries (a, b, c) under the heap's order (c < 0: none, a = b = inf) -> uniform (a, b, c)
    // and the lane wl that held it.  The minimum of g + h by DPP; one lane holds it in all but a few cases (then: the smallest g
    // among those, then the poses, one candidate after the other).
    auto wave_min = [&](double &a, double &b, int &c, int &wl) {
        const double m = wmin_dpp(a);
        unsigned long long eq = __ballot(c >= 0 && a == m);
        if (__popcll(eq) > 1) {
            const double m2 = wmin_dpp(((eq >> lane) & 1ull) ? b : INFINITY);
            eq &= __ballot(b == m2);
            if (__popcll(eq) > 1) {
                int best = __builtin_ctzll(eq), bid = __builtin_amdgcn_readlane(c, best);
                for (unsigned long long m_ = eq & (eq - 1ull); m_ != 0ull; m_ &= m_ - 1ull) {
                    const int l_ = __builtin_ctzll(m_), cid = __builtin_amdgcn_readlane(c, l_);
                    if (uni((int)less_pose(cid, bid)) != 0) { best = l_; bid = cid; }
                }
                eq = 1ull << best;
            }
        }
        wl = eq != 0ull ? (int)__builtin_ctzll(eq) : 0;
        a = m; b = rdlane(b, wl); c = eq != 0ull ? __builtin_amdgcn_readlane(c, wl) : -1;
    };
    // sink: entry (kgh, kg, kid) placed at slot i of a heap of n entries, sinking while a child is smaller.  Lane e fetches child e of
    // the group -- from LDS (levels 1 and 2) or, beyond, all sixty-four in one memory round trip.
    auto sink = [&](int i, double kgh, double kg, int kid, int n) {
        i = uni(i); n = uni(n);
        for (;;) {
            const int c0 = JPL_D * i + 1;
            if (c0 >= n) break;
            const int ci = c0 + lane;
            double a = INFINITY, b = INFINITY; int c = -1;
            if (c0 + JPL_D <= JPL_HEAP_CAP) {            // the whole group in LDS (slots beyond n: read, not used)
                const double a_ = hk_gh[ci], b_ = hk_g[ci]; const int c_ = hk_id[ci];
                if (ci < n) { a = a_; b = b_; c = c_; }
            } else {                                     // the whole group in the overflow (index clamped to the last entry)
                const int j = (ci < n ? ci : n - 1) - JPL_HEAP_CAP;
                const double a_ = ov_gh[j], b_ = ov_g[j]; const int c_ = ov_id[j];
                if (ci < n) { a = a_; b = b_; c = c_; }
            }
            int wl;
            wave_min(a, b, c, wl);
            if (!less_u(a, b, c, kgh, kg, kid)) break;
            JPL_CNT(8);
            if (lane == 0) hset(i, a, b, c);
            i = uni(c0 + wl);
        }
        if (lane == 0) hset(i, kgh, kg, kid);
    };
    // entry i read by every lane (one address), the values marked uniform
    auto hget_u = [&](int i, double &a, double &b, int &c) {
        if (i < JPL_HEAP_CAP) { a = uni(hk_gh[i]); b = uni(hk_g[i]); c = uni(hk_id[i]); }
        else { const int j = i - JPL_HEAP_CAP; a = uni(ov_gh[j]); b = uni(ov_g[j]); c = uni(ov_id[j]); }
    };
    auto refill_from_last = [&](int n) {                           // the root is vacant, n entries counting it: the last one takes it
        if (n > 1) { double a, b_; int c_; hget_u(n - 1, a, b_, c_); sink(0, a, b_, c_, n - 1); }
    };
    if (lane == 0) { // q = [(0, 0, start, start)]
        nx[0] = P.start[3 * r]; ny[0] = P.start[3 * r + 1]; nth[0] = P.start[3 * r + 2]; ng[0] = 0.0; npar[0] = 0; nprm[0] = -1;
        hk_gh[0] = 0.0; hk_g[0] = 0.0; hk_id[0] = 0;
    }
    n_heap = 1; n_nodes = 1;
    __syncthreads();
    // The root's key and pose, asked for as soon as the root is settled -- at the end of an expansion, in FRONT of its stores -- and
    // used by the next pop: its memory round trip runs under the stores' (a node made by the expansion under way: from LDS).
    double rt_g = 0.0, rt_x = 0.0, rt_y = 0.0, rt_th = 0.0;
    int rt_id = 0;
    auto fetch_root = [&]() {
        if (n_heap == 0) return;
        rt_g = uni(hk_g[0]); rt_id = uni(hk_id[0]);
        if (rt_id >= n_nodes) { rt_x = nw_x[rt_id - n_nodes]; rt_y = nw_y[rt_id - n_nodes]; rt_th = nw_th[rt_id - n_nodes]; }
        else { rt_x = nx[rt_id]; rt_y = ny[rt_id]; rt_th = nth[rt_id]; }
    };
    fetch_root();
#ifdef JPL_STAMPS
    jpl_t0 = __builtin_readcyclecounter();
#endif

    while (status < 0) {
        // ---------------- pop: the root is read (it stays where it is until the pushes refill it), dict check, goal test -- by every
        // lane alike (one address per load), so that nothing has to be handed from lane to lane
        if (n_heap == 0) { status = 1; break; }      // raise Exception("No solution found.")
        const double g = rt_g, x = uni(rt_x), y = uni(rt_y), th = uni(rt_th);   // (fetched when the root was settled: fetch_root)
        const int cur = rt_id;
        unsigned s = jpl_hash(x, y, th, hmask);
        int found = -1;
        for (;;) {
            const int j = uni(htab[s]);
            if (j < 0) break;
            const double jx = uni(nx[j]), jy = uni(ny[j]), jth = uni(nth[j]);
            if (jx == x && jy == y && jth == th) { found = j; break; }
            s = (s + 1) & hmask;
        }
        if (found >= 0 && g >= uni(ng[found])) {     // `if node in pred_dict and g >= pred_dict[node][0]: continue`
            JPL_T(0);
            refill_from_last(n_heap); --n_heap; JPL_WSYNC(); JPL_CNT(12); JPL_T(15);
            fetch_root();
            continue;
        }
        // pred_dict[node] = g, predecessor: slot s takes cur -- with the other stores of this expansion, at its end: on gfx9 a wait
        // for ANY load also waits for every store in flight (one counter), a microsecond each time stores had just been issued; the
        // stores now leave together, right in front of the next pop's loads, whose round trips the wait would cost anyway
        JPL_T(0);                                    // pop, dict check, goal test
        {
            const double dx = fmax(fmax(bx1 - x, 0.0), x - bx2), dy = fmax(fmax(by1 - y, 0.0), y - by2);
            if (sqrt(dx * dx + dy * dy) <= 1e-5 && fabs(th - gth) <= tol) { if (lane == 0) htab[s] = cur; ++n_exp; status = 0; goal_id = cur; break; }
        }
        ++n_exp;
        double cs, sn;
        sincos(th, &sn, &cs);
        const bool rot_only = (x == 0.0 && y == 0.0);     // create_2d_transform_mtx: a 2x2 rotation when there is nothing to translate
        // neighbour k's pose by lane k and the first probe of its dict look-up, asked for here: the round trip runs under the collision test
        double ex = 0.0, ey = 0.0, eth = 0.0;
        unsigned s2 = 0u;
        int j0 = -1;
        if (lane < NP) {
            ex = lpx * cs + lpy * (-sn); ey = lpx * sn + lpy * cs;
            if (!rot_only) { ex = ex + x; ey = ey + y; }
            eth = jpl_normalize_angle(lpth + th);
            s2 = jpl_hash(ex, ey, eth, hmask);
            j0 = htab[s2];
        }
        // ---------------- collision test of every primitive: lane = (primitive, collision point)
        if (lane < JPL_MAX_PRIM) nb_ok[lane] = 1;
        // obstacles in reach of this node
        const unsigned long long nearm = __ballot(lane < n_obs && !(sqrt((ocx - x) * (ocx - x) + (ocy - y) * (ocy - y)) > rmax + ocr));
        JPL_WSYNC();
        JPL_T(6);                                    // cos / sin, obstacles in reach
#ifdef JPL_STAMPS
        jpl_acc[11] += __popcll(nearm);
#endif
        // all lanes walk the same obstacles and half-planes (both uniform), each with its pairs: four half-planes per step, their twelve
        // coefficients in one batch of broadcast reads shared by the lane's pairs, no branch on a lane's own outcome (the walk with an
        // early exit per lane paid a dependent LDS round trip per half-plane and lasted as long as its slowest lane anyway)
        double wx[JPL_PASSES], wy[JPL_PASSES];
        bool hit[JPL_PASSES];
#pragma unroll
        for (int q = 0; q < JPL_PASSES; ++q) {
            wx[q] = ppx[q] * cs + ppy[q] * (-sn); wy[q] = ppx[q] * sn + ppy[q] * cs;
            if (!rot_only) { wx[q] = wx[q] + x; wy[q] = wy[q] + y; }
            hit[q] = false;
        }
        double jx = 0.0, jy = 0.0, jth = 0.0, jg = 0.0;          // the node that probe found (any): its pose and g, asked for as well
        if (lane < NP && j0 >= 0) { jx = nx[j0]; jy = ny[j0]; jth = nth[j0]; jg = ng[j0]; }
        // four obstacles per step: their offsets in one batch of reads, then the first four half-planes of each (48 coefficients) in
        // another -- two LDS round trips for up to four obstacles (one obstacle per step: two round trips each, 1.25k cycles)
        for (unsigned long long om_ = nearm; om_ != 0ull;) {
            int o_[4], nthis = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (om_ != 0ull) { o_[k] = __builtin_ctzll(om_); om_ &= om_ - 1ull; nthis = k + 1; }
                else o_[k] = o_[k > 0 ? k - 1 : 0];
            }
            int e0_[4], e1_[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { e0_[k] = hpo[o_[k]]; e1_[k] = hpo[o_[k] + 1]; }
            double cf[4][12];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 3 * (e0_[k] + j < e1_[k] ? e0_[k] + j : e0_[k]);   // (fewer than four: the first again; none: not used)
                    cf[k][3 * j] = hpl[e]; cf[k][3 * j + 1] = hpl[e + 1]; cf[k][3 * j + 2] = hpl[e + 2];
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= nthis) break;
                bool inside[JPL_PASSES];
#pragma unroll
                for (int q = 0; q < JPL_PASSES; ++q) {
                    inside[q] = true;
                    if (64 * q >= n_pairs || e1_[k] <= e0_[k]) continue;
                    const double v0 = (cf[k][0] * wx[q] + cf[k][1] * wy[q]) + cf[k][2], v1 = (cf[k][3] * wx[q] + cf[k][4] * wy[q]) + cf[k][5];
                    const double v2 = (cf[k][6] * wx[q] + cf[k][7] * wy[q]) + cf[k][8], v3 = (cf[k][9] * wx[q] + cf[k][10] * wy[q]) + cf[k][11];
                    inside[q] = (v0 <= 0.0) & (v1 <= 0.0) & (v2 <= 0.0) & (v3 <= 0.0);
                }
                for (int e = e0_[k] + 4; e < e1_[k]; e += 4) {                       // obstacles with more than four half-planes
                    const int ea = 3 * e, eb = 3 * (e + 1 < e1_[k] ? e + 1 : e), ec = 3 * (e + 2 < e1_[k] ? e + 2 : e), ed = 3 * (e + 3 < e1_[k] ? e + 3 : e);
                    const double a0 = hpl[ea], b0 = hpl[ea + 1], c0 = hpl[ea + 2], a1 = hpl[eb], b1 = hpl[eb + 1], c1 = hpl[eb + 2];
                    const double a2 = hpl[ec], b2 = hpl[ec + 1], c2 = hpl[ec + 2], a3 = hpl[ed], b3 = hpl[ed + 1], c3 = hpl[ed + 2];
#pragma unroll
                    for (int q = 0; q < JPL_PASSES; ++q) {
                        if (64 * q >= n_pairs) break;
                        const double v0 = (a0 * wx[q] + b0 * wy[q]) + c0, v1 = (a1 * wx[q] + b1 * wy[q]) + c1;
                        const double v2 = (a2 * wx[q] + b2 * wy[q]) + c2, v3 = (a3 * wx[q] + b3 * wy[q]) + c3;
                        inside[q] = inside[q] & (v0 <= 0.0) & (v1 <= 0.0) & (v2 <= 0.0) & (v3 <= 0.0);
                    }
                }
#pragma unroll
                for (int q = 0; q < JPL_PASSES; ++q) hit[q] = hit[q] | inside[q];
            }
        }
#pragma unroll
        for (int q = 0; q < JPL_PASSES; ++q)
            if (64 * q < n_pairs && hit[q] && pk[q] >= 0) nb_ok[pk[q]] = 0; // (benign race: every writer stores 0)
        JPL_WSYNC();
        JPL_T(1);                                    // collision test
        // ---------------- neighbour k by lane k: pose, edge cost, heuristic, dict look-up
        double my_gh = INFINITY, my_g = INFINITY, my_x = 0.0, my_y = 0.0, my_th = 0.0;
        int ok = 0;
        if (lane < NP) {
            ok = nb_ok[lane];
            if (ok) {
                const double steer = jpl_steer_change(th, eth);
                double obst = 0.0, center = 0.0;
                if (edge_obst) {
                    double best = INFINITY;
                    for (int e = 0; e < n_hp; ++e) {
                        const double a = hpl[3 * e], b = hpl[3 * e + 1], c = hpl[3 * e + 2];
                        best = fmin(best, fabs(a * ex + b * ey + c) / sqrt(a * a + b * b));
                    }
                    if (multi) obst = best > 0.0 ? 1.0 / best : INFINITY;        // `1.0 / d if d > 0.0 else inf` (:141)
                    else obst = best != 0.0 ? 1.0 / best : INFINITY;
                }
                if (wc_center != 0.0) center = sqrt(ex * ex + ey * ey);
                const double edge = ((wc_dist * lplen + wc_steer * steer) + wc_obst * obst) + wc_center * center;
                const double ngk = g + edge;
                // `if neighbor not in pred_dict or neighbor_g < pred_dict[neighbor][0]`
                if (j0 >= 0) {
                    if (jx == ex && jy == ey && jth == eth) { if (!(ngk < jg)) ok = 0; }
                    else {                                          // another pose in that slot: on along the chain
                        s2 = (s2 + 1) & hmask;
                        while (htab[s2] >= 0) {
                            const int j = htab[s2];
                            if (nx[j] == ex && ny[j] == ey && nth[j] == eth) { if (!(ngk < ng[j])) ok = 0; break; }
                            s2 = (s2 + 1) & hmask;
                        }
                    }
                }
                if (ex == x && ey == y && eth == th && !(ngk < g)) ok = 0;   // (the node itself: its dict entry is written at the end)
                if (ok) {
                    const double hs = jpl_steer_change(eth, gth);
                    double h;
                    if (multi) {    // e hypot(x - gx, y - gy) + p |((theta - gtheta) + pi) % 2 pi - pi| + o steering_change(node, goal) (:193-200)
                        const double dxy = hypot(ex - gx, ey - gy);
                        const double dth = fabs(jpl_pymod((eth - gth) + 3.141592653589793, 2 * 3.141592653589793) - 3.141592653589793);
                        h = (wh_dist * dxy + wh_theta * dth) + wh_steer * hs;
                    } else {
                        const double dxy = sqrt((ex - gx) * (ex - gx) + (ey - gy) * (ey - gy));
                        const double ad = fabs(eth - gth);
                        const double dth = fmin(ad, ad - tol / 2);
                        double hob = 0.0, hce = 0.0;
                        if (wh_obst != 0.0) hob = obst;
                        if (wh_center != 0.0) hce = sqrt(ex * ex + ey * ey);
                        h = (((wh_dist * dxy + wh_theta * dth) + wh_steer * hs) + wh_obst * hob) + wh_center * hce;
                    }
                    my_g = ngk; my_gh = ngk + h; my_x = ex; my_y = ey; my_th = eth;
                }
            }
        }
        JPL_T(2);                                    // neighbours
        // ---------------- pushes, ids in primitive order: every new node's own lane writes its record; the SMALLEST of them goes into
        // the root the pop left vacant (it sinks a level or two), the others are appended -- each by its own lane, which also looks
        // at its parent: an A* successor rarely has to climb (one step per expansion on the long searches), and only those that do
        // are walked up by lane 0.  Without a successor (a dead end) the last entry takes the root.
        // (round 2: lane 0 wrote nine records, moved the last entry to the root through 16 binary levels and walked every push up ~16)
        const unsigned long long okm = __ballot(ok != 0);
        const int cnt = __popcll(okm);
        if (n_nodes + cnt > cap || n_heap + cnt > JPL_HEAP_CAP + cap) { status = 4; break; }   // workspace exhausted
        const int my_id = ok ? n_nodes + __popcll(okm & ((1ull << lane) - 1ull)) : -1;
        if (ok) { nw_x[my_id - n_nodes] = my_x; nw_y[my_id - n_nodes] = my_y; nw_th[my_id - n_nodes] = my_th; }
        JPL_WSYNC();                        // (ties between keys are decided by the poses)
        JPL_T(3);                                    // records
        bool late = false;
        int pos = 0;
        if (cnt == 0) refill_from_last(n_heap);
        else {
            double a = my_gh, b = my_g; int c = my_id;             // (lanes without a successor: inf, inf, -1)
            int wl_;
            wave_min(a, b, c, wl_);
            sink(0, a, b, c, n_heap);
            JPL_T(5);
            JPL_WSYNC();
            const unsigned long long restm = okm & ~__ballot(ok && my_id == c);
            bool climbs = false;
            if (ok && my_id != c) {
                pos = n_heap + __popcll(restm & ((1ull << lane) - 1ull));
                if (pos < JPL_HEAP_CAP) { hk_gh[pos] = my_gh; hk_g[pos] = my_g; hk_id[pos] = my_id; }
                else late = true;                                  // (beyond the LDS part: stored at the end of the expansion)
                double pgh, pg; int pid_;
                const int pa = (pos - 1) / JPL_D;
                if (n_heap + cnt <= JPL_D * JPL_HEAP_CAP) { pgh = hk_gh[pa]; pg = hk_g[pa]; pid_ = hk_id[pa]; }   // (uniform: every parent in LDS)
                else hget(pa, pgh, pg, pid_);
                climbs = less(my_gh, my_g, my_id, pgh, pg, pid_);
            }
            const unsigned long long climbm = __ballot(climbs);
            JPL_T(10);
            if (climbm != 0ull) {
                JPL_CNT(17);
                JPL_WSYNC();
                JPL_T(18);
                // the few that climb, one after the other, the wave following: every lane reads the parent (one address), lane 0 writes
                for (unsigned long long m_ = climbm; m_ != 0ull; m_ &= m_ - 1ull) {
                    const int kl = __builtin_ctzll(m_);
                    if (lane == kl) late = false;                  // (its slot is written here)
                    int i = uni(n_heap + (int)__popcll(restm & ((1ull << kl) - 1ull)));
                    const double kgh = rdlane(my_gh, kl), kg = rdlane(my_g, kl);
                    const int kid = __builtin_amdgcn_readlane(my_id, kl);
                    const int i0_ = i;
                    while (i > 0) {
                        JPL_T(16);
                        const int pa = uni((i - 1) / JPL_D);
                        double pgh, pg; int pid_;
                        hget_u(pa, pgh, pg, pid_);
                        JPL_CNT(20);
                        JPL_T(19);
                        const bool lt_ = less_u(kgh, kg, kid, pgh, pg, pid_);
                        JPL_T(22);
                        if (!lt_) break;
                        JPL_CNT(9);
                        if (lane == 0) hset(i, pgh, pg, pid_);
                        i = pa;
                        JPL_T(23);
                    }
                    if (lane == 0) hset(i, kgh, kg, kid);
                    JPL_T(25);
                }
            }
        }
        JPL_T(26);
        JPL_WSYNC();
        { const int nh_ = n_heap; n_heap += cnt - 1; fetch_root(); n_heap = nh_; }   // (the next pop's root; n_nodes still counts the old nodes)
        // ---------------- the expansion's stores: node records, open-list entries beyond the LDS part, the dict entry of the popped node
        if (ok) { nx[my_id] = my_x; ny[my_id] = my_y; nth[my_id] = my_th; ng[my_id] = my_g; npar[my_id] = cur; nprm[my_id] = lane; }
        if (late) { ov_gh[pos - JPL_HEAP_CAP] = my_gh; ov_g[pos - JPL_HEAP_CAP] = my_g; ov_id[pos - JPL_HEAP_CAP] = my_id; }
        if (lane == 0) htab[s] = cur;
        n_heap += cnt - 1; n_nodes += cnt;      // (the vacant root is counted in n_heap: cnt entries in, the vacancy out)
        JPL_WSYNC();
        JPL_T(4);                                    // appends + climbs
    }

    // ---------------- path: follow the predecessors from the goal (each through the dict's current entry for its pose), write outputs
    __syncthreads();
#ifdef JPL_STAMPS
    if (lane == 0 && r < 64) { for (int k = 0; k < 32; ++k) jpl_clk[r][k] = jpl_acc[k]; jpl_clk[r][7] = n_exp; jpl_clk[r][13] = n_nodes; jpl_clk[r][14] = n_heap; }
#endif
    if (lane == 0) {
        int np_ = 0;
        if (status == 0) {
            int id = goal_id, len = 0;
            while (id != 0 && len <= P.max_path) { // count
                ++len;
                const int pa = npar[id];
                unsigned s = jpl_hash(nx[pa], ny[pa], nth[pa], hmask);
                int cur_best = pa;
                while (htab[s] >= 0) {
                    const int j = htab[s];
                    if (nx[j] == nx[pa] && ny[j] == ny[pa] && nth[j] == nth[pa]) { cur_best = j; break; }
                    s = (s + 1) & hmask;
                }
                id = cur_best;
            }
            if (len > P.max_path) status = 6; // path longer than the output arrays
            else {
                np_ = len;
                id = goal_id;
                for (int k = len; k >= 1; --k) {
                    P.prims[(size_t)r * P.max_path + k - 1] = nprm[id];
                    double *nd = P.nodes + ((size_t)r * (P.max_path + 1) + k) * 3;
                    nd[0] = nx[id]; nd[1] = ny[id]; nd[2] = nth[id];
                    const int pa = npar[id];
                    unsigned s = jpl_hash(nx[pa], ny[pa], nth[pa], hmask);
                    int cur_best = pa;
                    while (htab[s] >= 0) {
                        const int j = htab[s];
                        if (nx[j] == nx[pa] && ny[j] == ny[pa] && nth[j] == nth[pa]) { cur_best = j; break; }
                        s = (s + 1) & hmask;
                    }
                    id = cur_best;
                }
                double *nd = P.nodes + (size_t)r * (P.max_path + 1) * 3;
                nd[0] = nx[0]; nd[1] = ny[0]; nd[2] = nth[0];
                P.cost[r] = ng[goal_id];
            }
        }
        P.status[r] = status; P.n_prims[r] = np_; P.n_expanded[r] = n_exp;
        sh_i[5] = np_;
    }
    __syncthreads();
    // trajectory: segment s = primitive prims[s] placed at node s, all points but the last (path_to_full_trajectory)
    const int np_ = sh_i[5], seg = P.n_pts - 1;
    for (int e = lane; e < np_ * seg; e += 64) {
        const int sidx = e / seg, j = e - sidx * seg;
        const double *nd = P.nodes + ((size_t)r * (P.max_path + 1) + sidx) * 3;
        const int k = P.prims[(size_t)r * P.max_path + sidx];
        const double *pt = P.mp_pts + ((size_t)k * P.n_pts + j) * 3;
        const double c = cos(nd[2]), s = sin(nd[2]);
        double tx = pt[0] * c + pt[1] * (-s), ty = pt[0] * s + pt[1] * c;
        if (!(nd[0] == 0.0 && nd[1] == 0.0)) { tx = tx + nd[0]; ty = ty + nd[1]; }
        double *o = P.traj + ((size_t)r * P.max_path * seg + e) * 3;
        o[0] = tx; o[1] = ty; o[2] = pt[2] + nd[2];
    }
}
