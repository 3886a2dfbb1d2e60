// How the History recorder's buffers (jsim_loop_set_recorder) are read, stated once for reason_ticks_kernel, conflict_ticks_kernel,
// static_ticks_kernel, the episode kernels and the per-tick kernels that came after them (DESIGN.md section 20).  One wavefront per
// ego, ticks 64 at a time, lane t owns tick k0 + t.  Every mask is a ballot, so every branch on one is uniform.

struct RecorderBuf {
    int B, n_ticks;
    const double *rec;        // [n][B][JSIM_REC_FIELDS]
    const int *flags;         // [n][B]
    const double *x_first;    // [B][4] x, y, v, yaw at the start of tick 0
    const double *x_spawn;    // [B][4] the respawn state
};
static RecorderBuf recorder_buf(int B, int n_ticks, const double *rec, const int *flags, const double *x_first, const double *x_spawn)
{
    return RecorderBuf{B, n_ticks, rec, flags, x_first, x_spawn};
}

// A record with this flag ends an episode: the ego reached its goal or its age limit and is respawned behind it
__device__ __forceinline__ bool jrw_is_end(int flag) { return (flag & (JSIM_REC_GOAL | JSIM_REC_AGE)) != 0; }

// Ego e's flag of tick k, 0 beyond the records
__device__ __forceinline__ int jrw_flag(const RecorderBuf &R, int e, int k) { return k < R.n_ticks ? R.flags[(size_t)k * R.B + e] : 0; }

// The ticks of a chunk that end an episode, from every lane's tick k and its flag.  close_last: the last record closes the running
// episode too (conflicts and static write their episode outputs at an end; the reasons and the episode table leave it open)
__device__ __forceinline__ unsigned long long jrw_end_mask(const RecorderBuf &R, int k, int flag, bool close_last)
{
    return __ballot(k < R.n_ticks && ((close_last && k == R.n_ticks - 1) || jrw_is_end(flag)));
}

// An ego's pose at the start of tick k: x_first, x_spawn behind a record that ended an episode (after_end), or the record before
__device__ __forceinline__ void jrw_pose_at(const RecorderBuf &R, int e, int k, bool after_end, double &x, double &y, double &yaw)
{
    if (k == 0) {
        const double *p = R.x_first + 4 * (size_t)e;
        x = p[0]; y = p[1]; yaw = p[3];
    } else if (after_end) {
        const double *p = R.x_spawn + 4 * (size_t)e;
        x = p[0]; y = p[1]; yaw = p[3];
    } else {
        const double *p = R.rec + JSIM_REC_FIELDS * ((size_t)(k - 1) * R.B + e);
        x = p[0]; y = p[1]; yaw = p[2];
    }
}
__device__ __forceinline__ void jrw_pose(const RecorderBuf &R, int e, int k, double &x, double &y, double &yaw)
{
    jrw_pose_at(R, e, k, k > 0 && jrw_is_end(R.flags[(size_t)(k - 1) * R.B + e]), x, y, yaw);
}

// An ego's state (x, y, v, yaw) at the start of tick k: jrw_pose_at's rule with the speed (the cut-off replay, the fork and the
// predictions' scores read their states by it)
__device__ __forceinline__ void jct_state_at(const RecorderBuf &R, int e, int k, double &x, double &y, double &v, double &yaw)
{
    // one pointer and one order of loads, then a choice between values: the two layouts ((x, y, v, yaw) of a state, (x, y, yaw, v) of
    // a record) as two branches were merged by the compiler into stores to scratch at a computed place
    const bool state = k == 0 || jrw_is_end(R.flags[(size_t)(k - 1) * R.B + e]);
    const double *const first = R.x_first, *const spawn = R.x_spawn;
    const double *p = state ? (k == 0 ? first : spawn) + 4 * (size_t)e : R.rec + JSIM_REC_FIELDS * ((size_t)(k - 1) * R.B + e);
    const double q2 = p[2], q3 = p[3];
    x = p[0]; y = p[1]; v = state ? q2 : q3; yaw = state ? q3 : q2;
}

// The ticks of a chunk that start an episode: those behind an end, of this chunk or the last of the chunk before.  tick0: this is
// the first chunk and tick 0 counts as a start (for the episode outputs it does; for the reasons the carry decides instead)
__device__ __forceinline__ unsigned long long jrw_start_mask(unsigned long long e_prev, unsigned long long e_cur, bool tick0)
{
    return (e_cur << 1) | (tick0 ? 1ull : (e_prev >> 63));
}

// One chunk of the walk: its first tick, its ticks, the end masks of the chunk before and of this one, the start mask they give.
// The caller hands each chunk's end mask in, so it may fetch the next chunk's ahead of time (conflict_ticks_kernel's first sweep).
struct RecChunk {
    int k0, cnt;
    unsigned long long e_prev, e_cur, s_cur;
};
__device__ __forceinline__ void jrw_enter(RecChunk &C, const RecorderBuf &R, int k0, unsigned long long e_cur, bool tick0_starts)
{
    C.e_prev = k0 == 0 ? 0ull : C.e_cur;
    C.e_cur = e_cur;
    C.k0 = k0;
    C.cnt = (R.n_ticks - k0) < 64 ? (R.n_ticks - k0) : 64;
    C.s_cur = jrw_start_mask(C.e_prev, e_cur, k0 == 0 && tick0_starts);
}

// The lanes [pos, e] as a mask
__device__ __forceinline__ unsigned long long jrw_lanes(int pos, int e) { return (~0ull << pos) & (~0ull >> (63 - e)); }

// The episode segments of a chunk, one after the other: body(pos, e, starts, ends) for the lanes [pos, e]; starts: lane pos is an
// episode's first tick; ends: the episode ends with lane e's record (else it runs on into the next chunk)
template <class F> __device__ __forceinline__ void jrw_segments(const RecChunk &C, F &&body)
{
    for (int pos = 0; pos < C.cnt;) {
        const unsigned long long rem = C.e_cur >> pos;
        const int e = rem ? pos + (int)__builtin_ctzll(rem) : C.cnt - 1;
        body(pos, e, ((C.s_cur >> pos) & 1ull) != 0ull, rem != 0ull);
        pos = e + 1;
    }
}

// Slot q = this lane's tick of an episode table ep_i [n][B][ni], ep_d [n][B][nd]: off an episode's first tick it holds no episode
// outputs, -1 and NaN
__device__ __forceinline__ void jrw_blank_slot(const RecChunk &C, int lane, size_t q, int *ep_i, int ni, double *ep_d, int nd)
{
    if ((C.s_cur >> lane) & 1ull) return;
    for (int j = 0; j < ni; ++j) ep_i[ni * q + j] = -1;
    for (int j = 0; j < nd; ++j) ep_d[nd * q + j] = NAN;
}
