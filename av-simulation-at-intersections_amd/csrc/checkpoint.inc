// Checkpoints of a running loop (DESIGN.md section 30): the kernels that copy a loop's live state into a slot of its slabs and back
// (checkpoint_copy_kernel: one launch for every array of the state, plain vector stores), and that gather rows of slots into the
// buffers of a new loop (checkpoint_load_kernel: one wavefront per destination row; checkpoint_vehicles_kernel: the scripted
// vehicles of every (source set, slot) pair the rows name).  Copies only: no value is computed, so a restored or forked loop goes on
// bit for bit.  The loops' own kernels are not touched.
//
// The kernels are compiled in jsim_plan.hip's translation unit (-DJSIM_PLAN_TU), beside the plan record's, so that the library's
// main code object stays what it was, byte for byte (section 29 measured what growing it costs); the rest of the library sees the
// parameter structs and the declarations only.

// One array of a save or a restore: bytes is a multiple of 4, src and dst are 4-byte aligned (checked on the host)
struct CkptCopy {
    const void *src;
    void *dst;
    long long bytes;
};

// The table of one launch, passed by value: block (x, y) works on array y
struct CkptCopyP {
    int n;
    CkptCopy e[JSIM_CKPT_MAX_ARRAYS];
};

// One per-ego array of a gather: slab [n_slots][B][row_bytes] -> dst [n_rows][row_bytes]; row_bytes is a multiple of 4
struct CkptField {
    const char *slab;
    char *dst;
    long long row_bytes;
};

struct CkptLoadP {
    int B, n_rows, n_fields;
    const int *ego, *slot;    // [n_rows] the source ego and the slot of every destination row
    CkptField f[JSIM_CKPT_MAX_ARRAYS];
};

struct CkptVehP {
    int n_veh, n_obs;         // destination vehicles; vehicles per slot of the slab
    const int *src, *slot;    // [n_veh] the source vehicle and the slot of every destination vehicle
    const double *slab;       // [n_slots][n_obs][4]
    double *state;            // [n_veh][4]
};

#ifndef JSIM_PLAN_TU
__global__ void checkpoint_copy_kernel(const CkptCopyP P);
__global__ void checkpoint_load_kernel(const CkptLoadP P);
__global__ void checkpoint_vehicles_kernel(const CkptVehP P);
#else
template <class W> static __device__ __forceinline__ void ckpt_copy_words(const void *src, void *dst, size_t n, size_t i0, size_t step)
{
    const W *const s = (const W *)src;
    W *const d = (W *)dst;
    for (size_t i = i0; i < n; i += step) d[i] = s[i];
}

// Array blockIdx.y, grid-strided over blockIdx.x: 16-byte words where both pointers and the size allow them, else 8, else 4
__global__ __launch_bounds__(256) void checkpoint_copy_kernel(const CkptCopyP P)
{
    if ((int)blockIdx.y >= P.n) return;
    const CkptCopy c = P.e[blockIdx.y];
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    const unsigned long long bits = (unsigned long long)(uintptr_t)c.src | (unsigned long long)(uintptr_t)c.dst | (unsigned long long)c.bytes;
    if ((bits & 15ull) == 0ull) ckpt_copy_words<uint4>(c.src, c.dst, (size_t)c.bytes >> 4, i0, step);
    else if ((bits & 7ull) == 0ull) ckpt_copy_words<unsigned long long>(c.src, c.dst, (size_t)c.bytes >> 3, i0, step);
    else ckpt_copy_words<unsigned>(c.src, c.dst, (size_t)c.bytes >> 2, i0, step);
}

// One wavefront per destination row r: ego ego[r] of slot slot[r], array after array, the lanes side by side over the row's 4-byte
// words -- the T doubles of oa and od take the lanes 0 .. 2T - 1, a scalar takes lane 0 (and 1)
__global__ __launch_bounds__(64) void checkpoint_load_kernel(const CkptLoadP P)
{
    const int lane = threadIdx.x, r = blockIdx.x;
    if (r >= P.n_rows) return;
    const size_t from = (size_t)P.slot[r] * P.B + P.ego[r];
    for (int k = 0; k < P.n_fields; ++k) {
        const CkptField f = P.f[k];
        const unsigned *const s = (const unsigned *)(f.slab + from * (size_t)f.row_bytes);
        unsigned *const d = (unsigned *)(f.dst + (size_t)r * (size_t)f.row_bytes);
        const int words = (int)(f.row_bytes >> 2);
        for (int w = lane; w < words; w += 64) d[w] = s[w];
    }
}

// One thread per double of the destination vehicles' states
__global__ __launch_bounds__(256) void checkpoint_vehicles_kernel(const CkptVehP P)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)P.n_veh * 4) return;
    const size_t o = i >> 2, j = i & 3;
    P.state[i] = P.slab[((size_t)P.slot[o] * P.n_obs + P.src[o]) * 4 + j];
}
#endif
