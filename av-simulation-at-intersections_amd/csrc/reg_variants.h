// reg_variants.h -- the register-resident kernels libjsim_mpc.so instantiates, and which one a launch takes.  Host-only C++17:
// jsim_mpc.hip instantiates, declares and launches exactly these rows; config.REG_VARIANTS mirrors them for Python and a CPU test
// (tests/test_host_cpu.py) compiles this header to compare the table and the dispatch against config / bench.kernel_name.
#pragma once

#include <cstdlib>

// One row per instantiation: X(W, T, PRE, WPE, HELP)
//   W    1: mpc_step_reg_kernel<T, PRE, WPE, HELP> (one wavefront per ego; every row stored for 13 <= T <= 20, virtual speed rows for
//           21 <= T <= 31), 4: mpc_step_reg4_kernel<T, PRE> (four wavefronts per ego, two lanes per row; its rows carry WPE = 1,
//           HELP = false, which are not parameters of that template)
//   PRE  the loop glue inside the launch (the fused scenario loop)
//   WPE  waves per SIMD the register budget is set for (mpc_step_reg.inc): T = 13 fits 256 registers without scratch -- two waves
//        per SIMD at every batch size; T = 20 has a 256-register form for batches above one ego per SIMD
//   HELP three helper wavefronts per ego, taken at B <= one ego per CU.  Measured at 256 egos, closed loop (tools/dev/help_ab13.py):
//        T = 13 +8 %, 15 +6 %, 16 +11 %, 20 +11-14 %, 25 +6 %; T = 30 LOSES 2 % (448 registers, 72 KB of LDS: handing 61 rows of 60
//        doubles over costs what the helpers save) and has none.  With PRE as well: the reference's stock horizon and the headline's
//        (T = 16 with PRE and HELP is a build the ISA guard refuses -- vector code in front of a join block's exec restore, section 5
//        fact 6 of DESIGN.md -- and is not instantiated).
// The kernels are templates on T, fully unrolled: a horizon is fast if it has rows here (7 s of compile time per row) and runs on the
// LDS kernel otherwise (any T <= 48; 4-6 x slower: tools/dev/horizon_ab.py).  BASELINE.json's configurations use 13 (the
// reference's stock horizon), 20, 30 and 40; the others are there so that a horizon near them does not fall off that cliff.
// Grouped per horizon: a kernel translation unit of the split build (-DJSIM_KERNEL_TU=T) instantiates JSIM_REG_ROW_<T>.
#define JSIM_REG_ROW_13(X) X(1, 13, true, 1, false) X(1, 13, false, 2, false) X(1, 13, false, 1, true) X(1, 13, true, 1, true)
#define JSIM_REG_ROW_15(X) X(1, 15, true, 1, false) X(1, 15, false, 1, false) X(1, 15, false, 1, true)
#define JSIM_REG_ROW_16(X) X(1, 16, true, 1, false) X(1, 16, false, 1, false) X(1, 16, false, 1, true)
#define JSIM_REG_ROW_20(X) X(1, 20, true, 1, false) X(1, 20, false, 1, false) X(1, 20, false, 2, false) X(1, 20, false, 1, true) \
                           X(1, 20, true, 1, true)
#define JSIM_REG_ROW_25(X) X(1, 25, true, 1, false) X(1, 25, false, 1, false) X(1, 25, false, 1, true)
#define JSIM_REG_ROW_30(X) X(1, 30, true, 1, false) X(1, 30, false, 1, false)
#define JSIM_REG_ROW_32(X) X(4, 32, true, 1, false) X(4, 32, false, 1, false)
#define JSIM_REG_ROW_40(X) X(4, 40, true, 1, false) X(4, 40, false, 1, false)

#define JSIM_CAT_(a, b) a##b
#define JSIM_CAT(a, b) JSIM_CAT_(a, b)

#if defined(JSIM_DEV_NO_REG)   /* development builds of the planner / glue: no register kernel */
#define JSIM_REG_VARIANTS(X)
#elif defined(JSIM_DEV_ONLY_T) /* development builds: one horizon's rows (seconds instead of minutes to compile) */
#define JSIM_REG_VARIANTS(X) JSIM_CAT(JSIM_REG_ROW_, JSIM_DEV_ONLY_T)(X)
#else
#define JSIM_REG_VARIANTS(X) JSIM_REG_ROW_13(X) JSIM_REG_ROW_15(X) JSIM_REG_ROW_16(X) JSIM_REG_ROW_20(X) JSIM_REG_ROW_25(X) \
                             JSIM_REG_ROW_30(X) JSIM_REG_ROW_32(X) JSIM_REG_ROW_40(X)
#endif

struct RegVariant {
    int W, T; bool PRE; int WPE; bool HELP; // W = 0: no row, the LDS kernel
    constexpr bool operator==(const RegVariant &o) const
    {
        return W == o.W && T == o.T && PRE == o.PRE && WPE == o.WPE && HELP == o.HELP;
    }
    constexpr int threads() const { return W == 4 || HELP ? 256 : 64; }
};

constexpr bool has_reg_variant(const RegVariant &v)
{
#define JSIM_X(w, t, p, e, h) if (v == RegVariant{w, t, p, e, h}) return true;
    JSIM_REG_VARIANTS(JSIM_X)
#undef JSIM_X
    return false;
}

constexpr bool has_reg_kernel(int T)
{
#define JSIM_X(w, t, p, e, h) if (T == t) return true;
    JSIM_REG_VARIANTS(JSIM_X)
#undef JSIM_X
    return false;
}

// The row a launch of B egos takes.  HELP while there is at most one ego per CU (B <= help_max_b); otherwise two waves per SIMD where
// that is the horizon's only one-wave form or there are more egos than SIMDs (B >= w2_min_b); otherwise one wave per SIMD; otherwise
// the four-wave kernel.
constexpr RegVariant select_reg_variant(int T, int B, bool pre, int help_max_b, int w2_min_b)
{
    const RegVariant help = {1, T, pre, 1, true}, w2 = {1, T, pre, 2, false}, w1 = {1, T, pre, 1, false}, four = {4, T, pre, 1, false};
    if (B <= help_max_b && has_reg_variant(help)) return help;
    if (has_reg_variant(w2) && (!has_reg_variant(w1) || B >= w2_min_b)) return w2;
    if (has_reg_variant(w1)) return w1;
    if (has_reg_variant(four)) return four;
    return RegVariant{0, T, pre, 0, false};
}

// The thresholds, from the environment (A/B knobs): JSIM_W2_MIN_B, default 1025 (more egos than SIMDs: 256 CUs x 4); JSIM_HELP_MAX_B,
// default (unset or negative) the device's CU count -- a HELP ego needs a CU to itself (four wavefronts of 270-350 registers).
inline int reg_w2_min_b(const char *env) { return env ? std::atoi(env) : 1025; }
inline int reg_help_max_b(const char *env, int cu_count) { const int b = env ? std::atoi(env) : -1; return b < 0 ? cu_count : b; }
