// mpc_step_reg_chol.inc -- columns [JSIM_CH_K0, JSIM_CH_KE) of the one-wave register kernel's right-looking Cholesky factorisation,
// on the entries JSIM_CH_A(j), j in [JSIM_CH_K0, JSIM_CH_KE), of the lane's row (everything in front of column JSIM_CH_K0 already
// eliminated from them).  Included by mpc_step_reg.inc where the owner wavefront factors (all N columns; in the column-split HELP
// instantiations its half, [0, NS)) and in those instantiations' helper loop, where helper 2 factors [NS, N).
// Column k (entries j >= k, unscaled: c_j = A^(k)[j][k]) goes to Lc[k][.]; every lane reads it back as a broadcast
// vector and eliminates:  A[j] -= (A[k] / c_k) c_j ;  L[.][k] = c / sqrt(c_k).
// Look-ahead of one column: as soon as column k's entry c_{k+1} has updated A[k+1], column k + 1 is written out and
// its pivot's reciprocal root started -- its LDS round trip and that chain then run under the rest of column k's FMAs.
    {
        constexpr int K0 = JSIM_CH_K0, KE = JSIM_CH_KE;
        JSIM_OPAQUE_ZERO(zc_);
        const double *const LcC = Lc + zc_;
        double inv, tmul;
        {
            if (K0 == 0 ? lane < N : (lane >= K0 && lane < N)) Lc[K0 * LDC + lane] = JSIM_CH_A(K0);
            double ck = rdlane(JSIM_CH_A(K0), K0); // the pivot travels by v_readlane: its rsqrt chain overlaps the LDS round trip
            if (!(ck > 0.0)) ck = 1e-300;
            inv = fast_rsqrt(ck);
            tmul = JSIM_CH_A(K0) * (inv * inv);
        }
#pragma unroll
        for (int k = K0; k < KE; ++k) {
            LDS_SYNC(); // column k is in LDS
            const int j0 = k & ~1;
            const int nch = (KE - j0 + CCH - 1) / CCH;
            double2 cb[2][CCH / 2];
#pragma unroll
            for (int j = j0; j < j0 + CCH && j < KE; j += 2) cb[0][(j - j0) / 2] = *(const double2 *)&LcC[k * LDC + j];
            if (HELP) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (column k is written BEFORE its pivot: the helpers poll the pivot;
            if (lane == k) invc[k] = inv;                                      //  a wave's LDS operations are performed in order, the compiler keeps this one)
            const double tk = tmul;
            if (k + 1 < KE) { // the one update the next column needs, then publish it
                JSIM_STAGE();
                // (even k: only .y of the pair that holds column entry k + 1 is used; left alone, that read is narrowed to 8 bytes and every
                //  read behind it re-merged into 8-byte-aligned pairs, each with an address add of its own -- both halves count as used here)
                if (!(k & 1)) JSIM_PIN_PAIR(cb[0][0]);
                const double cn = ((k + 1) & 1) ? cb[0][(k + 1 - j0) / 2].y : cb[0][(k + 1 - j0) / 2].x;
                JSIM_CH_A(k + 1) = fma(-tk, cn, JSIM_CH_A(k + 1));
                JSIM_PIN(JSIM_CH_A(k + 1));
                if (lane >= k + 1 && lane < N) Lc[(k + 1) * LDC + lane] = JSIM_CH_A(k + 1);
                double ck = rdlane(JSIM_CH_A(k + 1), k + 1);
                if (!(ck > 0.0)) ck = 1e-300;
                inv = fast_rsqrt(ck);
                tmul = JSIM_CH_A(k + 1) * (inv * inv);
            }
#pragma unroll
            for (int c = 0; c < nch; ++c) {
                const int h = j0 + c * CCH;
                if (c + 1 < nch) {
#pragma unroll
                    for (int j = h + CCH; j < h + 2 * CCH && j < KE; j += 2) cb[(c + 1) & 1][(j - h - CCH) / 2] = *(const double2 *)&LcC[k * LDC + j];
                }
                // behind this chunk's reads: the next chunk's; behind the first chunk's also the pivot and column k + 1 (written above).
                // (In front of the stage boundary: behind it the scheduler moves the chunk's FMAs above the wait.)
                if ((CHW & 1) && k + 1 < KE) jsim_chunk_wait((c + 1 < nch ? ((h + 2 * CCH < KE ? h + 2 * CCH : KE) - (h + CCH)) / 2 : 0) + (c == 0 ? 2 : 0));
                JSIM_STAGE();
#pragma unroll
                for (int j = h; j < h + CCH && j < KE; j += 2) {
                    const double2 c2 = cb[c & 1][(j - h) / 2];
                    if (j > k + 1) { JSIM_CH_A(j) = fma(-tk, c2.x, JSIM_CH_A(j)); JSIM_PIN(JSIM_CH_A(j)); }
                    if (j + 1 > k + 1) { JSIM_CH_A(j + 1) = fma(-tk, c2.y, JSIM_CH_A(j + 1)); JSIM_PIN(JSIM_CH_A(j + 1)); }
                }
                JSIM_STAGE();
            }
        }
    }
