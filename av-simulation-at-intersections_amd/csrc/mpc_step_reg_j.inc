// mpc_step_reg_j.inc -- the rows of the augmented J of the one-wave register kernel: L y = rhs, column by column (Jr[N] declared by
// the includer).  Included by mpc_step_reg.inc twice: where the owner wavefront runs the phase itself (JSIM_J_WAIT empty), and in the
// HELP instantiations' helper loop, where a helper wavefront runs it BESIDE the owner's Cholesky, one column behind
// (JSIM_J_WAIT(n) = until the owner has published n columns of the factor).
    {
        JSIM_OPAQUE_ZERO(zj_);
        const double *const LcJ = Lc + zj_, *const invJ = invc + zj_, *const gvJ = gvc + zj_;
        const bool isrow = lane < N, isspd = !VS && lane >= N && lane < NR, isw = lane == NW;
        const int erow = isrow ? lane : -1;
        const int nspd = isspd ? lane - N : 0;
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            const double2 g2 = *(const double2 *)&gvJ[i];
            double r0 = isw ? g2.x : 0.0, r1 = isw ? g2.y : 0.0;
            r0 = (erow == i) ? 1.0 : r0;
            r1 = (erow == i + 1) ? 1.0 : r1;
            r0 = ((i >> 1) < nspd) ? dt : r0;
            Jr[i] = r0; Jr[i + 1] = r1;
        }
        // one software pipeline over all (column, chunk) pairs: while a chunk's FMAs issue, the next chunk -- of this column
        // or the first one of the next column -- is already in flight (pb toggles at compile time: everything is unrolled)
        double2 cb[2][CCH / 2];
        double invb[2];
        int pb = 0;
        JSIM_J_WAIT(1);
#pragma unroll
        for (int j = 0; j < CCH && j < N; j += 2) cb[0][j / 2] = *(const double2 *)&LcJ[j];
        invb[0] = invJ[0];
#pragma unroll
        for (int m = 0; m < N; ++m) {
            JSIM_J_WAIT(m + 2 < N ? m + 2 : N);   // (helper wavefront: columns m and m + 1 of the factor are published)
            const int j0 = m & ~1;
            const int nch = (N - j0 + CCH - 1) / CCH;
            double smul = 0.0;
#pragma unroll
            for (int c = 0; c < nch; ++c) {
                const int h = j0 + c * CCH;
                if (c + 1 < nch) {
#pragma unroll
                    for (int j = h + CCH; j < h + 2 * CCH && j < N; j += 2) cb[pb ^ 1][(j - h - CCH) / 2] = *(const double2 *)&LcJ[m * LDC + j];
                } else if (m + 1 < N) {
                    const int j1 = (m + 1) & ~1;
#pragma unroll
                    for (int j = j1; j < j1 + CCH && j < N; j += 2) cb[pb ^ 1][(j - j1) / 2] = *(const double2 *)&LcJ[(m + 1) * LDC + j];
                    invb[(m + 1) & 1] = invJ[m + 1];
                }
                // one wait for the chunk in hand (and the pivot read with it): behind it are this stage's reads -- the next chunk's, or the
                // next column's first chunk (without the pair an odd column does not use: it is never read) and its pivot
                if ((CHW & 2) && m + c > 0) {
                    const int j1 = (m + 1) & ~1;
                    jsim_chunk_wait(c + 1 < nch ? ((h + 2 * CCH < N ? h + 2 * CCH : N) - (h + CCH)) / 2
                                    : m + 1 < N ? ((j1 + CCH < N ? j1 + CCH : N) - j1) / 2 - ((m + 1) & 1) + 1 : 0);
                }
                JSIM_STAGE();
                if (c == 0) {
                    const double y = Jr[m] * invb[m & 1];
                    smul = y * invb[m & 1];
                    Jr[m] = y;
                }
#pragma unroll
                for (int j = h; j < h + CCH && j < N; j += 2) {
                    if (j == m) JSIM_PIN_PAIR(cb[pb][0]);   // (even m: .x of this pair is not used -- keep the read 16 bytes wide, see JSIM_PIN_PAIR)
                    const double2 c2 = cb[pb][(j - h) / 2];
                    if (j > m) { Jr[j] = fma(-c2.x, smul, Jr[j]); JSIM_PIN(Jr[j]); }
                    if (j + 1 > m) { Jr[j + 1] = fma(-c2.y, smul, Jr[j + 1]); JSIM_PIN(Jr[j + 1]); }
                }
                JSIM_STAGE();
                pb ^= 1;
            }
        }
    }
    if (lane == NW) {
#pragma unroll
        for (int j = 0; j < N; j += 2) *(double2 *)&wvc[j] = double2{Jr[j], Jr[j + 1]};
    }
