// mpc_step_reg_s2.inc -- S2 of the one-wave register kernel: rollout of the warm start from the current state
// (main/lib/mpc.py:115-129 _predict_motion -> lib/simulation.py:35-47).  Included by mpc_step_reg.inc where the phase runs: after S1
// in the plain kernels, INSIDE S1 in the HELP instantiations (the owner rolls out while the helper wavefronts scan the path -- the
// rollout does not need the index).  In: sx, sy, sv, syaw, wa_t, wtan (= tan of the warm start's clamped steer); out: bv, bth (lane t: state at time t), sn, cs
// -- and bx, by when the debug entry asks for xbar (P.dbg_xbar), their only reader.
    {
        const double tan_t = wtan; // tan of the clamped steer, evaluated where the warm start was written
        double vcur = sv;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            double vn = vcur + rdlane(wa_t, j) * dt;
            vn = (P.vmax_plant < vn) ? P.vmax_plant : vn;
            vn = (P.vmin > vn) ? P.vmin : vn;
            vcur = vn;
            if (lane == j + 1) bv = vn;
        }
        const double w = ((bv / P.L) * tan_t) * dt;
        // (short horizons keep the v_readlane chains: at T = 13 the three LDS round trips cost more than they save;
        //  A/B on one box: T = 13 -1.3 %, T = 20 +1.2 %, T = 30 +3.2 %)
        constexpr bool S2WIN = T >= 16;
        if (!S2WIN) {
        double thcur = syaw;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            thcur = thcur + rdlane(w, j);
            if (lane == j + 1) bth = thcur;
        }
        sincos(bth, &sn, &cs);
        if (P.dbg_xbar) { // the x and y sums have one reader, the debug entry's xbar: no solve needs them
        const double ix = (bv * cs) * dt, iy = (bv * sn) * dt;
        double xcur = sx, ycur = sy;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            xcur = xcur + rdlane(ix, j);
            ycur = ycur + rdlane(iy, j);
            if (lane == j + 1) { bx = xcur; by = ycur; }
        }
        }
        } else {
        // Sequential sums in the reference's order, every prefix at once: the T increments sit behind T zeros in LDS and
        // lane L adds z[L], .., z[L + T - 1] to the start value -- T - L exact no-ops (+ 0.0), then inc_0, .., inc_{L-1}.
        // One ds_read with an immediate offset and one add per term (the table area is free until S3 fills it).
        // (JSIM_S2_SCR: 4T doubles of the including wave's -- the owner's is the table area, free until S3 fills it)
        double *const zx = JSIM_S2_SCR, *const zy = JSIM_S2_SCR + 2 * T;
        static_assert(4 * T <= TQ_COUNT * TP, "scratch fits the table area");
        const int li = lane <= T ? lane : T;
        if (lane < T) { zx[lane] = 0.0; zx[T + lane] = w; }
        LDS_SYNC();
        {
            double th = syaw;
#pragma unroll
            for (int t = 0; t < T; ++t) th += zx[li + t];
            bth = th;
        }
        sincos(bth, &sn, &cs);
        if (P.dbg_xbar) { // the x and y sums have one reader, the debug entry's xbar: no solve needs them (nor zy's zeros)
            const double ix = (bv * cs) * dt, iy = (bv * sn) * dt;
            LDS_SYNC();
            if (lane < T) { zy[lane] = 0.0; zx[T + lane] = ix; zy[T + lane] = iy; }
            LDS_SYNC();
            double xc = sx, yc = sy;
#pragma unroll
            for (int t = 0; t < T; ++t) { xc += zx[li + t]; yc += zy[li + t]; }
            bx = xc; by = yc;
        }
        LDS_SYNC();
        }
    }
