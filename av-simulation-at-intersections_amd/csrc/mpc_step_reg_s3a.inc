// mpc_step_reg_s3a.inc -- the part of S3 (linearisation about the rollout) that needs neither the nearest index nor the reference
// window: the seven coefficients of lane t < T and the six prefix scans over them.  Included by mpc_step_reg.inc where it runs: in the
// owner's S3, and in helper 1's HB_NEXT, which runs it for the next tick under this tick's tail (the same operations on the same
// operands in the same order).  In: tl, lane, dt, P.L, the state sx, sy, sv, syaw and S2's bv, bth, sn, cs; out: al, be, alp, bep, ccx,
// ccy, kt (zero outside lane t < T) and PA, PB, PAP, PBP, FX, FY.
    if (tl) {
        al = dt * cs;
        be = (-dt * bv) * sn;
        alp = dt * sn;
        bep = (dt * bv) * cs;
        ccx = ((dt * bv) * sn) * bth;
        ccy = ((-dt * bv) * cs) * bth;
        kt = (dt * bv) / P.L;
    }
    PA = wexscan_dpp(al, lane); PB = wexscan_dpp(be, lane);
    PAP = wexscan_dpp(alp, lane); PBP = wexscan_dpp(bep, lane);
    FX = sx + wexscan_dpp(fma(al, sv, fma(be, syaw, ccx)), lane);
    FY = sy + wexscan_dpp(fma(alp, sv, fma(bep, syaw, ccy)), lane);
