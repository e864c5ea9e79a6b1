// hpe_opt_move_body.inc -- the statements of k_opt_move, included as text by it and by its
// lane form k_opt_move_b (hpe_optimise.hpp).  In scope: op (this swarm's DevOpt), og (the
// frame's descriptor), Hg (the hand), g (the generation).
    const DevObs o = *og;
    __shared__ Smem sm;
    __shared__ int flag;
    const int i = blockIdx.x, t = threadIdx.x;
    stage_hand<HPE_NT>(sm.hand, Hg);
    const DevHand *__restrict__ H = &sm.hand;
    const size_t e = (size_t)i * HPE_DOF + t;
    double xn = 0;
    if (t < HPE_DOF) {
        const double xo = op.x[e], vo = op.v[e], pbi = op.pb[e], gb = op.gbest[t];
        const double rp = philox_u01(op.seed, ST_OPT_RP, g, i, t);
        const double rg = philox_u01(op.seed, ST_OPT_RG, g, i, t);
        double vn = (op.w * vo + (op.c1 * rp) * (pbi - xo)) + (op.c2 * rg) * (gb - xo);
        xn = xo + vn;
        const double xr = xn;
        const double *lb = op.bounds, *ub = op.bounds + HPE_DOF;
        if (xr < lb[t]) { xn = lb[t]; vn = 0.; }
        if (xr > ub[t]) { xn = lb[t]; vn = 0.; }
        op.v[e] = vn;
        op.x[e] = xn;
        sm.fk.th[t] = xn;
    }
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt(cv, t);
    __syncthreads();
    const double fx = eval_block<EV_COST, HPE_NT>(sm, o, cv, H, nullptr, pre);
    const double pci = op.pc[i];
    if (fx < pci) {  // :682-686
        if (t < HPE_DOF) op.pb[e] = xn;
        if (t == 0) op.pc[i] = fx;
    }
    if (arrive_last_sharded(op.ctr, (unsigned)op.P, &flag)) opt_update_gbest(op, sm, true, g, false);
