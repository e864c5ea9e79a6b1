// hpe_opt_descent_body.inc -- the statements of k_opt_descent, included as text by it and by
// its lane form k_opt_descent_b (hpe_optimise.hpp).  In scope: STAGED (a constant expression),
// op (this swarm's DevOpt), og (the frame's descriptor), Hg (the hand), g (the generation).
    extern __shared__ __align__(16) unsigned char dyn[];
    const DevObs o = *og;
    __shared__ RefineSm rs;
    __shared__ DevHand hs;
    __shared__ double pbrow[32];
    __shared__ int sel_s[OPT_GRADITER];
    __shared__ int flag;
    const int i = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
    stage_hand<RF_NT>(hs, Hg);
    const DevHand *__restrict__ H = &hs;
    using CV = std::conditional_t<STAGED, CloudView, CloudGlobal>;
    CV cv;
    int32_t *match = op.match + (size_t)i * op.n_cap;
    if (STAGED) {
        double *cx = (double *)dyn, *cy = cx + o.n, *cz = cy + o.n;
        for (int p = t; p < o.n; p += RF_NT) {
            cx[p] = gp(o.cx)[p];
            cy[p] = gp(o.cy)[p];
            cz[p] = gp(o.cz)[p];
        }
        if constexpr (STAGED) cv = CV{cx, cy, cz, o.n};
        match = (int32_t *)(cz + o.n);
    }
    if constexpr (!STAGED) cv = obs_cloud(o);
    const size_t e = (size_t)i * HPE_DOF + t;
    double vel = 0.0;
    if (t < HPE_DOF) {
        rs.x0[t] = op.x[e];
        vel = op.v[e];
    }
    if (t < OPT_GRADITER) {  // permu = randi(graditer, [0, 25])
        const double u = philox_u01(op.seed, ST_OPT_PERM, g, i, t);
        const int s = (int)floor(u * HPE_DOF);
        sel_s[t] = s > HPE_DOF - 1 ? HPE_DOF - 1 : s;
    }
    double pci = op.pc[i];
    bool improved = false;
    __syncthreads();
    const double e5 = 1e-5;  // cal_gradient eps (PSO.cpp:384)
    double fk = 0;
    int evals = 0;
    StampClock sc;
    sc.start();
    for (int m = 0; m < OPT_GRADITER; ++m) {
        if (m == 0) {  // f_k = cal_cost2(ctheta, matchId, true)
            if (t < HPE_DOF) rs.base.th[t] = rs.x0[t];
            __syncthreads();
            if (w == 0) fk_wave<true>(rs.base, H);
            __syncthreads();
            const DepthG dg = depth_issue_w0(rs.base, o, H);
            double al = search_align<RF_NT, true>(rs.base, cv, H, match, load_pt(cv, t));
            double co = (t < 144) ? collide_term(rs.base, t, H) : 0.0;
            double dep = depth_finish(dg, o, t < HPE_NS);
            fk = block_sum1<RF_NT>(rs.red, (al * o.lambda + dep) + co);
            sc.lap(26);
        }
        const int sel = sel_s[m];
        if (w < 2) {  // cal_gradient: theta +/- eps on coordinate sel, frozen matchId
            if (l < HPE_DOF) rs.w[w].th[l] = (l == sel) ? (w ? rs.x0[l] - e5 : rs.x0[l] + e5) : rs.x0[l];
            wave_sync();
            const double f = eval_wave_frozen<true>(rs.w[w], o, cv, H, match);
            if (l == 0) rs.f[w] = f;
        }
        __syncthreads();
        const double gs = (rs.f[0] - rs.f[1]) / (2 * e5);
        // g is gs on coordinate sel, 0 elsewhere, p = -1 * g; dot(g, p) by two accumulators
        // (op_dot::direct_dot_arma) has the one nonzero term, exactly
        const double gl = (t == sel) ? gs : 0.0;
        const double pl = -1 * ((l == sel) ? gs : 0.0);  // p = -1 * g, this thread's lane
        const double gp = gs * (-1 * gs);
        __syncthreads();  // rs.f is the Goldstein nodes' next
        sc.lap(27);
        double facc = fk;
        const double tk = gold_tree<false, GOLD_OPT8>(rs, o, cv, H, match, fk, gp, pl, 0.0, evals, &facc);
        sc.start();
        if (t < HPE_DOF) rs.x0[t] = rs.x0[t] - tk * gl;
        __syncthreads();
        double f2 = fk;  // tk == 0: theta unchanged, same matchId -> same cost
        if (tk != 0) {
            if (m == 0) {  // cal_cost2(ctheta, matchId, true): rs.base holds the new spheres
                const DepthG dg = depth_issue_w0(rs.base, o, H);
                double al = search_align<RF_NT, true>(rs.base, cv, H, match, load_pt(cv, t));
                double co = (t < 144) ? collide_term(rs.base, t, H) : 0.0;
                double dep = depth_finish(dg, o, t < HPE_NS);
                f2 = block_sum1<RF_NT>(rs.red, (al * o.lambda + dep) + co);
            } else {
                f2 = facc;
            }
        }
        if (f2 < pci) {  // pcost / pbest_pos (:627-632)
            pci = f2;
            improved = true;
            if (t < HPE_DOF) pbrow[t] = rs.x0[t];
        }
        fk = f2;
        sc.lap(28);
    }
    if (t < HPE_DOF) {  // check_constraints(ctheta, cveloc): above max -> MIN (:372)
        const double *lb = op.bounds, *ub = op.bounds + HPE_DOF;
        const double xo = rs.x0[t];
        double xn = xo;
        if (xo < lb[t]) { xn = lb[t]; vel = 0.; }
        if (xo > ub[t]) { xn = lb[t]; vel = 0.; }
        op.x[e] = xn;
        op.v[e] = vel;
        if (improved) op.pb[e] = pbrow[t];
    }
    if (t == 0) op.pc[i] = pci;
    // last workgroup: gbest <- particles.col(argmin pcost) if better (:643-650)
    Smem &sm = *reinterpret_cast<Smem *>(&rs);  // the refine workspace is dead here
    static_assert(sizeof(Smem) <= sizeof(RefineSm), "Smem overlay");
    if (arrive_last_sharded(op.ctr, (unsigned)op.P, &flag)) opt_update_gbest(op, sm, false, 0, false);
