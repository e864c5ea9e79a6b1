// hpe_opt_init_body.inc -- the statements of k_opt_init, included as text by it and by its
// lane form k_opt_init_b (hpe_optimise.hpp).  In scope: op (this swarm's DevOpt), x0 (26
// doubles), og (the frame's descriptor), Hg (the hand).
    const DevObs o = *og;
    __shared__ Smem sm;
    __shared__ int flag;
    const int i = blockIdx.x, t = threadIdx.x;
    stage_hand<HPE_NT>(sm.hand, Hg);
    const DevHand *__restrict__ H = &sm.hand;
    const double *sd = op.bounds + 2 * HPE_DOF;
    if (t < HPE_DOF) {
        const size_t e = (size_t)i * HPE_DOF + t;
        const double x = x0[t] + op.normals[e] * sd[t];
        sm.fk.th[t] = x;
        op.x[e] = x;
        op.pb[e] = x;
        op.v[e] = 0.0;
    }
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt(cv, t);
    __syncthreads();
    const double c = eval_block<EV_COST, HPE_NT>(sm, o, cv, H, nullptr, pre);
    if (t == 0) op.pc[i] = c;
    if (arrive_last_sharded(op.ctr, (unsigned)op.P, &flag)) opt_update_gbest(op, sm, false, 0, true);
