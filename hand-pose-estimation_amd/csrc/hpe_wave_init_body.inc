// hpe_wave_init_body.inc -- the body of k_pso_init_w, included as text by k_pso_init_w and by
// its batched form k_pso_init_wb (hpe_kernels.hip), so both compile the same statements.  Names
// it expects in scope: WPP, COOP (compile-time), sw, x0, og, Hg.  The particle index comes from
// blockIdx.x alone: a batched launch keeps its lane in blockIdx.y.
    const DevObs o = *og;
    __shared__ DevHand hs;
    __shared__ FkSm fks[PW_WPB];
    __shared__ FiltSm fls[PW_WPB];
    __shared__ double xpart[PW_WPB];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, sub = w % WPP;
    const int i = blockIdx.x * (PW_WPB / WPP) + w / WPP, P = sw.P;
    const bool valid = i < P;
    const int ic = valid ? i : P - 1;
    const double hw = hand_word<PW_NT>(Hg);
    const DevHand *__restrict__ H = &hs;
    FkSm &f = fks[w];
    Link lk[3];
    push_lane_links(sw, 0, ic, l, 1, -1, lk);
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt1(cv, l + 64 * sub);
    const double *sd = sw.bounds + 2 * HPE_DOF;
    if (sw.ext && blockIdx.x == 0 && t == 0) sw.ext[HPE_DOF] = __builtin_inf();  // no candidate yet
    if (l < HPE_DOF) {  // particles = x0 + randn % std (PSO.cpp:67-72)
        const size_t e = (size_t)ic * HPE_DOF + l;
        const double x = x0[l] + sw.normals[e] * sd[l];
        f.th[l] = x;
        if (valid && sub == 0) {
            sw.xh[e] = x;
            sw.pb[e] = x;
            sw.v[e] = 0.0;
        }
    }
    hand_put<PW_NT>(hs, hw);
    __syncthreads();  // hand staged
    const double c = eval_wave_cost<WPP, COOP, PW_WPB>(fks, fls[w], o, cv, H, pre, sub, xpart);
    if (!valid || sub != 0) return;
    if (l == 0) {
        sw.pch[i] = c;
        gmin_lower(sw, 0, i, c);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) push_inbox_w(sw, 0, i, l + 64 * k, lk[k], 1, c, f.th);
