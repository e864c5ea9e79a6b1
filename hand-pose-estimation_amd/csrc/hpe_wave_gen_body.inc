// hpe_wave_gen_body.inc -- the body of k_pso_gen_w, included as text by k_pso_gen_w and by its
// batched form k_pso_gen_wb (hpe_kernels.hip), so both compile the same statements.  Names it
// expects in scope: XCH, ROW16, WPP, COOP (compile-time), sw, og, Hg, g, W1, C1, C2.  The
// particle index comes from blockIdx.x alone: a batched launch keeps its lane in blockIdx.y.
    // every argument word loaded at entry in one batch (see k_pso_gen)
    int z0 = 0;
    asm("" : "+s"(z0) : "s"(g), "s"(sw.gmin), "s"(sw.sig), "s"(sw.outl), "s"(sw.bounds),
        "s"(sw.xh), "s"(sw.pch), "s"(sw.pb), "s"(sw.v), "s"(sw.inbox), "s"(sw.ibtc),
        "s"(sw.P), "s"(sw.K));
    const DevObs o = *og;
    WAVE_TS2(g, 0);
    __shared__ DevHand hs;
    __shared__ FkSm fks[PW_WPB];
    __shared__ FiltSm fls[PW_WPB];
    __shared__ double xpart[PW_WPB];
    const int t = threadIdx.x + z0, w = t >> 6, l = t & 63, sub = w % WPP;
    const int i = blockIdx.x * (PW_WPB / WPP) + w / WPP, P = sw.P, K = sw.K;
    const bool valid = i < P;
    const int ic = valid ? i : P - 1;
    const double hw = hand_word<PW_NT>(Hg);  // staged into LDS before the block barrier
    const DevHand *__restrict__ H = &hs;
    FkSm &f = fks[w];
    // a helper wave (WPP > 1, cooperative FK): its particle's FK and state are the first
    // wave's, so it only stages its share of the hand, takes part in the FK and searches its
    // share of the cloud (the same barriers as the first wave's path).  At two waves per
    // particle the second wave then pushes the particle's pbest while the first writes it,
    // the push links loaded under the evaluation from the topology the first wave leaves in
    // LDS with the entry pbest row and cost (1,024 p: 11.0 -> 10.7 us per generation)
    constexpr bool hpush = COOP && WPP == 2;
    __shared__ double hrow[hpush ? PW_WPB : 1][HPE_DOF];
    __shared__ double hpc[hpush ? PW_WPB : 1];
    __shared__ int htopo[hpush ? PW_WPB : 1];
    if (COOP && WPP > 1 && __builtin_amdgcn_readfirstlane(sub) != 0) {
        const CloudGlobal cv = obs_cloud(o);
        const Pt pre = load_pt1(cv, l + 64 * sub);
        hand_put<PW_NT>(hs, hw);
        __syncthreads();
        Link lk[3];
        const int w0 = w - sub, tp = hpush ? htopo[hpush ? w0 : 0] : 0;
        if (hpush && sub == 1) push_lane_links(sw, g, ic, l, g + 1, tp, lk);
        const double fx = eval_wave_cost<WPP, COOP, PW_WPB>(fks, fls[w], o, cv, H, pre, sub, xpart, g);
        if constexpr (hpush) {
            if (!valid || sub != 1) return;
            const double pci = hpc[w0];
            const bool better = fx < pci;
            const double pn = better ? fx : pci;
            const double *row = better ? fks[w0].th : hrow[w0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int q = l + 64 * k;
                push_inbox_w(sw, g, i, q, lk[k], q < 3 * IB_FIELDS ? g + 1 : tp, pn, row);
            }
        }
        return;
    }
    // ---- round 1: every load of the generation, all independent and unconditional (the
    // push links follow once the topology is known)
    const CloudGlobal cv = obs_cloud(o);
    const size_t e = (size_t)ic * HPE_DOF + l;
    const size_t ec = (size_t)ic * HPE_DOF + (l < HPE_DOF ? l : HPE_DOF - 1);
    const double xo = sw.xh[(size_t)(g - 1) * P * HPE_DOF + ec];
    const double vo = sw.v[ec];
    const double pbi = sw.pb[ec];
    const double lbt = sw.bounds[ec - (size_t)ic * HPE_DOF];
    const double ubt = sw.bounds[ec - (size_t)ic * HPE_DOF + HPE_DOF];
    const double pci = sw.pch[(size_t)(g - 1) * P + ic];
    double tg[2], tc[2];
#pragma unroll
    for (int vr = 0; vr < 2; ++vr) {  // {tag, cost} of slot l: one 16-B load, contiguous run
        typedef double d2v __attribute__((ext_vector_type(2)));
        const d2v e = *(const d2v *)(sw.ibtc + 2 * ibtc_index(sw, (g - 1) & 1, vr, ic, l < K ? l : K - 1));
        tg[vr] = e.x;
        tc[vr] = e.y;
    }
    const unsigned long long gcell = gmin_load(sw, g - 1);
    const Sig pv = sw.sig[g > 1 ? g - 1 : 0];
    const double exr = XCH ? sw.ext[l <= HPE_DOF ? l : HPE_DOF] : 0.0;  // exchange (sw.ext)
    // the draws while the loads are in flight
    // one Philox pass for both draws: lanes 0..25 draw rp of dimension l, lanes 26..51 rg of
    // dimension l - 26, which one shuffle brings to lane l - 26
    const int dl = l < HPE_DOF ? l : (l < 2 * HPE_DOF ? l - HPE_DOF : 0);
    const double rd = philox_u01(sw.seed, l < HPE_DOF ? ST_RP : ST_RG, g, ic, dl);
    const double rp = rd;
    const double rg = __shfl(rd, l + HPE_DOF);
    const double fmin = gmin_reduce(gcell);
    // ---- end-of-generation update of g-1 (PSO.cpp:864-877), uniform
    Sig sg;
    if (g == 1) {
        sg.gcost = fmin < 1e100 ? fmin : 1e100;
        sg.count = 100;
        sg.topo = -1;
    } else {
        const bool imp = fmin < pv.gcost;
        sg.gcost = imp ? fmin : pv.gcost;
        sg.count = imp ? 0 : pv.count + 1;
        sg.topo = pv.topo;
    }
    if (sg.count > 0) sg.topo = g;
    if (i == 0 && l == 0 && sub == 0) sw.sig[g] = sg;
    const int topo = sg.topo, var = (topo == g) ? 1 : 0;
    // ---- informant (PSO.cpp:810-812)
    const int self_lane = ROW16 ? 15 : 63;  // one 16-lane row when K <= 15
    double v = __builtin_inf();
    int idx = 0x7fffffff, slot = -1;
    if (l < K) {
        const long long tag = __double_as_longlong(var ? tg[1] : tg[0]);
        if ((tag >> 32) == (((long long)(g - 1) << 16) | topo)) {
            v = var ? tc[1] : tc[0];
            idx = (int)(tag & 0xffffffff);
            slot = l;
        }
    } else if (l == self_lane) {
        v = pci;
        idx = ic;
    }
    if (v != v) v = __builtin_inf();
    int inf, islot;
    double infc = 0.0;
    if (ROW16) row0_argmin_lex(v, idx, slot, inf, islot, XCH ? &infc : nullptr);
    else wave_argmin_lex(v, idx, slot, inf, islot, XCH ? &infc : nullptr);
    const bool use_ext = XCH && readlane_f64(exr, HPE_DOF) < infc;  // strictly better
    WAVE_TS2(g, 1);
    // the lane's first cloud point, used after FK: issued behind round 1's loads, which the
    // informant choice waits for in issue order
    const Pt pre = load_pt1(cv, l + 64 * sub);
    // ---- velocity, position, check_constraints (PSO.cpp:824-842, 358-377)
    if (l < HPE_DOF) {
        double vn;
        if (inf == ic && !use_ext) {
            vn = W1 * vo + (C1 * rp) * (pbi - xo);
        } else {
            const double pbn = use_ext ? exr : sw.inbox[ib_index(sw, (g - 1) & 1, var, ic, islot) + 2 + l];
            vn = (W1 * vo + (C1 * rp) * (pbi - xo)) + (C2 * rg) * (pbn - xo);
        }
        double xn = xo + vn;
        const double xr = xn;
        if (xr < lbt) { xn = lbt; vn = 0.; }
        if (xr > ubt) { xn = lbt; vn = 0.; }  // above max -> MIN (PSO.cpp:372)
        if (valid && sub == 0) {
            sw.v[e] = vn;
            sw.xh[(size_t)g * P * HPE_DOF + e] = xn;
        }
        f.th[l] = xn;
    }
    // the push links, loaded before the evaluation so their round trip hides under it (121 ->
    // 127 VGPRs: still four waves per SIMD)
    Link lk[3];
    if (!hpush) push_lane_links(sw, g, ic, l, g + 1, topo, lk);
    if constexpr (hpush) {  // for the pushing helper
        if (l < HPE_DOF) hrow[w][l] = pbi;
        if (l == 0) {
            hpc[w] = pci;
            htopo[w] = topo;
        }
    }
    hand_put<PW_NT>(hs, hw);
    WAVE_TS2(g, 2);
    __syncthreads();  // hand staged (the only block-wide sync)
    WAVE_TS2(g, 3);
    // ---- evaluation and pbest (PSO.cpp:848-861)
    const double fx = eval_wave_cost<WPP, COOP, PW_WPB>(fks, fls[w], o, cv, H, pre, sub, xpart, g);
    WAVE_TS2(g, 8);
    if (!valid || sub != 0) return;
    const bool better = fx < pci;
    const double pn = better ? fx : pci;
    if (l < HPE_DOF) {
        const double row = better ? f.th[l] : pbi;
        sw.pb[e] = row;
        if (!hpush) f.th[l] = row;
    }
    if (l == 0) {
        sw.pch[(size_t)g * P + i] = pn;
        gmin_lower(sw, g, i, pn);
    }
    if (hpush) return;  // the second wave pushes
    wave_sync();
    WAVE_TS2(g, 9);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int q = l + 64 * k;
        push_inbox_w(sw, g, i, q, lk[k], q < 3 * IB_FIELDS ? g + 1 : topo, pn, f.th);
    }
    WAVE_TS2(g, 10);
