// hpe_refine_body.inc -- the body of k_refine, included as text by k_refine and by its batched
// form k_refine_lane (hpe_kernels.hip), so both compile the same statements.  Names it expects in
// scope: STAGED, MW, RIGID (compile-time), x0g, og, Hg, match_g, evals_out, do_refine, pa, mw,
// pk, ps (k_refine's parameters), and WIN (compile-time) with pw, the window the preparation
// workgroups read the next frame through (the batch calls' windowed kernels; elsewhere false
// and an unread DevWindow); SPEC, RUNNER (compile-time) with sp, the speculated translation
// block's words and ssm_p, its workgroup's SpecSm in LDS (hpe_kernels.hip; elsewhere false, an
// unread DevSpec and a null pointer): k_refine<..., SPEC>
// compiles the body twice, once as the runner's (RUNNER: workgroup 1) and once as everyone
// else's, so neither role carries the other's registers or branches in its loops.  There the
// body runs inside a lambda (its returns end the workgroup) and the kernel declares the shared
// variables once (HPE_REFINE_BODY_NO_DECLS).  Every statement of the speculated form sits
// behind `if constexpr`: without SPEC the body is the one-workgroup form's, statement for
// statement.
#ifndef HPE_REFINE_BODY_NO_DECLS
    extern __shared__ __align__(16) unsigned char dyn[];  // staged cloud + matchId / prep
#endif
    const int nhelp = MW ? mw.Q : SPEC ? 1 : 0;  // workgroups between the leader and preparation
    constexpr bool runner = SPEC && RUNNER;  // runs the translation block ahead of the leader
    if (MW && blockIdx.x >= 1 && (int)blockIdx.x <= nhelp) {
        if (do_refine) mw_helper<RIGID>(mw, blockIdx.x - 1, og, Hg, match_g);
        return;
    }
    if (blockIdx.x >= 1 && !runner) {
        const unsigned long long t0 = HPE_STAMPS ? __builtin_amdgcn_s_memtime() : 0;
        prep_workgroup<WIN>(pa, blockIdx.x - 1 - nhelp, dyn, &ps, &pw);
        if (HPE_STAMPS && threadIdx.x == 0) {  // diagnostic build: prep workgroup spans
            const int k = ((int)blockIdx.x - 1 - nhelp < PREP_BANDS) ? 24 : 25;
            atomicAdd(&hpe_stamps[k], __builtin_amdgcn_s_memtime() - t0);
            atomicAdd(&hpe_stamps[32 + k], 1ull);
        }
        return;
    }
    if (!do_refine) return;
    // the speculated form: this launch's epoch (each workgroup counts the launches it finished)
    unsigned sp_ep = 0;
    if constexpr (SPEC)
        sp_ep = (__hip_atomic_load(sp.epoch + (runner ? 32 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u) &
                SPEC_EP_MASK;
    const DevObs o = *og;  // the selected frame (device-resident: graph-stable args)
#ifndef HPE_REFINE_BODY_NO_DECLS
    __shared__ RefineSm rs;
    __shared__ DevHand hs;  // hand constants in LDS: keeps them out of the loop's registers
#endif
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    stage_hand<RF_NT>(hs, Hg);
    const DevHand *__restrict__ H = &hs;
    using CV = std::conditional_t<STAGED, CloudView, CloudGlobal>;
    CV cv;
    int32_t *match = match_g;
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
    // the speculated form's leader: the messages sent; runner: the message it works on
    [[maybe_unused]] int sp_seq = 0;
    if constexpr (runner) {
        // x0 comes with the first message (the exchange pick stays with the leader); none: the
        // leader is already past its rotation block, or never ran
        sp_seq = spec_wait(sp, *ssm_p, sp_ep, 0, false);
        if (sp_seq <= 0) {
            if (t == 0)
                __hip_atomic_store(sp.epoch + 32, sp_ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        spec_take_x0(*ssm_p, rs.x0);
    } else if (pk.gath) {
        // the previous frame's subswarm exchange: x0 = the best all-gathered state (k_pick_best's
        // rule), also stored to d_state and the previous frame's history row
        if (w == 0) {
            const double x = pick_apply(pk.gath, pick_best_row(pk.gath, pk.world, l), l, x0g,
                                        pk.hist, pk.cur);
            if (l < HPE_DOF) rs.x0[l] = x;
        }
    } else if (t < HPE_DOF) {
        rs.x0[t] = x0g[t];
    }
    if (t == 0) rs.ts_n = 0;
    REF_TS(rs.ts_n, 0);
#ifndef HPE_REFINE_BODY_NO_DECLS
    __shared__ int mwflag;
#endif
    MwLeader ml{mw, 0u, false};
    __syncthreads();
    if (RIGID) {  // (runner: from the first message -- x0's digits never change in a call)
        // hand-frame centres q (x0's digits, theta0 = -180, theta1..5 = 0: Tgb = I, u = 0)
        // and the call's constant self-collision penalty
        if (w == 0) {
            const double xl = rs.x0[l < HPE_DOF ? l : 0];
            const double thq = (l == 0) ? -180.0 : (l < 6) ? 0.0 : xl;
            if (l < HPE_DOF) rs.w[0].th[l] = thq;
            wave_sync();
            SphXYZ own;
            fk_wave<true>(rs.w[0], H, &own, &thq);
            if (l < HPE_NS) {
                rs.rg.q[l][0] = own.x;
                rs.rg.q[l][1] = own.y * -1;
                rs.rg.q[l][2] = own.z * -1;
            }
            CollPair cp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = collide_load(rs.w[0], k < 2 ? l + 64 * k : ((l < 16) ? l + 128 : l), H);
            double co = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double v = collide_value(cp[k], sqrt(collide_d2(cp[k])));
                co += (k < 2 || l < 16) ? v : 0.0;
            }
            co = wave_sum(co);
            if (l == 0) rs.rg.C = co;
        }
        __syncthreads();
    }
    StampClock sc;
    sc.start();
    int evals = 0;
    bool base_valid = false;
    const double e = 1e-5;  // cal_grad step (PSO.cpp:195)
    // clouds of at most FP_MAX points: each lane keeps its frozen points in registers
    const bool small = !MW && STAGED && o.n >= 1 && o.n <= FP_MAX;  // (N = 0: no point to clamp to)
    FrozenPts fpts;
    // the lane's sphere (lane l, clamped) off-image depth value, the same for every
    // evaluation of the call (depth_finish's md * md, computed once)
    const double md2_l = depth_off_sq(o, H->radii[l < HPE_NS ? l : HPE_NS - 1]);
    [[maybe_unused]] int verdict = 0;  // runner: the leader's word that ended a speculation early
    [[maybe_unused]] SpecPoll spoll{};
spec_again:  // the runner comes back here with every newer x0
    __attribute__((unused));
    if constexpr (runner) spoll = SpecPoll{sp, ssm_p, sp_ep, sp_seq};
    for (int blk = runner ? 1 : 0; blk < 2; ++blk) {
        const int lo = 3 * blk;  // start_idx (PSO.cpp:226-227); end_idx = lo + 2
        // Block 2 moves only the global position u = x0[3..5]: every FK of the block is
        // the stored rotation terms of x0 plus u (FK_TRANSLATE, bit-identical).
        FkX *Xt = nullptr;
        if (RIGID && blk == 1) {  // P = Rg q of the block's fixed rotation
            if (w == 0) rigid_wave<RG_STORE_P>(rs.w[0], rs.rg, rs.x0[l < HPE_DOF ? l : 0], nullptr, rs.rg.P);
            __syncthreads();
        } else if (blk == 1) {
            if (w == 0) {
                if (l < HPE_DOF) rs.w[0].th[l] = rs.x0[l];
                wave_sync();
                fk_wave_t<FK_STORE_X, true>(rs.w[0], H, &rs.X);
            }
            __syncthreads();
            Xt = &rs.X;
        }
        double tol = 1;
        int cnt = 0, iter = 0;
        while (tol > 1e-6 && iter < 15 && cnt < 1 && !(MW && ml.failed)) {
            if constexpr (SPEC && !runner) if (blk == 0) {
                // this search's x0 to the runner (stores only): should the search fail, the
                // translation block is already under way from the pose it leaves
                sp_seq += 1;
                if (w == SPEC_PW) spec_send(sp, (sp_ep << 5) | (unsigned)sp_seq, rs.x0);
            }
            // f_k = cal_cost2(x0, matchId, true).  The spheres of x0 are already in rs.base
            // when x0 is the accepted Goldstein point of the previous iteration
            // (x0 + tk*p == x0 - tk*g bitwise) or an unchanged x0.
            if (!base_valid) {
                if (t < HPE_DOF) rs.base.th[t] = rs.x0[t];
                __syncthreads();
                if (w == 0) {
                    if (RIGID) {
                        const double thl = rs.x0[l < HPE_DOF ? l : 0];
                        if (blk) rigid_wave<RG_TRANS>(rs.base, rs.rg, thl);
                        else rigid_wave<RG_ROT>(rs.base, rs.rg, thl);
                    } else if (Xt) {
                        fk_wave_t<FK_TRANSLATE>(rs.base, H, Xt);
                    } else {
                        fk_wave<true>(rs.base, H);
                    }
                }
                __syncthreads();
            }
            REF_TS(rs.ts_n, 1);
            double fk;
            if (MW) {
                fk = eval_corr<MW, RIGID>(rs, o, cv, H, match, &ml, &mwflag);
                REF_TS(rs.ts_n, 2);
                // cal_grad: x0 +/- e along the 3 block dims, one wave per evaluation
                if (w < 6) {
                    const int d = lo + (w >> 1);
                    if (l < HPE_DOF)
                        rs.w[w].th[l] = (l == d) ? ((w & 1) ? rs.x0[l] - e : rs.x0[l] + e) : rs.x0[l];
                }
                eval_nodes<MW, RIGID>(rs, 6, o, cv, H, match, Xt, &ml, &mwflag, nullptr, nullptr, blk);
            } else {
                // f_k = cal_cost2(x0, matchId, true) and cal_grad's six frozen evaluations
                // (x0 +/- e along the 3 block dims, one wave each) with one barrier between
                // them: the search stores matchId, and while the slowest search waves and the
                // corr sums finish, waves 0..5 already run the parts of their gradient point
                // that need no matchId (FK, depth gathers, collision)
                FrozenHead hd{};
                auto head = [&]() {
                    if (w < 6) {
                        const int d = lo + (w >> 1);
                        const double xl = rs.x0[l < HPE_DOF ? l : 0];
                        const double thl = (l == d) ? ((w & 1) ? xl - e : xl + e) : xl;
                        if (l < HPE_DOF) rs.w[w].th[l] = thl;
                        wave_sync();
                        if (RIGID) hd = blk ? rigid_head<RG_TRANS>(rs.w[w], o, H, rs.rg, thl)
                                            : rigid_head<RG_ROT>(rs.w[w], o, H, rs.rg, thl);
                        else hd = frozen_head<true>(rs.w[w], o, H, Xt, &thl);
                    }
                };
                const DepthG dgc = depth_issue_w0(rs.base, o, H);
                const bool young = w >= HPE_SETPRIO_FROM;  // as in eval_block
                if (young) __builtin_amdgcn_s_setprio(1);
                // (n <= 256) the items go where the SIMDs have room.  Chain form: waves 0..5
                // also run a gradient point's head below (FK), two of them on SIMDs 0 and 1
                // each, one on SIMDs 2 and 3; so waves 4, 5 search nothing and waves 6, 7 two
                // items.  Hand-frame form (HPE_RF_SPREAD): the heads are short (no DH chain),
                // so every wave takes one item and no wave searches twice.
                double al;
                if (small) {
                    const bool spread = RIGID && HPE_RF_SPREAD;
                    const int f0 = (w < 4 || spread) ? 64 * w : (w >= 6) ? 256 + 128 * (w - 6) : 0;
                    const int cnt = (w < 4 || spread) ? 1 : (w >= 6) ? 2 : 0;
                    al = search_align<RF_NT, true>(rs.base, cv, H, match, load_pt(cv, f0 + l),
                                                   f0 + l, BT_GENS, 64, cnt);
                } else {
                    al = search_align<RF_NT, true>(rs.base, cv, H, match, load_pt(cv, t));
                }
                if (young) __builtin_amdgcn_s_setprio(0);
                double co = (!RIGID && t < 144) ? collide_term(rs.base, t, H) : 0.0;
                const double dep = depth_finish(dgc, o, t < HPE_NS);
                const double tot = wave_sum((al * o.lambda + dep) + co);  // as block_sum1
                if (l == 0) rs.red[w][0] = tot;
                // runner: the polling wave has no gradient point; its load returns meanwhile
                [[maybe_unused]] unsigned long long pg = 0;
                if constexpr (runner) if (w == SPEC_PW) pg = spec_poll_issue(sp);
                head();
                __syncthreads();  // matchId complete, the corr partial sums in red
                if (small) load_frozen_pts(fpts, cv, match, l);
                fk = 0;
#pragma unroll
                for (int k = 0; k < RF_NW; ++k) fk += rs.red[k][0];
                if (RIGID) fk = fk + rs.rg.C;
                REF_TS(rs.ts_n, 2);
                if (w < 6) {
                    double f = RIGID ? frozen_tail<true>(rs.w[w], o, cv, H, match, hd,
                                                         small ? &fpts : nullptr, &md2_l)
                                     : frozen_tail(rs.w[w], o, cv, H, match, hd, small ? &fpts : nullptr);
                    if (RIGID) f = f + rs.rg.C;
                    if (l == 0) rs.fg[w] = f;
                }
                if constexpr (runner) if (w == SPEC_PW) spec_poll_take(*ssm_p, pg, sp_ep, sp_seq);
                __syncthreads();
                if constexpr (runner) {
                    verdict = __builtin_amdgcn_readfirstlane(ssm_p->verdict);  // decides exits (§7)
                    if (verdict != 0) break;
                }
            }
            ++evals;
            sc.lap(20);
            evals += 6;
            // cal_grad (PSO.cpp:197-212): g on the block dims, p = -1 * g, computed by every
            // thread for its lane -- no barrier: fg is rewritten only by the next iteration's
            // gradient points (the multi-workgroup form's rs.f by this search's first round,
            // hence its barrier)
            const double *fg = MW ? rs.f : rs.fg;
            const double g0 = (fg[0] - fg[1]) / (2 * e), g1 = (fg[2] - fg[3]) / (2 * e),
                         g2 = (fg[4] - fg[5]) / (2 * e);
            const int dl = l - lo;
            const double gl = (dl == 0) ? g0 : (dl == 1) ? g1 : (dl == 2) ? g2 : 0.0;
            const double pl = -1 * gl;
            if (MW) __syncthreads();
            REF_TS(rs.ts_n, 3);
            sc.lap(21);
            // g'p by op_dot::direct_dot_arma (two accumulators: even / odd indices).  g is
            // zero outside the block, and a zero term leaves an accumulator unchanged
            // (x + -0 = x; the empty sums stay zero), so the sums reduce to the block's
            // terms in the same order: block 0 (dims 0..2) v1 = g0 p0 + g2 p2, v2 = g1 p1;
            // block 1 (dims 3..5) v1 = g4 p4, v2 = g3 p3 + g5 p5.  Same for |g|^2 (tol).
            const double q0 = g0 * (-1 * g0), q1 = g1 * (-1 * g1), q2 = g2 * (-1 * g2);
            const double s0 = g0 * g0, s1 = g1 * g1, s2 = g2 * g2;
            const double gp = (blk == 0) ? (q0 + q2) + q1 : q1 + (q0 + q2);
            // goldstein(x0, grad, matchId, f_k, optfunc, tk, 30)
            // goldstein(x0, grad, matchId, f_k, optfunc, tk, 30), then x0 = x0 - tk*grad
            const double tk = gold_tree<MW, HPE_GOLD_POLICY, true, RIGID, runner>(
                rs, o, cv, H, match, fk, gp, pl, gl, evals, nullptr, Xt, &ml, &mwflag,
                small ? &fpts : nullptr, blk, &md2_l, &spoll, &verdict);
            if constexpr (runner) if (verdict != 0) break;  // (uniform: gold_tree's readfirstlane)
            sc.lap(22);
            if (tk == 0) cnt += 1;
            // tol = sqrt(sum(grad % grad)): arrayops::accumulate (two accumulators)
            tol = uniform_f64(sqrt((blk == 0) ? (s0 + s2) + s1 : s1 + (s0 + s2)));
            iter += 1;
            // gold_tree's last barrier published x0 and the accepted node's spheres
            base_valid = true;  // accepted node copied, or tk == 0 and x0 unchanged
            REF_TS(rs.ts_n, 5);
            sc.lap(23);
        }
        if constexpr (SPEC && !runner) if (blk == 0) {
            // the rotation block is over.  Its last search failed (cnt): x0 is the pose the
            // runner got with that search's message, so its translation block is this one's
            REF_TS(rs.ts_n, 6);
            if (w == 0) {
                const bool ok = spec_commit(sp, *ssm_p, (sp_ep << 5) | (unsigned)sp_seq, cnt >= 1);
                if (l == 0) ssm_p->verdict = ok ? 1 : 0;
            }
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane(ssm_p->verdict)) {  // decides the block below (§7)
                if (t < 3) rs.x0[3 + t] = ssm_p->res[t];
                evals += __builtin_amdgcn_readfirstlane(ssm_p->evals);
                __syncthreads();
                break;
            }
        }
    }
    if constexpr (runner) {
        // a finished block waits for the leader's word; a dropped one has it already
        if (verdict == 0) verdict = spec_wait(sp, *ssm_p, sp_ep, sp_seq, true);
        if (verdict > 0) {  // a newer x0: start over from it
            __syncthreads();
            spec_take_x0(*ssm_p, rs.x0);
            sp_seq = verdict;
            verdict = 0;
            evals = 0;
            base_valid = false;
            goto spec_again;
        }
        if (verdict == 0 && w == 0)  // committed: hand the block back
            spec_result(sp, (sp_ep << 5) | (unsigned)sp_seq, rs.x0, evals);
    }
    if constexpr (SPEC) {  // this workgroup's launch is over (visible at the kernel's end)
        if (t == 0)
            __hip_atomic_store(sp.epoch + (runner ? 32 : 0), sp_ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (runner) return;  // the leader alone writes the call's outputs
    if (MW) mw_publish(ml, rs, MW_JOB_EXIT, 0);
    REF_TS(rs.ts_n, 7);
    // a timed-out multi-workgroup refine has no defined result: the pose becomes NaN, so
    // this frame's PSO (and its cost) is NaN and never wins an exchange
    if (t < HPE_DOF) x0g[t] = (MW && ml.failed) ? __builtin_nan("") : rs.x0[t];
    if (t == 0 && evals_out) {
        *evals_out = evals;
        atomicAdd((unsigned long long *)(evals_out + 2), (unsigned long long)evals);  // running total
    }
