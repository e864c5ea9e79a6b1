// hpe_final_body.inc -- the body of k_pso_final, included as text by k_pso_final and by its
// batched form k_pso_final_b (hpe_kernels.hip), so both compile the same statements.  Names it
// expects in scope: TAIL, FILT (compile-time), sw, out, og, Hg, obs_out, same_eval, seq_dev,
// done_host, hist, fail, seq_table, seq_obs, seq_cur (k_pso_final's parameters).
    constexpr int CH = 2048;  // generations staged per pass
    // offline sequences (hpe_track_sequence_dev): the frame's history row and slot come
    // from the device cursor {slot, row}, and the next frame's descriptor is staged into the
    // descriptor every kernel of the chunk graph reads -- the graph is independent of the
    // slot range it tracks
    int seq_slot = 0;
    if (TAIL && seq_cur) {
        seq_slot = seq_cur[0];
        if (hist) hist += (size_t)(HPE_DOF + 1) * seq_cur[1];
    }
    // a timed-out multi-workgroup refine (DevMw::err, set until the host has reported it):
    // this frame's result is undefined, so bestp and cost become NaN
    const int failed = __builtin_amdgcn_readfirstlane(
        (TAIL && fail) ? __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
    __shared__ Smem sm;
    __shared__ double gm[CH];
    __shared__ int tp[CH];
    const int t = threadIdx.x, G = sw.G, P = sw.P;
    if (TAIL && seq_dev && t == HPE_NT - 64) {
        // pipelined tracking: this frame's refine launch (and the preparation of the next
        // frame inside it, which read a pinned host buffer) has completed; publish the
        // frame's sequence number to the host, which polls it before reusing that buffer.
        // Relaxed: the kernel boundary already retired those reads, and no store of this
        // kernel needs publishing with it.  Wave 7, idle until the first barrier, takes the
        // counter's load round trip instead of wave 0, which reads the gmin history.
        const unsigned long long n = *seq_dev + 1;
        *seq_dev = n;
        __hip_atomic_store(done_host, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (TAIL) stage_hand<HPE_NT>(sm.hand, Hg);
    // this frame's descriptor, read before the tail stages the next frame's into it (og IS
    // seq_obs in sequence mode, ADVICE r4).  (A round-5 form staged the next descriptor after
    // the tail's own evaluation, behind a barrier, and returned early before it on `failed`
    // (a per-lane atomic load) and `same_eval && last >= 0` (`last` read from LDS): exits the
    // compiler could not prove uniform, ahead of barriers -- undefined behaviour in the HIP
    // barrier model, not a proven compiler bug.  On the box its same-eval frames came out
    // with a re-evaluated cost (3.3e-7 relative off).  The cause was not isolated further;
    // every such exit is now made provably uniform (readfirstlane, DESIGN.md §7).)
    DevObs o_early{};
    if (TAIL) o_early = *og;
    // the frame descriptor handed back at the end, loaded now (off the final chain)
    const unsigned long long obs_word =
        (TAIL && obs_out && t < (int)(sizeof(DevObs) / 8)) ? ((const unsigned long long *)og)[t] : 0ull;
    double bp = 0.0;  // gbest_pos = zeros<vec> (PSO.cpp:739) if nothing beat 1e100
    double gcost = 1e100;
    int last = -1, count = 100;
    if (G <= 63) {
        // G + 1 <= 64 generations: the replay as scans over wave 0's lanes (lane k =
        // generation k), not a serial loop.  Costs are >= 0 or NaN, so their u64 bits
        // order like their values and NaN bits (never written, or all NaN) sort above
        // every cost: a u64 minimum is fmin, and "fm < gcost" is a u64 compare.
        if (t < 64) {
            unsigned long long key = ~0ull;
            if (t <= G) {
                double m = __builtin_nan("");
                for (int c = 0; c < GMIN_SHARDS; ++c) m = fmin(m, bits_to_f64(*gmin_cell(sw, t, c)));
                key = f64_to_bits(m);
            }
            const int topo = (t >= 1 && t <= G) ? sw.sig[t].topo : -1;
            const unsigned long long cap = f64_to_bits(1e100);  // gbest starts at 1e100
            const unsigned long long incl = wave_prefix_min_u64(key);
            const unsigned long long excl = min(from_left_u64(incl, ~0ull), cap);
            const bool imp = t >= 1 && t <= G && key < excl;  // PSO.cpp:864-872
            const unsigned long long mask = __ballot(imp);
            const int last0 = (readlane_u64(key, 0) < cap) ? 0 : -1;  // generation 0 (:755-760)
            last = mask ? 63 - __builtin_clzll(mask) : last0;
            if (t >= 1 && t <= G && sw.trace_g) {
                // count after generation t: 0 at an improvement, +1 otherwise, from 100
                const unsigned long long upto = mask & ((2ull << t) - 1);
                const int L = upto ? 63 - __builtin_clzll(upto) : 0;
                sw.trace_g[t - 1] = bits_to_f64(min(incl, cap));
                sw.trace_count[t - 1] = L >= 1 ? t - L : 100 + t;
                sw.trace_topo[t - 1] = topo;
            }
            if (t == 0) {
                sm.iscal[2] = last;
                sm.dscal[5] = bits_to_f64(min(readlane_u64(incl, G), cap));
            }
        }
    }
    for (int base = 0; G > 63 && base <= G; base += CH) {
        // all loads of the pass at once, then a serial replay from LDS by thread 0
        for (int k = t; k < CH && base + k <= G; k += HPE_NT) {
            double m = __builtin_nan("");  // all-ones (never written) is a NaN too
            for (int c = 0; c < GMIN_SHARDS; ++c)
                m = fmin(m, bits_to_f64(*gmin_cell(sw, base + k, c)));
            gm[k] = m;
            tp[k] = (base + k >= 1) ? sw.sig[base + k].topo : -1;
        }
        __syncthreads();
        if (t == 0) {
            const int n = (G - base + 1) < CH ? (G - base + 1) : CH;
            for (int k = 0; k < n; ++k) {
                const int g = base + k;
                const double fm = gm[k];
                if (g == 0) {
                    if (fm < gcost) {
                        gcost = fm;
                        last = 0;
                    }
                    continue;
                }
                if (fm < gcost) {
                    gcost = fm;
                    count = 0;
                    last = g;
                } else {
                    count += 1;
                }
                if (sw.trace_g) {
                    sw.trace_g[g - 1] = gcost;
                    sw.trace_count[g - 1] = count;
                    sw.trace_topo[g - 1] = tp[k];
                }
            }
        }
        __syncthreads();
    }
    if (G > 63 && t == 0) {
        sm.iscal[2] = last;
        sm.dscal[5] = gcost;
    }
    __syncthreads();
    last = __builtin_amdgcn_readfirstlane(sm.iscal[2]);  // decides the exit below (§7)
    gcost = sm.dscal[5];
    if (last >= 0 && P <= HPE_NT) {
        // one particle per thread: its pbest cost and its position row of generation
        // `last` in one round trip; the winner's thread writes bestp
        const int k = t < P ? t : P - 1;
        const double *row = sw.xh + ((size_t)last * P + k) * HPE_DOF;
        double r[HPE_DOF];
#pragma unroll
        for (int d = 0; d < HPE_DOF; ++d) r[d] = row[d];
        VI mine = {t < P ? nan_inf(sw.pch[(size_t)last * P + k]) : __builtin_inf(), t < P ? t : 0};
        const VI b = block_argmin(sm, mine);
        if (t == b.i) {
#pragma unroll
            for (int d = 0; d < HPE_DOF; ++d) {
                out[d] = r[d];
                sw.gpos[d] = r[d];
                if (hist) hist[d] = r[d];
            }
        }
        if (TAIL && !same_eval) {  // the tail below evaluates cal_cost(bestp)
            if (t == b.i) {
#pragma unroll
                for (int d = 0; d < HPE_DOF; ++d) sm.pbr[d] = r[d];
            }
            __syncthreads();
            if (t < HPE_DOF) bp = sm.pbr[t];
        }
    } else {
        if (last >= 0) {
            const double *pc = sw.pch + (size_t)last * P;
            VI mine = {__builtin_inf(), 0};
            for (int k = t; k < P; k += HPE_NT) {
                const double v = nan_inf(pc[k]);
                if (v < mine.v) {
                    mine.v = v;
                    mine.i = k;
                }
            }
            const VI b = block_argmin(sm, mine);
            if (t < HPE_DOF) bp = sw.xh[((size_t)last * P + b.i) * HPE_DOF + t];
        }
        // bestp stays in each thread's register: no barrier and no re-read of `out`
        if (t < HPE_DOF) {
            out[t] = bp;
            sw.gpos[t] = bp;
            if (hist) hist[t] = bp;
        }
    }
    if (t == 0) {
        out[HPE_DOF] = gcost;
        if (hist) hist[HPE_DOF] = gcost;
    }
    for (int c = t; c < (G + 1) * GMIN_SHARDS; c += HPE_NT) sw.gmin[(size_t)c * GMIN_STRIDE] = ~0ull;
    if (TAIL) {
        if (obs_out && t < (int)(sizeof(DevObs) / 8)) ((unsigned long long *)obs_out)[t] = obs_word;
        if (seq_cur) {
            const int nx = seq_slot + 1 < HPE_MAX_SLOTS ? seq_slot + 1 : seq_slot;
            if (seq_table && t < (int)(sizeof(DevObs) / 8))
                ((unsigned long long *)seq_obs)[t] = ((const unsigned long long *)(seq_table + nx))[t];
            if (t == 0) {
                seq_cur[0] = seq_slot + 1;
                seq_cur[1] = seq_cur[1] + 1;
            }
        }
        if (failed) {
            if (t <= HPE_DOF) {
                out[t] = __builtin_nan("");
                if (hist) hist[t] = __builtin_nan("");
            }
            return;
        }
        if (same_eval && last >= 0) return;  // out[26] = gcost = cal_cost(bestp)
        const DevObs o = o_early;
        if (t < HPE_DOF) sm.fk.th[t] = bp;
        const CloudGlobal cv = obs_cloud(o);
        const Pt pre = load_pt(cv, t);
        __syncthreads();
        const double c = eval_block<EV_COST, HPE_NT, true, FILT>(sm, o, cv, &sm.hand, nullptr, pre);
        if (t == 0) {
            out[HPE_DOF] = c;
            if (hist) hist[HPE_DOF] = c;
        }
    }
