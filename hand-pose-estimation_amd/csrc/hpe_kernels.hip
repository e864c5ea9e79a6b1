// hpe_kernels.hip -- gfx950 kernels of the PSO / costfunc / handmodel hot path.
//
//   k_build       handmodel::build_hand_model for a batch        (handmodel.cpp:259-298)
//   k_eval<MODE>  costfunc::cal_cost / cal_cost2 for a batch     (costfunc.cpp:31-127)
//   k_pso_init    generate_particles + initial evaluation        (PSO.cpp:56-74, 745-763)
//   k_pso_gen     one fused generation: gbest/count/topology of the previous
//                 generation, informant, velocity/position/clamp, evaluation,
//                 pbest update                                    (PSO.cpp:778-879)
//   k_pso_final   last gbest update, bestp                       (PSO.cpp:864-882)
//   k_refine      refine_init_pose as one persistent workgroup    (PSO.cpp:183-266, 438-480)
//   k_render      synthetic depth frames (bench/test input)
//
// One workgroup of HPE_NT threads per particle; see hpe_device.hpp for the block-level
// pieces and DESIGN.md for layout, rooflines and the parity argument.
#include <vector>

#include "hpe_device.hpp"
#include "hpe_prep.hpp"
#include "hpe_report.hpp"
#include "../../include/hpe.h"

// ------------------------------------------------------------------ batch kernels
__global__ __launch_bounds__(HPE_NT) void k_build(const double *__restrict__ theta, int P,
                                                  const DevHand *__restrict__ Hg,
                                                  double *__restrict__ S_out,
                                                  double *__restrict__ J_out) {
    __shared__ Smem sm;
    const int i = blockIdx.x, t = threadIdx.x;
    stage_hand<HPE_NT>(sm.hand, Hg);
    const DevHand *__restrict__ H = &sm.hand;
    if (t < HPE_DOF) sm.fk.th[t] = theta[(size_t)i * HPE_DOF + t];
    __syncthreads();
    if (t < 64) fk_wave(sm.fk, H);
    __syncthreads();
    if (t < 3 * HPE_NS) S_out[(size_t)i * 3 * HPE_NS + t] = (&sm.fk.S[0][0])[t];
    if (J_out && t < 63) {  // hand_joints rows: wrist, index..little joints 1-4, thumb 1-4
        double v;
        if (t < 3) v = sm.fk.th[3 + t];
        else {
            const int row = t / 3, c = t % 3, k = (row - 1) / 4, jr = 1 + (row - 1) % 4;
            const int d = (k < 4) ? k + 1 : 0;
            v = sm.fk.J[d][jr][c];
        }
        J_out[(size_t)i * 63 + t] = v;
    }
}

template <int MODE>
__global__ __launch_bounds__(HPE_NT) void k_eval(const double *__restrict__ theta, int P,
                                                 const DevObs *__restrict__ og, const DevHand *__restrict__ Hg,
                                                 double *__restrict__ cost,
                                                 int32_t *__restrict__ match,
                                                 double *__restrict__ terms) {
    const DevObs o = *og;  // the selected frame (device-resident: graph-stable args)
    __shared__ Smem sm;
    const int i = blockIdx.x, t = threadIdx.x;
    stage_hand<HPE_NT>(sm.hand, Hg);
    const DevHand *__restrict__ H = &sm.hand;
    if (t < HPE_DOF) sm.fk.th[t] = theta[(size_t)i * HPE_DOF + t];
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt(cv, t);
    __syncthreads();
    int32_t *m = match ? match + (size_t)i * o.n : nullptr;
    const double c = eval_block<MODE, HPE_NT>(sm, o, cv, H, m, pre);
    if (t == 0) {
        cost[i] = c;
        if (terms) {
            terms[3 * i + 0] = sm.dscal[0];
            terms[3 * i + 1] = sm.dscal[1];
            terms[3 * i + 2] = sm.dscal[2];
        }
    }
}

// Cost terms for caller-supplied sphere centres (costfunc::align_models, depth_penalty,
// self_collision_penalty and compute_correspondences take a sphere matrix, not a theta:
// costfunc.cpp:130-377).  S: P x 48 x 3 row-major, y/z already negated.
template <int MODE>
__global__ __launch_bounds__(HPE_NT) void k_eval_spheres(const double *__restrict__ S, int P,
                                                         const DevObs *__restrict__ og, const DevHand *__restrict__ Hg,
                                                         int32_t *__restrict__ match,
                                                         double *__restrict__ terms) {
    const DevObs o = *og;  // the selected frame (device-resident: graph-stable args)
    __shared__ Smem sm;
    const int i = blockIdx.x, t = threadIdx.x;
    stage_hand<HPE_NT>(sm.hand, Hg);
    const DevHand *__restrict__ H = &sm.hand;
    if (t < 3 * HPE_NS) {
        const int s = t / 3, r = t - 3 * s;
        const double v = S[(size_t)i * 3 * HPE_NS + t];
        sm.fk.S[s][r] = v;
        sm.fk.Sp[r][s] = (float)v;
    }
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt(cv, t);
    __syncthreads();
    eval_block<MODE, HPE_NT, false>(sm, o, cv, H, match + (size_t)i * o.n, pre);
    if (t == 0) {
        terms[3 * i + 0] = sm.dscal[0];
        terms[3 * i + 1] = sm.dscal[1];
        terms[3 * i + 2] = sm.dscal[2];
    }
}

// ------------------------------------------------------------------ PSO
// Lexicographic (value, index) minimum; NaN counts as +inf (Armadillo min(index)
// starts from +inf and keeps the first strictly smaller element).
struct VI {
    double v;
    int i;
};
__device__ __forceinline__ bool vi_less(VI a, VI b) {
    return a.v < b.v || (a.v == b.v && a.i < b.i);
}
__device__ __forceinline__ double nan_inf(double v) { return (v != v) ? __builtin_inf() : v; }

__device__ VI block_argmin(Smem &sm, VI mine) {
    int wi, unused;
    wave_argmin_lex(nan_inf(mine.v), mine.i, 0, wi, unused);
    mine.v = nan_inf(mine.v);
    {
        // the winner's value: every lane holding idx wi has the minimum
        const unsigned long long b = __ballot(mine.i == wi);
        mine.v = readlane_f64(mine.v, (int)__ffsll((long long)b) - 1);
        mine.i = wi;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm.red[w][0] = mine.v;
        sm.iscal[w] = mine.i;
    }
    __syncthreads();
    VI best = {sm.red[0][0], sm.iscal[0]};
#pragma unroll
    for (int k = 1; k < HPE_NW; ++k) {
        VI c = {sm.red[k][0], sm.iscal[k]};
        if (vi_less(c, best)) best = c;
    }
    __syncthreads();
    return best;
}

#define IB_KMAX 24  // max informant in-degree handled (host checks K <= IB_KMAX)

__device__ __forceinline__ double bits_to_f64(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ unsigned long long f64_to_bits(double v) {
    return (unsigned long long)__double_as_longlong(v);
}
// The generation's minimum pbest cost (the gmin the next generation's topology decision
// and k_pso_final read), sharded: particle i lowers cell i % GMIN_SHARDS.  All 256 blocks
// of a launch hitting ONE address serialise their atomics at the memory side for ~2 us of
// every generation; 32 cells on separate 128-B lines take 8 each.  Costs are >= 0 (or
// NaN), so u64 order is value order, and the min over the shards is order-free.
__device__ __forceinline__ unsigned long long *gmin_cell(const DevSwarm &sw, int g, int s) {
    return sw.gmin + ((size_t)g * GMIN_SHARDS + s) * GMIN_STRIDE;
}
__device__ __forceinline__ void gmin_lower(const DevSwarm &sw, int g, int i, double c) {
    atomicMin(gmin_cell(sw, g, i % GMIN_SHARDS), f64_to_bits(c));
}
// min over generation g's shards by one whole wave, in every lane; NaN if none was written.
// gmin_load issues lane l's cell (unconditional), gmin_reduce folds the wave.
__device__ __forceinline__ unsigned long long gmin_load(const DevSwarm &sw, int g) {
    const int l = threadIdx.x & 63;
    return *gmin_cell(sw, g, l < GMIN_SHARDS ? l : 0);
}
__device__ __forceinline__ double gmin_reduce(unsigned long long cell) {
    const int l = threadIdx.x & 63;
    double m = (l < GMIN_SHARDS) ? bits_to_f64(cell) : __builtin_nan("");
    m = fmin(m, dpp_f64<0xB1>(m));
    m = fmin(m, dpp_f64<0x4E>(m));
    m = fmin(m, dpp_f64<0x141>(m));
    m = fmin(m, dpp_f64<0x140>(m));
    return fmin(fmin(readlane_f64(m, 0), readlane_f64(m, 16)),
                fmin(readlane_f64(m, 32), readlane_f64(m, 48)));
}
__device__ __forceinline__ double gmin_read(const DevSwarm &sw, int g) {
    return gmin_reduce(gmin_load(sw, g));
}

__device__ __forceinline__ size_t ib_index(const DevSwarm &sw, int par, int var, int r, int slot) {
    return ((((size_t)par * 2 + var) * sw.P + r) * sw.K + slot) * IB_STRIDE;
}

// Push {tag = (g, topology, s), pbest cost, pbest row} of particle s after generation g
// into the inboxes of its receivers under the topology of generation g+1 (var 1) and
// under the kept topology topo_g (var 0).  Lane q in [0, 168): destination q / 28, field
// q % 28; (r, slot) = this lane's link, prefetched by the caller (r < 0: no push).
__device__ __forceinline__ void push_inbox(const DevSwarm &sw, int g, int s, int q, int r, int slot,
                                           int tt, double pc, const double *row) {
    if (r < 0) return;
    const int dst = q / IB_FIELDS, fld = q - IB_FIELDS * dst, var = dst < 3 ? 1 : 0;
    // the tag makes a slot valid only for the exact (g, topology) the reader expects,
    // whatever an earlier call left behind
    const double val = (fld == 0) ? __longlong_as_double(((long long)g << 48) | ((long long)tt << 32) | s)
                       : (fld == 1) ? pc : row[fld - 2];
    sw.inbox[ib_index(sw, g & 1, var, r, slot) + fld] = val;
}

// Link of lane q of the pushing waves for topology tt: {receiver, slot} as one 8-byte
// load.  Loaded unconditionally (a lane with nothing to push reads entry 0 and is marked
// !ok), so no branch merge makes the wave wait for it before its use at the push.
struct Link {
    long long raw;
    bool ok;
};
__device__ __forceinline__ Link load_link(const DevSwarm &sw, int g, int s, int q, int tt,
                                          bool want = true) {
    Link L;
    L.ok = want && g < sw.G && q >= 0 && q < 6 * IB_FIELDS && tt >= 1;
    const size_t k = L.ok ? ((size_t)tt * sw.P + s) * 3 + (q / IB_FIELDS) % 3 : 0;
    L.raw = ((const long long *)sw.outl)[k];
    return L;
}
__device__ __forceinline__ void push_inbox(const DevSwarm &sw, int g, int s, int q, const Link &L,
                                           int tt, double pc, const double *row) {
    push_inbox(sw, g, s, q, L.ok ? (int)(L.raw & 0xffffffff) : -1, (int)(L.raw >> 32), tt, pc, row);
}

// generate_particles + the initial evaluation (PSO.cpp:56-74, 748-763).
template <int NT, bool FILT = false>
__device__ __forceinline__ void pso_init_body(const DevSwarm &sw, const double *__restrict__ x0,
                                              const DevObs *__restrict__ og,
                                              const DevHand *__restrict__ Hg) {
    const DevObs o = *og;  // the selected frame (device-resident: graph-stable args)
    __shared__ Smem sm;
    const int t = threadIdx.x;
    const int i = (int)blockIdx.x;
    const double hw = hand_word<NT>(Hg);
    const DevHand *__restrict__ H = &sm.hand;
    const double *sd = sw.bounds + 2 * HPE_DOF;
    // pushing lanes: waves 1..3 (q = t - 64), topology 1 = rebuilt for gen 1
    const int q = t - 64;
    const Link lk = load_link(sw, 0, i, q, 1, q < 3 * IB_FIELDS);
    const CloudGlobal cv = obs_cloud(o);
    const Pt pre = load_pt(cv, t);
    if (t < HPE_DOF) {  // particles = x0 + randn % std (PSO.cpp:67-72)
        const size_t e = (size_t)i * HPE_DOF + t;
        const double x = x0[t] + sw.normals[e] * sd[t];
        sm.fk.th[t] = x;
        sw.xh[e] = x;
        sw.pb[e] = x;
        sw.v[e] = 0.0;
    }
    if (sw.ext && i == 0 && t == 0) sw.ext[HPE_DOF] = __builtin_inf();  // no candidate yet
    hand_put<NT>(sm.hand, hw);
    __syncthreads();
    const double c = eval_block<EV_COST, NT, true, FILT>(sm, o, cv, H, nullptr, pre, BT_GENS, nullptr, true);
    if (t == 0) {  // PSO.cpp:748-763; pbest costs are >= 0, so their bits order like values
        sw.pch[i] = c;
        gmin_lower(sw, 0, i, c);
    }
    push_inbox(sw, 0, i, q, lk, 1, c, sm.fk.th);
}

template <bool FILT>
__global__ __launch_bounds__(HPE_NT) void k_pso_init(DevSwarm sw, const double *__restrict__ x0,
                                                     const DevObs *__restrict__ og, const DevHand *__restrict__ Hg) {
    pso_init_body<HPE_NT, FILT>(sw, x0, og, Hg);
}

// One fused generation g >= 1 (PSO.cpp:781-879).  Wave 0 carries the serial part: every
// load of the generation at once (own state, draws, sig[g-1] / gmin[g-1], both inboxes),
// the topology decision, the informant, the velocity step and FK, with wave-level syncs
// only.  Waves 1..3 prefetch the push links meanwhile; then all 8 waves search.
// XCH: the opt-in per-generation exchange (sw.ext) is compiled in (k_pso_gen_x and the
// XCH forms); the default kernels carry none of it.  ROW16: every inbox holds at most 15
// slots (sw.K <= 15, the host's choice of instantiation): the informant argmin runs on one
// 16-lane DPP row.  (A run-time K test left one body for both cases: the compiler no longer
// duplicated the kernel per case, and the generation ran 0.15 us slower.)
template <int NT, bool XCH = false, bool ROW16 = true, bool FILT = false>
__device__ __forceinline__ void pso_gen_body(const DevSwarm &sw, const DevObs *__restrict__ og,
                                             const DevHand *__restrict__ Hg, int g, double W1,
                                             double C1, double C2, const InboxCounts &kin) {
    static_assert(NT >= 256 && NT % 64 == 0, "waves 1..3 push, wave 0 carries the particle");
    BLK_TS(g, 0);
    // every argument word round 1 needs, loaded at entry as one batch: left alone the
    // compiler fetched g and the gmin / sig / link / bounds pointers in a second scalar
    // round trip behind the first one's wait, ahead of every global load of the round
    // (a non-volatile asm: it touches no memory, so later loads keep their scalar form)
    int z0 = 0;
    asm("" : "+s"(z0) : "s"(g), "s"(sw.gmin), "s"(sw.sig), "s"(sw.outl), "s"(sw.bounds),
        "s"(sw.xh), "s"(sw.pch), "s"(sw.pb), "s"(sw.v), "s"(sw.inbox), "s"(sw.P), "s"(sw.K),
        "s"(og), "s"(Hg));
    StampClock sc;
    sc.begin();
    const DevObs o = *og;  // the selected frame (device-resident: graph-stable args)
    __shared__ Smem sm;
    __shared__ double ib[2][IB_KMAX][IB_FIELDS];
    const int P = sw.P, K = sw.K;
    const int i = (int)blockIdx.x + z0, t = threadIdx.x;
    // valid slots of this receiver's kept (0) / rebuilt (1) inbox: only these are read
    // (read at blockIdx.x, clamped, unconditionally: the address depends on no loaded
    // argument, so these loads leave with the argument loads instead of after them)
    const int kb = (int)blockIdx.x & (KIN_MAX - 1);
    const int k0r = kin.k0[kb], k1r = kin.k1[kb];
    const int k0 = (P <= KIN_MAX) ? k0r : K, k1 = (P <= KIN_MAX) ? k1r : K;
    // Round 1: every load of the generation is issued before any value is used (one
    // memory round trip): hand words, first cloud point, push links, inbox payload rows
    // (waves 1..7); own state, own pbest cost, inbox tags / costs, gmin cells, sig (wave 0).
    // staged into LDS before the first barrier (after the argument batch: issued ahead of
    // it, this load made the compiler wait for the first argument words alone)
    const double hw = hand_word<NT>((const DevHand *)((const char *)Hg + z0));
    const DevHand *__restrict__ H = &sm.hand;
    sc.lap(4);
    const CloudGlobal cv = obs_cloud(o);
    const size_t e = (size_t)i * HPE_DOF + t;
    const int q = t - 64;  // pushing lanes (waves 1..3): var-1 links now, var-0 after the decision
    const Link lk1 = load_link(sw, g, i, q, g + 1, q < 3 * IB_FIELDS);
    double pbi = 0, xo = 0, vo = 0, rp = 0, rg = 0;  // own state (lanes t < 26 of wave 0)
    double lbt = 0, ubt = 0;                          // bounds of dimension t
    int inf = 0, islot = -1, var = 0;
    double exr = 0.0;       // per-generation exchange (sw.ext): the candidate's row, lane t
    bool use_ext = false;   // ... and whether it beats this particle's informant
    if (t >= 64) {
        // ---- waves 1..7: both informant inboxes (payload rows) into LDS
        // the k0 valid kept slots, then the k1 valid rebuilt ones
        const double *src = sw.inbox + ib_index(sw, (g - 1) & 1, 0, i, 0);
        const size_t var_stride = (size_t)P * K * IB_STRIDE;
        const int n = (k0 + k1) * IB_FIELDS, u0 = t - 64;
        constexpr int NL = (2 * IB_KMAX * IB_FIELDS + NT - 65) / (NT - 64);  // loads per lane
        double a[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) {  // unconditional (clamped) loads: no early wait
            const int u = min(u0 + k * (NT - 64), max(n - 1, 0));
            const int vr = u >= k0 * IB_FIELDS ? 1 : 0;
            const int uv = u - vr * k0 * IB_FIELDS;  // field uv % 28 of row uv / 28
            const int off = (IB_STRIDE == IB_FIELDS) ? uv : (uv / IB_FIELDS) * IB_STRIDE + uv % IB_FIELDS;
            a[k] = src[vr * var_stride + off];
        }
        if (t < 64 + 2 * HPE_DOF) {  // wave 1 draws rp, rg while the loads are in flight
            const int j = t - 64, d = j < HPE_DOF ? j : j - HPE_DOF;
            sm.draws[j] = philox_u01(sw.seed, j < HPE_DOF ? ST_RP : ST_RG, g, i, d);
        }
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int u = u0 + k * (NT - 64);
            if (u < n) (&ib[0][0][0])[(u >= k0 * IB_FIELDS ? IB_KMAX * IB_FIELDS - k0 * IB_FIELDS : 0) + u] = a[k];
        }
    } else {
        // ---- wave 0, round 1: own state, gbest bookkeeping, inbox tags / costs
        const size_t ec = (size_t)i * HPE_DOF + (t < HPE_DOF ? t : HPE_DOF - 1);
        xo = sw.xh[(size_t)(g - 1) * P * HPE_DOF + ec];
        vo = sw.v[ec];
        pbi = sw.pb[ec];
        lbt = sw.bounds[ec - (size_t)i * HPE_DOF];
        ubt = sw.bounds[ec - (size_t)i * HPE_DOF + HPE_DOF];
        const double pci = sw.pch[(size_t)(g - 1) * P + i];  // own pbest cost (uniform)
        double tg[2], tc[2];
#pragma unroll
        for (int vr = 0; vr < 2; ++vr) {
            const int kv = vr ? k1 : k0;
            const double *sl = sw.inbox + ib_index(sw, (g - 1) & 1, vr, i, min(t, max(kv - 1, 0)));
            tg[vr] = sl[0];
            tc[vr] = sl[1];
        }
        const unsigned long long gcell = gmin_load(sw, g - 1);
        const Sig pv = sw.sig[g > 1 ? g - 1 : 0];
        if (XCH) exr = sw.ext[t <= HPE_DOF ? t : HPE_DOF];
        const double fmin = gmin_reduce(gcell);  // NaN when no value was written
        // informant = first argmin of pbest cost over {i} U incoming (PSO.cpp:810-812),
        // under BOTH variants while the gmin reduction is in flight (independent chains):
        // rebuilt = topology g, kept = the topology of g-1 (pv.topo); the decision below
        // only selects.  Candidates in lanes 0..k-1, self in lane 15 (K <= 15: one 16-lane
        // row) or 63.
        const int self_lane = ROW16 ? 15 : 63;
        int infv[2], islv[2];
        double infc[2];
#pragma unroll
        for (int vr = 0; vr < 2; ++vr) {
            const long long tag = __double_as_longlong(tg[vr]);
            const int tt = vr ? g : pv.topo;
            const bool ok = t < (vr ? k1 : k0) && (tag >> 32) == (((long long)(g - 1) << 16) | tt);
            const bool self = t == self_lane;  // L = eye
            double v = ok ? tc[vr] : (self ? pci : __builtin_inf());
            const int idx = ok ? (int)(tag & 0xffffffff) : (self ? i : 0x7fffffff);
            if (v != v) v = __builtin_inf();
            if (ROW16) row0_argmin_lex(v, idx, ok ? t : -1, infv[vr], islv[vr], XCH ? &infc[vr] : nullptr);
            else wave_argmin_lex(v, idx, ok ? t : -1, infv[vr], islv[vr], XCH ? &infc[vr] : nullptr);
        }
        BLK_TS(g, 6);
        // end-of-generation update of g-1 (PSO.cpp:864-877) / initial gbest (:755-760),
        // computed redundantly by every lane (uniform values)
        Sig sg;
        if (g == 1) {
            sg.gcost = fmin < 1e100 ? fmin : 1e100;
            sg.count = 100;  // PSO.cpp:768
            sg.topo = -1;
        } else {
            const bool imp = fmin < pv.gcost;
            sg.gcost = imp ? fmin : pv.gcost;
            sg.count = imp ? 0 : pv.count + 1;
            sg.topo = pv.topo;
        }
        if (sg.count > 0) sg.topo = g;  // topology rebuilt when count > 0 (PSO.cpp:790)
        if (i == 0 && t == 0) sw.sig[g] = sg;
        if (t == 0) {
            sm.iscal[0] = sg.topo;
            sm.dscal[4] = pci;
        }
        // var 1 iff topology g is in use; otherwise (count == 0, g >= 2) it is pv.topo
        var = (sg.topo == g) ? 1 : 0;
        sc.lap(0);
        inf = var ? infv[1] : infv[0];
        islot = var ? islv[1] : islv[0];
        // the exchanged candidate (index "P": after every local one) wins only strictly
        if (XCH) use_ext = readlane_f64(exr, HPE_DOF) < (var ? infc[1] : infc[0]);
        if (t < HPE_DOF) sm.pbr[t] = pbi;  // for the pushing waves, if x does not improve
        BLK_TS(g, 7);
        sc.lap(1);
    }
    hand_put<NT>(sm.hand, hw);
    // this thread's first cloud point, used after FK: issued behind round 1's loads, which
    // the informant choice and the row staging wait for in issue order
    const Pt pre = load_pt(cv, t);
    BLK_TS(g, 1);
    __syncthreads();  // informant rows and draws in LDS
    SphXYZ own0{0.0, 0.0, 0.0};  // wave 0: the centres FK leaves in registers
    BLK_TS(g, 2);
    if (t < 64) {
        double thl = 0.0;  // x of this lane's dimension, handed to FK's trig in a register
        // ---- velocity, position, check_constraints (PSO.cpp:824-842, 358-377)
        if (t < HPE_DOF) {
            rp = sm.draws[t];
            rg = sm.draws[HPE_DOF + t];
            double vn;
            if (inf == i && !use_ext) {
                vn = W1 * vo + (C1 * rp) * (pbi - xo);
            } else {
                const double pbn = use_ext ? exr : ib[var][islot][2 + t];
                vn = (W1 * vo + (C1 * rp) * (pbi - xo)) + (C2 * rg) * (pbn - xo);
            }
            double xn = xo + vn;
            const double xr = xn;
            if (xr < lbt) { xn = lbt; vn = 0.; }
            if (xr > ubt) { xn = lbt; vn = 0.; }  // above max -> MIN (PSO.cpp:372)
            sw.v[e] = vn;
            sw.xh[(size_t)g * P * HPE_DOF + e] = xn;
            sm.fk.th[t] = xn;
            thl = xn;
        }
        wave_sync();
        BLK_TS(g, 10);
        sc.lap(2);
        fk_wave(sm.fk, H, &own0, &thl);
    }
    __syncthreads();  // spheres, topology and own pbest cost published
    BLK_TS(g, 3);
    const int topo = sm.iscal[0];
    const double pci = sm.dscal[4];
    const Link lk0 = load_link(sw, g, i, q, topo, q >= 3 * IB_FIELDS);
    // ---- evaluation and pbest (PSO.cpp:848-861)
    const double fx = eval_block<EV_COST, NT, false, FILT>(sm, o, cv, H, nullptr, pre, g, &own0, true);
    BLK_TS(g, 4);
    sc.start();
    const bool better = fx < pci;
    const double pn = better ? fx : pci;
    if (t < HPE_DOF) sw.pb[e] = better ? sm.fk.th[t] : pbi;
    if (t == 0) {
        sw.pch[(size_t)g * P + i] = pn;
        gmin_lower(sw, g, i, pn);
    }
    // the pushed pbest row: this generation's x (in LDS since the velocity step) or the
    // entry pbest (staged before the first barrier); `better` is block-uniform, so no
    // barrier waits for wave 0 here
    push_inbox(sw, g, i, q, q < 3 * IB_FIELDS ? lk1 : lk0, q < 3 * IB_FIELDS ? g + 1 : topo, pn,
               better ? sm.fk.th : sm.pbr);
    BLK_TS(g, 5);
    sc.lap(3);
    sc.span(5);
}

template <bool ROW16, bool FILT>
__global__ __launch_bounds__(HPE_NT) void k_pso_gen(DevSwarm sw, const DevObs *__restrict__ og,
                                                    const DevHand *__restrict__ Hg, int g,
                                                    double W1, double C1, double C2,
                                                    InboxCounts kin) {
    pso_gen_body<HPE_NT, false, ROW16, FILT>(sw, og, Hg, g, W1, C1, C2, kin);
}
template <bool ROW16, bool FILT>
__global__ __launch_bounds__(HPE_NT) void k_pso_gen_x(DevSwarm sw, const DevObs *__restrict__ og,
                                                      const DevHand *__restrict__ Hg, int g,
                                                      double W1, double C1, double C2,
                                                      InboxCounts kin) {
    pso_gen_body<HPE_NT, true, ROW16, FILT>(sw, og, Hg, g, W1, C1, C2, kin);
}

// ---------------------------------------------------------------- wave-per-particle form
// For swarms much larger than the CU count (BASELINE configs 4 and 5) one workgroup per
// particle leaves the SIMDs idle during the single-wave FK and reductions; here each wave
// carries one particle end to end (same arithmetic and draws, per-wave syncs only) and
// PW_WPB particles share a workgroup, so the CU interleaves many particles' latency
// chains.  The informant's pbest row is read from the inbox after the choice.
#define PW_WPB 4
#define PW_NT (64 * PW_WPB)

__device__ __forceinline__ void push_lane_links(const DevSwarm &sw, int g, int i, int l, int tt0,
                                                int tt1, Link (&lk)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int q = l + 64 * k;
        const int tt = (q < 3 * IB_FIELDS) ? tt0 : tt1;
        lk[k] = load_link(sw, g, i, q, tt);
    }
}

// The wave form's pushes: {tag, cost} as ONE 16-B entry of the compact array ibtc
// [g&1][var][receiver][slot] (the receiver reads its K entries of a variant as one
// contiguous run, 2 lines, instead of the first 16 B of K rows, K lines), the pbest row into
// fields 2..27 of the inbox row (read only for the chosen informant).
__device__ __forceinline__ size_t ibtc_index(const DevSwarm &sw, int par, int var, int r, int slot) {
    return (((size_t)par * 2 + var) * sw.P + r) * sw.K + slot;
}
__device__ __forceinline__ void push_inbox_w(const DevSwarm &sw, int g, int s, int q, const Link &L,
                                             int tt, double pc, const double *row) {
    const int r = L.ok ? (int)(L.raw & 0xffffffff) : -1, slot = (int)(L.raw >> 32);
    if (r < 0) return;
    const int dst = q / IB_FIELDS, fld = q - IB_FIELDS * dst, var = dst < 3 ? 1 : 0;
    if (fld == 0) {
        typedef double d2v __attribute__((ext_vector_type(2)));
        const d2v e = {__longlong_as_double(((long long)g << 48) | ((long long)tt << 32) | s), pc};
        *(d2v *)(sw.ibtc + 2 * ibtc_index(sw, g & 1, var, r, slot)) = e;
    } else if (fld >= 2) {
        sw.inbox[ib_index(sw, g & 1, var, r, slot) + fld] = row[fld - 2];
    }
}

template <int WPP, bool COOP>
__global__ __launch_bounds__(PW_NT) void k_pso_init_w(DevSwarm sw, const double *__restrict__ x0,
                                                      const DevObs *__restrict__ og,
                                                      const DevHand *__restrict__ Hg) {
#include "hpe_wave_init_body.inc"
}

// one (four) waves per particle: four waves per SIMD, so every workgroup of a 4096 (1024) swarm is
// resident (the register count sits at the 128 boundary)
template <bool XCH, bool ROW16, int WPP, bool COOP>
__global__ __launch_bounds__(PW_NT, WPP == 2 ? 2 : 4) void k_pso_gen_w(DevSwarm sw, const DevObs *__restrict__ og,
                                                     const DevHand *__restrict__ Hg, int g,
                                                     double W1, double C1, double C2) {
#include "hpe_wave_gen_body.inc"
}

// The opt-in per-generation exchange (hpe_set_exchange): this subswarm's best after
// generation g -- {pbest row, pbest cost} of the first argmin of the generation's pbest
// costs (NaN as +inf, as the informant choice) -- into sw.ext, which the caller's
// collective then replaces by the best over all subswarms.  One workgroup.
__global__ __launch_bounds__(HPE_NT) void k_swarm_best(DevSwarm sw, int g) {
    __shared__ Smem sm;
    const int t = threadIdx.x, P = sw.P;
    VI mine = {__builtin_inf(), 0};
    for (int k = t; k < P; k += HPE_NT) {
        const double v = nan_inf(sw.pch[(size_t)g * P + k]);
        if (v < mine.v) {
            mine.v = v;
            mine.i = k;
        }
    }
    const VI b = block_argmin(sm, mine);
    if (t < HPE_DOF) sw.ext[t] = sw.pb[(size_t)b.i * HPE_DOF + t];
    if (t == HPE_DOF) sw.ext[HPE_DOF] = sw.pch[(size_t)g * P + b.i];
}

// Multi-GPU subswarms, the per-frame best of N (hpe_pick_best): state <- the
// row of gathered (world x 27: {bestp, cost} per rank) with the smallest cost, in one launch
// on the tracker stream right after the all-gather.  Exactly hpe/dist.py pick_best
// (torch.nan_to_num(cost, nan=inf) then the first argmin): NaN -> +inf, +inf -> the largest
// finite double, -inf -> the lowest; ties go to the lowest rank.  One wave, world <= 64.
// Inside a sequence (hist, cur: the library's own exchange, hpe_subswarm_init) the frame's
// history row gets the picked state too: row *cur - 1 of the row cursor, which the frame's
// final kernel has already advanced.
// The rule as a wave argmin (lane l = rank l; every lane gets the winner): the lexicographic
// minimum of (sanitised cost, rank) -- rows past world carry (+inf, rank >= world), so they
// lose to every real row, an all-NaN world included.
__device__ __forceinline__ int pick_best_row(const double *__restrict__ gathered, int world, int l) {
    double v = (l < world) ? gathered[(size_t)l * (HPE_DOF + 1) + HPE_DOF] : __builtin_inf();
    if (l < world) {
        if (v != v) v = __builtin_inf();
        else if (v == __builtin_inf()) v = 1.7976931348623157e308;
        else if (v == -__builtin_inf()) v = -1.7976931348623157e308;
    }
    int i = l;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (ov < v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
    return __builtin_amdgcn_readfirstlane(i);
}
// state <- the picked row; inside a sequence the frame's history row too (row *cur - 1).
__device__ __forceinline__ double pick_apply(const double *__restrict__ gathered, int w, int l,
                                             double *__restrict__ state, double *__restrict__ hist,
                                             const int *__restrict__ cur) {
    const double x = l <= HPE_DOF ? gathered[(size_t)w * (HPE_DOF + 1) + l] : 0.0;
    if (l <= HPE_DOF) state[l] = x;
    if (hist && cur && l <= HPE_DOF) hist[(size_t)(HPE_DOF + 1) * (cur[0] - 1) + l] = x;
    return x;
}
__global__ __launch_bounds__(64) void k_pick_best(const double *__restrict__ gathered, int world,
                                                  double *__restrict__ state,
                                                  double *__restrict__ hist = nullptr,
                                                  const int *__restrict__ cur = nullptr) {
    const int l = threadIdx.x;
    pick_apply(gathered, pick_best_row(gathered, world, l), l, state, hist, cur);
}

// The scripted transport of the subswarm exchange (hpe_subswarm_init_scripted), in the place
// of the all-gather: rows w != rank of script frame *k ([frames][world][27]) into the gather
// buffer; row `rank` (the frame's own result, k_pso_final's) is never written.  *k is the
// device-resident exchange counter, advanced here (past the last frame: back to 0), so a
// replayed chunk graph reads the script frame of its own exchange.  One wave.
__global__ __launch_bounds__(64) void k_script_rows(const double *__restrict__ script, int frames,
                                                    int world, int rank, int *__restrict__ k,
                                                    double *__restrict__ gathered) {
    const int l = threadIdx.x;
    int f = __builtin_amdgcn_readfirstlane(*k);  // every lane, before lane 0's store below
    if (f < 0 || f >= frames) f = 0;
    const int n = world * (HPE_DOF + 1);
    const double *__restrict__ src = script + (size_t)f * n;
    for (int i = l; i < n; i += 64)
        if (i / (HPE_DOF + 1) != rank) gathered[i] = src[i];
    if (l == 0) *k = f + 1 < frames ? f + 1 : 0;
}

// u64 wave helpers of k_pso_final's replay: lane l - 1's value (lane 0: fill), the
// inclusive prefix minimum over lanes 0..l (DPP row_shr 1/2/4/8, row_bcast 15/31; lanes
// without a source keep the identity, all ones), a lane's value in every lane.
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ unsigned long long dpp_min_src_u64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)v, CTRL, ROWMASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)(v >> 32), CTRL, ROWMASK, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_prefix_min_u64(unsigned long long v) {
    v = min(v, dpp_min_src_u64<0x111>(v));        // row_shr:1
    v = min(v, dpp_min_src_u64<0x112>(v));        // row_shr:2
    v = min(v, dpp_min_src_u64<0x114>(v));        // row_shr:4
    v = min(v, dpp_min_src_u64<0x118>(v));        // row_shr:8
    v = min(v, dpp_min_src_u64<0x142, 0xa>(v));   // row_bcast:15
    v = min(v, dpp_min_src_u64<0x143, 0xc>(v));   // row_bcast:31
    return v;
}
__device__ __forceinline__ unsigned long long from_left_u64(unsigned long long v, unsigned long long fill) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)fill, (int)(unsigned)v, 0x138, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(fill >> 32), (int)(unsigned)(v >> 32), 0x138, 0xf, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;  // wave_shr:1
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Last end-of-generation update and bestp = gbest_pos (PSO.cpp:864-882).  Replays the
// gbest / count sequence from gmin[], finds the last improving generation g* and takes
// particles.col(first argmin pcost) of that generation; resets gmin[] for the next call.
// TAIL (a tracked frame, testmodel.cpp:130-132): out[26] = cal_cost(bestp), and the
// frame descriptor used is copied to obs_out (the API's "selected frame").  When some
// generation improved, bestp = particles.col(argmin pcost) of the last improving
// generation g*, and that particle's pbest cost was set AT g* (an older value could not
// undercut the previous gbest), i.e. it IS cal_cost(bestp) computed by the same
// eval_block on the same theta: the gbest cost is kept, bit for bit (same_eval: the
// generations used the workgroup form).  Otherwise (nothing beat 1e100, bestp = zeros)
// the block evaluates it.
template <bool TAIL = false, bool FILT = false>
__global__ __launch_bounds__(HPE_NT) void k_pso_final(DevSwarm sw, double *__restrict__ out,
                                                      const DevObs *og = nullptr,
                                                      const DevHand *__restrict__ Hg = nullptr,
                                                      DevObs *__restrict__ obs_out = nullptr,
                                                      int same_eval = 0,
                                                      unsigned long long *__restrict__ seq_dev = nullptr,
                                                      unsigned long long *done_host = nullptr,
                                                      double *__restrict__ hist = nullptr,
                                                      const int *__restrict__ fail = nullptr,
                                                      const DevObs *__restrict__ seq_table = nullptr,
                                                      DevObs *seq_obs = nullptr,  // aliases og
                                                      int *__restrict__ seq_cur = nullptr) {
#include "hpe_final_body.inc"
}

// Start of an offline sequence (hpe_track_sequence_dev): the first frame's descriptor into
// the chunk graphs' descriptor, the cursor to {first slot, history row 0}.
__global__ void k_seq_begin(const DevObs *__restrict__ table, int first, DevObs *__restrict__ cur_obs,
                            int *__restrict__ cur) {
    const int t = threadIdx.x;
    if (t < (int)(sizeof(DevObs) / 8))
        ((unsigned long long *)cur_obs)[t] = ((const unsigned long long *)(table + first))[t];
    if (t == 0) {
        cur[0] = first;
        cur[1] = 0;
    }
}

// ------------------------------------------------------------------ refine
// refine_init_pose (PSO.cpp:216-266) with cal_grad (:183-214) and goldstein (:438-480)
// as ONE persistent workgroup of RF_NT threads.  Each iteration:
//   * f_k = cal_cost2(x0, matchId, true): FK by wave 0, search by all RF_NT threads;
//   * the 6 central differences run concurrently, one wave each (frozen matchId);
//   * the Goldstein bracket search is evaluated SPECULATIVELY: each wave evaluates one node
//     of a small tree of the search's next decisions (gold_tree, shapes below), then every
//     thread walks the tree with the serial algorithm's exact rules.  Identical arithmetic
//     on identical alphas: the result, the step tk and the evaluation count equal the
//     serial ones.
// Control flow is uniform: every thread evaluates the same scalar decisions from LDS.
#ifndef RF_NT
#define RF_NT 512
#endif
#define RF_NW (RF_NT / 64)
static_assert(RF_NW >= 8, "the speculation shapes use up to 8 waves");
#define RF_STAGE_MAX 2048  // clouds up to this size are staged in LDS with their matchId

struct __align__(16) RefineSm {
    FkSm w[RF_NW];
    FkSm base;  // spheres of the current x0
    double red[16][4];
    double x0[32];
    double f[RF_NW];
    double fg[RF_NW];  // the gradient points' costs (k_refine, single-workgroup form)
    FkX X;  // rotation-only joint terms of x0 (refine block 2: translation steps)
    RigidSm rg;  // hand-frame centres, block 2's rotated centres, collision (rigid refine)
    unsigned ts_n;  // diagnostic build: refine timeline entries written
};

// Goldstein bracket update (PSO.cpp:459-474), shared by the speculating waves and the walk.
__device__ __forceinline__ void gold_up(double &a, double b, double &alpha) {
    a = alpha;
    const double up = 2 * alpha, mid = 0.5 * (alpha + b);
    alpha = (mid < up) ? mid : up;  // std::min(t*alpha, 0.5*(alpha+b))
}
__device__ __forceinline__ void gold_down(double a, double &b, double &alpha) {
    b = alpha;
    alpha = 0.5 * (a + alpha);
}

// The hand-frame form's correspondence search takes one item on every wave (round 4: the
// chain form's spread balanced the SIMDs against the gradient heads' DH chains).
#ifndef HPE_RF_SPREAD
#define HPE_RF_SPREAD 1
#endif

// ---------------------------------------------------------------- multi-workgroup refine
// For clouds larger than RF_STAGE_MAX one CU is throughput-bound (every Goldstein round is
// seven frozen alignments of the whole cloud), so the refine launch adds Q helper
// workgroups.  Workgroup 0 keeps the whole serial algorithm; each batch of evaluations
// (the correspondence eval of x0, the gradient pairs, a Goldstein round) is published as
// a job.  Helper h owns cloud slice h (and its matchId, written by the correspondence
// job and read back by the same workgroup), computes the nodes' FK itself and returns one
// partial alignment sum per node.  Workgroup 0 computes depth + collision meanwhile and
// sums the partials in helper order (deterministic).  Hand-off per the G16 recipe:
// stores drained, barrier, agent release, counter; one-lane agent acquire, barrier.
// Every wait is bounded (~2 s): on a timeout the launch ends early with *err set.
#define MW_SPIN_MAX (1 << 21)
static_assert(MW_MAX_Q % MW_DONE_SHARDS == 0, "helpers split evenly over the shards");

__device__ __forceinline__ bool mw_wait_geq(unsigned *p, unsigned v, int spin) {
    for (int i = 0; i < spin; ++i) {
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            return true;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return false;
}

// A hand-off timed out: flag it on the device (hpe_sync) and in pinned host memory (the
// next tracking call), both plain stores of 1.
__device__ __forceinline__ void mw_fail(const DevMw &mw) {
    __hip_atomic_store(mw.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mw.err_host) __hip_atomic_store(mw.err_host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct MwLeader {
    DevMw mw;
    unsigned k;   // jobs published so far
    bool failed;  // a wait timed out: stop issuing work
};

// Workgroup 0: publish the next job (CORR: theta = rs.x0; FROZEN: rs.w[0..nn).th).
__device__ __forceinline__ void mw_publish(MwLeader &ml, RefineSm &rs, int type, int nn) {
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    if (type == MW_JOB_CORR) {
        if (t < HPE_DOF) ml.mw.job->th[0][t] = rs.x0[t];
    } else if (type == MW_JOB_FROZEN) {
        if (w < nn && l < HPE_DOF) ml.mw.job->th[w][l] = rs.w[w].th[l];
    }
    if (t == 0) {
        ml.mw.job->type = type;
        ml.mw.job->nnodes = nn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ml.k += 1;
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(&ml.mw.ctr[0], ml.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Workgroup 0: wait until every helper has returned job ml.k (each completion shard has
// counted Q / MW_DONE_SHARDS helpers per job).
__device__ void mw_collect(MwLeader &ml, int *flag) {
    if (threadIdx.x == 0) {
        bool ok = !ml.failed;
        const unsigned want = ml.k * (unsigned)(ml.mw.Q / MW_DONE_SHARDS);
        for (int s = 0; s < MW_DONE_SHARDS && ok; ++s)
            ok = mw_wait_geq(&ml.mw.ctr[32 * (1 + s)], want, ml.mw.spin);
        if (!ok) mw_fail(ml.mw);
        *flag = ok ? 1 : 0;
    }
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(*flag)) ml.failed = true;  // decides exits (§7)
}

// Node w's alignment sum: the Q partials folded by one wave in a fixed order.
__device__ __forceinline__ double mw_sum(const MwLeader &ml, int w) {
    const int l = threadIdx.x & 63;
    const double v = (l < ml.mw.Q) ? ml.mw.part[l * MW_MAX_NODES + w] : 0.0;
    return wave_sum(v);
}

// rs.f[w] = cal_cost2(rs.w[w].th, matchId, false) for w < nn; each wave has written its
// own rs.w[w].th.  Ends with a workgroup barrier.
// RIGID: the nodes' spheres by rigid_wave (rblk 0: rotation block, 1: translation block),
// the collision the constant rs.rg.C.
template <bool MW, bool RIGID = false, class CV>
__device__ __forceinline__ void eval_nodes(RefineSm &rs, int nn, const DevObs &o, const CV &cv,
                                           const DevHand *__restrict__ H,
                                           const int32_t *__restrict__ match, FkX *Xt,
                                           MwLeader *ml, int *flag, const double *thr = nullptr,
                                           const FrozenPts *fp = nullptr, int rblk = 0,
                                           const double *md2p = nullptr) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (!MW) {
        if (w < nn) {
            wave_sync();
            double f;
            if (RIGID) {
                const FrozenHead hd = rblk ? rigid_head<RG_TRANS>(rs.w[w], o, H, rs.rg, *thr)
                                           : rigid_head<RG_ROT>(rs.w[w], o, H, rs.rg, *thr);
                f = frozen_tail<true>(rs.w[w], o, cv, H, match, hd, fp, md2p) + rs.rg.C;
            } else {
                f = eval_wave_frozen<true>(rs.w[w], o, cv, H, match, Xt, thr, fp);
            }
            if (l == 0) rs.f[w] = f;
        }
        REF_TS(rs.ts_n, 9);  // wave 0's node done
        __syncthreads();
        REF_TS(rs.ts_n, 8);  // every node done
        return;
    }
    mw_publish(*ml, rs, MW_JOB_FROZEN, nn);
    double dep = 0.0, co = 0.0;
    if (w < nn) {  // depth + collision here while the helpers align
        if (RIGID) {
            const double thl = rs.w[w].th[l < HPE_DOF ? l : 0];
            if (rblk) rigid_wave<RG_TRANS>(rs.w[w], rs.rg, thl);
            else rigid_wave<RG_ROT>(rs.w[w], rs.rg, thl);
            dep = (l < HPE_NS) ? depth_term(rs.w[w], l, o, H) : 0.0;
            dep = wave_sum(dep);
        } else {
            if (Xt) fk_wave_t<FK_TRANSLATE>(rs.w[w], H, Xt);
            else fk_wave(rs.w[w], H);
            dep = (l < HPE_NS) ? depth_term(rs.w[w], l, o, H) : 0.0;
            co = collide_term(rs.w[w], l, H) + collide_term(rs.w[w], l + 64, H) +
                 ((l < 16) ? collide_term(rs.w[w], l + 128, H) : 0.0);
            wave_sum2(dep, co);
        }
    }
    mw_collect(*ml, flag);
    if (w < nn) {
        const double al = mw_sum(*ml, w);
        const double f = RIGID ? (al * o.lambda + dep) + rs.rg.C : (al * o.lambda + dep) + co;
        const double fr = ml->failed ? __builtin_nan("") : f;
        if (l == 0) rs.f[w] = fr;
    }
    __syncthreads();
}

// f_k = cal_cost2(x0, matchId, true) with the spheres of x0 in rs.base.
// The collision sum of a refine is one constant: the refine moves theta0..5 only, a rigid
// motion of the whole hand, so co here, in eval_nodes' MW branch and in frozen_head as the
// refine calls it (rs.rg.C in the rigid form) has the same value in every evaluation, cancels
// in every Goldstein test, and the call reports no cost.  A wrong pair map at these sites
// cannot change a result, so no test pins them; tests/test_gpu_collision.py pins collide_term
// through eval_block and frozen_head through pso_optimise's descent.
template <bool MW, bool RIGID = false, class CV>
__device__ __forceinline__ double eval_corr(RefineSm &rs, const DevObs &o, const CV &cv,
                                            const DevHand *__restrict__ H, int32_t *__restrict__ match,
                                            MwLeader *ml, int *flag) {
    const int t = threadIdx.x;
    if (MW) mw_publish(*ml, rs, MW_JOB_CORR, 1);
    const DepthG dg = depth_issue_w0(rs.base, o, H);
    const bool young = (t >> 6) >= HPE_SETPRIO_FROM;  // as in eval_block
    if (young) __builtin_amdgcn_s_setprio(1);
    double al = MW ? 0.0 : search_align<RF_NT, true>(rs.base, cv, H, match, load_pt(cv, t));
    if (young) __builtin_amdgcn_s_setprio(0);
    double co = (!RIGID && t < 144) ? collide_term(rs.base, t, H) : 0.0;
    double dep = depth_finish(dg, o, t < HPE_NS);
    block_sum3<RF_NT>(rs.red, al, dep, co);  // also publishes matchId to the block
    if (MW) {
        mw_collect(*ml, flag);
        al = mw_sum(*ml, 0);
        if (ml->failed) return __builtin_nan("");
    }
    if (RIGID) return (al * o.lambda + dep) + rs.rg.C;
    return (al * o.lambda + dep) + co;
}

// Helper workgroup h of a multi-workgroup refine launch: serve jobs until EXIT.
template <bool RIGID>
__device__ __forceinline__ void mw_helper(const DevMw &mw, int h, const DevObs *__restrict__ og,
                          const DevHand *__restrict__ Hg, int32_t *__restrict__ match_g) {
    __shared__ FkSm nodes[MW_MAX_NODES];
    __shared__ RigidSm hq;  // RIGID: hand-frame centres, built from the first job's digits
    bool have_q = false;
    __shared__ DevHand hs;
    __shared__ double red[16][4];
    __shared__ int sh[2];
    const DevObs o = *og;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    stage_hand<RF_NT>(hs, Hg);
    const DevHand *__restrict__ H = &hs;
    const int Q = mw.Q, per = (o.n + Q - 1) / Q;
    const int s0 = min(h * per, o.n), s1 = min(s0 + per, o.n);
    const CloudGlobal cs{gp(o.cx) + s0, gp(o.cy) + s0, gp(o.cz) + s0, s1 - s0};
    int32_t *ms = match_g + s0;
    __syncthreads();
    for (unsigned k = 1;; ++k) {
        if (t == 0) {
            int type = -1, nn = 0;
            if (mw_wait_geq(&mw.ctr[0], k, mw.spin)) {
                type = mw.job->type;
                nn = mw.job->nnodes;
            } else {
                mw_fail(mw);
            }
            sh[0] = type;
            sh[1] = nn;
        }
        __syncthreads();
        // uniform to the compiler: they decide the exit and the barriers below (§7)
        const int type = __builtin_amdgcn_readfirstlane(sh[0]), nn = __builtin_amdgcn_readfirstlane(sh[1]);
        if (type != MW_JOB_CORR && type != MW_JOB_FROZEN) {
            // the last helper out resets the counters for the next launch
            if (type == MW_JOB_EXIT && t == 0 &&
                atomicAdd(&mw.ctr[32 * (1 + MW_DONE_SHARDS)], 1u) == (unsigned)Q - 1) {
                for (int c = 0; c < MW_CTR_WORDS; c += 32) mw.ctr[c] = 0u;
            }
            return;
        }
        if (type == MW_JOB_CORR) {  // search + alignment over the slice, matchId stored
            const double th0 = mw.job->th[0][t < HPE_DOF ? t : 0];
            if (RIGID && !have_q) {  // the digits are fixed for the whole refine launch
                if (t < HPE_DOF) nodes[0].th[t] = (t == 0) ? -180.0 : (t < 6) ? 0.0 : th0;
                __syncthreads();
                if (w == 0) {
                    SphXYZ own;
                    fk_wave(nodes[0], H, &own);
                    if (l < HPE_NS) {
                        hq.q[l][0] = own.x;
                        hq.q[l][1] = own.y * -1;
                        hq.q[l][2] = own.z * -1;
                    }
                }
                have_q = true;
                __syncthreads();
            }
            if (t < HPE_DOF) nodes[0].th[t] = th0;
            __syncthreads();
            if (w == 0) {
                if (RIGID) rigid_wave<RG_ROT>(nodes[0], hq, th0);
                else fk_wave(nodes[0], H);
            }
            __syncthreads();
            double al = search_align<RF_NT, true>(nodes[0], cs, H, ms, load_pt(cs, t));
            double z1 = 0.0, z2 = 0.0;
            block_sum3<RF_NT>(red, al, z1, z2);
            if (t == 0) mw.part[h * MW_MAX_NODES] = al;
        } else if (w < nn) {  // one node per wave, frozen matchId of the slice
            const double thl = mw.job->th[w][l < HPE_DOF ? l : 0];
            if (l < HPE_DOF) nodes[w].th[l] = thl;
            wave_sync();
            if (RIGID) rigid_wave<RG_ROT>(nodes[w], hq, thl);  // (Rg q) + u == P + u
            else fk_wave(nodes[w], H);
            const double al = wave_sum(align_frozen(nodes[w], cs, H, ms, l, 64));
            if (l == 0) mw.part[h * MW_MAX_NODES + w] = al;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            atomicAdd(&mw.ctr[32 * (1 + h % MW_DONE_SHARDS)], 1u);
        }
    }
}

// ---------------------------------------------------------------- speculated translation block
// The two-workgroup form of the staged refine (DevSpec, hpe_layout.hpp).  The
// leader (workgroup 0) runs the serial algorithm and only ever stores: before each line search
// of the rotation block, wave SPEC_PW sends x0 as granules and goes on.  The runner (workgroup
// 1) runs the translation block from the newest x0 with the body's own statements; one of its
// waves loads the granules at the start of a round and looks at them at the round's end, so a
// newer x0 restarts it and an abort ends it without a wait of its own.  Only when the rotation
// block ends on a failing search (x0 unchanged: the runner started from the block's final
// pose) does the leader wait, bounded by DevSpec::spin polls, for the runner's x0[3..5] and
// evaluation count; otherwise, or when that wait runs out, it aborts the runner and runs the
// block itself.  A granule is one aligned 8-byte agent-scope store ({tag, 32-bit value}): a
// reader takes a message only when all its tags agree, so no fence orders anything.
#define SPEC_SPIN_MAX 1024       // the leader's polls for a committed result (~1 ms)
#define SPEC_IDLE_SPIN (1 << 20) // the runner's polls for its next word (the leader always sends one)
#define SPEC_PW (RF_NW - 1)      // the wave that sends (leader) and polls (runner)

struct SpecSm {
    unsigned half[SPEC_X0_GRAN];  // the newer x0 a poll found
    int verdict;                  // runner: 0 go on, > 0 restart from message `verdict`, -1 exit;
                                  // leader: 1 = the runner's result is in res / evals
    int evals;
    double res[3];
};
struct SpecPoll {  // the runner's view of the leader's words (gold_tree polls through it)
    DevSpec sp;
    SpecSm *sm;
    unsigned ep;  // this launch's epoch
    int seq;      // the message the runner works on
};

__device__ __forceinline__ unsigned long long spec_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void spec_store(unsigned long long *p, unsigned tag, unsigned v) {
    __hip_atomic_store(p, ((unsigned long long)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned spec_half(double x, int hi) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return hi ? (unsigned)(b >> 32) : (unsigned)b;
}
// Leader, one wave: message tag & 31 = x0 (26 doubles in LDS).  Stores only.
__device__ __forceinline__ void spec_send(const DevSpec &sp, unsigned tag, const double *x0) {
    const int l = threadIdx.x & 63;
    if (l < SPEC_X0_GRAN) spec_store(sp.g + l, tag, spec_half(x0[l >> 1], l & 1));
}
// Runner, one whole wave: load the message and the control granule ...
__device__ __forceinline__ unsigned long long spec_poll_issue(const DevSpec &sp) {
    const int l = threadIdx.x & 63;
    return spec_load(sp.g + (l < SPEC_CTL ? l : SPEC_CTL));
}
// ... and judge them: -1 the leader aborted, s > seq a whole message s of this launch (its x0
// into sm.half), else 0; *commit = the message the leader committed to (0: none).  The verdict
// goes to sm.verdict for the other waves (read behind the caller's barrier).
__device__ __forceinline__ int spec_poll_take(SpecSm &sm, unsigned long long g, unsigned ep,
                                              int seq, int *commit = nullptr) {
    const int l = threadIdx.x & 63;
    const unsigned tag = (unsigned)(g >> 32), val = (unsigned)g;
    const unsigned t0 = (unsigned)__builtin_amdgcn_readlane((int)tag, 0);
    const unsigned ct = (unsigned)__builtin_amdgcn_readlane((int)tag, SPEC_CTL);
    const unsigned cv = (unsigned)__builtin_amdgcn_readlane((int)val, SPEC_CTL);
    const bool whole = __all(l >= SPEC_X0_GRAN || tag == t0) != 0;
    const bool mine = (ct >> 5) == ep;
    int v = 0;
    if (mine && cv == SPEC_ABORT) {
        v = -1;
    } else if (whole && (t0 >> 5) == ep && (int)(t0 & 31u) > seq) {
        v = (int)(t0 & 31u);
        if (l < SPEC_X0_GRAN) sm.half[l] = val;
    }
    if (commit) *commit = (mine && cv == SPEC_COMMIT) ? (int)(ct & 31u) : 0;
    if (l == 0) sm.verdict = v;
    return v;
}
// Runner, every thread: wait for the next word that concerns it -- a message newer than seq,
// an abort, or (done: the block of message seq is finished) the commit of seq.  Returns the
// new message's number, 0 for the commit, -1 to exit (abort, or the polls ran out: the leader
// always sends an abort or a commit, so only a leader that never ran gets there).  Barriers
// at both ends: sm is free on entry and read by everyone on exit.
__device__ __forceinline__ int spec_wait(const DevSpec &sp, SpecSm &sm, unsigned ep, int seq, bool done) {
    __syncthreads();
    if (threadIdx.x < 64) {
        int v = -1;
        for (int i = 0; i < SPEC_IDLE_SPIN; ++i) {
            int commit = 0;
            const int r = spec_poll_take(sm, spec_poll_issue(sp), ep, seq, &commit);
            if (r != 0 || (done && commit == seq)) {
                v = r;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (threadIdx.x == 0) sm.verdict = v;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(sm.verdict);  // decides exits and barriers (§7)
}
// Runner, every thread: x0 = the message a poll left in sm.half.  Ends with a barrier.
__device__ __forceinline__ void spec_take_x0(const SpecSm &sm, double *x0) {
    const int t = threadIdx.x;
    if (t < HPE_DOF)
        x0[t] = __longlong_as_double((long long)(((unsigned long long)sm.half[2 * t + 1] << 32) | sm.half[2 * t]));
    __syncthreads();
}
// Runner, wave 0: the finished block's x0[3..5] and evaluation count, tagged with the message.
__device__ __forceinline__ void spec_result(const DevSpec &sp, unsigned tag, const double *x0, int evals) {
    const int l = threadIdx.x & 63;
    if (l < 6) spec_store(sp.g + SPEC_RES + l, tag, spec_half(x0[3 + (l >> 1)], l & 1));
    else if (l == 6) spec_store(sp.g + SPEC_RES + 6, tag, (unsigned)evals);
}
// Leader, wave 0: commit to message tag & 31 and wait, at most sp.spin polls, for its result;
// on any other end tell the runner to stop.  true: sm.res / sm.evals hold the result.
__device__ __forceinline__ bool spec_commit(const DevSpec &sp, SpecSm &sm, unsigned tag, bool failed) {
    const int l = threadIdx.x & 63;
    bool ok = false;
    if (failed && sp.spin > 0) {
        if (l == 0) spec_store(sp.g + SPEC_CTL, tag, SPEC_COMMIT);
        for (int i = 0; i < sp.spin && !ok; ++i) {
            const unsigned long long g = spec_load(sp.g + SPEC_RES + (l < 7 ? l : 6));
            ok = __all((unsigned)(g >> 32) == tag) != 0;
            if (ok) {
                const unsigned lo = (unsigned)__shfl((int)(unsigned)g, (l << 1) & 63);
                const unsigned hi = (unsigned)__shfl((int)(unsigned)g, ((l << 1) + 1) & 63);
                if (l < 3) sm.res[l] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
                if (l == 6) sm.evals = (int)(unsigned)g;
            } else {
                __builtin_amdgcn_s_sleep(2);
            }
        }
    }
    if (!ok && l == 0) spec_store(sp.g + SPEC_CTL, tag, SPEC_ABORT);
    return ok;
}

// Speculation shapes of the Goldstein search.  A round evaluates the nodes of a small
// tree of decision prefixes, relative to the bracket state (a, b, alpha) at the round's
// start: node j lies len decisions below it, decision k = bit k of bits (1 = "up": Armijo
// holds but Goldstein fails, PSO.cpp:461-466; 0 = "down": Armijo fails, :468-471), packed
// as byte j of nb = len << 5 | bits; nibble j of dn / up is node j's child (15: outside the
// shape, the round ends there).  Node 0 is the current alpha.  The shape depends on the
// previous round's last decision (context 0 = a search's first round, 1 = "down", 2 =
// "up"): the decision logs of the bench sequence (the oracle's refine over three 40-frame
// trajectories) are mostly runs -- "DDDDA" alone is ~27 % of the searches -- so deep runs
// are speculated where they are likely.  Rounds over those 1,297 searches: balanced depth 3
// (7 nodes, rounds 1-2) 3,807; the 8-node shapes 3,175; the 7-node shapes 3,361; the 4-node
// shapes 4,553 (one node per SIMD).  The tables are compile-time constants selected by the
// context (no memory read on the walk).  Identical arithmetic on identical alphas in every
// shape: the walk replays the serial rules, so the result, tk and the evaluation count
// equal the serial ones.
struct GoldShape {
    int n;
    unsigned long long nb;
    unsigned dn, up;
};
#define GOLD_BALANCED 0
#define GOLD_8 1
#define GOLD_4 2
#define GOLD_OPT8 3  // pso_optimise's descent (tools/gold_shapes.py optimise)
#define GOLD_MIX 4   // GOLD_8 after a search's start and a "down", GOLD_4 after an "up"
#ifndef HPE_GOLD_POLICY
#define HPE_GOLD_POLICY GOLD_MIX  // refine_init_pose
#endif
template <int POL>
__device__ __forceinline__ GoldShape gold_shape(int ctx) {
    constexpr GoldShape T[15] = {
    // GOLD_BALANCED
    {7, 0x0043414240212000ull, 0xfffff531u, 0xfffff642u},  // first: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU'
    {7, 0x0043414240212000ull, 0xfffff531u, 0xfffff642u},  // D: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU'
    {7, 0x0043414240212000ull, 0xfffff531u, 0xfffff642u},  // U: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU'
    // GOLD_8
    {8, 0xa080604340212000ull, 0xf76f5f31u, 0xfffff4f2u},  // first: '' 'D' 'U' 'DD' 'UU' 'DDD' 'DDDD' 'DDDDD'
    {8, 0x6043414240212000ull, 0xffff7531u, 0xfffff642u},  // D: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU' 'DDD'
    {8, 0x6243414240212000ull, 0xfff7f531u, 0xfffff642u},  // U: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU' 'DUD'
    // GOLD_4
    {4, 0x0000000043212000ull, 0xfffffff1u, 0xfffff3f2u},  // first: '' 'D' 'U' 'UU'
    {4, 0x0000000060402000ull, 0xfffff321u, 0xffffffffu},  // D: '' 'D' 'DD' 'DDD'
    {4, 0x0000000040212000ull, 0xffffff31u, 0xfffffff2u},  // U: '' 'D' 'U' 'DD'
    // GOLD_OPT8
    {8, 0xbf8f674340212000ull, 0xffffff31u, 0xf765f4f2u},  // first: '' 'D' 'U' 'DD' 'UU' 'UUU' 'UUUU' 'UUUUU'
    {8, 0x6043414240212000ull, 0xffff7531u, 0xfffff642u},  // D: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU' 'DDD'
    {8, 0x6743414240212000ull, 0xfffff531u, 0xf7fff642u},  // U: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU' 'UUU'
    // GOLD_MIX (4 nodes, one wave per SIMD, run a round in ~0.71 of an 8-node one)
    {8, 0xa080604340212000ull, 0xf76f5f31u, 0xfffff4f2u},  // first: '' 'D' 'U' 'DD' 'UU' 'DDD' 'DDDD' 'DDDDD'
    {8, 0x6043414240212000ull, 0xffff7531u, 0xfffff642u},  // D: '' 'D' 'U' 'DD' 'DU' 'UD' 'UU' 'DDD'
    {4, 0x0000000040212000ull, 0xffffff31u, 0xfffffff2u},  // U: '' 'D' 'U' 'DD'
    };
    return ctx == 0 ? T[3 * POL] : ctx == 1 ? T[3 * POL + 1] : T[3 * POL + 2];
}

// goldstein(x, g, matchId, f_k, optfunc, tk, 30) (PSO.cpp:438-480) along p from rs.x0
// with frozen correspondences, speculated per round with shape policy POL (above): wave w
// evaluates node w, then every thread walks the nodes with the serial algorithm's rules.
// pl: component (threadIdx.x & 63) of the direction p, in every thread.  Returns tk (0
// after 30 rejected trials); the accepted node's spheres are copied into rs.base and its
// cost to *f_acc.  UPD: the search also applies x0 = x0 - tk * g (PSO.cpp:256; gl =
// component threadIdx.x of g) before its last barrier.  evals grows by the serial count.
// POLL with poll (the speculated refine's runner): wave SPEC_PW loads the leader's words at the start of
// every round and judges them at its end; a verdict other than 0 goes to *drop and ends the
// search at once, its result void (the caller restarts or exits).
template <bool MW = false, int POL = GOLD_BALANCED, bool UPD = false, bool RIGID = false,
          bool POLL = false, class CV>
__device__ __forceinline__ double gold_tree(RefineSm &rs, const DevObs &o, const CV &cv,
                                            const DevHand *__restrict__ H,
                                            const int32_t *__restrict__ match, double fk,
                                            double gp, double pl, double gl, int &evals,
                                            double *f_acc, FkX *Xt = nullptr,
                                            MwLeader *ml = nullptr, int *flag = nullptr,
                                            const FrozenPts *fp = nullptr, int rblk = 0,
                                            const double *md2p = nullptr,
                                            const SpecPoll *poll = nullptr, int *drop = nullptr) {
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    StampClock sc;
    sc.start();
    double A = 0, B = 1e100, alpha = 0.5, tk = 0;
    int it = 0, accepted = -1, ctx = 0;
    bool done = false;
    [[maybe_unused]] unsigned long long path = 0;  // diagnostic build: decision bits (1 = up)
    while (!done) {
        const GoldShape sh = gold_shape<POL>(ctx);
        const int nn = sh.n;
        double thl = 0.0;  // theta[l] of this wave's node (FK's trig reads it in a register)
        [[maybe_unused]] unsigned long long pg = 0;
        if constexpr (POLL) if (w == SPEC_PW) pg = spec_poll_issue(poll->sp);
        if (w < nn) {
            const int nbw = (int)((sh.nb >> (8 * w)) & 0xff), len = nbw >> 5, bits = nbw & 31;
            double ga = A, gb = B, gal = alpha;
            for (int k = 0; k < len; ++k) {
                if ((bits >> k) & 1) gold_up(ga, gb, gal);
                else gold_down(ga, gb, gal);
            }
            thl = rs.x0[l < HPE_DOF ? l : 0] + gal * pl;
            if (l < HPE_DOF) rs.w[w].th[l] = thl;
        }
        eval_nodes<MW, RIGID>(rs, nn, o, cv, H, match, Xt, ml, flag, &thl, fp, rblk, md2p);
        if (MW && ml->failed) break;  // the launch is ending early (DevMw::err)
        // the serial rules walked level by level on the nodes' costs
        int node = 0;
        accepted = -1;
#pragma unroll
        for (int lev = 0; lev < 6; ++lev) {  // the deepest shape path is 6 nodes
            if (node >= 15 || done) break;
            if (it >= 30) {
                done = true;
                tk = 0;
                break;
            }
            ++it;
            const double f1 = rs.f[node];
            const double armijo = fk + 0.25 * alpha * gp;
            const double gold = fk + (1 - 0.25) * alpha * gp;
            if (f1 <= armijo) {
                if (f1 >= gold) {
                    tk = alpha;
                    done = true;
                    accepted = node;
                } else {
                    gold_up(A, B, alpha);
                    node = (int)((sh.up >> (4 * node)) & 15u);
                    ctx = 2;
                }
            } else {
                gold_down(A, B, alpha);
                node = (int)((sh.dn >> (4 * node)) & 15u);
                ctx = 1;
            }
        }
        if (!done && it >= 30) done = true;  // tk stays 0
        // the round's outcome decides the next round's barriers: provably uniform (every lane
        // walked the same LDS costs)
        done = __builtin_amdgcn_readfirstlane(done ? 1 : 0) != 0;
        ctx = __builtin_amdgcn_readfirstlane(ctx);
        // x0 is read only before eval_nodes' barrier in a round
        if (UPD && done && t < HPE_DOF) rs.x0[t] = rs.x0[t] - tk * gl;
        if (done && accepted >= 0) {  // keep the accepted node's spheres for the next f_k
            for (int q = t; q < (int)(offsetof(FkSm, J) / 8); q += RF_NT)
                ((double *)&rs.base)[q] = ((const double *)&rs.w[accepted])[q];
            if (f_acc) *f_acc = rs.f[accepted];
        }
        if constexpr (POLL) if (w == SPEC_PW) spec_poll_take(*poll->sm, pg, poll->ep, poll->seq);
        __syncthreads();
        if constexpr (POLL) {  // (sm.verdict is next written behind the next round's first barrier)
            const int v = __builtin_amdgcn_readfirstlane(poll->sm->verdict);  // decides exits (§7)
            if (v != 0) {
                *drop = v;
                break;
            }
        }
        REF_TS(rs.ts_n, 4);
        sc.lap(19);  // one speculated round
    }
    evals += it;
    if (HPE_STAMPS && blockIdx.x == 0 && t == 0) {  // decision statistics (diagnostic build)
        hpe_stamps[9] += (tk != 0) ? 1 : 0;
        hpe_stamps[30] += (unsigned long long)it;
        hpe_stamps[32 + 9] += 1;
    }
#if HPE_STAMPS
    if (t == 0 && !POLL) {  // every search of every block: {path bits, trials << 32, accepted << 40}
        const unsigned long long k = atomicAdd(&hpe_gold_log[0], 1ull);
        if (k < HPE_GOLD_LOG)
            hpe_gold_log[1 + k] = path | ((unsigned long long)it << 32) |
                                  ((unsigned long long)(tk != 0) << 40);
    }
#endif
    return tk;
}

// Grid 1 or 1 + PREP_WG: workgroup 0 refines the selected frame (do_refine != 0); the
// others, when present, prepare the NEXT frame meanwhile (hpe_prep.hpp) on
// CUs this single-workgroup refine leaves idle -- one launch, one stream, no cross-queue
// dependencies in the frame loop.
// MW (clouds > RF_STAGE_MAX): workgroups 1..mw.Q are the helpers of the multi-workgroup
// form above; the preparation workgroups follow them.
// RIGID: the hand-frame refine (rigid_wave, hpe_device.hpp): every evaluation of the call
// places its spheres as Rg q + u from centres q built once from x0's digit angles, the
// collision a constant of the call; HPE_REFINE_EXACT=1 selects the reference's chain.
// SPEC (STAGED, not MW): workgroup 1 is the runner of the speculated translation block (above)
// and the preparation workgroups follow it: grid 2 or 2 + PREP_WG.
template <bool STAGED, bool MW = false, bool RIGID = false, bool SPEC = false>
__global__ __launch_bounds__(RF_NT) void k_refine(double *__restrict__ x0g, const DevObs *__restrict__ og,
                                                  const DevHand *__restrict__ Hg,
                                                  int32_t *__restrict__ match_g,
                                                  int *__restrict__ evals_out, int do_refine,
                                                  PrepArgs pa, DevMw mw, DevPick pk, PrepSplit ps,
                                                  DevSpec sp) {
    static_assert(!SPEC || (STAGED && !MW), "the runner stages the cloud; no helpers");
    constexpr bool WIN = false;
    const DevWindow pw{};
    if constexpr (!SPEC) {
        constexpr bool RUNNER = false;
        SpecSm *const ssm_p = nullptr;
#include "hpe_refine_body.inc"
    } else {
        extern __shared__ __align__(16) unsigned char dyn[];  // staged cloud + matchId / prep
        __shared__ RefineSm rs;
        __shared__ DevHand hs;  // hand constants in LDS: keeps them out of the loop's registers
        __shared__ int mwflag;
        __shared__ SpecSm ssm;
        SpecSm *const ssm_p = &ssm;
        // the body once per role: the runner's copy, and the leader's and the preparation's
        auto body = [&](auto role) {
            constexpr bool RUNNER = decltype(role)::value;
#define HPE_REFINE_BODY_NO_DECLS
#include "hpe_refine_body.inc"
#undef HPE_REFINE_BODY_NO_DECLS
        };
        if (blockIdx.x == 1) body(std::true_type{});
        else body(std::false_type{});
    }
}

// ------------------------------------------------------------------ batched lanes
// hpe_track_batch_dev: B independent sequences in the same launches.  Lane = blockIdx.y; each
// kernel runs the body of the kernel it mirrors on its lane's state, so a lane computes what
// the single-sequence path computes, bit for bit.  The swarm stays BY VALUE in the arguments:
// the mutable arrays of all lanes are B identical arenas `stride` bytes apart, the argument
// holds lane 0's pointers, and a lane rebases them with scalar adds on the entry batch's
// words (no table of per-lane structs to load first).  normals, outl, bounds and the inbox
// counts are shared: every lane draws under the context's seed -- unless lane seeds are set
// (SEEDS below).  Lanes never communicate inside a frame; lane groups exchange rows after one
// (k_group_pick).
//
// One template per role -- k_pso_init_b, k_pso_gen_b, k_pso_init_wb, k_pso_gen_wb (pso_evolve in
// the workgroup and the wave form), k_pso_final_b, k_refine_lane, k_prepare_lane, k_window_b --
// and five independent axes, each a template parameter.  Every form of a role has one argument
// list; what a form does not read is passed null and never loaded.
//   SRC (LaneSrc): where the preparation workgroups find the lane's next raw frame.  They ride in
//     the refine launch, grid (1 + PREP_WG, B): workgroup (0, b) refines, (1.., b) run
//     prep_workgroup into the lane's other buffer, as k_refine's do.  All sources name the lane's
//     buffers, descriptors, scratch and hand-off counters (a 128-byte line of its own) by the
//     device table tab[parity][b] (PrepArgs; the kernels take tab + parity * HPE_BATCH_MAX).
//       NONE  no next frame: grid (1, B), do_refine the constant 1 (a prepared batch, and the
//             last frame of the others)
//       RAW   hpe_track_raw_batch_dev: frame cur[2 b] + 1 of the resident sequence raw_base[b]
//             (the cursor's slot word counts frames; k_pso_final_b advances it)
//       RING  hpe_track_batch_pipelined: tab[b].raw itself, the lane's pinned (mapped, coherent)
//             host buffer of the parity being prepared, read over PCIe inside the launch
//       U16   hpe_batch_pipeline_begin_u16: the ring holding unsigned 16-bit pixels, read in place
//             and multiplied by the batch's depth unit *unit -- device memory written at the
//             begin, never a captured argument (PrepArgsU16, hpe_prep.hpp)
//       VIEW  hpe_batch_pipeline_begin_view: the ring holding the lane's camera frame, 16-bit
//             pixels at the camera's resolution, read in place through the lane's view -- `unit`
//             names a ViewTab, the depth unit and the lanes' views behind it, device memory
//             written at the begin like the unit (PrepArgsView, hpe_prep.hpp)
//   WIN: hpe_set_batch_window.  The frame is read through the lane's window wtab[b] (the
//     DevWindow table next to the PrepArgs table, same parity offset), in the band workgroups and
//     the distance transform's mask alike (prep_workgroup<true>): the preparation of the frame
//     masked on the host.  One more independent load of the preparation workgroups alone.
//   PACED: hpe_set_batch_pacing(HPE_PACING_FREE).  The first statement tests the lane's activity
//     word act[lane] -- HPE_ACT_TRACK: the lane tracks its current frame in this call;
//     HPE_ACT_PREP: it prepares a next frame.  The host writes a call's 16 words on the stream
//     ahead of the frame's graph (k_lane_act): the graphs hold the table's address, never a mask.
//     One scalar load indexed by blockIdx, so the decision is workgroup-uniform; an idle
//     workgroup loads nothing through the lane's descriptor, state row, arena or table entries
//     (a lane that never held a frame has descriptors that name nothing), reaches no barrier,
//     counter or hand-off, and stores nothing -- but for lane 0's final workgroup, which
//     publishes the call's frame number whether or not lane 0 tracks.
//   HANDS: hpe_set_batch_hands.  The hand is entry blockIdx.y of the flat table (lane_hand).
//   SEEDS: hpe_set_batch_seeds, on the four roles that draw (k_pso_init_b, k_pso_gen_b,
//     k_pso_init_wb, k_pso_gen_wb).  The lane's normals, links, inbox counts and Philox key come
//     from per-lane device tables (lane_seeded); built in the HANDS shape alone, like PACED.
// The host names these combinations and no others (hpe_api.inc, the lane_*_kernel selectors):
// WIN needs a source; PACED is the live batch's, so RING, U16 or VIEW (or NONE, its ending frame), and
// is built in the HANDS shape alone -- the table holds the context's hand in every entry while
// no lane hands are set, which is pinned bit-identical to the !HANDS forms.
enum LaneSrc { LANE_SRC_NONE, LANE_SRC_RAW, LANE_SRC_RING, LANE_SRC_U16, LANE_SRC_VIEW };
#define HPE_ACT_TRACK 1
#define HPE_ACT_PREP 2
__device__ __forceinline__ DevSwarm lane_swarm(DevSwarm sw, size_t stride) {
    const size_t off = stride * blockIdx.y;
    sw.xh = (double *)((char *)sw.xh + off);
    sw.pch = (double *)((char *)sw.pch + off);
    sw.pb = (double *)((char *)sw.pb + off);
    sw.v = (double *)((char *)sw.v + off);
    sw.inbox = (double *)((char *)sw.inbox + off);
    sw.gmin = (unsigned long long *)((char *)sw.gmin + off);
    sw.sig = (Sig *)((char *)sw.sig + off);
    sw.gpos = (double *)((char *)sw.gpos + off);
    return sw;
}
// The lane's hand (hpe_set_batch_hands).  HANDS: entry blockIdx.y of the flat table the kernel
// receives where the kernel it mirrors receives the context's hand -- one scalar multiply-add on
// the argument word, like the arenas above.  !HANDS (no lane hands set: every entry is the
// context's hand): entry 0, the pointer as it came, and the kernel compiles as it did before
// there were lane hands.  (Indexing always cost nothing in itself, but the four scalar
// instructions at entry moved the compiler's schedule of the refine body: DESIGN.md 4.7.)
template <bool HANDS>
__device__ __forceinline__ const DevHand *lane_hand(const DevHand *__restrict__ tab) {
    return HANDS ? tab + blockIdx.y : tab;
}
// The lane's seed (hpe_set_batch_seeds).  SEEDS: what every lane shares under the context's seed
// -- the normals, the link table, the Philox key, and in the workgroup form the inbox counts --
// is the lane's own: the host lays B copies of normals and outl out back to back (lane 0's in the
// argument, as the arenas), so a lane rebases them by scalar multiply-adds on P and G, and takes
// its seed and its counts [lane][g] from the device table `ls`.  sw.K is the largest K over the
// lanes' seeds: it sizes and addresses the inbox alone -- outl names (receiver, slot) -- so a
// lane's values do not depend on it.  !SEEDS: the swarm as it came, `ls` never loaded, and the
// kernel compiles as it did before there were lane seeds.  The SEEDS forms are built in the HANDS
// shape alone, as the PACED ones are.
struct LaneSeeds {
    unsigned long long seed[16];
    const InboxCounts *kin;  // [lane][g], g = 0..G
};
static_assert(HPE_BATCH_MAX == 16, "LaneSeeds holds one seed per lane");
template <bool SEEDS>
__device__ __forceinline__ DevSwarm lane_seeded(DevSwarm sw, const LaneSeeds *__restrict__ ls) {
    if (SEEDS) {
        sw.normals += (size_t)sw.P * HPE_DOF * blockIdx.y;
        sw.outl += (size_t)(sw.G + 1) * sw.P * 6 * blockIdx.y;
        sw.seed = ls->seed[blockIdx.y];
    }
    return sw;
}
#define HPE_STATE_N (HPE_DOF + 1)  // {x0 -> bestp, cost} of one lane
#define HPE_EVALS_N 4              // a lane's refine evaluation counter {last, -, total (u64)}

// states: B x 27; obs: B descriptors, lane b's current frame (k_seq_begin_b / k_pso_final_b)
template <bool FILT, bool HANDS, bool PACED, bool SEEDS = false>
__global__ __launch_bounds__(HPE_NT) void k_pso_init_b(DevSwarm sw, size_t stride,
                                                       const double *__restrict__ states,
                                                       const DevObs *__restrict__ obs,
                                                       const DevHand *__restrict__ Hg,
                                                       const int *__restrict__ act,
                                                       const LaneSeeds *__restrict__ ls) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(HANDS || !SEEDS, "the seeded forms index the hand table");
    if (PACED && !(act[blockIdx.y] & HPE_ACT_TRACK)) return;
    pso_init_body<HPE_NT, FILT>(lane_swarm(lane_seeded<SEEDS>(sw, ls), stride),
                                states + (size_t)HPE_STATE_N * blockIdx.y, obs + blockIdx.y,
                                lane_hand<HANDS>(Hg));
}

// SEEDS: the inbox counts are the lane's, entry [lane][g] of the device table, not the by-value
// argument (which the host then leaves zero and the kernel never reads).
template <bool ROW16, bool FILT, bool HANDS, bool PACED, bool SEEDS = false>
__global__ __launch_bounds__(HPE_NT) void k_pso_gen_b(DevSwarm sw, size_t stride,
                                                      const DevObs *__restrict__ obs,
                                                      const DevHand *__restrict__ Hg, int g,
                                                      double W1, double C1, double C2,
                                                      InboxCounts kin,
                                                      const int *__restrict__ act,
                                                      const LaneSeeds *__restrict__ ls) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(HANDS || !SEEDS, "the seeded forms index the hand table");
    if (PACED && !(act[blockIdx.y] & HPE_ACT_TRACK)) return;
    if constexpr (SEEDS)
        pso_gen_body<HPE_NT, false, ROW16, FILT>(lane_swarm(lane_seeded<true>(sw, ls), stride),
                                                 obs + blockIdx.y, lane_hand<HANDS>(Hg), g, W1, C1, C2,
                                                 ls->kin[(size_t)(sw.G + 1) * blockIdx.y + g]);
    else
        pso_gen_body<HPE_NT, false, ROW16, FILT>(lane_swarm(sw, stride), obs + blockIdx.y, lane_hand<HANDS>(Hg),
                                                 g, W1, C1, C2, kin);
}

// k_pso_final's TAIL form on the lane's cursor cur[2 b] = {slot, row}: the row indexes hist
// over all lanes (lane b starts at row b n), and the next slot's descriptor is staged into
// obs[b].  The arguments are k_pso_final's own (the host passes same_eval = 1 and no
// selected-frame hand-back, pipeline counter or refine failure flag), so the body compiles as
// it does there.
// LIVE (the live batch): the cursor may be null (no cursor, history or slot table), and the
// batch's frame counter seq_b (published to done_host for the host's wait before it refills a
// pinned buffer) is bumped by lane 0's workgroup alone -- once per frame, not B times on one
// word.  One counter serves the batch: the refine launch of every lane, which read the pinned
// buffers, has retired before any workgroup of this launch starts.  blockIdx.y is uniform, and
// the body's counter branch reaches no barrier.
// PACED: publication does not depend on lane 0 being active.  When lane 0 idles, its workgroup
// bumps the counter and stores it to done_host as the body's first statement would (the same
// wave, the same stores), then leaves -- once per call, even when no lane tracks, so the host's
// wait on this parity's frame number always ends.
template <bool FILT, bool HANDS, bool LIVE, bool PACED, bool TAIL = true>
__global__ __launch_bounds__(HPE_NT) void k_pso_final_b(DevSwarm sw, size_t stride,
                                                        double *__restrict__ states, DevObs *obs,
                                                        const DevHand *__restrict__ hands,
                                                        DevObs *__restrict__ obs_out, int same_eval,
                                                        unsigned long long *__restrict__ seq_b,
                                                        unsigned long long *done_host,
                                                        double *__restrict__ hist,
                                                        const int *__restrict__ fail,
                                                        const DevObs *__restrict__ seq_table,
                                                        int *__restrict__ cur,
                                                        const int *__restrict__ act) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(LIVE || !PACED, "only a live batch is paced");
    if (PACED && !(act[blockIdx.y] & HPE_ACT_TRACK)) {
        if (blockIdx.y == 0 && threadIdx.x == HPE_NT - 64) {
            const unsigned long long n = *seq_b + 1;
            *seq_b = n;
            __hip_atomic_store(done_host, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const DevHand *__restrict__ const Hg = lane_hand<HANDS>(hands);
    sw = lane_swarm(sw, stride);
    double *__restrict__ const out = states + (size_t)HPE_STATE_N * blockIdx.y;
    DevObs *const seq_obs = obs + blockIdx.y;  // aliases og
    const DevObs *const og = seq_obs;
    int *__restrict__ const seq_cur = LIVE && !cur ? nullptr : cur + 2 * blockIdx.y;
    unsigned long long *__restrict__ const seq_dev = LIVE && blockIdx.y != 0 ? nullptr : seq_b;
#include "hpe_final_body.inc"
}

// Start of a batch call: lane b's first descriptor staged, its cursor at {first slot, row b n}.
struct BatchFirst {
    int slot[16];
};
__global__ void k_seq_begin_b(const DevObs *__restrict__ table, BatchFirst first, int n,
                              DevObs *__restrict__ obs, int *__restrict__ cur) {
    const int t = threadIdx.x, b = blockIdx.y;
    if (t < (int)(sizeof(DevObs) / 8))
        ((unsigned long long *)(obs + b))[t] = ((const unsigned long long *)(table + first.slot[b]))[t];
    if (t == 0) {
        cur[2 * b] = first.slot[b];
        cur[2 * b + 1] = b * n;
    }
}

// Start of a raw batch call: lane b's raw base, its cursor at {frame 0, row b n}.  Frame 0 goes
// to buffer parity 0 (k_prepare_lane below).
struct BatchRaw {
    const float *raw[16];
};
__global__ void k_raw_begin_b(BatchRaw first, int n, const float **__restrict__ raw_base,
                              int *__restrict__ cur) {
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        raw_base[b] = first.raw[b];
        cur[2 * b] = 0;
        cur[2 * b + 1] = b * n;
    }
}

// The preparation of lane blockIdx.y from source SRC: its table entry, and with it RAW: on raw
// frame cur + next (three independent loads); RING: nothing else; U16: the depth unit; VIEW: the
// unit and the lane's view, two more independent loads.  Only the preparation workgroups call it.
template <LaneSrc SRC>
__device__ __forceinline__ auto lane_prep(const PrepArgs *__restrict__ tab,
                                          const float *__restrict__ unit,
                                          const float *const *__restrict__ raw_base,
                                          const int *__restrict__ cur, int next) {
    // (each branch is the statements its forms were measured with -- the lane signed here,
    // unsigned below; the entry copied whole here, assigned below: DESIGN.md 4.7)
    if constexpr (SRC == LANE_SRC_RAW) {
        const int b = blockIdx.y;
        PrepArgs a = tab[b];
        a.raw = raw_base[b] + (size_t)(cur[2 * b] + next) * a.raw_stride;
        a.raw_row = nullptr;  // a.raw is the frame itself
        return a;
    } else if constexpr (SRC == LANE_SRC_U16) {
        PrepArgsU16 a;
        static_cast<PrepArgs &>(a) = tab[blockIdx.y];
        a.unit = *unit;
        return a;
    } else if constexpr (SRC == LANE_SRC_VIEW) {
        const ViewTab *__restrict__ const vt = (const ViewTab *)unit;
        PrepArgsView a;
        static_cast<PrepArgs &>(a) = tab[blockIdx.y];
        a.unit = vt->unit;
        a.view = vt->view[blockIdx.y];
        return a;
    } else {
        return tab[blockIdx.y];
    }
}

// k_prepare for every lane's first frame of a call (RAW: the frame at its cursor), grid
// (PREP_WG, B); PACED: only the lanes given a first frame prepare one
template <LaneSrc SRC, bool WIN, bool PACED>
__global__ __launch_bounds__(PREP_NT) void k_prepare_lane(const PrepArgs *__restrict__ tab,
                                                          const DevWindow *__restrict__ wtab,
                                                          const int *__restrict__ act,
                                                          const float *__restrict__ unit,
                                                          const float *const *__restrict__ raw_base,
                                                          const int *__restrict__ cur) {
    static_assert(SRC != LANE_SRC_NONE, "a preparation has a source");
    __shared__ __align__(16) unsigned char lds[prep_lds_bytes()];
    if (PACED && !(act[blockIdx.y] & HPE_ACT_PREP)) return;
    DevWindow pw{};
    if (WIN) pw = wtab[blockIdx.y];
    prep_workgroup<WIN>(lane_prep<SRC>(tab, unit, raw_base, cur, 0), blockIdx.x, lds, nullptr, &pw);
}

// The single-workgroup staged refine, one workgroup per lane: no exchange pick, no helpers.
// With a source, workgroups (1.., b) prepare the lane's next frame (do_refine = 0: the
// preparation only); workgroup (0, b) reads what it reads without one.  PACED: workgroup (0, b)
// runs iff the lane tracks, the preparation workgroups iff it prepares -- all nine or none, so an
// idle preparation never touches the lane's three hand-off counters, and a preparation that
// runs finds them as the last one left them.
template <bool RIGID, bool HANDS, LaneSrc SRC, bool WIN, bool PACED, bool STAGED = true, bool MW = false>
__global__ __launch_bounds__(RF_NT) void k_refine_lane(double *__restrict__ states,
                                                       const DevObs *__restrict__ obs,
                                                       const DevHand *__restrict__ hands,
                                                       int *__restrict__ evals_b, int do_refine_arg,
                                                       const PrepArgs *__restrict__ tab,
                                                       const DevWindow *__restrict__ wtab,
                                                       const int *__restrict__ act,
                                                       const float *__restrict__ unit,
                                                       const float *const *__restrict__ raw_base,
                                                       const int *__restrict__ cur) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(SRC != LANE_SRC_NONE || !WIN, "a window is the preparation's");
    if (PACED && !(act[blockIdx.y] & (SRC == LANE_SRC_NONE || blockIdx.x == 0 ? HPE_ACT_TRACK
                                                                              : HPE_ACT_PREP)))
        return;
    const DevHand *__restrict__ const Hg = lane_hand<HANDS>(hands);
    double *__restrict__ const x0g = states + (size_t)HPE_STATE_N * blockIdx.y;
    const DevObs *__restrict__ const og = obs + blockIdx.y;
    int32_t *const match_g = nullptr;  // the staged form keeps matchId in LDS
    int *__restrict__ const evals_out = evals_b + HPE_EVALS_N * blockIdx.y;
    const int do_refine = SRC == LANE_SRC_NONE ? 1 : do_refine_arg;
    decltype(lane_prep<SRC>(tab, unit, raw_base, cur, 1)) pa{};
    DevWindow pw{};
    if (SRC != LANE_SRC_NONE && blockIdx.x >= 1) {
        pa = lane_prep<SRC>(tab, unit, raw_base, cur, 1);
        if (WIN) pw = wtab[blockIdx.y];
    }
    const DevMw mw{};
    const DevPick pk{};
    const PrepSplit ps{};
    constexpr bool SPEC = false, RUNNER = false;  // lanes keep the one-workgroup body
    const DevSpec sp{};
    SpecSm *const ssm_p = nullptr;
#include "hpe_refine_body.inc"
}
static_assert(PREP_NT == RF_NT, "the preparation workgroups ride in the refine launch");

// The pose rule (include/hpe.h): the window of the context hand at pose th[0..25], by one wave.
// FK is fk_wave, as k_build runs it, so the centres are hpe_build_spheres' bit for bit; lane
// j < 48 takes sphere j in camera coordinates (y and z un-negated), every product rounded
// before its add, and the wave takes minima and maxima, which are order-free.  Any non-finite
// coordinate or z <= 0: the whole frame.  Lane 0 adds the depth bounds in raw units
// (win_raw_bounds) and stores the window (plain vector stores).
struct WinPar {
    double margin_xy, margin_z, focal;
    int to_cm, pad;  // the frames' unit conversion: the window's depth bounds in raw units
};
__device__ __forceinline__ double wave_min_f64(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ void window_wave(FkSm &f, const DevHand *__restrict__ H,
                                            const WinPar &par, DevWindow *__restrict__ out) {
    const int l = threadIdx.x & 63;
    fk_wave(f, H);
    const int j = l < HPE_NS ? l : HPE_NS - 1;  // lanes >= 48 repeat sphere 47: no effect on min / max
    const double x = f.S[j][0], y = f.S[j][1] * -1, z = f.S[j][2] * -1, R = H->radii[j];
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && z > 0;
    const bool open = __ballot(!ok) != 0ull;
    const double e = R + par.margin_xy, ez = R + par.margin_z;
    const double cl = floor((par.focal * (x - e) + 160.0 * z) / z);
    const double ch = floor((par.focal * (x + e) + 160.0 * z) / z);
    const double rl = floor((par.focal * (y - e) + 120.0 * z) / z);
    const double rh = floor((par.focal * (y + e) + 120.0 * z) / z);
    const double cmin = wave_min_f64(cl), cmax = wave_max_f64(ch);
    const double rmin = wave_min_f64(rl), rmax = wave_max_f64(rh);
    const double zmin = wave_min_f64(z - ez), zmax = wave_max_f64(z + ez);
    if (l == 0) {
        DevWindow w{};
        w.row_lo = open ? 0 : (int)fmin(fmax(rmin, 0.0), (double)HPE_IMG_H);
        w.row_hi = open ? HPE_IMG_H - 1 : (int)fmin(fmax(rmax, -1.0), (double)(HPE_IMG_H - 1));
        w.col_lo = open ? 0 : (int)fmin(fmax(cmin, 0.0), (double)HPE_IMG_W);
        w.col_hi = open ? HPE_IMG_W - 1 : (int)fmin(fmax(cmax, -1.0), (double)(HPE_IMG_W - 1));
        w.z_lo = open ? -__builtin_inf() : zmin;
        w.z_hi = open ? __builtin_inf() : zmax;
        win_raw_bounds(w, par.to_cm);
        *out = w;
    }
}

// HPE_WINDOW_FOLLOW: lane blockIdx.x's window from the pose its state holds now, into entry
// blockIdx.x of wout (the table of the parity the NEXT refine launch prepares into).  One wave
// per lane, a launch of its own before that refine launch: its refine workgroup overwrites the
// state at its end, so the preparation workgroups riding in it cannot read the pose themselves;
// the hand-off is the kernel boundary.  hpe_window_from_pose and hpe_lane_window_from_pose run
// the !HANDS form on one pose, with the hand they name as Hg.
// PACED (this kernel's lane dimension is x): the window of a lane that accepts no frame in this
// call stays as it was, and its state row -- a joining lane's may hold anything -- is not read.
template <bool HANDS, bool PACED>
__global__ __launch_bounds__(64) void k_window_b(const double *__restrict__ states,
                                                 const DevHand *__restrict__ Hg,
                                                 const WinPar *__restrict__ par,
                                                 DevWindow *__restrict__ wout,
                                                 const int *__restrict__ act) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    if (PACED && !(act[blockIdx.x] & HPE_ACT_PREP)) return;
#include "hpe_window_body.inc"
}

// ------------------------------------------------------------------ wave-form lanes
// hpe_set_batch_form(HPE_BATCH_FORM_WAVE): the lanes' pso_evolve in the wave-per-particle form,
// grid (ceil(P / (PW_WPB / WPP)), B).  A workgroup's particles belong to one lane (blockIdx.y),
// so it stages the hand once and reads one descriptor and one x0; each kernel runs the body of
// the kernel it mirrors (the same text) on its lane's arena, which here has the compact
// informant array ibtc too: the ninth array of a lane's arena, rebased like the other eight.
// No exchange form: lanes never communicate.  The final kernel is k_pso_final_b's with
// same_eval = 0 (it evaluates cal_cost(bestp) itself, as after k_pso_gen_w).
__device__ __forceinline__ DevSwarm lane_swarm_w(DevSwarm sw, size_t stride) {
    const size_t off = stride * blockIdx.y;
    sw = lane_swarm(sw, stride);
    sw.ibtc = (double *)((char *)sw.ibtc + off);
    return sw;
}

template <int WPP, bool COOP, bool HANDS, bool PACED, bool SEEDS = false>
__global__ __launch_bounds__(PW_NT) void k_pso_init_wb(DevSwarm sw, size_t stride,
                                                       const double *__restrict__ states,
                                                       const DevObs *__restrict__ obs,
                                                       const DevHand *__restrict__ hands,
                                                       const int *__restrict__ act,
                                                       const LaneSeeds *__restrict__ ls) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(HANDS || !SEEDS, "the seeded forms index the hand table");
    if (PACED && !(act[blockIdx.y] & HPE_ACT_TRACK)) return;
    const DevHand *__restrict__ const Hg = lane_hand<HANDS>(hands);
    sw = lane_swarm_w(lane_seeded<SEEDS>(sw, ls), stride);
    const double *__restrict__ const x0 = states + (size_t)HPE_STATE_N * blockIdx.y;
    const DevObs *__restrict__ const og = obs + blockIdx.y;
#include "hpe_wave_init_body.inc"
}

template <bool ROW16, int WPP, bool COOP, bool HANDS, bool PACED, bool SEEDS = false>
__global__ __launch_bounds__(PW_NT, WPP == 2 ? 2 : 4) void k_pso_gen_wb(DevSwarm sw, size_t stride,
                                                      const DevObs *__restrict__ obs,
                                                      const DevHand *__restrict__ hands, int g,
                                                      double W1, double C1, double C2,
                                                      const int *__restrict__ act,
                                                      const LaneSeeds *__restrict__ ls) {
    static_assert(HANDS || !PACED, "the idle-aware forms index the hand table");
    static_assert(HANDS || !SEEDS, "the seeded forms index the hand table");
    if (PACED && !(act[blockIdx.y] & HPE_ACT_TRACK)) return;
    const DevHand *__restrict__ const Hg = lane_hand<HANDS>(hands);
    constexpr bool XCH = false;  // no exchange inside a batch
    sw = lane_swarm_w(lane_seeded<SEEDS>(sw, ls), stride);
    const DevObs *__restrict__ const og = obs + blockIdx.y;
#include "hpe_wave_gen_body.inc"
}

// ------------------------------------------------------------------ lane pacing
// The activity words the PACED forms test (HPE_ACT_TRACK, HPE_ACT_PREP above)
struct LaneAct {
    int word[16];
};
static_assert(HPE_BATCH_MAX == 16, "LaneAct holds one word per lane");
// One call's activity words, by value (as k_seq_begin_b takes its slots)
__global__ void k_lane_act(LaneAct a, int *__restrict__ act) {
    const int t = threadIdx.x;
    if (t < HPE_BATCH_MAX) act[t] = a.word[t];
}

// ------------------------------------------------------------------ lane groups
// hpe_set_batch_groups: runs of consecutive lanes that track one stream as independent subswarms
// and carry the best of their results to the next frame -- the subswarm exchange's per-frame pick
// (k_pick_best, hpe/dist.py pick_best) between lanes, with no communicator.  One wave per lane
// after the frame's final launch and ahead of k_report_b (the kernel boundary is the hand-off: no
// counter, no spin); the wave of a group's first lane works, the others return at entry.  It
//   copies each of the group's rows of `states` -- what k_pso_final_b just wrote, the lane's own
//     {bestp, cost} -- into the own-rows table `own` (null: hpe_batch_group_pick, which picks
//     among arbitrary rows and leaves the table alone),
//   picks by pick_best_row: the smallest cost, NaN as +inf, ties to the lowest lane, an all-NaN
//     group its lowest lane, and
//   stores the picked row into every row of the group in `states` and, inside a resident call
//     (hist, cur), into each lane's history row of this frame: row cur[2 b + 1] - 1 of the row
//     cursor, which the final kernel has already advanced (as pick_apply).
// The groups are device memory the host writes while the stream is drained (the graphs hold the
// table's address, never a group).  act (a free-paced batch): a group idles as one -- the host
// refuses a split group -- so its first lane's word decides, and an idle group loads and stores
// nothing else.  Lane l < 27 of the wave carries column l of every row it loads before the first
// store of that column; the picked row's load depends on every cost, so no store of the wave
// precedes a load another lane still needs.  Plain vector stores.
struct LaneGroups {
    int first[16];  // lane b's group begins at lane first[b] ...
    int size[16];   // ... and holds size[b] lanes
};
static_assert(HPE_BATCH_MAX == 16, "LaneGroups holds one entry per lane");
__global__ __launch_bounds__(64) void k_group_pick(double *states, double *__restrict__ own,
                                                   double *__restrict__ hist, const int *__restrict__ cur,
                                                   const LaneGroups *__restrict__ grp,
                                                   const int *__restrict__ act) {
    const int b = blockIdx.x, l = threadIdx.x;
    if (grp->first[b] != b) return;
    if (act && !(act[b] & HPE_ACT_TRACK)) return;
    const int n = grp->size[b];
    double *const rows = states + (size_t)HPE_STATE_N * b;
    const int w = pick_best_row(rows, n, l);
    if (l > HPE_DOF) return;
    const double x = rows[(size_t)HPE_STATE_N * w + l];
    if (own)
        for (int m = 0; m < n; ++m) own[(size_t)HPE_STATE_N * (b + m) + l] = rows[(size_t)HPE_STATE_N * m + l];
    for (int m = 0; m < n; ++m) {
        rows[(size_t)HPE_STATE_N * m + l] = x;
        if (hist && cur) hist[(size_t)HPE_STATE_N * (cur[2 * (b + m) + 1] - 1) + l] = x;
    }
}

// ------------------------------------------------------------------ lane reports
// hpe_set_batch_report: what the host needs of a tracked lane, computed and delivered by one wave
// per lane after the frame's final launch (the kernel boundary is the hand-off: no counter, no
// spin) -- the state row, the hand's 21 joints under the lane's hand, their pixel positions and
// the lane's health, into the lane's ring in pinned host memory (hpe_report.hpp: the layout and
// the host reader).
//
// joints_wave: hand_joints and their projection at pose f.th, by one wave.  FK is fk_wave, as
// k_build runs it, and the 63 values are gathered as k_build gathers them, so jt is
// hpe_build_spheres' joints_out bit for bit.  Lane j < 21 then projects joint j by the pose
// rule's projection (window_wave) without the floor and the margins: hand_joints is not negated,
// so x, y, z are camera coordinates; every product is rounded before its add; a non-finite
// coordinate or z <= 0 gives NaN for both.  Returns {column, row} of joint l in lanes l < 21.
struct JointPx {
    double col, row;
};
__device__ __forceinline__ JointPx joints_wave(FkSm &f, const DevHand *__restrict__ H, double focal,
                                               double *__restrict__ jt) {
    const int l = threadIdx.x & 63;
    fk_wave(f, H);
    __syncthreads();  // (one wave: the joints fk_wave's lanes stored, before other lanes read them)
    if (l < 63) {  // hand_joints rows: wrist, index..little joints 1-4, thumb 1-4 (k_build)
        double v;
        if (l < 3) v = f.th[3 + l];
        else {
            const int row = l / 3, c = l % 3, k = (row - 1) / 4, jr = 1 + (row - 1) % 4;
            const int d = (k < 4) ? k + 1 : 0;
            v = f.J[d][jr][c];
        }
        jt[l] = v;
    }
    __syncthreads();
    const int j = l < 21 ? l : 20;
    const double x = jt[3 * j], y = jt[3 * j + 1], z = jt[3 * j + 2];
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && z > 0;
    JointPx p;
    p.col = ok ? (focal * x + 160.0 * z) / z : __builtin_nan("");
    p.row = ok ? (focal * y + 120.0 * z) / z : __builtin_nan("");
    return p;
}
// Stage lane hand `src` and the 26 angles of `row` for joints_wave (one wave).
__device__ __forceinline__ void joints_stage(DevHand &hs, FkSm &f, const DevHand *__restrict__ src,
                                             const double *__restrict__ row) {
    const int l = threadIdx.x & 63;
    for (int q = l; q < (int)(sizeof(DevHand) / 8); q += 64) ((double *)&hs)[q] = gp((const double *)src)[q];
    if (l < HPE_DOF) f.th[l] = gp(row)[l];
}

// The reports' device words: the watch rule, the ring depth and the batch's focal (written by
// the begin, the stream drained), and per lane the report counter and the bad streak.
struct RepPar {
    double cost_max, focal;
    int n_min, streak, depth, pad;
};
struct RepDev {
    unsigned long long *ring;      // [HPE_BATCH_MAX][HPE_REP_DEPTH_MAX] slots (the host ring's device address)
    const RepPar *par;
    unsigned long long *lane_seq;  // [HPE_BATCH_MAX]
    int *streak;                   // [HPE_BATCH_MAX]
};
// Grid B, one wave per lane: sibling of k_window_b.  act (null in lockstep): a lane whose
// HPE_ACT_TRACK bit is clear returns at entry, and so does a lane outside `sel` (a by-value word,
// as k_lane_act takes its words: the lanes hpe_batch_pipeline_optimise selected; the frame graphs
// hold the constant all-lanes word) -- it loads and stores nothing else.  The hand table holds
// the context's hand in every entry while no lane hands are set, so entry `lane` is the lane's
// hand either way.  info: the preparation's records of the frame just tracked (kind TRACK: the
// buffer parity the final launch used) or currently prepared (INIT) -- n is its n_full, the points
// the preparation found before downsampling: the descriptor's own n is 250 for every downsampled
// frame, an empty one included, and a live batch always downsamples.  frame_no: the batch's frame
// counter, which a TRACK frame's final launch has already bumped.
// Publication, at system scope: lane 0 stores begin = seq; release; the payload by plain 8-byte
// vector stores spread over the wave; the wave waits for its own stores, takes a release fence
// and waits again (the wait AFTER the fence: the fence's own wait may be dropped); lane 0 stores
// end = seq.  One wave owns the whole slot, so its own vmcnt covers every payload store.
__global__ __launch_bounds__(64) void k_report_b(const double *__restrict__ states,
                                                 const DevHand *__restrict__ hands,
                                                 const PrepInfo *__restrict__ info,
                                                 const unsigned long long *__restrict__ frame_no,
                                                 RepDev rd, const int *__restrict__ act,
                                                 unsigned sel, int kind) {
    const int b = blockIdx.x, l = threadIdx.x;
    if (act && !(act[b] & HPE_ACT_TRACK)) return;
    if (!(sel >> b & 1)) return;
    __shared__ DevHand hs;
    __shared__ FkSm fk;
    __shared__ double jt[64];
    const double *__restrict__ const row = states + (size_t)HPE_STATE_N * b;
    joints_stage(hs, fk, hands + b, row);
    const double sv = gp(row)[l < HPE_STATE_N ? l : HPE_STATE_N - 1];  // lanes < 27: the state row
    const RepPar par = *rd.par;
    const int n = gp(info + b)->n_full;
    const unsigned long long call = *gp(frame_no);
    const unsigned long long seq = gp(rd.lane_seq)[b] + 1;
    const int streak_was = gp(rd.streak)[b];
    __syncthreads();
    const JointPx px = joints_wave(fk, &hs, par.focal, jt);
    const double cost = __shfl(sv, HPE_DOF);
    const bool nan = __ballot(l < HPE_STATE_N && !isfinite(sv)) != 0ull;
    const bool suspect = kind == HPE_REPORT_TRACK && (!(cost <= par.cost_max) || n < par.n_min);
    const int bad = suspect ? streak_was + 1 : 0;
    const int flags = (nan ? HPE_REPORT_F_NAN : 0) | (n == 0 ? HPE_REPORT_F_EMPTY : 0) |
                      (suspect ? HPE_REPORT_F_SUSPECT : 0) |
                      (suspect && par.streak > 0 && bad >= par.streak ? HPE_REPORT_F_LOST : 0);
    if (l == 0) {
        rd.lane_seq[b] = seq;
        rd.streak[b] = bad;
    }
    typedef HPE_GAS unsigned long long gu64;
    typedef HPE_GAS double gf64;
    gu64 *const slot = (gu64 *)rd.ring + ((size_t)b * HPE_REP_DEPTH_MAX + (size_t)((seq - 1) % (unsigned)par.depth)) *
                                             (HPE_REP_SLOT / 8);
    if (l == 0) __hip_atomic_store(slot, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    gu64 *const rep = slot + 1;  // hpe_lane_report: 5 header words, state, joints, px
    if (l < 5) {
        const unsigned long long hw = l == 0   ? seq
                                      : l == 1 ? call
                                      : l == 2 ? ((unsigned long long)(unsigned)kind << 32) | (unsigned)b
                                      : l == 3 ? ((unsigned long long)(unsigned)flags << 32) | (unsigned)n
                                               : (unsigned long long)(unsigned)bad;
        rep[l] = hw;
    }
    if (l < HPE_STATE_N) ((gf64 *)rep)[5 + l] = sv;
    if (l < 63) ((gf64 *)rep)[5 + HPE_STATE_N + l] = jt[l];
    if (l < 21) {
        ((gf64 *)rep)[5 + HPE_STATE_N + 63 + 2 * l] = px.col;
        ((gf64 *)rep)[5 + HPE_STATE_N + 63 + 2 * l + 1] = px.row;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (l == 0)
        __hip_atomic_store(slot + 1 + HPE_REP_WORDS, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static_assert(5 + HPE_STATE_N + 63 + 42 == HPE_REP_WORDS, "the report's words");

// hpe_lane_joints_dev: the same device function over a history, grid (n, B), one wave per row:
// row b n + f of hist under lane b's hand, to joints[b][f][21][3] and (px non-null) px[b][f][21][2].
__global__ __launch_bounds__(64) void k_lane_joints_b(const double *__restrict__ hist,
                                                      const DevHand *__restrict__ hands, double focal,
                                                      double *__restrict__ joints,
                                                      double *__restrict__ px) {
    __shared__ DevHand hs;
    __shared__ FkSm fk;
    __shared__ double jt[64];
    const int l = threadIdx.x;
    const size_t r = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    joints_stage(hs, fk, hands + blockIdx.y, hist + r * HPE_STATE_N);
    __syncthreads();
    const JointPx p = joints_wave(fk, &hs, focal, jt);
    if (l < 63) joints[r * 63 + l] = jt[l];
    if (px && l < 21) {
        px[r * 42 + 2 * l] = p.col;
        px[r * 42 + 2 * l + 1] = p.row;
    }
}

// ------------------------------------------------------------------ lane location
#include "hpe_locate.hpp"

// ------------------------------------------------------------------ lane cleaning
#include "hpe_clean.hpp"

#include "hpe_optimise.hpp"

// ------------------------------------------------------------------ synthetic frames
__global__ void k_render(const double *__restrict__ S, const DevHand *__restrict__ H,
                         double focal, float *__restrict__ out) {
    __shared__ double C[HPE_NS][4];
    const int t = threadIdx.x;
    if (t < HPE_NS) {  // back to the camera frame (un-negate y, z)
        C[t][0] = S[3 * t];
        C[t][1] = -S[3 * t + 1];
        C[t][2] = -S[3 * t + 2];
        C[t][3] = H->radii[t];
    }
    __syncthreads();
    const int pix = blockIdx.x * blockDim.x + t;
    if (pix >= HPE_IMG_H * HPE_IMG_W) return;
    const int r = pix / HPE_IMG_W, c = pix % HPE_IMG_W;
    const double dx = (c - 160.0) / focal, dy = (r - 120.0) / focal;
    const double dd = dx * dx + dy * dy + 1.0;
    double best = __builtin_inf();
    for (int j = 0; j < HPE_NS; ++j) {
        const double b = dx * C[j][0] + dy * C[j][1] + C[j][2];
        const double cc = (C[j][0] * C[j][0] + C[j][1] * C[j][1] + C[j][2] * C[j][2]) -
                          C[j][3] * C[j][3];
        const double disc = b * b - dd * cc;
        if (disc >= 0) {
            const double tt = (b - sqrt(disc)) / dd;
            if (tt > 0 && tt < best) best = tt;
        }
    }
    out[pix] = (best < __builtin_inf()) ? (float)(best * 10.0) : 0.0f;
}

#if HPE_STAMPS
// Diagnostic build only: per-block k_pso_gen stamps, then cleared (not part of include/hpe.h).
extern "C" int hpe_debug_blk_ts(unsigned long long *out) {
    if (!out) return HPE_E_ARG;
    const size_t nb = sizeof(unsigned long long) * BT_GENS * BT_BLK * BT_PTS;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hpe_blk_ts), nb, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return HPE_E_HIP;
    std::vector<unsigned long long> z(BT_GENS * BT_BLK * BT_PTS, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(hpe_blk_ts), z.data(), nb, 0, hipMemcpyHostToDevice) != hipSuccess)
        return HPE_E_HIP;
    return HPE_OK;
}
// Diagnostic build only: the refine timeline of the last frame, then cleared.
extern "C" int hpe_debug_ref_ts(unsigned long long *out) {
    if (!out) return HPE_E_ARG;
    const size_t nb = sizeof(unsigned long long) * RT_LOG;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hpe_ref_ts), nb, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return HPE_E_HIP;
    std::vector<unsigned long long> z(RT_LOG, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(hpe_ref_ts), z.data(), nb, 0, hipMemcpyHostToDevice) != hipSuccess)
        return HPE_E_HIP;
    return HPE_OK;
}
// Diagnostic build only: the Goldstein decision log (not part of include/hpe.h).
extern "C" int hpe_debug_gold_log(unsigned long long *out, int n) {
    if (!out || n < 1) return HPE_E_ARG;
    if (n > HPE_GOLD_LOG + 1) n = HPE_GOLD_LOG + 1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hpe_gold_log), sizeof(unsigned long long) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return HPE_E_HIP;
    const unsigned long long z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(hpe_gold_log), &z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess)
        return HPE_E_HIP;
    return HPE_OK;
}
#endif

extern "C" int hpe_debug_stamps(unsigned long long *out64) {
    if (!out64) return HPE_E_ARG;
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(hpe_stamps), sizeof(unsigned long long) * 64, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return HPE_E_HIP;
    unsigned long long z[64] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(hpe_stamps), z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess)
        return HPE_E_HIP;
    return HPE_STAMPS;
}

#include "hpe_api.inc"
