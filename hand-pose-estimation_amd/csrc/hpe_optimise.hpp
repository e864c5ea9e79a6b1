// hpe_optimise.hpp -- pso_optimise (PSO.cpp:539-712) on the device.
// Included by hpe_kernels.hip after k_refine: it reuses RefineSm and gold_tree.
//
// One generation is two launches over P workgroups (one particle each):
//   k_opt_descent  ten single-coordinate descent steps per particle (:592-639): f_k,
//                  cal_gradient on coordinate permu(m) (:380-405, two waves), the
//                  speculated Goldstein tree, the step and the pbest update;
//                  check_constraints; then gbest <- particles.col(argmin pcost) (:643-650)
//   k_opt_move     the global-best velocity / position update with w, c1, c2 (:652-677),
//                  cal_cost (:679-689), pbest, then gbest / count (:692-704)
// The gbest update at the end of each phase is done by the last workgroup to arrive
// (release / acquire at agent scope, hpe_prep.hpp:prep_arrive_last), so no extra launch.
// The kernels' statements are text of their own (hpe_opt_*_body.inc): the lane forms at the
// end of this file include the same text.
//
// Evaluations that the serial code repeats on identical inputs are reused, bitwise:
//   * f_k of step m >= 1 is cal_cost2(theta, matchId, false) of the theta and matchId
//     the previous step ended with -- the value that step's f_k update computed;
//   * the post-step cal_cost2 of a step m >= 1 equals the accepted Goldstein trial
//     (theta + tk * (-g) == theta - tk * g in IEEE arithmetic, same frozen matchId), or
//     f_k when tk = 0; at m = 0 it re-matches (cal_corr), unless tk = 0 left theta as is.
#pragma once

#define OPT_GRADITER 10  // graditer (PSO.cpp:575)

// Arma Col::min(index) over pcost by one workgroup; with (fmin < gbest cost) the gbest
// takes particles.col(fmin_id).  count_mode: count = 0 on improvement, += 1 otherwise
// (:700-703; the descent phase only resets it, :647).  g > 0 records the trace.
__device__ void opt_update_gbest(const DevOpt &op, Smem &sm, bool count_mode, int g,
                                 bool init) {
    const int t = threadIdx.x;
    VI mine = {__builtin_inf(), t < op.P ? t : 0x7fffffff};
    for (int p = t; p < op.P; p += HPE_NT) {
        const double c = op.pc[p];
        if (c < mine.v) {  // NaN never wins: Armadillo's scan starts from +inf
            mine.v = c;
            mine.i = p;
        }
    }
    const VI best = block_argmin(sm, mine);
    const double gc = init ? 1e100 : op.gbest[26];
    const double cnt = init ? 0.0 : op.gbest[27];
    const bool imp = best.v < gc;
    __syncthreads();
    if (t < HPE_DOF) {
        if (imp) op.gbest[t] = op.x[(size_t)best.i * HPE_DOF + t];
        else if (init) op.gbest[t] = 0.0;  // gbest_pos = zeros (:548)
    }
    if (t == 0) {
        const double nc = imp ? best.v : gc;
        op.gbest[26] = nc;
        op.gbest[27] = imp ? 0.0 : (count_mode ? cnt + 1.0 : cnt);
        if (g > 0) op.trace[g - 1] = nc;
    }
}

// generate_particles(particles, x0, num_p, false) and the initial costs (:553-569).
__global__ __launch_bounds__(HPE_NT) void k_opt_init(DevOpt op, const double *__restrict__ x0,
                                                     const DevObs *__restrict__ og,
                                                     const DevHand *__restrict__ Hg) {
#include "hpe_opt_init_body.inc"
}

// Descent phase of generation g (iter = g + 1).  Cloud (+ matchId) staged in LDS when
// the frame has at most RF_STAGE_MAX points, as in k_refine.
template <bool STAGED>
__global__ __launch_bounds__(RF_NT) void k_opt_descent(DevOpt op, const DevObs *__restrict__ og,
                                                       const DevHand *__restrict__ Hg, int g) {
#include "hpe_opt_descent_body.inc"
}

// Velocity / position / cost phase of generation g.
__global__ __launch_bounds__(HPE_NT) void k_opt_move(DevOpt op, const DevObs *__restrict__ og,
                                                     const DevHand *__restrict__ Hg, int g) {
#include "hpe_opt_move_body.inc"
}

// ------------------------------------------------------------------ lane forms
// hpe_pso_optimise_batch / hpe_batch_pipeline_optimise: L lanes' pso_optimise in the same
// launches, grid (P, L).  blockIdx.y indexes the call's lane list (by value: a call on a subset
// of a live batch's lanes launches no idle workgroups); the lane it names picks everything
// else -- descriptor obs[lane], hand hands[lane] (the table is always indexed: it holds the
// context's hand in every entry while no lane hands are set), state row states + 27 lane, and
// its own arena.  The arenas of all lanes are identical, `stride` bytes apart; the argument
// holds lane 0's pointers and a lane rebases them with scalar adds, as lane_swarm does.
// normals and bounds are shared: every lane draws under the context's seed, particle
// i = blockIdx.x.  Each lane counts its arrivals in counter words of its own, so lanes never
// communicate, and opt_update_gbest reads every pc of its lane after the acquire: a lane's
// result does not depend on which of its workgroups arrives last.
struct OptLaneList {
    int lane[16];
};
__device__ __forceinline__ DevOpt lane_opt(DevOpt op, size_t stride, int lane) {
    const size_t off = stride * (size_t)lane;
    op.x = (double *)((char *)op.x + off);
    op.v = (double *)((char *)op.v + off);
    op.pb = (double *)((char *)op.pb + off);
    op.pc = (double *)((char *)op.pc + off);
    op.gbest = (double *)((char *)op.gbest + off);
    op.trace = (double *)((char *)op.trace + off);
    op.ctr = (unsigned *)((char *)op.ctr + off);
    return op;
}

__global__ __launch_bounds__(HPE_NT) void k_opt_init_b(DevOpt op, size_t stride, OptLaneList ll,
                                                       const double *__restrict__ states,
                                                       const DevObs *__restrict__ obs,
                                                       const DevHand *__restrict__ hands) {
    const int lane = ll.lane[blockIdx.y];
    op = lane_opt(op, stride, lane);
    const double *__restrict__ const x0 = states + (size_t)HPE_STATE_N * lane;
    const DevObs *__restrict__ const og = obs + lane;
    const DevHand *__restrict__ const Hg = hands + lane;
#include "hpe_opt_init_body.inc"
}

// The staged statements only: the batch calls refuse clouds above RF_STAGE_MAX.  The dynamic
// LDS is the largest lane's; the body sizes its arrays by its own o.n.  (A template so that
// the body's `if constexpr` discards the other form's statements; only <true> is instantiated.)
template <bool STAGED = true>
__global__ __launch_bounds__(RF_NT) void k_opt_descent_b(DevOpt op, size_t stride, OptLaneList ll,
                                                         const DevObs *__restrict__ obs,
                                                         const DevHand *__restrict__ hands, int g) {
    static_assert(STAGED, "the lane form is the staged descent");
    const int lane = ll.lane[blockIdx.y];
    op = lane_opt(op, stride, lane);
    const DevObs *__restrict__ const og = obs + lane;
    const DevHand *__restrict__ const Hg = hands + lane;
#include "hpe_opt_descent_body.inc"
}

__global__ __launch_bounds__(HPE_NT) void k_opt_move_b(DevOpt op, size_t stride, OptLaneList ll,
                                                       const DevObs *__restrict__ obs,
                                                       const DevHand *__restrict__ hands, int g) {
    const int lane = ll.lane[blockIdx.y];
    op = lane_opt(op, stride, lane);
    const DevObs *__restrict__ const og = obs + lane;
    const DevHand *__restrict__ const Hg = hands + lane;
#include "hpe_opt_move_body.inc"
}

// The call's last launch, one wave per lane: {gbest[0..25], cost} to the lane's state row
// and, with trace != NULL, its G gbest costs to row `lane` of trace.
__global__ __launch_bounds__(64) void k_opt_result_b(DevOpt op, size_t stride, OptLaneList ll,
                                                     double *__restrict__ states,
                                                     double *__restrict__ trace) {
    const int lane = ll.lane[blockIdx.y], t = threadIdx.x;
    op = lane_opt(op, stride, lane);
    if (t < HPE_STATE_N) states[(size_t)HPE_STATE_N * lane + t] = op.gbest[t];
    if (trace)
        for (int g = t; g < op.G; g += 64) trace[(size_t)lane * op.G + g] = op.trace[g];
}

// The slot call's descriptors: lane b's from the slot table into the call's own table.
__global__ void k_opt_stage_b(const DevObs *__restrict__ table, BatchFirst first,
                              DevObs *__restrict__ obs) {
    const int t = threadIdx.x, b = blockIdx.y;
    if (t < (int)(sizeof(DevObs) / 8))
        ((unsigned long long *)(obs + b))[t] = ((const unsigned long long *)(table + first.slot[b]))[t];
}
