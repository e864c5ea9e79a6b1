/*
 * include/hpe.h -- C ABI of the MI355X-native PSO / costfunc / handmodel hot path.
 *
 * Drop-in boundary for hjurong/hand-pose-estimation (reference paths below are
 * /root/reference/src file:line).  Plain pointers and sizes only; no exceptions
 * or C++ types cross it.  Every entry point returns 0 on success and a negative
 * HPE_E* code on failure; hpe_last_error(ctx) returns the message.
 *
 * Conventions (matching the reference):
 *   - theta: 26 doubles per particle, degrees for angles, cm for position
 *     (handmodel.cpp:123-149); a batch is column-major 26 x P (PSO.cpp:67), i.e.
 *     particle-contiguous, exactly Armadillo's mat::memptr() layout.
 *   - sphere centres: 48 x 3 per particle, row-major here ([sphere][xyz]),
 *     with y and z negated (handmodel.cpp:288).
 *   - depth: 240 x 320 row-major ([v][u]); cm after preprocessing.
 *   - cloud: N x 3 row-major (X, -Y, -Z) cm (observedmodel.cpp:157-161).
 *   - match ids: int32 sphere index per cloud point (uvec matchId, costfunc.h:27).
 *
 * Ownership: the caller owns every host buffer; they are copied in/out and not
 * retained after return.  The context owns all device memory and one HIP stream.
 * Threading: one context per host thread per device; multi-GPU = one context per
 * device.
 */
#ifndef HPE_H
#define HPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPE_ABI_VERSION 1

#define HPE_OK 0
#define HPE_E_ARG -1      /* bad argument (null pointer, size out of range) */
#define HPE_E_HIP -2      /* HIP runtime error */
#define HPE_E_STATE -3    /* call order (e.g. no frame set, no PSO params) */
#define HPE_E_NOMEM -4    /* allocation failed */
#define HPE_E_NODEVICE -5 /* no gfx950 device visible */

typedef struct hpe_ctx hpe_ctx;

/* Hand geometry.  Replaces handmodel(h_geo, h_spacing, tb_spheres, fg_spheres,
 * h_CMC, sphR) (handmodel.h:9-10, handmodel.cpp:10-27).  Sphere counts must be
 * tb {2,2,2,2}, fg {4,2,2,2}: the reference hard-codes 8 + 4x10 rows
 * (handmodel.cpp:272-286). */
typedef struct {
    double geo_cm[20];    /* misc/hgeo.dat / 10, thumb first (handmodel.cpp:107-121) */
    double radii_cm[48];  /* misc/rad.dat / 10 (testmodel.cpp:49) */
    double cmc_deg[5];    /* testmodel.cpp:37 */
    double spacing_cm[5]; /* testmodel.cpp:36; narrowed to float like fingermodel.h:43 */
    int32_t tb_spheres[4];
    int32_t fg_spheres[4];
} hpe_hand_params;

/* Observation of one frame, already preprocessed (observedmodel getters,
 * observedmodel.h:51-63 / observedmodel.cpp:383-409). */
typedef struct {
    const double *depth_cm; /* 240*320 */
    const float *dt;        /* 240*320 distance transform of the background, px */
    const double *cloud;    /* n*3 */
    int32_t n;
    double scale;           /* cm per pixel (get_img_scale) */
    double dtmax;           /* max(dt) (costfunc.cpp:298) */
    double K[9];            /* camera matrix row-major (get_camera_mat) */
} hpe_frame;

int hpe_abi_version(void);
const char *hpe_last_error(const hpe_ctx *ctx);

/* Context: device buffers, the hand constants and one stream on `device`. */
int hpe_create(hpe_ctx **out, int device, const hpe_hand_params *hand);
int hpe_destroy(hpe_ctx *ctx);
/* hipStream_t of the context (for callers that order their own work after ours). */
void *hpe_stream(hpe_ctx *ctx);
int hpe_sync(hpe_ctx *ctx);

/* observedmodel::init_observation / next_frame preprocessing on the host
 * (observedmodel.cpp:110-219, 272-369): depth .bin (float mm, 240x320 row-major)
 * -> depth cm, cloud (optionally down-sampled to 250), scale, distance transform.
 * cloud_out capacity: 76800*3 doubles. */
int hpe_preprocess_depth(const float *depth_mm, int to_cm, int downsample, double focal,
                         double *depth_cm_out, float *dt_out, double *cloud_out,
                         int32_t *n_out, double *scale_out, double *dtmax_out,
                         double K_out[9]);

/* Frame residency.  `slot` in [0, 4096): a frame stored once stays in HBM; select
 * makes it the observation every following call uses (next_frame equivalent,
 * observedmodel.cpp:420-430).  hpe_set_frame = store into slot 0 + select 0. */
int hpe_store_frame(hpe_ctx *ctx, int slot, const hpe_frame *frame);
int hpe_select_frame(hpe_ctx *ctx, int slot);
int hpe_set_frame(hpe_ctx *ctx, const hpe_frame *frame);

/* observedmodel::next_frame on the GPU (observedmodel.cpp:110-219, 272-369): the raw
 * depth .bin (float mm, 240x320 row-major, host memory) is copied through a pinned
 * buffer and preprocessed by one workgroup on the context's preprocessing stream --
 * depth cm, cloud (down-sampled to 250 points when `downsample`), cm-per-pixel scale,
 * 5x5 chamfer distance transform and its max -- straight into frame slot `slot`.
 * Asynchronous: the call returns once the host buffer is copied; hpe_select_frame(slot)
 * orders the tracking stream after it, so frame f+1 is prepared while frame f is tracked.
 * Cloud, depth, DT, its max and the scale equal hpe_preprocess_depth bit for bit. */
int hpe_prepare_frame(hpe_ctx *ctx, int slot, const float *depth_mm, int to_cm, int downsample,
                      double focal);

/* Copies a stored or prepared frame back to the host (tests, debugging); synchronises.
 * cloud: n*3 doubles (capacity 76800*3); any output may be NULL. */
int hpe_frame_readback(hpe_ctx *ctx, int slot, double *depth_cm, float *dt, double *cloud,
                       int32_t *n_out, double *scale_out, double *dtmax_out);

/* handmodel::build_hand_model for a batch (handmodel.cpp:259-298).
 * theta: 26*P; S_out: P*48*3; joints_out (optional, may be NULL): P*21*3
 * (hand_joints, handmodel.cpp:291-296). */
int hpe_build_spheres(hpe_ctx *ctx, const double *theta, int P, double *S_out,
                      double *joints_out);

/* costfunc::cal_cost for a batch (costfunc.cpp:89-127; with_collision != 0 gives
 * cal_cost2(theta, matchId, true) of costfunc.cpp:31-86).  Replaces the OpenMP
 * particle loops of PSO.cpp:748-763 and :848-861.
 * match_out (optional): P*n int32 correspondences (compute_correspondences). */
int hpe_eval_costs(hpe_ctx *ctx, const double *theta, int P, int with_collision,
                   double *cost_out, int32_t *match_out);

/* costfunc::cal_cost2(theta, matchId, compute_corr, debug) (costfunc.cpp:31-86).
 * match_inout: n int32; written when compute_corr != 0, read otherwise.
 * terms_out (optional): {align, depth, collision}. */
int hpe_cal_cost2(hpe_ctx *ctx, const double theta[26], int32_t *match_inout,
                  int compute_corr, double *cost_out, double terms_out[3]);

/* The cost terms for caller-supplied sphere centres: costfunc::compute_correspondences
 * (costfunc.cpp:306-343), align_models (:346-377), depth_penalty (:227-304) and
 * self_collision_penalty (:130-197), which take a sphere matrix rather than a theta.
 * S: P*48*3 (row-major per particle, y/z negated as build_hand_model returns them).
 * match_inout: P*n int32, written when compute_corr != 0, read otherwise.
 * terms_out: P*3 {align, depth, collision}. */
int hpe_eval_spheres(hpe_ctx *ctx, const double *S, int P, int compute_corr,
                     int32_t *match_inout, double *terms_out);

/* PSO::set_pso_params (PSO.cpp:38-54).  pso_evolve uses the SPSO-2011 constants
 * (PSO.cpp:772-774); pso_optimise uses omega/phip/phig; minstep/minfunc are kept for
 * API parity (no caller reads them). */
int hpe_set_pso_params(hpe_ctx *ctx, const double ub[26], const double lb[26],
                       const double stdv[26], double omega, double phip, double phig,
                       int maxiter, double minstep, double minfunc);
/* The reference reseeds with 1000 on every pso_evolve (PSO.cpp:722). */
int hpe_set_seed(hpe_ctx *ctx, uint64_t seed);

/* PSO::pso_evolve(optfunc, x0, num_p, bestp) (PSO.cpp:717-886).
 * bestcost_out (optional) = gbest cost (pbest cost of the gbest generation). */
int hpe_pso_evolve(hpe_ctx *ctx, const double x0[26], int num_p, double bestp[26],
                   double *bestcost_out);

/* Multi-GPU subswarms, the per-frame best of N after the caller's all-gather
 * of every rank's 27-double state: d_state <- the row of d_gathered (world x 27 device
 * doubles, {bestp, cost} per rank) with the smallest cost -- NaN never wins, ties go to the
 * lowest rank (hpe/dist.py pick_best) -- as one launch on hpe_stream(ctx).  world 1..64.
 * Replaces the reference's shared gbest across its OpenMP loop (PSO.cpp:848-861). */
int hpe_pick_best(hpe_ctx *ctx, const double *d_gathered, int world, double *d_state);

/* Multi-GPU subswarms with the per-frame exchange inside the library (SURVEY.md §8e;
 * BASELINE config 5).  One process per GPU, one context each, seed 1000 + rank
 * (hpe_set_seed).  Rank 0 calls hpe_subswarm_unique_id and hands the 128 bytes to the other
 * ranks (any channel, e.g. a torch.distributed broadcast); then every rank calls
 * hpe_subswarm_init with them -- collective, RCCL's ncclCommInitRank on this context's device.
 * From then on every tracked frame of the context (hpe_track_frame[_dev],
 * hpe_track_pipelined, hpe_track_sequence_dev, hpe_track_raw_sequence_dev) ends with an
 * all-gather of every rank's {bestp, cost} (27 doubles, RCCL over xGMI) and the pick of
 * hpe_pick_best, on hpe_stream(ctx): d_state (and the frame's d_hist row) holds the best of
 * all subswarms, which every rank tracks the next frame from (testmodel.cpp:138).  The
 * exchange is captured into the tracking graphs with the frames, so N ranks run the N = 1
 * loop.  Every rank must issue the same tracking calls in the same order.  nranks = 1 is
 * allowed (the all-gather is in place: RCCL moves nothing).  hpe_subswarm_enable(ctx, 0)
 * suspends the exchange (the communicator stays), 1 resumes it, 2 resumes it with every
 * tracking call launching directly instead of through graphs -- the form the library falls
 * back to by itself (noted once on stderr) if a capture holding the collective fails.
 * hpe_subswarm_fini destroys the communicator (hpe_destroy does too).  hpe_subswarm_info:
 * world size, rank, the RCCL version (ncclGetVersion), whether the exchange runs inside
 * captured graphs (in_graphs) and, if gathered_out != NULL, a synchronous copy of the
 * gather buffer, nranks x 27 doubles (row r = rank r's last frame result; NaN before the
 * first).  RCCL is opened at run time (librccl.so.1): without it hpe_subswarm_unique_id /
 * _init return HPE_E_STATE and nothing else changes.  Any output pointer may be NULL. */
#define HPE_SUBSWARM_ID_BYTES 128
int hpe_subswarm_unique_id(unsigned char id_out[HPE_SUBSWARM_ID_BYTES]);
int hpe_subswarm_init(hpe_ctx *ctx, const unsigned char id[HPE_SUBSWARM_ID_BYTES], int nranks,
                      int rank);
int hpe_subswarm_enable(hpe_ctx *ctx, int on);
int hpe_subswarm_fini(hpe_ctx *ctx);
int hpe_subswarm_info(hpe_ctx *ctx, int32_t *nranks, int32_t *rank, int32_t *version,
                      int32_t *in_graphs, double *gathered_out);

/* The scripted transport of the same exchange.  It communicates with NOBODY: it exists so
 * that the N-rank device path (the final kernel writing gather row `rank`, the pick over
 * several rows inside the next refine launch and at a chunk's end, the history row) can be
 * executed and checked on one GPU, in one process, with no communicator and without RCCL.
 * script is host memory, frames x nranks x 27 doubles ({bestp, cost} per rank and exchange);
 * the library copies it to device memory of its own.  Where hpe_subswarm_init's exchange
 * calls the all-gather, a one-wave kernel on hpe_stream(ctx) copies rows w != rank of
 * script[k] into the gather buffer (row `rank` stays the frame's own result) and advances k,
 * a device-resident exchange counter: a replayed chunk graph reads the script frame of its
 * own exchange; past the last frame k wraps to 0.  Everything after "the gather buffer holds
 * nranks rows" is the RCCL transport's own code, and hpe_subswarm_enable / _info / _fini act
 * on either transport.  Calling it again on a context whose live scripted transport has the
 * same nranks, rank and frames (exchange not suspended) loads the new contents and rewinds
 * k, and the captured tracking graphs keep serving; any other call replaces the live
 * transport (either kind), as hpe_subswarm_init does.  The gather buffer is NaN afterwards.
 * HPE_E_ARG: null ctx or script, nranks outside 1..64, rank outside [0, nranks), frames < 1. */
int hpe_subswarm_init_scripted(hpe_ctx *ctx, int nranks, int rank, const double *script,
                               int frames);

/* Opt-in per-generation exchange between subswarms (ICP-PSO style; NOT the reference's
 * algorithm, whose gbest never enters the velocity, PSO.cpp:824-832).  every > 0: after
 * every `every`-th generation g < maxiter-1 of each pso_evolve of this context (standalone
 * or inside a tracking call) the library writes this subswarm's best pbest {pose[26], cost}
 * into d_ext (27 doubles of caller-owned device memory), then calls
 * fn(user, d_ext, g), which must enqueue on hpe_stream(ctx) the collective that replaces
 * d_ext by the best over all subswarms (lowest cost, ties to the lowest rank) and return
 * 0.  From generation g + 1 on, d_ext is an extra informant candidate of every particle:
 * it replaces the particle's informant when its cost is strictly lower (PSO.cpp:807-832 with
 * one more candidate, ranked after the local ones).  Tracking calls run without graph
 * replay while it is on.  every = 0 turns it off (fn, user, d_ext ignored). */
typedef int (*hpe_exchange_fn)(void *user, double *d_ext, int generation);
int hpe_set_exchange(hpe_ctx *ctx, int every, double *d_ext, hpe_exchange_fn fn, void *user);

/* Per-generation trace of the last pso_evolve (debug / parity):
 * gbest cost, stagnation count, topology generation; arrays of maxiter-1. */
int hpe_pso_trace(hpe_ctx *ctx, double *gbest, int32_t *count, int32_t *topo, int n);

/* PSO::pso_optimise(optfunc, x0, num_p, bestp) (PSO.cpp:539-712): global-best PSO with
 * omega/phip/phig whose particles first take 10 single-coordinate Goldstein steps every
 * generation.  maxiter-1 generations.  Draws: Philox streams 5..8 under hpe_set_seed's
 * seed (the reference draws from an unseeded Armadillo stream).  bestcost_out optional;
 * gbest_trace optional, trace_len <= maxiter-1 gbest costs, one per generation. */
int hpe_pso_optimise(hpe_ctx *ctx, const double x0[26], int num_p, double bestp[26],
                     double *bestcost_out, double *gbest_trace, int trace_len);

/* PSO::refine_init_pose(x0, optfunc) (PSO.cpp:216-266).  evals_out optional. */
int hpe_refine_init_pose(hpe_ctx *ctx, double x0[26], int32_t *evals_out);

/* Sphere placement inside refine_init_pose (every refine of this context, including the
 * tracking loops).  exact = 0 (default): the hand-frame form -- refine moves theta0..5
 * only (PSO.cpp:225-227), so each evaluation places S = Rg(theta0..2) q + u from centres q
 * built once per call, and the self-collision penalty is a constant of the call; spheres
 * within 1e-12 cm and costs within 1e-13 relative of the reference's DH chain
 * (DESIGN.md §2).  exact = 1: the reference's chain on every evaluation (bit-identical
 * FK).  The environment variable HPE_REFINE_EXACT=1 sets the default at hpe_create.
 * Cached tracking graphs are rebuilt on change. */
int hpe_set_refine_exact(hpe_ctx *ctx, int exact);
int hpe_get_refine_exact(const hpe_ctx *ctx);

/* Speculated translation block of refine_init_pose on clouds of at most 2048 points (every
 * refine of this context, the tracking loops included).  on = 1 (default): the refine launch
 * carries a second workgroup that runs the translation block (theta3..5) from the pose of
 * every rotation-block line search while that search runs; when the rotation block ends on a
 * failing search, which leaves the pose unchanged, the result is taken from it instead of
 * being computed after the search.  The pose and the evaluation count are bit for bit those
 * of on = 0, the one-workgroup form; every wait is bounded and falls back to it (DESIGN.md
 * §4.3).  The environment variable HPE_REFINE_SPEC=0/1 sets the default at hpe_create.
 * Cached tracking graphs are rebuilt on change. */
int hpe_set_refine_spec(hpe_ctx *ctx, int on);
int hpe_get_refine_spec(const hpe_ctx *ctx);

/* One tracked frame of test_full (testmodel.cpp:124-138) on the selected frame:
 * [refine_init_pose] -> pso_evolve -> cost = cal_cost(bestp) -> x0 = bestp.
 * x0_inout: 26 doubles (host).  cost_out optional. */
int hpe_track_frame(hpe_ctx *ctx, int num_p, int refine, double x0_inout[26],
                    double *cost_out);

/* Same, device-resident: d_state is a device pointer to 27 doubles
 * {x0[26], cost}; read as x0, overwritten with {bestp, cost}.  Asynchronous on
 * hpe_stream(ctx): no host synchronisation. */
int hpe_track_frame_dev(hpe_ctx *ctx, int num_p, int refine, double *d_state);

/* Offline tracking of a recorded sequence: test_full's loop (testmodel.cpp:117-139) over
 * frames already resident in HBM, slots first_slot .. first_slot+n-1 (hpe_store_frame /
 * hpe_prepare_frame), each tracked exactly like hpe_track_frame_dev on its own slot and
 * d_state carried from frame to frame.  Frames are captured frames_per_graph at a time
 * into one graph (0: HPE_SEQ_CHUNK), so the graph-to-graph gap is paid once per chunk;
 * the chunk graphs read each frame's descriptor and history row through a device cursor
 * (k_seq_begin starts it, each frame's final kernel advances it), so a captured chunk
 * serves every chunk of the same shape (frames, kernel forms, d_state, d_hist) wherever
 * its slots lie.  d_hist (device, optional): n x 27 doubles,
 * frame f's {bestp, cost}.  Asynchronous on hpe_stream(ctx); the last frame is the
 * selected one afterwards, and a later hpe_prepare_frame waits for the sequence. */
#define HPE_SEQ_CHUNK 8
#define HPE_SEQ_MAX_CHUNK 32
int hpe_track_sequence_dev(hpe_ctx *ctx, int num_p, int refine, double *d_state,
                           int first_slot, int n, int frames_per_graph, double *d_hist);

/* B independent sequences tracked in the SAME launches (a dataset run, two hands in one depth
 * stream, a multi-camera rig): lane b is
 *   hpe_track_sequence_dev(ctx, num_p, refine, d_states + 27 b, first_slots[b], n,
 *                          frames_per_graph, d_hist + 27 n b)
 * bit for bit -- the context's seed, PSO parameters and refine form -- but a generation launch
 * covers B x num_p particles, a refine launch is B workgroups on B CUs, and one captured graph
 * holds a chunk of frames of all lanes.  d_states: device, B x 27 {x0 -> bestp, cost}.
 * first_slots: host, B entries (copied before return); the lanes' slot ranges may overlap or
 * coincide (frames are only read).  d_hist (device, optional): B x n x 27, lane b's frame f at
 * row b n + f.  Asynchronous on hpe_stream(ctx).  Chunk graphs are keyed by their shape
 * (num_p, generations, refine, frames, kernel forms, B, d_states, d_hist), not by the slots or n:
 * per-lane device cursors name each frame.  The selected frame stays as it was, hpe_pso_trace
 * is not updated, and hpe_refine_eval_count counts every lane's evaluations.
 * Supported (anything else is refused, never run another way): 1 <= B <= HPE_BATCH_MAX; num_p
 * in the workgroup-per-particle form (below 1024 by default); every frame at most 2048 cloud
 * points (the single-workgroup refine); for each frame index all lanes on the same side of 256
 * cloud points (one kernel form per launch) -- HPE_E_ARG; no live subswarm transport and no
 * hpe_set_exchange -- HPE_E_STATE.  The slots are prepared already: this call prepares nothing
 * and ignores the lane windows' mode (hpe_set_batch_window). */
#define HPE_BATCH_MAX 16
int hpe_track_batch_dev(hpe_ctx *ctx, int num_p, int refine, int B, double *d_states,
                        const int32_t *first_slots, int n, int frames_per_graph, double *d_hist);

/* Pipelined tracking: test_full's loop (testmodel.cpp:117-139) with next_frame
 * (observedmodel.cpp:420-430) of frame f+1 running INSIDE frame f's refine launch, on CUs
 * the single-workgroup refine leaves idle: one stream, one replayed graph per frame.
 * hpe_pipeline_begin prepares the first raw depth frame (float mm, 240x320, host).
 * hpe_track_pipelined tracks the current frame exactly like hpe_track_frame_dev
 * (d_state: 27 device doubles {x0 -> bestp, cost}) and, if next_depth_mm != NULL, copies
 * it (host) and prepares it as the next current frame; NULL ends the sequence. */
int hpe_pipeline_begin(hpe_ctx *ctx, const float *depth_mm, int to_cm, int downsample,
                       double focal);
int hpe_track_pipelined(hpe_ctx *ctx, int num_p, int refine, double *d_state,
                        const float *next_depth_mm);

/* Resident raw sequence: test_full's loop (testmodel.cpp:117-139) over n raw depth frames
 * already in HBM -- d_raw_mm: device, n x 240x320 float mm, frame after frame -- with
 * next_frame (observedmodel.cpp:420-430) of frame f+1 inside frame f's refine launch, as
 * hpe_track_pipelined does, and frames_per_graph frames (0: HPE_SEQ_CHUNK) captured into one
 * graph, so the graph-to-graph gap is paid once per chunk.  The preparation reads its raw
 * frame through a device row cursor that each frame's final kernel advances: a captured
 * chunk serves every chunk of the same shape.  Frame 0 is prepared first, on the same
 * stream.  d_state: 27 device doubles {x0 -> bestp, cost} carried from frame to frame;
 * d_hist (device, optional): n x 27 doubles, frame f's {bestp, cost}.  Asynchronous on
 * hpe_stream(ctx); ends a pipelined sequence in progress. */
int hpe_track_raw_sequence_dev(hpe_ctx *ctx, int num_p, int refine, double *d_state,
                               const float *d_raw_mm, int n, int to_cm, int downsample,
                               double focal, int frames_per_graph, double *d_hist);

/* Copies one of the pipeline's two prepared-frame buffers (hpe_track_pipelined,
 * hpe_track_raw_sequence_dev: frame f of a sequence is prepared into buffer f & 1) back to the
 * host, as hpe_frame_readback does for a slot (tests, debugging); synchronises.
 * cloud: n*3 doubles (capacity 76800*3); any output may be NULL. */
int hpe_pipe_readback(hpe_ctx *ctx, int parity, double *depth_cm, float *dt, double *cloud,
                      int32_t *n_out, double *scale_out, double *dtmax_out);

/* B resident raw sequences tracked in the SAME launches (what a multi-camera rig, two hands in
 * one depth stream or a dataset run delivers): lane b is
 *   hpe_track_raw_sequence_dev(ctx, num_p, refine, d_states + 27 b, d_raw_mm[b], n, to_cm,
 *                              downsample, focal, frames_per_graph, d_hist + 27 n b)
 * bit for bit -- the context's seed, PSO parameters and refine form -- in hpe_track_batch_dev's
 * launches, with next_frame of every lane's frame f+1 inside frame f's refine launch: grid
 * (1 + 9, B), lane b's refine workgroup and the nine that prepare its next frame, each on a CU
 * of its own.  d_raw_mm: host array of B device pointers, each n x 240x320 float mm (copied
 * before return; lanes may name the same buffer).  d_states: device, B x 27.  d_hist (device,
 * optional): B x n x 27, lane b's frame f at row b n + f.  Asynchronous on hpe_stream(ctx).
 * Chunk graphs are keyed by their shape (num_p, generations, refine, frames, buffer parity,
 * whether the last frame prepares another, B, to_cm, downsample, focal, d_states, d_hist), not
 * by the raw pointers or n: a lane's raw base and frame cursor live in device memory.  The call
 * owns its frame buffers and preparation scratch (about 4.6 MB per lane): a pipelined sequence
 * in progress and the other calls' cached graphs stay valid, the selected frame stays as it
 * was, hpe_pso_trace is not updated, and hpe_refine_eval_count counts every lane's evaluations.
 * Supported (anything else is refused, never run another way): 1 <= B <= HPE_BATCH_MAX; num_p
 * in the workgroup-per-particle form; downsample != 0 (250-point clouds: the single-workgroup
 * refine) -- HPE_E_ARG; no live subswarm transport and no hpe_set_exchange -- HPE_E_STATE. */
int hpe_track_raw_batch_dev(hpe_ctx *ctx, int num_p, int refine, int B, double *d_states,
                            const float *const *d_raw_mm, int n, int to_cm, int downsample,
                            double focal, int frames_per_graph, double *d_hist);

/* A live batch: B raw depth streams whose frames arrive one at a time in host memory (a
 * multi-camera rig), one frame of every lane tracked per call in hpe_track_raw_batch_dev's
 * launches.  Lane b computes, bit for bit, what
 *   hpe_pipeline_begin(ctx, depth_mm[b], to_cm, downsample, focal), then per frame
 *   hpe_track_pipelined(ctx, num_p, refine, d_states + 27 b, next_depth_mm[b])
 * computes on the same context (its seed, PSO parameters and refine form): one refine launch of
 * grid (1 + 9, B) whose preparation workgroups read lane b's next frame straight from that
 * lane's pinned host buffer, the batch's generation launches and one final launch -- one
 * replayed graph per frame, keyed by its shape (num_p, generations, refine, B, d_states, buffer
 * parity, whether a next frame is prepared, to_cm, focal), never by host pointers.
 * depth_mm, next_depth_mm: host arrays of B host pointers, each one 240x320 float mm frame,
 * copied into the library's pinned buffers before the call returns (the caller may overwrite
 * its frames at once).  next_depth_mm == NULL (or every entry NULL) tracks the current frames
 * and ends the batch; some but not all entries NULL is HPE_E_ARG: lanes advance in lockstep.
 * (The default pacing: under hpe_set_batch_pacing(HPE_PACING_FREE), below, lanes skip calls, join
 * late and pause.)  To change the lane count, end the batch and begin another; the caller owns d_states (device,
 * B x 27 {x0 -> bestp, cost}, read and overwritten every call), so poses carry over.
 * Asynchronous on hpe_stream(ctx).  Before a pinned buffer is refilled the host waits (bounded,
 * HPE_E_HIP on a timeout) for the frame number the final launch publishes to host memory.
 * The batch shares hpe_track_raw_batch_dev's lane buffers: that call ends a live batch in
 * progress.  A single pipelined sequence in progress and the other calls' cached graphs stay
 * valid, the selected frame stays as it was, hpe_pso_trace is not updated, and
 * hpe_refine_eval_count counts every lane's evaluations.
 * Refused, never run another way: B outside 1..HPE_BATCH_MAX, a null array, lane pointer or
 * d_states, focal <= 0, downsample == 0, num_p in the wave form -- HPE_E_ARG; a live subswarm
 * transport or hpe_set_exchange, HPE_PIPE_UPLOAD=1 in the environment at begin (the upload form
 * is not built for lanes), hpe_track_batch_pipelined without a begin, after the batch ended or
 * with a B other than the begin's -- HPE_E_STATE. */
int hpe_batch_pipeline_begin(hpe_ctx *ctx, int B, const float *const *depth_mm,
                             int to_cm, int downsample, double focal);
int hpe_track_batch_pipelined(hpe_ctx *ctx, int num_p, int refine, int B, double *d_states,
                              const float *const *next_depth_mm);

/* Lane input: what a live batch's frames are, and who fills the lanes' pinned buffers.
 *
 * 16-bit frames.  Depth cameras deliver unsigned 16-bit pixels in a depth unit (1 mm, or a
 * fraction of one).  hpe_batch_pipeline_begin_u16 / hpe_track_batch_pipelined_u16 are the two
 * calls above on such frames: depth, next_depth are host arrays of B host pointers, each one
 * 240x320 uint16_t frame, and pixel value u stands for the raw float
 *   rv = (float)u * unit_mm                       (one fp32 multiply; 0 stays 0, "no depth")
 * on which everything is the float calls' computation: lane b equals, bit for bit,
 * hpe_pipeline_begin + hpe_track_pipelined on that stream converted on the host by that rule --
 * with windows, lane hands, either pacing, either batch form, reports and
 * hpe_batch_pipeline_optimise.  The library copies 2 bytes per pixel into the lanes' pinned
 * buffers (the float batch's, a u16 frame fills the first half: one context runs float and u16
 * batches in turn without reallocating), and the preparation workgroups read the 16-bit pixels in
 * place, unsigned, and multiply: half the bytes cross the host link, and no launch is added.
 * unit_mm lives in device memory, written at the begin: two u16 batches of one shape with
 * different units replay the same graphs.  A batch keeps the format it began with:
 * hpe_track_batch_pipelined on a u16 batch and hpe_track_batch_pipelined_u16 on a float batch are
 * HPE_E_STATE.  unit_mm not finite or <= 0 -- HPE_E_ARG; every other refusal is the float calls'.
 *
 * Filling a buffer in place.  Between a begin and the end of the batch, in either format,
 * hpe_batch_frame_buffer returns lane `lane`'s pinned buffer of the parity the NEXT track call
 * reads, and in *bytes_out (optional) the bytes one frame of the batch's format takes.  Before
 * it returns it waits, bounded (HPE_E_HIP on expiry), until the device has read the frame that
 * buffer last held -- the wait the track call makes before its copy.  The caller writes the
 * lane's next frame there (a camera SDK's receive buffer can be that memory) and passes the same
 * pointer as that lane's entry of the next frame array: the track call recognises it and copies
 * nothing for that lane.  Other lanes of the call may pass ordinary arrays (copied as ever), or
 * NULL under free pacing.  Asking again before the track call returns the same pointer.  After a
 * track call the pointer names a buffer whose frame is current: passing it again is refused with
 * HPE_E_ARG ("stale frame buffer") and changes nothing; ask again after every track call.  Frame
 * 0 is always copied by the begin.  Nothing captured changes: an in-place call replays the
 * graphs of a copying call.  No live batch -- HPE_E_STATE; a lane outside the batch or a null
 * buf_out -- HPE_E_ARG. */
int hpe_batch_pipeline_begin_u16(hpe_ctx *ctx, int B, const uint16_t *const *depth,
                                 float unit_mm, int to_cm, int downsample, double focal);
int hpe_track_batch_pipelined_u16(hpe_ctx *ctx, int num_p, int refine, int B, double *d_states,
                                  const uint16_t *const *next_depth);
int hpe_batch_frame_buffer(hpe_ctx *ctx, int lane, void **buf_out, size_t *bytes_out);

/* Lane views: a live batch on 16-bit frames at the camera's own resolution.  No depth camera
 * delivers 240x320 frames with the principal point at (160, 120): a view tells the library how
 * the model image lies in a lane's camera image, and the preparation's load does the crop and
 * the decimation.  Model pixel (r, c), 0 <= r < 240, 0 <= c < 320, reads camera pixel (sr, sc):
 *   sr = row0 + step * r
 *   sc = col0 + step * (flags & HPE_VIEW_FLIP_COLS ? 319 - c : c)
 * and its 16-bit value is cam[sr * pitch + sc] if 0 <= sr < height && 0 <= sc < width, else 0
 * ("no depth", like any other hole).  This is a pick (nearest-neighbour decimation), the usual
 * reduction for depth: averaging would invent surfaces across depth edges.  A hole at the picked
 * pixel stays a hole, whatever its camera neighbours hold; block rules (min-non-zero, median) are
 * not offered in the pick ("Lane cleaning" below runs a neighbourhood rule on the picked image).
 * The flip tracks a left hand, or a camera that faces the user, with the right-hand
 * model.  The picked value follows the u16 batch's rule unchanged: rv = (float)u * unit_mm.
 *
 * hpe_batch_pipeline_begin_view is hpe_batch_pipeline_begin_u16 with views[b] (host, B entries,
 * read before return) the view of lane b -- cameras of one model still differ in principal point,
 * so the origins differ per lane -- and frames[b] a camera frame of pitch * height pixels.  focal
 * is the MODEL image's focal length, the camera's fx divided by step; one focal serves the batch,
 * as in every other batch call: lanes whose fx / step differ are the caller's to reconcile (the
 * library cannot know, and does not check).  Tracking is hpe_track_batch_pipelined_u16: on a view
 * batch next_depth[b] is a camera frame of lane b's view.  hpe_batch_frame_buffer returns a
 * buffer of pitch * height * 2 bytes for the lane and reports that size, so a camera SDK delivers
 * its native frame there and the track call copies nothing.  Lane b equals, bit for bit after
 * every frame, hpe_pipeline_begin + hpe_track_pipelined on that stream reduced on the host by the
 * rule above and converted by the u16 rule (hpe/view.py: View.reduce, then depth_u16_to_mm) --
 * with windows, lane hands, either pacing, either batch form, reports,
 * hpe_batch_pipeline_optimise and hpe_batch_pipeline_locate, which reads the lane's camera frame
 * through its view in all three passes.  The views live in a device table written at the begin,
 * never a captured argument: two view batches of one shape with different views replay the same
 * graphs.  The pinned buffers grow at the begin to the largest lane frame (the stream drained,
 * all lanes or none) and never shrink: a context runs float, u16 and view batches in turn, and
 * reallocates only when a frame does not fit.
 *
 * Coordinates.  Window bounds, report pixels, locate search bounds and results all stay in
 * MODEL-image coordinates.  Model pixel (r, c) -- fractional for a report's px or a located centre
 * -- is camera pixel
 *   row = row0 + step * r,   col = col0 + step * (FLIP ? 319 - c : c)
 * and a model window [lo, hi] covers camera rows row0 + step * lo .. row0 + step * hi (columns
 * likewise; under the flip the two column ends swap).
 *
 * hpe_view_fit (host only, no context) fits a view of the given step to a camera's intrinsics:
 *   row0 = lrint(cy - 120.0 * step),  col0 = lrint(cx - 160.0 * step)
 *   (under the flip col0 = lrint(cx - 159.0 * step): model column 160 reads camera column cx)
 *   *focal_out = fx / step
 * residual_px (optional) receives what the rounding left: the principal point's offset from model
 * pixel (160, 120) in model pixels, {column, row}.  hpe_batch_views_readback synchronises and
 * copies the table's first B entries (the last view begin's), like hpe_batch_windows_readback.
 *
 * Refused with HPE_E_ARG, nothing changed: null views (or out), step outside 1..8, width or
 * height < 1, pitch < width, pitch or height > HPE_VIEW_DIM_MAX, pitch * height >
 * HPE_VIEW_PIXELS_MAX (4 MiB per frame; 1920x1080 fits), an unknown flag bit, non-zero pad; for
 * hpe_view_fit also fx, cx or cy not finite, fx <= 0, or an origin beyond +-1e9 pixels.  A view lying wholly outside its camera
 * image is legal: it reads empty frames.  hpe_track_batch_pipelined (float) on a view batch is
 * HPE_E_STATE, as on a u16 batch; hpe_batch_views_readback without a view batch begun on the
 * context is HPE_E_STATE.  Every other refusal is the u16 begin's. */
#define HPE_VIEW_FLIP_COLS 1u
#define HPE_VIEW_DIM_MAX 2048
#define HPE_VIEW_PIXELS_MAX 2097152
typedef struct hpe_view {    /* 32 bytes */
    int32_t width, height;   /* camera image, pixels */
    int32_t pitch;           /* pixels from one camera row to the next, >= width */
    int32_t row0, col0;      /* camera pixel of model pixel (0, 0); may be negative */
    int32_t step;            /* 1..8: camera pixels per model pixel, both axes */
    uint32_t flags;          /* HPE_VIEW_FLIP_COLS or 0 */
    int32_t pad;             /* 0 */
} hpe_view;
int hpe_batch_pipeline_begin_view(hpe_ctx *ctx, int B, const uint16_t *const *frames,
                                  const hpe_view *views, float unit_mm, int to_cm,
                                  int downsample, double focal);
int hpe_view_fit(int width, int height, int pitch, double fx, double cx, double cy, int step,
                 uint32_t flags, hpe_view *out, double *focal_out, double residual_px[2]);
int hpe_batch_views_readback(hpe_ctx *ctx, int B, hpe_view *out);

/* Lane cleaning: a live batch's 16-bit frames cleaned on the device, per lane, ahead of the
 * preparation.  A real depth camera delivers flying pixels at the hand's silhouette, at depths
 * between the hand and the background, which pass a window's depth range and enter the point
 * cloud, and isolated speckle, which the distance transform's mask takes for hand.  The rule is
 * on integers, so it is bit-exact.  F is the lane's 240x320 model image of 16-bit values -- for a
 * view lane the pick the view defines, so neighbours are MODEL-image neighbours -- and the eight
 * neighbours q of pixel p read 0 where they fall outside the image.  With u = F[p],
 *   near(q)  <=>  F[q] != 0 && |F[q] - u| <= edge      (the difference in 32-bit integers)
 *   s = the number of near neighbours
 *   out[p] = 0                       if u == 0       (a hole stays a hole: nothing is invented)
 *          = 0                       if s < support  (the flying pixel, the speckle)
 *          = sorted(C)[s / 2]        with HPE_CLEAN_MEDIAN, C = {u} + {F[q] : near(q)}, s + 1
 *                                    values ascending: the median, the lower one of an even count
 *          = u                       otherwise
 * Every output depends on the input image alone: one pass, never in place.  support = 0 without
 * the flag is the identity.  edge is in the frame's raw units.  hpe/clean.py is the rule in numpy.
 *
 * hpe_set_batch_clean gives lane b the parameters params[b] (host, B entries, read before return)
 * from the next hpe_batch_pipeline_begin_u16 / _begin_view on; params == NULL turns cleaning off
 * (the default; B is then ignored).  A cleaned batch runs one more launch per frame, k_clean_b,
 * directly ahead of the launch that prepares the lanes' next frames (at a begin, ahead of the
 * preparation): it reads each lane's pinned buffer -- every pixel once per workgroup that needs
 * it, so the rows either side of an 8-row tile's border twice, 1.25 reads per pixel in all --
 * through the lane's view on a view batch, and writes the cleaned 240x320 frame to device memory, from where the u16 preparation reads it.
 * Everything downstream -- windows, lane hands, both pacings, both batch forms, reports, seeds and
 * groups, hpe_batch_pipeline_optimise -- works unchanged, hpe_batch_frame_buffer keeps its
 * contract, and hpe_batch_pipeline_locate reads the lane's cleaned current frame.  Lane b equals,
 * bit for bit after every frame, hpe_pipeline_begin + hpe_track_pipelined on the stream cleaned on
 * the host by the rule above (after the view's reduction) and converted by the u16 rule.  The
 * parameters live in a device table, never a captured argument: other parameters replay the same
 * graphs.  While a live batch that began with cleaning on is in progress, non-NULL params of the
 * same B are accepted: the call drains the stream, rewrites the table, and the new parameters
 * apply from the next frame cleaned (the next frames of the following track call).  With cleaning
 * off a batch launches exactly what it launches without this section.
 *
 * hpe_clean_defaults (host only, no context) fills {edge = lrint(15 / unit_mm) (at least 1, at
 * most 65535), support = 3, HPE_CLEAN_MEDIAN} for frames of unit_mm millimetres per count:
 * untuned, tried on rendered scenes with synthetic camera noise only (hpe/synth.py camera_noise).
 * hpe_clean_depth_u16 applies the rule to one host frame by the same kernel, through a staging
 * buffer, and synchronises: frame is 240x320, or with a view a pitch x height camera frame; out
 * receives 240x320 values.  hpe_batch_clean_readback synchronises and copies lane `lane`'s cleaned
 * frame of buffer parity `parity` (0: the begin's frames, then alternating).
 *
 * Refused with HPE_E_ARG, nothing changed: B outside 1..HPE_BATCH_MAX, support > 8, an unknown
 * flag bit, non-zero pad; a u16 or view begin whose B differs from the B the parameters were set
 * for; null frame, params or out, an invalid view, a unit_mm that is not finite and positive;
 * parity outside 0..1, a lane outside the cleaned batch.  HPE_E_STATE: turning cleaning on or off,
 * or other parameters for another B, while a live batch is in progress; hpe_batch_pipeline_begin
 * (float frames) and hpe_track_raw_batch_dev while cleaning is set -- the rule is defined on
 * 16-bit values, and it is refused, never run another way; hpe_batch_clean_readback without a
 * cleaned batch begun on the context.  hpe_track_batch_dev prepares nothing and ignores the
 * setting, as it ignores windows. */
#define HPE_CLEAN_MEDIAN 1u
typedef struct hpe_clean {   /* 8 bytes */
    uint16_t edge;           /* raw units: a neighbour within this of the pixel is near */
    uint8_t support;         /* 0..8: near neighbours a pixel needs to stay */
    uint8_t flags;           /* HPE_CLEAN_MEDIAN or 0 */
    uint32_t pad;            /* 0 */
} hpe_clean;
int hpe_clean_defaults(float unit_mm, hpe_clean *out);
int hpe_set_batch_clean(hpe_ctx *ctx, int B, const hpe_clean *params);
int hpe_clean_depth_u16(hpe_ctx *ctx, const uint16_t *frame, const hpe_view *view,
                        const hpe_clean *params, uint16_t *out);
int hpe_batch_clean_readback(hpe_ctx *ctx, int parity, int lane, uint16_t *out);

/* The form of pso_evolve in the three batch calls above (hpe_track_batch_dev,
 * hpe_track_raw_batch_dev, hpe_batch_pipeline_begin / hpe_track_batch_pipelined).
 * HPE_BATCH_FORM_AUTO (default): as described there -- a workgroup per particle, and num_p in the
 * wave form refused.  HPE_BATCH_FORM_WAVE: every lane's pso_evolve in the wave-per-particle form
 * (k_pso_init_wb / k_pso_gen_wb on grid (workgroups of one lane, B), then the batch's final kernel
 * evaluating cal_cost(bestp) itself), whatever num_p is -- 1024 and more included -- and whatever
 * HPE_PSO_FORM says; the refine launches, the preparation and the hand-offs are the same, and so
 * is every other refusal.  Waves per particle: hpe_batch_wave_wpp(ctx, num_p, B), the single
 * call's rule applied to the LAUNCH's particle count -- the forced HPE_PSO_WPP if set at
 * hpe_create, otherwise 2 while B * num_p <= 1024 and 1 beyond.  Lane b then computes, bit for
 * bit, what the batch call's single-sequence counterpart (hpe_track_sequence_dev,
 * hpe_track_raw_sequence_dev, hpe_pipeline_begin + hpe_track_pipelined) computes on a context
 * created under HPE_PSO_FORM=wave and HPE_PSO_WPP=<that value> -- the yardstick; the two
 * waves-per-particle forms are not bit-identical to each other, nor to the workgroup form.
 * The batch graphs are keyed by the form and its waves per particle: switching back and forth
 * replays, it captures nothing again.  Any other value of form: HPE_E_ARG.  A live batch keeps
 * the form it began with: while one is in progress a different form is refused with HPE_E_STATE
 * and nothing changes (setting the form it has is HPE_OK); end the batch first.
 * When to set it: from two lanes up.  Measured on one MI355X at 256 particles per lane against
 * the default form (DESIGN.md §4.7 "Wave-form lanes"): 1.12x the tracked frames at 2 lanes, 1.5x
 * at 4, 2.0x at 8, 2.8x at 16 -- and 0.82x at one lane, which is better left on AUTO.
 * hpe_batch_wave_wpp returns 1 or 2 whatever the current form is; num_p outside 1..8192 or B
 * outside 1..HPE_BATCH_MAX: HPE_E_ARG. */
#define HPE_BATCH_FORM_AUTO 0
#define HPE_BATCH_FORM_WAVE 1
int hpe_set_batch_form(hpe_ctx *ctx, int form);
int hpe_batch_wave_wpp(hpe_ctx *ctx, int num_p, int B);

/* Lane windows: every lane of hpe_track_raw_batch_dev and of the live batch
 * (hpe_batch_pipeline_begin / hpe_track_batch_pipelined) segments its depth frames by a window of
 * its own -- an image rectangle and a depth range -- applied inside the lanes' preparation (the
 * one that rides in the refine launch), so a live camera's forearm, body and table, or the other
 * hand of a two-hand stream, never reach the cloud or the distance transform.  Two lanes that
 * name the same raw buffer then see one hand each.
 *
 * Masking rule.  Pixel (r, c) with raw value rv is kept iff row_lo <= r <= row_hi,
 * col_lo <= c <= col_hi and z_lo <= Z <= z_hi, where Z is the preparation's converted depth,
 * exactly to_cm ? (double)rv / 10. : (double)rv.  Every other pixel is read as if its raw value
 * were 0.0f, by the cloud's band workgroups and by the distance transform's mask alike.  So
 * lo > hi or a NaN bound keeps nothing, {0, 239, 0, 319, -inf, +inf} keeps everything, and the
 * windowed preparation of a frame is the plain preparation of that frame masked on the host
 * (hpe/window.py: apply) -- bit for bit.
 *
 * Pose rule (hpe_window_from_pose, and on the device under HPE_WINDOW_FOLLOW).  S: the 48
 * centres hpe_build_spheres returns for theta, bit for bit; R: the context hand's radii.  For
 * sphere j: x = S[j][0], y = S[j][1] * -1, z = S[j][2] * -1 (camera coordinates),
 *   e  = R[j] + margin_xy
 *   cl = floor((focal*(x-e) + 160.0*z) / z),  ch the same with x+e
 *   rl = floor((focal*(y-e) + 120.0*z) / z),  rh the same with y+e
 *   zl = z - (R[j] + margin_z),               zh = z + (R[j] + margin_z)
 * every product rounded before its add.  The window is
 *   col_lo = (int)min(max(min_j cl, 0), 320)    col_hi = (int)min(max(max_j ch, -1), 319)
 *   row_lo = (int)min(max(min_j rl, 0), 240)    row_hi = (int)min(max(max_j rh, -1), 239)
 *   z_lo = min_j zl                             z_hi = max_j zh
 * If any coordinate of any centre is not finite, or any z <= 0, the window is the whole frame
 * {0, 239, 0, 319, -inf, +inf} (fail open: a NaN pose after a failed refine, a hand at or
 * behind the camera).  hpe/window.py: from_spheres is the same rule in numpy.
 *
 * hpe_set_batch_window sets the mode of the context for B lanes, from the next
 * hpe_track_raw_batch_dev call or hpe_batch_pipeline_begin on:
 *   HPE_WINDOW_OFF (default)  everything as without windows; init and the margins are ignored.
 *   HPE_WINDOW_FIXED   lane b's every frame is masked by init[b].
 *   HPE_WINDOW_FOLLOW  frame 0 is masked by init[b] (hpe_window_from_pose on the lane's x0);
 *       frame g >= 1 by the pose rule, with the call's focal and these margins, on what
 *       d_states + 27 b holds when frame g-1's refine launch starts: the x0 the caller passed
 *       for g = 1, frame g-2's bestp for g >= 2 -- the newest pose there is when frame g is
 *       prepared, which happens inside frame g-1's refine launch.  A one-wave kernel per lane
 *       (k_window_b) runs before that launch, on the stream, with no synchronisation.
 * init (host, B windows) and the margins (cm) are copied; they live in device memory, so a
 * change between two calls takes effect and the tracking graphs, keyed by the mode alone,
 * replay: OFF -> FOLLOW -> OFF captures nothing the third time.  Windows work under both batch
 * forms (hpe_set_batch_form).  hpe_track_batch_dev (prepared slots) prepares nothing and ignores
 * the mode, as do the single-sequence calls.
 * hpe_window_from_pose: the pose rule on the device for one pose (host theta) with the given
 * focal and margins; synchronises.  hpe_batch_windows_readback: synchronises and copies the B
 * lane windows of one buffer parity (frame f of a call is prepared into parity f & 1, through the
 * window of that parity) to out.
 * Refused, never run another way: a mode outside 0..2, B outside 1..HPE_BATCH_MAX, a null init
 * with a mode other than OFF, a negative or non-finite margin (focal <= 0, null pointers, a
 * parity outside 0..1 in the other two calls), and a batch call or begin whose B differs from
 * the B the windows were set for -- HPE_E_ARG; hpe_set_batch_window while a live batch is in
 * progress -- HPE_E_STATE: the batch keeps the mode, windows and margins it began with, as it
 * keeps its form; hpe_batch_windows_readback before any raw or live batch -- HPE_E_STATE. */
typedef struct hpe_window {      /* 32 bytes; every bound inclusive */
    int32_t row_lo, row_hi, col_lo, col_hi;   /* rows 0..239, columns 0..319 */
    double z_lo, z_hi;           /* in the converted depth's unit (cm with to_cm) */
} hpe_window;
#define HPE_WINDOW_OFF 0
#define HPE_WINDOW_FIXED 1
#define HPE_WINDOW_FOLLOW 2
int hpe_set_batch_window(hpe_ctx *ctx, int mode, int B, const hpe_window *init,
                         double margin_xy, double margin_z);
int hpe_window_from_pose(hpe_ctx *ctx, const double theta[26], double focal,
                         double margin_xy, double margin_z, hpe_window *out);
int hpe_batch_windows_readback(hpe_ctx *ctx, int parity, int B, hpe_window *out);

/* Lane hands: every lane of the three batch calls (hpe_track_batch_dev, hpe_track_raw_batch_dev,
 * hpe_batch_pipeline_begin / hpe_track_batch_pipelined) tracks with a hand model of its own --
 * several subjects of a dataset, several people in front of a rig, or one stream under several
 * candidate hand sizes -- under both batch forms.
 *
 * hpe_set_batch_hands: hands is a host array of B entries, copied before return.  From the next
 * batch call or hpe_batch_pipeline_begin on, lane b computes everything with hands[b] -- FK, the
 * radii, the collision term, the hand-frame refine's centres and the FOLLOW window rule -- and
 * equals the single-sequence call on a context created with hands[b], bit for bit.  hands == NULL
 * (the default state): every lane uses the context's hand again; B is ignored.  The hands live in
 * one device table the lane kernels index by their lane, so a change between two calls of one
 * shape replays the tracking graphs and captures nothing.  The single-sequence calls,
 * hpe_build_spheres, hpe_eval_costs, hpe_window_from_pose, hpe_render_depth and the optimiser
 * always use the context's hand.
 * hpe_lane_window_from_pose: hpe_window_from_pose with R and S of lane `lane`'s hand (the
 * context's hand while none are set: then the two calls agree bit for bit) -- init[lane] of a
 * FOLLOW batch with lane hands.  Synchronises.
 * Refused, and nothing changes: with non-NULL hands, B outside 1..HPE_BATCH_MAX, an entry whose
 * sphere counts are not tb {2,2,2,2} / fg {4,2,2,2} (hpe_create's check) or that holds a
 * non-finite value -- HPE_E_ARG; a batch call or begin whose B differs from the B the hands were
 * set for -- HPE_E_ARG; hpe_set_batch_hands while a live batch is in progress -- HPE_E_STATE: the
 * batch keeps the hands it began with; a lane outside 0..HPE_BATCH_MAX-1 -- HPE_E_ARG. */
int hpe_set_batch_hands(hpe_ctx *ctx, int B, const hpe_hand_params *hands);
int hpe_lane_window_from_pose(hpe_ctx *ctx, int lane, const double theta[26], double focal,
                              double margin_xy, double margin_z, hpe_window *out);

/* Lane seeds and groups: N subswarms per stream as lanes of the same launches, with the best of
 * them carried to the next frame -- SURVEY 8e's independent subswarms and per-frame best-of-N
 * (hpe_subswarm_init, hpe_pick_best) on one GPU, with no communicator and no extra process.
 *
 * hpe_set_batch_seeds: seeds is a host array of B entries, copied before return.  From the next
 * hpe_track_batch_dev or hpe_track_raw_batch_dev call, or the next hpe_batch_pipeline_begin*, lane
 * b's pso_evolve draws under seeds[b] -- the normals table, the link topology and its inbox
 * counts, and the Philox key of the per-generation draws -- in both batch forms, at one and two
 * waves per particle: lane b equals the single-sequence call on a context after
 * hpe_set_seed(seeds[b]), bit for bit.  seeds == NULL (the default state): every lane uses the
 * context's seed again; B is ignored.  Two lanes may hold the same seed.  The refine draws nothing
 * and is untouched.  hpe_pso_optimise_batch and hpe_batch_pipeline_optimise keep the context's
 * seed for every lane.  The seeds live in device tables built at the next batch call for its
 * num_p and maxiter; new seeds between two calls of one shape rewrite the tables in place (the
 * stream drained) and replay the tracking graphs -- nothing is captured -- unless the largest
 * informant in-degree K over the seeds changes, which sizes the lanes' inboxes: then the graphs of
 * the batch calls are captured again.
 *
 * hpe_set_batch_groups: sizes is a host array of n_groups positive entries summing to B; group g
 * is the next sizes[g] consecutive lanes.  n_groups == 0 or sizes == NULL turns groups off (the
 * default state).  With groups on, after every tracked frame of every group, in all three batch
 * calls: lane b's own result {bestp, cost} is kept in an own-rows table of B x 27 doubles in
 * device memory (hpe_batch_group_rows), and every row of the group in d_states -- and the lanes'
 * d_hist rows of that frame -- becomes the group's best own row by hpe_pick_best's rule: the
 * smallest cost wins, a NaN cost never wins, ties go to the lowest lane, and a group whose costs
 * are all NaN takes its lowest lane's row.  The next frame's refine reads its lane's row of
 * d_states as ever, so whatever writes rows between two calls keeps working
 * (hpe_batch_pipeline_optimise, hpe_batch_pipeline_locate, a caller's own write ordered on the
 * stream); reports carry the lane's row of d_states, the picked one; FOLLOW windows follow the
 * picked pose.  No pick happens before a group's first frame: each lane starts from the row the
 * caller gave it.  A group of one lane behaves bit for bit like no group.  The caller passes the
 * same frames for every lane of a group; nothing checks that it does.
 * Free pacing (HPE_PACING_FREE): a group advances as one.  In the begin and in every track call
 * the entries of a group's lanes are all NULL or all non-NULL, else HPE_E_ARG and nothing
 * changes; a group that idles in a call keeps its rows of d_states and its own rows bit for bit.
 *
 * hpe_batch_group_pick: the same pick on arbitrary rows, asynchronous on hpe_stream(ctx).
 * d_states is device memory, B x 27; every group's rows are replaced by the group's best row.
 * After hpe_batch_pipeline_optimise over a group it starts the group from its best
 * initialisation.  It does not touch the own-rows table.
 * hpe_batch_group_rows: synchronises and copies the own-rows table, B x 27, to host memory: each
 * lane's own result of the last frame it tracked.
 *
 * Refused, and nothing changes: B outside 1..HPE_BATCH_MAX (with non-NULL seeds or sizes), sizes
 * that are not positive or do not sum to B, a batch call or begin (or hpe_batch_group_pick,
 * hpe_batch_group_rows) whose B differs from the B the seeds or groups were set for, null
 * d_states or rows_out -- HPE_E_ARG; either setter while a live batch is in progress --
 * HPE_E_STATE: the batch keeps what it began with, as it keeps its form, windows, hands and
 * pacing; hpe_batch_group_pick with no groups set, hpe_batch_group_rows before any grouped frame
 * was tracked since the groups were set -- HPE_E_STATE; a batch call under seeds of which one has
 * an informant in-degree above the inbox bound (24) -- HPE_E_ARG, as for the context's seed. */
int hpe_set_batch_seeds(hpe_ctx *ctx, int B, const uint64_t *seeds);
int hpe_set_batch_groups(hpe_ctx *ctx, int B, int n_groups, const int32_t *sizes);
int hpe_batch_group_pick(hpe_ctx *ctx, int B, double *d_states);
int hpe_batch_group_rows(hpe_ctx *ctx, int B, double *rows_out);

/* Lane pacing: whether the lanes of a live batch (hpe_batch_pipeline_begin /
 * hpe_track_batch_pipelined) advance in lockstep.  Cameras of a rig are not frame-locked: a 30 Hz
 * and a 60 Hz camera share it, a USB camera drops a frame, a person leaves one view.
 *
 * hpe_set_batch_pacing sets the mode of the context, read at hpe_batch_pipeline_begin; a live
 * batch keeps the pacing it began with, as it keeps its form, windows and hands.
 *   HPE_PACING_LOCKSTEP (default)  everything as described above: a frame for every lane or for
 *       none, in the begin and in every call.
 *   HPE_PACING_FREE  a lane with no new frame idles for that call, and a lane may start empty and
 *       join later:
 *     begin.  depth_mm[b] may be NULL: lane b starts empty, nothing is copied or prepared for it.
 *       At least one entry must be non-NULL (HPE_E_ARG).  A lane is PENDING iff it was given a
 *       frame.
 *     hpe_track_batch_pipelined with a non-NULL next_depth_mm array.  Any subset of its entries
 *       may be NULL, all of them included.  Lane b tracks its current frame in this call iff it
 *       is pending; its next frame is copied and prepared iff next_depth_mm[b] != NULL; afterwards
 *       it is pending iff next_depth_mm[b] != NULL.  The batch stays alive even if no entry is
 *       set: a call in which no lane is pending (prepare-only) and a call in which every entry is
 *       NULL (track-only) are both legal.
 *     next_depth_mm == NULL (the array itself) tracks the pending lanes and ends the batch.
 *     An idle lane is untouched.  For a lane that does not track in a call, its 27 doubles in
 *       d_states and its refine evaluation counter are bit for bit what they were.  The caller
 *       may rewrite such a lane's row between two calls (re-initialising after a pause): a write
 *       ordered on hpe_stream(ctx) takes effect.  A lane that joins reads its row when its first
 *       frame is tracked, not before (under HPE_WINDOW_FOLLOW: when that frame is accepted, for
 *       its window -- below).
 *     The yardstick.  Let F0 .. Fm-1 be the frames lane b was given, in order, whatever calls
 *       they arrived in.  Lane b's state after the call that tracks Fi equals, bit for bit, state
 *       i of the single loop on the same context with the same form and refine form:
 *       hpe_pipeline_begin(F0), then hpe_track_pipelined(..., Fi+1).  If the caller rewrote the
 *       lane's row while it idled, the comparison is against the single loop restarted from that
 *       row.
 *     Windows.  HPE_WINDOW_FIXED is unchanged.  HPE_WINDOW_FOLLOW: a frame given to the begin is
 *       masked by init[b]; the window of any later frame is the pose rule on what d_states + 27 b
 *       holds when the call that accepts that frame starts its launches -- the lane's newest pose
 *       at that moment, whether or not the lane also tracks in that call.  The window of a lane
 *       that accepts no frame in a call stays as it was.
 *     Lane hands, both batch forms and both refine forms are supported, with their yardsticks.
 *     Frame publication happens once per call whatever the lanes do, and the host's bounded wait
 *       before it refills a pinned buffer (HPE_E_HIP on a timeout) is the lockstep batch's.
 * The masks never enter a graph's key: one table of 16 activity words in device memory, written
 * on the stream before each frame's graph, decides in the kernels which lanes run.  A batch with
 * arbitrary masks captures at most three graphs (two buffer parities with preparation, the ending
 * frame); a second batch of that shape with other masks captures none; the lockstep graphs are
 * their own.
 * hpe_set_batch_pacing: a mode outside 0..1 -- HPE_E_ARG; another mode while a live batch is in
 * progress -- HPE_E_STATE, and nothing changes (the mode the batch has is HPE_OK).  The resident
 * batch calls (hpe_track_batch_dev, hpe_track_raw_batch_dev) and the single-sequence calls ignore
 * the mode.
 * hpe_batch_pending: bit b of *mask_out set: lane b holds a prepared frame that the next
 * hpe_track_batch_pipelined will track (under LOCKSTEP: every lane of the batch).  Host
 * bookkeeping only, no synchronisation.  HPE_E_STATE without a live batch; a null pointer --
 * HPE_E_ARG.
 * When to set it: when the streams are not frame-locked.  Measured on one MI355X at 256 particles
 * per lane (DESIGN.md §4.7 "Lane pacing"): a free-paced batch whose lanes all have every frame
 * runs about 1 % slower than the lockstep batch, at one lane as at 4 and 16 and in both batch
 * forms (+0.7 to +1.4 % where the session's spread allowed a reading) -- the entry test of the
 * ~34 launches of a frame; the activity words themselves are written only when they change.  With
 * a staggered drop of one frame in 4 per lane it tracks 1.12x to 1.31x the frames of the only
 * course open without it, ending the batch and beginning another at every change of the lane set
 * (1.08x to 1.21x at one frame in 2).  A rig whose lanes are frame-locked is better left on
 * LOCKSTEP. */
#define HPE_PACING_LOCKSTEP 0   /* default: everything as without pacing */
#define HPE_PACING_FREE 1
int hpe_set_batch_pacing(hpe_ctx *ctx, int mode);
int hpe_batch_pending(hpe_ctx *ctx, uint32_t *mask_out);

/* Lane initialisation: the first pose of every lane of a batch, by pso_optimise in the SAME
 * launches (grid num_p x lanes; 2 (maxiter-1) + 3 launches per call whatever B is).
 *
 * hpe_pso_optimise_batch: B lanes on stored slots.  Lane b is
 *   hpe_select_frame(ctx, slots[b]); hpe_pso_optimise(ctx, x0 = d_states[27 b ..], num_p, ...)
 * bit for bit on a context created with lane b's hand (hpe_set_batch_hands; the context's own
 * hand while none are set) under the same seed and PSO parameters: bestp, cost and the gbest
 * trace.  d_states: device, B x 27 {x0 -> bestp, cost}.  slots: host, B entries (copied before
 * return; lanes may share a slot).  d_trace (device, optional): B x (maxiter-1), row b = lane b's
 * gbest cost after each generation.  Asynchronous on hpe_stream(ctx): x0 is read and the result
 * written on the device, there is no host synchronisation, and the call waits on the stream for
 * slots still being prepared (hpe_prepare_frame), as hpe_track_batch_dev does.  With maxiter <= 1
 * (no generation) the result is the initial swarm's best, as in the single call.  The selected
 * frame stays as it was; hpe_pso_trace and hpe_refine_eval_count are not touched; a later
 * hpe_prepare_frame waits for the call.
 *
 * hpe_batch_pipeline_optimise: the same on a live batch's CURRENT prepared frames -- the
 * descriptors of the buffer parity the next hpe_track_batch_pipelined tracks -- through the
 * lanes' windows (the frames are the masked ones) and hands.  lanes: bit b set = lane b is
 * optimised; the other lanes' rows of d_states (and of d_trace) are left bit for bit untouched,
 * and no workgroup is launched for them.  It changes nothing of the live batch's own state
 * (parity, pending mask, frame numbers, pinned buffers): the tracking call that follows reads the
 * optimised rows as its x0.  The use: frame 0 of a rig, a lane that joins late under
 * HPE_PACING_FREE, a lane that lost its hand and is re-initialised (the policy is the caller's).
 *
 * Refused, never run another way, and a refusal changes nothing: B outside 1..HPE_BATCH_MAX, null
 * d_states or slots, a slot that holds no frame or more than 2048 cloud points (the lane form is
 * the staged descent), lanes == 0 or a bit at or above B -- HPE_E_ARG; num_p outside 1..8192 --
 * HPE_E_ARG; hpe_set_pso_params not called, lane hands set for another B, no live batch or a B
 * other than the begin's, a selected lane that holds no prepared frame (not in hpe_batch_pending)
 * -- HPE_E_STATE.
 * When to use it: whenever more than one lane needs a first pose, or a lane needs its own hand or
 * its live frame.  Measured on one MI355X at num_p = 32, maxiter = 200, 250-point frames
 * (DESIGN.md §4.7 "Lane initialisation"): one call for 2 / 4 / 8 / 16 lanes takes 64.7 / 67.9 /
 * 70.9 / 122.1 ms against 61.2 ms per lane of B consecutive hpe_pso_optimise calls (1.9x, 3.6x,
 * 7.0x, 8.1x): a lane fills 32 of the 256 CUs, so up to 8 lanes cost about one lane's time and 16
 * lanes two rounds.  At ONE lane it is 0.2-0.3 % slower than hpe_pso_optimise (two small launches
 * more): there it offers only what the single call cannot do -- the lane's hand, a live lane's
 * frame, no host synchronisation. */
int hpe_pso_optimise_batch(hpe_ctx *ctx, int num_p, int B, double *d_states,
                           const int32_t *slots, double *d_trace);
int hpe_batch_pipeline_optimise(hpe_ctx *ctx, int num_p, int B, double *d_states,
                                uint32_t lanes, double *d_trace);

/* Lane reports: every tracked frame of a live batch's lane, delivered to the host by the device
 * inside the frame's graph -- no stream synchronisation, no device-to-host copy.
 *
 * hpe_set_batch_report(depth, watch): depth 0 (default) is off, and everything runs as without
 * reports.  depth in 2..64 gives every lane a ring of `depth` slots in pinned, mapped, coherent
 * host memory; a slot is {begin word, hpe_lane_report, end word} padded to 1152 bytes, and slot
 * (seq - 1) % depth holds the lane's report number seq.  After the final launch of every
 * hpe_track_batch_pipelined one more launch (k_report_b, one wave per lane, part of the frame's
 * graph) writes a TRACK report for every lane that tracked in the call (an idle lane of a
 * free-paced batch writes nothing); hpe_batch_pipeline_optimise writes an INIT report for each
 * lane it selected.  A report holds the lane's row of d_states bit for bit, the hand's 21 joints
 * at that pose under the LANE's hand (rows as hpe_build_spheres' joints_out: wrist, index ..
 * little joints 1-4, thumb 1-4; camera coordinates, cm), each joint's pixel position
 *   column = (focal x + 160 z) / z,  row = (focal y + 120 z) / z
 * (fp64, every product rounded before its add; both NaN when a coordinate is not finite or
 * z <= 0; hpe.report.project_joints is the host mirror), the frame's point count n -- the points
 * the preparation found in the frame (through the lane's window) BEFORE downsampling, what
 * hpe_preprocess_depth returns in n_out with downsample = 0: the tracked cloud itself always
 * holds 250 points, even of an empty frame -- the batch's frame number and the lane's health flags.
 *
 * The watch rule (the thresholds are the caller's; NULL means {+inf, 0, 0}, which never holds):
 * a TRACK report is SUSPECT iff !(cost <= cost_max) || n < n_min -- a NaN cost is suspect.
 * bad_streak counts the lane's consecutive SUSPECT TRACK reports (a device word per lane, zeroed
 * by a healthy report, by an INIT report and by the begin); LOST is set iff streak > 0 &&
 * bad_streak >= streak.  The library only reports: the application re-initialises a lost lane
 * with hpe_batch_pipeline_optimise.
 *
 * The setting is read at hpe_batch_pipeline_begin, which resets every lane's seq to 0 and clears
 * the rings; the rings survive the end of a batch and stay readable until the next begin.
 * Changing the setting while a live batch is in progress is HPE_E_STATE and changes nothing.
 * Any other depth, or a watch with streak < 0 or n_min < 0: HPE_E_ARG.
 *
 * hpe_batch_report never blocks and never touches the stream: seq == 0 asks for the lane's newest
 * complete report (out->seq == 0: none yet); a specific seq that is not in the ring, not yet or
 * no longer, is HPE_E_STATE.  hpe_batch_report_wait waits, at most timeout_ms, for that report to
 * complete; seq == 0 there is the last report enqueued for the lane (out->seq == 0 if none was);
 * HPE_E_HIP on expiry.  hpe_batch_lost ORs bit b for every lane b whose newest report has
 * HPE_REPORT_F_LOST.  A lane outside the batch or a null out: HPE_E_ARG; no batch with reports
 * begun: HPE_E_STATE.
 *
 * hpe_lane_joints_dev: the same joints and pixels for the resident batches, from their history:
 * row b n + f of d_hist (27 doubles) under lane b's hand, into d_joints[b][f][21][3] and, if
 * d_px is non-null, d_px[b][f][21][2] (device memory).  Asynchronous on hpe_stream(ctx).
 * HPE_E_ARG: B outside 1..HPE_BATCH_MAX, n < 1, null d_hist or d_joints, focal <= 0 with a
 * non-null d_px. */
#define HPE_REPORT_TRACK 1          /* kind: a tracked frame */
#define HPE_REPORT_INIT  2          /* kind: hpe_batch_pipeline_optimise wrote the lane's row */
#define HPE_REPORT_F_NAN     1      /* a state entry is not finite */
#define HPE_REPORT_F_EMPTY   2      /* n == 0 */
#define HPE_REPORT_F_SUSPECT 4      /* the watch rule held for this frame */
#define HPE_REPORT_F_LOST    8      /* ... for `streak` consecutive TRACK reports of the lane */
typedef struct hpe_lane_report {    /* 1096 bytes, every field naturally aligned */
    uint64_t seq;                   /* this lane's report number since the begin, from 1 */
    uint64_t call;                  /* the batch's frame number, the one the final launch publishes */
    int32_t lane, kind, n, flags, bad_streak, pad;
    double state[27];               /* the lane's row of d_states {bestp, cost}, bit for bit */
    double joints[21][3];           /* hand_joints rows, as hpe_build_spheres' joints_out */
    double px[21][2];               /* {column, row} of each joint in the 320x240 image */
} hpe_lane_report;
typedef struct { double cost_max; int32_t n_min; int32_t streak; } hpe_report_watch;

size_t hpe_lane_report_size(void);
int hpe_set_batch_report(hpe_ctx *ctx, int depth, const hpe_report_watch *watch);
int hpe_batch_report(hpe_ctx *ctx, int lane, uint64_t seq, hpe_lane_report *out);
int hpe_batch_report_wait(hpe_ctx *ctx, int lane, uint64_t seq, int timeout_ms, hpe_lane_report *out);
int hpe_batch_lost(hpe_ctx *ctx, uint32_t *mask_out);
int hpe_lane_joints_dev(hpe_ctx *ctx, int B, int n, const double *d_hist, double focal,
                        double *d_joints, double *d_px);

/* Lane location: where the hand is in a lane's raw depth frame, found on the device -- the first
 * window and pose of a rig's lane, and both again for a lane whose report says LOST.  A camera
 * delivers neither a segmented hand nor a pose: without this the application pulls the frame to
 * the host, segments it there and pushes a window and a pose back.  With it the loop closes on the
 * device: begin -> locate -> optimise -> track -> LOST -> locate -> optimise -> track.
 *
 * The location rule (hpe/locate.py is the same rule in numpy, and the device result equals it bit
 * for bit, doubles included).  Input: one raw 240x320 frame, float mm or 16-bit pixels of unit_mm
 * each (rv = (float)u * unit_mm, the u16 batch's rule), to_cm, focal and hpe_locate_params.
 * Z = to_cm ? (double)rv / 10. : (double)rv, the preparation's own expression.  A pixel is VALID
 * iff rv is finite, rv > 0 and it lies inside `search` in row, column and Z (the masking rule's
 * comparisons, every bound inclusive).  Its depth bin is k = min(K-1, (int)floor(Z / bin)),
 * K = 2048 (one fp64 division; the clamp is made in fp64, before the conversion).
 *   1. Histogram of k over the valid pixels; k_near = the smallest k whose cumulative count
 *      exceeds `skip` (that many nearest pixels are ignored: speckle).  None: found = 0, and
 *      k_near = -1.
 *   2. Pass 1: the valid pixels with k_near <= k <= k_near + sb, sb = (int)ceil(slab / bin):
 *      integer sums m1, Sr, Sc, Sk; r1 = (double)Sr / (double)m1, c1 likewise,
 *      z1 = ((double)Sk / (double)m1 + 0.5) * bin.
 *   3. The box around (r, c, z): hx = (focal * half_xy) / z; rows ceil(r - hx) .. floor(r + hx),
 *      columns likewise, each bound clamped in fp64 to the image and to `search` before its
 *      conversion to int, as the pose rule clamps:
 *        row_lo = (int)min(max(ceil(r - hx), max(0, search.row_lo)), 240)
 *        row_hi = (int)min(max(floor(r + hx), -1), min(239, search.row_hi))     (columns: 320, 319)
 *      depth max(z - half_z, search.z_lo) .. min(z + half_z, search.z_hi).
 *   4. Pass 2: the valid pixels inside the box around (r1, c1, z1), by row, column and Z: sums m2,
 *      Sr, Sc, Sk.  m2 < min_pixels (or m2 == 0): found = 0.  Otherwise (r2, c2, z2) as in pass 1.
 *   5. found = 1; window = the box around (r2, c2, z2); px = {c2, r2}; centre =
 *      {((c2 - 160.0) * z2) / focal, ((r2 - 120.0) * z2) / focal, z2}: camera coordinates, the
 *      inverse of the reports' pixel rule.
 * A result that is not found carries the counts it reached (k_near, m1, m2) and zeros for px,
 * centre and window.  The rule finds the object nearest the camera inside `search`: keeping the
 * body and the other hand out of `search` is the caller's part, as it is for the lane windows.
 * hpe_locate_defaults fills {the whole frame, 0.5, 12, 11, 11, 20, 200} (cm with to_cm): untuned
 * values, tried on rendered scenes only (DESIGN.md 4.7 "Lane location").
 *
 * The placement rule.  Given a pose T[26] -- the caller's guess of rotation and digits, the
 * reference's x0 for instance -- the lane's row becomes T with theta 3..5 replaced by
 * T[3..5] + (centre - cen), cen the mean of the 48 sphere centres of T under the lane's hand in
 * camera coordinates (hpe_build_spheres' centres with y and z negated back, summed in sphere order,
 * divided by 48).  theta 3..5 is a camera-frame translation, so the row's sphere centroid lands on
 * centre (to the FK's 1e-9 cm).  The row's 27th entry is left as it is.
 *
 * hpe_locate_depth: the rule alone on one host frame (u16 != 0: 16-bit pixels), synchronous,
 * through a staging buffer of the context; params == NULL: the defaults; out->seq and out->lane
 * are 0.  Single-sequence users then mask with hpe/window.py: apply.
 *
 * hpe_batch_pipeline_locate: on a live batch, for the lanes of `lanes` (bit b = lane b), which must
 * hold a prepared frame (hpe_batch_pending).  Asynchronous on hpe_stream(ctx), three launches:
 *   1. k_locate_b, one workgroup per lane, on the lane's CURRENT raw frame -- the pinned buffer of
 *      the parity the next track call tracks, read in place.  It stays intact until the track call
 *      after that, in-place-filled buffers included: the locate call marks the buffers in use
 *      until the next track call's frame has completed, so a host that runs ahead of the device
 *      waits there (that track call's copy, hpe_batch_frame_buffer) exactly as it waits for a
 *      frame that is still being prepared.
 *   2. A found lane's window goes into the window table: both parities under HPE_WINDOW_FIXED, the
 *      current parity under HPE_WINDOW_FOLLOW (the next call's pose rule takes over as ever).  Its
 *      current frame is PREPARED AGAIN through that window (the begin's preparation kernel, gated
 *      by an activity table the locate kernel filled).
 *   3. The placed row is written to d_states + 27 b.  tmpl: host, B x 26, read before return.
 *   params: host, B entries, or NULL for the defaults in every lane; only the selected lanes'
 *   entries are read and checked.
 * An unselected lane, and a selected lane that is not found, stays untouched: its window in both
 * parities, its prepared frame, its row, its pending state and its hand-off counters, bit for bit.
 * Nothing of the batch's own state changes (parity, pending mask, frame numbers), and no tracking
 * graph is captured or invalidated: the windows live in device memory.
 *
 * hpe_batch_locate_result: lane `lane`'s newest result, from a small table in pinned mapped host
 * memory that the locate kernel publishes with the report ring's begin / end words; seq counts the
 * lane's locates since the begin.  It waits, at most timeout_ms, for the last locate enqueued for
 * the lane (none since the begin: out->seq == 0 at once) and does not synchronise the stream;
 * HPE_E_HIP on expiry.
 *
 * Refused, and a refusal changes nothing: a null pointer, bin <= 0 or not finite, a negative or
 * non-finite slab or half size, a negative skip or min_pixels, focal <= 0 or not finite, a u16
 * unit_mm not finite or <= 0, lanes == 0 or a bit at or above B, a lane outside the batch --
 * HPE_E_ARG; no live batch or a B other than the begin's, window mode OFF (the table is not read
 * then), a selected lane that holds no prepared frame -- HPE_E_STATE. */
typedef struct hpe_locate_params {
    hpe_window search;      /* where to look: rectangle and depth range, bounds inclusive */
    double bin;             /* depth quantum in the converted unit (cm with to_cm), > 0 */
    double slab;            /* pass 1: depth extent behind the nearest depth */
    double half_xy, half_z; /* half sizes of the hand box */
    int32_t skip;           /* that many nearest valid pixels are ignored (speckle), >= 0 */
    int32_t min_pixels;     /* fewer pixels in the box: not found */
} hpe_locate_params;
typedef struct hpe_locate {     /* 104 bytes, every field naturally aligned */
    uint64_t seq;               /* the lane's locates since the begin, from 1 (hpe_locate_depth: 0) */
    int32_t lane, found, k_near, m1, m2, pad;
    double px[2];               /* {column, row} of the located centre */
    double centre[3];           /* camera coordinates, converted unit */
    hpe_window window;
} hpe_locate;
int hpe_locate_defaults(hpe_locate_params *p);
int hpe_locate_depth(hpe_ctx *ctx, const void *frame, int u16, float unit_mm, int to_cm,
                     double focal, const hpe_locate_params *params, hpe_locate *out);
int hpe_batch_pipeline_locate(hpe_ctx *ctx, int B, double *d_states, uint32_t lanes,
                              const double *tmpl, const hpe_locate_params *params);
int hpe_batch_locate_result(hpe_ctx *ctx, int lane, int timeout_ms, hpe_locate *out);

/* Kernel timing with HIP events on the context stream (bench instrumentation).
 * While enabled, every dispatch of the profiled kernels is launched through
 * hipExtLaunchKernel with a start/stop event pair (dispatch-packet timestamps: the
 * kernel's own execution interval, as rocprofv3 --kernel-trace reports it).
 * hpe_profile_read_kernel synchronises and returns the launch count and total/min/max
 * device milliseconds of one kernel since the last enable; hpe_profile_read is
 * hpe_profile_read_kernel(HPE_PROF_PSO_GEN). */
#define HPE_PROF_PSO_GEN 0   /* k_pso_gen: one fused PSO generation */
#define HPE_PROF_REFINE 1    /* k_refine: refine_init_pose (+ fused next-frame preparation) */
#define HPE_PROF_PSO_INIT 2  /* k_pso_init */
#define HPE_PROF_PSO_FINAL 3 /* k_pso_final */
#define HPE_PROF_PREP 4      /* k_preprocess (hpe_prepare_frame, preprocessing stream) */
#define HPE_PROF_OPT_DESCENT 5 /* k_opt_descent: pso_optimise descent phase */
#define HPE_PROF_OPT_MOVE 6    /* k_opt_move: pso_optimise velocity / cost phase */
#define HPE_PROF_SWARM_BEST 7 /* k_swarm_best: a subswarm's best for the per-generation exchange */
#define HPE_PROF_EXCHANGE 8   /* the per-frame subswarm exchange (RCCL all-gather + k_pick_best) */
#define HPE_PROF_KERNELS 9
int hpe_profile_enable(hpe_ctx *ctx, int on);
int hpe_profile_read(hpe_ctx *ctx, int32_t *launches, double *total_ms, double *min_ms,
                     double *max_ms);
int hpe_profile_read_kernel(hpe_ctx *ctx, int kernel, int32_t *launches, double *total_ms,
                            double *min_ms, double *max_ms);
/* Evaluations done by refine_init_pose launches (cal_cost2 calls, PSO.cpp:216-266) since
 * the context was created or last reset (bench instrumentation: the algorithmic work of
 * the k_refine launches).  Synchronises; reset != 0 zeroes the count after reading. */
int hpe_refine_eval_count(hpe_ctx *ctx, uint64_t *total, int reset);

/* Number of graphs this context has captured (tracking graphs are captured once per shape
 * and replayed; tests check that a replay captured nothing). */
int hpe_graph_captures(const hpe_ctx *ctx, uint64_t *n);

/* Diagnostic build only (libhpe_stamps.so): per-phase shader-clock cycle sums
 * [0..31] and lap counts [32..63] of block 0, reset on read.  Returns 1 in the
 * stamps build, 0 in the product build (all zeros). */
int hpe_debug_stamps(unsigned long long *out64);

/* Synthetic 240x320 depth (float mm, zero background) of the 48-sphere model at
 * pose theta: front-most ray/sphere hit per pixel centre under K(focal).  Bench /
 * test input generator (no MSRA data on the box). */
int hpe_render_depth(hpe_ctx *ctx, const double theta[26], double focal, float *depth_mm_out);

#ifdef __cplusplus
}
#endif
#endif
