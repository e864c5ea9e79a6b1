// hpe_api.inc -- host implementation of include/hpe.h (included at the end of
// hpe_kernels.hip so the launches see the kernel templates).
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <mutex>

#include <hip/hip_ext.h>
#include <rccl/rccl.h>  // types only: RCCL itself is opened at run time (rccl_api)

#include "../../include/hpe.h"
#include "hpe_host.hpp"
#include "hpe_own.hpp"

namespace {

#define HPE_RAW_RING 8  // pinned staging buffers for raw depth frames in flight

struct Slot {
    DevBuf<double> cx, cy, cz, depth;
    DevBuf<float> dt;
    int n = 0, cap = 0;
    double scale = 0, dtmax = 0, K[9] = {0};
    bool valid = false;
    // prepared on the device (hpe_prepare_frame): n / scale / dtmax live in HBM until a
    // host-side call needs them (known == false); n_max bounds n without a readback
    bool dev = false, known = true;
    int n_max = 0;
    Event ready;  // prep stream: frame written
    Event done;   // main stream: last work that read the frame
    bool done_valid = false;
};
static_assert(std::is_nothrow_move_constructible<Slot>::value, "std::vector<Slot> grows by moving");

struct Swarm {
    int P = 0, G = -1, K = 0;
    uint64_t seed = 0;
    DevBuf<double> xh, pch, pb, inbox, ibtc, v, gpos, normals, bounds, trace_g;
    DevBuf<unsigned long long> gmin;
    DevBuf<int> trace_count, trace_topo, outl;
    DevBuf<Sig> sig;
    std::vector<InboxCounts> kin;  // per generation 0..G (P <= KIN_MAX)
    // hpe_track_batch_dev: the mutable arrays (xh, pch, pb, v, inbox, gmin, sig, gpos, and last
    // ibtc, which only wave-form lanes touch) of `lanes` lanes, one arena per lane `stride` bytes
    // apart; off[]: the arrays within an arena.
    // The arrays above stay the single-sequence calls' own (their cached graphs keep them).
    DevBuf<char> arena;
    size_t stride = 0, off[9] = {0};
    int lanes = 0;
    // hpe_set_batch_seeds: the lanes' own draw tables for (P, G, tab_seeds) -- a copy of normals
    // and of outl per lane, back to back, the inbox counts [lane][g] and the LaneSeeds entry that
    // names them -- and what the arenas were last used under: arena_seeds (empty: the context's
    // seed) and laneK, the K that sizes their inboxes (the largest over arena_seeds; K itself
    // while no seeds are set).  ensure_lane_seeds keeps all of it.
    DevBuf<double> lane_normals;
    DevBuf<int> lane_outl;
    DevBuf<InboxCounts> lane_kin;
    DevBuf<LaneSeeds> lane_ls;
    std::vector<uint64_t> tab_seeds, arena_seeds;
    int tab_lanes = 0, tab_K = 0, laneK = 0;  // (tab_K: the largest K over tab_seeds)
};

// RCCL entry points of the library's own subswarm exchange (hpe_subswarm_init), opened at
// first use: the process's RCCL when one is loaded already (torch's, matched by soname),
// else the system one.  libhpe.so itself links no RCCL, so loading it needs none.
struct RcclApi {
    bool ok = false;
    char why[256] = {0};
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclGetVersion) get_version = nullptr;
};

const RcclApi &rccl_api() {
    static RcclApi a;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            snprintf(a.why, sizeof(a.why), "RCCL not found: %s", dlerror());
            return;
        }
        a.get_unique_id = (decltype(a.get_unique_id))dlsym(h, "ncclGetUniqueId");
        a.comm_init_rank = (decltype(a.comm_init_rank))dlsym(h, "ncclCommInitRank");
        a.all_gather = (decltype(a.all_gather))dlsym(h, "ncclAllGather");
        a.comm_destroy = (decltype(a.comm_destroy))dlsym(h, "ncclCommDestroy");
        a.error_string = (decltype(a.error_string))dlsym(h, "ncclGetErrorString");
        a.get_version = (decltype(a.get_version))dlsym(h, "ncclGetVersion");
        a.ok = a.get_unique_id && a.comm_init_rank && a.all_gather && a.comm_destroy &&
               a.error_string && a.get_version;
        if (!a.ok) snprintf(a.why, sizeof(a.why), "RCCL lacks an entry point");
    });
    return a;
}

struct OptState {  // pso_optimise buffers, rebuilt when P / G / seed / cloud bound grow
    int P = 0, G = -1, n_cap = 0;
    uint64_t seed = 0;
    DevBuf<double> x, v, pb, pc, gbest, trace, normals, bounds;
    DevBuf<int32_t> match;
    DevBuf<unsigned> ctr;
};

// The lane forms' state (hpe_pso_optimise_batch, hpe_batch_pipeline_optimise): per lane one
// arena {x, v, pb, pc, gbest, trace, ctr}, `stride` bytes apart (off[]: the arrays within an
// arena, each on a 128-byte line of its own), the shared normals and bounds, and the slot
// call's descriptor table.  Grown, never shrunk; rebuilt when P or the seed changes or G
// outgrows the trace.  No graph holds any of it: the calls launch directly.
struct OptLanes {
    int P = 0, G = -1, lanes = 0;
    uint64_t seed = 0;
    DevBuf<char> arena;
    size_t stride = 0, off[7] = {0};
    DevBuf<double> normals, bounds;
    double bounds_h[3 * HPE_DOF] = {0};  // what `bounds` holds
    bool bounds_set = false;
    DevBuf<DevObs> d_obs;  // [HPE_BATCH_MAX]
    void reset() {  // everything but the descriptor table
        arena.reset(), normals.reset(), bounds.reset();
        P = 0, G = -1, lanes = 0, bounds_set = false;
    }
};

// What a captured tracking graph depends on besides the context's seed and epoch: one key for
// the tracking calls, a field a call does not use left zero.  A launch decision that is not
// in the key replays the wrong kernels (a cached chunk of 250-point frames on 400-point ones).
struct GraphKey {
    int P, G, refine, k;
    // bit i: frame i of the chunk takes the staged refine (n_max <= RF_STAGE_MAX) / the FILT
    // kernels (n_max > HPE_NT / 2, launch_pso's choice)
    unsigned staged, filt;
    int parity, tail_next, next, cur, B, to_cm, downsample;
    int wave;  // a batch in the wave form (hpe_set_batch_form): its waves per particle; else 0
    int win;   // the lane windows' mode (hpe_set_batch_window): other kernels, one more launch
    int hands; // lane hands are set (hpe_set_batch_hands): the lane kernels that index the table
    int pacing; // a live batch's pacing (hpe_set_batch_pacing): FREE takes the idle-aware kernels
    int report; // lane reports are on (hpe_set_batch_report): one more launch, k_report_b; else 0
    int u16;    // a live batch of 16-bit frames (hpe_batch_pipeline_begin_u16): the u16 ring
                // kernels; never its depth unit, which device memory holds
    int view;   // ... read through lane views (hpe_batch_pipeline_begin_view): the view kernels;
                // never a view, which device memory holds too
    int seeds;  // lane seeds are set (hpe_set_batch_seeds): the SEEDS kernels; never a seed, which
                // device memory holds
    int groups; // lane groups are set (hpe_set_batch_groups): one more launch, k_group_pick; never
                // a group, which device memory holds
    int clean;  // lane cleaning is on (hpe_set_batch_clean): one more launch, k_clean_b, and the
                // u16 preparation on the staging frames; never a parameter, which device memory holds
    double focal;
    const void *in;  // the raw frames' base
    double *state, *hist;  // a lane's or the batch's states; the history rows
    bool operator==(const GraphKey &o) const {  // written out: the struct has padding
        return P == o.P && G == o.G && refine == o.refine && k == o.k && staged == o.staged &&
               filt == o.filt && parity == o.parity && tail_next == o.tail_next &&
               next == o.next && cur == o.cur && B == o.B && wave == o.wave && win == o.win &&
               hands == o.hands && pacing == o.pacing && report == o.report && u16 == o.u16 &&
               view == o.view && seeds == o.seeds && groups == o.groups && clean == o.clean &&
               to_cm == o.to_cm &&
               downsample == o.downsample && focal == o.focal && in == o.in &&
               state == o.state && hist == o.hist;
    }
};

// The fields every call sets; the rest zero until the call fills in its own.
GraphKey graph_key(int P, int G, int refine, double *state, double *hist = nullptr) {
    GraphKey key{};
    key.P = P;
    key.G = G;
    key.refine = refine;
    key.state = state;
    key.hist = hist;
    return key;
}

// One tracking call's captured graphs (run_graphed).  At `cap` entries the next capture empties
// the cache; drop_stale: it also drops the graphs of another seed or epoch, which never match.
struct GraphCache {
    struct Entry {
        GraphKey key;
        uint64_t seed;
        unsigned epoch;
        hipGraphExec_t exec;
    };
    std::vector<Entry> entries;
    size_t cap;
    bool drop_stale;
};

// Everything the launches of one tracked frame of a single sequence depend on besides the swarm
// (launch_pso, refine_launch, subswarm_exchange): built by the tracking call for each frame it
// enqueues, so an enqueue function leaves nothing to set back, however often it runs.
struct FrameIo {
    const DevObs *obs;  // the descriptor the kernels read
    int n_max;          // a bound on its n (no readback of a device-prepared frame): it picks the
                        // kernel forms -- the staged refine, the FILT kernels
    double *state;      // 27 doubles: x0 in, {bestp, cost} out
    double *hist = nullptr;       // the frame's {bestp, cost} also stored there (sequences)
    DevObs *hand_back = nullptr;  // the final kernel copies *obs there (d_obs_active), or null
    // the sequence cursor: the final kernel stages the next frame's descriptor from slots into
    // seq_obs and advances cur {slot, history row}; a raw sequence has the row cursor alone
    const DevObs *slots = nullptr;
    DevObs *seq_obs = nullptr;
    int *cur = nullptr;
    // a pipelined frame: the final kernel bumps *seq and publishes it to the host word
    unsigned long long *seq = nullptr, *done_host = nullptr;
    // the exchange's pick is left to the next frame's refine launch (it follows in the chunk)
    bool defer_pick = false;
};

// The same for one frame of B lanes (track_lane_frame): lane b on descriptor obs[b] and cursor
// cur[2 b].
struct LaneFrameIo {
    DevObs *obs;           // the lanes' descriptors (of this buffer parity)
    bool filt;             // the FILT kernels (all lanes agree)
    double *hist;          // the history rows, or null
    const DevObs *slots;   // the table the final kernel stages lane b's next frame from; null:
                           // the preparation does that, and the cursor's slot word counts frames
    int *cur;              // the lanes' cursors, or null (the live batch keeps none)
    // the other parity's preparation table: the refine launch prepares every lane's next frame
    // (null: no next frame), from the lanes' raw bases read through cur (null: the pinned ring)
    const PrepArgs *prep = nullptr;
    const float *const *raw = nullptr;
    // the live batch: its final kernel bumps *seq and publishes it to the host word
    unsigned long long *seq = nullptr, *done_host = nullptr;
    // lane windows (hpe_set_batch_window): the window table of the parity `prep` prepares into
    // (null: no windows); follow: k_window_b rewrites it from the lanes' states first
    DevWindow *win = nullptr;
    bool follow = false;
    // lane pacing (hpe_set_batch_pacing, HPE_PACING_FREE): the lanes' activity words, which the
    // idle-aware kernel forms test at entry (null: lockstep, the plain forms)
    const int *act = nullptr;
    // lane input: the pinned ring holds 16-bit pixels, in this depth unit (device memory; null:
    // float frames)
    const float *unit = nullptr;
    // ... camera frames read through the lanes' views: unit then names the batch's ViewTab
    bool view = false;
    // lane cleaning: k_clean_b on this table of the parity `prep` prepares (null: off), ahead of
    // the refine launch; clean_view: the batch's ViewTab where the pinned buffers hold camera
    // frames (prep then names the staging frames, and view is false: the u16 forms read them)
    const CleanArgs *clean = nullptr;
    const CleanTab *clean_par = nullptr;
    const ViewTab *clean_view = nullptr;
};

}  // namespace

struct hpe_ctx {
    int device = 0;
    // The three streams stand before every other owner: members are destroyed in reverse order
    // of declaration, so all memory and every event goes first, then the pipeline's copy stream,
    // the preparation stream and, last as ever, the context stream.  Keep them first.
    Stream stream;
    Stream prep;       // device preprocessing (hpe_prepare_frame): one frame in flight at a time
    Stream pipe_copy;  // the pipeline's raw upload (Pipe::zero_copy off)
    char err[512] = {0};
    DevHand hand;
    DevBuf<DevHand> d_hand;
    // the batch lanes' hands (hpe_set_batch_hands): one flat table, entry b lane b's, which the
    // lane kernels' HANDS forms index by their lane; the context's hand in every entry while
    // lane_hands_B == 0, when the !HANDS forms run (they read entry 0).  The graphs hold its
    // address alone, and key whether hands are set (GraphKey::hands): rewriting the table (the
    // stream drained) captures nothing.
    DevBuf<DevHand> d_lane_hands;     // [HPE_BATCH_MAX]
    int lane_hands_B = 0;             // the B the lane hands were set for, 0: none
    // the batch lanes' seeds (hpe_set_batch_seeds): entry b lane b's, empty: the context's seed
    // for every lane.  The swarm holds the tables built from them (Swarm::lane_*).
    std::vector<uint64_t> lane_seeds;
    // the batch lanes' groups (hpe_set_batch_groups): the device table k_group_pick reads (the
    // graphs hold its address alone and key whether groups are set, GraphKey::groups), its host
    // copy, and the own-rows table [HPE_BATCH_MAX][27] -- every lane's own {bestp, cost} of the
    // last grouped frame it tracked (group_rows: one has been enqueued since the groups were set)
    DevBuf<LaneGroups> d_lane_groups;
    LaneGroups lane_groups{};
    int lane_groups_B = 0;            // the B the groups were set for, 0: none
    DevBuf<double> d_group_own;
    bool group_rows = false;
    std::vector<Slot> slots;
    int cur = -1;
    // scratch
    DevBuf<double> d_theta, d_cost, d_terms, d_S, d_J;
    int theta_cap = 0;
    DevBuf<int32_t> d_match;
    size_t match_cap = 0;
    DevBuf<double> d_state;  // 27 doubles: x0/bestp + cost
    // frame descriptors in HBM: one per slot + the selected one, which every kernel reads
    // (kernel arguments stay identical from frame to frame, so a frame replays as a graph)
    DevBuf<DevObs> d_obs, d_obs_active;
    // offline sequences: the descriptor the chunk graphs read and the cursor {slot, row}
    DevBuf<DevObs> d_seq_obs;
    DevBuf<int> d_seq_cur;
    // (no mode of the context says which descriptor, cursor or counter a tracked frame's launches
    // use: the tracking call hands them over in a FrameIo, for B lanes a LaneFrameIo, per frame)
    // the captured graphs, a cache per tracking call:
    // GC_FRAME: one tracked frame (refine + pso_evolve + cal_cost), replayed per frame
    // GC_PIPE: a pipelined frame, per buffer parity and whether it prepares a next frame
    // GC_SEQ, GC_RAW: a chunk of resident frames / of resident raw frames, keyed by its shape
    //     (not its slots)
    // GC_BATCH, GC_RAW_BATCH: the same chunks for B lanes
    // GC_LIVE_BATCH: a pipelined frame of B lanes, per buffer parity and whether it prepares
    //     next frames (GC_PIPE's cap)
    enum { GC_FRAME, GC_PIPE, GC_SEQ, GC_RAW, GC_BATCH, GC_RAW_BATCH, GC_LIVE_BATCH, GC_N };
    GraphCache graphs[GC_N] = {{{}, 1, false}, {{}, 16, false}, {{}, 64, true},
                               {{}, 64, true}, {{}, 64, true}, {{}, 64, true},
                               {{}, 16, false}};
    // device preprocessing (hpe_prepare_frame) on the stream prep
    DevBuf<float> d_raw;
    DevBuf<double> d_tmp, d_ctb;
    DevBuf<unsigned> d_prep_ctr;
    DevBuf<int> d_dtf;
    DevBuf<PrepInfo> d_info;  // [HPE_MAX_SLOTS]
    HostBuf<float> h_raw[HPE_RAW_RING];
    Event raw_ev[HPE_RAW_RING];
    bool raw_ev_valid[HPE_RAW_RING] = {};
    Event main_mark;
    int raw_k = 0;
    // pipelined tracking (hpe_pipeline_begin / hpe_track_pipelined): two frame buffers,
    // frame f+1 prepared inside frame f's refine launch
    struct Pipe {
        Slot fr[2];
        DevBuf<DevObs> d_obs;     // [2]
        DevBuf<PrepInfo> d_info;  // [2]
        DevBuf<float> d_raw;  // [2][npix]: raw frame by buffer parity
        // zero copy (default): the preparation workgroups read the raw frame straight from
        // its pinned (coherent, mapped) host buffer over PCIe, inside the refine launch they
        // ride in -- no upload, no cross-queue wait between frames.  HPE_PIPE_UPLOAD=1: the
        // raw upload of the next frame runs on a copy stream (SDMA) while the previous
        // frame computes, and the frame's graph waits on raw_ready.
        HostBuf<float> h_raw[2];
        bool zero_copy = true;
        // buffer reuse without event markers on the stream: every pipelined frame's final
        // kernel bumps d_seq and stores it to the pinned word h_done (system scope); the
        // host reuses pinned buffer k once h_done >= used_seq[k], the number of the frame
        // whose refine launch read it (zero copy)
        DevBuf<unsigned long long> d_seq;
        HostBuf<unsigned long long> h_done;
        // the split distance transform of resident raw sequences (PrepSplit): the forward
        // scans by frame parity, and {first hand row [2], sequence length, -}
        DevBuf<int> d_dtf2;   // [2][npix]
        DevBuf<int> d_split;  // [4]
        unsigned long long enq = 0, used_seq[2] = {0, 0};
        Event used[2], raw_ready[2];
        bool used_valid[2] = {false, false};
        int cur = -1, to_cm = 1, downsample = 1;
        double focal = 241.42;
    } pipe;
    // batched lanes (hpe_track_batch_dev): per lane the current-frame descriptor the chunk
    // graphs read, the cursor {slot, history row} and the refine evaluation counter
    DevBuf<DevObs> d_bobs;  // [HPE_BATCH_MAX]
    DevBuf<int> d_bcur;     // [HPE_BATCH_MAX][2]
    DevBuf<int> d_bevals;   // [HPE_BATCH_MAX][HPE_EVALS_N]
    // batched raw lanes (hpe_track_raw_batch_dev): per lane one arena holding two frame buffers
    // (depth, DT, a 250-point cloud each) and the preparation scratch (tmp, ctb, dtf); the
    // descriptors, PrepInfo and PrepArgs tables by [parity][lane]; the lane's hand-off counters
    // (a 128-byte line each), raw base and cursor {frame, history row}.  The chunk graphs hold
    // only the tables' addresses, which never change: arenas are added, never moved.
    struct RawBatch {
        DevBuf<char> arena[HPE_BATCH_MAX];
        int lanes = 0, to_cm = -1;
        double focal = 0;
        DevBuf<DevObs> d_obs;         // [2][HPE_BATCH_MAX]
        DevBuf<PrepInfo> d_info;      // [2][HPE_BATCH_MAX]
        DevBuf<PrepArgs> d_tab;       // [2][HPE_BATCH_MAX]
        DevBuf<unsigned> d_ctr;       // [HPE_BATCH_MAX][32]
        DevBuf<const float *> d_raw;  // [HPE_BATCH_MAX]
        DevBuf<int> d_cur;            // [HPE_BATCH_MAX][2]
        std::vector<PrepArgs> tab;    // d_tab's host copy, and how often it was rewritten
        unsigned tab_gen = 0;
    } rb;
    // a live batch (hpe_batch_pipeline_begin / hpe_track_batch_pipelined) on the raw batch's
    // lane arenas and descriptors: per lane two pinned mapped host buffers, a two-deep ring by
    // frame parity, which the preparation workgroups read in place (zero copy); d_tab is rb.d_tab
    // with each entry's raw frame naming its pinned buffer (rewritten when rb's is: tab_gen).
    // The hand-off is the single pipeline's: the final launch bumps d_seq and stores it to the
    // pinned word h_done, and the host refills the buffers of parity k once h_done >=
    // used_seq[k], the number of the frame whose refine launch read them.
    struct LiveBatch {
        HostBuf<float> h_raw[2][HPE_BATCH_MAX];
        int lanes = 0;  // lanes that have their pinned buffers
        DevBuf<PrepArgs> d_tab;  // [2][HPE_BATCH_MAX]
        unsigned tab_gen = 0;
        int tab_lanes = 0;
        DevBuf<unsigned long long> d_seq;
        HostBuf<unsigned long long> h_done;
        unsigned long long enq = 0, used_seq[2] = {0, 0};
        int B = 0, cur = -1, to_cm = 1;  // cur: the current frames' parity, -1: no batch
        double focal = 0;
        // lane pacing: the mode the batch began with; bit b of pending: lane b holds a prepared
        // frame the next call tracks (every lane under LOCKSTEP); the lanes' activity words in
        // device memory, written on the stream ahead of a frame's graph (k_lane_act)
        int pacing = HPE_PACING_LOCKSTEP;
        uint32_t pending = 0;
        DevBuf<int> d_act;  // [HPE_BATCH_MAX]
        // the words d_act holds once the stream reaches this point (act_known): a call whose
        // words are these enqueues no write -- a batch whose lanes all have every frame writes
        // them once
        int act_words[HPE_BATCH_MAX] = {};
        bool act_known = false;
        bool report = false;  // the batch began with lane reports on (it keeps that)
        // lane input: the batch's frames are 16-bit pixels (it keeps the format it began with)
        // in a depth unit (mm per count) that the begin writes to d_unit; a u16 frame fills the
        // first half of the lane's pinned buffer
        bool u16 = false;
        float unit_mm = 1.f;  // the host's copy of *d_unit (the locate kernel takes it by value)
        DevBuf<float> d_unit;
        // lane views (hpe_batch_pipeline_begin_view): a u16 batch whose lane b delivers camera
        // frames of views[b]; d_view holds the unit and the views (ViewTab), written at the begin,
        // and stands where d_unit stands for a plain u16 batch.  views_B: the lanes of the last
        // view begin (hpe_batch_views_readback), 0: none yet
        bool view = false;
        hpe_view views[HPE_BATCH_MAX] = {};
        int views_B = 0;
        DevBuf<ViewTab> d_view;
        // what every pinned buffer holds, in floats: one 240x320 float frame, or more once a view
        // batch needed it (grown for all lanes at once, never shrunk)
        size_t raw_floats = (size_t)HPE_IMG_H * HPE_IMG_W;
        size_t frame_bytes(int lane) const {
            if (view) return sizeof(uint16_t) * (size_t)views[lane].pitch * (size_t)views[lane].height;
            return (u16 ? sizeof(uint16_t) : sizeof(float)) * (size_t)HPE_IMG_H * HPE_IMG_W;
        }
        const float *unit_arg() const {  // the lane kernels' `unit` argument
            return view ? (const float *)d_view.get() : u16 ? d_unit.get() : nullptr;
        }
        // lane cleaning (hpe_set_batch_clean).  clean_B, clean_par: the setting the next u16 or
        // view begin reads (0: off).  clean: the batch in progress began with cleaning on (it
        // keeps that); cleaned_B: the lanes of the last cleaned begin (hpe_batch_clean_readback),
        // 0: none yet.  d_stage holds the cleaned 240x320 frames by [parity][lane], d_cargs
        // k_clean_b's table of {pinned buffer, staging frame}, d_cpar the lanes' parameters and
        // d_ctab the PrepArgs table whose raw frames are the staging frames: allocated together
        // by the first begin with cleaning on, never moved (the graphs hold their addresses).
        int clean_B = 0;
        hpe_clean clean_par[HPE_BATCH_MAX] = {};
        bool clean = false;
        int cleaned_B = 0;
        DevBuf<unsigned short> d_stage;  // [2][HPE_BATCH_MAX][240 * 320]
        DevBuf<CleanArgs> d_cargs;       // [2][HPE_BATCH_MAX]
        DevBuf<CleanTab> d_cpar;
        DevBuf<PrepArgs> d_ctab;         // [2][HPE_BATCH_MAX]
        unsigned short *stage(int parity, int lane) const {
            return d_stage.get() + ((size_t)parity * HPE_BATCH_MAX + lane) * HPE_IMG_H * HPE_IMG_W;
        }
        // what the preparation reads: a cleaned batch's staging frames in the u16 form -- also
        // for a view batch, whose ViewTab has the unit at offset 0 -- else the pinned ring
        const PrepArgs *prep_tab() const { return clean ? d_ctab.get() : d_tab.get(); }
        LaneSrc src() const {
            return clean ? LANE_SRC_U16 : view ? LANE_SRC_VIEW : u16 ? LANE_SRC_U16 : LANE_SRC_RING;
        }
    } live;
    // hpe_clean_depth_u16's own frames and tables (allocated by its first call; the source grows
    // to the largest camera frame given)
    struct CleanOne {
        DevBuf<unsigned short> d_src, d_dst;
        size_t src_pixels = 0;
        DevBuf<CleanArgs> d_args;
        DevBuf<CleanTab> d_par;
        DevBuf<ViewTab> d_view;
    } clean_one;
    // lane reports (hpe_set_batch_report): the setting the next begin reads (depth 0: off), and
    // what the rings hold -- the depth and lane count of the last batch begun with reports on
    // (ring_depth 0: nothing to read), per lane the reports enqueued since that begin.  The ring
    // (pinned, mapped, coherent, like h_done), the lanes' device words and the parameters are
    // allocated once, at full size, by the first set that turns reports on: their addresses, all
    // the graphs hold, never change, and the depth is read from d_par.
    struct Report {
        int depth = 0;
        hpe_report_watch watch = {HUGE_VAL, 0, 0};
        int ring_depth = 0, ring_B = 0;
        unsigned long long enq[HPE_BATCH_MAX] = {};
        HostBuf<char> h_ring;
        DevBuf<unsigned long long> d_lane_seq;  // [HPE_BATCH_MAX]
        DevBuf<int> d_streak;                   // [HPE_BATCH_MAX]
        DevBuf<RepPar> d_par;
    } rep;
    // lane location (hpe_locate_depth, hpe_batch_pipeline_locate): allocated by the first begin
    // with the windows on, or by the first hpe_locate_depth.
    // Entries [0, HPE_BATCH_MAX) of d_res and d_act are the live batch's lanes, entry
    // HPE_BATCH_MAX is hpe_locate_depth's own.  d_act is the locate-owned activity table: the
    // locate kernel fills it, the preparation and the placement that follow are gated by it.
    // h_tab: a slot per lane in pinned, mapped, coherent host memory (LOC_SLOT bytes: begin
    // word, hpe_locate, end word), d_seq the lanes' locate counters; B, enq: the lane count of
    // the last live batch begun and the locates enqueued per lane since that begin.
    struct Locate {
        DevBuf<hpe_locate> d_res;          // [HPE_BATCH_MAX + 1]
        DevBuf<int> d_act;                 // [HPE_BATCH_MAX + 1]
        DevBuf<unsigned long long> d_seq;  // [HPE_BATCH_MAX]
        HostBuf<char> h_tab;
        DevBuf<float> d_frame;             // hpe_locate_depth's staging buffer, one frame
        int B = 0;
        unsigned long long enq[HPE_BATCH_MAX] = {};
    } loc;
    // lane windows (hpe_set_batch_window): the mode, and what the next raw batch call or live
    // begin writes to the device -- init into both parities of the window table d_tab (next to
    // rb.d_tab, allocated with it), the margins and the call's focal into d_par -- after the
    // stream has drained.  Device memory, not the graphs, holds them: the graphs key the mode.
    struct LaneWin {
        int mode = HPE_WINDOW_OFF, B = 0;
        double margin_xy = 0, margin_z = 0;
        std::vector<DevWindow> init;
        DevBuf<DevWindow> d_tab;  // [2][HPE_BATCH_MAX]
        DevBuf<WinPar> d_par;
        // hpe_window_from_pose's own pose, parameters and result
        DevBuf<double> d_one_state;
        DevBuf<WinPar> d_one_par;
        DevBuf<DevWindow> d_one;
    } win;
    Event seq_done;  // recorded after a sequence: its slots' last reader
    bool seq_done_valid = false;
    unsigned epoch = 1;  // bumped whenever a buffer a captured graph uses is reallocated
    int batch_form = HPE_BATCH_FORM_AUTO;  // the batch calls' pso_evolve form (hpe_set_batch_form)
    int batch_pacing = HPE_PACING_LOCKSTEP;  // the next live batch's pacing (hpe_set_batch_pacing)
    int pso_form = 0;    // 0 auto, 1 workgroup per particle, 2 wave per particle
    static constexpr int wave_form_min_p = 1024;
    int pso_wpp = 0;      // waves per particle of the wave form (0: auto)
    static constexpr int wpp2_max_p = 1024;
    bool fk_coop = true;  // the wave form's FK by the whole workgroup (HPE_FK_COOP)
    bool use_graph = true;
    // resident raw sequences split each frame's distance transform over two refine launches
    // (HPE_PREP_SPLIT=0: the whole transform in one, as the pipelined loop has it)
    bool prep_split = true;
    HostBuf<double> h_pinned;  // 256 doubles: [0,64) results, [64,128) inputs
    DevBuf<int> d_evals;
    // multi-workgroup refine (clouds > RF_STAGE_MAX); HPE_REFINE_MW=0 keeps one workgroup
    DevBuf<MwJob> d_mw_job;
    DevBuf<double> d_mw_part;
    DevBuf<unsigned> d_mw_ctr;
    DevBuf<int> d_mw_err;
    HostBuf<int> h_mw_err;  // pinned copy of the flag (mapped)
    int mw_spin = MW_SPIN_MAX;  // HPE_MW_SPIN: polls per wait (a test forces timeouts with 0)
    int mw_fits = -1;  // the multi-workgroup launch fits co-resident (occupancy), -1 unknown
    bool refine_mw = true;
    bool refine_exact = false;  // refine spheres by the reference's chain (else hand frame)
    // speculated translation block (hpe_set_refine_spec): the staged refine's second workgroup
    bool refine_spec = true;
    DevBuf<unsigned long long> d_spec_g;  // DevSpec::g
    DevBuf<unsigned> d_spec_ep;           // DevSpec::epoch
    int spec_spin = SPEC_SPIN_MAX;  // HPE_SPEC_SPIN: the leader's polls for a result (tests: 0)
    int spec_fits = -1;  // both refine workgroups and the preparation fit co-resident, -1 unknown
    unsigned long long captures = 0;  // graphs captured so far (hpe_graph_captures)
    // opt-in per-generation exchange (hpe_set_exchange)
    int xch_every = 0;
    double *xch_ext = nullptr;
    hpe_exchange_fn xch_fn = nullptr;
    void *xch_user = nullptr;
    // multi-GPU subswarms with the per-frame exchange inside the library (hpe_subswarm_init):
    // after every tracked frame, an RCCL all-gather of {bestp, cost} and the pick, on the
    // context stream -- captured into the tracking graphs with the frames
    struct Subswarm {
        ncclComm_t comm = nullptr;
        // the scripted transport (hpe_subswarm_init_scripted) in the communicator's place:
        // peer rows [script_frames][nranks][27] and the device exchange counter
        DevBuf<double> d_script;
        DevBuf<int> d_script_k;
        int script_frames = 0;
        bool transport() const { return comm || d_script; }
        int nranks = 0, rank = 0;
        bool on = false;
        DevBuf<double> d_gath;  // [nranks][27]: row `rank` is this rank's frame result
        // the exchange inside captured graphs (1), or direct launches while it is on (0): set
        // by hpe_subswarm_enable(ctx, 2), or when a capture holding the collective fails
        bool graphs = true;
        char note[256] = {0};
    } ss;
    DevBuf<float> d_render;
    // PSO parameters
    double lb[26], ub[26], sd[26];
    double omega = 0.7298, phip = 1.49618, phig = 1.49618, minstep = 1e-6, minfunc = 1e-6;
    int maxiter = 100;
    bool params = false;
    bool bounds_dirty = true;
    uint64_t seed = 1000;
    Swarm sw;
    OptState opt;
    OptLanes optl;
    // kernel timing: hipExtLaunchKernel start/stop events (dispatch-packet timestamps,
    // the same interval rocprofv3 --kernel-trace reports), one pool per kernel
    bool prof = false;
    struct Pool {
        std::vector<Event> ev;  // pairs
        size_t used = 0;
    } pools[HPE_PROF_KERNELS];
};

// Launch on the context stream; while profiling, bracket the dispatch with events.
template <typename F, typename... A>
static void launch(hpe_ctx *c, int which, F kernel, dim3 grid, dim3 block, unsigned lds, A... args) {
    hpe_ctx::Pool &pl = c->pools[which];
    if (c->prof && pl.used + 2 <= pl.ev.size()) {
        hipExtLaunchKernelGGL(kernel, grid, block, lds, c->stream, pl.ev[pl.used], pl.ev[pl.used + 1],
                              0, args...);
        pl.used += 2;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, args...);
    }
}

static int fail(hpe_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(c, expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail((c), HPE_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                              \
    } while (0)

static DevObs make_obs(const Slot &s) {
    DevObs o;
    o.cx = s.cx;
    o.cy = s.cy;
    o.cz = s.cz;
    o.depth = s.depth;
    o.dt = s.dt;
    o.n = s.n;
    o.lambda = (double)HPE_NS / (double)s.n;  // costfunc.cpp:372
    o.scale = s.scale;
    o.dtmax = s.dtmax;
    for (int k = 0; k < 9; ++k) o.K[k] = s.K[k];
    return o;
}

// Host copy of a device-prepared frame's scalars (synchronises with its preparation).
static int slot_known(hpe_ctx *c, Slot &s, int slot) {
    if (s.known) return HPE_OK;
    PrepInfo pi;
    HIPCHK(c, hipEventSynchronize(s.ready));
    HIPCHK(c, hipMemcpy(&pi, c->d_info + slot, sizeof(pi), hipMemcpyDeviceToHost));
    s.n = pi.n;
    s.scale = pi.scale;
    s.dtmax = pi.dtmax;
    s.known = true;
    return HPE_OK;
}

static int need_frame(hpe_ctx *c, DevObs *o) {
    if (c->cur < 0 || c->cur >= (int)c->slots.size() || !c->slots[c->cur].valid)
        return fail(c, HPE_E_STATE, "no frame selected (hpe_set_frame / hpe_select_frame)");
    int rc = slot_known(c, c->slots[c->cur], c->cur);
    if (rc) return rc;
    *o = make_obs(c->slots[c->cur]);
    return HPE_OK;
}

static int ensure_theta(hpe_ctx *c, int P) {
    if (P <= c->theta_cap) return HPE_OK;
    ++c->epoch;
    c->theta_cap = 0;
    HIPCHK(c, alloc_all(c->d_theta, (size_t)P * HPE_DOF, c->d_cost, (size_t)P, c->d_terms, (size_t)P * 3,
                        c->d_S, (size_t)P * 3 * HPE_NS, c->d_J, (size_t)P * 63));
    c->theta_cap = P;
    return HPE_OK;
}

static int ensure_match(hpe_ctx *c, size_t n) {
    if (n <= c->match_cap) return HPE_OK;
    ++c->epoch;
    c->match_cap = 0;
    HIPCHK(c, c->d_match.alloc(n));
    c->match_cap = n;
    return HPE_OK;
}

// A frame buffer's depth and DT images once, and its cloud grown to `need` points: each group
// all or nothing, and a slot whose cloud could not be grown is invalid, with capacity 0.
static hipError_t slot_buffers(Slot &s, int need) {
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W, n = (size_t)need;
    hipError_t e = s.depth ? hipSuccess : alloc_all(s.depth, npix, s.dt, npix);
    if (e != hipSuccess || need <= s.cap) return e;
    s.cap = 0;
    s.valid = false;
    if ((e = alloc_all(s.cx, n, s.cy, n, s.cz, n)) == hipSuccess) s.cap = need;
    return e;
}

// The lane arenas of a batch call (Swarm::arena): grown, never shrunk, with the epoch bumped
// so that batch graphs holding the old arenas are dropped.
static int ensure_lanes(hpe_ctx *c, int lanes) {
    Swarm &s = c->sw;
    if (lanes <= s.lanes) return HPE_OK;
    ++c->epoch;
    s.arena.reset();
    s.lanes = 0;
    const size_t n = (size_t)s.P * HPE_DOF, G1 = (size_t)s.G + 1;
    const size_t bytes[9] = {sizeof(double) * G1 * n,                                      // xh
                             sizeof(double) * G1 * s.P,                                    // pch
                             sizeof(double) * n,                                           // pb
                             sizeof(double) * n,                                           // v
                             sizeof(double) * 4 * s.P * s.laneK * IB_STRIDE,               // inbox
                             sizeof(unsigned long long) * G1 * GMIN_SHARDS * GMIN_STRIDE,  // gmin
                             sizeof(Sig) * G1,                                             // sig
                             sizeof(double) * HPE_DOF,                                     // gpos
                             sizeof(double) * 8 * s.P * s.laneK};                          // ibtc
    size_t at = 0;
    for (int k = 0; k < 9; ++k) {  // every array on a 256-byte boundary, as hipMalloc gives
        s.off[k] = at;
        at += (bytes[k] + 255) & ~(size_t)255;
    }
    s.stride = at;
    HIPCHK(c, s.arena.alloc(s.stride * lanes));
    // empty inbox and ibtc slots (tag -1) and unwritten gmin cells are all-ones; the rest is
    // written before it is read
    HIPCHK(c, hipMemset(s.arena, 0xFF, s.stride * lanes));
    s.lanes = lanes;
    return HPE_OK;
}

// The inbox counts of one seed's topologies (InboxCounts, P <= KIN_MAX): kin[g] for g = 0..G from
// make_links' in-degrees.
static void inbox_counts(int P, int G, const std::vector<int> &indeg, InboxCounts *kin) {
    std::vector<int> kept(P, 0);  // max in-degree over topologies 1..g-1
    for (int g = 1; g <= G; ++g) {
        for (int r = 0; r < P; ++r) {
            kin[g].k0[r] = (uint8_t)kept[r];
            kin[g].k1[r] = (uint8_t)indeg[(size_t)g * P + r];
        }
        for (int r = 0; r < P; ++r) kept[r] = std::max(kept[r], indeg[(size_t)g * P + r]);
    }
}

// The lanes' own draw tables (hpe_set_batch_seeds) of the swarm as it stands, for c->lane_seeds,
// and the arenas' K.  make_links and make_normals run once per distinct seed.  A seed set whose
// largest K exceeds IB_KMAX is refused before anything changes.  The tables are grown, never
// shrunk (the epoch bumped: the graphs hold their addresses), and rewritten in place once the
// stream has drained when only the seeds change -- the graphs of that shape replay on the new
// tables and nothing is captured.  Whenever the seeds the arenas were last used under change
// (lane seeds set, changed or cleared), the arenas are emptied again: an inbox slot a new
// topology never fills could still hold the old one's push of the same generation, whose tag
// matches (the wave form and swarms above KIN_MAX read all K slots by tag).  A changed K drops
// the arenas instead: ensure_lanes builds them at the new size.
static int ensure_lane_seeds(hpe_ctx *c) {
    Swarm &s = c->sw;
    const std::vector<uint64_t> &want = c->lane_seeds;
    const int B = (int)want.size(), P = s.P, G = s.G;
    if (want == s.arena_seeds && (B || s.laneK == s.K)) return HPE_OK;
    int K = s.K;
    if (B && want != s.tab_seeds) {
        const size_t n = (size_t)P * HPE_DOF, G1 = (size_t)G + 1, no = G1 * P * 6;
        std::vector<double> nrm(n * B);
        std::vector<int> outl(no * B), lk(B, 0);
        std::vector<InboxCounts> kin(G1 * B, InboxCounts{});
        LaneSeeds ls{};
        for (int b = 0; b < B; ++b) {
            ls.seed[b] = want[b];
            int same = 0;
            while (want[same] != want[b]) ++same;
            if (same < b) {  // an earlier lane's seed: its tables again
                std::copy_n(nrm.begin() + n * same, n, nrm.begin() + n * b);
                std::copy_n(outl.begin() + no * same, no, outl.begin() + no * b);
                std::copy_n(kin.begin() + G1 * same, G1, kin.begin() + G1 * b);
                lk[b] = lk[same];
                continue;
            }
            std::vector<int> o, indeg;
            lk[b] = hpe::make_links(want[b], P, G, o, &indeg);
            if (lk[b] > IB_KMAX)
                return fail(c, HPE_E_ARG, "lane %d: informant in-degree %d > %d", b, lk[b], IB_KMAX);
            std::copy(o.begin(), o.end(), outl.begin() + no * b);
            if (P <= KIN_MAX) inbox_counts(P, G, indeg, kin.data() + G1 * b);
            hpe::make_normals(want[b], P, nrm.data() + n * b);
        }
        K = *std::max_element(lk.begin(), lk.end());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight read the tables
        if (B > s.tab_lanes) {
            ++c->epoch;
            s.tab_lanes = 0;
            s.tab_seeds.clear();
            HIPCHK(c, s.lane_normals.alloc(n * B));
            HIPCHK(c, s.lane_outl.alloc(no * B));
            HIPCHK(c, s.lane_kin.alloc(G1 * B));
            if (!s.lane_ls) HIPCHK(c, s.lane_ls.alloc(1));
            s.tab_lanes = B;
        }
        s.tab_seeds.clear();  // (a copy that fails part way leaves tables of no seed set)
        ls.kin = s.lane_kin;
        HIPCHK(c, hipMemcpy(s.lane_normals, nrm.data(), sizeof(double) * nrm.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(s.lane_outl, outl.data(), sizeof(int) * outl.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(s.lane_kin, kin.data(), sizeof(InboxCounts) * kin.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(s.lane_ls, &ls, sizeof(ls), hipMemcpyHostToDevice));
        s.tab_seeds = want;
        s.tab_K = K;
    } else if (B) {
        K = s.tab_K;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K != s.laneK) {  // other inboxes: ensure_lanes builds the arenas again
        s.laneK = K;
        s.arena.reset();
        s.lanes = 0;
    } else if (s.lanes) {
        HIPCHK(c, hipMemset(s.arena, 0xFF, s.stride * s.lanes));
    }
    s.arena_seeds = want;
    return HPE_OK;
}

// Swarm buffers + draw tables for (P, G, seed); rebuilt only when one changes.  lanes > 0
// (hpe_track_batch_dev): also that many lane arenas, and the lanes' own draw tables when lane
// seeds are set.
static int ensure_swarm(hpe_ctx *c, int P, int G, int lanes = 0) {
    if (c->sw.P == P && c->sw.G == G && c->sw.seed == c->seed) {
        if (lanes)
            if (int rc = ensure_lane_seeds(c)) return rc;
        return ensure_lanes(c, lanes);
    }
    ++c->epoch;
    c->sw = Swarm{};
    Swarm s;  // built here and moved in whole: a failure leaves the context's swarm empty
    if (G > 32767) return fail(c, HPE_E_ARG, "maxiter %d too large", G + 1);
    std::vector<int> outl, indeg;
    const int K = hpe::make_links(c->seed, P, G, outl, &indeg);
    if (K > IB_KMAX) return fail(c, HPE_E_ARG, "informant in-degree %d > %d", K, IB_KMAX);
    s.kin.clear();
    if (P <= KIN_MAX) {  // valid inbox slots per receiver and generation (InboxCounts)
        s.kin.assign((size_t)G + 1, InboxCounts{});
        inbox_counts(P, G, indeg, s.kin.data());
    }
    const size_t n = (size_t)P * HPE_DOF;
    HIPCHK(c, s.xh.alloc((size_t)(G + 1) * n));
    HIPCHK(c, s.pch.alloc((size_t)(G + 1) * P));
    HIPCHK(c, s.pb.alloc(n));
    const size_t ibn = (size_t)4 * P * K * IB_STRIDE;
    HIPCHK(c, s.inbox.alloc(ibn));
    HIPCHK(c, hipMemset(s.inbox, 0xFF, sizeof(double) * ibn));  // tag -1: empty slot
    HIPCHK(c, s.ibtc.alloc((size_t)8 * P * K));
    HIPCHK(c, hipMemset(s.ibtc, 0xFF, sizeof(double) * 8 * P * K));
    HIPCHK(c, s.v.alloc(n));
    HIPCHK(c, s.gpos.alloc((size_t)HPE_DOF));
    HIPCHK(c, s.normals.alloc(n));
    HIPCHK(c, s.bounds.alloc((size_t)4 * HPE_DOF));
    const size_t ng = (size_t)(G + 1) * GMIN_SHARDS * GMIN_STRIDE;
    HIPCHK(c, s.gmin.alloc(ng));
    HIPCHK(c, hipMemset(s.gmin, 0xFF, sizeof(unsigned long long) * ng));
    HIPCHK(c, s.trace_g.alloc((size_t)(G > 0 ? G : 1)));
    HIPCHK(c, s.trace_count.alloc((size_t)(G > 0 ? G : 1)));
    HIPCHK(c, s.trace_topo.alloc((size_t)(G > 0 ? G : 1)));
    HIPCHK(c, s.sig.alloc((size_t)G + 1));
    std::vector<double> nrm(n);
    hpe::make_normals(c->seed, P, nrm.data());
    HIPCHK(c, hipMemcpy(s.normals, nrm.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(c, s.outl.alloc(outl.size()));
    HIPCHK(c, hipMemcpy(s.outl, outl.data(), sizeof(int) * outl.size(), hipMemcpyHostToDevice));
    s.P = P;
    s.G = G;
    s.K = s.laneK = K;
    s.seed = c->seed;
    c->sw = std::move(s);
    c->bounds_dirty = true;
    if (lanes)
        if (int rc = ensure_lane_seeds(c)) return rc;
    return ensure_lanes(c, lanes);
}

static DevSwarm dev_swarm(hpe_ctx *c) {
    Swarm &s = c->sw;
    DevSwarm d;
    d.xh = s.xh;
    d.pch = s.pch;
    d.pb = s.pb;
    d.inbox = s.inbox;
    d.ibtc = s.ibtc;
    d.v = s.v;
    d.gmin = s.gmin;
    d.sig = s.sig;
    d.normals = s.normals;
    d.outl = s.outl;
    d.bounds = s.bounds;
    d.gpos = s.gpos;
    d.trace_g = s.trace_g;
    d.trace_count = s.trace_count;
    d.trace_topo = s.trace_topo;
    d.ext = c->xch_every > 0 ? c->xch_ext : nullptr;
    d.seed = s.seed;
    d.P = s.P;
    d.G = s.G;
    d.K = s.K;
    return d;
}

// Lane 0 of the batch arenas (the kernels add blockIdx.y * stride); the tables every lane
// shares come from the swarm -- with lane seeds set, lane 0's of the lanes' own tables (the SEEDS
// kernels add their lane's offset, and read d.seed from the LaneSeeds entry).  K is the arenas'.
// No trace (hpe_pso_trace is not updated), no exchange.
static DevSwarm batch_swarm(hpe_ctx *c) {
    Swarm &s = c->sw;
    DevSwarm d = dev_swarm(c);
    d.K = s.laneK;
    if (!c->lane_seeds.empty()) {
        d.normals = s.lane_normals;
        d.outl = s.lane_outl;
    }
    d.xh = (double *)(s.arena + s.off[0]);
    d.pch = (double *)(s.arena + s.off[1]);
    d.pb = (double *)(s.arena + s.off[2]);
    d.v = (double *)(s.arena + s.off[3]);
    d.inbox = (double *)(s.arena + s.off[4]);
    d.gmin = (unsigned long long *)(s.arena + s.off[5]);
    d.sig = (Sig *)(s.arena + s.off[6]);
    d.gpos = (double *)(s.arena + s.off[7]);
    d.ibtc = (double *)(s.arena + s.off[8]);
    d.trace_g = nullptr;
    d.trace_count = d.trace_topo = nullptr;
    d.ext = nullptr;
    return d;
}

// Kernel form of a PSO generation: one workgroup per particle while the swarm is about
// the CU count or smaller (latency-bound), one wave per particle beyond (throughput).
// HPE_PSO_FORM=block|wave overrides (tests exercise both).
static bool pso_wave_form(hpe_ctx *c, int P) {
    if (c->pso_form == 1) return false;
    if (c->pso_form == 2) return true;
    return P >= c->wave_form_min_p;
}
// The wave form's generation kernel for (waves per particle, cooperative FK, exchange,
// K <= 15).
typedef void (*WaveGenFn)(DevSwarm, const DevObs *, const DevHand *, int, double, double, double);
template <int WPP, bool COOP>
static WaveGenFn wave_gen_kernel_t(bool x, bool r16) {
    return x ? (r16 ? k_pso_gen_w<true, true, WPP, COOP> : k_pso_gen_w<true, false, WPP, COOP>)
             : (r16 ? k_pso_gen_w<false, true, WPP, COOP> : k_pso_gen_w<false, false, WPP, COOP>);
}
static WaveGenFn wave_gen_kernel(int wpp, bool coop, bool x, bool r16) {
    if (wpp == 2) return coop ? wave_gen_kernel_t<2, true>(x, r16) : wave_gen_kernel_t<2, false>(x, r16);
    return coop ? wave_gen_kernel_t<1, true>(x, r16) : wave_gen_kernel_t<1, false>(x, r16);
}
// (its lane form's: lane_wave_gen_kernel, with the lane frame)

// Waves per particle of the wave form: two while the swarm leaves SIMDs idle at one (the
// search's latency halves), one beyond (the duplicated FK would cost throughput).
// HPE_PSO_WPP=1|2 overrides (tests).
static int pso_wpp(hpe_ctx *c, int P) {
    if (c->pso_wpp) return c->pso_wpp;
    return P <= c->wpp2_max_p ? 2 : 1;
}
// ... of a wave-form batch (hpe_set_batch_form): the rule on the launch's B * P particles, and
// zero for a batch in the workgroup form (the batch graphs' key field).
static int batch_wave_wpp(hpe_ctx *c, int P, int B) {
    return c->batch_form == HPE_BATCH_FORM_WAVE ? pso_wpp(c, B * P) : 0;
}

// PSO bounds / std to HBM when they changed (synchronous: never inside a graph capture).
static int upload_bounds(hpe_ctx *c) {
    if (!c->bounds_dirty) return HPE_OK;
    double b[4 * HPE_DOF];
    std::memcpy(b, c->lb, sizeof(c->lb));
    std::memcpy(b + HPE_DOF, c->ub, sizeof(c->ub));
    std::memcpy(b + 2 * HPE_DOF, c->sd, sizeof(c->sd));
    std::memset(b + 3 * HPE_DOF, 0, sizeof(double) * HPE_DOF);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->sw.bounds, b, sizeof(b), hipMemcpyHostToDevice));
    c->bounds_dirty = false;
    return HPE_OK;
}

// The lanes' descriptors, cursors and refine evaluation counters (every batch call counts in
// d_bevals).
static int ensure_batch_lanes(hpe_ctx *c) {
    if (!c->d_bevals) {  // assigned last, zeroed: a block that failed part way runs again in full
        HIPCHK(c, alloc_all(c->d_bobs, HPE_BATCH_MAX, c->d_bcur, 2 * HPE_BATCH_MAX));
        DevBuf<int> evals;
        HIPCHK(c, evals.alloc(HPE_BATCH_MAX * HPE_EVALS_N));
        HIPCHK(c, hipMemset(evals, 0, sizeof(int) * HPE_BATCH_MAX * HPE_EVALS_N));
        c->d_bevals = std::move(evals);
    }
    return HPE_OK;
}

static int generations(const hpe_ctx *c) {  // PSO.cpp:778 runs maxiter-1 times
    return c->maxiter - 1 > 0 ? c->maxiter - 1 : 0;
}

// What every tracking call allocates before any capture, for swarms of P particles and `lanes`
// lanes (0: a single sequence): the refine's match buffer or the lanes' tables, the swarm, the
// bounds.  Returns G >= 0, or the error code (< 0).
static int ensure_tracking(hpe_ctx *c, int P, int lanes) {
    const int G = generations(c);
    int rc = lanes ? ensure_batch_lanes(c) : ensure_match(c, (size_t)HPE_IMG_H * HPE_IMG_W);
    if (!rc) rc = ensure_swarm(c, P, G, lanes);
    if (!rc) rc = upload_bounds(c);
    return rc ? rc : G;
}

// The per-generation exchange (hpe_set_exchange) after generation g of G: this swarm's
// best into the caller's buffer, then the caller's collective on the context stream.
static int exchange_after(hpe_ctx *c, const DevSwarm &d, int g, int G) {
    if (c->xch_every <= 0 || g % c->xch_every != 0 || g >= G) return HPE_OK;
    launch(c, HPE_PROF_SWARM_BEST, k_swarm_best, dim3(1), dim3(HPE_NT), 0, d, g);
    HIPCHK(c, hipGetLastError());
    const int r = c->xch_fn(c->xch_user, c->xch_ext, g);
    if (r) return fail(c, HPE_E_STATE, "exchange callback failed (%d) after generation %d", r, g);
    return HPE_OK;
}

// The library's subswarm exchange after a tracked frame's final kernel (SURVEY.md §8e,
// PSO.cpp:848-861 sharded).  The final kernel has written this rank's {bestp, cost} into
// row `rank` of the gather buffer (subswarm_out); the all-gather is in place (no local copy:
// at one rank RCCL has nothing to move), then d_state <- the best row (k_pick_best; ties to
// the lowest rank), on the context stream.  In a sequence, the frame's history row (row
// io.cur[1] - 1) gets the picked state too.  io.defer_pick (a refine launch follows in the same
// chunk): the pick is handed to the caller instead (*pick) and rides in that launch, one launch
// fewer per frame; the chunk loop carries it from this frame to the next as a local.  While
// profiling, an event pair brackets the exchange (HPE_PROF_EXCHANGE).
// With the scripted transport a one-wave kernel stands where the all-gather does: it copies
// the peers' rows of the script frame the device exchange counter names (k_script_rows).
static bool subswarm_active(const hpe_ctx *c) { return c->ss.transport() && c->ss.on; }
static double *subswarm_out(hpe_ctx *c, double *d_state) {
    return subswarm_active(c) ? c->ss.d_gath + (size_t)c->ss.rank * (HPE_DOF + 1) : d_state;
}
static int subswarm_exchange(hpe_ctx *c, const FrameIo &io, DevPick *pick) {
    if (!subswarm_active(c)) return HPE_OK;
    const int *cur = io.cur ? io.cur + 1 : nullptr;  // the history row cursor
    hpe_ctx::Pool &pl = c->pools[HPE_PROF_EXCHANGE];
    const bool timed = c->prof && pl.used + 2 <= pl.ev.size();
    if (timed) HIPCHK(c, hipEventRecord(pl.ev[pl.used], c->stream));
    if (c->ss.comm) {
        const RcclApi &api = rccl_api();
        double *row = c->ss.d_gath + (size_t)c->ss.rank * (HPE_DOF + 1);
        const ncclResult_t r = api.all_gather(row, c->ss.d_gath, HPE_DOF + 1, ncclFloat64,
                                              c->ss.comm, c->stream);
        if (r != ncclSuccess)
            return fail(c, HPE_E_HIP, "subswarm all-gather: %s", api.error_string(r));
    } else {
        hipLaunchKernelGGL(k_script_rows, dim3(1), dim3(64), 0, c->stream,
                           (const double *)c->ss.d_script, c->ss.script_frames, c->ss.nranks,
                           c->ss.rank, c->ss.d_script_k, c->ss.d_gath);
        HIPCHK(c, hipGetLastError());
    }
    if (io.defer_pick) {
        *pick = DevPick{c->ss.d_gath, io.hist, cur, c->ss.nranks};
    } else {
        hipLaunchKernelGGL(k_pick_best, dim3(1), dim3(64), 0, c->stream, (const double *)c->ss.d_gath,
                           c->ss.nranks, io.state, io.hist, cur);
        HIPCHK(c, hipGetLastError());
    }
    if (timed) {
        HIPCHK(c, hipEventRecord(pl.ev[pl.used + 1], c->stream));
        pl.used += 2;
    }
    return HPE_OK;
}

// Tracking calls launch directly instead of capturing / replaying graphs: while profiling,
// with HPE_NO_GRAPH=1, with the per-generation exchange (a host callback between
// generations), and with the subswarm exchange when it runs outside graphs.
static bool direct_launches(const hpe_ctx *c) {
    return c->prof || !c->use_graph || c->xch_every > 0 || (subswarm_active(c) && !c->ss.graphs);
}

// End a capture begun on the context stream: instantiate it into *exec.  If the capture or
// its instantiation failed while the subswarm exchange is on (RCCL refusing the collective in
// a capture), the exchange falls back to direct launches for this and every later call --
// noted once on stderr and in hpe_subswarm_info -- and *direct tells the caller to enqueue
// the same work directly; every rank takes the same path, so the collectives stay matched.
static int end_capture(hpe_ctx *c, int rc, hipGraphExec_t *exec, bool *direct) {
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    hipError_t ei = hipSuccess;
    if (!rc && e == hipSuccess) ei = hipGraphInstantiateWithFlags(exec, g, 0);
    if (g) (void)hipGraphDestroy(g);
    *direct = false;
    if (!rc && e == hipSuccess && ei == hipSuccess) return HPE_OK;
    if (subswarm_active(c)) {
        snprintf(c->ss.note, sizeof(c->ss.note), "the subswarm exchange could not be captured "
                 "(%s); tracking calls launch directly", rc ? c->err : hipGetErrorString(e != hipSuccess ? e : ei));
        std::fprintf(stderr, "hpe: %s\n", c->ss.note);
        (void)hipGetLastError();
        c->ss.graphs = false;
        *exec = nullptr;
        *direct = true;
        return HPE_OK;
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, HPE_E_HIP, "graph capture: %s", hipGetErrorString(e));
    return fail(c, HPE_E_HIP, "graph instantiate: %s", hipGetErrorString(ei));
}

// Run the launches enqueue() makes on the context stream: directly (direct_launches, or the
// capture's exchange fallback), or as gc's graph of this key, seed and epoch -- replayed, or
// captured now and kept.  Before the new graph is kept, the cache's stale graphs go (drop_stale)
// and, at its cap, all of them.
template <class Enq>
static int run_graphed(hpe_ctx *c, GraphCache &gc, const GraphKey &key, Enq enqueue) {
    if (direct_launches(c)) return enqueue();
    std::vector<GraphCache::Entry> &es = gc.entries;
    hipGraphExec_t exec = nullptr;
    for (const auto &e : es)
        if (e.key == key && e.seed == c->seed && e.epoch == c->epoch) exec = e.exec;
    if (!exec) {
        HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        ++c->captures;
        bool direct = false;
        if (int rc = end_capture(c, enqueue(), &exec, &direct)) return rc;
        if (direct) return enqueue();
        const auto stale = [&](const GraphCache::Entry &e) {
            return gc.drop_stale && (e.epoch != c->epoch || e.seed != c->seed);
        };
        size_t live = 0;
        for (const auto &e : es) live += !stale(e);
        const bool full = live >= gc.cap;
        // A graph about to be destroyed may still be in flight: not every epoch bump comes
        // from a reallocation that drained the device (hpe_set_refine_exact and
        // hpe_set_exchange only bump it).  Wait for the stream first, once, and only when
        // there is something to destroy.
        if (full || live < es.size()) HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t q = 0; q < es.size();) {
            if (full || stale(es[q])) {
                (void)hipGraphExecDestroy(es[q].exec);
                es[q] = es.back();
                es.pop_back();
            } else {
                ++q;
            }
        }
        es.push_back({key, c->seed, c->epoch, exec});
    }
    HIPCHK(c, hipGraphLaunch(exec, c->stream));
    return HPE_OK;
}

// pso_evolve on the device: x0 and the result live in d_state (27 doubles).
// The swarm of P particles is the caller's to have built (ensure_swarm, upload_bounds).
// tail: fuse cal_cost(bestp) and the rest of io (the hand-back, the cursor, the frame counter,
// the history row) into the final kernel, then the subswarm exchange (*pick: see there).
static int launch_pso(hpe_ctx *c, int P, const FrameIo &io, bool tail, DevPick *pick = nullptr) {
    int rc;
    double *d_state = io.state;
    DevSwarm d = dev_swarm(c);
    const int G = d.G;
    const double W1 = 1. / (2 * std::log(2.0)), C1 = 0.5 + std::log(2.0), C2 = C1;  // :772-774
    // clouds of more than HPE_NT / 2 points (a bound): the workgroup form's cal_cost by the
    // filter search (eval_block FILT), the same choice for every kernel of the frame
    const bool filt = io.n_max > HPE_NT / 2;
    if (pso_wave_form(c, P)) {  // one wave per particle (large swarms)
        const int wpp = pso_wpp(c, P);
        const int per_wg = PW_WPB / wpp;
        const dim3 grid((P + per_wg - 1) / per_wg);
        const bool coop = c->fk_coop;
        auto ki = wpp == 2 ? (coop ? k_pso_init_w<2, true> : k_pso_init_w<2, false>)
                           : (coop ? k_pso_init_w<1, true> : k_pso_init_w<1, false>);
        launch(c, HPE_PROF_PSO_INIT, ki, grid, dim3(PW_NT), 0, d, (const double *)d_state,
               io.obs, (const DevHand *)c->d_hand);
        const bool x = d.ext != nullptr, r16 = d.K <= 15;
        auto kw = wave_gen_kernel(wpp, coop, x, r16);
        for (int g = 1; g <= G; ++g) {
            launch(c, HPE_PROF_PSO_GEN, kw, grid, dim3(PW_NT), 0, d, io.obs,
                   (const DevHand *)c->d_hand, g, W1, C1, C2);
            if ((rc = exchange_after(c, d, g, G))) return rc;
        }
    } else {  // one workgroup per particle (latency form)
        launch(c, HPE_PROF_PSO_INIT, filt ? k_pso_init<true> : k_pso_init<false>, dim3(P), dim3(HPE_NT), 0, d,
               (const double *)d_state, io.obs, (const DevHand *)c->d_hand);
        static const InboxCounts all_k{};  // P > KIN_MAX: the kernel reads K slots
        for (int g = 1; g <= G; ++g) {
            const InboxCounts &kg = c->sw.kin.empty() ? all_k : c->sw.kin[g];
            // the exchange forms only when it is on; the 16-lane informant row when K <= 15
            const bool x = d.ext != nullptr, r16 = d.K <= 15;
            launch(c, HPE_PROF_PSO_GEN,
                   filt ? (x ? (r16 ? k_pso_gen_x<true, true> : k_pso_gen_x<false, true>)
                             : (r16 ? k_pso_gen<true, true> : k_pso_gen<false, true>))
                        : (x ? (r16 ? k_pso_gen_x<true, false> : k_pso_gen_x<false, false>)
                             : (r16 ? k_pso_gen<true, false> : k_pso_gen<false, false>)),
                   dim3(P), dim3(HPE_NT), 0, d, io.obs, (const DevHand *)c->d_hand, g,
                   W1, C1, C2, kg);
            if ((rc = exchange_after(c, d, g, G))) return rc;
        }
    }
    HIPCHK(c, hipGetLastError());
    if (tail) {
        launch(c, HPE_PROF_PSO_FINAL, filt ? k_pso_final<true, true> : k_pso_final<true, false>, dim3(1), dim3(HPE_NT), 0, d,
               subswarm_out(c, d_state), io.obs, (const DevHand *)c->d_hand, io.hand_back,
               pso_wave_form(c, P) ? 0 : 1, io.seq, io.done_host, io.hist,
               (const int *)c->d_mw_err, io.slots, io.seq_obs, io.cur);
        HIPCHK(c, hipGetLastError());
        if ((rc = subswarm_exchange(c, io, pick))) return rc;
    } else {
        launch(c, HPE_PROF_PSO_FINAL, k_pso_final<false>, dim3(1), dim3(HPE_NT), 0, d, d_state,
               (const DevObs *)nullptr, (const DevHand *)nullptr, (DevObs *)nullptr, 0,
               (unsigned long long *)nullptr, (unsigned long long *)nullptr, (double *)nullptr,
               (const int *)nullptr, (const DevObs *)nullptr, (DevObs *)nullptr, (int *)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// Scratch shared with hpe_prepare_frame (tmp cloud, scale terms, DT rows, counter).
static int ensure_prep_scratch(hpe_ctx *c) {
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (!c->d_prep_ctr) {  // assigned last, zeroed (as ensure_batch_lanes)
        HIPCHK(c, alloc_all(c->d_tmp, 3 * npix, c->d_ctb, npix, c->d_dtf, npix));
        DevBuf<unsigned> ctr;
        HIPCHK(c, ctr.alloc(3));
        HIPCHK(c, hipMemset(ctr, 0, 3 * sizeof(unsigned)));
        c->d_prep_ctr = std::move(ctr);
    }
    return HPE_OK;
}

static PrepArgs prep_args(hpe_ctx *c, Slot &s, const float *raw, int to_cm, int downsample,
                          double focal, DevObs *obs_out, PrepInfo *info) {
    PrepArgs a;
    a.raw = raw;
    a.to_cm = to_cm ? 1 : 0;
    a.downsample = downsample ? 1 : 0;
    a.focal = focal;
    a.depth_cm = s.depth;
    a.cx = s.cx;
    a.cy = s.cy;
    a.cz = s.cz;
    a.tmp = c->d_tmp;
    a.ctb = c->d_ctb;
    a.dt = s.dt;
    a.dtf = c->d_dtf;
    a.info = info;
    a.obs_out = obs_out;
    a.ctr = c->d_prep_ctr;
    a.raw_row = nullptr;
    a.raw_stride = 0;
    return a;
}

// hpe_create's and hpe_set_batch_hands' check of one hand: the sphere counts the kernels are
// built for.
static bool hand_counts_ok(const hpe_hand_params &h) {
    const int tb[4] = {2, 2, 2, 2}, fg[4] = {4, 2, 2, 2};
    for (int k = 0; k < 4; ++k)
        if (h.tb_spheres[k] != tb[k] || h.fg_spheres[k] != fg[k]) return false;
    return true;
}
// ... and every value finite (a lane hand: one lane's NaN would otherwise pass for a failed track)
static bool hand_values_finite(const hpe_hand_params &h) {
    for (double v : h.geo_cm)
        if (!std::isfinite(v)) return false;
    for (double v : h.radii_cm)
        if (!std::isfinite(v)) return false;
    for (double v : h.cmc_deg)
        if (!std::isfinite(v)) return false;
    for (double v : h.spacing_cm)
        if (!std::isfinite(v)) return false;
    return true;
}

// Every entry of the lane hand table <- the context's hand (hpe_create; hands == NULL).
static hipError_t reset_lane_hands(hpe_ctx *c) {
    std::vector<DevHand> tab(HPE_BATCH_MAX, c->hand);
    return hipMemcpy(c->d_lane_hands, tab.data(), sizeof(DevHand) * tab.size(), hipMemcpyHostToDevice);
}

static int check_P(hpe_ctx *c, int P) {
    if (P < 1 || P > 8192) return fail(c, HPE_E_ARG, "num_p %d out of range [1, 8192]", P);
    return HPE_OK;
}

extern "C" {

int hpe_abi_version(void) { return HPE_ABI_VERSION; }

const char *hpe_last_error(const hpe_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int hpe_preprocess_depth(const float *depth_mm, int to_cm, int downsample, double focal,
                         double *depth_cm_out, float *dt_out, double *cloud_out,
                         int32_t *n_out, double *scale_out, double *dtmax_out,
                         double K_out[9]) {
    if (!depth_mm || !depth_cm_out || !dt_out || !cloud_out || !n_out || !scale_out ||
        !dtmax_out || !K_out)
        return HPE_E_ARG;
    return hpe::preprocess_depth(depth_mm, to_cm, downsample, focal, depth_cm_out, dt_out,
                                 cloud_out, n_out, scale_out, dtmax_out, K_out);
}

int hpe_create(hpe_ctx **out, int device, const hpe_hand_params *hand) {
    if (!out || !hand) return HPE_E_ARG;
    *out = nullptr;
    if (!hand_counts_ok(*hand)) return HPE_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return HPE_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HPE_E_NODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HPE_E_NODEVICE;
    hpe_ctx *c = new (std::nothrow) hpe_ctx();
    if (!c) return HPE_E_NOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || c->stream.ensure(hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return HPE_E_HIP;
    }
    hpe::build_dev_hand(*hand, c->hand);
    if (c->d_hand.alloc(1) != hipSuccess ||
        hipMemcpy(c->d_hand, &c->hand, sizeof(DevHand), hipMemcpyHostToDevice) != hipSuccess ||
        c->d_lane_hands.alloc(HPE_BATCH_MAX) != hipSuccess || reset_lane_hands(c) != hipSuccess ||
        c->d_state.alloc(32) != hipSuccess || c->d_evals.alloc(4) != hipSuccess ||
        hipMemset(c->d_evals, 0, 4 * sizeof(int)) != hipSuccess ||
        c->d_obs.alloc(HPE_MAX_SLOTS) != hipSuccess || c->d_obs_active.alloc(1) != hipSuccess ||
        c->d_seq_obs.alloc(1) != hipSuccess || c->d_seq_cur.alloc(2) != hipSuccess ||
        c->d_mw_job.alloc(1) != hipSuccess ||
        c->d_mw_part.alloc((size_t)MW_MAX_Q * MW_MAX_NODES) != hipSuccess ||
        c->d_mw_ctr.alloc(MW_CTR_WORDS) != hipSuccess ||
        hipMemset(c->d_mw_ctr, 0, MW_CTR_WORDS * sizeof(unsigned)) != hipSuccess ||
        c->d_mw_err.alloc(1) != hipSuccess || hipMemset(c->d_mw_err, 0, sizeof(int)) != hipSuccess ||
        c->d_spec_g.alloc(SPEC_GRAN) != hipSuccess ||
        hipMemset(c->d_spec_g, 0, SPEC_GRAN * sizeof(unsigned long long)) != hipSuccess ||
        c->d_spec_ep.alloc(64) != hipSuccess ||
        hipMemset(c->d_spec_ep, 0, 64 * sizeof(unsigned)) != hipSuccess ||
        c->h_pinned.alloc(256, 0) != hipSuccess || c->h_mw_err.alloc(1, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        hpe_destroy(c);
        return HPE_E_HIP;
    }
    c->slots.resize(1);
    if (const char *pf = std::getenv("HPE_PSO_FORM"))
        c->pso_form = std::strcmp(pf, "block") == 0 ? 1 : std::strcmp(pf, "wave") == 0 ? 2 : 0;
    if (const char *wp = std::getenv("HPE_PSO_WPP")) {
        const int v = std::atoi(wp);
        c->pso_wpp = (v == 1 || v == 2) ? v : 0;
    }
    if (const char *fc = std::getenv("HPE_FK_COOP")) c->fk_coop = std::atoi(fc) != 0;
    if (const char *rm = std::getenv("HPE_REFINE_MW")) c->refine_mw = rm[0] != '0';
    if (const char *re = std::getenv("HPE_REFINE_EXACT")) c->refine_exact = re[0] == '1';
    if (const char *sp = std::getenv("HPE_MW_SPIN")) c->mw_spin = std::max(0, std::atoi(sp));
    if (const char *rs = std::getenv("HPE_REFINE_SPEC")) c->refine_spec = rs[0] != '0';
    if (const char *ss = std::getenv("HPE_SPEC_SPIN")) c->spec_spin = std::max(0, std::atoi(ss));
    if (const char *ps = std::getenv("HPE_PREP_SPLIT")) c->prep_split = ps[0] != '0';
    *c->h_mw_err = 0;
    const char *ng = std::getenv("HPE_NO_GRAPH");
    c->use_graph = !(ng && ng[0] == '1');
    *out = c;
    return HPE_OK;
}

// Every cached tracking graph destroyed (the stream drained first).  Graphs that captured the
// subswarm exchange hold RCCL resources, so they go before the communicator does.
static void drop_graphs(hpe_ctx *c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (GraphCache &gc : c->graphs) {
        for (auto &e : gc.entries) (void)hipGraphExecDestroy(e.exec);
        gc.entries.clear();
    }
}

// What has an order the owners cannot express: the streams drained, then the graphs before the
// communicator their exchange nodes use, then the context -- whose members release themselves,
// the streams last (hpe_ctx::stream).
int hpe_destroy(hpe_ctx *c) {
    if (!c) return HPE_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->prep) (void)hipStreamSynchronize(c->prep);
    drop_graphs(c);
    if (c->ss.comm) (void)rccl_api().comm_destroy(c->ss.comm);
    delete c;
    return HPE_OK;
}

void *hpe_stream(hpe_ctx *c) { return c ? (void *)c->stream.get() : nullptr; }

static int mw_check(hpe_ctx *c);

// Also surfaces a multi-workgroup refine hand-off timeout of any frame enqueued since the
// last check (device flag, cleared when read): pipelined and device-state frames run
// without a per-frame host check.
int hpe_sync(hpe_ctx *c) {
    if (!c) return HPE_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return mw_check(c);
}

int hpe_store_frame(hpe_ctx *c, int slot, const hpe_frame *f) {
    if (!c) return HPE_E_ARG;
    if (!f || !f->depth_cm || !f->dt || (!f->cloud && f->n > 0) || f->n < 0 || f->n > 76800 ||
        slot < 0 || slot >= HPE_MAX_SLOTS)
        return fail(c, HPE_E_ARG, "bad frame (slot %d, n %d)", slot, f ? f->n : -1);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // in-flight work may read this slot
    if (c->prep) HIPCHK(c, hipStreamSynchronize(c->prep));
    if ((int)c->slots.size() <= slot) c->slots.resize(slot + 1);
    Slot &s = c->slots[slot];
    HIPCHK(c, slot_buffers(s, f->n));
    std::vector<double> soa(3 * (size_t)f->n);  // AoS (N x 3) -> SoA for coalesced loads
    for (int p = 0; p < f->n; ++p)
        for (int q = 0; q < 3; ++q) soa[(size_t)q * f->n + p] = f->cloud[3 * (size_t)p + q];
    HIPCHK(c, hipMemcpy(s.depth, f->depth_cm, sizeof(double) * HPE_IMG_H * HPE_IMG_W, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(s.dt, f->dt, sizeof(float) * HPE_IMG_H * HPE_IMG_W, hipMemcpyHostToDevice));
    if (f->n > 0) {
        HIPCHK(c, hipMemcpy(s.cx, soa.data(), sizeof(double) * f->n, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(s.cy, soa.data() + f->n, sizeof(double) * f->n, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(s.cz, soa.data() + 2 * (size_t)f->n, sizeof(double) * f->n, hipMemcpyHostToDevice));
    }
    s.n = f->n;
    s.scale = f->scale;
    s.dtmax = f->dtmax;
    std::memcpy(s.K, f->K, sizeof(s.K));
    s.valid = true;
    s.dev = false;
    s.known = true;
    s.n_max = f->n;
    const DevObs od = make_obs(s);
    HIPCHK(c, hipMemcpy(c->d_obs + slot, &od, sizeof(DevObs), hipMemcpyHostToDevice));
    if (slot == c->cur)
        HIPCHK(c, hipMemcpy(c->d_obs_active, &od, sizeof(DevObs), hipMemcpyHostToDevice));
    int rc = ensure_match(c, (size_t)(f->n > 0 ? f->n : 1));
    return rc;
}

int hpe_select_frame(hpe_ctx *c, int slot) {
    if (!c) return HPE_E_ARG;
    if (slot < 0 || slot >= (int)c->slots.size() || !c->slots[slot].valid)
        return fail(c, HPE_E_ARG, "slot %d holds no frame", slot);
    HIPCHK(c, hipSetDevice(c->device));
    Slot &s = c->slots[slot];
    if (slot != c->cur || s.dev) {  // stream-ordered: work already queued keeps its frame
        if (c->cur >= 0 && c->cur != slot) {  // everything queued so far used the old frame
            Slot &o = c->slots[c->cur];
            HIPCHK(c, o.done.ensure(hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(o.done, c->stream));
            o.done_valid = true;
        }
        if (s.dev) HIPCHK(c, hipStreamWaitEvent(c->stream, s.ready, 0));
        HIPCHK(c, hipMemcpyAsync(c->d_obs_active, c->d_obs + slot, sizeof(DevObs),
                                 hipMemcpyDeviceToDevice, c->stream));
    }
    c->cur = slot;
    return HPE_OK;
}

int hpe_prepare_frame(hpe_ctx *c, int slot, const float *depth_mm, int to_cm, int downsample,
                      double focal) {
    if (!c) return HPE_E_ARG;
    if (!depth_mm || slot < 0 || slot >= HPE_MAX_SLOTS || !(focal > 0))
        return fail(c, HPE_E_ARG, "bad arguments (slot %d)", slot);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    HIPCHK(c, c->prep.ensure(hipStreamNonBlocking));
    if (!c->raw_ev[HPE_RAW_RING - 1]) {  // created last: a block that failed part way runs again
        HIPCHK(c, c->d_raw.alloc(npix));
        int rc0 = ensure_prep_scratch(c);
        if (rc0) return rc0;
        HIPCHK(c, c->d_info.alloc((size_t)HPE_MAX_SLOTS));
        for (int k = 0; k < HPE_RAW_RING; ++k) {
            HIPCHK(c, c->h_raw[k].alloc(npix, 0));
            HIPCHK(c, c->raw_ev[k].ensure(hipEventDisableTiming));
        }
    }
    if ((int)c->slots.size() <= slot) c->slots.resize(slot + 1);
    Slot &s = c->slots[slot];
    const int need = downsample ? 250 : (int)npix;
    if (!s.depth || s.cap < need) {  // (re)allocation: nothing may still use the slot
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->prep));
        if (s.cap < need) ++c->epoch;
        HIPCHK(c, slot_buffers(s, need));
    }
    HIPCHK(c, s.ready.ensure(hipEventDisableTiming));
    // the frame's previous contents may still be read by queued tracking work
    if (slot == c->cur) {
        HIPCHK(c, s.done.ensure(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(s.done, c->stream));
        s.done_valid = true;
    }
    if (s.done_valid) HIPCHK(c, hipStreamWaitEvent(c->prep, s.done, 0));
    if (c->seq_done_valid) HIPCHK(c, hipStreamWaitEvent(c->prep, c->seq_done, 0));
    // start once the tracking stream has finished the work queued so far: a frame
    // prepared just before the current one is tracked then runs beside that frame's
    // single-workgroup refine rather than beside the full-chip PSO generations
    {
        HIPCHK(c, c->main_mark.ensure(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->main_mark, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->prep, c->main_mark, 0));
    }
    // raw depth through a pinned double buffer
    const int k = c->raw_k;
    c->raw_k = (k + 1) % HPE_RAW_RING;
    if (c->raw_ev_valid[k]) HIPCHK(c, hipEventSynchronize(c->raw_ev[k]));
    std::memcpy(c->h_raw[k], depth_mm, sizeof(float) * npix);
    HIPCHK(c, hipMemcpyAsync(c->d_raw, c->h_raw[k], sizeof(float) * npix, hipMemcpyHostToDevice, c->prep));
    HIPCHK(c, hipEventRecord(c->raw_ev[k], c->prep));
    c->raw_ev_valid[k] = true;
    hpe_ctx::Pool &pl = c->pools[HPE_PROF_PREP];
    const bool rec = c->prof && pl.used + 2 <= pl.ev.size();
    if (rec) HIPCHK(c, hipEventRecord(pl.ev[pl.used], c->prep));
    const PrepArgs pa = prep_args(c, s, c->d_raw, to_cm, downsample, focal, c->d_obs + slot,
                                  c->d_info + slot);
    hipLaunchKernelGGL(k_prepare, dim3(PREP_WG), dim3(PREP_NT), 0, c->prep, pa);
    if (rec) {
        HIPCHK(c, hipEventRecord(pl.ev[pl.used + 1], c->prep));
        pl.used += 2;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s.ready, c->prep));
    const double Kv[9] = {focal, 0.0, 160.0, 0.0, focal, 120.0, 0.0, 0.0, 1.0};
    std::memcpy(s.K, Kv, sizeof(Kv));
    s.valid = true;
    s.dev = true;
    s.known = false;
    s.n_max = need;
    return HPE_OK;
}

int hpe_frame_readback(hpe_ctx *c, int slot, double *depth_cm, float *dt, double *cloud,
                       int32_t *n_out, double *scale_out, double *dtmax_out) {
    if (!c) return HPE_E_ARG;
    if (slot < 0 || slot >= (int)c->slots.size() || !c->slots[slot].valid)
        return fail(c, HPE_E_ARG, "slot %d holds no frame", slot);
    HIPCHK(c, hipSetDevice(c->device));
    Slot &s = c->slots[slot];
    int rc = slot_known(c, s, slot);
    if (rc) return rc;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (depth_cm) HIPCHK(c, hipMemcpy(depth_cm, s.depth, sizeof(double) * npix, hipMemcpyDeviceToHost));
    if (dt) HIPCHK(c, hipMemcpy(dt, s.dt, sizeof(float) * npix, hipMemcpyDeviceToHost));
    if (cloud && s.n > 0) {
        std::vector<double> soa(3 * (size_t)s.n);
        HIPCHK(c, hipMemcpy(soa.data(), s.cx, sizeof(double) * s.n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(soa.data() + s.n, s.cy, sizeof(double) * s.n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(soa.data() + 2 * (size_t)s.n, s.cz, sizeof(double) * s.n, hipMemcpyDeviceToHost));
        for (int p = 0; p < s.n; ++p)
            for (int q = 0; q < 3; ++q) cloud[3 * (size_t)p + q] = soa[(size_t)q * s.n + p];
    }
    if (n_out) *n_out = s.n;
    if (scale_out) *scale_out = s.scale;
    if (dtmax_out) *dtmax_out = s.dtmax;
    return HPE_OK;
}

int hpe_set_frame(hpe_ctx *c, const hpe_frame *f) {
    int rc = hpe_store_frame(c, 0, f);
    return rc ? rc : hpe_select_frame(c, 0);
}

int hpe_build_spheres(hpe_ctx *c, const double *theta, int P, double *S_out, double *J_out) {
    if (!c) return HPE_E_ARG;
    if (!theta || !S_out || P < 1) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_theta(c, P);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * HPE_DOF * P, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_build, dim3(P), dim3(HPE_NT), 0, c->stream, c->d_theta, P, c->d_hand,
                       c->d_S, J_out ? c->d_J : nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(S_out, c->d_S, sizeof(double) * 3 * HPE_NS * P, hipMemcpyDeviceToHost, c->stream));
    if (J_out)
        HIPCHK(c, hipMemcpyAsync(J_out, c->d_J, sizeof(double) * 63 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HPE_OK;
}

int hpe_eval_costs(hpe_ctx *c, const double *theta, int P, int with_collision, double *cost_out,
                   int32_t *match_out) {
    if (!c) return HPE_E_ARG;
    if (!theta || !cost_out || P < 1) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    int rc = need_frame(c, &o);
    if (rc) return rc;
    if ((rc = ensure_theta(c, P))) return rc;
    int32_t *dm = nullptr;
    if (match_out) {
        if ((rc = ensure_match(c, (size_t)P * (o.n > 0 ? o.n : 1)))) return rc;
        dm = c->d_match;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * HPE_DOF * P, hipMemcpyHostToDevice, c->stream));
    if (with_collision) {
        // cal_cost2 needs a match buffer even when the caller does not want it back
        if ((rc = ensure_match(c, (size_t)P * (o.n > 0 ? o.n : 1)))) return rc;
        hipLaunchKernelGGL(k_eval<EV_COST2_CORR>, dim3(P), dim3(HPE_NT), 0, c->stream,
                           c->d_theta, P, c->d_obs_active, c->d_hand, c->d_cost, c->d_match, c->d_terms);
        dm = c->d_match;
    } else if (dm) {
        hipLaunchKernelGGL(k_eval<EV_COST_STORE>, dim3(P), dim3(HPE_NT), 0, c->stream,
                           c->d_theta, P, c->d_obs_active, c->d_hand, c->d_cost, dm, c->d_terms);
    } else {
        hipLaunchKernelGGL(k_eval<EV_COST>, dim3(P), dim3(HPE_NT), 0, c->stream, c->d_theta, P,
                           c->d_obs_active, c->d_hand, c->d_cost, (int32_t *)nullptr, c->d_terms);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cost_out, c->d_cost, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
    if (match_out)
        HIPCHK(c, hipMemcpyAsync(match_out, dm, sizeof(int32_t) * (size_t)P * o.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HPE_OK;
}

int hpe_cal_cost2(hpe_ctx *c, const double theta[26], int32_t *match, int compute_corr,
                  double *cost_out, double terms_out[3]) {
    if (!c) return HPE_E_ARG;
    if (!theta || !match || !cost_out) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    int rc = need_frame(c, &o);
    if (rc) return rc;
    if ((rc = ensure_theta(c, 1))) return rc;
    if ((rc = ensure_match(c, (size_t)(o.n > 0 ? o.n : 1)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice, c->stream));
    if (compute_corr) {
        hipLaunchKernelGGL(k_eval<EV_COST2_CORR>, dim3(1), dim3(HPE_NT), 0, c->stream, c->d_theta,
                           1, c->d_obs_active, c->d_hand, c->d_cost, c->d_match, c->d_terms);
    } else {
        for (int p = 0; p < o.n; ++p)
            if (match[p] < 0 || match[p] >= HPE_NS)
                return fail(c, HPE_E_ARG, "match[%d] = %d out of range", p, match[p]);
        HIPCHK(c, hipMemcpyAsync(c->d_match, match, sizeof(int32_t) * o.n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_eval<EV_COST2_FROZEN>, dim3(1), dim3(HPE_NT), 0, c->stream,
                           c->d_theta, 1, c->d_obs_active, c->d_hand, c->d_cost, c->d_match, c->d_terms);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->d_cost, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_pinned + 1, c->d_terms, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    if (compute_corr)
        HIPCHK(c, hipMemcpyAsync(match, c->d_match, sizeof(int32_t) * o.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *cost_out = c->h_pinned[0];
    if (terms_out) std::memcpy(terms_out, c->h_pinned + 1, sizeof(double) * 3);
    return HPE_OK;
}

int hpe_eval_spheres(hpe_ctx *c, const double *S, int P, int compute_corr, int32_t *match,
                     double *terms_out) {
    if (!c) return HPE_E_ARG;
    if (!S || !match || !terms_out || P < 1) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    int rc = need_frame(c, &o);
    if (rc) return rc;
    if ((rc = ensure_theta(c, P))) return rc;
    const size_t nm = (size_t)P * o.n;
    if ((rc = ensure_match(c, nm > 0 ? nm : 1))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_S, S, sizeof(double) * 3 * HPE_NS * P, hipMemcpyHostToDevice, c->stream));
    if (compute_corr) {
        hipLaunchKernelGGL(k_eval_spheres<EV_COST2_CORR>, dim3(P), dim3(HPE_NT), 0, c->stream,
                           c->d_S, P, c->d_obs_active, c->d_hand, c->d_match, c->d_terms);
    } else {
        for (size_t q = 0; q < nm; ++q)
            if (match[q] < 0 || match[q] >= HPE_NS)
                return fail(c, HPE_E_ARG, "match[%zu] = %d out of range", q, match[q]);
        HIPCHK(c, hipMemcpyAsync(c->d_match, match, sizeof(int32_t) * nm, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_eval_spheres<EV_COST2_FROZEN>, dim3(P), dim3(HPE_NT), 0, c->stream,
                           c->d_S, P, c->d_obs_active, c->d_hand, c->d_match, c->d_terms);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(terms_out, c->d_terms, sizeof(double) * 3 * P, hipMemcpyDeviceToHost, c->stream));
    if (compute_corr)
        HIPCHK(c, hipMemcpyAsync(match, c->d_match, sizeof(int32_t) * nm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HPE_OK;
}

int hpe_set_pso_params(hpe_ctx *c, const double ub[26], const double lb[26], const double sd[26],
                       double omega, double phip, double phig, int maxiter, double minstep,
                       double minfunc) {
    if (!c) return HPE_E_ARG;
    if (!ub || !lb || !sd || maxiter < 1 || maxiter > 100000)
        return fail(c, HPE_E_ARG, "bad PSO parameters (maxiter %d)", maxiter);
    std::memcpy(c->ub, ub, sizeof(c->ub));
    std::memcpy(c->lb, lb, sizeof(c->lb));
    std::memcpy(c->sd, sd, sizeof(c->sd));
    c->omega = omega;
    c->phip = phip;
    c->phig = phig;
    c->maxiter = maxiter;
    c->minstep = minstep;
    c->minfunc = minfunc;
    c->params = true;
    c->bounds_dirty = true;
    return HPE_OK;
}

int hpe_set_seed(hpe_ctx *c, uint64_t seed) {
    if (!c) return HPE_E_ARG;
    c->seed = seed;
    return HPE_OK;
}

int hpe_pso_evolve(hpe_ctx *c, const double x0[26], int P, double bestp[26], double *bestcost) {
    if (!c) return HPE_E_ARG;
    if (!x0 || !bestp) return fail(c, HPE_E_ARG, "bad arguments");
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    int rc = check_P(c, P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    if ((rc = need_frame(c, &o))) return rc;
    std::memcpy(c->h_pinned + 64, x0, sizeof(double) * HPE_DOF);
    HIPCHK(c, hipMemcpyAsync(c->d_state, c->h_pinned + 64, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice, c->stream));
    if ((rc = ensure_swarm(c, P, generations(c))) || (rc = upload_bounds(c))) return rc;
    if ((rc = launch_pso(c, P, FrameIo{c->d_obs_active, o.n, c->d_state}, false))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->d_state, sizeof(double) * 27, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(bestp, c->h_pinned, sizeof(double) * HPE_DOF);
    if (bestcost) *bestcost = c->h_pinned[26];
    return HPE_OK;
}

int hpe_pso_trace(hpe_ctx *c, double *gbest, int32_t *count, int32_t *topo, int n) {
    if (!c) return HPE_E_ARG;
    if (n < 0 || n > c->sw.G) return fail(c, HPE_E_ARG, "trace length %d > G %d", n, c->sw.G);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n == 0) return HPE_OK;
    if (gbest) HIPCHK(c, hipMemcpy(gbest, c->sw.trace_g, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (count) HIPCHK(c, hipMemcpy(count, c->sw.trace_count, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (topo) HIPCHK(c, hipMemcpy(topo, c->sw.trace_topo, sizeof(int) * n, hipMemcpyDeviceToHost));
    return HPE_OK;
}

// pso_optimise buffers for (P, G, seed, cloud size n); per-particle matchId in HBM only
// for clouds too large for the descent kernel's LDS.
static int ensure_opt(hpe_ctx *c, int P, int G, int n) {
    OptState &s = c->opt;
    const int need_n = n > RF_STAGE_MAX ? n : 0;
    if (s.P == P && s.G >= G && s.seed == c->seed && s.n_cap >= need_n) return HPE_OK;
    s = OptState{};
    OptState o;  // built here and moved in whole
    const size_t e = (size_t)P * HPE_DOF;
    HIPCHK(c, alloc_all(o.x, e, o.v, e, o.pb, e, o.pc, (size_t)P, o.gbest, (size_t)28,
                        o.trace, (size_t)(G > 0 ? G : 1), o.normals, e, o.bounds, (size_t)3 * HPE_DOF,
                        o.match, (size_t)P * (need_n > 0 ? need_n : 1), o.ctr, (size_t)ARRIVE_SHARDS * 32 + 1));
    HIPCHK(c, hipMemset(o.ctr, 0, sizeof(unsigned) * (ARRIVE_SHARDS * 32 + 1)));
    std::vector<double> nrm(e);
    hpe::make_normals(c->seed, P, nrm.data(), ST_OPT_NORMAL);
    HIPCHK(c, hipMemcpy(o.normals, nrm.data(), sizeof(double) * e, hipMemcpyHostToDevice));
    o.P = P;
    o.G = G;
    o.n_cap = need_n;
    o.seed = c->seed;
    s = std::move(o);
    return HPE_OK;
}

int hpe_pso_optimise(hpe_ctx *c, const double x0[26], int P, double bestp[26],
                     double *bestcost, double *gbest_trace, int trace_len) {
    if (!c) return HPE_E_ARG;
    if (!x0 || !bestp) return fail(c, HPE_E_ARG, "bad arguments");
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    int rc = check_P(c, P);
    if (rc) return rc;
    const int G = generations(c);  // while (iter < maxiter), iter from 1
    if (trace_len < 0 || trace_len > G || (trace_len > 0 && !gbest_trace))
        return fail(c, HPE_E_ARG, "trace length %d > maxiter-1 = %d", trace_len, G);
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    if ((rc = need_frame(c, &o))) return rc;
    if ((rc = ensure_opt(c, P, G, o.n))) return rc;
    OptState &s = c->opt;
    double b[3 * HPE_DOF];
    std::memcpy(b, c->lb, sizeof(c->lb));
    std::memcpy(b + HPE_DOF, c->ub, sizeof(c->ub));
    std::memcpy(b + 2 * HPE_DOF, c->sd, sizeof(c->sd));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(s.bounds, b, sizeof(b), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_state, x0, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice));
    DevOpt d;
    d.x = s.x;
    d.v = s.v;
    d.pb = s.pb;
    d.pc = s.pc;
    d.gbest = s.gbest;
    d.trace = s.trace;
    d.match = s.match;
    d.ctr = s.ctr;
    d.normals = s.normals;
    d.bounds = s.bounds;
    d.seed = c->seed;
    d.P = P;
    d.G = G;
    d.n_cap = s.n_cap;
    d.w = c->omega;
    d.c1 = c->phip;
    d.c2 = c->phig;
    const bool staged = o.n <= RF_STAGE_MAX;
    const unsigned lds = staged ? (unsigned)((size_t)o.n * (3 * sizeof(double) + sizeof(int32_t))) : 0u;
    launch(c, HPE_PROF_PSO_INIT, k_opt_init, dim3(P), dim3(HPE_NT), 0, d, (const double *)c->d_state,
           c->d_obs_active.get(), (const DevHand *)c->d_hand);
    for (int g = 1; g <= G; ++g) {
        if (staged)
            launch(c, HPE_PROF_OPT_DESCENT, k_opt_descent<true>, dim3(P), dim3(RF_NT), lds, d,
                   c->d_obs_active.get(), (const DevHand *)c->d_hand, g);
        else
            launch(c, HPE_PROF_OPT_DESCENT, k_opt_descent<false>, dim3(P), dim3(RF_NT), lds, d,
                   c->d_obs_active.get(), (const DevHand *)c->d_hand, g);
        launch(c, HPE_PROF_OPT_MOVE, k_opt_move, dim3(P), dim3(HPE_NT), 0, d, c->d_obs_active.get(),
               (const DevHand *)c->d_hand, g);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, s.gbest, sizeof(double) * 27, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(bestp, c->h_pinned, sizeof(double) * HPE_DOF);
    if (bestcost) *bestcost = c->h_pinned[26];
    if (trace_len > 0)
        HIPCHK(c, hipMemcpy(gbest_trace, s.trace, sizeof(double) * trace_len, hipMemcpyDeviceToHost));
    return HPE_OK;
}

#define RF_DYN_LDS (126u * 1024u)
static_assert(RF_DYN_LDS >= RF_STAGE_MAX * (3 * sizeof(double) + sizeof(int32_t)), "staging");

// The multi-workgroup refine's hand-offs need workgroup 0, its MW_MAX_Q helpers and the
// preparation workgroups resident at once: chosen only if the device's occupancy for that
// kernel holds them all (else the single-workgroup form runs the full cloud, slower but
// with no cross-workgroup wait).  Cached per context.
static bool mw_fits(hpe_ctx *c) {
    if (c->mw_fits < 0) {
        int per_cu = 0, cus = 0;
        auto k = c->refine_exact ? k_refine<false, true> : k_refine<false, true, true>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, RF_NT, prep_lds_bytes()) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess)
            per_cu = cus = 0;
        c->mw_fits = (long)per_cu * cus >= 1 + MW_MAX_Q + PREP_WG ? 1 : 0;
    }
    return c->mw_fits == 1;
}

// The speculated translation block gains only with the leader, the runner and the preparation
// workgroups resident at once (a runner that starts late only costs the leader its bounded
// wait): checked once per context and refine form, as mw_fits; else the one-workgroup form.
static bool spec_fits(hpe_ctx *c) {
    if (c->spec_fits < 0) {
        int per_cu = 0, cus = 0;
        auto k = c->refine_exact ? k_refine<true, false, false, true> : k_refine<true, false, true, true>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, RF_NT, RF_DYN_LDS) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess)
            per_cu = cus = 0;
        c->spec_fits = (long)per_cu * cus >= 2 + PREP_WG ? 1 : 0;
    }
    return c->spec_fits == 1;
}

// refine_init_pose on io's frame (do_refine) and, when pa != NULL, the next frame's
// preparation in the same launch (workgroups 1, 2).  *pick: the previous frame's exchange
// pick, which this launch takes (and empties: do_refine is the chunk loops' rule).
static int refine_launch(hpe_ctx *c, const FrameIo &io, int do_refine, const PrepArgs *pa = nullptr,
                         const PrepSplit *split = nullptr, DevPick *pick = nullptr) {
    int rc = ensure_match(c, (size_t)(io.n_max > 0 ? io.n_max : 1));
    if (rc) return rc;
    double *d_x0 = io.state;
    PrepArgs none;
    std::memset(&none, 0, sizeof(none));
    const PrepArgs a = pa ? *pa : none;
    const PrepSplit ps = (pa && split) ? *split : PrepSplit{};
    DevMw mw;
    std::memset(&mw, 0, sizeof(mw));
    const DevPick pk = pick ? *pick : DevPick{};
    if (pick) *pick = DevPick{};
    const DevSpec nosp{};
    if (io.n_max <= RF_STAGE_MAX && c->refine_spec && spec_fits(c)) {
        // two refine workgroups (the leader and the translation block's runner), each with the
        // padded dynamic LDS below and so a CU of its own; the preparation workgroups follow
        const DevSpec sp{c->d_spec_g, c->d_spec_ep, c->spec_spin};
        const dim3 grid(pa ? 2 + PREP_WG : 2);
        launch(c, HPE_PROF_REFINE,
               c->refine_exact ? k_refine<true, false, false, true> : k_refine<true, false, true, true>,
               grid, dim3(RF_NT), RF_DYN_LDS, d_x0, io.obs, (const DevHand *)c->d_hand,
               c->d_match.get(), c->d_evals.get(), do_refine, a, mw, pk, ps, sp);
    } else if (io.n_max <= RF_STAGE_MAX) {
        // The dynamic LDS is padded to (almost) the whole CU: no other workgroup can share
        // the CU of this single-workgroup, latency-bound kernel.  Fixed size: the launch is
        // identical for every frame.
        const dim3 grid(pa ? 1 + PREP_WG : 1);
        launch(c, HPE_PROF_REFINE, c->refine_exact ? k_refine<true> : k_refine<true, false, true>,
               grid, dim3(RF_NT), RF_DYN_LDS, d_x0, io.obs, (const DevHand *)c->d_hand,
               c->d_match.get(), c->d_evals.get(), do_refine, a, mw, pk, ps, nosp);
    } else if (c->refine_mw && mw_fits(c)) {  // multi-workgroup form: MW_MAX_Q helpers own cloud slices
        mw.job = c->d_mw_job;
        mw.part = c->d_mw_part;
        mw.ctr = c->d_mw_ctr;
        mw.err = c->d_mw_err;
        mw.err_host = c->h_mw_err.dev();
        mw.Q = MW_MAX_Q;
        mw.spin = c->mw_spin;
        const dim3 grid(1 + MW_MAX_Q + (pa ? PREP_WG : 0));
        launch(c, HPE_PROF_REFINE,
               c->refine_exact ? k_refine<false, true> : k_refine<false, true, true>, grid,
               dim3(RF_NT), (unsigned)prep_lds_bytes(), d_x0, io.obs, (const DevHand *)c->d_hand,
               c->d_match.get(), c->d_evals.get(), do_refine, a, mw, pk, ps, nosp);
    } else {
        const dim3 grid(pa ? 1 + PREP_WG : 1);
        launch(c, HPE_PROF_REFINE, c->refine_exact ? k_refine<false> : k_refine<false, false, true>,
               grid, dim3(RF_NT), RF_DYN_LDS, d_x0,
               io.obs, (const DevHand *)c->d_hand, c->d_match.get(), c->d_evals.get(), do_refine, a,
               mw, pk, ps, nosp);
    }
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// A multi-workgroup refine whose waits timed out (DevMw::err) ended early: report it
// and reset the hand-off counters (synchronous).
static int mw_check(hpe_ctx *c) {
    if (!c->d_mw_err) return HPE_OK;
    int err = 0;
    HIPCHK(c, hipMemcpy(&err, c->d_mw_err, sizeof(int), hipMemcpyDeviceToHost));
    if (!err && !(c->h_mw_err && *(volatile int *)c->h_mw_err)) return HPE_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the failed launch has ended
    HIPCHK(c, hipMemset(c->d_mw_ctr, 0, MW_CTR_WORDS * sizeof(unsigned)));
    HIPCHK(c, hipMemset(c->d_mw_err, 0, sizeof(int)));
    if (c->h_mw_err) *(volatile int *)c->h_mw_err = 0;
    return fail(c, HPE_E_HIP, "multi-workgroup refine: a helper hand-off timed out (that "
                              "frame's pose and cost are NaN, and so are those of the frames "
                              "enqueued after it in the same submission)");
}

// A tracking call first surfaces a timeout of an earlier frame's multi-workgroup refine that
// the kernel has already flagged in pinned host memory (no synchronisation unless set).
static int mw_check_async(hpe_ctx *c) {
    if (c->h_mw_err && *(volatile int *)c->h_mw_err) return mw_check(c);
    return HPE_OK;
}

// One tracked frame of a single sequence (testmodel.cpp:126-132), the frame every single-sequence
// tracking call enqueues: refine_init_pose (:126) with, when next != NULL, the following
// frame's preparation (next_frame of the next iteration) in the same launch; then pso_evolve
// (:130) and c = cal_cost(bestp) (:132) over the gbest cost in one final kernel, and the
// subswarm exchange.  *pick: the exchange's deferred pick, carried from frame to frame of a chunk.
static int track_frame(hpe_ctx *c, int P, int refine, const FrameIo &io,
                       const PrepArgs *next = nullptr, const PrepSplit *split = nullptr,
                       DevPick *pick = nullptr) {
    if (refine || next)
        if (int rc = refine_launch(c, io, refine, next, split, pick)) return rc;
    return launch_pso(c, P, io, true, pick);
}

// What the four chunked tracking calls (sequence, raw sequence and their batches) check first.
static int check_chunked_call(hpe_ctx *c, int P, int frames_per_graph) {
    if (int rc = mw_check_async(c)) return rc;
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    if (int rc = check_P(c, P)) return rc;
    if (frames_per_graph < 0 || frames_per_graph > HPE_SEQ_MAX_CHUNK)
        return fail(c, HPE_E_ARG, "frames_per_graph %d out of range [0, %d]", frames_per_graph,
                    HPE_SEQ_MAX_CHUNK);
    return HPE_OK;
}

// ... and the two batch calls after it: the lane count, and what a batch runs without.
static int check_batch_call(hpe_ctx *c, int P, int B) {
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (c->batch_form == HPE_BATCH_FORM_AUTO && pso_wave_form(c, P))
        return fail(c, HPE_E_ARG, "num_p %d takes the wave form: a batch needs the workgroup form "
                    "(num_p < %d)", P, c->wave_form_min_p);
    if (c->ss.transport())
        return fail(c, HPE_E_STATE, "a subswarm transport is live: a batch runs without the "
                    "exchange (hpe_subswarm_fini)");
    if (c->xch_every > 0)
        return fail(c, HPE_E_STATE, "the per-generation exchange is on (hpe_set_exchange)");
    return HPE_OK;
}

// The chunked calls' trailer: the call is its frames' last reader, and hpe_prepare_frame waits
// for this event before it writes a slot.
static int mark_seq_done(hpe_ctx *c) {
    HIPCHK(c, c->seq_done.ensure(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->seq_done, c->stream));
    c->seq_done_valid = true;
    return HPE_OK;
}

int hpe_pick_best(hpe_ctx *c, const double *d_gathered, int world, double *d_state) {
    if (!c) return HPE_E_ARG;
    if (!d_gathered || !d_state || world < 1 || world > 64)
        return fail(c, HPE_E_ARG, "pick_best: null buffer or world %d outside [1, 64]", world);
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_pick_best, dim3(1), dim3(64), 0, c->stream, d_gathered, world, d_state);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

int hpe_set_exchange(hpe_ctx *c, int every, double *d_ext, hpe_exchange_fn fn, void *user) {
    if (!c || every < 0) return HPE_E_ARG;
    if (every > 0 && (!d_ext || !fn)) return fail(c, HPE_E_ARG, "exchange: null buffer or callback");
    c->xch_every = every;
    c->xch_ext = every > 0 ? d_ext : nullptr;
    c->xch_fn = every > 0 ? fn : nullptr;
    c->xch_user = every > 0 ? user : nullptr;
    ++c->epoch;  // the captured graphs do not contain the exchange
    return HPE_OK;
}

int hpe_subswarm_unique_id(unsigned char id_out[HPE_SUBSWARM_ID_BYTES]) {
    if (!id_out) return HPE_E_ARG;
    const RcclApi &api = rccl_api();
    if (!api.ok) return HPE_E_STATE;
    static_assert(sizeof(ncclUniqueId) == HPE_SUBSWARM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    if (api.get_unique_id(&id) != ncclSuccess) return HPE_E_HIP;
    std::memcpy(id_out, &id, sizeof(id));
    return HPE_OK;
}

int hpe_subswarm_fini(hpe_ctx *c) {
    if (!c) return HPE_E_ARG;
    if (!c->ss.transport()) return HPE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    drop_graphs(c);  // graphs holding the exchange go before the communicator / the script
    const ncclResult_t r = c->ss.comm ? rccl_api().comm_destroy(c->ss.comm) : ncclSuccess;
    c->ss.comm = nullptr;
    c->ss.d_script.reset();
    c->ss.d_script_k.reset();
    c->ss.script_frames = 0;
    c->ss.on = false;
    c->ss.nranks = 0;
    c->ss.d_gath.reset();
    ++c->epoch;  // the captured tracking graphs hold the exchange
    if (r != ncclSuccess) return fail(c, HPE_E_HIP, "ncclCommDestroy: %s", rccl_api().error_string(r));
    return HPE_OK;
}

int hpe_subswarm_init_scripted(hpe_ctx *c, int nranks, int rank, const double *script, int frames) {
    if (!c) return HPE_E_ARG;
    if (!script || nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks || frames < 1)
        return fail(c, HPE_E_ARG, "subswarm_init_scripted: null script, %d frames, or rank %d of "
                                  "%d outside [0, %d), world 1..64", frames, rank, nranks, nranks);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t rows = (size_t)nranks * (HPE_DOF + 1), n = (size_t)frames * rows;
    // a script of the live one's shape: new contents into the same buffers (the captured
    // graphs read them at replay); anything else is a new transport
    const bool same = c->ss.d_script && !c->ss.comm && c->ss.on && c->ss.nranks == nranks &&
                      c->ss.rank == rank && c->ss.script_frames == frames;
    if (same) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        int rc = hpe_subswarm_fini(c);
        if (rc) return rc;
        if (alloc_all(c->ss.d_gath, rows, c->ss.d_script, n, c->ss.d_script_k, 1) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, HPE_E_HIP, "subswarm_init_scripted: no device memory for %d frames", frames);
        }
        c->ss.script_frames = frames;
        c->ss.nranks = nranks;
        c->ss.rank = rank;
        c->ss.on = true;
        c->ss.graphs = true;
        c->ss.note[0] = 0;
        ++c->epoch;
    }
    HIPCHK(c, hipMemcpy(c->ss.d_script, script, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->ss.d_script_k, 0, sizeof(int)));  // rewound
    HIPCHK(c, hipMemset(c->ss.d_gath, 0xFF, sizeof(double) * rows));  // NaN
    return HPE_OK;
}

int hpe_subswarm_init(hpe_ctx *c, const unsigned char id[HPE_SUBSWARM_ID_BYTES], int nranks,
                      int rank) {
    if (!c) return HPE_E_ARG;
    if (!id || nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks)
        return fail(c, HPE_E_ARG, "subswarm_init: null id or rank %d of %d outside [0, %d), "
                                  "world 1..64", rank, nranks, nranks);
    const RcclApi &api = rccl_api();
    if (!api.ok) return fail(c, HPE_E_STATE, "%s", api.why);
    int rc = hpe_subswarm_fini(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->ss.d_gath.alloc((size_t)nranks * (HPE_DOF + 1)));
    HIPCHK(c, hipMemset(c->ss.d_gath, 0xFF, sizeof(double) * nranks * (HPE_DOF + 1)));  // NaN
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = api.comm_init_rank(&comm, nranks, uid, rank);
    if (r != ncclSuccess) {
        c->ss.d_gath.reset();
        return fail(c, HPE_E_HIP, "ncclCommInitRank(%d of %d): %s", rank, nranks, api.error_string(r));
    }
    c->ss.comm = comm;
    c->ss.nranks = nranks;
    c->ss.rank = rank;
    c->ss.on = true;
    c->ss.graphs = true;
    c->ss.note[0] = 0;
    ++c->epoch;
    // one all-gather now, outside any graph capture (every rank is here): RCCL sets up its
    // peer connections at a communicator's first collective; then the buffer back to NaN
    const ncclResult_t r1 = api.all_gather(c->d_state, c->ss.d_gath, HPE_DOF + 1, ncclFloat64,
                                           comm, c->stream);
    if (r1 != ncclSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)api.comm_destroy(comm);
        c->ss.comm = nullptr;
        c->ss.on = false;
        c->ss.nranks = 0;
        c->ss.d_gath.reset();
        return fail(c, HPE_E_HIP, "subswarm warm-up all-gather: %s", api.error_string(r1));
    }
    HIPCHK(c, hipMemsetAsync(c->ss.d_gath, 0xFF, sizeof(double) * nranks * (HPE_DOF + 1), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HPE_OK;
}

int hpe_subswarm_enable(hpe_ctx *c, int on) {
    if (!c) return HPE_E_ARG;
    if (on < 0 || on > 2) return fail(c, HPE_E_ARG, "subswarm_enable: mode %d not in 0..2", on);
    if (!c->ss.transport()) return fail(c, HPE_E_STATE, "hpe_subswarm_init not called");
    if (c->ss.on != (on != 0)) {
        c->ss.on = on != 0;
        ++c->epoch;  // the captured tracking graphs hold the exchange (or not)
    }
    if (on == 2) c->ss.graphs = false;  // direct launches while the exchange is on
    else if (on == 1 && !c->ss.note[0]) c->ss.graphs = true;  // unless a capture failed
    return HPE_OK;
}

int hpe_subswarm_info(hpe_ctx *c, int32_t *nranks, int32_t *rank, int32_t *version,
                      int32_t *in_graphs, double *gathered_out) {
    if (!c) return HPE_E_ARG;
    const bool set = c->ss.transport();
    if (in_graphs) *in_graphs = (set && c->ss.graphs) ? 1 : 0;
    if (nranks) *nranks = set ? c->ss.nranks : 0;
    if (rank) *rank = set ? c->ss.rank : 0;
    if (version) {
        *version = 0;
        const RcclApi &api = rccl_api();
        int v = 0;
        if (api.ok && api.get_version(&v) == ncclSuccess) *version = v;
    }
    if (gathered_out && set) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(gathered_out, c->ss.d_gath, sizeof(double) * c->ss.nranks * (HPE_DOF + 1),
                            hipMemcpyDeviceToHost));
    }
    return HPE_OK;
}

int hpe_set_refine_exact(hpe_ctx *c, int exact) {
    if (!c) return HPE_E_ARG;
    if (c->refine_exact != (exact != 0)) {
        c->refine_exact = exact != 0;
        c->mw_fits = -1;
        c->spec_fits = -1;
        ++c->epoch;  // the captured tracking graphs hold the other refine kernel
    }
    return HPE_OK;
}

int hpe_set_refine_spec(hpe_ctx *c, int on) {
    if (!c) return HPE_E_ARG;
    if (c->refine_spec != (on != 0)) {
        c->refine_spec = on != 0;
        ++c->epoch;  // the captured tracking graphs hold the other refine launch
    }
    return HPE_OK;
}

int hpe_get_refine_spec(const hpe_ctx *c) { return c && c->refine_spec ? 1 : 0; }

int hpe_get_refine_exact(const hpe_ctx *c) { return c && c->refine_exact ? 1 : 0; }

int hpe_graph_captures(const hpe_ctx *c, uint64_t *n) {
    if (!c || !n) return HPE_E_ARG;
    *n = c->captures;
    return HPE_OK;
}

int hpe_refine_init_pose(hpe_ctx *c, double x0[26], int32_t *evals_out) {
    if (!c) return HPE_E_ARG;
    if (!x0) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevObs o;
    int rc = need_frame(c, &o);
    if (rc) return rc;
    std::memcpy(c->h_pinned + 64, x0, sizeof(double) * HPE_DOF);
    HIPCHK(c, hipMemcpyAsync(c->d_state, c->h_pinned + 64, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice, c->stream));
    if ((rc = refine_launch(c, FrameIo{c->d_obs_active, o.n, c->d_state}, 1))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->d_state, sizeof(double) * HPE_DOF, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_pinned + 32, c->d_evals, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = mw_check(c))) return rc;
    std::memcpy(x0, c->h_pinned, sizeof(double) * HPE_DOF);
    if (evals_out) std::memcpy(evals_out, c->h_pinned + 32, sizeof(int));
    return HPE_OK;
}

int hpe_track_frame_dev(hpe_ctx *c, int P, int refine, double *d_state) {
    if (!c) return HPE_E_ARG;
    if (int erc = mw_check_async(c)) return erc;
    if (!d_state) return fail(c, HPE_E_ARG, "null device state");
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    int rc = check_P(c, P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->cur < 0 || c->cur >= (int)c->slots.size() || !c->slots[c->cur].valid)
        return fail(c, HPE_E_STATE, "no frame selected (hpe_set_frame / hpe_select_frame)");
    // host-side launch decisions need only a bound on n (no readback of a device-prepared
    // frame): the staged refine for clouds that fit LDS
    const FrameIo io{c->d_obs_active, c->slots[c->cur].n_max, d_state};
    // allocate everything the frame touches before any capture
    const int G = ensure_tracking(c, P, 0);
    if (G < 0) return G;
    GraphKey key = graph_key(P, G, refine, d_state);
    key.staged = io.n_max <= RF_STAGE_MAX;
    return run_graphed(c, c->graphs[hpe_ctx::GC_FRAME], key,
                       [&] { return track_frame(c, P, refine, io); });
}

int hpe_track_frame(hpe_ctx *c, int P, int refine, double x0[26], double *cost_out) {
    if (!c) return HPE_E_ARG;
    if (!x0) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(c->h_pinned + 64, x0, sizeof(double) * HPE_DOF);
    HIPCHK(c, hipMemcpyAsync(c->d_state, c->h_pinned + 64, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice, c->stream));
    int rc = hpe_track_frame_dev(c, P, refine, c->d_state);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->d_state, sizeof(double) * 27, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(x0, c->h_pinned, sizeof(double) * HPE_DOF);
    if (cost_out) *cost_out = c->h_pinned[26];
    return mw_check(c);
}

// ---------------------------------------------------------------- pipelined tracking
// The pipeline's buffers: two prepared-frame slots with clouds of `need` points, their
// descriptors, the raw staging (pinned and device) and the frame counter.
static int ensure_pipe(hpe_ctx *c, int need) {
    int rc = ensure_prep_scratch(c);
    if (rc) return rc;
    hpe_ctx::Pipe &pp = c->pipe;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (!pp.d_obs) {
        DevBuf<DevObs> obs;  // moved in last: a block that failed part way runs again in full
        HIPCHK(c, obs.alloc(2));
        HIPCHK(c, pp.d_info.alloc(2));
        HIPCHK(c, pp.d_raw.alloc(2 * npix));
        HIPCHK(c, c->pipe_copy.ensure(hipStreamNonBlocking));
        if (const char *u = std::getenv("HPE_PIPE_UPLOAD")) pp.zero_copy = u[0] != '1';
        HIPCHK(c, pp.d_seq.alloc(1));
        HIPCHK(c, pp.d_dtf2.alloc(2 * npix));
        HIPCHK(c, pp.d_split.alloc(4));
        HIPCHK(c, hipMemset(pp.d_split, 0, 4 * sizeof(int)));
        HIPCHK(c, pp.h_done.alloc(1, hipHostMallocMapped | hipHostMallocCoherent));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(c, pp.h_raw[k].alloc(npix, hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(c, pp.used[k].ensure(hipEventDisableTiming));
            HIPCHK(c, pp.raw_ready[k].ensure(hipEventDisableTiming));
        }
        pp.d_obs = std::move(obs);
    }
    for (int k = 0; k < 2; ++k) {
        Slot &f = pp.fr[k];
        if (f.cap < need) {  // a buffer about to go is no sequence's current frame
            ++c->epoch;
            pp.cur = -1;
        }
        HIPCHK(c, slot_buffers(f, need));
        f.valid = true;
        f.n_max = need;
        pp.used_valid[k] = false;
    }
    return HPE_OK;
}

int hpe_pipeline_begin(hpe_ctx *c, const float *depth_mm, int to_cm, int downsample, double focal) {
    if (!c) return HPE_E_ARG;
    if (!depth_mm || !(focal > 0)) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prep) HIPCHK(c, hipStreamSynchronize(c->prep));
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    int rc = ensure_pipe(c, downsample ? 250 : (int)npix);
    if (rc) return rc;
    hpe_ctx::Pipe &pp = c->pipe;
    pp.to_cm = to_cm ? 1 : 0;
    pp.downsample = downsample ? 1 : 0;
    pp.focal = focal;
    HIPCHK(c, hipMemsetAsync(pp.d_seq, 0, sizeof(unsigned long long), c->stream));
    __atomic_store_n(pp.h_done.get(), 0ull, __ATOMIC_RELEASE);
    pp.enq = 0;
    pp.used_seq[0] = pp.used_seq[1] = 0;
    // the first frame: prepared on the tracking stream
    std::memcpy(pp.h_raw[0], depth_mm, sizeof(float) * npix);
    HIPCHK(c, hipMemcpyAsync(pp.d_raw, pp.h_raw[0], sizeof(float) * npix, hipMemcpyHostToDevice, c->stream));
    const PrepArgs pa = prep_args(c, pp.fr[0], pp.d_raw, pp.to_cm, pp.downsample, focal, pp.d_obs,
                                  pp.d_info);
    hipLaunchKernelGGL(k_prepare, dim3(PREP_WG), dim3(PREP_NT), 0, c->stream, pa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    pp.cur = 0;
    c->cur = -1;  // the selected frame is the pipeline's
    return HPE_OK;
}

// A tracked frame in the pipeline's prepared buffer `cur` (the pipelined loop, a raw sequence):
// the kernels read that buffer's descriptor directly (a graph is per parity), and the final
// kernel hands it back to d_obs_active for the API's later calls.
static FrameIo pipe_frame_io(hpe_ctx *c, int cur, double *d_state, double *hist = nullptr) {
    FrameIo io{c->pipe.d_obs + cur, c->pipe.fr[cur].n_max, d_state, hist};
    io.hand_back = c->d_obs_active;
    return io;
}

// k frames of an offline sequence, one after the other on the tracking stream: each
// exactly hpe_track_frame_dev's launches, on the descriptor d_seq_obs that the previous
// frame's final kernel staged from the device cursor (k_seq_begin starts it), with the
// frame's {bestp, cost} stored to the history row the cursor names.  The launches depend
// on the frames only through n_max (the kernel forms), so one captured chunk graph serves
// every chunk of the same shape, whatever its slots.
static int enqueue_seq_chunk(hpe_ctx *c, int P, int refine, double *d_state, int slot0, int k,
                             double *hist) {
    DevPick pick{};  // the exchange's, from a frame to the next one's refine launch
    for (int i = 0; i < k; ++i) {
        // host-side launch decisions need only a bound on n
        FrameIo io{c->d_seq_obs, c->slots[slot0 + i].n_max, d_state, hist};
        io.hand_back = c->d_obs_active;  // each frame, for the API's later calls
        io.slots = c->d_obs;
        io.seq_obs = c->d_seq_obs;
        io.cur = c->d_seq_cur;
        io.defer_pick = refine && i + 1 < k;
        if (int rc = track_frame(c, P, refine, io, nullptr, nullptr, &pick)) return rc;
    }
    return HPE_OK;
}

int hpe_track_sequence_dev(hpe_ctx *c, int P, int refine, double *d_state, int first_slot,
                           int n, int frames_per_graph, double *d_hist) {
    if (!c) return HPE_E_ARG;
    int rc = check_chunked_call(c, P, frames_per_graph);
    if (rc) return rc;
    if (!d_state) return fail(c, HPE_E_ARG, "null device state");
    if (n < 1 || first_slot < 0 || first_slot + n > (int)c->slots.size())
        return fail(c, HPE_E_ARG, "frames [%d, %d) are not all stored slots", first_slot,
                    first_slot + n);
    for (int f = 0; f < n; ++f)
        if (!c->slots[first_slot + f].valid)
            return fail(c, HPE_E_ARG, "slot %d holds no frame", first_slot + f);
    HIPCHK(c, hipSetDevice(c->device));
    const int G = ensure_tracking(c, P, 0);
    if (G < 0) return G;
    // frames prepared on the preprocessing stream: the tracking stream waits for the ones
    // still running, once, before the first chunk (no markers between chunks)
    for (int f = 0; f < n; ++f) {
        Slot &s = c->slots[first_slot + f];
        if (s.dev && s.ready && hipEventQuery(s.ready) != hipSuccess)
            HIPCHK(c, hipStreamWaitEvent(c->stream, s.ready, 0));
    }
    const int K = frames_per_graph ? frames_per_graph : HPE_SEQ_CHUNK;
    // the device cursor: frame first_slot's descriptor staged, history row 0
    // (no profiling slot: it is not a k_pso_final dispatch)
    hipLaunchKernelGGL(k_seq_begin, dim3(1), dim3(64), 0, c->stream, (const DevObs *)c->d_obs,
                       first_slot, c->d_seq_obs, c->d_seq_cur);
    HIPCHK(c, hipGetLastError());
    double *hist = d_hist;  // rows advance with the cursor
    for (int f0 = 0; f0 < n; f0 += K) {
        const int k = n - f0 < K ? n - f0 : K, slot0 = first_slot + f0;
        GraphKey key = graph_key(P, G, refine, d_state, hist);
        key.k = k;
        for (int i = 0; i < k; ++i) {  // keyed by the chunk's shape, not its slots
            if (c->slots[slot0 + i].n_max <= RF_STAGE_MAX) key.staged |= 1u << i;
            if (c->slots[slot0 + i].n_max > HPE_NT / 2) key.filt |= 1u << i;
        }
        if ((rc = run_graphed(c, c->graphs[hpe_ctx::GC_SEQ], key, [&] {
                 return enqueue_seq_chunk(c, P, refine, d_state, slot0, k, hist);
             })))
            return rc;
    }
    // the last frame's descriptor is the selected one now (handed back by its final kernel)
    c->cur = first_slot + n - 1;
    return mark_seq_done(c);
}

// The kernel forms of one frame of B lanes: the axes of hpe_kernels.hip's lane templates, derived
// once from the frame's targets and the context.
struct LaneForm {
    bool hands;   // the HANDS forms: lane hands are set (the batch graphs' key field), or paced,
                  // or seeded
    bool seeds;   // hpe_set_batch_seeds: the SEEDS forms of the kernels that draw, in the HANDS
                  // shape alone (as the paced ones)
    LaneSrc src;  // the refine launch prepares every lane's next frame from there (NONE: no next)
    bool win;     // ... through the lanes' windows
    bool paced;   // HPE_PACING_FREE: the idle-aware forms, in the HANDS shape alone (the table
                  // holds the context's hand in every entry while no lane hands are set)
    bool live;    // the live batch: the final launch publishes the batch's frame number
    bool rigid;
    int wpp;      // HPE_BATCH_FORM_WAVE: waves per particle (0: the workgroup form)
    bool coop, r16, filt;
};
static int lane_hands_set(const hpe_ctx *c) { return c->lane_hands_B ? 1 : 0; }
static LaneForm lane_form(hpe_ctx *c, int P, int B, const DevSwarm &d, const LaneFrameIo &io) {
    LaneForm f{};
    f.paced = io.act != nullptr;
    f.seeds = !c->lane_seeds.empty();
    f.hands = f.paced || f.seeds || lane_hands_set(c);
    f.src = !io.prep ? LANE_SRC_NONE : io.unit ? (io.view ? LANE_SRC_VIEW : LANE_SRC_U16) : io.raw ? LANE_SRC_RAW : LANE_SRC_RING;
    f.win = io.prep && io.win;
    f.live = io.seq != nullptr;
    f.rigid = !c->refine_exact;
    f.wpp = batch_wave_wpp(c, P, B);
    f.coop = c->fk_coop;
    f.r16 = d.K <= 15;
    f.filt = io.filt;  // (every live cloud is bounded by 250 points: the non-FILT kernels)
    return f;
}

// One selector per role: the instantiations the host can reach and no others (WIN needs a source;
// PACED is the live batch's -- the ring, 16-bit or not, or through views -- in the HANDS shape and
// never FILT).
extern "C++" {
typedef void (*LaneRefineFn)(double *, const DevObs *, const DevHand *, int *, int, const PrepArgs *,
                             const DevWindow *, const int *, const float *, const float *const *,
                             const int *);
template <bool RIGID, bool HANDS, bool PACED>
static LaneRefineFn lane_refine_kernel_t(LaneSrc src, bool win) {
    switch (src) {
    case LANE_SRC_NONE:
        return k_refine_lane<RIGID, HANDS, LANE_SRC_NONE, false, PACED>;
    case LANE_SRC_RING:
        return win ? k_refine_lane<RIGID, HANDS, LANE_SRC_RING, true, PACED>
                   : k_refine_lane<RIGID, HANDS, LANE_SRC_RING, false, PACED>;
    case LANE_SRC_U16:
        return win ? k_refine_lane<RIGID, HANDS, LANE_SRC_U16, true, PACED>
                   : k_refine_lane<RIGID, HANDS, LANE_SRC_U16, false, PACED>;
    case LANE_SRC_VIEW:
        return win ? k_refine_lane<RIGID, HANDS, LANE_SRC_VIEW, true, PACED>
                   : k_refine_lane<RIGID, HANDS, LANE_SRC_VIEW, false, PACED>;
    case LANE_SRC_RAW:
        if constexpr (!PACED)
            return win ? k_refine_lane<RIGID, HANDS, LANE_SRC_RAW, true, false>
                       : k_refine_lane<RIGID, HANDS, LANE_SRC_RAW, false, false>;
    }
    return nullptr;  // a raw batch is never paced
}
static LaneRefineFn lane_refine_kernel(const LaneForm &f) {
    if (f.paced)
        return f.rigid ? lane_refine_kernel_t<true, true, true>(f.src, f.win)
                       : lane_refine_kernel_t<false, true, true>(f.src, f.win);
    if (f.hands)
        return f.rigid ? lane_refine_kernel_t<true, true, false>(f.src, f.win)
                       : lane_refine_kernel_t<false, true, false>(f.src, f.win);
    return f.rigid ? lane_refine_kernel_t<true, false, false>(f.src, f.win)
                   : lane_refine_kernel_t<false, false, false>(f.src, f.win);
}

// (the first frame's preparation: the batch calls' begins)
typedef void (*LanePrepareFn)(const PrepArgs *, const DevWindow *, const int *, const float *,
                              const float *const *, const int *);
template <LaneSrc SRC>
static LanePrepareFn lane_prepare_kernel_t(bool win, bool paced) {
    if constexpr (SRC != LANE_SRC_RAW)
        if (paced) return win ? k_prepare_lane<SRC, true, true> : k_prepare_lane<SRC, false, true>;
    return win ? k_prepare_lane<SRC, true, false> : k_prepare_lane<SRC, false, false>;
}
static LanePrepareFn lane_prepare_kernel(LaneSrc src, bool win, bool paced) {
    if (src == LANE_SRC_RAW) return lane_prepare_kernel_t<LANE_SRC_RAW>(win, false);
    if (src == LANE_SRC_VIEW) return lane_prepare_kernel_t<LANE_SRC_VIEW>(win, paced);
    return src == LANE_SRC_U16 ? lane_prepare_kernel_t<LANE_SRC_U16>(win, paced)
                               : lane_prepare_kernel_t<LANE_SRC_RING>(win, paced);
}

typedef void (*LaneWindowFn)(const double *, const DevHand *, const WinPar *, DevWindow *, const int *);
static LaneWindowFn lane_window_kernel(const LaneForm &f) {
    return f.paced ? k_window_b<true, true> : f.hands ? k_window_b<true, false> : k_window_b<false, false>;
}

// init: both forms have one argument list
typedef void (*LaneInitFn)(DevSwarm, size_t, const double *, const DevObs *, const DevHand *,
                           const int *, const LaneSeeds *);
template <bool HANDS, bool PACED, bool SEEDS = false>
static LaneInitFn lane_init_kernel_t(const LaneForm &f) {
    if (f.wpp == 2)
        return f.coop ? k_pso_init_wb<2, true, HANDS, PACED, SEEDS> : k_pso_init_wb<2, false, HANDS, PACED, SEEDS>;
    if (f.wpp)
        return f.coop ? k_pso_init_wb<1, true, HANDS, PACED, SEEDS> : k_pso_init_wb<1, false, HANDS, PACED, SEEDS>;
    if constexpr (!PACED)
        if (f.filt) return k_pso_init_b<true, HANDS, false, SEEDS>;
    return k_pso_init_b<false, HANDS, PACED, SEEDS>;
}
static LaneInitFn lane_init_kernel(const LaneForm &f) {
    if (f.seeds) return f.paced ? lane_init_kernel_t<true, true, true>(f) : lane_init_kernel_t<true, false, true>(f);
    return f.paced ? lane_init_kernel_t<true, true>(f)
                   : f.hands ? lane_init_kernel_t<true, false>(f) : lane_init_kernel_t<false, false>(f);
}

typedef void (*LaneGenFn)(DevSwarm, size_t, const DevObs *, const DevHand *, int, double, double,
                          double, InboxCounts, const int *, const LaneSeeds *);
template <bool HANDS, bool PACED, bool SEEDS = false>
static LaneGenFn lane_gen_kernel_t(const LaneForm &f) {
    if constexpr (!PACED)
        if (f.filt)
            return f.r16 ? k_pso_gen_b<true, true, HANDS, false, SEEDS> : k_pso_gen_b<false, true, HANDS, false, SEEDS>;
    return f.r16 ? k_pso_gen_b<true, false, HANDS, PACED, SEEDS> : k_pso_gen_b<false, false, HANDS, PACED, SEEDS>;
}
static LaneGenFn lane_gen_kernel(const LaneForm &f) {
    if (f.seeds) return f.paced ? lane_gen_kernel_t<true, true, true>(f) : lane_gen_kernel_t<true, false, true>(f);
    return f.paced ? lane_gen_kernel_t<true, true>(f)
                   : f.hands ? lane_gen_kernel_t<true, false>(f) : lane_gen_kernel_t<false, false>(f);
}

// the wave form's generation (no exchange, no inbox counts)
typedef void (*LaneWaveGenFn)(DevSwarm, size_t, const DevObs *, const DevHand *, int, double, double,
                              double, const int *, const LaneSeeds *);
template <int WPP, bool HANDS, bool PACED, bool SEEDS>
static LaneWaveGenFn lane_wave_gen_kernel_t(bool coop, bool r16) {
    return coop ? (r16 ? k_pso_gen_wb<true, WPP, true, HANDS, PACED, SEEDS> : k_pso_gen_wb<false, WPP, true, HANDS, PACED, SEEDS>)
                : (r16 ? k_pso_gen_wb<true, WPP, false, HANDS, PACED, SEEDS> : k_pso_gen_wb<false, WPP, false, HANDS, PACED, SEEDS>);
}
template <bool HANDS, bool PACED, bool SEEDS = false>
static LaneWaveGenFn lane_wave_gen_kernel_t(const LaneForm &f) {
    return f.wpp == 2 ? lane_wave_gen_kernel_t<2, HANDS, PACED, SEEDS>(f.coop, f.r16)
                      : lane_wave_gen_kernel_t<1, HANDS, PACED, SEEDS>(f.coop, f.r16);
}
static LaneWaveGenFn lane_wave_gen_kernel(const LaneForm &f) {
    if (f.seeds)
        return f.paced ? lane_wave_gen_kernel_t<true, true, true>(f) : lane_wave_gen_kernel_t<true, false, true>(f);
    return f.paced ? lane_wave_gen_kernel_t<true, true>(f)
                   : f.hands ? lane_wave_gen_kernel_t<true, false>(f)
                             : lane_wave_gen_kernel_t<false, false>(f);
}

typedef void (*LaneFinalFn)(DevSwarm, size_t, double *, DevObs *, const DevHand *, DevObs *, int,
                            unsigned long long *, unsigned long long *, double *, const int *,
                            const DevObs *, int *, const int *);
static LaneFinalFn lane_final_kernel(const LaneForm &f) {
    if (f.paced) return k_pso_final_b<false, true, true, true>;
    if (f.live) return f.hands ? k_pso_final_b<false, true, true, false> : k_pso_final_b<false, false, true, false>;
    if (f.hands) return f.filt ? k_pso_final_b<true, true, false, false> : k_pso_final_b<false, true, false, false>;
    return f.filt ? k_pso_final_b<true, false, false, false> : k_pso_final_b<false, false, false, false>;
}
}  // extern "C++"

// One tracked frame of B lanes, the frame every batch call enqueues: track_frame's launches with a
// lane dimension, each lane on its own descriptor io.obs[b], cursor io.cur[2 b] and arena b of the
// swarm (batch_swarm).  FOLLOW: first every lane's window from the pose its state holds now --
// the refine workgroup overwrites it -- into the parity being prepared.  The refine launch (the
// CU-filling LDS size puts the lanes on B CUs) is on grid (1, B), or with a next frame on
// (1 + PREP_WG, B): it then carries every lane's preparation, read through the raw cursor or from
// the pinned ring, as a raw sequence's and the pipelined loop's do (testmodel.cpp:126 + next_frame
// of the following iteration).  Then pso_evolve and cal_cost(bestp): launch_pso's workgroup form
// with the lane dimension -- init and the generations on (P, B) -- or, HPE_BATCH_FORM_WAVE, its
// wave form on (ceil(P / particles per workgroup), B) at pso_wpp(B * P) waves per particle, no
// inbox counts; the final kernel on (1, B), in the wave form with same_eval = 0: it evaluates
// cal_cost(bestp).  A free-paced batch (io.act) enqueues the same launches whatever the lanes'
// masks are: which lanes track and which prepare is decided on the device, by the words the call
// wrote on the stream before this graph.
static int track_lane_frame(hpe_ctx *c, int P, int refine, int B, double *d_states,
                            const LaneFrameIo &io) {
    const DevSwarm d = batch_swarm(c);
    const LaneForm f = lane_form(c, P, B, d, io);
    const DevObs *obs = io.obs;
    const DevHand *hand = c->d_lane_hands;  // the table: lane b's kernels read entry b
    const int *act = io.act;
    const bool prep = f.src != LANE_SRC_NONE;
    const LaneRefineFn kr = lane_refine_kernel(f);
    if (!kr) return fail(c, HPE_E_STATE, "a paced frame has no raw cursor");
    if (f.win && io.follow)
        hipLaunchKernelGGL(lane_window_kernel(f), dim3(B), dim3(64), 0, c->stream,
                           (const double *)d_states, hand, (const WinPar *)c->win.d_par, io.win, act);
    if (prep && io.clean)  // lane cleaning: the next frames, from the pinned ring to the staging
        hipLaunchKernelGGL(io.clean_view ? k_clean_b<true> : k_clean_b<false>,
                           dim3(CLEAN_TILES, B), dim3(CLEAN_NT), 0, c->stream, io.clean,
                           io.clean_par, io.clean_view, act);
    if (prep || refine)
        launch(c, HPE_PROF_REFINE, kr, dim3(prep ? 1 + PREP_WG : 1, B), dim3(RF_NT), RF_DYN_LDS,
               d_states, obs, hand, c->d_bevals.get(), refine ? 1 : 0, io.prep, (const DevWindow *)io.win,
               act, io.unit, io.raw, (const int *)io.cur);
    const size_t stride = c->sw.stride;
    const double W1 = 1. / (2 * std::log(2.0)), C1 = 0.5 + std::log(2.0), C2 = C1;  // PSO.cpp:772-774
    const int per_wg = f.wpp ? PW_WPB / f.wpp : 1;  // one or two waves per particle, or a workgroup
    const dim3 grid((P + per_wg - 1) / per_wg, B), block(f.wpp ? PW_NT : HPE_NT);
    // lane seeds: the lanes' table entry (null: every lane draws under the context's seed)
    const LaneSeeds *ls = f.seeds ? c->sw.lane_ls.get() : nullptr;
    launch(c, HPE_PROF_PSO_INIT, lane_init_kernel(f), grid, block, 0, d, stride,
           (const double *)d_states, obs, hand, act, ls);
    if (f.wpp) {
        const LaneWaveGenFn kw = lane_wave_gen_kernel(f);
        for (int g = 1; g <= d.G; ++g)
            launch(c, HPE_PROF_PSO_GEN, kw, grid, block, 0, d, stride, obs, hand, g, W1, C1, C2, act, ls);
    } else {
        // P > KIN_MAX: the kernel reads K slots; seeded: its lane's counts from the device table
        static const InboxCounts all_k{};
        const LaneGenFn kg = lane_gen_kernel(f);
        for (int g = 1; g <= d.G; ++g)
            launch(c, HPE_PROF_PSO_GEN, kg, grid, block, 0, d, stride, obs, hand, g, W1, C1, C2,
                   c->sw.kin.empty() || f.seeds ? all_k : c->sw.kin[g], act, ls);
    }
    launch(c, HPE_PROF_PSO_FINAL, lane_final_kernel(f), dim3(1, B), dim3(HPE_NT), 0, d, stride, d_states,
           io.obs, hand, (DevObs *)nullptr, f.wpp ? 0 : 1, io.seq, io.done_host, io.hist,
           (const int *)nullptr, io.slots, io.cur, act);
    // lane groups: every group's rows become its best own row, ahead of the reports and of the
    // next frame's windows and refine, which read the rows
    if (c->lane_groups_B)
        hipLaunchKernelGGL(k_group_pick, dim3(B), dim3(64), 0, c->stream, d_states, c->d_group_own.get(),
                           io.hist, (const int *)io.cur, (const LaneGroups *)c->d_lane_groups, act);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

int hpe_set_batch_form(hpe_ctx *c, int form) {
    if (!c) return HPE_E_ARG;
    if (form != HPE_BATCH_FORM_AUTO && form != HPE_BATCH_FORM_WAVE)
        return fail(c, HPE_E_ARG, "batch form %d is neither HPE_BATCH_FORM_AUTO nor _WAVE", form);
    // a live batch keeps the form it began with (every frame of a stream from one form, as in the
    // single loop it is checked against)
    if (c->live.cur >= 0 && form != c->batch_form)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the form it began with "
                    "(end it first)");
    c->batch_form = form;  // no epoch bump: the batch graphs are keyed by the form (GraphKey::wave)
    return HPE_OK;
}

int hpe_set_batch_pacing(hpe_ctx *c, int mode) {
    if (!c) return HPE_E_ARG;
    if (mode != HPE_PACING_LOCKSTEP && mode != HPE_PACING_FREE)
        return fail(c, HPE_E_ARG, "batch pacing %d is neither HPE_PACING_LOCKSTEP nor _FREE", mode);
    // read at the begin: a live batch keeps the pacing it began with
    if (c->live.cur >= 0 && mode != c->live.pacing)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the pacing it began "
                    "with (end it first)");
    c->batch_pacing = mode;  // no epoch bump: the live graphs are keyed by it (GraphKey::pacing)
    return HPE_OK;
}

int hpe_batch_pending(hpe_ctx *c, uint32_t *mask_out) {
    if (!c) return HPE_E_ARG;
    if (!mask_out) return fail(c, HPE_E_ARG, "null mask");
    if (c->live.cur < 0)
        return fail(c, HPE_E_STATE, "no live batch: hpe_batch_pipeline_begin not called, or the "
                    "batch ended");
    *mask_out = c->live.pending;
    return HPE_OK;
}

int hpe_set_batch_window(hpe_ctx *c, int mode, int B, const hpe_window *init, double margin_xy,
                         double margin_z) {
    if (!c) return HPE_E_ARG;
    if (mode != HPE_WINDOW_OFF && mode != HPE_WINDOW_FIXED && mode != HPE_WINDOW_FOLLOW)
        return fail(c, HPE_E_ARG, "window mode %d is none of HPE_WINDOW_OFF, _FIXED, _FOLLOW", mode);
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "windows for %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (mode != HPE_WINDOW_OFF && !init) return fail(c, HPE_E_ARG, "null init windows");
    if (!(margin_xy >= 0) || !(margin_z >= 0) || std::isinf(margin_xy) || std::isinf(margin_z))
        return fail(c, HPE_E_ARG, "margins %g, %g: negative or not finite", margin_xy, margin_z);
    if (c->live.cur >= 0)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the windows it began "
                    "with (end it first)");
    hpe_ctx::LaneWin &w = c->win;
    w.mode = mode;  // no epoch bump: the batch graphs are keyed by the mode (GraphKey::win)
    w.B = B;
    w.margin_xy = margin_xy;
    w.margin_z = margin_z;
    w.init.clear();
    if (mode != HPE_WINDOW_OFF)
        for (int b = 0; b < B; ++b)
            w.init.push_back(DevWindow{init[b].row_lo, init[b].row_hi, init[b].col_lo,
                                       init[b].col_hi, init[b].z_lo, init[b].z_hi, 0.f, 0.f, {0, 0}});
    return HPE_OK;
}

// A batch call's or begin's lane count against the windows' (no windows: any).
static int check_window_lanes(hpe_ctx *c, int B) {
    if (c->win.mode != HPE_WINDOW_OFF && B != c->win.B)
        return fail(c, HPE_E_ARG, "%d lanes, the windows were set for %d (hpe_set_batch_window)", B,
                    c->win.B);
    return HPE_OK;
}

// Frame 0 of a windowed batch: init into both parities of the window table, the margins and
// the call's focal and unit conversion beside it; every entry with its depth bounds in raw units
// (win_raw_bounds).  The stream drains first: launches in flight read the table, and under
// FOLLOW they write it.  (ensure_raw_batch allocated the table.)
static int write_windows(hpe_ctx *c, double focal, int to_cm) {
    hpe_ctx::LaneWin &w = c->win;
    if (w.mode == HPE_WINDOW_OFF) return HPE_OK;
    DevWindow tab[2 * HPE_BATCH_MAX] = {};
    for (int p = 0; p < 2; ++p)
        for (int b = 0; b < w.B; ++b) {
            DevWindow &e = tab[p * HPE_BATCH_MAX + b];
            e = w.init[b];
            win_raw_bounds(e, to_cm);
        }
    const WinPar par{w.margin_xy, w.margin_z, focal, to_cm, 0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(w.d_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(w.d_par, &par, sizeof(par), hipMemcpyHostToDevice));
    return HPE_OK;
}

// The pose rule for one host pose under one device hand: hpe_window_from_pose (the context's
// hand) and hpe_lane_window_from_pose (a lane's entry of the table).
static int window_from_pose(hpe_ctx *c, const DevHand *hand, const double *theta, double focal,
                            double margin_xy, double margin_z, hpe_window *out) {
    if (!theta || !out) return fail(c, HPE_E_ARG, "null pose or window");
    if (!(focal > 0)) return fail(c, HPE_E_ARG, "focal %g is not positive", focal);
    if (!(margin_xy >= 0) || !(margin_z >= 0) || std::isinf(margin_xy) || std::isinf(margin_z))
        return fail(c, HPE_E_ARG, "margins %g, %g: negative or not finite", margin_xy, margin_z);
    HIPCHK(c, hipSetDevice(c->device));
    hpe_ctx::LaneWin &w = c->win;
    if (!w.d_one) HIPCHK(c, alloc_all(w.d_one_state, (size_t)HPE_STATE_N, w.d_one_par, 1, w.d_one, 1));
    const WinPar par{margin_xy, margin_z, focal, 1, 0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(w.d_one_state, theta, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(w.d_one_par, &par, sizeof(par), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_window_b<false, false>), dim3(1), dim3(64), 0, c->stream,
                       (const double *)w.d_one_state, hand, (const WinPar *)w.d_one_par, w.d_one,
                       (const int *)nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevWindow r;
    HIPCHK(c, hipMemcpy(&r, w.d_one, sizeof(r), hipMemcpyDeviceToHost));
    *out = hpe_window{r.row_lo, r.row_hi, r.col_lo, r.col_hi, r.z_lo, r.z_hi};
    return HPE_OK;
}

int hpe_window_from_pose(hpe_ctx *c, const double *theta, double focal, double margin_xy,
                         double margin_z, hpe_window *out) {
    if (!c) return HPE_E_ARG;
    return window_from_pose(c, c->d_hand, theta, focal, margin_xy, margin_z, out);
}

int hpe_lane_window_from_pose(hpe_ctx *c, int lane, const double *theta, double focal,
                              double margin_xy, double margin_z, hpe_window *out) {
    if (!c) return HPE_E_ARG;
    if (lane < 0 || lane >= HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "lane %d out of range [0, %d]", lane, HPE_BATCH_MAX - 1);
    return window_from_pose(c, c->d_lane_hands + lane, theta, focal, margin_xy, margin_z, out);
}

int hpe_set_batch_hands(hpe_ctx *c, int B, const hpe_hand_params *hands) {
    if (!c) return HPE_E_ARG;
    if (hands) {
        if (B < 1 || B > HPE_BATCH_MAX)
            return fail(c, HPE_E_ARG, "hands for %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
        for (int b = 0; b < B; ++b) {
            if (!hand_counts_ok(hands[b]))
                return fail(c, HPE_E_ARG, "lane %d: sphere counts are not tb {2,2,2,2}, fg {4,2,2,2}", b);
            if (!hand_values_finite(hands[b]))
                return fail(c, HPE_E_ARG, "lane %d: a hand parameter is not finite", b);
        }
    }
    if (c->live.cur >= 0)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the hands it began with "
                    "(end it first)");
    // lanes past B keep the context's hand: no batch call reads them while B is set
    std::vector<DevHand> tab(HPE_BATCH_MAX, c->hand);
    for (int b = 0; hands && b < B; ++b) hpe::build_dev_hand(hands[b], tab[b]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight read the table
    HIPCHK(c, hipMemcpy(c->d_lane_hands, tab.data(), sizeof(DevHand) * tab.size(),
                        hipMemcpyHostToDevice));
    c->lane_hands_B = hands ? B : 0;  // no epoch bump: the graphs hold the table's address and
                                      // key whether hands are set (GraphKey::hands)
    return HPE_OK;
}

// A batch call's or begin's lane count against the lane hands' (no lane hands: any).
static int check_hand_lanes(hpe_ctx *c, int B) {
    if (c->lane_hands_B && B != c->lane_hands_B)
        return fail(c, HPE_E_ARG, "%d lanes, the hands were set for %d (hpe_set_batch_hands)", B,
                    c->lane_hands_B);
    return HPE_OK;
}

// ---------------------------------------------------------------- lane seeds and groups
int hpe_set_batch_seeds(hpe_ctx *c, int B, const uint64_t *seeds) {
    if (!c) return HPE_E_ARG;
    if (seeds && (B < 1 || B > HPE_BATCH_MAX))
        return fail(c, HPE_E_ARG, "seeds for %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (c->live.cur >= 0)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the seeds it began with "
                    "(end it first)");
    // the tables follow at the next batch call, for its (P, G): ensure_lane_seeds.  No epoch bump:
    // the graphs hold the tables' addresses and key whether seeds are set (GraphKey::seeds)
    if (seeds) c->lane_seeds.assign(seeds, seeds + B);
    else c->lane_seeds.clear();
    return HPE_OK;
}

int hpe_set_batch_groups(hpe_ctx *c, int B, int n_groups, const int32_t *sizes) {
    if (!c) return HPE_E_ARG;
    const bool on = n_groups != 0 && sizes;
    LaneGroups g{};
    if (on) {
        if (B < 1 || B > HPE_BATCH_MAX)
            return fail(c, HPE_E_ARG, "groups over %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
        if (n_groups < 0 || n_groups > B)
            return fail(c, HPE_E_ARG, "%d groups over %d lanes", n_groups, B);
        int at = 0;
        for (int k = 0; k < n_groups; ++k) {
            if (sizes[k] < 1 || sizes[k] > B - at)
                return fail(c, HPE_E_ARG, "group %d: size %d is not positive, or the sizes pass %d "
                            "lanes", k, (int)sizes[k], B);
            for (int m = 0; m < sizes[k]; ++m) g.first[at + m] = at, g.size[at + m] = sizes[k];
            at += sizes[k];
        }
        if (at != B) return fail(c, HPE_E_ARG, "the group sizes sum to %d, not to %d lanes", at, B);
    }
    if (c->live.cur >= 0)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the groups it began "
                    "with (end it first)");
    if (on) {
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->d_group_own) {  // once, never reallocated: the graphs hold both addresses
            DevBuf<LaneGroups> tab;
            HIPCHK(c, tab.alloc(1));
            HIPCHK(c, c->d_group_own.alloc((size_t)HPE_BATCH_MAX * HPE_STATE_N));
            c->d_lane_groups = std::move(tab);
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight read the table
        HIPCHK(c, hipMemcpy(c->d_lane_groups, &g, sizeof(g), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemset(c->d_group_own, 0, sizeof(double) * HPE_BATCH_MAX * HPE_STATE_N));
    }
    c->lane_groups = g;
    c->lane_groups_B = on ? B : 0;  // no epoch bump: GraphKey::groups
    c->group_rows = false;
    return HPE_OK;
}

// A batch call's or begin's lane count against the lane seeds' and groups' (none set: any).
static int check_seed_group_lanes(hpe_ctx *c, int B) {
    if (!c->lane_seeds.empty() && B != (int)c->lane_seeds.size())
        return fail(c, HPE_E_ARG, "%d lanes, the seeds were set for %d (hpe_set_batch_seeds)", B,
                    (int)c->lane_seeds.size());
    if (c->lane_groups_B && B != c->lane_groups_B)
        return fail(c, HPE_E_ARG, "%d lanes, the groups were set for %d (hpe_set_batch_groups)", B,
                    c->lane_groups_B);
    return HPE_OK;
}

// Free pacing: a group advances as one -- the entries of a group's lanes (bit b of `given`) are
// all null or all non-null.
static int check_group_frames(hpe_ctx *c, int B, uint32_t given) {
    for (int b = 0; c->lane_groups_B && b < B; ++b)
        if ((given >> b & 1) != (given >> c->lane_groups.first[b] & 1))
            return fail(c, HPE_E_ARG, "lane %d: a frame for some lanes of its group only (a group "
                        "advances as one)", b);
    return HPE_OK;
}

int hpe_batch_group_pick(hpe_ctx *c, int B, double *d_states) {
    if (!c) return HPE_E_ARG;
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (!d_states) return fail(c, HPE_E_ARG, "null device states");
    if (!c->lane_groups_B) return fail(c, HPE_E_STATE, "no lane groups are set (hpe_set_batch_groups)");
    if (int rc = check_seed_group_lanes(c, B)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_group_pick, dim3(B), dim3(64), 0, c->stream, d_states, (double *)nullptr,
                       (double *)nullptr, (const int *)nullptr, (const LaneGroups *)c->d_lane_groups,
                       (const int *)nullptr);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

int hpe_batch_group_rows(hpe_ctx *c, int B, double *rows_out) {
    if (!c) return HPE_E_ARG;
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (!rows_out) return fail(c, HPE_E_ARG, "null rows");
    if (!c->lane_groups_B || !c->group_rows)
        return fail(c, HPE_E_STATE, "no grouped frame has been tracked (hpe_set_batch_groups)");
    if (B != c->lane_groups_B)
        return fail(c, HPE_E_ARG, "%d lanes, the groups were set for %d (hpe_set_batch_groups)", B,
                    c->lane_groups_B);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(rows_out, c->d_group_own, sizeof(double) * (size_t)B * HPE_STATE_N,
                        hipMemcpyDeviceToHost));
    return HPE_OK;
}

int hpe_batch_windows_readback(hpe_ctx *c, int parity, int B, hpe_window *out) {
    if (!c) return HPE_E_ARG;
    if (parity < 0 || parity > 1) return fail(c, HPE_E_ARG, "buffer parity %d", parity);
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "windows of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (!out) return fail(c, HPE_E_ARG, "null windows");
    if (!c->rb.d_obs)  // (the table is allocated with the raw batch's)
        return fail(c, HPE_E_STATE, "no window table: no raw or live batch has run yet");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevWindow tab[HPE_BATCH_MAX];
    HIPCHK(c, hipMemcpy(tab, c->win.d_tab + parity * HPE_BATCH_MAX, sizeof(DevWindow) * B,
                        hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        out[b] = hpe_window{tab[b].row_lo, tab[b].row_hi, tab[b].col_lo, tab[b].col_hi, tab[b].z_lo,
                            tab[b].z_hi};
    return HPE_OK;
}

int hpe_batch_wave_wpp(hpe_ctx *c, int P, int B) {
    if (!c) return HPE_E_ARG;
    if (int rc = check_P(c, P)) return rc;
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    return pso_wpp(c, B * P);
}

int hpe_track_batch_dev(hpe_ctx *c, int P, int refine, int B, double *d_states,
                        const int32_t *first_slots, int n, int frames_per_graph, double *d_hist) {
    if (!c) return HPE_E_ARG;
    int rc = check_chunked_call(c, P, frames_per_graph);
    if (rc || (rc = check_batch_call(c, P, B)) || (rc = check_hand_lanes(c, B)) ||
        (rc = check_seed_group_lanes(c, B)))
        return rc;
    if (!d_states || !first_slots) return fail(c, HPE_E_ARG, "null device states or first slots");
    if (n < 1) return fail(c, HPE_E_ARG, "n = %d frames", n);
    for (int b = 0; b < B; ++b) {
        const int s0 = first_slots[b];
        if (s0 < 0 || (long long)s0 + n > (long long)c->slots.size())
            return fail(c, HPE_E_ARG, "lane %d: frames [%d, %lld) are not all stored slots", b, s0,
                        (long long)s0 + n);
        for (int f = 0; f < n; ++f) {
            const Slot &s = c->slots[s0 + f];
            if (!s.valid) return fail(c, HPE_E_ARG, "lane %d: slot %d holds no frame", b, s0 + f);
            if (s.n_max > RF_STAGE_MAX)
                return fail(c, HPE_E_ARG, "lane %d: slot %d holds up to %d points, a batch takes the "
                            "single-workgroup refine (<= %d)", b, s0 + f, s.n_max, RF_STAGE_MAX);
            if ((s.n_max > HPE_NT / 2) != (c->slots[first_slots[0] + f].n_max > HPE_NT / 2))
                return fail(c, HPE_E_ARG, "frame %d: lanes 0 and %d disagree on clouds above %d "
                            "points (one kernel form per launch)", f, b, HPE_NT / 2);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int G = ensure_tracking(c, P, B);
    if (G < 0) return G;
    // frames prepared on the preprocessing stream: the tracking stream waits for the ones
    // still running, once, before the first chunk
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < n; ++f) {
            Slot &s = c->slots[first_slots[b] + f];
            if (s.dev && s.ready && hipEventQuery(s.ready) != hipSuccess)
                HIPCHK(c, hipStreamWaitEvent(c->stream, s.ready, 0));
        }
    BatchFirst first{};
    for (int b = 0; b < B; ++b) first.slot[b] = first_slots[b];
    hipLaunchKernelGGL(k_seq_begin_b, dim3(1, B), dim3(64), 0, c->stream, (const DevObs *)c->d_obs,
                       first, n, c->d_bobs, c->d_bcur);
    HIPCHK(c, hipGetLastError());
    const int K = frames_per_graph ? frames_per_graph : HPE_SEQ_CHUNK;
    for (int f0 = 0; f0 < n; f0 += K) {
        const int k = n - f0 < K ? n - f0 : K;
        GraphKey key = graph_key(P, G, refine, d_states, d_hist);  // the shape, not the slots
        key.k = k;
        key.B = B;
        key.wave = batch_wave_wpp(c, P, B);
        key.hands = lane_hands_set(c);
        key.seeds = !c->lane_seeds.empty();
        key.groups = c->lane_groups_B ? 1 : 0;
        for (int i = 0; i < k; ++i)
            if (c->slots[first_slots[0] + f0 + i].n_max > HPE_NT / 2) key.filt |= 1u << i;
        // k frames of B lanes, one after the other on the tracking stream: each lane on its own
        // descriptor d_bobs[b] and cursor d_bcur[2 b], its next frame staged from the slot table
        if ((rc = run_graphed(c, c->graphs[hpe_ctx::GC_BATCH], key, [&] {
                 int erc = HPE_OK;
                 for (int i = 0; i < k && !erc; ++i) {
                     const bool filt = (key.filt >> i) & 1u;
                     erc = track_lane_frame(c, P, refine, B, d_states,
                                            LaneFrameIo{c->d_bobs, filt, d_hist, c->d_obs, c->d_bcur});
                 }
                 return erc;
             })))
            return rc;
        if (c->lane_groups_B) c->group_rows = true;
    }
    return mark_seq_done(c);
}

// Host wait for pipelined frame n (1-based) to have run its final kernel, by polling the
// pinned word p (the single pipeline's or the live batch's h_done) that the kernel stores with
// system scope; bounded (~20 s), false on timeout.
static bool wait_frame_done(const volatile unsigned long long *p, unsigned long long n) {
    if (__atomic_load_n(p, __ATOMIC_ACQUIRE) >= n) return true;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (__atomic_load_n(p, __ATOMIC_ACQUIRE) >= n) return true;
        if ((it & 1023) == 1023) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return false;
            std::this_thread::yield();
        }
    }
}

int hpe_track_pipelined(hpe_ctx *c, int P, int refine, double *d_state, const float *next_depth_mm) {
    if (!c) return HPE_E_ARG;
    if (int erc = mw_check_async(c)) return erc;
    if (!d_state) return fail(c, HPE_E_ARG, "null device state");
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    hpe_ctx::Pipe &pp = c->pipe;
    if (pp.cur < 0) return fail(c, HPE_E_STATE, "hpe_pipeline_begin not called");
    int rc = check_P(c, P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int cur = pp.cur, nxt = cur ^ 1, next = next_depth_mm ? 1 : 0;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (next) {  // the pinned and device buffers' previous frame (two ago) must be done
        if (pp.zero_copy) {
            if (pp.used_seq[nxt] && !wait_frame_done(pp.h_done, pp.used_seq[nxt]))
                return fail(c, HPE_E_HIP, "pipelined frame %llu did not complete",
                            (unsigned long long)pp.used_seq[nxt]);
        } else if (pp.used_valid[nxt]) {
            HIPCHK(c, hipEventSynchronize(pp.used[nxt]));
        }
        std::memcpy(pp.h_raw[nxt], next_depth_mm, sizeof(float) * npix);
        if (!pp.zero_copy) {  // SDMA upload, overlapping the frame still running
            HIPCHK(c, hipMemcpyAsync(pp.d_raw + nxt * npix, pp.h_raw[nxt], sizeof(float) * npix,
                                     hipMemcpyHostToDevice, c->pipe_copy));
            HIPCHK(c, hipEventRecord(pp.raw_ready[nxt], c->pipe_copy));
            HIPCHK(c, hipStreamWaitEvent(c->stream, pp.raw_ready[nxt], 0));
        }
    }
    const int G = ensure_tracking(c, P, 0);
    if (G < 0) return G;
    GraphKey key = graph_key(P, G, refine, d_state);
    key.staged = pp.fr[cur].n_max <= RF_STAGE_MAX;
    key.next = next;
    key.cur = cur;
    FrameIo io = pipe_frame_io(c, cur, d_state);
    if (pp.zero_copy) {  // the final kernel publishes the frame's number
        io.seq = pp.d_seq;
        io.done_host = pp.h_done.dev();
    }
    // the next raw frame: in its pinned host buffer (zero copy) or uploaded to d_raw[nxt]
    const float *raw = pp.zero_copy ? pp.h_raw[nxt].dev() : pp.d_raw + nxt * npix;
    const PrepArgs pa = prep_args(c, pp.fr[nxt], raw, pp.to_cm, pp.downsample, pp.focal,
                                  pp.d_obs + nxt, pp.d_info + nxt);
    rc = run_graphed(c, c->graphs[hpe_ctx::GC_PIPE], key,
                     [&] { return track_frame(c, P, refine, io, next ? &pa : nullptr); });
    if (rc) return rc;
    ++pp.enq;  // this frame's number; its final kernel publishes it to h_done
    if (next) {
        if (pp.zero_copy) {
            pp.used_seq[nxt] = pp.enq;  // its refine launch reads h_raw[nxt]
        } else {
            HIPCHK(c, hipEventRecord(pp.used[nxt], c->stream));
            pp.used_valid[nxt] = true;
        }
        pp.cur = nxt;
    } else {
        pp.cur = -1;  // the sequence ended
    }
    return HPE_OK;
}

// k frames of a resident raw sequence, the first in prepared buffer `parity`: each exactly a
// pipelined frame -- refine with the next raw frame's preparation in the same launch (read
// through the row cursor: raw + (row + 1) frames), pso_evolve, cal_cost(bestp) -- with its
// {bestp, cost} stored to the history row the cursor names.  The launches depend on the
// chunk only through its shape (k, parity, whether its last frame prepares another).
static int enqueue_raw_chunk(hpe_ctx *c, int P, int refine, double *d_state, const float *raw,
                             int parity, int k, bool tail_next, double *hist) {
    hpe_ctx::Pipe &pp = c->pipe;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    DevPick pick{};  // the exchange's, from a frame to the next one's refine launch
    for (int i = 0; i < k; ++i) {
        const int cur = (parity + i) & 1, nxt = cur ^ 1;
        const bool next = i + 1 < k || tail_next;
        PrepArgs pa = prep_args(c, pp.fr[nxt], raw, pp.to_cm, pp.downsample, pp.focal,
                                pp.d_obs + nxt, pp.d_info + nxt);
        pa.raw_row = c->d_seq_cur + 1;
        pa.raw_stride = npix;
        // the split transform: this launch scans the next frame backward from the forward
        // values the previous launch (or the prologue) left in that frame's parity, and the
        // frame after it (if the sequence has one: a device word, not the graph) forward
        PrepSplit ps{};
        if (c->prep_split) {
            pa.dtf = pp.d_dtf2 + nxt * npix;
            ps.dtf_next = pp.d_dtf2 + cur * npix;
            ps.r0 = pp.d_split + nxt;
            ps.r0_next = pp.d_split + cur;
            ps.seq_n = pp.d_split + 2;
        }
        FrameIo io = pipe_frame_io(c, cur, d_state, hist);
        io.cur = c->d_seq_cur;  // the row cursor alone
        io.defer_pick = refine && i + 1 < k;
        if (int rc = track_frame(c, P, refine, io, next ? &pa : nullptr, &ps, &pick)) return rc;
    }
    return HPE_OK;
}

int hpe_track_raw_sequence_dev(hpe_ctx *c, int P, int refine, double *d_state,
                               const float *d_raw_mm, int n, int to_cm, int downsample,
                               double focal, int frames_per_graph, double *d_hist) {
    if (!c) return HPE_E_ARG;
    int rc = check_chunked_call(c, P, frames_per_graph);
    if (rc) return rc;
    if (!d_state || !d_raw_mm || n < 1 || !(focal > 0)) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    const int need = downsample ? 250 : (int)npix;
    hpe_ctx::Pipe &pp = c->pipe;
    // the preparation scratch is shared with hpe_prepare_frame's stream; a reallocation
    // needs every earlier reader of the frame buffers done
    if (c->prep) HIPCHK(c, hipStreamSynchronize(c->prep));
    if (!pp.d_obs || pp.fr[0].cap < need || pp.fr[1].cap < need)
        HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_pipe(c, need))) return rc;
    pp.to_cm = to_cm ? 1 : 0;
    pp.downsample = downsample ? 1 : 0;
    pp.focal = focal;
    pp.cur = -1;  // a pipelined sequence in progress ends here
    const int G = ensure_tracking(c, P, 0);
    if (G < 0) return G;
    // frame 0 prepared on the tracking stream, the row cursor at 0
    HIPCHK(c, hipMemsetAsync(c->d_seq_cur, 0, 2 * sizeof(int), c->stream));
    PrepArgs p0 = prep_args(c, pp.fr[0], d_raw_mm, pp.to_cm, pp.downsample, focal, pp.d_obs,
                            pp.d_info);
    if (c->prep_split) {  // + the sequence length and frame 1's forward scan (parity 1)
        p0.raw_stride = npix;
        PrepSplit s0{};
        s0.dtf_next = pp.d_dtf2 + npix;
        s0.r0_next = pp.d_split + 1;
        s0.seq_n = pp.d_split + 2;
        hipLaunchKernelGGL(k_prepare_seq, dim3(PREP_WG + 1), dim3(PREP_NT), 0, c->stream, p0, s0, n);
    } else {
        hipLaunchKernelGGL(k_prepare, dim3(PREP_WG), dim3(PREP_NT), 0, c->stream, p0);
    }
    HIPCHK(c, hipGetLastError());
    const int K = frames_per_graph ? frames_per_graph : HPE_SEQ_CHUNK;
    const int staged = pp.fr[0].n_max <= RF_STAGE_MAX;
    for (int f0 = 0; f0 < n; f0 += K) {
        const int k = n - f0 < K ? n - f0 : K, parity = f0 & 1, tail_next = f0 + k < n;
        GraphKey key = graph_key(P, G, refine, d_state, d_hist);
        key.k = k;
        key.parity = parity;
        key.tail_next = tail_next;
        key.staged = staged;
        key.to_cm = pp.to_cm;
        key.downsample = pp.downsample;
        key.focal = focal;
        key.in = d_raw_mm;
        if ((rc = run_graphed(c, c->graphs[hpe_ctx::GC_RAW], key, [&] {
                 return enqueue_raw_chunk(c, P, refine, d_state, d_raw_mm, parity, k, tail_next, d_hist);
             })))
            return rc;
    }
    // the last frame's descriptor is the selected one now (handed back by its final kernel)
    c->cur = -1;
    return mark_seq_done(c);
}

int hpe_pipe_readback(hpe_ctx *c, int parity, double *depth_cm, float *dt, double *cloud,
                      int32_t *n_out, double *scale_out, double *dtmax_out) {
    if (!c) return HPE_E_ARG;
    hpe_ctx::Pipe &pp = c->pipe;
    if (parity < 0 || parity > 1 || !pp.d_obs || !pp.fr[parity].depth)
        return fail(c, HPE_E_ARG, "pipeline buffer %d holds no frame", parity);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const Slot &s = pp.fr[parity];
    PrepInfo pi;
    HIPCHK(c, hipMemcpy(&pi, pp.d_info + parity, sizeof(pi), hipMemcpyDeviceToHost));
    if (pi.n < 0 || pi.n > s.cap) return fail(c, HPE_E_STATE, "pipeline buffer %d: n = %d", parity, pi.n);
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (depth_cm) HIPCHK(c, hipMemcpy(depth_cm, s.depth, sizeof(double) * npix, hipMemcpyDeviceToHost));
    if (dt) HIPCHK(c, hipMemcpy(dt, s.dt, sizeof(float) * npix, hipMemcpyDeviceToHost));
    if (cloud && pi.n > 0) {
        const size_t n = (size_t)pi.n;
        std::vector<double> soa(3 * n);
        HIPCHK(c, hipMemcpy(soa.data(), s.cx, sizeof(double) * n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(soa.data() + n, s.cy, sizeof(double) * n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(soa.data() + 2 * n, s.cz, sizeof(double) * n, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < n; ++p)
            for (int q = 0; q < 3; ++q) cloud[3 * p + q] = soa[(size_t)q * n + p];
    }
    if (n_out) *n_out = pi.n;
    if (scale_out) *scale_out = pi.scale;
    if (dtmax_out) *dtmax_out = pi.dtmax;
    return HPE_OK;
}

// The raw batch's buffers for B lanes prepared with (to_cm, focal): the fixed tables once, an
// arena per new lane, and the PrepArgs table rewritten when a lane is added or the preparation
// parameters change (after the stream has drained: launches in flight read it).
static int ensure_raw_batch(hpe_ctx *c, int B, int to_cm, double focal) {
    hpe_ctx::RawBatch &rb = c->rb;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W, M = HPE_BATCH_MAX;
    if (!rb.d_obs) {
        DevBuf<DevObs> obs;  // moved in last: a block that failed part way runs again in full
        HIPCHK(c, obs.alloc(2 * M));
        HIPCHK(c, rb.d_info.alloc(2 * M));
        HIPCHK(c, rb.d_tab.alloc(2 * M));
        HIPCHK(c, rb.d_ctr.alloc(32 * M));
        HIPCHK(c, hipMemset(rb.d_ctr, 0, sizeof(unsigned) * 32 * M));
        HIPCHK(c, rb.d_raw.alloc(M));
        HIPCHK(c, rb.d_cur.alloc(2 * M));
        // the lane windows' table, by [parity][lane] like d_tab, and their parameters; until a
        // windowed call writes them, whole-frame windows
        HIPCHK(c, c->win.d_tab.alloc(2 * M));
        HIPCHK(c, c->win.d_par.alloc(1));
        std::vector<DevWindow> whole(2 * M, DevWindow{0, HPE_IMG_H - 1, 0, HPE_IMG_W - 1, -HUGE_VAL,
                                                      HUGE_VAL, -HUGE_VALF, HUGE_VALF, {0, 0}});
        HIPCHK(c, hipMemcpy(c->win.d_tab, whole.data(), sizeof(DevWindow) * whole.size(),
                            hipMemcpyHostToDevice));
        HIPCHK(c, hipMemset(c->win.d_par, 0, sizeof(WinPar)));
        rb.d_obs = std::move(obs);
    }
    if (B <= rb.lanes && to_cm == rb.to_cm && focal == rb.focal) return HPE_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rb.to_cm = -1;  // no table until it is written below
    // a lane's arena: per parity {depth, dt, cx, cy, cz}, then tmp, ctb, dtf; every array on a
    // 256-byte boundary
    const size_t cloud = (sizeof(double) * 250 + 255) & ~(size_t)255;
    const size_t o_dt = sizeof(double) * npix, o_c = o_dt + sizeof(float) * npix,
                 frame = o_c + 3 * cloud;
    const size_t o_tmp = 2 * frame, o_ctb = o_tmp + sizeof(double) * 3 * npix,
                 o_dtf = o_ctb + sizeof(double) * npix, bytes = o_dtf + sizeof(int) * npix;
    while (rb.lanes < B) {
        HIPCHK(c, rb.arena[rb.lanes].alloc(bytes));
        ++rb.lanes;
    }
    std::vector<PrepArgs> &tab = rb.tab;
    tab.resize(2 * M);
    std::memset((void *)tab.data(), 0, sizeof(PrepArgs) * tab.size());
    for (int p = 0; p < 2; ++p)
        for (int b = 0; b < rb.lanes; ++b) {
            char *f = rb.arena[b] + p * frame;
            PrepArgs &a = tab[p * M + b];
            a.to_cm = to_cm;
            a.downsample = 1;
            a.focal = focal;
            a.depth_cm = (double *)f;
            a.dt = (float *)(f + o_dt);
            a.cx = (double *)(f + o_c);
            a.cy = (double *)(f + o_c + cloud);
            a.cz = (double *)(f + o_c + 2 * cloud);
            a.tmp = (double *)(rb.arena[b] + o_tmp);
            a.ctb = (double *)(rb.arena[b] + o_ctb);
            a.dtf = (int *)(rb.arena[b] + o_dtf);
            a.info = rb.d_info + p * M + b;
            a.obs_out = rb.d_obs + p * M + b;
            a.ctr = rb.d_ctr + 32 * b;
            a.raw_stride = npix;
        }
    HIPCHK(c, hipMemcpy(rb.d_tab, tab.data(), sizeof(PrepArgs) * tab.size(), hipMemcpyHostToDevice));
    ++rb.tab_gen;
    rb.to_cm = to_cm;
    rb.focal = focal;
    return HPE_OK;
}

// k frames of B raw lanes, the first in the lanes' prepared buffers `parity`: per frame the
// launches of a prepared batch's on the parity's descriptors, the refine launch carrying every
// lane's next preparation whenever a next frame exists, as enqueue_raw_chunk's does for one
// sequence.  Every cloud is bounded by 250 points: the staged refine and the non-FILT kernels.
static int enqueue_raw_batch_chunk(hpe_ctx *c, int P, int refine, int B, double *d_states,
                                   int parity, int k, bool tail_next, double *hist) {
    hpe_ctx::RawBatch &rb = c->rb;
    for (int i = 0; i < k; ++i) {
        const int cur = (parity + i) & 1, nxt = cur ^ 1;
        // no slot table: the cursor's slot word counts the lane's frames (the preparation's)
        LaneFrameIo io{rb.d_obs + cur * HPE_BATCH_MAX, false, hist, nullptr, rb.d_cur};
        if (i + 1 < k || tail_next) io.prep = rb.d_tab + nxt * HPE_BATCH_MAX;
        io.raw = rb.d_raw;
        if (c->win.mode != HPE_WINDOW_OFF) io.win = c->win.d_tab + nxt * HPE_BATCH_MAX;
        io.follow = c->win.mode == HPE_WINDOW_FOLLOW;
        if (int rc = track_lane_frame(c, P, refine, B, d_states, io)) return rc;
    }
    return HPE_OK;
}

int hpe_track_raw_batch_dev(hpe_ctx *c, int P, int refine, int B, double *d_states,
                            const float *const *d_raw_mm, int n, int to_cm, int downsample,
                            double focal, int frames_per_graph, double *d_hist) {
    if (!c) return HPE_E_ARG;
    int rc = check_chunked_call(c, P, frames_per_graph);
    if (rc || (rc = check_batch_call(c, P, B))) return rc;
    if (!d_states || !d_raw_mm) return fail(c, HPE_E_ARG, "null device states or raw pointers");
    for (int b = 0; b < B; ++b)
        if (!d_raw_mm[b]) return fail(c, HPE_E_ARG, "lane %d: null raw frames", b);
    if (n < 1) return fail(c, HPE_E_ARG, "n = %d frames", n);
    if (!(focal > 0)) return fail(c, HPE_E_ARG, "focal %g is not positive", focal);
    if (!downsample)
        return fail(c, HPE_E_ARG, "downsample = 0: full clouds hold up to %d points, a batch takes "
                    "the single-workgroup refine (<= %d)", HPE_IMG_H * HPE_IMG_W, RF_STAGE_MAX);
    if ((rc = check_window_lanes(c, B)) || (rc = check_hand_lanes(c, B)) ||
        (rc = check_seed_group_lanes(c, B)))
        return rc;
    if (c->live.clean_B)
        return fail(c, HPE_E_STATE, "lane cleaning is set (hpe_set_batch_clean): it cleans a live "
                    "batch's 16-bit frames, resident float sequences are refused (turn it off)");
    HIPCHK(c, hipSetDevice(c->device));
    to_cm = to_cm ? 1 : 0;
    if ((rc = ensure_raw_batch(c, B, to_cm, focal))) return rc;
    const int G = ensure_tracking(c, P, B);
    if (G < 0) return G;
    c->live.cur = -1;  // a live batch in progress (the same lane buffers) ends here
    if ((rc = write_windows(c, focal, to_cm))) return rc;
    hpe_ctx::RawBatch &rb = c->rb;
    // the lanes' raw bases and cursors, then frame 0 of every lane into buffer parity 0
    BatchRaw first{};
    for (int b = 0; b < B; ++b) first.raw[b] = d_raw_mm[b];
    hipLaunchKernelGGL(k_raw_begin_b, dim3(1, B), dim3(64), 0, c->stream, first, n, rb.d_raw, rb.d_cur);
    const bool win = c->win.mode != HPE_WINDOW_OFF;
    hipLaunchKernelGGL(lane_prepare_kernel(LANE_SRC_RAW, win, false), dim3(PREP_WG, B), dim3(PREP_NT),
                       0, c->stream, (const PrepArgs *)rb.d_tab,
                       (const DevWindow *)(win ? c->win.d_tab : nullptr), (const int *)nullptr,
                       (const float *)nullptr, (const float *const *)rb.d_raw, (const int *)rb.d_cur);
    HIPCHK(c, hipGetLastError());
    const int K = frames_per_graph ? frames_per_graph : HPE_SEQ_CHUNK;
    for (int f0 = 0; f0 < n; f0 += K) {
        const int k = n - f0 < K ? n - f0 : K, parity = f0 & 1, tail_next = f0 + k < n;
        GraphKey key = graph_key(P, G, refine, d_states, d_hist);  // not the raw buffers or n
        key.k = k;
        key.parity = parity;
        key.tail_next = tail_next;
        key.B = B;
        key.wave = batch_wave_wpp(c, P, B);
        key.win = c->win.mode;
        key.hands = lane_hands_set(c);
        key.seeds = !c->lane_seeds.empty();
        key.groups = c->lane_groups_B ? 1 : 0;
        key.to_cm = to_cm;
        key.downsample = 1;
        key.focal = focal;
        if ((rc = run_graphed(c, c->graphs[hpe_ctx::GC_RAW_BATCH], key, [&] {
                 return enqueue_raw_batch_chunk(c, P, refine, B, d_states, parity, k, tail_next,
                                                d_hist);
             })))
            return rc;
        if (c->lane_groups_B) c->group_rows = true;
    }
    return mark_seq_done(c);
}

// ---------------------------------------------------------------- live batched lanes
// The live batch's own buffers for B lanes on the raw batch's (ensure_raw_batch first): the
// pinned ring of every new lane, the frame counter, and the ring form of the PrepArgs table --
// rb's entries with raw = the lane's pinned buffer of that parity -- rewritten whenever rb's
// table was or a lane got its ring (the stream drained first: launches in flight read it).
// need_floats: what a pinned buffer must hold, in floats -- one 240x320 float frame, or a view
// batch's largest camera frame; buffers that are too small are replaced for every lane at once.
static int ensure_live_batch(hpe_ctx *c, int B, size_t need_floats) {
    hpe_ctx::LiveBatch &lv = c->live;
    const size_t M = HPE_BATCH_MAX;
    if (!lv.d_tab) {
        DevBuf<PrepArgs> tab;  // moved in last: a block that failed part way runs again in full
        HIPCHK(c, tab.alloc(2 * M));
        HIPCHK(c, lv.d_seq.alloc(1));
        HIPCHK(c, lv.d_act.alloc(HPE_BATCH_MAX));  // the lanes' activity words (lane pacing)
        HIPCHK(c, hipMemset(lv.d_act, 0, sizeof(int) * HPE_BATCH_MAX));
        HIPCHK(c, lv.d_unit.alloc(1));  // a u16 batch's depth unit (lane input)
        HIPCHK(c, lv.d_view.alloc(1));  // a view batch's unit and views
        HIPCHK(c, lv.h_done.alloc(1, hipHostMallocMapped | hipHostMallocCoherent));
        lv.d_tab = std::move(tab);
    }
    const unsigned pin = hipHostMallocMapped | hipHostMallocCoherent;
    if (need_floats > lv.raw_floats) {
        // a view batch whose largest camera frame does not fit: every lane's ring again at that
        // size (the stream has drained: nothing reads the old buffers), all lanes or none -- the
        // new buffers are built aside and moved in together, and the table is rewritten below
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<HostBuf<float>> fresh(2 * (size_t)lv.lanes);
        for (auto &h : fresh) HIPCHK(c, h.alloc(need_floats, pin));
        for (int p = 0; p < 2; ++p)
            for (int b = 0; b < lv.lanes; ++b) lv.h_raw[p][b] = std::move(fresh[p * (size_t)lv.lanes + b]);
        lv.raw_floats = need_floats;
        lv.tab_lanes = -1;
    }
    for (; lv.lanes < B; ++lv.lanes)  // (a lane counts once both its buffers are there)
        for (int p = 0; p < 2; ++p)
            if (!lv.h_raw[p][lv.lanes]) HIPCHK(c, lv.h_raw[p][lv.lanes].alloc(lv.raw_floats, pin));
    if (lv.tab_gen == c->rb.tab_gen && lv.tab_lanes == lv.lanes) return HPE_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<PrepArgs> tab = c->rb.tab;
    for (int p = 0; p < 2; ++p)
        for (int b = 0; b < lv.lanes; ++b) tab[p * M + b].raw = lv.h_raw[p][b].dev();
    HIPCHK(c, hipMemcpy(lv.d_tab, tab.data(), sizeof(PrepArgs) * tab.size(), hipMemcpyHostToDevice));
    lv.tab_gen = c->rb.tab_gen;
    lv.tab_lanes = lv.lanes;
    return HPE_OK;
}

// Lane cleaning's part of a begin with cleaning on (ensure_live_batch first; the stream has
// drained): the staging frames and the three tables, allocated once, all or none, and never
// moved; then the tables written -- the pinned buffers may have been replaced, rb's table
// rewritten and the parameters set again since the last cleaned begin.
static int ensure_clean(hpe_ctx *c) {
    hpe_ctx::LiveBatch &lv = c->live;
    const size_t M = HPE_BATCH_MAX, npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    if (!lv.d_stage) {
        HIPCHK(c, alloc_all(lv.d_cargs, 2 * M, lv.d_cpar, 1, lv.d_ctab, 2 * M));
        // the frames, the guard, moved in last and zeroed first (a lane that has had no frame yet
        // reads back empty): a block that failed part way runs again in full -- the three tables
        // may then still be allocated, and DevBuf::alloc releases what it holds before it allocates
        DevBuf<unsigned short> stage;
        HIPCHK(c, stage.alloc(2 * M * npix));
        HIPCHK(c, hipMemset(stage, 0, sizeof(unsigned short) * 2 * M * npix));
        lv.d_stage = std::move(stage);
    }
    std::vector<CleanArgs> args(2 * M, CleanArgs{nullptr, nullptr});
    std::vector<PrepArgs> tab = c->rb.tab;
    for (int p = 0; p < 2; ++p)
        for (int b = 0; b < lv.lanes; ++b) {
            args[p * M + b] = CleanArgs{(const unsigned short *)lv.h_raw[p][b].dev(), lv.stage(p, b)};
            tab[p * M + b].raw = (const float *)lv.stage(p, b);
        }
    HIPCHK(c, hipMemcpy(lv.d_cargs, args.data(), sizeof(CleanArgs) * args.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(lv.d_ctab, tab.data(), sizeof(PrepArgs) * tab.size(), hipMemcpyHostToDevice));
    CleanTab pt{};
    std::memcpy(pt.par, lv.clean_par, sizeof(pt.par));
    HIPCHK(c, hipMemcpy(lv.d_cpar, &pt, sizeof(pt), hipMemcpyHostToDevice));
    return HPE_OK;
}

// (The frame-array helpers take the lanes' frames as untyped pointers: float or 16-bit frames.)
// Every entry of a lane frame array non-null: 1; every entry null: 0; mixed: -1.
static int lane_frames(const void *const *frames, int B) {
    int set = 0;
    for (int b = 0; b < B; ++b) set += frames[b] != nullptr;
    return set == B ? 1 : set == 0 ? 0 : -1;
}
// Bit b: entry b is non-null.
static uint32_t lane_mask(const void *const *frames, int B) {
    uint32_t m = 0;
    for (int b = 0; b < B; ++b) m |= (uint32_t)(frames[b] != nullptr) << b;
    return m;
}

// One call's activity words of a free-paced batch (HPE_ACT_TRACK: the lane tracks its current
// frame, HPE_ACT_PREP: it prepares a next one), written on the stream ahead of the frame's graph
// -- outside it: a captured argument could not change between replays.  Stream order makes the
// one table enough while earlier calls are still in flight, and lets a call whose words are the
// ones the table already holds at that point of the stream skip the launch (measured: the launch
// ahead of every graph was most of what free pacing cost a batch with full masks, DESIGN.md 4.7).
static void write_lane_act(hpe_ctx *c, int B, uint32_t track, uint32_t prep) {
    hpe_ctx::LiveBatch &lv = c->live;
    LaneAct a{};
    for (int b = 0; b < B; ++b)
        a.word[b] = (track >> b & 1 ? HPE_ACT_TRACK : 0) | (prep >> b & 1 ? HPE_ACT_PREP : 0);
    if (lv.act_known && !std::memcmp(a.word, lv.act_words, sizeof(a.word))) return;
    hipLaunchKernelGGL(k_lane_act, dim3(1), dim3(64), 0, c->stream, a, lv.d_act);
    std::memcpy(lv.act_words, a.word, sizeof(a.word));
    lv.act_known = true;
}

// ---------------------------------------------------------------- lane reports
static const size_t REP_LANE_BYTES = (size_t)HPE_REP_SLOT * HPE_REP_DEPTH_MAX;

size_t hpe_lane_report_size(void) { return sizeof(hpe_lane_report); }

int hpe_set_batch_report(hpe_ctx *c, int depth, const hpe_report_watch *watch) {
    if (!c) return HPE_E_ARG;
    if (depth != 0 && (depth < 2 || depth > HPE_REP_DEPTH_MAX))
        return fail(c, HPE_E_ARG, "report depth %d is neither 0 nor in [2, %d]", depth,
                    HPE_REP_DEPTH_MAX);
    const hpe_report_watch w = watch ? *watch : hpe_report_watch{HUGE_VAL, 0, 0};
    if (w.streak < 0 || w.n_min < 0)
        return fail(c, HPE_E_ARG, "report watch: streak %d or n_min %d is negative", w.streak, w.n_min);
    hpe_ctx::Report &r = c->rep;
    const bool same = depth == r.depth && std::memcmp(&w.cost_max, &r.watch.cost_max, sizeof(double)) == 0 &&
                      w.n_min == r.watch.n_min && w.streak == r.watch.streak;
    // read at the begin: a live batch keeps the reports it began with (hpe_set_batch_form's rule)
    if (c->live.cur >= 0 && !same)
        return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps the reports it began "
                    "with (end it first)");
    if (depth && !r.d_par) {  // once, at full size: never inside a capture, never moved
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, r.h_ring.alloc(REP_LANE_BYTES * HPE_BATCH_MAX, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(r.h_ring, 0, REP_LANE_BYTES * HPE_BATCH_MAX);
        // d_par, the guard, last: a set that failed part way runs again in full
        HIPCHK(c, alloc_all(r.d_lane_seq, HPE_BATCH_MAX, r.d_streak, HPE_BATCH_MAX, r.d_par, 1));
    }
    r.depth = depth;  // no epoch bump: the live graphs are keyed by it (GraphKey::report)
    r.watch = w;
    return HPE_OK;
}

// The begin's part (the stream drained): with reports on, every lane's seq and streak to 0, the
// rings cleared, the watch rule, depth and focal to the device; off: nothing left to read.
static int begin_reports(hpe_ctx *c, int B, double focal) {
    hpe_ctx::Report &r = c->rep;
    c->live.report = r.depth != 0;
    r.ring_depth = 0;
    if (!r.depth) return HPE_OK;
    const RepPar par{r.watch.cost_max, focal, r.watch.n_min, r.watch.streak, r.depth, 0};
    HIPCHK(c, hipMemcpy(r.d_par, &par, sizeof(par), hipMemcpyHostToDevice));
    // (on the stream, as the frame counter is zeroed: the begin synchronises it before it returns)
    HIPCHK(c, hipMemsetAsync(r.d_lane_seq, 0, sizeof(unsigned long long) * HPE_BATCH_MAX, c->stream));
    HIPCHK(c, hipMemsetAsync(r.d_streak, 0, sizeof(int) * HPE_BATCH_MAX, c->stream));
    std::memset(r.h_ring, 0, REP_LANE_BYTES * HPE_BATCH_MAX);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    std::memset(r.enq, 0, sizeof(r.enq));
    r.ring_depth = r.depth;
    r.ring_B = B;
    return HPE_OK;
}

// The report launch of B lanes, after a frame's final launch (TRACK: act as the frame's kernels
// take it, every lane selected) or after a lane initialisation's last launch (INIT: `sel`), on
// the preparation records of buffer parity `parity`: the frames just tracked, or held prepared.
static int enqueue_report(hpe_ctx *c, int B, const double *d_states, int parity, const int *act,
                          unsigned sel, int kind) {
    const hpe_ctx::Report &r = c->rep;
    const RepDev rd{(unsigned long long *)r.h_ring.dev(), r.d_par, r.d_lane_seq, r.d_streak};
    hipLaunchKernelGGL(k_report_b, dim3(B), dim3(64), 0, c->stream, d_states,
                       (const DevHand *)c->d_lane_hands,
                       (const PrepInfo *)c->rb.d_info + parity * HPE_BATCH_MAX,
                       (const unsigned long long *)c->live.d_seq, rd, act, sel, kind);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// What the three read calls check first; the lane's ring.
static int report_ring(hpe_ctx *c, int lane, const void *out, const char **ring) {
    const hpe_ctx::Report &r = c->rep;
    if (!out) return fail(c, HPE_E_ARG, "null report");
    if (!r.ring_depth)
        return fail(c, HPE_E_STATE, "no batch with lane reports has begun (hpe_set_batch_report)");
    if (lane < 0 || lane >= r.ring_B)
        return fail(c, HPE_E_ARG, "lane %d outside the batch's %d lanes", lane, r.ring_B);
    *ring = r.h_ring + REP_LANE_BYTES * lane;
    return HPE_OK;
}

int hpe_batch_report(hpe_ctx *c, int lane, uint64_t seq, hpe_lane_report *out) {
    if (!c) return HPE_E_ARG;
    const char *ring = nullptr;
    if (int rc = report_ring(c, lane, out, &ring)) return rc;
    if (!seq) {
        hpe_report::read_newest(ring, c->rep.ring_depth, out);
        return HPE_OK;
    }
    if (!hpe_report::read_seq(ring, c->rep.ring_depth, seq, out))
        return fail(c, HPE_E_STATE, "lane %d: report %llu is not in the ring (not yet, or no longer)",
                    lane, (unsigned long long)seq);
    return HPE_OK;
}

int hpe_batch_report_wait(hpe_ctx *c, int lane, uint64_t seq, int timeout_ms, hpe_lane_report *out) {
    if (!c) return HPE_E_ARG;
    const char *ring = nullptr;
    if (int rc = report_ring(c, lane, out, &ring)) return rc;
    const hpe_ctx::Report &r = c->rep;
    const uint64_t enq = r.enq[lane];
    if (!seq && !enq) {  // nothing was enqueued for the lane
        out->seq = 0;
        return HPE_OK;
    }
    if (!seq) seq = enq;
    if (seq > enq || seq + (uint64_t)r.ring_depth <= enq)
        return fail(c, HPE_E_STATE, "lane %d: report %llu was not enqueued, or its slot has been "
                    "enqueued again (%llu reports, depth %d)", lane, (unsigned long long)seq,
                    (unsigned long long)enq, r.ring_depth);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (hpe_report::read_seq(ring, r.ring_depth, seq, out)) return HPE_OK;
        if ((it & 255) == 255) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 0))
                return fail(c, HPE_E_HIP, "lane %d: report %llu did not complete in %d ms", lane,
                            (unsigned long long)seq, timeout_ms);
            std::this_thread::yield();
        }
    }
}

int hpe_batch_lost(hpe_ctx *c, uint32_t *mask_out) {
    if (!c) return HPE_E_ARG;
    const char *ring = nullptr;
    if (int rc = report_ring(c, 0, mask_out, &ring)) return rc;
    uint32_t m = 0;
    hpe_lane_report rep;
    for (int b = 0; b < c->rep.ring_B; ++b)
        if (hpe_report::read_newest(ring + REP_LANE_BYTES * b, c->rep.ring_depth, &rep) &&
            (rep.flags & HPE_REPORT_F_LOST))
            m |= 1u << b;
    *mask_out = m;
    return HPE_OK;
}

int hpe_lane_joints_dev(hpe_ctx *c, int B, int n, const double *d_hist, double focal,
                        double *d_joints, double *d_px) {
    if (!c) return HPE_E_ARG;
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (n < 1) return fail(c, HPE_E_ARG, "%d history rows per lane", n);
    if (!d_hist || !d_joints) return fail(c, HPE_E_ARG, "null history or joints");
    if (d_px && !(focal > 0)) return fail(c, HPE_E_ARG, "focal %g is not positive", focal);
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_lane_joints_b, dim3(n, B), dim3(64), 0, c->stream, d_hist,
                       (const DevHand *)c->d_lane_hands, focal, d_joints, d_px);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// Lane location's buffers (allocated by the first begin with the windows on, or by the first
// hpe_locate_depth; zeroed, as a begin leaves them).
static int ensure_locate(hpe_ctx *c) {
    hpe_ctx::Locate &lo = c->loc;
    if (lo.d_frame) return HPE_OK;
    const size_t M = HPE_BATCH_MAX;
    HIPCHK(c, lo.h_tab.alloc((size_t)LOC_SLOT * M, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(lo.h_tab, 0, (size_t)LOC_SLOT * M);
    HIPCHK(c, lo.d_res.alloc(M + 1));
    // (zeroed on the stream: the launches that read them follow it there)
    HIPCHK(c, lo.d_act.alloc(M + 1));
    HIPCHK(c, hipMemsetAsync(lo.d_act, 0, sizeof(int) * (M + 1), c->stream));
    HIPCHK(c, lo.d_seq.alloc(M));
    HIPCHK(c, hipMemsetAsync(lo.d_seq, 0, sizeof(unsigned long long) * M, c->stream));
    HIPCHK(c, lo.d_frame.alloc((size_t)HPE_IMG_H * HPE_IMG_W));  // the guard, last (as hpe_set_batch_report)
    return HPE_OK;
}

// The begin's part (the stream drained): every lane's locate counter to 0, the host table cleared.
static int begin_locates(hpe_ctx *c, int B) {
    hpe_ctx::Locate &lo = c->loc;
    lo.B = B;
    std::memset(lo.enq, 0, sizeof(lo.enq));
    if (!lo.d_frame) return HPE_OK;  // nothing allocated yet: ensure_locate zeroes what it makes
    HIPCHK(c, hipMemsetAsync(lo.d_seq, 0, sizeof(unsigned long long) * HPE_BATCH_MAX, c->stream));
    std::memset(lo.h_tab, 0, (size_t)LOC_SLOT * HPE_BATCH_MAX);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    return HPE_OK;
}

static int check_view(hpe_ctx *c, const hpe_view &v, int lane);

// The begin of a live batch in either frame format: u16 false, float mm frames; true, 16-bit
// frames of unit_mm each -- 240x320, or with `views` lane b's camera frame of views[b].
static int live_batch_begin(hpe_ctx *c, int B, const void *const *depth_mm, bool u16, float unit_mm,
                            int to_cm, int downsample, double focal,
                            const hpe_view *views = nullptr) {
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    size_t need_floats = (size_t)HPE_IMG_H * HPE_IMG_W;
    for (int b = 0; views && b < B; ++b) {
        if (int vrc = check_view(c, views[b], b)) return vrc;
        const size_t fl = ((size_t)views[b].pitch * (size_t)views[b].height + 1) / 2;
        if (fl > need_floats) need_floats = fl;
    }
    // lane cleaning: the rule is defined on 16-bit values, and the parameters are the lanes'
    const bool clean = c->live.clean_B != 0;
    if (clean && !u16)
        return fail(c, HPE_E_STATE, "lane cleaning is set (hpe_set_batch_clean): it cleans 16-bit "
                    "frames, a float batch is refused (turn it off, or begin a u16 or view batch)");
    if (clean && B != c->live.clean_B)
        return fail(c, HPE_E_ARG, "%d lanes, the cleaning parameters were set for %d", B,
                    c->live.clean_B);
    const bool paced = c->batch_pacing == HPE_PACING_FREE;
    if (!depth_mm || (!paced && lane_frames(depth_mm, B) != 1))
        return fail(c, HPE_E_ARG, "null frame array or lane frame");
    const uint32_t given = lane_mask(depth_mm, B);
    if (!given)
        return fail(c, HPE_E_ARG, "no lane frame: a free-paced batch begins with at least one");
    if (!(focal > 0)) return fail(c, HPE_E_ARG, "focal %g is not positive", focal);
    if (!downsample)
        return fail(c, HPE_E_ARG, "downsample = 0: full clouds hold up to %d points, a batch takes "
                    "the single-workgroup refine (<= %d)", HPE_IMG_H * HPE_IMG_W, RF_STAGE_MAX);
    if (c->ss.transport())
        return fail(c, HPE_E_STATE, "a subswarm transport is live: a batch runs without the "
                    "exchange (hpe_subswarm_fini)");
    if (c->xch_every > 0)
        return fail(c, HPE_E_STATE, "the per-generation exchange is on (hpe_set_exchange)");
    if (const char *u = std::getenv("HPE_PIPE_UPLOAD"))
        if (u[0] == '1')
            return fail(c, HPE_E_STATE, "HPE_PIPE_UPLOAD=1: the upload form is not built for lanes "
                        "(a live batch reads its pinned buffers in place)");
    if (int wrc = check_window_lanes(c, B)) return wrc;
    if (int hrc = check_hand_lanes(c, B)) return hrc;
    if (int src = check_seed_group_lanes(c, B)) return src;
    if (paced)
        if (int grc = check_group_frames(c, B, given)) return grc;
    if (u16 && !(std::isfinite(unit_mm) && unit_mm > 0))
        return fail(c, HPE_E_ARG, "depth unit %g mm is not finite and positive", (double)unit_mm);
    HIPCHK(c, hipSetDevice(c->device));
    // the frames of a batch in progress are done with: its pinned buffers are free to refill
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hpe_ctx::LiveBatch &lv = c->live;
    lv.cur = -1;
    to_cm = to_cm ? 1 : 0;
    int rc = ensure_batch_lanes(c);
    if (rc || (rc = ensure_raw_batch(c, B, to_cm, focal)) || (rc = ensure_live_batch(c, B, need_floats))) return rc;
    if ((rc = write_windows(c, focal, to_cm))) return rc;
    lv.clean = false;
    if (clean) {
        if ((rc = ensure_clean(c))) return rc;
        lv.clean = true;
        lv.cleaned_B = B;
    }
    lv.u16 = u16;
    lv.view = views != nullptr;
    if (views) {  // the unit and the views, one block (the stream has drained)
        ViewTab vt{};
        vt.unit = unit_mm;
        std::memcpy(vt.view, views, sizeof(hpe_view) * (size_t)B);
        HIPCHK(c, hipMemcpy(lv.d_view, &vt, sizeof(vt), hipMemcpyHostToDevice));
        std::memcpy(lv.views, views, sizeof(hpe_view) * (size_t)B);
        lv.views_B = B;
    }
    // the depth unit, as the windows' parameters: device memory, not the graphs, holds it (the
    // stream has drained)
    if (u16) HIPCHK(c, hipMemcpy(lv.d_unit, &unit_mm, sizeof(float), hipMemcpyHostToDevice));
    lv.unit_mm = u16 ? unit_mm : 1.f;
    HIPCHK(c, hipMemsetAsync(lv.d_seq, 0, sizeof(unsigned long long), c->stream));
    __atomic_store_n(lv.h_done.get(), 0ull, __ATOMIC_RELEASE);
    lv.enq = 0;
    lv.used_seq[0] = lv.used_seq[1] = 0;
    // lane location's buffers, while nothing is in flight: a locate call of this batch (it needs
    // the windows on) then allocates nothing and stays asynchronous
    if (c->win.mode != HPE_WINDOW_OFF && (rc = ensure_locate(c))) return rc;
    if ((rc = begin_reports(c, B, focal)) || (rc = begin_locates(c, B))) return rc;
    // frame 0 of every lane: into its pinned buffer of parity 0, prepared from there
    for (int b = 0; b < B; ++b)
        if ((given >> b & 1) && depth_mm[b] != lv.h_raw[0][b])
            std::memcpy(lv.h_raw[0][b], depth_mm[b], lv.frame_bytes(b));
    const bool win = c->win.mode != HPE_WINDOW_OFF;
    // paced: only the lanes given a frame prepare one; the others start empty
    if (paced) write_lane_act(c, B, 0, given);
    if (lv.clean)  // cleaned first, from the pinned buffers to the staging frames of parity 0
        hipLaunchKernelGGL(lv.view ? k_clean_b<true> : k_clean_b<false>, dim3(CLEAN_TILES, B),
                           dim3(CLEAN_NT), 0, c->stream, (const CleanArgs *)lv.d_cargs,
                           (const CleanTab *)lv.d_cpar,
                           (const ViewTab *)(lv.view ? lv.d_view.get() : nullptr),
                           (const int *)(paced ? lv.d_act : nullptr));
    hipLaunchKernelGGL(lane_prepare_kernel(lv.src(), win, paced),
                       dim3(PREP_WG, B), dim3(PREP_NT), 0, c->stream, lv.prep_tab(),
                       (const DevWindow *)(win ? c->win.d_tab : nullptr),
                       (const int *)(paced ? lv.d_act : nullptr),
                       lv.unit_arg(), (const float *const *)nullptr,
                       (const int *)nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lv.B = B;
    lv.to_cm = to_cm;
    lv.focal = focal;
    lv.pacing = c->batch_pacing;
    lv.pending = given;
    lv.cur = 0;
    return HPE_OK;
}

int hpe_batch_pipeline_begin(hpe_ctx *c, int B, const float *const *depth_mm, int to_cm,
                             int downsample, double focal) {
    if (!c) return HPE_E_ARG;
    return live_batch_begin(c, B, (const void *const *)depth_mm, false, 1.f, to_cm, downsample, focal);
}

int hpe_batch_pipeline_begin_u16(hpe_ctx *c, int B, const uint16_t *const *depth, float unit_mm,
                                 int to_cm, int downsample, double focal) {
    if (!c) return HPE_E_ARG;
    return live_batch_begin(c, B, (const void *const *)depth, true, unit_mm, to_cm, downsample, focal);
}

// One lane's view against the refusals of include/hpe.h "Lane views".
static int check_view(hpe_ctx *c, const hpe_view &v, int lane) {
    if (v.step < 1 || v.step > 8)
        return fail(c, HPE_E_ARG, "lane %d: view step %d outside 1..8", lane, v.step);
    if (v.width < 1 || v.height < 1 || v.pitch < v.width)
        return fail(c, HPE_E_ARG, "lane %d: view of a %d x %d camera image with pitch %d", lane,
                    v.width, v.height, v.pitch);
    if (v.pitch > HPE_VIEW_DIM_MAX || v.height > HPE_VIEW_DIM_MAX ||
        (long long)v.pitch * v.height > HPE_VIEW_PIXELS_MAX)
        return fail(c, HPE_E_ARG, "lane %d: view pitch %d or height %d above %d, or more than %d "
                    "pixels per frame", lane, v.pitch, v.height, HPE_VIEW_DIM_MAX, HPE_VIEW_PIXELS_MAX);
    if ((v.flags & ~HPE_VIEW_FLIP_COLS) || v.pad)
        return fail(c, HPE_E_ARG, "lane %d: unknown view flags 0x%x or non-zero pad %d", lane,
                    v.flags, v.pad);
    return HPE_OK;
}

int hpe_batch_pipeline_begin_view(hpe_ctx *c, int B, const uint16_t *const *frames,
                                  const hpe_view *views, float unit_mm, int to_cm,
                                  int downsample, double focal) {
    if (!c) return HPE_E_ARG;
    if (!views) return fail(c, HPE_E_ARG, "null views");
    return live_batch_begin(c, B, (const void *const *)frames, true, unit_mm, to_cm, downsample,
                            focal, views);
}

int hpe_view_fit(int width, int height, int pitch, double fx, double cx, double cy, int step,
                 uint32_t flags, hpe_view *out, double *focal_out, double residual_px[2]) {
    if (!out || !std::isfinite(fx) || !(fx > 0) || !std::isfinite(cx) || !std::isfinite(cy))
        return HPE_E_ARG;
    const bool flip = (flags & HPE_VIEW_FLIP_COLS) != 0;
    const double r0 = cy - 120.0 * step, c0 = cx - (flip ? 159.0 : 160.0) * step;
    if (!(std::fabs(r0) < 1e9) || !(std::fabs(c0) < 1e9)) return HPE_E_ARG;
    const hpe_view v = {width, height, pitch, (int32_t)std::lrint(r0), (int32_t)std::lrint(c0),
                        step, flags, 0};
    if (check_view(nullptr, v, 0)) return HPE_E_ARG;
    *out = v;
    if (focal_out) *focal_out = fx / step;
    if (residual_px) {  // the principal point in model pixels, less (160, 120)
        const double mc = (cx - v.col0) / step;
        residual_px[0] = (flip ? 319.0 - mc : mc) - 160.0;
        residual_px[1] = (cy - v.row0) / step - 120.0;
    }
    return HPE_OK;
}

int hpe_batch_views_readback(hpe_ctx *c, int B, hpe_view *out) {
    if (!c) return HPE_E_ARG;
    if (!out) return fail(c, HPE_E_ARG, "null views");
    hpe_ctx::LiveBatch &lv = c->live;
    if (!lv.views_B) return fail(c, HPE_E_STATE, "no view batch has begun (hpe_batch_pipeline_begin_view)");
    if (B < 1 || B > lv.views_B)
        return fail(c, HPE_E_ARG, "%d lanes, the last view batch began with %d", B, lv.views_B);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, (const char *)lv.d_view.get() + offsetof(ViewTab, view),
                        sizeof(hpe_view) * (size_t)B, hipMemcpyDeviceToHost));
    return HPE_OK;
}

// ---------------------------------------------------------------- lane cleaning
static_assert(offsetof(ViewTab, unit) == 0, "a cleaned view batch's u16 preparation reads the unit there");

int hpe_clean_defaults(float unit_mm, hpe_clean *out) {
    if (!out || !(std::isfinite(unit_mm) && unit_mm > 0)) return HPE_E_ARG;
    const double e = std::nearbyint(15.0 / (double)unit_mm);
    *out = hpe_clean{(uint16_t)(e < 1 ? 1 : e > 65535 ? 65535 : e), 3, HPE_CLEAN_MEDIAN, 0};
    return HPE_OK;
}

// One lane's parameters against the refusals of include/hpe.h "Lane cleaning".
static int check_clean(hpe_ctx *c, const hpe_clean &p, int lane) {
    if (p.support > 8)
        return fail(c, HPE_E_ARG, "lane %d: clean support %d above 8", lane, (int)p.support);
    if ((p.flags & ~HPE_CLEAN_MEDIAN) || p.pad)
        return fail(c, HPE_E_ARG, "lane %d: unknown clean flags 0x%x or non-zero pad %u", lane,
                    (unsigned)p.flags, (unsigned)p.pad);
    return HPE_OK;
}

int hpe_set_batch_clean(hpe_ctx *c, int B, const hpe_clean *params) {
    if (!c) return HPE_E_ARG;
    hpe_ctx::LiveBatch &lv = c->live;
    if (params) {
        if (B < 1 || B > HPE_BATCH_MAX)
            return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
        for (int b = 0; b < B; ++b)
            if (int rc = check_clean(c, params[b], b)) return rc;
    }
    if (lv.cur >= 0) {  // a live batch keeps cleaning on or off, and its lanes
        if ((params != nullptr) != lv.clean)
            return fail(c, HPE_E_STATE, "a live batch is in progress: it keeps lane cleaning %s, as "
                        "it began (end it first)", lv.clean ? "on" : "off");
        if (params && B != lv.B)
            return fail(c, HPE_E_STATE, "a live batch of %d lanes is in progress: cleaning "
                        "parameters for %d lanes (end it first)", lv.B, B);
    }
    if (!params) {
        lv.clean_B = 0;
        return HPE_OK;
    }
    if (lv.cur >= 0) {  // the table, once nothing in flight reads it: from the next frame cleaned
        CleanTab pt{};
        std::memcpy(pt.par, params, sizeof(hpe_clean) * (size_t)B);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(lv.d_cpar, &pt, sizeof(pt), hipMemcpyHostToDevice));
    }
    std::memset(lv.clean_par, 0, sizeof(lv.clean_par));
    std::memcpy(lv.clean_par, params, sizeof(hpe_clean) * (size_t)B);
    lv.clean_B = B;
    return HPE_OK;
}

int hpe_clean_depth_u16(hpe_ctx *c, const uint16_t *frame, const hpe_view *view,
                        const hpe_clean *params, uint16_t *out) {
    if (!c) return HPE_E_ARG;
    if (!frame || !params || !out) return fail(c, HPE_E_ARG, "null frame, parameters or result");
    if (int rc = check_clean(c, *params, 0)) return rc;
    if (view)
        if (int rc = check_view(c, *view, 0)) return rc;
    const size_t npix = (size_t)HPE_IMG_H * HPE_IMG_W;
    const size_t src_pixels = view ? (size_t)view->pitch * (size_t)view->height : npix;
    HIPCHK(c, hipSetDevice(c->device));
    hpe_ctx::CleanOne &o = c->clean_one;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier call's kernel may still read the buffers
    if (!o.d_dst) {
        HIPCHK(c, alloc_all(o.d_args, 1, o.d_par, 1, o.d_view, 1, o.d_dst, npix));
        o.src_pixels = 0;
    }
    if (src_pixels > o.src_pixels) {
        o.src_pixels = 0;
        HIPCHK(c, o.d_src.alloc(src_pixels));
        o.src_pixels = src_pixels;
    }
    const CleanArgs args{o.d_src.get(), o.d_dst.get()};
    CleanTab pt{};
    pt.par[0] = *params;
    ViewTab vt{};
    if (view) vt.view[0] = *view;
    HIPCHK(c, hipMemcpy(o.d_src, frame, sizeof(uint16_t) * src_pixels, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(o.d_args, &args, sizeof(args), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(o.d_par, &pt, sizeof(pt), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(o.d_view, &vt, sizeof(vt), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(view ? k_clean_b<true> : k_clean_b<false>, dim3(CLEAN_TILES, 1),
                       dim3(CLEAN_NT), 0, c->stream, (const CleanArgs *)o.d_args,
                       (const CleanTab *)o.d_par, (const ViewTab *)(view ? o.d_view.get() : nullptr),
                       (const int *)nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, o.d_dst, sizeof(uint16_t) * npix, hipMemcpyDeviceToHost));
    return HPE_OK;
}

int hpe_batch_clean_readback(hpe_ctx *c, int parity, int lane, uint16_t *out) {
    if (!c) return HPE_E_ARG;
    if (!out) return fail(c, HPE_E_ARG, "null frame");
    hpe_ctx::LiveBatch &lv = c->live;
    if (!lv.cleaned_B)
        return fail(c, HPE_E_STATE, "no cleaned batch has begun (hpe_set_batch_clean before the begin)");
    if (parity < 0 || parity > 1) return fail(c, HPE_E_ARG, "buffer parity %d", parity);
    if (lane < 0 || lane >= lv.cleaned_B)
        return fail(c, HPE_E_ARG, "lane %d outside the cleaned batch's %d lanes", lane, lv.cleaned_B);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, lv.stage(parity, lane), sizeof(uint16_t) * (size_t)HPE_IMG_H * HPE_IMG_W,
                        hipMemcpyDeviceToHost));
    return HPE_OK;
}

// Lane `lane`'s pinned buffer of the parity the next track call reads, once the device has read
// the frame it last held (the track call's own wait, before its copy).
int hpe_batch_frame_buffer(hpe_ctx *c, int lane, void **buf_out, size_t *bytes_out) {
    if (!c) return HPE_E_ARG;
    if (!buf_out) return fail(c, HPE_E_ARG, "null buffer pointer");
    hpe_ctx::LiveBatch &lv = c->live;
    if (lv.cur < 0)
        return fail(c, HPE_E_STATE, "no live batch: hpe_batch_pipeline_begin not called, or the "
                    "batch ended");
    if (lane < 0 || lane >= lv.B)
        return fail(c, HPE_E_ARG, "lane %d outside the batch's %d lanes", lane, lv.B);
    const int nxt = lv.cur ^ 1;
    if (lv.used_seq[nxt] && !wait_frame_done(lv.h_done, lv.used_seq[nxt]))
        return fail(c, HPE_E_HIP, "live batch frame %llu did not complete",
                    (unsigned long long)lv.used_seq[nxt]);
    *buf_out = lv.h_raw[nxt][lane];
    if (bytes_out) *bytes_out = lv.frame_bytes(lane);
    return HPE_OK;
}

// The track call of a live batch in either frame format (u16: the entry point's).
static int live_batch_track(hpe_ctx *c, int P, int refine, int B, double *d_states,
                            const void *const *next_depth_mm, bool u16) {
    if (int erc = mw_check_async(c)) return erc;
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    int rc = check_P(c, P);
    if (rc || (rc = check_batch_call(c, P, B))) return rc;
    if (!d_states) return fail(c, HPE_E_ARG, "null device states");
    hpe_ctx::LiveBatch &lv = c->live;
    // a free-paced batch (it keeps the pacing it began with) takes any subset of next frames, and
    // a non-null array keeps it alive; in lockstep, a frame for every lane or for none
    const bool paced = lv.cur >= 0 && lv.pacing == HPE_PACING_FREE;
    const int next = !next_depth_mm ? 0 : paced ? 1 : lane_frames(next_depth_mm, B);
    if (next < 0)
        return fail(c, HPE_E_ARG, "next frames for some lanes only: lanes advance in lockstep");
    if (lv.cur < 0)
        return fail(c, HPE_E_STATE, "no live batch: hpe_batch_pipeline_begin not called, or the "
                    "batch ended");
    if (B != lv.B)
        return fail(c, HPE_E_STATE, "%d lanes, the batch began with %d (end it and begin another)",
                    B, lv.B);
    if (u16 != lv.u16)
        return fail(c, HPE_E_STATE, "the batch began with %s frames and keeps that format: this is "
                    "the track call for %s frames", lv.u16 ? "u16" : "f32", u16 ? "u16" : "f32");
    HIPCHK(c, hipSetDevice(c->device));
    const int cur = lv.cur, nxt = cur ^ 1;
    const uint32_t all = B < 32 ? (1u << B) - 1 : ~0u;
    const uint32_t given = !next ? 0 : paced ? lane_mask(next_depth_mm, B) : all;
    if (paced)
        if (int grc = check_group_frames(c, B, given)) return grc;
    // a lane's own pinned buffer as its next frame (hpe_batch_frame_buffer) was filled in place;
    // a buffer of the other parity holds a current frame: its pointer is from before an earlier call
    for (int b = 0; b < B; ++b)
        for (int k = 0; (given >> b & 1) && k < B; ++k)
            if (next_depth_mm[b] == lv.h_raw[cur][k])
                return fail(c, HPE_E_ARG, "lane %d: stale frame buffer (lane %d's, which holds its "
                            "current frame: ask hpe_batch_frame_buffer after every track call)", b, k);
    if (given) {  // the pinned buffers' previous frames (two ago) must have been read
        if (lv.used_seq[nxt] && !wait_frame_done(lv.h_done, lv.used_seq[nxt]))
            return fail(c, HPE_E_HIP, "live batch frame %llu did not complete",
                        (unsigned long long)lv.used_seq[nxt]);
        for (int b = 0; b < B; ++b)  // only the lanes given a frame, and not one filled in place
            if ((given >> b & 1) && next_depth_mm[b] != lv.h_raw[nxt][b])
                std::memcpy(lv.h_raw[nxt][b], next_depth_mm[b], lv.frame_bytes(b));
    }
    const int G = ensure_tracking(c, P, B);  // (the lanes' tables are the begin's)
    if (G < 0) return G;
    GraphKey key = graph_key(P, G, refine, d_states);  // the shape: never a host pointer
    key.B = B;
    key.wave = batch_wave_wpp(c, P, B);
    key.win = c->win.mode;  // the begin's: it cannot change while the batch lives
    key.hands = lane_hands_set(c);  // ... nor can the hands
    key.seeds = !c->lane_seeds.empty();  // ... nor the seeds
    key.groups = c->lane_groups_B ? 1 : 0;  // ... nor the groups
    key.pacing = lv.pacing;  // ... nor the pacing; FREE: next is "the array is non-null", and
                             // the lanes' masks are never part of the key
    key.cur = cur;
    key.next = next;
    key.to_cm = lv.to_cm;
    key.downsample = 1;
    key.focal = lv.focal;
    key.u16 = lv.u16 ? 1 : 0;  // ... nor the frame format (never the unit)
    key.view = lv.view ? 1 : 0;  // ... nor whether it is read through views (never a view)
    // a frame of a raw batch's on the descriptors of parity cur, with the ring's preparation (the
    // next frames read from the pinned buffers of parity nxt), no history or cursor, and the final
    // launch that publishes the batch's frame number
    LaneFrameIo io{c->rb.d_obs + cur * HPE_BATCH_MAX, false, nullptr, nullptr, nullptr};
    if (next) io.prep = lv.prep_tab() + nxt * HPE_BATCH_MAX;
    if (c->win.mode != HPE_WINDOW_OFF) io.win = c->win.d_tab + nxt * HPE_BATCH_MAX;
    io.follow = c->win.mode == HPE_WINDOW_FOLLOW;
    io.seq = lv.d_seq;
    io.done_host = lv.h_done.dev();
    io.unit = lv.unit_arg();
    io.view = lv.view && !lv.clean;
    key.clean = lv.clean ? 1 : 0;  // ... nor whether it is cleaned (never a parameter)
    if (lv.clean) {  // k_clean_b ahead of the refine launch, then the u16 forms on the staging
        io.clean = lv.d_cargs + nxt * HPE_BATCH_MAX;
        io.clean_par = lv.d_cpar;
        if (lv.view) io.clean_view = lv.d_view;
    }
    if (paced) {
        write_lane_act(c, B, lv.pending, given);
        io.act = lv.d_act;
    }
    key.report = lv.report ? 1 : 0;  // ... nor whether reports are on (never their depth or watch)
    // with reports on, k_report_b follows the final launch inside the frame's graph: the lanes
    // that track in this call, on the buffer parity the final launch used
    if ((rc = run_graphed(c, c->graphs[hpe_ctx::GC_LIVE_BATCH], key, [&] {
             if (int erc = track_lane_frame(c, P, refine, B, d_states, io)) return erc;
             return lv.report ? enqueue_report(c, B, d_states, cur, io.act, all, HPE_REPORT_TRACK)
                              : HPE_OK;
         })))
        return rc;
    if (c->lane_groups_B) c->group_rows = true;
    if (lv.report)
        for (int b = 0; b < B; ++b) c->rep.enq[b] += (paced ? lv.pending : all) >> b & 1;
    ++lv.enq;  // this frame's number; lane 0's final workgroup publishes it to h_done
    if (given) lv.used_seq[nxt] = lv.enq;  // its refine launch reads h_raw[nxt]
    lv.pending = given;
    lv.cur = next ? nxt : -1;
    return HPE_OK;
}

int hpe_track_batch_pipelined(hpe_ctx *c, int P, int refine, int B, double *d_states,
                              const float *const *next_depth_mm) {
    if (!c) return HPE_E_ARG;
    return live_batch_track(c, P, refine, B, d_states, (const void *const *)next_depth_mm, false);
}

int hpe_track_batch_pipelined_u16(hpe_ctx *c, int P, int refine, int B, double *d_states,
                                  const uint16_t *const *next_depth) {
    if (!c) return HPE_E_ARG;
    return live_batch_track(c, P, refine, B, d_states, (const void *const *)next_depth, true);
}

// ---------------------------------------------------------------- lane initialisation
// The lane forms' arenas for swarms of P particles, G generations and `lanes` lanes, and the
// bounds the context holds now.  Nothing a captured graph uses: no epoch bump.
static int ensure_opt_lanes(hpe_ctx *c, int P, int G, int lanes) {
    OptLanes &s = c->optl;
    if (!s.d_obs) HIPCHK(c, s.d_obs.alloc(HPE_BATCH_MAX));
    if (!(s.P == P && s.G >= G && s.seed == c->seed && s.lanes >= lanes)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight use the arenas
        if (lanes < s.lanes) lanes = s.lanes;        // grown, never shrunk
        if (G < s.G) G = s.G;
        s.reset();
        const size_t e = sizeof(double) * (size_t)P * HPE_DOF;
        const size_t bytes[7] = {e, e, e, sizeof(double) * (size_t)P, sizeof(double) * 28,
                                 sizeof(double) * (size_t)(G > 0 ? G : 1),
                                 sizeof(unsigned) * (ARRIVE_SHARDS * 32 + 1)};
        size_t at = 0;
        for (int k = 0; k < 7; ++k) {  // every array, the counters included, on lines of its own
            s.off[k] = at;
            at += (bytes[k] + 127) & ~(size_t)127;
        }
        s.stride = at;
        HIPCHK(c, alloc_all(s.arena, s.stride * (size_t)lanes, s.normals, (size_t)P * HPE_DOF,
                            s.bounds, (size_t)3 * HPE_DOF));
        // the counters start at 0 (on the stream: the launches that count follow it there)
        HIPCHK(c, hipMemsetAsync(s.arena, 0, s.stride * (size_t)lanes, c->stream));
        std::vector<double> nrm((size_t)P * HPE_DOF);
        hpe::make_normals(c->seed, P, nrm.data(), ST_OPT_NORMAL);
        HIPCHK(c, hipMemcpy(s.normals, nrm.data(), e, hipMemcpyHostToDevice));
        s.P = P;
        s.G = G;
        s.lanes = lanes;
        s.seed = c->seed;
    }
    double b[3 * HPE_DOF];
    std::memcpy(b, c->lb, sizeof(c->lb));
    std::memcpy(b + HPE_DOF, c->ub, sizeof(c->ub));
    std::memcpy(b + 2 * HPE_DOF, c->sd, sizeof(c->sd));
    if (!s.bounds_set || std::memcmp(b, s.bounds_h, sizeof(b))) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // launches in flight read the old bounds
        HIPCHK(c, hipMemcpy(s.bounds, b, sizeof(b), hipMemcpyHostToDevice));
        std::memcpy(s.bounds_h, b, sizeof(b));
        s.bounds_set = true;
    }
    return HPE_OK;
}

// pso_optimise of the L lanes of `ll` in the same launches, direct and asynchronous: lane b on
// descriptor obs[b] (at most n_max points each), hand d_lane_hands[b], x0 = d_states + 27 b,
// which the trailing launch overwrites with {bestp, cost}; its trace to row b of d_trace.  The
// generation index is a kernel argument and a call runs once per batch, so nothing is captured.
static int enqueue_opt_lanes(hpe_ctx *c, int P, int G, const DevObs *obs, const OptLaneList &ll,
                             int L, int n_max, double *d_states, double *d_trace) {
    const OptLanes &s = c->optl;
    DevOpt d;
    d.x = (double *)(s.arena + s.off[0]);
    d.v = (double *)(s.arena + s.off[1]);
    d.pb = (double *)(s.arena + s.off[2]);
    d.pc = (double *)(s.arena + s.off[3]);
    d.gbest = (double *)(s.arena + s.off[4]);
    d.trace = (double *)(s.arena + s.off[5]);
    d.match = nullptr;  // the staged descent keeps matchId in LDS
    d.ctr = (unsigned *)(s.arena + s.off[6]);
    d.normals = s.normals;
    d.bounds = s.bounds;
    d.seed = c->seed;
    d.P = P;
    d.G = G;
    d.n_cap = 0;
    d.w = c->omega;
    d.c1 = c->phip;
    d.c2 = c->phig;
    const DevHand *hands = c->d_lane_hands;
    const unsigned lds = (unsigned)((size_t)n_max * (3 * sizeof(double) + sizeof(int32_t)));
    const dim3 grid(P, L);
    hipLaunchKernelGGL(k_opt_init_b, grid, dim3(HPE_NT), 0, c->stream, d, s.stride, ll,
                       (const double *)d_states, obs, hands);
    for (int g = 1; g <= G; ++g) {
        hipLaunchKernelGGL(k_opt_descent_b<true>, grid, dim3(RF_NT), lds, c->stream, d, s.stride, ll, obs,
                           hands, g);
        hipLaunchKernelGGL(k_opt_move_b, grid, dim3(HPE_NT), 0, c->stream, d, s.stride, ll, obs,
                           hands, g);
    }
    hipLaunchKernelGGL(k_opt_result_b, dim3(1, L), dim3(64), 0, c->stream, d, s.stride, ll, d_states,
                       d_trace);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// What both lane initialisation calls check first (the context is not null).
static int check_opt_lanes_call(hpe_ctx *c, int P, int B, const double *d_states) {
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (!d_states) return fail(c, HPE_E_ARG, "null device states");
    if (!c->params) return fail(c, HPE_E_STATE, "hpe_set_pso_params not called");
    if (int rc = check_P(c, P)) return rc;
    if (check_hand_lanes(c, B)) return HPE_E_STATE;  // (its message stands)
    return HPE_OK;
}

int hpe_pso_optimise_batch(hpe_ctx *c, int P, int B, double *d_states, const int32_t *slots,
                           double *d_trace) {
    if (!c) return HPE_E_ARG;
    if (!slots) return fail(c, HPE_E_ARG, "null slots");
    int rc = check_opt_lanes_call(c, P, B, d_states);
    if (rc) return rc;
    int n_max = 0;
    for (int b = 0; b < B; ++b) {
        const int sl = slots[b];
        if (sl < 0 || sl >= (int)c->slots.size() || !c->slots[sl].valid)
            return fail(c, HPE_E_ARG, "lane %d: slot %d holds no frame", b, sl);
        const Slot &s = c->slots[sl];
        if (s.n_max > RF_STAGE_MAX)
            return fail(c, HPE_E_ARG, "lane %d: slot %d holds up to %d points, the lane form takes "
                        "the staged descent (<= %d)", b, sl, s.n_max, RF_STAGE_MAX);
        if (s.n_max > n_max) n_max = s.n_max;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int G = generations(c);
    if ((rc = ensure_opt_lanes(c, P, G, B))) return rc;
    for (int b = 0; b < B; ++b) {  // frames still being prepared on the preprocessing stream
        Slot &s = c->slots[slots[b]];
        if (s.dev && s.ready && hipEventQuery(s.ready) != hipSuccess)
            HIPCHK(c, hipStreamWaitEvent(c->stream, s.ready, 0));
    }
    BatchFirst first{};
    OptLaneList ll{};
    for (int b = 0; b < B; ++b) {
        first.slot[b] = slots[b];
        ll.lane[b] = b;
    }
    hipLaunchKernelGGL(k_opt_stage_b, dim3(1, B), dim3(64), 0, c->stream, (const DevObs *)c->d_obs,
                       first, c->optl.d_obs);
    if ((rc = enqueue_opt_lanes(c, P, G, c->optl.d_obs, ll, B, n_max, d_states, d_trace))) return rc;
    return mark_seq_done(c);  // the call is its slots' last reader
}

int hpe_batch_pipeline_optimise(hpe_ctx *c, int P, int B, double *d_states, uint32_t lanes,
                                double *d_trace) {
    if (!c) return HPE_E_ARG;
    int rc = check_opt_lanes_call(c, P, B, d_states);
    if (rc) return rc;
    if (!lanes || (B < 32 && lanes >> B))
        return fail(c, HPE_E_ARG, "lane mask 0x%x: empty, or a bit at or above B = %d", lanes, B);
    const hpe_ctx::LiveBatch &lv = c->live;
    if (lv.cur < 0)
        return fail(c, HPE_E_STATE, "no live batch: hpe_batch_pipeline_begin not called, or the "
                    "batch ended");
    if (B != lv.B)
        return fail(c, HPE_E_STATE, "%d lanes, the batch began with %d", B, lv.B);
    if (lanes & ~lv.pending)
        return fail(c, HPE_E_STATE, "lane mask 0x%x: lanes 0x%x hold no prepared frame "
                    "(hpe_batch_pending)", lanes, lanes & ~lv.pending);
    HIPCHK(c, hipSetDevice(c->device));
    const int G = generations(c);
    if ((rc = ensure_opt_lanes(c, P, G, B))) return rc;
    OptLaneList ll{};
    int L = 0;
    for (int b = 0; b < B; ++b)
        if (lanes >> b & 1) ll.lane[L++] = b;
    // the current frames' descriptors, as the next hpe_track_batch_pipelined reads them; every
    // live cloud is bounded by 250 points
    const DevObs *obs = c->rb.d_obs + lv.cur * HPE_BATCH_MAX;
    if ((rc = enqueue_opt_lanes(c, P, G, obs, ll, L, 250, d_states, d_trace))) return rc;
    if (!lv.report) return HPE_OK;
    // an INIT report of every selected lane: its new row, n of its prepared frame, the streak zeroed
    if ((rc = enqueue_report(c, B, d_states, lv.cur, nullptr, lanes, HPE_REPORT_INIT))) return rc;
    for (int b = 0; b < B; ++b) c->rep.enq[b] += lanes >> b & 1;
    return HPE_OK;
}

// ---------------------------------------------------------------- lane location
static const hpe_locate_params LOC_DEFAULTS = {
    {0, HPE_IMG_H - 1, 0, HPE_IMG_W - 1, -HUGE_VAL, HUGE_VAL}, 0.5, 12.0, 11.0, 11.0, 20, 200};

int hpe_locate_defaults(hpe_locate_params *p) {
    if (!p) return HPE_E_ARG;
    *p = LOC_DEFAULTS;
    return HPE_OK;
}

// One lane's parameters checked and in the kernel's form (sb = ceil(slab / bin), at most LOC_K).
static int locate_par(hpe_ctx *c, const hpe_locate_params &p, int lane, LocPar *out) {
    if (!(p.bin > 0) || std::isinf(p.bin))
        return fail(c, HPE_E_ARG, "lane %d: locate bin %g is not positive and finite", lane, p.bin);
    if (!(p.slab >= 0) || !(p.half_xy >= 0) || !(p.half_z >= 0) || std::isinf(p.slab) ||
        std::isinf(p.half_xy) || std::isinf(p.half_z))
        return fail(c, HPE_E_ARG, "lane %d: locate slab %g or half sizes %g, %g: negative or not "
                    "finite", lane, p.slab, p.half_xy, p.half_z);
    if (p.skip < 0 || p.min_pixels < 0)
        return fail(c, HPE_E_ARG, "lane %d: locate skip %d or min_pixels %d is negative", lane,
                    p.skip, p.min_pixels);
    const double sb = std::ceil(p.slab / p.bin);
    *out = LocPar{p.search.row_lo, p.search.row_hi, p.search.col_lo, p.search.col_hi,
                  p.search.z_lo, p.search.z_hi, p.bin, p.half_xy, p.half_z,
                  sb < (double)LOC_K ? (int)sb : LOC_K, p.skip, p.min_pixels, 0};
    return HPE_OK;
}

int hpe_locate_depth(hpe_ctx *c, const void *frame, int u16, float unit_mm, int to_cm, double focal,
                     const hpe_locate_params *params, hpe_locate *out) {
    if (!c) return HPE_E_ARG;
    if (!frame || !out) return fail(c, HPE_E_ARG, "null frame or result");
    if (!(focal > 0) || std::isinf(focal)) return fail(c, HPE_E_ARG, "focal %g is not positive and finite", focal);
    if (u16 && !(std::isfinite(unit_mm) && unit_mm > 0))
        return fail(c, HPE_E_ARG, "depth unit %g mm is not finite and positive", (double)unit_mm);
    LocLanes ln{};
    if (int rc = locate_par(c, params ? *params : LOC_DEFAULTS, 0, &ln.par[0])) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_locate(c)) return rc;
    hpe_ctx::Locate &lo = c->loc;
    const size_t bytes = (u16 ? sizeof(uint16_t) : sizeof(float)) * (size_t)HPE_IMG_H * HPE_IMG_W;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier call's kernel may still read the buffer
    HIPCHK(c, hipMemcpy(lo.d_frame, frame, bytes, hipMemcpyHostToDevice));
    ln.raw[0] = lo.d_frame;
    const float unit = u16 ? unit_mm : 1.f;
    // (entry HPE_BATCH_MAX of the record and activity tables: a live batch's entries stay as they are)
    const auto k_locate = u16 ? k_locate_b<true> : k_locate_b<false>;
    hipLaunchKernelGGL(k_locate, dim3(1), dim3(LOC_NT), 0, c->stream, ln, 1u, unit, to_cm ? 1 : 0, focal, (DevWindow *)nullptr, (DevWindow *)nullptr,
                       lo.d_act + HPE_BATCH_MAX, lo.d_res + HPE_BATCH_MAX,
                       (unsigned long long *)nullptr, (unsigned long long *)nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, lo.d_res + HPE_BATCH_MAX, sizeof(*out), hipMemcpyDeviceToHost));
    return HPE_OK;
}

int hpe_batch_pipeline_locate(hpe_ctx *c, int B, double *d_states, uint32_t lanes,
                              const double *tmpl, const hpe_locate_params *params) {
    if (!c) return HPE_E_ARG;
    if (B < 1 || B > HPE_BATCH_MAX)
        return fail(c, HPE_E_ARG, "batch of %d lanes out of range [1, %d]", B, HPE_BATCH_MAX);
    if (!d_states || !tmpl) return fail(c, HPE_E_ARG, "null device states or pose templates");
    if (!lanes || (B < 32 && lanes >> B))
        return fail(c, HPE_E_ARG, "lane mask 0x%x: empty, or a bit at or above B = %d", lanes, B);
    LocLanesView ln{};
    for (int b = 0; b < B; ++b)  // the selected lanes' entries alone are read
        if (lanes >> b & 1)
            if (int rc = locate_par(c, params ? params[b] : LOC_DEFAULTS, b, &ln.par[b])) return rc;
    hpe_ctx::LiveBatch &lv = c->live;
    if (lv.cur < 0)
        return fail(c, HPE_E_STATE, "no live batch: hpe_batch_pipeline_begin not called, or the "
                    "batch ended");
    if (B != lv.B) return fail(c, HPE_E_STATE, "%d lanes, the batch began with %d", B, lv.B);
    if (c->win.mode == HPE_WINDOW_OFF)
        return fail(c, HPE_E_STATE, "the lane windows are off: the located window would not be read "
                    "(hpe_set_batch_window before the begin)");
    if (lanes & ~lv.pending)
        return fail(c, HPE_E_STATE, "lane mask 0x%x: lanes 0x%x hold no prepared frame "
                    "(hpe_batch_pending)", lanes, lanes & ~lv.pending);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_locate(c)) return rc;
    hpe_ctx::Locate &lo = c->loc;
    const int cur = lv.cur, M = HPE_BATCH_MAX;
    // the lanes' current raw frames: the pinned buffers of the parity the next track call tracks
    for (int b = 0; b < B; ++b)
        if (lanes >> b & 1)  // (a cleaned batch: the lane's cleaned frame, a 240x320 u16 frame)
            ln.raw[b] = lv.clean ? (const void *)lv.stage(cur, b) : (const void *)lv.h_raw[cur][b].dev();
    DevWindow *const wcur = c->win.d_tab + cur * M;
    DevWindow *const woth = c->win.mode == HPE_WINDOW_FIXED ? c->win.d_tab + (cur ^ 1) * M : nullptr;
    if (lv.view && !lv.clean) {  // the lanes' camera frames, read through their views
        std::memcpy(ln.view, lv.views, sizeof(ln.view));
        hipLaunchKernelGGL((k_locate_b<true, true>), dim3(B), dim3(LOC_NT), 0, c->stream, ln,
                           (unsigned)lanes, lv.unit_mm, lv.to_cm, lv.focal, wcur, woth, lo.d_act.get(),
                           lo.d_res.get(), lo.d_seq.get(), (unsigned long long *)lo.h_tab.dev());
    } else {
        const auto k_locate = lv.u16 ? k_locate_b<true> : k_locate_b<false>;
        hipLaunchKernelGGL(k_locate, dim3(B), dim3(LOC_NT), 0, c->stream, (const LocLanes &)ln,
                           (unsigned)lanes, lv.unit_mm, lv.to_cm, lv.focal, wcur, woth, lo.d_act.get(),
                           lo.d_res.get(), lo.d_seq.get(), (unsigned long long *)lo.h_tab.dev());
    }
    HIPCHK(c, hipGetLastError());
    // the locate kernel is enqueued: it advances the selected lanes' device counters, and it and
    // the preparation below read the pinned buffers of parity cur in place, behind everything
    // already on the stream.  So those buffers stay in use until the NEXT track call's frame
    // (number enq + 1, whose launches follow these) has completed: the track call after it and
    // hpe_batch_frame_buffer wait for that number before the host refills them.
    for (int b = 0; b < B; ++b) lo.enq[b] += lanes >> b & 1;
    lv.used_seq[cur] = lv.enq + 1;
    // the found lanes' current frames prepared again through their new windows: the begin's
    // kernel in its windowed, idle-aware form, gated by the table the locate kernel filled
    hipLaunchKernelGGL(lane_prepare_kernel(lv.src(), true, true),
                       dim3(PREP_WG, B), dim3(PREP_NT), 0, c->stream,
                       lv.prep_tab() + cur * M, (const DevWindow *)wcur,
                       (const int *)lo.d_act, lv.unit_arg(),
                       (const float *const *)nullptr, (const int *)nullptr);
    LocTmpl tp{};
    std::memcpy(tp.th, tmpl, sizeof(double) * HPE_DOF * (size_t)B);
    hipLaunchKernelGGL(k_locate_place_b, dim3(B), dim3(64), 0, c->stream, tp,
                       (const DevHand *)c->d_lane_hands, (const hpe_locate *)lo.d_res,
                       (const int *)lo.d_act, d_states);
    HIPCHK(c, hipGetLastError());
    return HPE_OK;
}

// Result `seq` (>= 1) of a lane's host slot into *out: true iff the slot held exactly that
// result, complete, for the whole copy (hpe_report::read_seq's order).
static bool locate_read(const char *slot, uint64_t seq, hpe_locate *out) {
    const uint64_t *w = (const uint64_t *)slot;
    if (__atomic_load_n(w + 1 + LOC_WORDS, __ATOMIC_ACQUIRE) != seq) return false;
    uint64_t *o = (uint64_t *)out;
    for (int k = 0; k < LOC_WORDS; ++k) o[k] = __atomic_load_n(w + 1 + k, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return __atomic_load_n(w, __ATOMIC_RELAXED) == seq;
}

int hpe_batch_locate_result(hpe_ctx *c, int lane, int timeout_ms, hpe_locate *out) {
    if (!c) return HPE_E_ARG;
    if (!out) return fail(c, HPE_E_ARG, "null result");
    const hpe_ctx::Locate &lo = c->loc;
    if (!lo.B) return fail(c, HPE_E_STATE, "no live batch has begun (hpe_batch_pipeline_begin)");
    if (lane < 0 || lane >= lo.B)
        return fail(c, HPE_E_ARG, "lane %d outside the batch's %d lanes", lane, lo.B);
    const uint64_t seq = lo.enq[lane];
    if (!seq) {  // nothing was enqueued for the lane since the begin
        std::memset(out, 0, sizeof(*out));
        return HPE_OK;
    }
    const char *slot = lo.h_tab + (size_t)LOC_SLOT * lane;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (locate_read(slot, seq, out)) return HPE_OK;
        if ((it & 255) == 255) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms > 0 ? timeout_ms : 0))
                return fail(c, HPE_E_HIP, "lane %d: locate result %llu did not complete in %d ms", lane,
                            (unsigned long long)seq, timeout_ms);
            std::this_thread::yield();
        }
    }
}

int hpe_profile_enable(hpe_ctx *c, int on) {
    if (!c) return HPE_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &pl : c->pools) {
        if (on && pl.ev.empty()) {
            std::vector<Event> ev(2 * 8192);  // published whole
            for (auto &e : ev) HIPCHK(c, e.ensure(hipEventDefault));
            pl.ev = std::move(ev);
        }
        pl.used = 0;
    }
    c->prof = on != 0;
    return HPE_OK;
}

int hpe_profile_read_kernel(hpe_ctx *c, int kernel, int32_t *launches, double *total_ms,
                            double *min_ms, double *max_ms) {
    if (!c || !launches || !total_ms) return HPE_E_ARG;
    if (kernel < 0 || kernel >= HPE_PROF_KERNELS) return fail(c, HPE_E_ARG, "kernel id %d", kernel);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prep) HIPCHK(c, hipStreamSynchronize(c->prep));
    const hpe_ctx::Pool &pl = c->pools[kernel];
    double tot = 0, mn = 1e300, mx = 0;
    for (size_t k = 0; k + 1 < pl.used; k += 2) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, pl.ev[k], pl.ev[k + 1]));
        tot += ms;
        mn = ms < mn ? ms : mn;
        mx = ms > mx ? ms : mx;
    }
    *launches = (int32_t)(pl.used / 2);
    *total_ms = tot;
    if (min_ms) *min_ms = pl.used ? mn : 0;
    if (max_ms) *max_ms = mx;
    return HPE_OK;
}

int hpe_refine_eval_count(hpe_ctx *c, uint64_t *total, int reset) {
    if (!c || !total) return HPE_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    HIPCHK(c, hipMemcpy(&v, c->d_evals + 2, sizeof(v), hipMemcpyDeviceToHost));
    if (c->d_bevals) {  // the lanes of hpe_track_batch_dev count for themselves
        int lanes[HPE_BATCH_MAX * HPE_EVALS_N];
        HIPCHK(c, hipMemcpy(lanes, c->d_bevals, sizeof(lanes), hipMemcpyDeviceToHost));
        for (int b = 0; b < HPE_BATCH_MAX; ++b) {
            unsigned long long lv;
            std::memcpy(&lv, lanes + HPE_EVALS_N * b + 2, sizeof(lv));
            v += lv;
        }
        if (reset) HIPCHK(c, hipMemset(c->d_bevals, 0, sizeof(lanes)));
    }
    *total = v;
    if (reset) HIPCHK(c, hipMemset(c->d_evals + 2, 0, sizeof(v)));
    return HPE_OK;
}

int hpe_profile_read(hpe_ctx *c, int32_t *launches, double *total_ms, double *min_ms,
                     double *max_ms) {
    return hpe_profile_read_kernel(c, HPE_PROF_PSO_GEN, launches, total_ms, min_ms, max_ms);
}

int hpe_render_depth(hpe_ctx *c, const double theta[26], double focal, float *out) {
    if (!c) return HPE_E_ARG;
    if (!theta || !out) return fail(c, HPE_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_theta(c, 1);
    if (rc) return rc;
    if (!c->d_render) HIPCHK(c, c->d_render.alloc((size_t)HPE_IMG_H * HPE_IMG_W));
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * HPE_DOF, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_build, dim3(1), dim3(HPE_NT), 0, c->stream, c->d_theta, 1, c->d_hand,
                       c->d_S, (double *)nullptr);
    const int np = HPE_IMG_H * HPE_IMG_W;
    hipLaunchKernelGGL(k_render, dim3((np + 255) / 256), dim3(256), 0, c->stream, c->d_S,
                       c->d_hand, focal, c->d_render);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->d_render, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HPE_OK;
}

}  // extern "C"
