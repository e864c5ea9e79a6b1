// hpe_report.hpp -- the lane reports' ring layout and its HOST reader (no HIP types: the
// kernels, the C ABI and a stand-alone host test include it).
//
// A lane's ring is `depth` slots of HPE_REP_SLOT bytes in pinned, mapped, coherent host memory;
// slot (seq - 1) % depth holds the lane's report number seq (from 1):
//     u64 begin | hpe_lane_report (1096 bytes = 137 words) | u64 end | padding to 1152
// The writer (k_report_b, one wave per slot) follows the seqlock writer's order: begin = seq,
// release, the payload, release, end = seq.  The reader runs it backwards: an acquire load of
// end, the payload, an acquire fence, begin -- the copy is report `seq` iff both words equal
// seq.  (end == seq: every payload store of seq is visible; begin == seq after the copy: no
// later report had started to overwrite it.)  The payload is copied as relaxed 8-byte atomic
// loads: a copy that races with the writer is discarded, never undefined.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hpe.h"

#define HPE_REP_WORDS 137    // sizeof(hpe_lane_report) / 8
#define HPE_REP_SLOT 1152    // 8 + 1096 + 8, padded to a multiple of 128
#define HPE_REP_DEPTH_MAX 64
static_assert(sizeof(hpe_lane_report) == 8 * HPE_REP_WORDS, "hpe_lane_report is 1096 bytes");
static_assert(offsetof(hpe_lane_report, state) == 40 && offsetof(hpe_lane_report, joints) == 256 &&
              offsetof(hpe_lane_report, px) == 760, "hpe_lane_report's layout (include/hpe.h)");
static_assert(HPE_REP_SLOT % 128 == 0 && HPE_REP_SLOT >= 8 * (HPE_REP_WORDS + 2), "slot size");

namespace hpe_report {

inline const uint64_t *slot_words(const void *ring, int slot) {
    return (const uint64_t *)((const char *)ring + (size_t)HPE_REP_SLOT * slot);
}

// Report `seq` (>= 1) of a ring of `depth` slots into *out: true iff the slot held exactly that
// report, complete, for the whole copy.
inline bool read_seq(const void *ring, int depth, uint64_t seq, hpe_lane_report *out) {
    if (seq == 0) return false;
    const uint64_t *w = slot_words(ring, (int)((seq - 1) % (uint64_t)depth));
    if (__atomic_load_n(w + 1 + HPE_REP_WORDS, __ATOMIC_ACQUIRE) != seq) return false;
    uint64_t *o = (uint64_t *)out;
    for (int k = 0; k < HPE_REP_WORDS; ++k) o[k] = __atomic_load_n(w + 1 + k, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return __atomic_load_n(w, __ATOMIC_RELAXED) == seq;
}

// The newest complete report of the ring into *out; its seq, or 0 (and out->seq = 0) if the ring
// holds none.  Candidates are the slots' end words, newest first: the slot a writer is inside
// still carries the end word of the report it overwrites, fails its check and yields to the
// report before it.
inline uint64_t read_newest(const void *ring, int depth, hpe_lane_report *out) {
    uint64_t cand[HPE_REP_DEPTH_MAX];
    int nc = 0;
    for (int s = 0; s < depth; ++s) {
        const uint64_t e = __atomic_load_n(slot_words(ring, s) + 1 + HPE_REP_WORDS, __ATOMIC_ACQUIRE);
        if (e && (int)((e - 1) % (uint64_t)depth) == s) cand[nc++] = e;
    }
    while (nc) {
        int m = 0;
        for (int k = 1; k < nc; ++k)
            if (cand[k] > cand[m]) m = k;
        if (read_seq(ring, depth, cand[m], out)) return cand[m];
        cand[m] = cand[--nc];
    }
    out->seq = 0;
    return 0;
}

}  // namespace hpe_report
