// report_ring_host.cpp -- the lane reports' host reader (csrc/hpe_report.hpp) against a writer
// that plays k_report_b's publication order from a second host thread: begin = seq, release,
// the payload, release, end = seq.  Stand-alone (no GPU, no HIP): it checks the newest-report
// rule, the overwritten-slot rule, and that a half-written slot (begin != end) is never returned.
// Every payload word of report seq is word_of(seq, k), so a copy mixed from two reports shows.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "hpe_report.hpp"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);          \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint64_t word_of(uint64_t seq, int k) { return k == 0 ? seq : seq * 1000003ull + (uint64_t)k; }

static uint64_t *slot_of(std::vector<uint64_t> &ring, int depth, uint64_t seq) {
    return ring.data() + (size_t)((seq - 1) % (uint64_t)depth) * (HPE_REP_SLOT / 8);
}
// the writer's order; stop_after: leave the slot half written after that many payload words
static void write_report(std::vector<uint64_t> &ring, int depth, uint64_t seq, int stop_after = -1) {
    uint64_t *w = slot_of(ring, depth, seq);
    __atomic_store_n(w, seq, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    for (int k = 0; k < HPE_REP_WORDS; ++k) {
        if (k == stop_after) return;
        __atomic_store_n(w + 1 + k, word_of(seq, k), __ATOMIC_RELAXED);
    }
    if (stop_after >= 0) return;
    __atomic_store_n(w + 1 + HPE_REP_WORDS, seq, __ATOMIC_RELEASE);
}
static bool whole(const hpe_lane_report &r, uint64_t seq) {
    uint64_t v[HPE_REP_WORDS];
    std::memcpy(v, &r, sizeof(v));
    for (int k = 0; k < HPE_REP_WORDS; ++k)
        if (v[k] != word_of(seq, k)) return false;
    return true;
}

static void quiescent(int depth, int n) {
    std::vector<uint64_t> ring((size_t)depth * (HPE_REP_SLOT / 8), 0);
    hpe_lane_report r;
    CHECK(hpe_report::read_newest(ring.data(), depth, &r) == 0 && r.seq == 0);  // an empty ring
    CHECK(!hpe_report::read_seq(ring.data(), depth, 1, &r));
    CHECK(!hpe_report::read_seq(ring.data(), depth, 0, &r));
    for (int s = 1; s <= n; ++s) {
        write_report(ring, depth, (uint64_t)s);
        // the newest-report rule
        CHECK(hpe_report::read_newest(ring.data(), depth, &r) == (uint64_t)s && whole(r, (uint64_t)s));
        // the ring holds the last `depth` reports and no other: not yet, and no longer
        for (int q = s; q > s - depth && q >= 1; --q)
            CHECK(hpe_report::read_seq(ring.data(), depth, (uint64_t)q, &r) && whole(r, (uint64_t)q));
        CHECK(!hpe_report::read_seq(ring.data(), depth, (uint64_t)s + 1, &r));
        if (s - depth >= 1) CHECK(!hpe_report::read_seq(ring.data(), depth, (uint64_t)(s - depth), &r));
    }
}

static void half_written() {
    const int depth = 2;
    std::vector<uint64_t> ring((size_t)depth * (HPE_REP_SLOT / 8), 0);
    hpe_lane_report r;
    for (uint64_t s = 1; s <= 5; ++s) write_report(ring, depth, s);  // slot 0: 5, slot 1: 4
    for (int stop : {0, 1, 70, HPE_REP_WORDS}) {
        write_report(ring, depth, 4);           // slot 1 whole again
        write_report(ring, depth, 6, stop);     // ... and half overwritten: begin 6, end 4
        CHECK(!hpe_report::read_seq(ring.data(), depth, 4, &r));
        CHECK(!hpe_report::read_seq(ring.data(), depth, 6, &r));
        CHECK(hpe_report::read_newest(ring.data(), depth, &r) == 5 && whole(r, 5));
    }
    write_report(ring, depth, 7, 3);  // both slots half written: nothing to return
    CHECK(hpe_report::read_newest(ring.data(), depth, &r) == 0 && r.seq == 0);
    write_report(ring, depth, 6);
    CHECK(hpe_report::read_newest(ring.data(), depth, &r) == 6 && whole(r, 6));
    // an end word that does not belong to its slot is no candidate
    std::vector<uint64_t> odd((size_t)depth * (HPE_REP_SLOT / 8), 0);
    odd[0] = 2;
    odd[1 + HPE_REP_WORDS] = 2;  // report 2 lives in slot 1, not 0
    CHECK(hpe_report::read_newest(odd.data(), depth, &r) == 0);
}

static void concurrent(int depth, uint64_t n) {
    std::vector<uint64_t> ring((size_t)depth * (HPE_REP_SLOT / 8), 0);
    std::atomic<bool> done{false};
    std::thread writer([&] {
        for (uint64_t s = 1; s <= n; ++s) write_report(ring, depth, s);
        done.store(true, std::memory_order_release);
    });
    hpe_lane_report r;
    uint64_t last = 0, got = 0, by_seq = 0;
    for (bool fin = false; !fin;) {
        fin = done.load(std::memory_order_acquire);
        const uint64_t s = hpe_report::read_newest(ring.data(), depth, &r);
        if (s) {
            ++got;
            CHECK(whole(r, s));  // never a mix of two reports
            CHECK(s >= last);    // the newest never goes back
            last = s;
            if (s > 1 && hpe_report::read_seq(ring.data(), depth, s - 1, &r)) {
                ++by_seq;
                CHECK(whole(r, s - 1));
            }
        } else {
            CHECK(r.seq == 0);
        }
    }
    writer.join();
    CHECK(hpe_report::read_newest(ring.data(), depth, &r) == n && whole(r, n));
    CHECK(got > 0);
    std::printf("depth %d: %llu reports written, %llu newest reads, %llu reads by seq\n", depth,
                (unsigned long long)n, (unsigned long long)got, (unsigned long long)by_seq);
}

int main() {
    static_assert(sizeof(hpe_lane_report) == 1096, "hpe_lane_report");
    for (int depth : {2, 3, 4, 64}) quiescent(depth, 3 * depth + 1);
    half_written();
    concurrent(2, 200000);
    concurrent(5, 200000);
    std::printf(fails ? "report ring: %d checks failed\n" : "report ring: ok\n", fails);
    return fails ? 1 : 0;
}
