// own_check.cpp -- the resource owners of csrc/hpe_own.hpp and the all-or-nothing shapes the
// context's ensure_* functions build from them, on a fake allocator that counts what is live and
// can fail its n-th call.  Host only: no HIP runtime is linked (make own_check).
//
// Every shape is run with the failure injected at call 1, 2, ... until a run meets none.  After a
// failed run: the targets and the bookkeeping beside them are unchanged, or empty and zero; a retry
// succeeds.  At the end of every run nothing is live and nothing was freed twice.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <vector>

#include "hpe_own.hpp"

static int g_fail = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
            ++g_fail;                                                   \
        }                                                               \
    } while (0)

struct Fake {
    static inline std::set<void *> live;
    static inline int calls = 0, fail_at = 0, bad_free = 0;
    static inline size_t last_bytes = 0;
    static hipError_t make(void **p, size_t bytes) {
        last_bytes = bytes;
        if (++calls == fail_at) {
            *p = (void *)16;  // poison: an owner must not keep what a failed call left
            return hipErrorOutOfMemory;
        }
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        return hipSuccess;
    }
    static hipError_t drop(void *p) {
        if (!live.erase(p)) return ++bad_free, hipErrorInvalidValue;  // never made, or freed twice
        std::free(p);
        return hipSuccess;
    }
    static hipError_t dev_alloc(void **p, size_t bytes) { return make(p, bytes); }
    static hipError_t dev_free(void *p) { return drop(p); }
    static hipError_t host_alloc(void **p, size_t bytes, unsigned) { return make(p, bytes); }
    static hipError_t host_alias(void **d, void *h) {
        if (++calls == fail_at) return hipErrorInvalidValue;
        *d = h;
        return hipSuccess;
    }
    static hipError_t host_free(void *p) { return drop(p); }
    static hipError_t event_create(hipEvent_t *e, unsigned) { return make((void **)e, 1); }
    static hipError_t event_destroy(hipEvent_t e) { return drop((void *)e); }
    static hipError_t stream_create(hipStream_t *s, unsigned) { return make((void **)s, 1); }
    static hipError_t stream_destroy(hipStream_t s) { return drop((void *)s); }
};
template <typename T>
using Dev = DevBuf<T, Fake>;
template <typename T>
using Host = HostBuf<T, Fake>;
using Ev = EventOf<Fake>;
using St = StreamOf<Fake>;
static const unsigned MAPPED = hipHostMallocMapped | hipHostMallocCoherent;

static void clean(const char *what) {
    if (!Fake::live.empty() || Fake::bad_free) {
        std::printf("FAIL %s: %zu live, %d bad frees\n", what, Fake::live.size(), Fake::bad_free);
        ++g_fail;
    }
    Fake::bad_free = 0;
}

// run(t) on a fresh target from make(): with the failure at every call in turn; a failed run
// is checked by failed(t), then retried without a failure and checked by built(t).
template <typename Make, typename Run, typename Failed, typename Built>
static void inject(const char *what, Make make, Run run, Failed failed, Built built) {
    for (int at = 1;; ++at) {
        bool hit;
        {
            auto t = make();
            Fake::calls = 0;
            Fake::fail_at = at;
            const bool ok = run(t);
            hit = Fake::calls >= at;
            Fake::fail_at = 0;
            CHECK(ok == !hit);
            if (!ok) {
                failed(t);
                CHECK(run(t));
            }
            built(t);
        }
        clean(what);
        if (!hit) {
            std::printf("%-28s %2d failure points\n", what, at - 1);
            return;
        }
    }
}

struct SlotLike {  // Slot's owners
    Dev<double> cx, cy, cz, depth;
    Dev<float> dt;
    int cap = 0;
    bool valid = false;
    Ev ready, done;
};
static_assert(std::is_nothrow_move_constructible<SlotLike>::value, "vector growth moves");
static_assert(!std::is_copy_constructible<Dev<int>>::value && !std::is_copy_assignable<Dev<int>>::value, "");

// slot_buffers: the images once, the cloud grown, each group all or nothing
static bool slot_buffers(SlotLike &s, int need) {
    hipError_t e = s.depth ? hipSuccess : alloc_all(s.depth, 64, s.dt, 64);
    if (e != hipSuccess || need <= s.cap) return e == hipSuccess;
    s.cap = 0;
    s.valid = false;
    if ((e = alloc_all(s.cx, need, s.cy, need, s.cz, need)) == hipSuccess) s.cap = need;
    return e == hipSuccess;
}

static void owners() {
    {
        Dev<double> a;
        CHECK(!a && a.size() == 0);
        CHECK(a.alloc(0) == hipSuccess && a && a.size() == 0 && Fake::last_bytes == sizeof(double));
        CHECK(a.alloc(5) == hipSuccess && a.size() == 5 && Fake::last_bytes == 5 * sizeof(double));
        CHECK(Fake::live.size() == 1);  // the first allocation went when the second was made
        double *p = a;
        Dev<double> b(std::move(a));
        CHECK(!a && a.size() == 0 && b.get() == p && b.size() == 5);
        Dev<double> c;
        CHECK(c.alloc(3) == hipSuccess);
        c = std::move(b);  // frees c's own
        CHECK(!b && c.get() == p && c.size() == 5 && Fake::live.size() == 1);
        Dev<double> &self = c;
        c = std::move(self);
        CHECK(c.get() == p && c.size() == 5 && Fake::live.size() == 1);
        CHECK(c + 2 == p + 2);
        c.reset();
        c.reset();
        CHECK(!c && c.size() == 0 && Fake::live.empty());
        Fake::calls = 0, Fake::fail_at = 1;
        CHECK(c.alloc(4) != hipSuccess && !c && c.size() == 0);
        Fake::fail_at = 0;
    }
    clean("DevBuf");
    {
        Host<float> h, plain;
        CHECK(h.alloc(8, MAPPED) == hipSuccess && h.dev() == h.get() && h.size() == 8);
        CHECK(plain.alloc(8, 0) == hipSuccess && plain && !plain.dev());
        float *p = h;
        Host<float> g(std::move(h));
        CHECK(!h && !h.dev() && g.get() == p && g.dev() == p);
        plain = std::move(g);
        CHECK(plain.get() == p && plain.dev() == p && Fake::live.size() == 1);
        Host<float> &self = plain;
        plain = std::move(self);
        CHECK(plain.get() == p && plain.dev() == p && plain.size() == 8);
        for (int at = 1; at <= 2; ++at) {  // the allocation, then the alias: nothing kept
            Fake::calls = 0, Fake::fail_at = at;
            CHECK(h.alloc(2, MAPPED) != hipSuccess && !h && !h.dev() && Fake::live.size() == 1);
            Fake::fail_at = 0;
        }
        plain.reset();
        CHECK(!plain && !plain.dev() && Fake::live.empty());
    }
    clean("HostBuf");
    {
        Ev e;
        St s;
        CHECK(!e && !s);
        Fake::calls = 0;
        CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && e.ensure(hipEventDisableTiming) == hipSuccess);
        CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && Fake::calls == 2);  // created once
        hipEvent_t raw = e;
        Ev f(std::move(e));
        CHECK(!e && f.get() == raw);
        e = std::move(f);
        Ev &self = e;
        e = std::move(self);
        CHECK(e.get() == raw && Fake::live.size() == 2);
        Fake::calls = 0, Fake::fail_at = 1;
        CHECK(f.ensure(0) != hipSuccess && !f);
        Fake::fail_at = 0;
        e.reset();
        CHECK(!e && Fake::live.size() == 1);
    }
    clean("Event, Stream");
    {  // std::vector<Slot> grows by resize
        std::vector<SlotLike> v(1);
        for (int n = 1; n <= 40; ++n) {
            v.resize(n);
            CHECK(slot_buffers(v[n - 1], 10 + n) && v[n - 1].ready.ensure(0) == hipSuccess);
        }
        CHECK(Fake::live.size() == 40 * 6);
        for (int n = 0; n < 40; ++n) CHECK(v[n].cx && v[n].cap == 11 + n && v[n].ready);
    }
    clean("vector of slots");
}

struct Theta {  // ensure_theta: five buffers and a capacity, regrown in place
    Dev<double> theta, cost, terms, S, J;
    int cap = 0;
};
static bool ensure_theta(Theta &t, int P) {
    if (P <= t.cap) return true;
    t.cap = 0;
    if (alloc_all(t.theta, 26 * P, t.cost, P, t.terms, 3 * P, t.S, 144 * P, t.J, 63 * P) != hipSuccess)
        return false;
    t.cap = P;
    return true;
}

struct SwarmLike {  // ensure_swarm, ensure_opt: emptied, built in a local, moved in whole
    int P = 0;
    Dev<double> xh, inbox;
    Dev<int> outl;
    Dev<char> arena;
};
static bool ensure_swarm(SwarmLike &dst, int P) {
    if (dst.P == P) return true;
    dst = SwarmLike{};
    SwarmLike s;
    if (alloc_all(s.xh, 26 * P, s.inbox, 4 * P) != hipSuccess) return false;
    if (s.outl.alloc(P) != hipSuccess) return false;
    s.P = P;
    dst = std::move(s);
    return true;
}

struct PipeLike {  // ensure_pipe and the other first-time blocks: guarded by the owner assigned last
    Dev<int> d_obs, d_info, d_split;
    Host<unsigned long long> h_done;
    Host<float> h_raw[2];
    Ev used[2];
    St copy;
};
static bool ensure_pipe(PipeLike &p) {
    if (p.d_obs) return true;
    Dev<int> obs;
    bool ok = obs.alloc(2) == hipSuccess && p.d_info.alloc(2) == hipSuccess &&
              p.copy.ensure(hipStreamNonBlocking) == hipSuccess && p.d_split.alloc(4) == hipSuccess &&
              p.h_done.alloc(1, MAPPED) == hipSuccess;
    for (int k = 0; ok && k < 2; ++k)
        ok = p.h_raw[k].alloc(100, MAPPED) == hipSuccess && p.used[k].ensure(hipEventDisableTiming) == hipSuccess;
    if (ok) p.d_obs = std::move(obs);
    return ok;
}

struct RingLike {  // ensure_live_batch's lanes: a lane counts once both its pinned buffers are there
    Host<float> h_raw[2][4];
    int lanes = 0;
};
static bool ensure_ring(RingLike &r, int B) {
    for (; r.lanes < B; ++r.lanes)
        for (int p = 0; p < 2; ++p)
            if (!r.h_raw[p][r.lanes] && r.h_raw[p][r.lanes].alloc(100, MAPPED) != hipSuccess) return false;
    return true;
}

struct PoolLike {  // hpe_profile_enable: the events made before the vector is published
    std::vector<Ev> ev;
};
static bool enable(PoolLike &pl) {
    if (!pl.ev.empty()) return true;
    std::vector<Ev> ev(6);
    for (auto &e : ev)
        if (e.ensure(hipEventDefault) != hipSuccess) return false;
    pl.ev = std::move(ev);
    return true;
}

int main() {
    owners();
    const auto theta_empty = [](Theta &t) { CHECK(!t.theta && !t.cost && !t.terms && !t.S && !t.J && t.cap == 0); };
    const auto theta_built = [](Theta &t) { CHECK(t.theta && t.cost && t.terms && t.S && t.J && t.cap == 8 && t.J.size() == 63 * 8); };
    inject("ensure_theta, first", [] { return Theta{}; }, [](Theta &t) { return ensure_theta(t, 8); }, theta_empty, theta_built);
    inject("ensure_theta, grown", [] { Theta t; CHECK(ensure_theta(t, 2)); return t; },
           [](Theta &t) { return ensure_theta(t, 8); }, theta_empty, theta_built);
    const auto slot_failed = [](SlotLike &s) {
        CHECK(!s.depth == !s.dt);  // the images: both or neither
        CHECK(!s.cx && !s.cy && !s.cz && s.cap == 0 && !s.valid);
    };
    const auto slot_built = [](SlotLike &s) { CHECK(s.depth && s.dt && s.cx && s.cy && s.cz && s.cap == 250); };
    inject("slot_buffers, first", [] { return SlotLike{}; }, [](SlotLike &s) { return slot_buffers(s, 250); }, slot_failed, slot_built);
    inject("slot_buffers, grown", [] { SlotLike s; CHECK(slot_buffers(s, 20)); s.valid = true; return s; },
           [](SlotLike &s) { return slot_buffers(s, 250); }, slot_failed, slot_built);
    const auto swarm_empty = [](SwarmLike &s) { CHECK(!s.xh && !s.inbox && !s.outl && !s.arena && s.P == 0); };
    const auto swarm_built = [](SwarmLike &s) { CHECK(s.xh && s.inbox && s.outl && s.P == 16); };
    inject("ensure_swarm, first", [] { return SwarmLike{}; }, [](SwarmLike &s) { return ensure_swarm(s, 16); }, swarm_empty, swarm_built);
    inject("ensure_swarm, rebuilt", [] { SwarmLike s; CHECK(ensure_swarm(s, 4) && s.arena.alloc(9) == hipSuccess); return s; },
           [](SwarmLike &s) { return ensure_swarm(s, 16); }, swarm_empty, swarm_built);
    inject("first-time block (pipe)", [] { return PipeLike{}; }, ensure_pipe,
           [](PipeLike &p) { CHECK(!p.d_obs); },  // the guard: the block runs again in full
           [](PipeLike &p) {
               CHECK(p.d_obs && p.d_info && p.d_split && p.h_done.dev() && p.copy);
               for (int k = 0; k < 2; ++k) CHECK(p.h_raw[k].dev() && p.used[k]);
           });
    inject("pinned ring lanes", [] { RingLike r; CHECK(ensure_ring(r, 1)); return r; },
           [](RingLike &r) { return ensure_ring(r, 3); },
           [](RingLike &r) { CHECK(r.lanes >= 1 && r.lanes < 3 && r.h_raw[0][0] && r.h_raw[1][0]); },
           [](RingLike &r) {
               CHECK(r.lanes == 3);
               for (int b = 0; b < 3; ++b) CHECK(r.h_raw[0][b].dev() && r.h_raw[1][b].dev());
           });
    inject("profile pool", [] { return PoolLike{}; }, enable, [](PoolLike &p) { CHECK(p.ev.empty()); },
           [](PoolLike &p) {
               CHECK(p.ev.size() == 6);
               for (auto &e : p.ev) CHECK(e);
           });
    if (g_fail) return std::printf("own_check: %d failures\n", g_fail), 1;
    std::printf("own_check: ok\n");
    return 0;
}
