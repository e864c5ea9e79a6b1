// hpe_own.hpp -- move-only owners of the context's GPU resources (host only: the HIP runtime
// API header and the standard library).  A member of one of these types is released by its
// destructor, so hpe_ctx keeps no list of what to free.  The allocator is a policy parameter
// (default: HIP); tools/own_check.cpp substitutes a counting fake and runs the owners and the
// two all-or-nothing helpers at the end of this file on the CPU.
#pragma once
#include <cstddef>
#include <utility>

#include <hip/hip_runtime_api.h>

struct HipAlloc {
    static hipError_t dev_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t dev_free(void *p) { return hipFree(p); }
    static hipError_t host_alloc(void **p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static hipError_t host_alias(void **d, void *h) { return hipHostGetDevicePointer(d, h, 0); }
    static hipError_t host_free(void *p) { return hipHostFree(p); }
    static hipError_t event_create(hipEvent_t *e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
    static hipError_t event_destroy(hipEvent_t e) { return hipEventDestroy(e); }
    static hipError_t stream_create(hipStream_t *s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
    static hipError_t stream_destroy(hipStream_t s) { return hipStreamDestroy(s); }
};

// Device memory of n elements (0 elements allocate 1).  Converts to T *, so pointer arithmetic,
// null tests and copies read as on a bare pointer; not copyable, so a launch that would take it
// by value says .get().
template <typename T, typename A = HipAlloc>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (&o != this) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n) {  // the old memory goes first; empty after a failure
        reset();
        const hipError_t e = A::dev_alloc((void **)&p_, sizeof(T) * (n ? n : 1));
        if (e == hipSuccess) n_ = n;
        else p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)A::dev_free((void *)p_);
        p_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    operator T *() const { return p_; }
};

// Pinned host memory with the hipHostMalloc flags; with hipHostMallocMapped among them, dev() is
// its device alias, fetched in the same alloc.
template <typename T, typename A = HipAlloc>
class HostBuf {
    T *p_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;

public:
    HostBuf() = default;
    HostBuf(HostBuf &&o) noexcept
        : p_(std::exchange(o.p_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    HostBuf &operator=(HostBuf &&o) noexcept {
        if (&o != this) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            dev_ = std::exchange(o.dev_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~HostBuf() { reset(); }
    hipError_t alloc(size_t n, unsigned flags) {
        reset();
        hipError_t e = A::host_alloc((void **)&p_, sizeof(T) * (n ? n : 1), flags);
        if (e != hipSuccess) p_ = nullptr;
        else if (flags & hipHostMallocMapped) e = A::host_alias((void **)&dev_, (void *)p_);
        if (e == hipSuccess) n_ = n;
        else reset();
        return e;
    }
    void reset() {
        if (p_) (void)A::host_free((void *)p_);
        p_ = dev_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    T *dev() const { return dev_; }
    size_t size() const { return n_; }
    operator T *() const { return p_; }
};

// An event or a stream, created at first use by ensure(flags) and destroyed, never synchronised,
// by the destructor.
template <typename H, hipError_t (*Create)(H *, unsigned), hipError_t (*Destroy)(H)>
class Handle {
    H h_ = nullptr;

public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        if (&o != this) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    hipError_t ensure(unsigned flags) {
        if (h_) return hipSuccess;
        const hipError_t e = Create(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
};
template <typename A = HipAlloc>
using EventOf = Handle<hipEvent_t, A::event_create, A::event_destroy>;
template <typename A = HipAlloc>
using StreamOf = Handle<hipStream_t, A::stream_create, A::stream_destroy>;
using Event = EventOf<>;
using Stream = StreamOf<>;

// All or nothing, for a run of device buffers: alloc_all(a, na, b, nb, ...) allocates them in that
// order, and after the first failure every one of them is empty -- the caller zeroes the capacity
// it keeps beside them before the call and sets it after.
inline void reset_all() {}
template <typename B, typename... Rest>
void reset_all(B &b, size_t, Rest &&...rest) {
    b.reset();
    reset_all(rest...);
}
inline hipError_t alloc_all() { return hipSuccess; }
template <typename B, typename... Rest>
hipError_t alloc_all(B &b, size_t n, Rest &&...rest) {
    hipError_t e = b.alloc(n);
    if (e == hipSuccess) e = alloc_all(rest...);
    if (e != hipSuccess) reset_all(b, n, rest...);
    return e;
}

// All or nothing, for a block that also creates pinned memory and events or fills what it
// allocates: fill(fresh) builds a new T and returns 0 on success, and only then does it replace
// dst -- after a failure dst is as it was and everything fill made is released.
template <typename T, typename F>
auto build_into(T &dst, F fill) -> decltype(fill(dst)) {
    T fresh;
    const auto rc = fill(fresh);
    if (!rc) dst = std::move(fresh);
    return rc;
}
