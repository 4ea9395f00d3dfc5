// lpc_resource.hpp -- move-only owners of the runtime's GPU resources: device
// memory, pinned host memory, streams and events.  A resource is released by
// its owner's destructor and nowhere else, so a struct that holds owners (the
// handle, a population, a staged batch, a device-resident source) needs no
// release code of its own: adding a member is all it takes.
//
// The device and pinned bytes the owners hold are counted process-wide
// (lpc_debug_live_bytes): two relaxed atomic adds per allocation, none per
// launch.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace lpcr {

inline std::atomic<int64_t> g_device_bytes{0};   // held by DBuf
inline std::atomic<int64_t> g_pinned_bytes{0};   // held by Pinned

// A block of device memory (hipMalloc / hipFree).
struct DBuf {
    void *p = nullptr;
    size_t bytes = 0;

    DBuf() = default;
    DBuf(DBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DBuf &operator=(DBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p; bytes = o.bytes;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~DBuf() { reset(); }

    // a fresh block of n bytes; the old one goes first
    hipError_t alloc(size_t n)
    {
        reset();
        const hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = n;
        g_device_bytes.fetch_add((int64_t)n, std::memory_order_relaxed);
        return hipSuccess;
    }
    void reset()
    {
        if (p) {
            (void)hipFree(p);
            g_device_bytes.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
        }
        p = nullptr;
        bytes = 0;
    }
};

// A block of pinned host memory (hipHostMalloc / hipHostFree) holding T's.
template <class T>
struct Pinned {
    T *p = nullptr;
    size_t bytes = 0;

    Pinned() = default;
    Pinned(Pinned &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Pinned &operator=(Pinned &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p; bytes = o.bytes;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~Pinned() { reset(); }
    operator T *() const { return p; }

    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault)
    {
        reset();
        const hipError_t e = hipHostMalloc((void **)&p, n, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = n;
        g_pinned_bytes.fetch_add((int64_t)n, std::memory_order_relaxed);
        return hipSuccess;
    }
    void reset()
    {
        if (p) {
            (void)hipHostFree((void *)p);
            g_pinned_bytes.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
        }
        p = nullptr;
        bytes = 0;
    }
};

// A stream; reads as the raw hipStream_t wherever one is expected.
struct Stream {
    hipStream_t s = nullptr;

    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) { reset(); s = o.s; o.s = nullptr; }
        return *this;
    }
    ~Stream() { reset(); }
    operator hipStream_t() const { return s; }

    hipError_t create(unsigned flags = hipStreamNonBlocking)
    {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e != hipSuccess) s = nullptr;
        return e;
    }
    void reset()
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};

// An event; reads as the raw hipEvent_t wherever one is expected.
struct Event {
    hipEvent_t e = nullptr;

    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return e; }

    hipError_t create(unsigned flags = hipEventDisableTiming)
    {
        reset();
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess) e = nullptr;
        return rc;
    }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};

}  // namespace lpcr
