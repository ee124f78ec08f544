// devres.hpp -- the device resources the host side holds, each owned by a type: device memory (DevBuf), an event (DevEvent),
// pinned host memory (PinnedBuf), the stream (DevStream), a camera-key slot (CamSlot).  Every one is empty when default
// constructed, gives its resource back in its destructor and on release(), and moves but does not copy; a moved-from value is
// empty.  So a struct made of them -- CrHandle, DevScene, SahDeviceWork, a function's locals -- needs no list of what to free,
// and these are the only places in the library that free, destroy, allocate or create one of these resources.  Reads the HIP
// runtime's declarations alone, so a stand-in for them lets a CPU program check all of it (tests/handle_lifetime_check.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace cr {

struct DevBuf {
    void* p = nullptr;      // what users address: raw + pad
    void* raw = nullptr;    // the allocation (hipMalloc aligns it to 256 bytes); nullptr with p set: borrowed, see borrow()
    size_t bytes = 0, pad = 0;
    // pad: bytes skipped at the front, so that p is deliberately MISaligned by that much (see entry_pad)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), raw(o.raw), bytes(o.bytes), pad(o.pad) { o.forget(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; raw = o.raw; bytes = o.bytes; pad = o.pad; o.forget(); }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n, size_t front_pad = 0) {
        if (n <= bytes && front_pad == pad) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&raw, n + front_pad);
        if (e == hipSuccess) { bytes = n; pad = front_pad; p = (char*)raw + front_pad; }
        else raw = nullptr;
        return e;
    }
    void release() { if (raw) (void)hipFree(raw); forget(); }
    // The lender's block under this name too: same p, bytes and pad, owning nothing -- release(), the destructor and an
    // ensure() that has to reallocate leave the lender's block alone.  The lender must outlive the use.
    void borrow(const DevBuf& lender) { release(); p = lender.p; bytes = lender.bytes; pad = lender.pad; }
private:
    void forget() { p = raw = nullptr; bytes = 0; pad = 0; }
};

struct DevEvent {
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { release(); ev = o.ev; o.ev = nullptr; } return *this; }
    ~DevEvent() { release(); }
    hipError_t create(unsigned flags = hipEventDefault) {   // once: a later call does nothing
        if (ev) return hipSuccess;
        hipError_t e = flags == hipEventDefault ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, flags);
        if (e != hipSuccess) ev = nullptr;
        return e;
    }
    void release() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    operator hipEvent_t() const { return ev; }
    explicit operator bool() const { return ev != nullptr; }
private:
    hipEvent_t ev = nullptr;
};

struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    hipError_t ensure(size_t n, unsigned flags = hipHostMallocDefault) {   // grow-only; left empty on failure
        if (n <= bytes) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(&p, n, flags);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

struct DevStream {
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    DevStream(DevStream&& o) noexcept : s(o.s) { o.s = nullptr; }
    DevStream& operator=(DevStream&& o) noexcept { if (this != &o) { release(); s = o.s; o.s = nullptr; } return *this; }
    ~DevStream() { release(); }
    hipError_t create(unsigned flags) {   // once: a later call does nothing
        if (s) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e != hipSuccess) s = nullptr;
        return e;
    }
    void release() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    operator hipStream_t() const { return s; }
    explicit operator bool() const { return s != nullptr; }
private:
    hipStream_t s = nullptr;
};

// A render's camera keyframes travel through a slot: pinned host memory that is filled, its device copy, and the event that
// says the copy has run (CrHandle::cam).
struct CamSlot {
    PinnedBuf host;
    DevBuf dev;
    DevEvent ev;
    // the slot's three resources together, or none of them: after a failure the slot is empty and a later call tries again
    hipError_t acquire(size_t bytes) {
        hipError_t e = host.ensure(bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = dev.ensure(bytes);
        if (e == hipSuccess) e = ev.create(hipEventDisableTiming);
        if (e != hipSuccess) release();
        return e;
    }
    void release() { host.release(); dev.release(); ev.release(); }
    explicit operator bool() const { return host.p != nullptr; }
};

}   // namespace cr
