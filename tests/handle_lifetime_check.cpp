// handle_lifetime_check.cpp -- the owning types of crucible_amd/csrc/devres.hpp and the whole CrHandle of handle.hpp, run on the
// CPU against tests/hip_stub/hip/hip_runtime.h, which counts what is live and logs every call.  Built and run by
// tests/test_handle_lifetime_host.py (g++ -fsanitize=address,undefined); that test also writes handle_touch.inc, the code that
// touches every owning member of CrHandle as it found them in handle.hpp.  Prints one "ok <section>" line per section; the
// first check that fails prints its line and ends the program with status 1.
#include "handle.hpp"

#include <cstdio>
#include <set>
#include <vector>

using namespace hip_stub;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static size_t mark() { return state().log.size(); }                       // a place in the log
static size_t calls_since(size_t m) { return state().log.size() - m; }
static bool empty(const DevBuf& b) { return !b.p && !b.raw && b.bytes == 0 && b.pad == 0; }

// What the stub's counter is worth: a block nobody owns stays live
struct RawScratch { void* p = nullptr; };

static void check_devbuf() {
    size_t at_scope_end;
    {
        DevBuf b;
        CHECK(empty(b));
        size_t m = mark();
        CHECK(b.ensure(100) == hipSuccess && b.bytes == 100 && b.pad == 0 && b.p && b.p == b.raw);
        CHECK(calls_since(m) == 1 && calls("hipMalloc", m) == 1 && live(kDevice) == 1);
        m = mark();
        CHECK(b.ensure(100) == hipSuccess && calls_since(m) == 0);           // same size and pad: no HIP call at all
        CHECK(b.ensure(40) == hipSuccess && calls_since(m) == 0 && b.bytes == 100);   // a smaller request: the early return
        CHECK(b.ensure(200) == hipSuccess && b.bytes == 200);                // larger: frees once, then allocates once
        CHECK(calls_since(m) == 2 && state().log[m].name == "hipFree" && state().log[m + 1].name == "hipMalloc" && live(kDevice) == 1);
        m = mark();
        CHECK(b.ensure(200, 32) == hipSuccess && calls_since(m) == 2);       // a changed front_pad reallocates
        CHECK(b.pad == 32 && b.bytes == 200 && b.p == (char*)b.raw + 32 && live(kDevice) == 1);
        m = mark();
        CHECK(b.ensure(64, 32) == hipSuccess && calls_since(m) == 0);
        b.release();
        CHECK(empty(b) && live() == 0 && calls_since(m) == 1);
        b.release();                                                         // twice is harmless
        CHECK(empty(b) && calls_since(m) == 1);
        CHECK(b.ensure(8) == hipSuccess);
        at_scope_end = mark();
    }                                                                        // the destructor frees exactly once
    CHECK(live() == 0 && calls_since(at_scope_end) == 1 && calls("hipFree", at_scope_end) == 1);
    {   // negative control
        RawScratch s;
        CHECK(hipMalloc(&s.p, 8) == hipSuccess);
        RawScratch gone = s;
        s = RawScratch();
        CHECK(live(kDevice) == 1);                                           // the counter sees the leak
        CHECK(hipFree(gone.p) == hipSuccess && live() == 0);
    }
    {   // a failed ensure leaves the buffer empty and nothing live
        DevBuf b;
        fail_nth_allocation(1);
        CHECK(b.ensure(16) == hipErrorOutOfMemory && empty(b) && live() == 0);
        CHECK(b.ensure(16) == hipSuccess);
        fail_nth_allocation(1);
        CHECK(b.ensure(32, 8) == hipErrorOutOfMemory && empty(b) && live() == 0);   // what it held went first
        CHECK(hipGetLastError() == hipErrorOutOfMemory && hipGetLastError() == hipSuccess);
    }
    {   // moves
        DevBuf a;
        CHECK(a.ensure(48, 16) == hipSuccess);
        void* const p = a.p; void* const raw = a.raw;
        size_t m = mark();
        DevBuf b(std::move(a));
        CHECK(empty(a) && b.p == p && b.raw == raw && b.bytes == 48 && b.pad == 16 && calls_since(m) == 0);
        DevBuf c;
        CHECK(c.ensure(24) == hipSuccess && live(kDevice) == 2);
        m = mark();
        c = std::move(b);                                                    // frees what the target held
        CHECK(empty(b) && c.raw == raw && c.bytes == 48 && calls_since(m) == 1 && calls("hipFree", m) == 1 && live(kDevice) == 1);
        DevBuf& self = c;
        m = mark();
        c = std::move(self);                                                 // self-move is safe
        CHECK(c.raw == raw && c.p == p && c.bytes == 48 && c.pad == 16 && calls_since(m) == 0);
    }
    CHECK(live() == 0);
    {   // std::vector<DevBuf>, as the group keeps its per-member buffers
        std::vector<DevBuf> v;
        v.resize(3);
        for (DevBuf& b : v) CHECK(b.ensure(10) == hipSuccess);
        void* const first = v[0].p;
        v.resize(50);                                                        // moves the three
        CHECK(v[0].p == first && v[2].bytes == 10 && empty(v[49]) && live(kDevice) == 3);
        CHECK(v[40].ensure(10) == hipSuccess && live(kDevice) == 4);
        v.resize(2);
        CHECK(live(kDevice) == 2);
    }
    CHECK(live() == 0);
    {   // a borrower never frees the lender's block
        DevBuf lender;
        CHECK(lender.ensure(64, 16) == hipSuccess);
        size_t m = mark();
        {
            DevBuf b;
            b.borrow(lender);
            CHECK(b.p == lender.p && b.bytes == 64 && b.pad == 16 && !b.raw);
        }                                                                    // its destruction
        CHECK(calls_since(m) == 0 && live(kDevice) == 1);
        DevBuf b;
        b.borrow(lender);
        b.release();                                                         // its release
        CHECK(empty(b) && calls_since(m) == 0);
        b.borrow(lender);
        CHECK(b.ensure(32, 16) == hipSuccess && calls_since(m) == 0 && b.p == lender.p);   // fits: still the lender's
        CHECK(b.ensure(128, 16) == hipSuccess);                              // does not fit: a block of its own, the lender's stays
        CHECK(calls_since(m) == 1 && calls("hipMalloc", m) == 1 && b.raw && b.p != lender.p && live(kDevice) == 2);
        DevBuf owner;
        CHECK(owner.ensure(8) == hipSuccess && live(kDevice) == 3);
        owner.borrow(lender);                                                // an owner that turns borrower gives its own block back
        CHECK(live(kDevice) == 2 && owner.p == lender.p);
        DevBuf moved(std::move(owner));                                      // a moved borrower is still one
        CHECK(moved.p == lender.p && !moved.raw && empty(owner));
    }
    CHECK(live() == 0);
    puts("ok DevBuf");
}

static void check_event_pinned_stream() {
    size_t at_scope_end;
    {
        DevEvent e;
        CHECK(!e && (hipEvent_t)e == nullptr);
        size_t m = mark();
        CHECK(e.create() == hipSuccess && e && calls_since(m) == 1 && calls("hipEventCreate", m) == 1);
        hipEvent_t const raw = e;
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e == raw && calls_since(m) == 1);   // once
        DevEvent f(std::move(e));
        CHECK(!e && (hipEvent_t)f == raw);
        DevEvent g;
        CHECK(g.create(hipEventDisableTiming) == hipSuccess && calls("hipEventCreateWithFlags", m) == 1 && live(kEvent) == 2);
        g = std::move(f);
        CHECK(!f && (hipEvent_t)g == raw && live(kEvent) == 1);
        DevEvent& self = g;
        g = std::move(self);
        CHECK((hipEvent_t)g == raw && live(kEvent) == 1);
        fail_nth_allocation(1);
        CHECK(e.create() == hipErrorOutOfMemory && !e && live(kEvent) == 1);
        g.release(); g.release();
        CHECK(!g && live() == 0);
        CHECK(g.create() == hipSuccess);
        at_scope_end = mark();
    }
    CHECK(live() == 0 && calls_since(at_scope_end) == 1 && calls("hipEventDestroy", at_scope_end) == 1);
    {   // negative control
        hipEvent_t leaked = nullptr;
        CHECK(hipEventCreate(&leaked) == hipSuccess && live(kEvent) == 1);
        CHECK(hipEventDestroy(leaked) == hipSuccess);
    }
    {
        PinnedBuf b;
        size_t m = mark();
        CHECK(b.ensure(100, hipHostMallocDefault) == hipSuccess && b.p && b.bytes == 100 && calls_since(m) == 1);
        CHECK(b.ensure(100) == hipSuccess && b.ensure(10) == hipSuccess && calls_since(m) == 1 && b.bytes == 100);   // grow-only
        CHECK(b.ensure(200, hipHostMallocMapped) == hipSuccess && b.bytes == 200);
        CHECK(calls_since(m) == 3 && state().log[m + 1].name == "hipHostFree" && state().log[m + 2].name == "hipHostMalloc" && live(kPinned) == 1);
        void* const p = b.p;
        PinnedBuf c(std::move(b));
        CHECK(!b.p && b.bytes == 0 && c.p == p && c.bytes == 200);
        PinnedBuf d;
        CHECK(d.ensure(8) == hipSuccess && live(kPinned) == 2);
        d = std::move(c);
        CHECK(!c.p && d.p == p && live(kPinned) == 1);
        PinnedBuf& self = d;
        d = std::move(self);
        CHECK(d.p == p && d.bytes == 200 && live(kPinned) == 1);
        fail_nth_allocation(1);
        CHECK(d.ensure(400) == hipErrorOutOfMemory && !d.p && d.bytes == 0 && live() == 0);   // left empty
        d.release(); d.release();
        CHECK(d.ensure(8) == hipSuccess);
        at_scope_end = mark();
    }
    CHECK(live() == 0 && calls_since(at_scope_end) == 1 && calls("hipHostFree", at_scope_end) == 1);
    {   // negative control
        RawScratch s;
        CHECK(hipHostMalloc(&s.p, 8, hipHostMallocDefault) == hipSuccess && live(kPinned) == 1);
        CHECK(hipHostFree(s.p) == hipSuccess);
    }
    {
        DevStream s;
        CHECK(!s && (hipStream_t)s == nullptr);
        size_t m = mark();
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s && s.create(hipStreamNonBlocking) == hipSuccess && calls_since(m) == 1);
        hipStream_t const raw = s;
        DevStream t(std::move(s));
        CHECK(!s && (hipStream_t)t == raw && live(kStream) == 1);
        s = std::move(t);
        CHECK(!t && (hipStream_t)s == raw && live(kStream) == 1);
        fail_nth_allocation(1);
        CHECK(t.create(hipStreamNonBlocking) == hipErrorOutOfMemory && !t);
    }
    CHECK(live() == 0 && state().log.back().name == "hipStreamDestroy");
    (void)hipGetLastError();
    puts("ok DevEvent PinnedBuf DevStream");
}

static void check_camslot() {
    const size_t bytes = 512 * 56;
    for (long nth = 1; nth <= 3; nth++) {   // the pinned block, the device block, the event: each failing in turn
        CamSlot s;
        fail_nth_allocation(nth);
        CHECK(s.acquire(bytes) == hipErrorOutOfMemory);
        CHECK(!s && !s.host.p && s.host.bytes == 0 && empty(s.dev) && !s.ev && live() == 0);
        size_t m = mark();
        CHECK(s.acquire(bytes) == hipSuccess && s && s.host.p && s.host.bytes == bytes && s.dev.p && s.dev.bytes == bytes && s.ev);
        CHECK(calls_since(m) == 3 && state().log[m].name == "hipHostMalloc" && state().log[m + 1].name == "hipMalloc" &&
              state().log[m + 2].name == "hipEventCreateWithFlags");
        CHECK(live(kPinned) == 1 && live(kDevice) == 1 && live(kEvent) == 1);
    }
    CHECK(live() == 0);
    (void)hipGetLastError();
    puts("ok CamSlot");
}

// Touching every owning member of a handle, whatever it is an array of
template <typename T, size_t N, typename F> static void each(T (&a)[N], F f) { for (T& x : a) f(x); }
template <typename T, typename F> static void each(T& x, F f) { f(x); }
static size_t n_bufs, n_events, n_pinned, n_slots, n_streams;
static void ensure_buf(DevBuf& b) { CHECK(b.ensure(64) == hipSuccess && b.raw); n_bufs++; }
static void create_event(DevEvent& e) { CHECK(e.create() == hipSuccess && e); n_events++; }
static void ensure_pinned(PinnedBuf& b) { CHECK(b.ensure(64) == hipSuccess && b.p); n_pinned++; }
static void acquire_slot(CamSlot& s) { CHECK(s.acquire(64) == hipSuccess && s); n_slots++; }
static void create_stream(DevStream& s) { CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s); n_streams++; }

#include "handle_touch.inc"   // touch_handle(CrHandle&), touch_sah_work(SahDeviceWork&): written by the test from handle.hpp's declarations

static void check_handle() {
    {   // a handle that made nothing gives nothing back
        CrHandle* h = new CrHandle();
        h->device = 3;
        size_t m = mark();
        delete h;
        CHECK(calls_since(m) == 1 && state().log[m].name == "hipSetDevice" && state().device == 3);
    }
    CrHandle* h = new CrHandle();
    h->device = 5;
    touch_handle(*h);
    CHECK(n_streams == 1 && n_slots == CrHandle::kCamSlots && n_bufs >= 90 && n_events >= 13 && n_pinned >= 2);
    CHECK(live(kStream) == 1 && live(kEvent) == n_events + n_slots && live(kPinned) == n_pinned + n_slots && live(kDevice) == n_bufs + n_slots);
    // the frame trees' side tables are the base trees': six owned blocks go, nothing of the lenders'
    cr::alias_side_tables(h->f32, h->s32);
    cr::alias_side_tables(h->f64, h->s64);
    CHECK(live(kDevice) == n_bufs + n_slots - 6 && h->f32.mats.p == h->s32.mats.p && h->f64.keys.p == h->s64.keys.p && !h->f64.texs.raw);
    const size_t live_before = live();
    size_t m = mark();
    delete h;
    const std::vector<Call>& log = state().log;
    CHECK(live() == 0);
    CHECK(log[m].name == "hipSetDevice" && state().device == 5 && log[m + 1].name == "hipStreamSynchronize");
    CHECK(log.back().name == "hipStreamDestroy" && calls("hipStreamDestroy", m) == 1);
    std::set<long> given_back;
    for (size_t i = m + 2; i < log.size(); i++) {
        CHECK(log[i].name == "hipFree" || log[i].name == "hipHostFree" || log[i].name == "hipEventDestroy" || log[i].name == "hipStreamDestroy");
        CHECK(given_back.insert(log[i].serial).second);   // no object twice
    }
    CHECK(given_back.size() == live_before);
    {   // SahDeviceWork::release, which an upload without CR_BVH_BUILD_DEVICE calls
        SahDeviceWork w;
        n_bufs = 0;
        touch_sah_work(w);
        CHECK(n_bufs >= 14 && live(kDevice) == n_bufs);
        w.release();
        CHECK(live() == 0 && !w.box.p && !w.slots[1].raw);
        w.release();
        CHECK(w.ctr.ensure(8) == hipSuccess);
    }
    CHECK(live() == 0);
    puts("ok CrHandle");
}

int main() {
    check_devbuf();
    check_event_pinned_stream();
    check_camslot();
    check_handle();
    CHECK(live() == 0);
    return 0;
}
