// A stand-in for <hip/hip_runtime.h>, written for tests/handle_lifetime_check.cpp: the few runtime calls that
// crucible_amd/csrc/devres.hpp and handle.hpp name, on the CPU, with book-keeping a test can read.
//   - every object handed out (device block, pinned block, event, stream) gets a serial number and is live until it is given back;
//   - every call is logged with the serial number of the object it was about;
//   - giving back what is not live (twice, never made, null) aborts;
//   - fail_nth_allocation(n): the n-th allocating call from now (hipMalloc, hipHostMalloc, hipEventCreate*, hipStreamCreate*) fails.
// Blocks are real heap memory, so the address sanitizer and its leak check see them too.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

typedef enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
enum : unsigned { hipEventDefault = 0x0, hipEventDisableTiming = 0x2 };
enum : unsigned { hipHostMallocDefault = 0x0, hipHostMallocMapped = 0x2 };
enum : unsigned { hipStreamDefault = 0x0, hipStreamNonBlocking = 0x1 };

namespace hip_stub {

enum Kind { kDevice, kPinned, kEvent, kStream, kKinds };
struct Call { std::string name; long serial; };   // serial 0: the call was about no object
struct State {
    std::map<const void*, long> live[kKinds];
    std::vector<Call> log;
    long next_serial = 1, fail_in = 0;
    hipError_t last_error = hipSuccess;
    int device = -1;
};
inline State& state() { static State s; return s; }

inline size_t live(Kind k) { return state().live[k].size(); }
inline size_t live() { size_t n = 0; for (int k = 0; k < kKinds; k++) n += live((Kind)k); return n; }
inline void fail_nth_allocation(long n) { state().fail_in = n; }
inline size_t calls(const char* name, size_t from = 0) {
    size_t n = 0;
    for (size_t i = from; i < state().log.size(); i++) n += state().log[i].name == name;
    return n;
}

inline hipError_t make(Kind k, const char* name, void** out, size_t bytes) {
    State& s = state();
    if (s.fail_in > 0 && --s.fail_in == 0) {
        s.log.push_back({std::string(name) + " (failed)", 0});
        return s.last_error = hipErrorOutOfMemory;   // *out is left as it was, as the runtime leaves it
    }
    *out = malloc(bytes ? bytes : 1);
    if (!*out) abort();
    s.live[k][*out] = s.next_serial;
    s.log.push_back({name, s.next_serial++});
    return hipSuccess;
}
inline hipError_t give_back(Kind k, const char* name, void* obj) {
    State& s = state();
    auto it = s.live[k].find(obj);
    if (it == s.live[k].end()) { fprintf(stderr, "hip_stub: %s(%p): not live\n", name, obj); abort(); }
    s.log.push_back({name, it->second});
    s.live[k].erase(it);
    free(obj);
    return hipSuccess;
}
inline hipError_t use(Kind k, const char* name, const void* obj) {
    State& s = state();
    auto it = s.live[k].find(obj);
    if (it == s.live[k].end()) { fprintf(stderr, "hip_stub: %s(%p): not live\n", name, obj); abort(); }
    s.log.push_back({name, it->second});
    return hipSuccess;
}

}   // namespace hip_stub

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_stub::make(hip_stub::kDevice, "hipMalloc", p, bytes); }
inline hipError_t hipFree(void* p) { return hip_stub::give_back(hip_stub::kDevice, "hipFree", p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_stub::make(hip_stub::kPinned, "hipHostMalloc", p, bytes); }
inline hipError_t hipHostFree(void* p) { return hip_stub::give_back(hip_stub::kPinned, "hipHostFree", p); }
inline hipError_t hipEventCreate(hipEvent_t* e) { return hip_stub::make(hip_stub::kEvent, "hipEventCreate", (void**)e, 1); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hip_stub::make(hip_stub::kEvent, "hipEventCreateWithFlags", (void**)e, 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub::give_back(hip_stub::kEvent, "hipEventDestroy", e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hip_stub::make(hip_stub::kStream, "hipStreamCreateWithFlags", (void**)s, 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_stub::give_back(hip_stub::kStream, "hipStreamDestroy", s); }
inline hipError_t hipStreamSynchronize(hipStream_t s) { return hip_stub::use(hip_stub::kStream, "hipStreamSynchronize", s); }
inline hipError_t hipSetDevice(int device) { hip_stub::state().device = device; hip_stub::state().log.push_back({"hipSetDevice", 0}); return hipSuccess; }
inline hipError_t hipGetLastError() { hipError_t e = hip_stub::state().last_error; hip_stub::state().last_error = hipSuccess; return e; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid argument"; }
