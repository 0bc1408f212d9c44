// A stand-in for <hip/hip_runtime.h>, for host-only builds of csrc/ctx.h and csrc/ctx_mem.h
// (tests/native/ctx_mem_main.cpp): the calls those headers make, backed by malloc.  It counts
// the live device buffers, pinned buffers, events and streams, keeps the calls' names in order,
// and can be told to fail the k-th allocation from now.  Freeing or destroying what is not
// live aborts.  No GPU, no HIP.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string_view>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1;
typedef struct fakehip_event* hipEvent_t;
typedef struct fakehip_stream* hipStream_t;
struct fakehip_event {
    int recorded;
};
struct fakehip_stream {
    int unused;
};
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

namespace fakehip {
inline std::set<void*> dev, pin, events, streams;  // what is live
inline std::vector<const char*> calls;             // every call's name, in order
inline int fail_alloc_in = 0;                      // k > 0: the k-th allocation from now fails
inline int events_created = 0;

inline hipError_t alloc(const char* name, std::set<void*>& live, void** p, size_t bytes) {
    calls.push_back(name);
    if (fail_alloc_in > 0 && --fail_alloc_in == 0) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
inline hipError_t release(const char* name, std::set<void*>& live, void* p) {
    calls.push_back(name);
    if (!live.erase(p)) {
        printf("%s of %p, which is not live\n", name, p);
        abort();
    }
    free(p);
    return hipSuccess;
}
// how often `name` was called since position `from` of the log
inline int count(const char* name, size_t from = 0) {
    int n = 0;
    for (size_t i = from; i < calls.size(); ++i) n += std::string_view(calls[i]) == name;
    return n;
}
}  // namespace fakehip

inline const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
inline hipError_t hipMalloc(void** p, size_t bytes) { return fakehip::alloc("hipMalloc", fakehip::dev, p, bytes); }
inline hipError_t hipFree(void* p) { return fakehip::release("hipFree", fakehip::dev, p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    return fakehip::alloc("hipHostMalloc", fakehip::pin, p, bytes);
}
inline hipError_t hipHostFree(void* p) { return fakehip::release("hipHostFree", fakehip::pin, p); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    ++fakehip::events_created;
    fakehip::calls.push_back("hipEventCreateWithFlags");
    *e = (hipEvent_t)calloc(1, sizeof(fakehip_event));
    fakehip::events.insert(*e);
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fakehip::release("hipEventDestroy", fakehip::events, e); }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    fakehip::calls.push_back("hipEventRecord");
    e->recorded = 1;
    return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e) {
    fakehip::calls.push_back("hipEventSynchronize");
    return e->recorded ? hipSuccess : hipErrorInvalidValue;  // (the project waits only behind a record)
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    fakehip::calls.push_back("hipStreamCreateWithFlags");
    *s = (hipStream_t)calloc(1, sizeof(fakehip_stream));
    fakehip::streams.insert(*s);
    return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) { return fakehip::release("hipStreamDestroy", fakehip::streams, s); }
inline hipError_t hipStreamSynchronize(hipStream_t) {
    fakehip::calls.push_back("hipStreamSynchronize");
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    fakehip::calls.push_back("hipMemcpyAsync");
    memcpy(dst, src, bytes);  // (at once: the sanitizer then sees a copy past either buffer)
    return hipSuccess;
}
