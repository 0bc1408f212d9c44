// ctx_mem.h -- the types that own what a bn_ctx holds on the device and in pinned memory:
// buffers (DevBuf, PinBuf), the pinned upload channels with their fence (UploadChannel,
// Fence) and the registries of the handles a context hands out (HandleList).  Each frees
// what it holds in its destructor, so a member of bn_ctx or of a handle needs no line in
// any teardown.  Host code only: the HIP runtime header and standard headers, nothing with
// device code in it (tests/native/ctx_mem_main.cpp builds it against a stand-in runtime).
// ctx.h includes it and defines fail and ws_drain behind bn_ctx.  Not a public header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bn254mi.h"

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface
namespace bn {

// the call's return code, its message left in the context
inline int fail(bn_ctx* c, int code, const std::string& msg);
// before freeing workspace buffers: wait until no queued work can still read them
inline int ws_drain(bn_ctx* c);

#define HIPCHK(ctx, x)                                                                   \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess)                                                            \
            return fail(ctx, BN_ERR_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

#define RET_IF(x)              \
    do {                       \
        int r_ = (x);          \
        if (r_) return r_;     \
    } while (0)

// A device (or, kPinned, a pinned host) buffer of T and its capacity in elements.  Move-only;
// reads as T* where a kernel argument is wanted; the destructor frees and ignores the result.
template <class T, bool kPinned>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        std::swap(p_, o.p_), std::swap(cap_, o.cap_);
        return *this;
    }
    ~Buf() {
        if (p_) (void)dealloc();
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }  // where the pointer type has to be deduced, or cast
    size_t cap() const { return cap_; }

    // Grown to `need` elements (at least `floor`; never shrunk).  Queued kernels may still
    // read the old device buffer, so growing drains first: when there is an old buffer, or
    // always (drain_always: the products' buffers).  A pinned buffer's only device users are
    // copies that its caller has waited for: it never drains.
    int grow(bn_ctx* c, size_t need, size_t floor = 0, bool drain_always = false) {
        return need <= cap_ ? BN_OK : replace(c, need, floor, drain_always);
    }
    // grow's steps past the comparison (UploadChannel keeps the capacity it compares with)
    int replace(bn_ctx* c, size_t need, size_t floor = 0, bool drain_always = false) {
        if (!kPinned && (p_ || drain_always)) RET_IF(ws_drain(c));
        RET_IF(release(c));
        return alloc(c, std::max(need, floor));
    }
    // freed, a failure reported; null and capacity 0 from here until alloc has succeeded
    int release(bn_ctx* c) {
        if (p_) HIPCHK(c, dealloc());
        p_ = nullptr;
        cap_ = 0;
        return BN_OK;
    }
    // n elements for an empty buffer
    int alloc(bn_ctx* c, size_t n) {
        if constexpr (kPinned)
            HIPCHK(c, hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault));
        else
            HIPCHK(c, hipMalloc((void**)&p_, n * sizeof(T)));
        cap_ = n;
        return BN_OK;
    }

private:
    hipError_t dealloc() {
        if constexpr (kPinned)
            return hipHostFree(p_);
        else
            return hipFree(p_);
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T>
using DevBuf = Buf<T, false>;
template <class T>
using PinBuf = Buf<T, true>;

// Device buffers under one capacity *cap (the pairing workspace: buffer i holds per[i]
// elements per unit of it), grown together to n units, at least `floor`: drained if there
// was a workspace, every old buffer freed, then every new one allocated; *cap is 0 in between.
template <class... B>
int grow_together(bn_ctx* c, size_t* cap, size_t n, size_t floor, const size_t (&per)[sizeof...(B)], B&... buf) {
    if (n <= *cap) return BN_OK;
    n = std::max(n, floor);
    if (*cap) RET_IF(ws_drain(c));
    int rc = BN_OK;
    ((rc = rc ? rc : buf.release(c)), ...);
    RET_IF(rc);
    *cap = 0;
    const size_t* k = per;
    ((rc = rc ? rc : buf.alloc(c, n * *k++)), ...);
    RET_IF(rc);
    *cap = n;
    return BN_OK;
}

// An event behind the latest copy out of a pinned source, and whether that copy may still
// run.  A call waits before its host code rewrites (or replaces) the source, and records
// behind its own copy.  The event is created on first use.
class Fence {
public:
    Fence() = default;
    Fence(const Fence&) = delete;
    Fence& operator=(const Fence&) = delete;
    ~Fence() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    bool pending() const { return pending_; }
    int wait(bn_ctx* c) {
        RET_IF(ready(c));
        if (pending_) {
            HIPCHK(c, hipEventSynchronize(ev_));
            pending_ = false;
        }
        return BN_OK;
    }
    int record(bn_ctx* c, hipStream_t s) {
        RET_IF(ready(c));
        HIPCHK(c, hipEventRecord(ev_, s));
        pending_ = true;
        return BN_OK;
    }

private:
    int ready(bn_ctx* c) {
        if (!ev_) HIPCHK(c, hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        return BN_OK;
    }
    hipEvent_t ev_ = nullptr;
    bool pending_ = false;
};

// Words that go up in one copy in front of a call's kernels: the pinned source h, the device
// copy d, one capacity for both (at least 4096 words).  A call's order is wait (the fence),
// grow, fill h, copy, record (the fence); several channels may share one fence.
struct UploadChannel {
    PinBuf<uint32_t> h;
    DevBuf<uint32_t> d;
    size_t cap = 0;  // words; 0 while either buffer is being replaced

    // room for `words` (0: nothing to do); the copy that may still read h is waited for first,
    // and the kernels that may still read d are drained
    int grow(bn_ctx* c, Fence& fence, size_t words) {
        if (!words) return BN_OK;
        RET_IF(fence.wait(c));
        if (words <= cap) return BN_OK;
        cap = 0;
        RET_IF(d.replace(c, words, 4096, true));
        RET_IF(h.replace(c, d.cap()));
        cap = d.cap();
        return BN_OK;
    }
    // the first `words` words of h -> d on s
    int copy(bn_ctx* c, size_t words, hipStream_t s) {
        HIPCHK(c, hipMemcpyAsync(d, h, words * 4, hipMemcpyHostToDevice, s));
        return BN_OK;
    }
};

// The handles of one kind that a context made and has not destroyed yet.  It owns them:
// deleting a handle frees its tables (its DevBuf members), and the list's destructor deletes
// the handles still alive.
template <class H>
class HandleList {
public:
    HandleList() = default;
    HandleList(const HandleList&) = delete;
    HandleList& operator=(const HandleList&) = delete;
    ~HandleList() {
        for (H* h : v_) delete h;
    }
    // a live handle of this context (looked up, not dereferenced: another context's handle,
    // or a destroyed one, is refused)
    bool live(const H* h) const { return h && std::find(v_.begin(), v_.end(), h) != v_.end(); }
    H* adopt(std::unique_ptr<H> h) {
        v_.push_back(h.get());
        return h.release();
    }
    // The end of a build queued on s with outcome rc.  The host forms (wait) wait for the
    // build before they return.  On failure the stream is synchronized, so that nothing
    // queued can still write the tables, and then the handle is dropped.
    int settle(bn_ctx* c, std::unique_ptr<H> h, int rc, bool wait, hipStream_t s, H** out) {
        if (rc == BN_OK && wait && hipStreamSynchronize(s) != hipSuccess) rc = fail(c, BN_ERR_HIP, "hipStreamSynchronize");
        if (rc != BN_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        *out = adopt(std::move(h));
        return BN_OK;
    }
    // every call that reads the tables has recorded ws_event behind its work: drained first
    int destroy(bn_ctx* c, H* h, const char* refusal) {
        if (!live(h)) return fail(c, BN_ERR_INVALID_ARGUMENT, refusal);
        RET_IF(ws_drain(c));
        v_.erase(std::find(v_.begin(), v_.end(), h));
        delete h;
        return BN_OK;
    }

private:
    std::vector<H*> v_;
};

}  // namespace bn
#pragma GCC visibility pop
