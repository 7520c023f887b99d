// yolo355 -- the host-side pieces every library of the project needs, and nothing of a kernel: the error return, HIPCHK,
// DeviceGuard, DevMem (how host state gets device memory), its HIP form, DevOwner (the one owner of that memory) and DevScope.
// libyolo355.so gets it through y355_common.h; loss.hip and anchors.hip include it alone.  The error codes are yolo355.h's;
// the companions' families carry the same numbers (each asserts it next to its include).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/yolo355.h"

// keeps msg for the library's last-error call, returns code: one definition per library (engine.hip, loss.hip, anchors.hip),
// and host_state_check.cpp's own
int y355_fail(int code, const std::string &msg);
// a HIP call of a function that returns a y355 error code: on failure Y355_EHIP, the call and HIP's text as the message
#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return y355_fail(Y355_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// the companions' device convention: an entry point works on its handle's device and leaves the caller's current one as it
// found it (libyolo355.so's entry points leave theirs set)
struct DeviceGuard {
    int prev = -1;
    hipError_t set(int dev) {
        hipError_t e = hipGetDevice(&prev);
        return e != hipSuccess ? e : hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// How a piece of host-side state (HeadState of head_nms.h, FrameStage of y355_common.h, ...) gets and fills device memory: the
// HIP calls in the handles (y355_hip_mem), the host heap with a failure at the k-th allocation in host_state_check.cpp.
struct DevMem {
    std::function<int(void **p, size_t bytes, bool zero)> alloc;   // != 0: failure, y355_fail holds the message
    std::function<void(void *p)> release;
    // host -> device copy once everything enqueued on s has run (what s has in flight may still read dst); != 0: failure
    std::function<int(void *dst, const void *src, size_t bytes, hipStream_t s)> upload;
};
inline int y355_hip_alloc(void **p, size_t bytes, bool zero) {
    HIPCHK(hipMalloc(p, bytes ? bytes : 16));
    if (zero) {
        const hipError_t e_ = hipMemset(*p, 0, bytes ? bytes : 16);
        if (e_ != hipSuccess) {
            (void)hipFree(*p);
            return y355_fail(Y355_EHIP, std::string("hipMemset(*p, 0, bytes ? bytes : 16): ") + hipGetErrorString(e_));
        }
    }
    return 0;
}
inline int y355_hip_upload(void *dst, const void *src, size_t bytes, hipStream_t s) {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
inline const DevMem &y355_hip_mem(void) {
    static const DevMem m{y355_hip_alloc, [](void *p) { (void)hipFree(p); }, y355_hip_upload};
    return m;
}

// The one owner of a piece of host state's device memory (HeadState, FrameStage, HandleCore, y355_apeval, y355_pipeline,
// y355_loss, y355_anchors, ConvOpMem of y355_conv_op, and a DevScope for what lives as long as one call): what it got and has
// not dropped goes back in y355_dev_release_all, whatever the fields that pointed to it say by then.
struct DevOwner {
    DevMem mem;
    std::vector<void *> allocs;
};
// *p = count elements (of `elem` bytes: 1 = count is in bytes) the owner now holds, zeroed on demand; a failure (the allocator's
// code) leaves *p alone
template <typename T>
inline int y355_dev_get(DevOwner &o, T **p, size_t count, bool zero = false, size_t elem = sizeof(T)) {
    void *q = nullptr;
    if (int rc = o.mem.alloc(&q, count * elem, zero)) return rc;
    o.allocs.push_back(q);
    *p = (T *)q;
    return 0;
}
// releases what the pointers hold, forgets it, nulls them; a null one is left alone
template <typename... T>
inline void y355_dev_drop(DevOwner &o, T **...p) {
    for (void *q : {(void *)*p...}) {
        if (q) o.mem.release(q);
        o.allocs.erase(std::remove(o.allocs.begin(), o.allocs.end(), q), o.allocs.end());
    }
    ((*p = nullptr), ...);
}
// several arrays (null now) of count elements each (<true>: zeroed): all of them or, after a failure, none
template <bool Zero = false, typename... T>
inline int y355_dev_get_all(DevOwner &o, size_t count, T **...p) {
    int rc = 0;
    ((rc = rc ? rc : y355_dev_get(o, p, count, Zero)), ...);
    if (rc) y355_dev_drop(o, p...);
    return rc;
}
// one array, or several of one capacity *have (elements of each): nothing when they are there and need <= *have, else dropped
// and got again at `need` (<true>: zeroed); a failure leaves every one of them null and *have = 0
template <bool Zero = false, typename... T>
inline int y355_dev_grow(DevOwner &o, size_t *have, size_t need, T **...p) {
    if (need <= *have && (... && (*p != nullptr))) return 0;
    y355_dev_drop(o, p...);
    const int rc = y355_dev_get_all<Zero>(o, need, p...);
    *have = rc ? 0 : need;
    return rc;
}
// all or nothing across sizes: m = y355_dev_mark before a step's allocations; y355_dev_rollback(o, m) releases them when one
// failed (their pointers: written to a copy of the state that is thrown away, or nulled by the caller)
inline size_t y355_dev_mark(const DevOwner &o) { return o.allocs.size(); }
inline void y355_dev_rollback(DevOwner &o, size_t mark) {
    for (; o.allocs.size() > mark; o.allocs.pop_back()) o.mem.release(o.allocs.back());
}
inline void y355_dev_release_all(DevOwner &o) { y355_dev_rollback(o, 0); }       // idempotent

// The device memory of one call (the host-pointer forms of ops.hip, y355_head_f32_ex): an owner on the HIP calls whose memory
// goes back when the call returns, whichever way.
struct DevScope : DevOwner {
    DevScope() : DevOwner{y355_hip_mem(), {}} {}
    DevScope(const DevScope &) = delete;
    DevScope &operator=(const DevScope &) = delete;
    ~DevScope() { y355_dev_release_all(*this); }
};
