// pm_host.h -- host-side support of the add-on translation units (gipuma_fuse.hip, gipuma_pyramid.hip, gipuma_prior.hip,
// gipuma_cloud.hip): the library's last-error text, the check of a HIP call, the check of a device ordinal and CallScope,
// the owner of one call's stream, events and scratch buffers (fusion, cloud search, cloud thinning).  No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/gipuma_hip.h"

// the library's last-error text (gipuma_hip.hip; hidden, not part of the C-ABI)
extern "C" __attribute__((visibility("hidden"))) void gipuma_set_last_error(const char *text);

namespace pm_host {

// sets the last-error text and returns `code`: `return fail(GIPUMA_HIP_ERR_ARG, "...")`
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    gipuma_set_last_error(buf);
    return code;
}

#define HIP_OK(expr)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return pm_host::fail(GIPUMA_HIP_ERR_DEVICE, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

inline int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// 0 when `device_id` names a visible device; the last check of an entry point, after those of its own arguments
inline int check_device(int device_id)
{
    const int n = device_count();
    if (n < 1) return fail(GIPUMA_HIP_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(GIPUMA_HIP_ERR_ARG, "device_id out of range");
    return 0;
}

// What a call with per-call scratch owns: its stream (the caller's, or a non-blocking one of its own), a handful of
// events and the device buffers allocated through it.  All of it goes on every way out of the call, after the stream has
// been waited for.  Buffers that outlive the call are not allocated here: they belong to the handle that returns them.
struct CallScope {
    static constexpr int kMaxEvents = 4;
    hipStream_t st = nullptr;
    hipEvent_t e[kMaxEvents] = {nullptr, nullptr, nullptr, nullptr};

    CallScope() = default;
    CallScope(const CallScope &) = delete;
    CallScope &operator=(const CallScope &) = delete;
    ~CallScope()
    {
        if (st) (void)hipStreamSynchronize(st);  // (nothing of this call is in flight when its buffers go)
        for (void *p : bufs_) (void)hipFree(p);
        for (hipEvent_t ev : e)
            if (ev) (void)hipEventDestroy(ev);
        if (own_) (void)hipStreamDestroy(own_);
    }

    // the current device's: `stream` (a hipStream_t) or, for null, a stream of the scope's own; e[0 .. n_events)
    int open(void *stream, int n_events)
    {
        if (stream) {
            st = (hipStream_t)stream;
        } else {
            HIP_OK(hipStreamCreateWithFlags(&own_, hipStreamNonBlocking));
            st = own_;
        }
        for (int k = 0; k < n_events && k < kMaxEvents; ++k) HIP_OK(hipEventCreate(&e[k]));
        return 0;
    }

    // p = `count` uninitialised T on the device, the scope's to free; several in a row:
    //     if (sc.alloc(a, n) || sc.alloc(b, m)) return GIPUMA_HIP_ERR_DEVICE;
    template <class T>
    int alloc(T *&p, size_t count)
    {
        bufs_.push_back(nullptr);
        const hipError_t err = hipMalloc(&bufs_.back(), sizeof(T) * count);
        if (err != hipSuccess) return fail(GIPUMA_HIP_ERR_DEVICE, "hipMalloc of %zu bytes: %s", sizeof(T) * count, hipGetErrorString(err));
        p = (T *)bufs_.back();
        return 0;
    }

private:
    hipStream_t own_ = nullptr;
    std::vector<void *> bufs_;
};

}  // namespace pm_host
