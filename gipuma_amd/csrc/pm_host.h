// pm_host.h -- host-side support of the add-on translation units (gipuma_fuse.hip, gipuma_pyramid.hip, gipuma_prior.hip):
// the library's last-error text, the check of a HIP call and the check of a device ordinal.  No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

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

}  // namespace pm_host
