// gipuma_pyramid.hip -- one pyramid level of an image plane on gfx950.
//
// The contract (include/gipuma_hip.h), restated on the CPU in float32 by tests/pyramid_ref.py:
//
//     out[Y][X] = floorf(((in[2Y][2X] + in[2Y][2X+1]) + (in[2Y+1][2X] + in[2Y+1][2X+1])) * 0.25f + 0.5f)
//
// per channel, for Y < rows >> 1, X < cols >> 1 (a last odd row or column is dropped).  For the integer-valued 0..255
// planes the front-ends deliver every step is exact in fp32 and the result is integer-valued again, so a coarse plane
// passes the session's 8-bit test like its parent and the coarse session runs the packed-window kernels.
//
// pyr::downsample2_kernel<CH, VEC>: one lane per VEC / 2 output pixels of a gray plane (VEC = 4: two 16-byte loads, one
// 8-byte store; VEC = 2: two 8-byte loads; VEC = 1: a plane whose address or pitch is not 8-byte aligned, four 4-byte
// loads), one lane per output pixel of a colour plane (four 16-byte loads, or sixteen 4-byte ones).  Pure streaming: the
// kernel reads every input byte once, no LDS, no atomics.
#include <hip/hip_runtime.h>

#include "pm_host.h"

using pm_host::fail;

namespace pyr {

constexpr int kBlockX = 64, kBlockY = 4;  // one wavefront per output row of the block

// Loads and stores through the global address space (flat_* accesses count on lgkmcnt as well as vmcnt; pm_core.h DevPtr)
#if defined(__HIP_DEVICE_COMPILE__)
#define PYR_GLOBAL __attribute__((address_space(1)))
#else
#define PYR_GLOBAL
#endif
template <class T>
__device__ __forceinline__ T ld(const float *p)
{
    return *(const PYR_GLOBAL T *)p;
}
template <class T>
__device__ __forceinline__ void st(float *p, T v)
{
    *(PYR_GLOBAL T *)p = v;
}

__device__ __forceinline__ float mean4(float a, float b, float c, float d)
{
    return floorf(((a + b) + (c + d)) * 0.25f + 0.5f);
}

template <int CH, int VEC>
__global__ __launch_bounds__(kBlockX *kBlockY) void downsample2_kernel(const float *__restrict__ src, int orows, int ocols,
                                                                      int pitch, float *__restrict__ dst, int dst_pitch)
{
    const int lane_x = blockIdx.x * kBlockX + threadIdx.x;
    const int Y = blockIdx.y * kBlockY + threadIdx.y;
    if (Y >= orows) return;
    const float *r0 = src + (size_t)(2 * Y) * (size_t)pitch;
    const float *r1 = r0 + pitch;
    float *o = dst + (size_t)Y * (size_t)dst_pitch;
    if constexpr (CH == 1 && VEC == 4) {
        const int X = 2 * lane_x;
        if (X >= ocols) return;
        if (X + 1 < ocols) {
            const float4 a = ld<float4>(r0 + 2 * X), b = ld<float4>(r1 + 2 * X);
            st<float2>(o + X, make_float2(mean4(a.x, a.y, b.x, b.y), mean4(a.z, a.w, b.z, b.w)));
        } else {  // (the last pixel of an odd output row: the second half of a 16-byte load may lie outside the plane)
            const float2 a = ld<float2>(r0 + 2 * X), b = ld<float2>(r1 + 2 * X);
            st<float>(o + X, mean4(a.x, a.y, b.x, b.y));
        }
    } else if constexpr (CH == 1 && VEC == 2) {
        const int X = lane_x;
        if (X >= ocols) return;
        const float2 a = ld<float2>(r0 + 2 * X), b = ld<float2>(r1 + 2 * X);
        st<float>(o + X, mean4(a.x, a.y, b.x, b.y));
    } else if constexpr (CH == 1) {
        const int X = lane_x;
        if (X >= ocols) return;
        st<float>(o + X, mean4(ld<float>(r0 + 2 * X), ld<float>(r0 + 2 * X + 1), ld<float>(r1 + 2 * X), ld<float>(r1 + 2 * X + 1)));
    } else if constexpr (VEC == 4) {
        const int X = lane_x;
        if (X >= ocols) return;
        const float4 a = ld<float4>(r0 + 8 * X), b = ld<float4>(r0 + 8 * X + 4);
        const float4 c = ld<float4>(r1 + 8 * X), d = ld<float4>(r1 + 8 * X + 4);
        st<float4>(o + 4 * X, make_float4(mean4(a.x, b.x, c.x, d.x), mean4(a.y, b.y, c.y, d.y), mean4(a.z, b.z, c.z, d.z),
                                          mean4(a.w, b.w, c.w, d.w)));
    } else {
        const int X = lane_x;
        if (X >= ocols) return;
        for (int k = 0; k < 4; k++)
            st<float>(o + 4 * X + k, mean4(ld<float>(r0 + 8 * X + k), ld<float>(r0 + 8 * X + 4 + k), ld<float>(r1 + 8 * X + k),
                                           ld<float>(r1 + 8 * X + 4 + k)));
    }
}

}  // namespace pyr

namespace {

bool aligned(const void *p, int pitch, int floats) { return (uintptr_t)p % (4u * floats) == 0 && pitch % floats == 0; }

}  // namespace

extern "C" {

int gipuma_hip_downsample(const float *src_dev, int rows, int cols, int pitch, int channels, float *dst_dev, int dst_pitch,
                          int device_id, void *stream)
{
    if (!src_dev || !dst_dev) return fail(GIPUMA_HIP_ERR_ARG, "downsample: null plane");
    if (channels != 1 && channels != 4) return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "downsample: channels must be 1 or 4");
    if (rows < 2 || cols < 2 || rows > 32768 || cols > 32768) return fail(GIPUMA_HIP_ERR_ARG, "downsample: rows x cols out of range");
    const int orows = rows >> 1, ocols = cols >> 1;
    if (pitch < cols * channels || dst_pitch < ocols * channels)
        return fail(GIPUMA_HIP_ERR_ARG, "downsample: a pitch (in floats) is shorter than its row");
    if (const int rc = pm_host::check_device(device_id)) return rc;
    HIP_OK(hipSetDevice(device_id));
    hipStream_t st = (hipStream_t)stream;
    const bool in16 = aligned(src_dev, pitch, 4), in8 = aligned(src_dev, pitch, 2);
    const bool two = channels == 1 && in16 && aligned(dst_dev, dst_pitch, 2);  // two output pixels per lane
    const int lanes_x = two ? (ocols + 1) / 2 : ocols;
    const dim3 block(pyr::kBlockX, pyr::kBlockY), grid((lanes_x + pyr::kBlockX - 1) / pyr::kBlockX, (orows + pyr::kBlockY - 1) / pyr::kBlockY);
    void (*k)(const float *, int, int, int, float *, int);
    if (channels == 4)
        k = (in16 && aligned(dst_dev, dst_pitch, 4)) ? pyr::downsample2_kernel<4, 4> : pyr::downsample2_kernel<4, 1>;
    else if (two)
        k = pyr::downsample2_kernel<1, 4>;
    else
        k = in8 ? pyr::downsample2_kernel<1, 2> : pyr::downsample2_kernel<1, 1>;
    hipLaunchKernelGGL(k, grid, block, 0, st, src_dev, orows, ocols, pitch, dst_dev, dst_pitch);
    HIP_OK(hipGetLastError());
    if (!st) HIP_OK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
