// pm_view.h -- the geometry of one view (gipuma_hip_fusion_view: bp = R^T K^-1, c = C, P = [K R | -K R C]) on the device,
// shared by the depth-map fusion (gipuma_fuse.hip) and the cross-view prior (gipuma_prior.hip).
//
// Both contracts (include/gipuma_hip.h) are restated in numpy float32 (tests/view_ref.py) and the
// kernels must equal the restatements in every bit, so the order of operations IS the contract, and this is the one place
// where it is written in code: float32 + - * in the order of the formula above each function (-ffp-contract=off).  A view
// is any struct with the members named (fuse::View, prior::Source, prior::Target), taken by reference, never copied: its
// constants keep their one address each, relative to the view, and are read with scalar loads as when written in place.
#pragma once
#include <hip/hip_runtime.h>

namespace pm_view {

struct Vec3 {  // (a plain struct, not HIP's float3: three scalars to the compiler, like the x0, x1, x2 written by hand)
    float x, y, z;
};

// Loads through the global address space: a pointer held as an integer (or loaded from memory) is a generic one to the
// compiler, and its accesses would be flat_* (pm_core.h DevPtr, tests/test_isa_waits.py).
template <class T>
__device__ __forceinline__ T load_global(uint64_t base, int idx)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(1))) T *)base)[idx];
#else
    return ((const T *)base)[idx];
#endif
}

// valid(z): finite, > 0, and inside depth_min / depth_max where those are > 0.  Spelled twice: bounds passed as values
// (the prior) are both read before the test, bounds in a parameter block taken by reference (the fusion) each where the
// test comes to it.  Same truth value, other branches: forwarding either to the other changes a kernel's opcode counts.
__device__ __forceinline__ bool valid_depth(float z, float depth_min, float depth_max)
{
    return isfinite(z) && z > 0.f && (depth_min <= 0.f || z >= depth_min) && (depth_max <= 0.f || z <= depth_max);
}
template <class Bounds>
__device__ __forceinline__ bool valid_depth(float z, const Bounds &p)
{
    return isfinite(z) && z > 0.f && (p.depth_min <= 0.f || z >= p.depth_min) && (p.depth_max <= 0.f || z <= p.depth_max);
}

// a . b = (a_0 b_0 + a_1 b_1) + a_2 b_2
__device__ __forceinline__ float dot(const Vec3 &a, const Vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// r = bp (x, y, 1):  r_k = (bp[k][0] x + bp[k][1] y) + bp[k][2]
template <class View>
__device__ __forceinline__ Vec3 ray(const View &v, float x, float y)
{
    return {(v.bp[0] * x + v.bp[1] * y) + v.bp[2], (v.bp[3] * x + v.bp[4] * y) + v.bp[5], (v.bp[6] * x + v.bp[7] * y) + v.bp[8]};
}

// X = c + z (bp (x, y, 1)):  X_k = c[k] + z * ((bp[k][0] x + bp[k][1] y) + bp[k][2])
template <class View>
__device__ __forceinline__ Vec3 backproject(const View &v, float z, float x, float y)
{
    const Vec3 r = ray(v, x, y);
    return {v.c[0] + z * r.x, v.c[1] + z * r.y, v.c[2] + z * r.z};
}

// h = P (X, 1):  h_k = ((P[k][0] X_0 + P[k][1] X_1) + P[k][2] X_2) + P[k][3]
template <class View>
__device__ __forceinline__ Vec3 project(const View &v, const Vec3 &X)
{
    return {((v.P[0] * X.x + v.P[1] * X.y) + v.P[2] * X.z) + v.P[3], ((v.P[4] * X.x + v.P[5] * X.y) + v.P[6] * X.z) + v.P[7],
            ((v.P[8] * X.x + v.P[9] * X.y) + v.P[10] * X.z) + v.P[11]};
}

}  // namespace pm_view
