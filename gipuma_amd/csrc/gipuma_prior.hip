// gipuma_prior.hip -- the cross-view prior on gfx950: the solved (n_world, depth) maps of other cameras, carried into a
// new reference camera as the start of its solve.
//
// The contract (include/gipuma_hip.h) is restated on the CPU in float32 by tests/prior_ref.py; every
// operation below is one of + - * /, floorf in the order the contract writes it, compiled with -ffp-contract=off, so the
// two agree in every bit.
//
// On one stream, per call:
//   hipMemsetAsync          zbuf (one 64-bit key per target pixel) to all ones, the three class counts to zero
//   prior::splat_kernel     grid.y = source; one lane per source pixel: one 16-byte load, back-project, project into the
//                           target, and one 64-bit unsigned atomic minimum of (depth bits, source ordinal, source pixel)
//                           on the target pixel it lands in.  The camera constants sit in the kernel arguments: the
//                           source's are read with scalar loads (blockIdx.y is wave-uniform).
//   prior::resolve_kernel   one lane per target pixel: its key (or, for an empty pixel with `fill`, the smallest of the
//                           8 neighbours'), the winner's texel once more, the intersection of its plane with the pixel's
//                           own ray; one float4 store, and per wavefront one integer atomic add per class count (spread over
//                           256 slots per class, which the host sums when the counts are asked for).
// A minimum and an integer sum do not depend on the order of their operands: the result is the same for every launch
// geometry and every order the workgroups run in.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "pm_host.h"
#include "pm_view.h"

using pm_host::fail;

namespace prior {

constexpr int kBlock = 256;  // pixels per workgroup: 4 wavefronts
constexpr unsigned long long kEmpty = ~0ull;
// The class counts are summed into kSlots words per class (a wavefront adds to the slot of its number) and the host adds
// the slots up: one word takes about 90 atomics per microsecond, and a 1600x1200 frame has 30 000 wavefronts.
constexpr int kSlots = 256;

using namespace pm_view;  // the contract's operation order: load_global, valid_depth, ray, backproject, project, dot

struct Source {  // 64 bytes
    uint64_t norm4, cost;
    float bp[9], c[3];
};
struct Target {
    float bp[9], c[3], P[12];
};
struct Args {  // passed by value: the kernel argument segment (2.2 KB of its 4 KB)
    int rows, cols, n_sources, fill;
    float depth_min, depth_max, max_cost, g2;
    Target t;
    Source src[GIPUMA_HIP_MAX_VIEWS];
};

__global__ __launch_bounds__(kBlock) void splat_kernel(Args a, unsigned long long *__restrict__ zbuf)
{
    const int npix = a.rows * a.cols;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= npix) return;
    const int k = blockIdx.y;  // wave-uniform: the source's constants come through scalar loads
    const Source &s = a.src[k];
    const float4 m = load_global<float4>(s.norm4, idx);
    const float z = m.w;
    const Vec3 n = {m.x, m.y, m.z};
    if (!valid_depth(z, a.depth_min, a.depth_max)) return;
    if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z))) return;
    if (!(dot(n, n) > 0.f)) return;
    if (s.cost && !(load_global<float>(s.cost, idx) <= a.max_cost)) return;
    const Vec3 X = backproject(s, z, (float)(idx % a.cols), (float)(idx / a.cols));
    const Vec3 h = project(a.t, X);
    if (!(h.z > 0.f) || !valid_depth(h.z, a.depth_min, a.depth_max)) return;
    const float qx = floorf(h.x / h.z + 0.5f);
    const float qy = floorf(h.y / h.z + 0.5f);
    if (!(qx >= 0.f && qx < (float)a.cols && qy >= 0.f && qy < (float)a.rows)) return;
    if (!(dot(n, ray(a.t, qx, qy)) < 0.f)) return;  // the surface does not face the target camera
    const unsigned long long key =
        ((unsigned long long)__float_as_uint(h.z) << 32) | (unsigned long long)((uint32_t)k * (uint32_t)npix + (uint32_t)idx);
    // (qx, qy) passed the bounds test above: the index is inside zbuf's rows * cols entries
    atomicMin(&zbuf[(size_t)((int)qy * a.cols + (int)qx)], key);
}

__global__ __launch_bounds__(kBlock) void resolve_kernel(Args a, const unsigned long long *__restrict__ zbuf,
                                                         float4 *__restrict__ out, uint32_t *__restrict__ counts)
{
    const int npix = a.rows * a.cols;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    int cls = -1;  // 0 direct, 1 filled, 2 empty; -1: no pixel
    if (pix < npix) {
        const int x = pix % a.cols, y = pix / a.cols;
        unsigned long long key = zbuf[pix];
        cls = 0;
        if (key == kEmpty && a.fill) {
            cls = 1;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= a.rows) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= a.cols || (dx == 0 && dy == 0)) continue;
                    const unsigned long long n = zbuf[yy * a.cols + xx];
                    key = n < key ? n : key;
                }
            }
        }
        float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
        if (key == kEmpty) {
            cls = 2;
        } else {
            const uint32_t low = (uint32_t)key;
            const int k = (int)(low / (uint32_t)npix), idx = (int)(low % (uint32_t)npix);  // k < n_sources: splat wrote it
            const Source &s = a.src[k];
            const float4 m = load_global<float4>(s.norm4, idx);
            const Vec3 n = {m.x, m.y, m.z};
            const Vec3 X = backproject(s, m.w, (float)(idx % a.cols), (float)(idx / a.cols));
            const Target &t = a.t;
            const Vec3 r = ray(t, (float)x, (float)y);
            const float den = dot(n, r);
            const float zc = dot(n, Vec3{X.x - t.c[0], X.y - t.c[1], X.z - t.c[2]}) / den;
            const bool good = den * den > a.g2 * (dot(n, n) * dot(r, r)) && valid_depth(zc, a.depth_min, a.depth_max);
            if (cls == 0)
                res = make_float4(m.x, m.y, m.z, good ? zc : __uint_as_float((uint32_t)(key >> 32)));
            else if (good)
                res = make_float4(m.x, m.y, m.z, zc);
            else
                cls = 2;
        }
        out[pix] = res;
    }
    const int slot = (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kSlots - 1);
    for (int c = 0; c < 3; ++c) {  // one integer add per wavefront and class
        const unsigned long long b = __ballot(cls == c);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counts[c * kSlots + slot], (uint32_t)__popcll(b));
    }
}

}  // namespace prior

namespace {

// The scratch of a device, kept between calls (a call that frees would have to wait for the device): the key plane, grown
// when a larger frame comes, the counts and the event pair.  Calls on one device share it, so they must not overlap.
struct Scratch {
    unsigned long long *zbuf = nullptr;
    size_t capacity = 0;  // keys
    uint32_t *counts = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::mutex mutex;  // held for a call on this device; calls on other devices do not wait for it
};
std::mutex g_mutex;  // guards the map only (its nodes do not move)
std::map<int, Scratch> g_scratch;

int run(const gipuma_hip_prior_desc *d, float *prior_dev, int64_t counts[3], float *device_ms)
{
    const size_t npix = (size_t)d->rows * d->cols;
    const int S = d->n_sources;
    Scratch *found;
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        found = &g_scratch[d->device_id];
    }
    Scratch &sc = *found;
    std::lock_guard<std::mutex> lock(sc.mutex);
    HIP_OK(hipSetDevice(d->device_id));
    if (sc.capacity < npix) {
        if (sc.zbuf) HIP_OK(hipFree(sc.zbuf));  // (waits for the calls that still use it)
        sc.zbuf = nullptr;
        sc.capacity = 0;
        HIP_OK(hipMalloc(&sc.zbuf, sizeof(unsigned long long) * npix));
        sc.capacity = npix;
    }
    if (!sc.counts) HIP_OK(hipMalloc(&sc.counts, sizeof(uint32_t) * 3 * prior::kSlots));
    if (!sc.e0) HIP_OK(hipEventCreate(&sc.e0));
    if (!sc.e1) HIP_OK(hipEventCreate(&sc.e1));

    prior::Args a;
    memset(&a, 0, sizeof a);
    a.rows = d->rows;
    a.cols = d->cols;
    a.n_sources = S;
    a.fill = d->fill;
    a.depth_min = d->depth_min;
    a.depth_max = d->depth_max;
    a.max_cost = d->max_cost;
    a.g2 = d->grazing_cos * d->grazing_cos;
    memcpy(a.t.bp, d->target.bp, sizeof a.t.bp);
    memcpy(a.t.c, d->target.c, sizeof a.t.c);
    memcpy(a.t.P, d->target.P, sizeof a.t.P);
    for (int k = 0; k < S; ++k) {
        a.src[k].norm4 = (uint64_t)(uintptr_t)d->sources[k].norm4;
        a.src[k].cost = d->costs ? (uint64_t)(uintptr_t)d->costs[k] : 0;
        memcpy(a.src[k].bp, d->sources[k].bp, sizeof a.src[k].bp);
        memcpy(a.src[k].c, d->sources[k].c, sizeof a.src[k].c);
    }
    hipStream_t st = (hipStream_t)d->stream;
    const int nblocks = (int)((npix + prior::kBlock - 1) / prior::kBlock);
    if (device_ms) HIP_OK(hipEventRecord(sc.e0, st));
    HIP_OK(hipMemsetAsync(sc.zbuf, 0xFF, sizeof(unsigned long long) * npix, st));
    HIP_OK(hipMemsetAsync(sc.counts, 0, sizeof(uint32_t) * 3 * prior::kSlots, st));
    hipLaunchKernelGGL(prior::splat_kernel, dim3(nblocks, S), dim3(prior::kBlock), 0, st, a, sc.zbuf);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(prior::resolve_kernel, dim3(nblocks), dim3(prior::kBlock), 0, st, a, sc.zbuf, (float4 *)prior_dev,
                       sc.counts);
    HIP_OK(hipGetLastError());
    if (device_ms) HIP_OK(hipEventRecord(sc.e1, st));
    if (counts) {
        uint32_t c[3 * prior::kSlots];
        HIP_OK(hipMemcpyAsync(c, sc.counts, sizeof c, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) {
            counts[i] = 0;
            for (int k = 0; k < prior::kSlots; ++k) counts[i] += c[i * prior::kSlots + k];
        }
    }
    if (device_ms) {
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(device_ms, sc.e0, sc.e1));
    }
    if (!d->stream) HIP_OK(hipStreamSynchronize(st));  // the null stream: complete on return (gipuma_hip_downsample)
    return 0;
}

}  // namespace

extern "C" int gipuma_hip_prior_from_views(const gipuma_hip_prior_desc *d, float *prior_dev, int64_t counts[3], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    if (d->abi_version != GIPUMA_HIP_ABI_VERSION) return fail(GIPUMA_HIP_ERR_ARG, "prior: abi_version mismatch");
    if (d->rows < 1 || d->cols < 1 || (int64_t)d->rows * d->cols > (1ll << 30))
        return fail(GIPUMA_HIP_ERR_ARG, "prior: rows x cols out of range");
    if (d->n_sources < 1 || d->n_sources > GIPUMA_HIP_MAX_VIEWS) return fail(GIPUMA_HIP_ERR_ARG, "prior: n_sources must be 1..32");
    if (!d->sources) return fail(GIPUMA_HIP_ERR_ARG, "prior: null sources");
    for (int k = 0; k < d->n_sources; ++k) {
        if (!d->sources[k].norm4) return fail(GIPUMA_HIP_ERR_ARG, "prior: a source without a norm4 plane");
        if (d->costs && !d->costs[k]) return fail(GIPUMA_HIP_ERR_ARG, "prior: costs given, but a source without a cost plane");
    }
    if (d->costs && d->max_cost != d->max_cost) return fail(GIPUMA_HIP_ERR_ARG, "prior: max_cost is not a number");
    if (!(d->grazing_cos >= 0.f && d->grazing_cos <= 1.f)) return fail(GIPUMA_HIP_ERR_ARG, "prior: grazing_cos must be in 0..1");
    if (d->fill != 0 && d->fill != 1) return fail(GIPUMA_HIP_ERR_ARG, "prior: fill must be 0 or 1");
    if (!prior_dev) return fail(GIPUMA_HIP_ERR_ARG, "prior: null output plane");
    if ((int64_t)d->n_sources * d->rows * d->cols >= (1ll << 32))
        return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "prior: n_sources x rows x cols must stay below 2^32 (the key's low word)");
    if (const int rc = pm_host::check_device(d->device_id)) return rc;
    return run(d, prior_dev, counts, device_ms);
}
