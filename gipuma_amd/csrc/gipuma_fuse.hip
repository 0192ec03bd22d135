// gipuma_fuse.hip -- depth-map fusion on gfx950: per-view (n_world, depth) planes -> one point cloud.
//
// The contract (include/gipuma_hip.h) is restated on the CPU in float32 by tests/fusion_ref.py; every
// operation below is one of + - * /, sqrtf, floorf in the order the contract writes it, compiled with -ffp-contract=off,
// so the two agree in every bit.
//
// Per view i, on one stream, three launches:
//   fuse::evaluate_kernel  one lane per pixel of view i: back-project, test against every other view (a wave-uniform
//                          loop; the view table is read with scalar loads, the partner pixel with one 16-byte gather),
//                          average, and -- for an emitted pixel -- mark the consistent partner pixels in their views'
//                          `used` masks (a second pass over the partners re-runs the tests: no view limit below 512).
//                          Writes the pixel's record to a staging plane, its emit flag and its workgroup's count.
//   fuse::scan_kernel      one workgroup: exclusive scan of the workgroup counts, and the view's total.
//   fuse::scatter_kernel   the emitted records, compacted in (y, x) order, to the output after the earlier views'.
// The only stores of evaluate_kernel that other lanes read are idempotent byte stores of 1 to OTHER views' masks, and the
// consistency test does not read those masks; they reach view i + 1 through the kernel boundary.  No atomics: the
// result does not depend on the launch geometry or on the order workgroups run in.  The host reads each view's total
// (4 bytes) before its scatter, to grow the output buffer when needed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "pm_host.h"
#include "pm_view.h"

using pm_host::fail;

namespace fuse {

constexpr int kBlock = 256;  // pixels per workgroup of evaluate / scatter: 4 wavefronts
constexpr int kScan = 1024;  // threads of the scan workgroup

using namespace pm_view;  // the contract's operation order: load_global, valid_depth, backproject, project, dot

struct View {  // gipuma_hip_fusion_view with the planes as integers (device table, scalar loads)
    uint64_t norm4, gray;
    float bp[9], c[3], P[12], fb;
    float pad[3];
};
struct Params {
    int rows, cols, n_views, num_consistent;
    float disp_thresh, cos_t, depth_min, depth_max;
};

// The consistency test of X (normal n) against view v.  On success q = the partner's pixel index, (qx, qy) its
// coordinates and m its (n', z').
__device__ __forceinline__ bool consistent(const View &v, const Params &p, const Vec3 &X, const Vec3 &n, int &q, float &qx,
                                           float &qy, float4 &m)
{
    const Vec3 h = project(v, X);
    if (!(h.z > 0.f)) return false;
    qx = floorf(h.x / h.z + 0.5f);
    qy = floorf(h.y / h.z + 0.5f);
    if (!(qx >= 0.f && qx <= (float)(p.cols - 1) && qy >= 0.f && qy <= (float)(p.rows - 1))) return false;
    q = (int)qy * p.cols + (int)qx;
    m = load_global<float4>(v.norm4, q);
    if (!valid_depth(m.w, p)) return false;
    if (!(fabsf(v.fb / h.z - v.fb / m.w) < p.disp_thresh)) return false;
    return dot(n, Vec3{m.x, m.y, m.z}) > p.cos_t;
}

__global__ __launch_bounds__(kBlock) void evaluate_kernel(const View *__restrict__ views, Params p, int i,
                                                          uint8_t *__restrict__ used, float4 *__restrict__ stage,
                                                          uint8_t *__restrict__ flags, uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t wave_counts[kBlock / 64];
    const int npix = p.rows * p.cols;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    bool emit = false;
    if (pix < npix) {
        const View &vi = views[i];
        const float4 s = load_global<float4>(vi.norm4, pix);
        const float z = s.w;
        if (valid_depth(z, p) && !used[(size_t)i * npix + pix]) {
            const Vec3 X = backproject(vi, z, (float)(pix % p.cols), (float)(pix / p.cols));
            const Vec3 n = {s.x, s.y, s.z};
            float S0 = X.x, S1 = X.y, S2 = X.z, N0 = s.x, N1 = s.y, N2 = s.z;
            float SG = vi.gray ? load_global<float>(vi.gray, pix) : 0.f;
            int count = 0;
            for (int j = 0; j < p.n_views; ++j) {  // wave-uniform
                if (j == i) continue;
                const View &vj = views[j];
                int q;
                float qx, qy;
                float4 m;
                if (!consistent(vj, p, X, n, q, qx, qy, m)) continue;
                ++count;
                const Vec3 Xj = backproject(vj, m.w, qx, qy);
                S0 += Xj.x;
                S1 += Xj.y;
                S2 += Xj.z;
                N0 += m.x;
                N1 += m.y;
                N2 += m.z;
                if (vj.gray) SG += load_global<float>(vj.gray, q);
            }
            if (count >= p.num_consistent) {
                emit = true;
                const float k = (float)(count + 1);
                const float len = sqrtf((N0 * N0 + N1 * N1) + N2 * N2);
                const float g = fminf(255.f, floorf(SG / k + 0.5f));
                stage[2 * (size_t)pix] = make_float4(S0 / k, S1 / k, S2 / k, N0 / len);
                stage[2 * (size_t)pix + 1] = make_float4(N1 / len, N2 / len, g, 0.f);
                for (int j = 0; j < p.n_views; ++j) {  // the marks: the same tests once more
                    if (j == i) continue;
                    int q;
                    float qx, qy;
                    float4 m;
                    if (consistent(views[j], p, X, n, q, qx, qy, m)) used[(size_t)j * npix + q] = 1;
                }
            }
        }
        flags[pix] = emit ? 1 : 0;
    }
    const uint64_t b = __ballot(emit);
    if ((threadIdx.x & 63) == 0) wave_counts[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += wave_counts[w];
        block_counts[blockIdx.x] = t;
    }
}

// exclusive scan of n workgroup counts (one workgroup, chunks of kScan); *total = their sum
__global__ __launch_bounds__(kScan) void scan_kernel(const uint32_t *__restrict__ counts, uint32_t *__restrict__ offsets, int n,
                                                     uint32_t *__restrict__ total)
{
    __shared__ uint32_t s[kScan];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < n; base += kScan) {
        const int k = base + t;
        const uint32_t v = k < n ? counts[k] : 0u;
        s[t] = v;
        __syncthreads();
        for (int off = 1; off < kScan; off <<= 1) {
            const uint32_t a = t >= off ? s[t - off] : 0u;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (k < n) offsets[k] = carry + s[t] - v;
        carry += s[kScan - 1];
        __syncthreads();  // (every lane has read s[kScan - 1] before the next chunk overwrites it)
    }
    if (t == 0) *total = carry;
}

__global__ __launch_bounds__(kBlock) void scatter_kernel(const uint8_t *__restrict__ flags, const float4 *__restrict__ stage,
                                                         const uint32_t *__restrict__ offsets, int npix, float4 *__restrict__ out)
{
    __shared__ uint32_t wave_counts[kBlock / 64];
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    const bool emit = pix < npix && flags[pix];
    const uint64_t b = __ballot(emit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_counts[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (emit) {
        uint32_t dst = offsets[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) dst += wave_counts[w];
        out[2 * (size_t)dst] = stage[2 * (size_t)pix];
        out[2 * (size_t)dst + 1] = stage[2 * (size_t)pix + 1];
    }
}

}  // namespace fuse

struct gipuma_hip_fusion {
    int device = 0;
    int rows = 0, cols = 0, n_views = 0;
    int64_t n_points = 0;
    std::vector<int64_t> per_view;
    float ms = 0.f;
    float4 *points = nullptr;  // n_points x 2 float4: (x, y, z, nx), (ny, nz, gray, 0)
    uint8_t *used = nullptr;   // n_views x rows x cols
};

namespace {

int run(const gipuma_hip_fusion_desc *d, gipuma_hip_fusion *f)
{
    const int V = d->n_views, npix = d->rows * d->cols;
    const int nblocks = (npix + fuse::kBlock - 1) / fuse::kBlock;
    f->device = d->device_id;
    f->rows = d->rows;
    f->cols = d->cols;
    f->n_views = V;
    f->per_view.assign(V, 0);
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;  // the call's scratch: freed on every way out of gipuma_hip_fuse
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    std::vector<fuse::View> table(V);
    for (int v = 0; v < V; ++v) {
        const gipuma_hip_fusion_view &s = d->views[v];
        fuse::View &t = table[v];
        memset(&t, 0, sizeof t);
        t.norm4 = (uint64_t)(uintptr_t)s.norm4;
        t.gray = (uint64_t)(uintptr_t)s.gray;
        memcpy(t.bp, s.bp, sizeof t.bp);
        memcpy(t.c, s.c, sizeof t.c);
        memcpy(t.P, s.P, sizeof t.P);
        t.fb = s.fb;
    }
    fuse::Params p;
    p.rows = d->rows;
    p.cols = d->cols;
    p.n_views = V;
    p.num_consistent = d->num_consistent;
    p.disp_thresh = d->disp_thresh;
    p.cos_t = (float)cos((double)d->normal_thresh * M_PI / 180.0);
    p.depth_min = d->depth_min;
    p.depth_max = d->depth_max;

    fuse::View *views;
    float4 *stage;
    uint8_t *flags;
    uint32_t *counts, *offsets, *total;
    if (sc.alloc(views, V) || sc.alloc(stage, 2 * (size_t)npix) || sc.alloc(flags, npix) || sc.alloc(counts, nblocks) ||
        sc.alloc(offsets, nblocks) || sc.alloc(total, 1))
        return GIPUMA_HIP_ERR_DEVICE;
    HIP_OK(hipMalloc(&f->used, (size_t)V * npix));  // (what outlives the call is the handle's)
    int64_t capacity = npix;
    HIP_OK(hipMalloc(&f->points, sizeof(float4) * 2 * (size_t)capacity));
    HIP_OK(hipMemcpyAsync(views, table.data(), sizeof(fuse::View) * V, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(f->used, 0, (size_t)V * npix, st));

    HIP_OK(hipEventRecord(sc.e[0], st));
    for (int i = 0; i < V; ++i) {
        hipLaunchKernelGGL(fuse::evaluate_kernel, dim3(nblocks), dim3(fuse::kBlock), 0, st, views, p, i, f->used, stage, flags, counts);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(fuse::scan_kernel, dim3(1), dim3(fuse::kScan), 0, st, counts, offsets, nblocks, total);
        HIP_OK(hipGetLastError());
        uint32_t n = 0;
        HIP_OK(hipMemcpyAsync(&n, total, sizeof n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (n > (uint32_t)npix) return fail(GIPUMA_HIP_ERR_DEVICE, "fusion: a view emitted more points than it has pixels");
        if (f->n_points + n > capacity) {  // grow (doubling), keeping the points of the earlier views
            int64_t want = capacity;
            while (want < f->n_points + n) want *= 2;
            float4 *grown = nullptr;
            HIP_OK(hipMalloc(&grown, sizeof(float4) * 2 * (size_t)want));
            hipError_t e = hipMemcpyAsync(grown, f->points, sizeof(float4) * 2 * (size_t)f->n_points, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                (void)hipFree(grown);
                return fail(GIPUMA_HIP_ERR_DEVICE, "fusion: growing the point buffer: %s", hipGetErrorString(e));
            }
            (void)hipFree(f->points);
            f->points = grown;
            capacity = want;
        }
        if (n) {
            hipLaunchKernelGGL(fuse::scatter_kernel, dim3(nblocks), dim3(fuse::kBlock), 0, st, flags, stage, offsets, npix,
                               f->points + 2 * f->n_points);
            HIP_OK(hipGetLastError());
        }
        f->per_view[i] = n;
        f->n_points += n;
    }
    HIP_OK(hipEventRecord(sc.e[1], st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipEventElapsedTime(&f->ms, sc.e[0], sc.e[1]));
    return 0;
}

}  // namespace

extern "C" {

int gipuma_hip_fuse(const gipuma_hip_fusion_desc *d, gipuma_hip_fusion **out)
{
    if (!out) return fail(GIPUMA_HIP_ERR_ARG, "null out pointer");
    *out = nullptr;
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    if (d->abi_version != GIPUMA_HIP_ABI_VERSION) return fail(GIPUMA_HIP_ERR_ARG, "fusion: abi_version mismatch");
    if (d->rows < 1 || d->cols < 1 || (int64_t)d->rows * d->cols > (1ll << 30))
        return fail(GIPUMA_HIP_ERR_ARG, "fusion: rows x cols out of range");
    if (d->n_views < 2 || d->n_views > GIPUMA_HIP_FUSION_MAX_VIEWS)
        return fail(GIPUMA_HIP_ERR_ARG, "fusion: n_views must be 2..512 (MAX_IMAGES)");
    if (d->num_consistent < 1) return fail(GIPUMA_HIP_ERR_ARG, "fusion: num_consistent must be >= 1");
    if (!d->views) return fail(GIPUMA_HIP_ERR_ARG, "fusion: null views");
    for (int v = 0; v < d->n_views; ++v)
        if (!d->views[v].norm4) return fail(GIPUMA_HIP_ERR_ARG, "fusion: a view without a norm4 plane");
    if (!(d->disp_thresh >= 0.f) || !(d->normal_thresh >= 0.f))
        return fail(GIPUMA_HIP_ERR_ARG, "fusion: thresholds must be >= 0");
    if (const int rc = pm_host::check_device(d->device_id)) return rc;
    gipuma_hip_fusion *f = new (std::nothrow) gipuma_hip_fusion;
    if (!f) return fail(GIPUMA_HIP_ERR_DEVICE, "out of host memory");
    const int rc = run(d, f);
    if (rc) {
        gipuma_hip_fusion_free(f);
        return rc;
    }
    *out = f;
    return 0;
}

int gipuma_hip_fusion_count(const gipuma_hip_fusion *f, int64_t *n_points, int64_t *per_view, float *device_ms)
{
    if (!f) return fail(GIPUMA_HIP_ERR_ARG, "null fusion handle");
    if (n_points) *n_points = f->n_points;
    if (per_view) memcpy(per_view, f->per_view.data(), sizeof(int64_t) * f->per_view.size());
    if (device_ms) *device_ms = f->ms;
    return 0;
}

int gipuma_hip_fusion_points(const gipuma_hip_fusion *f, void *vertices, int64_t first, int64_t count)
{
    if (!f || (!vertices && count)) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    if (first < 0 || count < 0 || first > f->n_points - count) return fail(GIPUMA_HIP_ERR_ARG, "fusion: point range out of bounds");
    if (!count) return 0;
    HIP_OK(hipSetDevice(f->device));
    std::vector<float4> rec(2 * (size_t)count);
    HIP_OK(hipMemcpy(rec.data(), f->points + 2 * first, sizeof(float4) * rec.size(), hipMemcpyDeviceToHost));
    unsigned char *o = (unsigned char *)vertices;
    for (int64_t k = 0; k < count; ++k, o += 27) {
        const float4 a = rec[2 * k], b = rec[2 * k + 1];
        const float v[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        memcpy(o, v, sizeof v);
        o[24] = o[25] = o[26] = (unsigned char)b.z;
    }
    return 0;
}

int gipuma_hip_fusion_used(const gipuma_hip_fusion *f, uint8_t *masks)
{
    if (!f || !masks) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    HIP_OK(hipSetDevice(f->device));
    HIP_OK(hipMemcpy(masks, f->used, (size_t)f->n_views * f->rows * f->cols, hipMemcpyDeviceToHost));
    return 0;
}

int gipuma_hip_fusion_free(gipuma_hip_fusion *f)
{
    if (!f) return 0;
    (void)hipSetDevice(f->device);
    (void)hipFree(f->points);
    (void)hipFree(f->used);
    delete f;
    return 0;
}

}  // extern "C"
