// gipuma_normals.hip -- a cloud's normals and surface variation from its k nearest neighbours on gfx950: the geometric normal of
// the surface the points form, and how flat it is there (gipuma_hip_cloud_normals, restated on the CPU by
// tests/normals_ref.py on the lists of tests/knn_ref.py).
//
// The contract, defined without any grid (include/gipuma_hip.h).  list(i), m(i): DESIGN.md 17's k nearest other finite points of i
// within the radius, ascending in (d2, j), and their number.  A point that is not finite or has m(i) < 3 is SHORT: normal (0, 0, 0),
// variation +inf.  Otherwise, with M = m(i) + 1 (the point itself counts, at d = 0):
//     d_s = P_list(i)[s] - P_i per coordinate in float32, widened to float64;  S1 = sum d_s, S2 = sum d_s d_s^T in float64, in
//     slot order from 0 (each product of two widened floats is exact);  C = M S2 - S1 S1^T (M^2 times the covariance, six entries)
//     trace(C) = (C00 + C11) + C22 <= 0 or not finite: DEGENERATE, the short values
//     (w, V) = six sweeps of cyclic Jacobi on C in float64 (rotate, below);  e = the smallest w, the lowest index on a tie
//     normal = float32 of column e of V, its sign by `orient`;  variation = float32((w_e > 0 ? w_e : 0) / ((w_0 + w_1) + w_2))
// The list does not depend on the order the records are visited in and everything after it is a fixed sequence of
// float64 + - * / sqrt on the list in slot order: the outputs equal the restatement in every bit, at every grid, run after run.
//
// Launches, all on one stream:
//   cloud::OwnGrid (box_*, count_kernel<false>, scan_kernel, scatter_kernel; gipuma_cloud.hip)   the thinning's set-up
//   nrm::clear_kernel                              the short values everywhere: what a point that is never sorted keeps
//   nrm::estimate_kernel<K>, once, K = the smallest of 8 / 16 / 32 that holds k: one lane per sorted position.  Phase 1 is
//                                                  cloud::nearest_lists (pm_cloud.h), knn::topk_kernel's walk and insertion; phase
//                                                  2, fully unrolled over the slots so that the list stays in named registers,
//                                                  gathers P_j from the caller's array and accumulates S1, S2; then C, the sweeps,
//                                                  the selection and the sign.  The results go to the caller's index.
// No scratch memory, no flat instructions, no LDS, integer atomics only.  The unit spells no float32 fused multiply-add; the float64
// ones in its assembly are the compiler's own correctly rounded `/` and sqrt.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pm_cloud.h"

using pm_host::fail;

namespace nrm {

using namespace cloud;  // (Rec, Grid, nearest_lists, kBlock)

constexpr int kMinK = 3, kMaxK = 32;
enum { kEstimated = cloud::kStats, kFlipped, kCounters };  // the device counters, behind cloud's (kTargets: the finite points)

// what a point that is never sorted keeps (each where the caller asked for the output); the six entries of C are 0 there
__global__ __launch_bounds__(kBlock) void clear_kernel(uint32_t n, float *__restrict__ out_normal, float *__restrict__ out_variation,
                                                       uint32_t *__restrict__ out_m, double *__restrict__ out_scatter)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (out_normal)
        for (int c = 0; c < 3; ++c) out_normal[3 * (size_t)i + c] = 0.f;
    if (out_variation) out_variation[i] = INFINITY;
    if (out_m) out_m[i] = 0u;
    if (out_scatter)
        for (int c = 0; c < 6; ++c) out_scatter[6 * (size_t)i + c] = 0.0;
}

// One Jacobi rotation of the pair (p, q), r the third index, on the symmetric A and the accumulated V (rows 0 .. 2), entry by
// entry in this order; skipped where a_pq is exactly 0.  theta^2 may overflow to +inf: then t = +-0, c = 1, s = +-0, the diagonal
// and the other entries keep their values and a_pq -- below 2^-500 of the diagonal's difference -- becomes 0.
__device__ __forceinline__ void rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                       double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double u = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double t = theta < 0.0 ? -u : u;  // (sgn(0) = +1)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;
    v0p = c * x0 - s * y0;
    v0q = s * x0 + c * y0;
    v1p = c * x1 - s * y1;
    v1q = s * x1 + c * y1;
    v2p = c * x2 - s * y2;
    v2q = s * x2 + c * y2;
}

__device__ __forceinline__ double canonical(double x) { return x != x ? __longlong_as_double(0x7ff8000000000000ll) : x; }

// *n_sorted: the number of sorted (finite) points, as the histogram left it on the device.  pts: the caller's array, from which
// phase 2 gathers by the listed index.  orient 0 / 1 / 2: DESIGN.md 19's sign rules; view: the viewpoint, guide: the guide normals.
template <int K>
__global__ __launch_bounds__(kBlock) void estimate_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends,
                                                          const uint32_t *__restrict__ n_sorted, Grid g, float reach, int k,
                                                          const float *__restrict__ pts, int orient, float view_x, float view_y,
                                                          float view_z, const float *__restrict__ guide, float *__restrict__ out_normal,
                                                          float *__restrict__ out_variation, uint32_t *__restrict__ out_m,
                                                          double *__restrict__ out_scatter, uint32_t *__restrict__ counters)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    bool estimated = false, flipped = false;
    if (pos < *n_sorted) {
        const Rec a = sorted[pos];
        float d[K];
        uint32_t j[K];
        nearest_lists<K>(sorted, ends, g, reach, a, pos, d, j);
        // phase 2: the sums over the first k slots, in slot order (the filled slots are the first m)
        uint32_t m = 0;
        double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < k && j[s] != ~0u) {
                const float *q = pts + 3 * (size_t)j[s];
                const double dx = (double)(q[0] - a.x), dy = (double)(q[1] - a.y), dz = (double)(q[2] - a.z);
                ++m;
                s1x = s1x + dx;
                s1y = s1y + dy;
                s1z = s1z + dz;
                sxx = sxx + dx * dx;
                sxy = sxy + dx * dy;
                sxz = sxz + dx * dz;
                syy = syy + dy * dy;
                syz = syz + dy * dz;
                szz = szz + dz * dz;
            }
        if (out_m) out_m[a.j] = m;
        if (m >= (uint32_t)kMinK) {
            const double M = (double)(m + 1u);
            double a00 = M * sxx - s1x * s1x, a01 = M * sxy - s1x * s1y, a02 = M * sxz - s1x * s1z;
            double a11 = M * syy - s1y * s1y, a12 = M * syz - s1y * s1z, a22 = M * szz - s1z * s1z;
            if (out_scatter) {
                double *c = out_scatter + 6 * (size_t)a.j;
                c[0] = canonical(a00), c[1] = canonical(a01), c[2] = canonical(a02);
                c[3] = canonical(a11), c[4] = canonical(a12), c[5] = canonical(a22);
            }
            const double trace = (a00 + a11) + a22;
            estimated = trace > 0.0 && trace < (double)INFINITY;
            if (estimated) {
                double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
                for (int sweep = 0; sweep < 6; ++sweep) {
                    rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
                    rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
                    rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
                }
                // (selects of VALUES, the unary plus: a conditional on the variables themselves selects their addresses, and the
                //  nine entries of V then go through scratch memory)
                const bool b1 = a11 < a00;
                const double w1 = b1 ? +a11 : +a00;
                const bool b2 = a22 < w1;
                const double w = b2 ? +a22 : w1;
                const double ex = b2 ? +v02 : b1 ? +v01 : +v00, ey = b2 ? +v12 : b1 ? +v11 : +v10, ez = b2 ? +v22 : b1 ? +v21 : +v20;
                float nx = (float)ex, ny = (float)ey, nz = (float)ez;
                const float variation = (float)((w > 0.0 ? w : 0.0) / ((a00 + a11) + a22));
                // the sign: the dot of rule 1 or 2 where it is finite and not 0, else rule 0
                double dot = 0.0;
                if (orient == 1)
                    dot = ((double)nx * ((double)view_x - (double)a.x) + (double)ny * ((double)view_y - (double)a.y)) +
                          (double)nz * ((double)view_z - (double)a.z);
                if (orient == 2) {
                    const float *gd = guide + 3 * (size_t)a.j;
                    dot = ((double)nx * (double)gd[0] + (double)ny * (double)gd[1]) + (double)nz * (double)gd[2];
                }
                if (dot != 0.0 && fabs(dot) < (double)INFINITY) {
                    flipped = dot < 0.0;
                } else {  // the component of largest magnitude is made positive, the lowest axis on a tie
                    float big = nx;
                    if (fabsf(ny) > fabsf(big)) big = ny;
                    if (fabsf(nz) > fabsf(big)) big = nz;
                    flipped = big < 0.f;
                }
                if (flipped) nx = -nx, ny = -ny, nz = -nz;
                if (out_normal) {
                    float *o = out_normal + 3 * (size_t)a.j;
                    o[0] = nx, o[1] = ny, o[2] = nz;
                }
                if (out_variation) out_variation[a.j] = variation;
            }
        }
    }
    // the counters: one atomic each per wavefront (integer sums: the totals do not depend on the order)
    const uint64_t be = __ballot(estimated), bf = __ballot(flipped);
    if ((threadIdx.x & 63) == 0) {
        if (be) atomicAdd(&counters[kEstimated], (uint32_t)__popcll(be));
        if (bf) atomicAdd(&counters[kFlipped], (uint32_t)__popcll(bf));
    }
}

}  // namespace nrm

namespace {

int run_normals(const gipuma_hip_normals_desc *d, float *normal_dev, float *variation_dev, uint32_t *count_dev, double *scatter_dev,
                int64_t info[8], float *device_ms)
{
    const uint32_t n = (uint32_t)d->n_points, k = (uint32_t)d->k;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    cloud::OwnGrid og;
    uint32_t counters[nrm::kCounters] = {};
    float ms = 0.f;

    if (n) {
        // every output comes out of the kernel with the estimated points' entries written over the clearing
        if (const int rc = og.box.alloc(sc, n)) return rc;
        HIP_OK(hipEventRecord(sc.e[0], st));
        hipLaunchKernelGGL(nrm::clear_kernel, cloud::blocks_for(n), dim3(cloud::kBlock), 0, st, n, normal_dev, variation_dev, count_dev,
                           scatter_dev);
        HIP_OK(hipGetLastError());
        if (const int rc = og.lay(sc, d->points, n, d->radius, d->grid, nrm::kCounters)) return rc;
        if (og.any) {  // (else: every point is short)
            if (const int rc = og.sort(st, d->points, n)) return rc;
            const auto kernel = k <= 8 ? nrm::estimate_kernel<8> : k <= 16 ? nrm::estimate_kernel<16> : nrm::estimate_kernel<nrm::kMaxK>;
            hipLaunchKernelGGL(kernel, cloud::blocks_for(n), dim3(cloud::kBlock), 0, st, og.sorted, og.cells, og.counters + cloud::kTargets,
                               og.l.g, cloud::kReach * d->radius, (int)k, d->points, (int)d->orient, d->viewpoint[0], d->viewpoint[1],
                               d->viewpoint[2], d->guide, normal_dev, variation_dev, count_dev, scatter_dev, og.counters);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(counters, og.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipEventRecord(sc.e[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms, sc.e[0], sc.e[1]));
    }
    og.report(info, n, counters[cloud::kTargets], counters[nrm::kEstimated], counters[nrm::kFlipped]);
    if (device_ms) *device_ms = ms;
    return 0;
}

}  // namespace

extern "C" int gipuma_hip_cloud_normals(const gipuma_hip_normals_desc *d, float *normal_dev, float *variation_dev, uint32_t *count_dev,
                                        double *scatter_dev, int64_t info[8], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    const char *own = d->k < nrm::kMinK || d->k > nrm::kMaxK ? "k must be 3..32"
                      : d->orient < 0 || d->orient > 2       ? "orient must be 0 (largest component), 1 (viewpoint) or 2 (guide)"
                      : d->orient == 2 && d->n_points && !d->guide ? "orient 2 needs the guide normals"
                      : d->orient == 1 && !(std::isfinite(d->viewpoint[0]) && std::isfinite(d->viewpoint[1]) && std::isfinite(d->viewpoint[2]))
                          ? "orient 1 needs a finite viewpoint" : nullptr;
    if (const int rc = cloud::check_args("normals", d->abi_version, d->n_points, 0,
                                         d->n_points && (!d->points || (!normal_dev && !variation_dev && !count_dev && !scatter_dev)),
                                         "radius", d->radius, own, d->grid, d->device_id))
        return rc;
    return run_normals(d, normal_dev, variation_dev, count_dev, scatter_dev, info, device_ms);
}
