// pm_cloud.h -- what the cloud units share (gipuma_cloud.hip: search, thinning, neighbour count, k-NN lists; gipuma_components.hip:
// connected components; gipuma_normals.hip: normals from the k-NN lists).  Device: the sorted record, the grid, cell_of, d2_of
// (the contract's d2), Reach (the cells a lane visits, with kReach: why no neighbour is skipped) and nearest_lists (a lane's k-NN
// list).  Host: Box, Layout and OwnGrid, a cloud sorted on a grid over its
// own box, and check_args, the entry points' common checks.  The set-up KERNELS (box, histogram, scan, scatter) are defined
// once, in gipuma_cloud.hip; the host steps that launch them are out-of-line functions of that unit, declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pm_host.h"

namespace cloud {

constexpr int kBlock = 256;        // points per workgroup: 4 wavefronts
constexpr int kBoxBlocks = 1024;   // workgroups (at most) of the first box stage
constexpr int kMaxGrid = 256;      // cells along the longest axis: at most 2^24 cells
enum { kEarly = 0, kSearched = 1, kFound = 2, kTargets = 3, kStats = 4 };  // the device counters

struct Grid {
    float lo[3], hi[3];  // bounding box of the finite targets
    float h, inv_h;      // cell edge, 1 / h
    float r2;            // max_dist^2
    int g[3];            // cells per axis, 1 .. kMaxGrid
};

struct __align__(16) Rec {  // a sorted point: its coordinates and its index in the caller's array
    float x, y, z;
    int32_t j;
};

// The cell of coordinate p along an axis with g cells: clamp(floor((p - lo) * inv_h), 0, g - 1).  p - lo, the product
// with inv_h > 0, floorf, the clamp and the conversion are each non-decreasing in p, so cell_of is MONOTONIC in p; the
// search relies on nothing else about it.  (Clamped as a float, before the conversion: a query far outside the box may
// give +-inf here, never NaN -- p and lo are finite, inv_h is finite and > 0.)  The clamp is what places a query outside
// the box: in the nearest cell of the border, which keeps the monotonicity.
__device__ __forceinline__ int cell_of(float p, float lo, float inv_h, int g)
{
    if (g == 1) return 0;
    const float t = floorf((p - lo) * inv_h);
    return (int)fminf(fmaxf(t, 0.f), (float)(g - 1));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// The contract's d2 of a point a and a sorted point b, the one place it is written for every client's kernel.
__device__ __forceinline__ float d2_of(const Rec &a, const Rec &b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// The reach of a lane's cell range.  Lane a visits, per axis k, the cells cell_of(fl(a_k - reach)) .. cell_of(fl(a_k +
// reach)) with reach = fl(kReach * radius).  No neighbour is skipped: let b be finite with d2(a, b) <= r2.
//   * d2 is a sum of non-negative floats and rounding is monotonic, so fl(d_k * d_k) <= d2 <= r2 = fl(radius * radius)
//     <= radius^2 (1 + 2^-24) for d_k = fl(a_k - b_k).  Either d_k * d_k < 2^-126, and then |d_k| < 2^-63 < radius, or
//     the product is rounded with relative error 2^-24: d_k^2 <= radius^2 (1 + 2^-24) / (1 - 2^-24).  A difference of
//     floats never underflows, |a_k - b_k| <= |d_k| / (1 - 2^-24).  Together the REAL |a_k - b_k| <= radius (1 + 2^-22).
//   * reach >= 1.01 (1 - 2^-24)^2 radius > 1.009 radius (kReach is 1.01 rounded to a float; no underflow, the grid is
//     only used for 2^-40 <= radius <= 2^40), so the real x = a_k - reach < a_k - radius (1 + 2^-22) <= b_k.  b_k is a
//     float and rounding is monotonic: b_k >= fl(x), the value the lane computes.  An overflow to -inf only lowers it.
//   * cell_of is monotonic: cell_of(b_k) >= cell_of(fl(a_k - reach)).  The upper end is the mirror image.
// Nothing here depends on how cell_of rounds, only on its monotonicity; the slack of 0.9 % is spent on a bound that
// needs 2^-22.  Outside 2^-40 .. 2^40 (radius or cell edge) the host takes G = 1: one cell, every point visited.
// The statement is about this range and any finite b within the radius, whatever a client (thin, support) then asks of b.
constexpr float kReach = 1.01f;
inline bool reach_holds(float radius) { return radius >= 0x1p-40f && radius <= 0x1p40f; }

struct Reach {
    int x0, x1, y0, y1, z0, z1;

    __device__ __forceinline__ Reach(const Rec &a, float reach, const Grid &g)
        : x0(cell_of(a.x - reach, g.lo[0], g.inv_h, g.g[0])), x1(cell_of(a.x + reach, g.lo[0], g.inv_h, g.g[0])),
          y0(cell_of(a.y - reach, g.lo[1], g.inv_h, g.g[1])), y1(cell_of(a.y + reach, g.lo[1], g.inv_h, g.g[1])),
          z0(cell_of(a.z - reach, g.lo[2], g.inv_h, g.g[2])), z1(cell_of(a.z + reach, g.lo[2], g.inv_h, g.g[2])) {}
    // Cells are numbered x fastest and ends[] is what scatter_kernel leaves: the cells x0 .. x1 of the row (y, z) hold the
    // one contiguous range sorted[beg .. end), as a row of a shell's face does in search_kernel.
    __device__ __forceinline__ void row(const uint32_t *__restrict__ ends, const Grid &g, int y, int z, uint32_t &beg, uint32_t &end) const
    {
        const int c0 = (z * g.g[1] + y) * g.g[0] + x0;
        end = ends[c0 + (x1 - x0)];
        beg = c0 ? ends[c0 - 1] : 0u;
    }
};

// A lane's k-NN list, written once for knn::topk_kernel and nrm::estimate_kernel: the K smallest pairs (d2, j) of
// the finite points other than sorted[pos] within the radius of a = sorted[pos], ascending.  The lane walks the cells of its Reach
// row by row.  An empty slot is (+inf, -1) and indices compare UNSIGNED, so that -1 loses to every real index: where r2 = +inf
// a neighbour whose d2 overflowed to +inf (inf <= inf) displaces an empty slot and ties are still decided by the index.
// A record that passes the gate is below the last slot; it is carried down the list: each slot keeps the smaller of itself
// and the carry and hands the larger on, and what falls out of slot K - 1 is the old last pair.  Every loop over the slots is
// fully unrolled: d[] and j[] are 2K named registers, never indexed at run time.
template <int K>
__device__ __forceinline__ void nearest_lists(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends, const Grid &g, float reach,
                                              const Rec &a, uint32_t pos, float (&d)[K], uint32_t (&j)[K])
{
    const Reach r(a, reach, g);
#pragma unroll
    for (int s = 0; s < K; ++s) d[s] = INFINITY, j[s] = ~0u;
    for (int z = r.z0; z <= r.z1; ++z)
        for (int y = r.y0; y <= r.y1; ++y) {
            uint32_t p, end;
            for (r.row(ends, g, y, z, p, end); p < end; ++p) {
                const Rec b = sorted[p];
                float cd = d2_of(a, b);
                uint32_t cj = (uint32_t)b.j;
                if (!(cd <= g.r2) || p == pos || !(cd < d[K - 1] || (cd == d[K - 1] && cj < j[K - 1]))) continue;
#pragma unroll
                for (int s = 0; s < K; ++s) {
                    const bool below = cd < d[s] || (cd == d[s] && cj < j[s]);
                    const float td = d[s];
                    const uint32_t tj = j[s];
                    d[s] = below ? cd : td;
                    j[s] = below ? cj : tj;
                    cd = below ? td : cd;
                    cj = below ? tj : cj;
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host steps that build the grid.  They enqueue on the caller's stream, record no events and allocate only where the
// name says so: the callers place their timed windows around them.  The steps that launch a set-up kernel are defined in
// gipuma_cloud.hip, next to the kernels.
// ---------------------------------------------------------------------------------------------------------------------
#define PM_CLOUD_HOST __attribute__((visibility("hidden")))  // (out of line, in gipuma_cloud.hip; not part of the C-ABI)

inline dim3 blocks_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

// The box of a cloud's finite points.  enqueue() and read() are two calls, so that a caller may record an event between
// the kernels and the host's read.
struct Box {
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};  // lo[3], hi[3]; this where no point is finite
    float *partial = nullptr, *dev = nullptr;
    int nblocks = 0;

    int alloc(pm_host::CallScope &sc, uint32_t n)
    {
        nblocks = (int)(blocks_for(n).x < (uint32_t)kBoxBlocks ? blocks_for(n).x : (uint32_t)kBoxBlocks);
        return sc.alloc(partial, 6 * (size_t)nblocks) || sc.alloc(dev, 6) ? GIPUMA_HIP_ERR_DEVICE : 0;
    }
    PM_CLOUD_HOST int enqueue(hipStream_t st, const float *pts, uint32_t n) const;
    int read(hipStream_t st)  // (one host read)
    {
        HIP_OK(hipMemcpyAsync(v, dev, sizeof v, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    }
    bool any_finite() const { return v[0] <= v[3] && v[1] <= v[4] && v[2] <= v[5]; }
    float longest_extent() const { return fmaxf(fmaxf(fmaxf(0.f, v[3] - v[0]), v[4] - v[1]), v[5] - v[2]); }
};

// The grid over a box (lay_out, gipuma_cloud.hip): one cell edge h for all axes, G cells along the longest one.
struct Layout {
    Grid g;
    uint32_t ncells;
    int64_t report[4];  // G and the cells along x, y, z, as last_stats[0 .. 3] and the thinning's info[4 .. 7] report them
};

// A cloud sorted on a grid over its OWN box: the host set-up of the thinning, the neighbour count, the k-NN lists, the
// connected components and the normals.  The steps are calls of their own, as Box's are, so that a caller's event and its own memsets keep
// their places on the stream.
struct OwnGrid {
    Box box;        // (the caller allocates it, before its first event)
    Layout l = {};  // (the report stays 0 where no point is finite)
    bool any = false;
    Rec *sorted = nullptr;
    uint32_t *cells = nullptr, *counters = nullptr;
    int32_t *cellid = nullptr;

    // the box kernels and the host's read; where a point is finite (`any`) the layout (thin's automatic G for grid 0, one
    // cell unless reach_holds), the buffers and the memsets of the cells and of the caller's n_counters counters
    PM_CLOUD_HOST int lay(pm_host::CallScope &sc, const float *pts, uint32_t n, float radius, int grid, int n_counters);
    // the counting sort: cells[] goes out as the cells' ends, counters[kTargets] as the number of finite points
    PM_CLOUD_HOST int sort(hipStream_t st, const float *pts, uint32_t n) const;
    // info[8] of the four calls: kept (knn: complete), dropped (knn: short), not finite, the caller's fourth figure, G, cells x, y, z
    void report(int64_t info[8], uint32_t n, uint32_t finite, uint32_t kept, uint32_t fourth) const
    {
        const int64_t figures[4] = {kept, (int64_t)finite - kept, (int64_t)n - finite, fourth};
        if (info) memcpy(info, figures, sizeof figures), memcpy(info + 4, l.report, sizeof l.report);
    }
};

// The checks the entry points share, in their order, `what` before every text.  null_pointer: the entry point's own
// rule; own: the text of the first of its own checks that fails (null: none), reported in its place with own_rc.  The device
// comes last.
PM_CLOUD_HOST int check_args(const char *what, int abi_version, int64_t n0, int64_t n1, bool null_pointer, const char *dist_name,
                             float dist, const char *own, int grid, int device_id, int own_rc = GIPUMA_HIP_ERR_ARG);

}  // namespace cloud
