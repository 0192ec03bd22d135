// gipuma_cloud.hip -- nearest neighbours between two point clouds on gfx950: the search behind the cloud-against-cloud
// score (accuracy / completeness).
//
// The contract (include/gipuma_hip.h) is restated on the CPU in numpy float32 by tests/cloud_ref.py as a
// brute-force search.  For query a and target b, float32 without contraction (-ffp-contract=off):
//     dx = a.x - b.x;  dy = a.y - b.y;  dz = a.z - b.z;  d2 = (dx*dx + dy*dy) + dz*dz
//     b is a candidate iff it is finite, d2 is finite and d2 <= r2 (r2 = max_dist * max_dist);  the answer is the
//     smallest (d2, j).
// A minimum over (d2, j) pairs does not depend on the order the candidates are visited in, so a uniform grid over the
// targets may prune the search as long as it never skips a target the brute force would accept or prefer: the result
// then equals the brute force in every bit.  Why each shortcut keeps that promise is written where it is taken
// (cell_of, the box early-out in count_kernel, the shell stop in search_kernel).
//
// Launches, all on one stream:
//   cloud::box_partial_kernel / box_final_kernel   bounding box of the finite targets, a two-stage min / max reduction
//                                                  (no float atomics); the host reads the 24 bytes and lays the grid out
//   cloud::count_kernel<false>, scan_kernel, scatter_kernel    counting sort of the targets by cell: histogram, exclusive
//                                                  scan over the cells (one workgroup, carry across chunks), scatter
//   cloud::count_kernel<true>, scan_kernel, scatter_kernel     the same for the queries, so that the lanes of a wavefront
//                                                  visit the same cells; a query that is not finite or lies farther than
//                                                  max_dist from the targets' box is answered "none" here and not sorted
//   cloud::search_kernel                           one lane per sorted query: shells of growing Chebyshev distance around
//                                                  its cell; the result goes to the query's original index
// The histogram and the scatter use integer atomics (as the prior's z-buffer does), so the order of the points INSIDE a
// cell varies from run to run.  The contract's result does not depend on that order: the search carries (d2, j) compared
// lexicographically, and a cell's points are all visited or all skipped.
//
// The same grid has four more clients, on the cloud's own box: thinning it to a minimum point spacing (namespace thin,
// DESIGN.md 15, gipuma_hip_cloud_thin), counting each point's neighbours within a radius (namespace support, DESIGN.md
// 16, gipuma_hip_cloud_neighbours), listing each point's k nearest neighbours with their mean distance (namespace knn,
// DESIGN.md 17, gipuma_hip_cloud_knn) and -- the fourth, in a unit of its own, gipuma_components.hip -- labelling the
// connected components of its radius graph (namespace comp, DESIGN.md 18, gipuma_hip_cloud_components).  What they share is
// written once in namespace cloud, in pm_cloud.h.  Device: d2_of (the contract's d2, the search's too) and Reach (the cells a
// lane visits and a row's records, with kReach: why no neighbour is skipped).  Host: Box, Layout, OwnGrid, which runs the
// set-up for the four, and check_args; lay_out and sort_by_cell, which the search takes for its targets, stay here, as do the
// set-up kernels and the bodies of the host steps that launch them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pm_cloud.h"
#include "pm_hash.h"
#include "pm_host.h"

using pm_host::fail;
namespace thin { inline int automatic_grid(float longest, float radius); }  // (the thinning's rule, below; cloud::OwnGrid takes it)

namespace cloud {

constexpr int kScan = 1024;        // threads of the scan workgroup
constexpr int kItems = 16;         // cells per thread and chunk of the scan: a chunk is 16384 cells

// min of lo[3] / max of hi[3] over the workgroup, left in lane 0's m[]
__device__ __forceinline__ void reduce_box(float (*s)[kBlock], float m[6])
{
    const int t = threadIdx.x;
    for (int k = 0; k < 6; ++k) s[k][t] = m[k];
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (t < off)
            for (int k = 0; k < 6; ++k) s[k][t] = k < 3 ? fminf(s[k][t], s[k][t + off]) : fmaxf(s[k][t], s[k][t + off]);
        __syncthreads();
    }
    for (int k = 0; k < 6; ++k) m[k] = s[k][0];
}

// per workgroup: (lo, hi) of its finite points; +inf / -inf where it has none
__global__ __launch_bounds__(kBlock) void box_partial_kernel(const float *__restrict__ pts, uint32_t n, float *__restrict__ partial)
{
    __shared__ float s[6][kBlock];
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {  // (n < 2^31: i does not wrap)
        const float *p = pts + 3 * (size_t)i;
        const float x = p[0], y = p[1], z = p[2];
        if (!finite3(x, y, z)) continue;
        m[0] = fminf(m[0], x);
        m[1] = fminf(m[1], y);
        m[2] = fminf(m[2], z);
        m[3] = fmaxf(m[3], x);
        m[4] = fmaxf(m[4], y);
        m[5] = fmaxf(m[5], z);
    }
    reduce_box(s, m);
    if (threadIdx.x < 6) partial[blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void box_final_kernel(const float *__restrict__ partial, int nblocks, float *__restrict__ box)
{
    __shared__ float s[6][kBlock];
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
        for (int k = 0; k < 6; ++k) m[k] = k < 3 ? fminf(m[k], partial[b * 6 + k]) : fmaxf(m[k], partial[b * 6 + k]);
    reduce_box(s, m);
    if (threadIdx.x < 6) box[threadIdx.x] = s[threadIdx.x][0];
}

// The histogram: cellid[i] = the point's cell, or -1 for a point that takes no part; counts[cell] += 1.
// Targets: a point that is not finite takes no part (it is never a neighbour).
// Queries: a query that is not finite, or lies outside the targets' box by more than max_dist, is answered "none" here.
//   The box early-out, from monotonicity alone: every finite target b has lo <= b <= hi in each coordinate.  For a.x < lo.x,
//   rounding is monotonic, so fl(b.x - a.x) >= fl(lo.x - a.x) = ex >= 0: the contract's |dx| is at least ex, the same on the
//   other side with hi, and ex = 0 inside.  Squaring a non-negative float and adding non-negative floats are monotonic too:
//   the contract's d2 of EVERY target is >= E2 = (ex*ex + ey*ey) + ez*ez, computed in the contract's order.  E2 > r2
//   therefore means no candidate.  No margin is needed and none is taken.
template <bool kQuery>
__global__ __launch_bounds__(kBlock) void count_kernel(const float *__restrict__ pts, uint32_t n, Grid g, int32_t *__restrict__ cellid,
                                                       uint32_t *__restrict__ counts, float *__restrict__ out_d2,
                                                       int32_t *__restrict__ out_idx, uint32_t *__restrict__ stats)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool early = false, sorted = false;
    if (i < n) {
        const float *p = pts + 3 * (size_t)i;
        const float x = p[0], y = p[1], z = p[2];
        int c = -1;
        if (finite3(x, y, z)) {
            if (kQuery) {
                const float ex = fmaxf(fmaxf(g.lo[0] - x, x - g.hi[0]), 0.f);
                const float ey = fmaxf(fmaxf(g.lo[1] - y, y - g.hi[1]), 0.f);
                const float ez = fmaxf(fmaxf(g.lo[2] - z, z - g.hi[2]), 0.f);
                early = (ex * ex + ey * ey) + ez * ez > g.r2;
            }
            if (!early) {
                c = (cell_of(z, g.lo[2], g.inv_h, g.g[2]) * g.g[1] + cell_of(y, g.lo[1], g.inv_h, g.g[1])) * g.g[0] +
                    cell_of(x, g.lo[0], g.inv_h, g.g[0]);
                atomicAdd(&counts[c], 1u);
                sorted = true;
            }
        }
        cellid[i] = c;
        if (kQuery && c < 0) {
            out_d2[i] = INFINITY;
            out_idx[i] = -1;
        }
    }
    // the counters: one atomic per wavefront (integer sums: the totals do not depend on the order)
    const uint64_t be = __ballot(early), bs = __ballot(sorted);
    if ((threadIdx.x & 63) == 0) {
        if (kQuery && be) atomicAdd(&stats[kEarly], (uint32_t)__popcll(be));
        if (!kQuery && bs) atomicAdd(&stats[kTargets], (uint32_t)__popcll(bs));
    }
}

// Exclusive scan of n cell counts, in place (one workgroup; kItems consecutive cells per thread, chunks of kScan * kItems
// cells with a carry from chunk to chunk, as fuse::scan_kernel carries one); *total = their sum when asked for.
__global__ __launch_bounds__(kScan) void scan_kernel(uint32_t *__restrict__ cells, uint32_t n, uint32_t *__restrict__ total)
{
    __shared__ uint32_t s[kScan];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += kScan * kItems) {  // (n <= 2^24)
        const uint32_t k0 = base + t * kItems;
        uint32_t v[kItems], sum = 0;
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            v[e] = k0 + e < n ? cells[k0 + e] : 0u;
            sum += v[e];
        }
        s[t] = sum;
        __syncthreads();
        for (uint32_t off = 1; off < kScan; off <<= 1) {
            const uint32_t a = t >= off ? s[t - off] : 0u;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        uint32_t run = carry + s[t] - sum;
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            if (k0 + e < n) cells[k0 + e] = run;
            run += v[e];
        }
        carry += s[kScan - 1];
        __syncthreads();  // (every lane has read s[kScan - 1] before the next chunk overwrites it)
    }
    if (t == 0 && total) *total = carry;
}

// The scatter: cursor[] comes in as the cells' starts and goes out as their ENDS (each point takes the next free place of
// its cell), so cell c ends up holding sorted[c ? cursor[c - 1] : 0 .. cursor[c]).
__global__ __launch_bounds__(kBlock) void scatter_kernel(const float *__restrict__ pts, uint32_t n, const int32_t *__restrict__ cellid,
                                                         uint32_t *__restrict__ cursor, Rec *__restrict__ sorted)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cellid[i];
    if (c < 0) return;
    const float *p = pts + 3 * (size_t)i;
    const uint32_t pos = atomicAdd(&cursor[c], 1u);
    sorted[pos] = Rec{p[0], p[1], p[2], (int32_t)i};
}

// every query "none": the targets hold no finite point
__global__ __launch_bounds__(kBlock) void none_kernel(uint32_t n, float *__restrict__ out_d2, int32_t *__restrict__ out_idx)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out_d2[i] = INFINITY;
    out_idx[i] = -1;
}

// The slack of the shell stop.  After shells 0 .. s every cell within Chebyshev distance s of the query's cell has been
// visited (the grid's border clips the shells, it hides no cell).  An unvisited target b differs from the query a by at
// least s + 1 cells along some axis k; take cell(b) >= cell(a) + s + 1, the other side is the mirror image.  With
// t(p) = fl(fl(p - lo) * inv_h), the value cell_of floors and clamps:
//   * t(a) < cell(a) + 1.  By definition where a's cell is not clamped; a cell clamped from below has t(a) < 0 and
//     cell(a) = 0; a cell clamped from above is the axis' last one, and no cell lies beyond it.
//   * t(b) >= cell(b) >= cell(a) + s + 1: b's cell is not clamped from below (it is >= 1), and a clamp from above only
//     lowers the cell.
//   so t(b) - t(a) > s, whatever the rounding did.  Both bounds are at most kMaxGrid + 1 = 257, and t(p) carries two
//   roundings of relative size 2^-24 (p - lo, the product): against the real (p - lo) * inv_h each bound moves by at
//   most 257 * 2^-23 < 2^-14 cells, so the real (b_k - a_k) * inv_h > s - 2^-13.  inv_h = fl(1 / h) >= (1 - 2^-24) / h:
//   b_k - a_k > 0.9998 s h for s >= 1.
//   * The contract's d2 is a sum of non-negative terms, each of dx, dx*dx and the two sums rounded once:
//     d2 >= (b_k - a_k)^2 (1 - 2^-24)^5 > 0.9995 (s h)^2.  (No underflow: the grid is only used for 2^-40 <= h <= 2^40.)
//   * The threshold fl(fl(fl(0.99f * s) * h)^2) <= 0.99000002^2 (1 + 2^-24)^3 (s h)^2 < 0.9802 (s h)^2.
// Hence every unvisited target has d2 > threshold, STRICTLY, with 2 % to spare where 0.05 % are needed: it can neither
// beat nor tie a best_d2 <= threshold, and with threshold >= r2 it is no candidate.  The stop is tested from s = 1 on.
constexpr float kShellSlack = 0.99f;

__device__ __forceinline__ void visit(const Rec *__restrict__ sorted, uint32_t beg, uint32_t end, const Rec &a, float r2, float &best,
                                      int32_t &bj)
{
    for (uint32_t p = beg; p < end; ++p) {
        const Rec b = sorted[p];
        const float d2 = d2_of(a, b);
        // A d2 of +inf (an overflow; r2 may be +inf too) is no candidate: +inf means "none" and nothing else.  It never
        // passes d2 < best, and it ties best only while best is still INFINITY, i.e. bj = -1, which no index is below
        // (a SIGNED comparison).  A finite best has bj >= 0: the lowest index wins the tie.
        if (d2 <= r2 && (d2 < best || (d2 == best && b.j < bj))) {
            best = d2;
            bj = b.j;
        }
    }
}

// One lane per sorted query.  Cells are numbered x fastest, so the cells x0 .. x1 of one (y, z) row hold one contiguous
// range of the sorted targets: a row on a y or z face of the shell is visited as one range, any other row through the
// shell's two x ends only.
__global__ __launch_bounds__(kBlock) void search_kernel(const Rec *__restrict__ queries, const uint32_t *__restrict__ n_sorted,
                                                        const Rec *__restrict__ targets, const uint32_t *__restrict__ ends, Grid g,
                                                        float *__restrict__ out_d2, int32_t *__restrict__ out_idx,
                                                        uint32_t *__restrict__ stats)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool found = false;
    if (t < *n_sorted) {
        const Rec a = queries[t];
        const int cx = cell_of(a.x, g.lo[0], g.inv_h, g.g[0]), cy = cell_of(a.y, g.lo[1], g.inv_h, g.g[1]),
                  cz = cell_of(a.z, g.lo[2], g.inv_h, g.g[2]);
        float best = INFINITY;
        int32_t bj = -1;
        for (int s = 0;; ++s) {
            const int x0 = max(cx - s, 0), x1 = min(cx + s, g.g[0] - 1);
            const int y0 = max(cy - s, 0), y1 = min(cy + s, g.g[1] - 1);
            const int z0 = max(cz - s, 0), z1 = min(cz + s, g.g[2] - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.g[1] + y) * g.g[0];
                    if (abs(z - cz) == s || abs(y - cy) == s) {
                        const int c0 = row + x0, c1 = row + x1;
                        visit(targets, c0 ? ends[c0 - 1] : 0u, ends[c1], a, g.r2, best, bj);
                    } else {  // (s >= 1 here: the two ends are different cells)
                        if (cx - s >= 0) {
                            const int c = row + cx - s;
                            visit(targets, c ? ends[c - 1] : 0u, ends[c], a, g.r2, best, bj);
                        }
                        if (cx + s <= g.g[0] - 1) {
                            const int c = row + cx + s;
                            visit(targets, ends[c - 1], ends[c], a, g.r2, best, bj);
                        }
                    }
                }
            // the whole grid has been visited: the shell has left it on all six sides
            if (cx - s <= 0 && cx + s >= g.g[0] - 1 && cy - s <= 0 && cy + s >= g.g[1] - 1 && cz - s <= 0 && cz + s >= g.g[2] - 1)
                break;
            if (s >= 1) {  // (see kShellSlack)
                const float reach = (kShellSlack * (float)s) * g.h;
                const float thr = reach * reach;
                if ((bj >= 0 && best <= thr) || thr >= g.r2) break;
            }
        }
        found = bj >= 0;
        out_d2[a.j] = best;
        out_idx[a.j] = bj;
    }
    const uint64_t b = __ballot(found);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&stats[kFound], (uint32_t)__popcll(b));
}

// The automatic G from n_b.  Fused clouds are surface samples: of the G^3 cells of a grid, in the order of G^2 hold
// points.  G = ceil(sqrt(n_b / 2)) gives about two targets per occupied cell -- a first shell of some tens of distance
// tests -- until the cap of 256 (n_b > 131072); beyond it the cells fill up in proportion to n_b.
inline int automatic_grid(int64_t n_targets)
{
    const int g = (int)ceil(sqrt((double)n_targets / 2.0));
    return g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g;
}

// The set-up kernels' launches: Box::enqueue here, OwnGrid::lay and OwnGrid::sort below (pm_cloud.h declares them).
int Box::enqueue(hipStream_t st, const float *pts, uint32_t n) const
{
    hipLaunchKernelGGL(box_partial_kernel, dim3(nblocks), dim3(kBlock), 0, st, pts, n, partial);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(box_final_kernel, dim3(1), dim3(kBlock), 0, st, partial, nblocks, dev);
    HIP_OK(hipGetLastError());
    return 0;
}

// The grid over a box: one cell edge h for all axes, G cells along the longest one; an axis of zero extent gets one cell.
// One cell (G = 1: every point visited, the brute force) where a client's shortcut is not proven: h outside 2^-40 .. 2^40
// (squares would underflow or overflow; an infinite extent ends up here), or the client says that its own derivation does
// not hold (`shortcut_holds`: the search's kShellSlack wants a finite r2, the thinning's kReach a radius in that range).
inline Layout lay_out(const Box &box, int G, float r2, bool shortcut_holds)
{
    Layout l;
    Grid &g = l.g;
    float ext[3];
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = box.v[k];
        g.hi[k] = box.v[3 + k];
        ext[k] = box.v[3 + k] - box.v[k];
    }
    g.r2 = r2;
    g.h = box.longest_extent() / (float)G;
    if (!(g.h >= 0x1p-40f && g.h <= 0x1p40f) || !shortcut_holds) G = 1;
    if (G == 1) g.h = 1.f;
    g.inv_h = 1.f / g.h;
    for (int k = 0; k < 3; ++k) {
        const int cells = G == 1 || !(ext[k] > 0.f) ? 1 : (int)floorf(ext[k] * g.inv_h) + 1;
        g.g[k] = cells < 1 ? 1 : cells > G ? G : cells;
    }
    l.ncells = (uint32_t)g.g[0] * g.g[1] * g.g[2];
    l.report[0] = G;
    for (int k = 0; k < 3; ++k) l.report[1 + k] = g.g[k];
    return l;
}

// The counting sort of a cloud by cell: histogram, exclusive scan, scatter.  cells[ncells] comes in ZEROED (the caller's
// memset, wherever on the stream it stands) and goes out as the cells' ends; cellid[n] and sorted[n] are scratch and
// result.  kQuery, out_d2, out_idx: count_kernel's; *total = the number of sorted points when asked for.
template <bool kQuery>
int sort_by_cell(hipStream_t st, const float *pts, uint32_t n, const Layout &l, int32_t *cellid, uint32_t *cells, Rec *sorted,
                 float *out_d2, int32_t *out_idx, uint32_t *stats, uint32_t *total)
{
    hipLaunchKernelGGL(count_kernel<kQuery>, blocks_for(n), dim3(kBlock), 0, st, pts, n, l.g, cellid, cells, out_d2, out_idx, stats);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScan), 0, st, cells, l.ncells, total);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(scatter_kernel, blocks_for(n), dim3(kBlock), 0, st, pts, n, cellid, cells, sorted);
    HIP_OK(hipGetLastError());
    return 0;
}

// OwnGrid's two steps that launch (pm_cloud.h): the box kernels and the host's read, then the layout, the buffers and the
// memsets; the counting sort.
int OwnGrid::lay(pm_host::CallScope &sc, const float *pts, uint32_t n, float radius, int grid, int n_counters)
{
    if (const int rc = box.enqueue(sc.st, pts, n)) return rc;
    if (const int rc = box.read(sc.st)) return rc;
    if (!(any = box.any_finite())) return 0;
    l = lay_out(box, grid ? grid : thin::automatic_grid(box.longest_extent(), radius), radius * radius, reach_holds(radius));
    if (sc.alloc(cells, l.ncells) || sc.alloc(counters, n_counters) || sc.alloc(cellid, n) || sc.alloc(sorted, n))
        return GIPUMA_HIP_ERR_DEVICE;
    HIP_OK(hipMemsetAsync(cells, 0, sizeof(uint32_t) * l.ncells, sc.st));
    HIP_OK(hipMemsetAsync(counters, 0, sizeof(uint32_t) * n_counters, sc.st));
    return 0;
}

int OwnGrid::sort(hipStream_t st, const float *pts, uint32_t n) const
{
    return sort_by_cell<false>(st, pts, n, l, cellid, cells, sorted, nullptr, nullptr, counters, nullptr);
}

// The checks the entry points share (pm_cloud.h), in their order, `what` before every text.  null_pointer: the entry point's own
// rule; own: the text of the first of its own checks that fails (null: none), reported in its place with own_rc.  The device
// comes last.
int check_args(const char *what, int abi_version, int64_t n0, int64_t n1, bool null_pointer, const char *dist_name, float dist,
               const char *own, int grid, int device_id, int own_rc)
{
    if (abi_version != GIPUMA_HIP_ABI_VERSION) return fail(GIPUMA_HIP_ERR_ARG, "%s: abi_version mismatch", what);
    if (n0 < 0 || n1 < 0) return fail(GIPUMA_HIP_ERR_ARG, "%s: negative point count", what);
    if ((n0 | n1) >= (1ll << 31)) return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "%s: a cloud may hold at most 2^31 - 1 points", what);
    if (null_pointer) return fail(GIPUMA_HIP_ERR_ARG, "%s: null pointer with a non-zero point count", what);
    if (!(dist > 0.f) || !std::isfinite(dist)) return fail(GIPUMA_HIP_ERR_ARG, "%s: %s must be > 0 and finite", what, dist_name);
    if (own) return fail(own_rc, "%s: %s", what, own);
    if (grid < 0 || grid > cloud::kMaxGrid) return fail(GIPUMA_HIP_ERR_ARG, "%s: grid must be 0 (automatic) or 1..256", what);
    return pm_host::check_device(device_id);
}

}  // namespace cloud

// ---------------------------------------------------------------------------------------------------------------------
// Thinning to a minimum point spacing (restated on the CPU by tests/thin_ref.py).  The contract, defined
// without any grid: the finite points are visited in ascending key(i) = (prio(i), i); a point is KEPT iff no point kept
// before it has d2 <= r2 (cloud's d2, inclusive radius) -- the lexicographically first maximal independent set of the
// radius graph.  A point that is not finite is never kept and never suppresses.
//
// Launches, all on one stream:
//   cloud::OwnGrid (box_*, count_kernel<false>, scan_kernel, scatter_kernel)   the finite points sorted by cell, once
//   thin::round_kernel, once per round t = 1, 2, ...   one lane per UNDECIDED point, taken from a worklist of sorted
//                                                  positions, over the cells of its cloud::Reach; survivors are appended
//                                                  to the other worklist (one ballot and one atomicAdd per wavefront);
//                                                  the host reads the 4-byte survivor count and sizes the next launch
// One uint32 of state per SORTED POSITION (a cell's states are contiguous, like its records): 0 = undecided, a point
// decided in round t stores 2t + kept.  In round t a reader takes a state s for decided only if (s >> 1) < t: a value
// stored in the current round reads as undecided whether or not the reader sees it, so the in-place plain stores give
// synchronous (Jacobi) rounds and every run decides the same points in the same round.  Lane i, over the neighbours
// j != i with d2 <= r2 and key(j) < key(i):
//     some such j decided-kept         -> i is DROPPED (and may stop looking)
//     else no such j undecided         -> i is KEPT
//     else                             -> i stays undecided
// By induction over the key both decisions are the sequential pass's: i is decided only from lower-key neighbours whose
// decisions are final, and those are all the sequential pass looks at.  The lowest-key undecided point has no undecided
// lower-key neighbour, so every round decides at least one point: the host stops with an error if one does not.
// Cells are visited whole and both tests are "exists" predicates: the order of the points inside a cell cannot matter.
// ---------------------------------------------------------------------------------------------------------------------
namespace thin {

using namespace cloud;  // (Rec, Grid, Reach, d2_of, kBlock)

enum { kKept = cloud::kStats, kSurvivors, kCounters };  // the device counters, behind cloud's (kTargets: the finite points)

// prio(i) of the hashed order: mix32(mix32(seed + 0x9E3779B9) ^ (i + 0x85EBCA6B)); salt is the inner mix32, from the host.
using pm::mix32;
__device__ __forceinline__ uint32_t prio_of(int32_t i, uint32_t salt, bool hashed) { return hashed ? mix32(salt ^ ((uint32_t)i + 0x85EBCA6BU)) : 0u; }

// One round.  n_in undecided points: the sorted positions list_in[0 .. n_in), or 0 .. n_in itself when list_in is null
// (round 1: every sorted point).
__global__ __launch_bounds__(kBlock) void round_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends, Grid g, float reach,
                                                       uint32_t salt, int hashed, uint32_t round, uint32_t *state,
                                                       const uint32_t *__restrict__ list_in, uint32_t n_in,
                                                       uint32_t *__restrict__ list_out, uint32_t *__restrict__ counters,
                                                       uint8_t *__restrict__ keep)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false, survives = false;
    uint32_t pos = 0;
    if (t < n_in) {
        pos = list_in ? list_in[t] : t;
        const Rec a = sorted[pos];
        const uint32_t pa = prio_of(a.j, salt, hashed);
        const Reach r(a, reach, g);
        bool dropped = false, blocked = false;
        for (int z = r.z0; z <= r.z1 && !dropped; ++z)
            for (int y = r.y0; y <= r.y1 && !dropped; ++y) {
                uint32_t p, end;
                for (r.row(ends, g, y, z, p, end); p < end; ++p) {
                    const Rec b = sorted[p];
                    if (!(d2_of(a, b) <= g.r2) || p == pos) continue;
                    const uint32_t pb = prio_of(b.j, salt, hashed);
                    if (!(pb < pa || (pb == pa && b.j < a.j))) continue;  // (only lower keys decide about a)
                    const uint32_t s = state[p];
                    if (s == 0u || (s >> 1) >= round) {
                        blocked = true;  // undecided, or decided in this very round
                    } else if (s & 1u) {
                        dropped = true;
                        break;
                    }
                }
            }
        kept = !dropped && !blocked;
        survives = !dropped && blocked;
        if (!survives) state[pos] = 2u * round + (kept ? 1u : 0u);
        if (kept) keep[a.j] = 1;  // (the mask comes in cleared)
    }
    // the counters and the worklist: one atomic each per wavefront (integer sums; the list's order is free)
    const uint64_t bk = __ballot(kept), bs = __ballot(survives);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) {
        if (bk) atomicAdd(&counters[kKept], (uint32_t)__popcll(bk));
        if (bs) base = atomicAdd(&counters[kSurvivors], (uint32_t)__popcll(bs));
    }
    base = __shfl(base, 0);
    if (survives) list_out[base + (uint32_t)__popcll(bs & ((1ull << lane) - 1ull))] = pos;
}

// The automatic G: a cell edge of about the radius -- never below it -- where 256 cells allow it, so that a lane's range
// of 2.02 radii covers three, at most four, cells per axis; 256 where the radius is below 1/256 of the longest extent
// (the cells then hold more than a neighbourhood; the result stays exact and the rounds get slower).  Reasoned, not
// measured.
inline int automatic_grid(float longest, float radius)
{
    const double q = (double)longest / (double)radius;
    return q >= (double)cloud::kMaxGrid ? cloud::kMaxGrid : q < 1.0 ? 1 : (int)q;
}

}  // namespace thin

// ---------------------------------------------------------------------------------------------------------------------
// Counting a point's neighbours within a radius, to drop the isolated ones (restated on the CPU by
// tests/neighbours_ref.py).  The contract, defined without any grid: for a finite point i,
//     exact(i) = #{ j != i : P_j finite and d2(i, j) <= r2 }      (cloud's d2, the thinning's inclusive radius; j != i by
//                                                                  index, so an exact copy is a neighbour)
//     count(i) = max_count > 0 ? min(exact(i), max_count) : exact(i);   keep(i) = count(i) >= min_neighbours
// and 0, 0 for a point that is not finite, which no other point counts either.  A count is the cardinality of a set: it
// does not depend on the order the records are visited in.
//
// Launches, all on one stream:
//   cloud::OwnGrid (box_*, count_kernel<false>, scan_kernel, scatter_kernel)   the thinning's set-up
//   support::count_kernel, once                    one lane per sorted position over the cells of its cloud::Reach, the
//                                                  thinning's range; the lane's counter goes to the caller's index
// The lanes of a wavefront are neighbours in the sorted order: they stand in the same or in adjacent cells, walk the same
// rows and load the same records, which the vector cache serves once per wavefront.  There is no LDS staging.
// ---------------------------------------------------------------------------------------------------------------------
namespace support {

using namespace cloud;  // (Rec, Grid, Reach, d2_of, kBlock)

enum { kKept = cloud::kStats, kSaturated, kCounters };  // the device counters, behind cloud's (kTargets: the finite points)

// *n_sorted: the number of sorted (finite) points, as the histogram left it on the device.  max_count = 0 counts without
// a limit: a counter never comes back to 0 (fewer than 2^31 points).  With a limit the lane leaves all three loops when
// it reaches it; min_neighbours <= max_count then, so stopping there cannot change `kept`.
__global__ __launch_bounds__(kBlock) void count_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends,
                                                       const uint32_t *__restrict__ n_sorted, Grid g, float reach, uint32_t max_count,
                                                       uint32_t min_neighbours, uint32_t *__restrict__ count_out,
                                                       uint8_t *__restrict__ keep_out, uint32_t *__restrict__ counters)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false, full = false;
    if (pos < *n_sorted) {
        const Rec a = sorted[pos];
        const Reach r(a, reach, g);
        uint32_t count = 0;
        for (int z = r.z0; z <= r.z1 && !full; ++z)
            for (int y = r.y0; y <= r.y1 && !full; ++y) {
                uint32_t p, end;
                for (r.row(ends, g, y, z, p, end); p < end; ++p) {
                    const Rec b = sorted[p];
                    if (d2_of(a, b) <= g.r2 && p != pos && ++count == max_count) {
                        full = true;
                        break;
                    }
                }
            }
        kept = count >= min_neighbours;
        if (count_out) count_out[a.j] = count;
        if (keep_out && kept) keep_out[a.j] = 1;  // (both outputs come in cleared)
    }
    // the counters: one atomic each per wavefront (integer sums: the totals do not depend on the order)
    const uint64_t bk = __ballot(kept), bf = __ballot(full);
    if ((threadIdx.x & 63) == 0) {
        if (bk) atomicAdd(&counters[kKept], (uint32_t)__popcll(bk));
        if (bf) atomicAdd(&counters[kSaturated], (uint32_t)__popcll(bf));
    }
}

}  // namespace support

// ---------------------------------------------------------------------------------------------------------------------
// The k nearest neighbours of every point inside its own cloud, and their mean distance: statistical outlier removal
// (restated on the CPU by tests/knn_ref.py).  The contract, defined without any grid: for a finite point i,
//     N(i)    = { j != i : P_j finite and d2(i, j) <= r2 }          (cloud's d2, the thinning's inclusive radius, j != i by index)
//     list(i) = the min(k, |N(i)|) smallest pairs (d2(i, j), j) of N(i), lexicographically, ascending;  m(i) = its length
//     mean(i) = m(i) == k ? (((sqrt(d2_0) + sqrt(d2_1)) + ...) + sqrt(d2_{k-1})) / (float)k : +inf
// float32, the sum in ascending slot order, every sqrt and the division correctly rounded; a point that is not finite has
// m = 0, empty slots (+inf, -1) and mean = +inf, and no other point lists it.  The k smallest of a set of distinct pairs,
// sorted, do not depend on the order the records are visited in.
//
// Launches, all on one stream:
//   cloud::OwnGrid (box_*, count_kernel<false>, scan_kernel, scatter_kernel)   the thinning's set-up
//   knn::clear_kernel                              (+inf, -1), 0 and +inf everywhere: what a point that is never sorted keeps
//   knn::topk_kernel<K>, once, K = the smallest of 8 / 16 / 32 that holds k: one lane per sorted position over the cells of
//                                                  its cloud::Reach (no neighbour is skipped: kReach); the results go to
//                                                  the caller's index
// The lane's list is K (d2, j) pairs in NAMED registers: every loop over the slots is fully unrolled, so no slot is indexed
// at run time and the compiler has no reason to put the list into scratch memory, which the unit does not use.  There is
// no LDS staging and the walk does not shrink to the current k-th distance: both are unmeasured ideas.
// ---------------------------------------------------------------------------------------------------------------------
namespace knn {

using namespace cloud;  // (Rec, Grid, Reach, d2_of, kBlock)

constexpr int kMaxK = 32;
enum { kComplete = cloud::kStats, kShort, kCounters };  // the device counters, behind cloud's (kTargets: the finite points)

// The unit spells no fused multiply-add (its assembly is tested for that), and the compiler's own correctly rounded sqrtf
// and `/` are built from them.  So both are written here: the hardware's approximation, then ONE step to the neighbouring
// float decided by exact arithmetic in double -- a float has 24 significant bits, the midpoint of two adjacent floats 25, and
// a product of two such numbers at most 50: it is exact in a double's 53, whatever the rounding mode.
__device__ __forceinline__ float up(float s) { return __uint_as_float(__float_as_uint(s) + 1u); }    // (s > 0, finite, not the largest)
__device__ __forceinline__ float down(float s) { return __uint_as_float(__float_as_uint(s) - 1u); }  // (s > 0)

// sqrt(x), correctly rounded, for x >= 0 or +inf.  v_sqrt_f32 is good to 1 ulp on normal inputs, so the correctly rounded
// root is s or one of its two neighbours: it is the float whose interval between the midpoints to its neighbours holds the
// real root, i.e. lo^2 < x < hi^2.  (A midpoint's square has an odd 50th bit: it is no float, and equality cannot occur.)
// An x below 2^-96 (subnormals among them, which the instruction does not take) is scaled by 2^64, its root by 2^-32, both
// exactly: the root of the smallest subnormal is 2^-74.5.
__device__ __forceinline__ float root(float x)
{
    if (!(x > 0.f) || x == INFINITY) return x;  // 0 and +inf are their own roots
    const bool tiny = x < 0x1p-96f;
    const float xs = tiny ? x * 0x1p64f : x;
    float s = __builtin_amdgcn_sqrtf(xs);
#pragma unroll
    for (int step = 0; step < 2; ++step) {  // (one step is what 1 ulp needs; the second costs a compare and asks nothing of it)
        const double hi = 0.5 * ((double)s + (double)up(s)), lo = 0.5 * ((double)s + (double)down(s));
        if ((double)xs > hi * hi) s = up(s);
        else if ((double)xs < lo * lo) s = down(s);
    }
    return tiny ? s * 0x1p-32f : s;
}

// a / k, correctly rounded, for a >= 0 or +inf and an integer 1 <= k <= 32 (inv_k = 1.0 / k in double, from the host).
// The double product is within 2^-52 of the quotient, so its rounding to float is the answer or its neighbour on the side
// of a midpoint; q is right iff lo * k <= a <= hi * k for the two midpoints, products of 25 and 6 bits, exact.  a is 0 or at
// least 2^-75 here (a sum of roots), so q is normal, and a normal quotient by an integer below 2^24 is never a midpoint.
__device__ __forceinline__ float quotient(float a, float k, double inv_k)
{
    if (!(a > 0.f) || a == INFINITY) return a;
    float q = (float)((double)a * inv_k);
    const double hi = 0.5 * ((double)q + (double)up(q)), lo = 0.5 * ((double)q + (double)down(q));
    if ((double)a > hi * (double)k) q = up(q);
    else if ((double)a < lo * (double)k) q = down(q);
    return q;
}

// what a point that is never sorted keeps: empty slots, m = 0, mean = +inf (each where the caller asked for the output)
__global__ __launch_bounds__(kBlock) void clear_kernel(uint32_t n, uint32_t slots, float *__restrict__ out_d2, int32_t *__restrict__ out_idx,
                                                       uint32_t *__restrict__ out_m, float *__restrict__ out_mean)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // (slots = n * k < 2^31)
    if (i < slots) {
        if (out_d2) out_d2[i] = INFINITY;
        if (out_idx) out_idx[i] = -1;
    }
    if (i < n) {
        if (out_m) out_m[i] = 0u;
        if (out_mean) out_mean[i] = INFINITY;
    }
}

// *n_sorted: the number of sorted (finite) points, as the histogram left it on the device.  The list is ascending in
// (d2, j), an empty slot is (+inf, -1): cloud::nearest_lists (pm_cloud.h), the walk and the compare-and-carry insertion.
template <int K>
__global__ __launch_bounds__(kBlock) void topk_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends,
                                                      const uint32_t *__restrict__ n_sorted, Grid g, float reach, int k, double inv_k,
                                                      float *__restrict__ out_d2, int32_t *__restrict__ out_idx,
                                                      uint32_t *__restrict__ out_m, float *__restrict__ out_mean,
                                                      uint32_t *__restrict__ counters)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    bool complete = false, is_short = false;
    if (pos < *n_sorted) {
        const Rec a = sorted[pos];
        float d[K];
        uint32_t j[K];
        nearest_lists<K>(sorted, ends, g, reach, a, pos, d, j);
        // the outputs: slots k .. K - 1 are never written out; m counts the filled ones of the first k
        uint32_t m = 0;
        float sum = 0.f;
        const size_t base = (size_t)a.j * (size_t)k;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < k) {
                m += j[s] != ~0u;
                sum = sum + root(d[s]);
                if (out_d2) out_d2[base + s] = d[s];
                if (out_idx) out_idx[base + s] = (int32_t)j[s];
            }
        complete = m == (uint32_t)k;
        is_short = !complete;
        if (out_m) out_m[a.j] = m;
        if (out_mean) out_mean[a.j] = complete ? quotient(sum, (float)k, inv_k) : INFINITY;
    }
    // the counters: one atomic each per wavefront (integer sums: the totals do not depend on the order)
    const uint64_t bc = __ballot(complete), bs = __ballot(is_short);
    if ((threadIdx.x & 63) == 0) {
        if (bc) atomicAdd(&counters[kComplete], (uint32_t)__popcll(bc));
        if (bs) atomicAdd(&counters[kShort], (uint32_t)__popcll(bs));
    }
}

}  // namespace knn

namespace {

thread_local int64_t last_stats[6] = {0, 0, 0, 0, 0, 0};  // gipuma_hip_cloud_last_stats

int run(const gipuma_hip_cloud_desc *d, float *d2_dev, int32_t *idx_dev, int64_t counts[2], float *device_ms)
{
    const uint32_t na = (uint32_t)d->n_queries, nb = (uint32_t)d->n_targets;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 4)) return rc;
    hipStream_t st = sc.st;
    const dim3 block(cloud::kBlock);
    float ms_box = 0.f, ms_rest = 0.f;
    int64_t found = 0;

    // the box of the finite targets
    cloud::Box box;
    if (na && nb) {
        if (const int rc = box.alloc(sc, nb)) return rc;
        HIP_OK(hipEventRecord(sc.e[0], st));
        if (const int rc = box.enqueue(st, d->targets, nb)) return rc;
        HIP_OK(hipEventRecord(sc.e[1], st));
        if (const int rc = box.read(st)) return rc;
        HIP_OK(hipEventElapsedTime(&ms_box, sc.e[0], sc.e[1]));
    }

    if (na && !box.any_finite()) {
        HIP_OK(hipEventRecord(sc.e[2], st));
        hipLaunchKernelGGL(cloud::none_kernel, cloud::blocks_for(na), block, 0, st, na, d2_dev, idx_dev);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(sc.e[3], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms_rest, sc.e[2], sc.e[3]));
    } else if (na) {
        // the grid; the derivation of kShellSlack does not hold for an infinite r2
        const float r2 = d->max_dist * d->max_dist;
        const cloud::Layout l = cloud::lay_out(box, d->grid ? d->grid : cloud::automatic_grid(d->n_targets), r2, std::isfinite(r2));
        for (int k = 0; k < 4; ++k) last_stats[k] = l.report[k];

        uint32_t *cells_b, *cells_a, *stats_dev;
        int32_t *cellid_b, *cellid_a;
        cloud::Rec *sorted_b, *sorted_a;
        if (sc.alloc(cells_b, l.ncells) || sc.alloc(cells_a, l.ncells) || sc.alloc(stats_dev, cloud::kStats) || sc.alloc(cellid_b, nb) ||
            sc.alloc(cellid_a, na) || sc.alloc(sorted_b, nb) || sc.alloc(sorted_a, na))
            return GIPUMA_HIP_ERR_DEVICE;

        HIP_OK(hipEventRecord(sc.e[2], st));
        HIP_OK(hipMemsetAsync(cells_b, 0, sizeof(uint32_t) * l.ncells, st));
        HIP_OK(hipMemsetAsync(cells_a, 0, sizeof(uint32_t) * l.ncells, st));
        HIP_OK(hipMemsetAsync(stats_dev, 0, sizeof(uint32_t) * cloud::kStats, st));
        if (const int rc = cloud::sort_by_cell<false>(st, d->targets, nb, l, cellid_b, cells_b, sorted_b, nullptr, nullptr, stats_dev, nullptr))
            return rc;
        if (const int rc = cloud::sort_by_cell<true>(st, d->queries, na, l, cellid_a, cells_a, sorted_a, d2_dev, idx_dev, stats_dev,
                                                     stats_dev + cloud::kSearched))
            return rc;
        hipLaunchKernelGGL(cloud::search_kernel, cloud::blocks_for(na), block, 0, st, sorted_a, stats_dev + cloud::kSearched, sorted_b,
                           cells_b, l.g, d2_dev, idx_dev, stats_dev);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(sc.e[3], st));
        uint32_t stats[cloud::kStats];
        HIP_OK(hipMemcpyAsync(stats, stats_dev, sizeof stats, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms_rest, sc.e[2], sc.e[3]));
        found = stats[cloud::kFound];
        last_stats[4] = stats[cloud::kEarly];
        last_stats[5] = stats[cloud::kSearched];
    }
    if (counts) {
        counts[0] = found;
        counts[1] = (int64_t)na - found;
    }
    if (device_ms) *device_ms = ms_box + ms_rest;
    return 0;
}

int run_thin(const gipuma_hip_thin_desc *d, uint8_t *keep_dev, int64_t info[8], float *device_ms)
{
    const uint32_t n = (uint32_t)d->n_points;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    cloud::OwnGrid og;
    uint32_t finite = 0, kept = 0, rounds = 0;
    float ms = 0.f;

    if (n) {
        // the mask comes out of the rounds with the kept points set
        if (const int rc = og.box.alloc(sc, n)) return rc;
        HIP_OK(hipEventRecord(sc.e[0], st));
        HIP_OK(hipMemsetAsync(keep_dev, 0, n, st));
        if (const int rc = og.lay(sc, d->points, n, d->radius, d->grid, thin::kCounters)) return rc;
        if (og.any) {  // (else: nothing is kept)
            uint32_t *state, *list[2];
            if (sc.alloc(state, n) || sc.alloc(list[0], n) || sc.alloc(list[1], n)) return GIPUMA_HIP_ERR_DEVICE;
            HIP_OK(hipMemsetAsync(state, 0, sizeof(uint32_t) * n, st));
            if (const int rc = og.sort(st, d->points, n)) return rc;
            HIP_OK(hipMemcpyAsync(&finite, og.counters + cloud::kTargets, sizeof finite, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            // the rounds: the host reads the survivor count after each and sizes the next launch with it
            const float reach = cloud::kReach * d->radius;
            const uint32_t salt = pm::mix32(d->seed + 0x9E3779B9U);
            uint32_t undecided = finite;
            while (undecided) {
                ++rounds;
                uint32_t survivors = 0;
                HIP_OK(hipMemsetAsync(og.counters + thin::kSurvivors, 0, sizeof(uint32_t), st));
                hipLaunchKernelGGL(thin::round_kernel, cloud::blocks_for(undecided), dim3(cloud::kBlock), 0, st, og.sorted, og.cells,
                                   og.l.g, reach, salt, d->order == 0 ? 1 : 0, rounds, state,
                                   rounds == 1 ? (const uint32_t *)nullptr : list[rounds & 1], undecided, list[(rounds + 1) & 1],
                                   og.counters, keep_dev);
                HIP_OK(hipGetLastError());
                HIP_OK(hipMemcpyAsync(&survivors, og.counters + thin::kSurvivors, sizeof survivors, hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
                if (survivors >= undecided)  // (the lowest-key undecided point is always decided: this bounds the loop)
                    return fail(GIPUMA_HIP_ERR_DEVICE, "thin: round %u decided none of its %u undecided points", rounds, undecided);
                undecided = survivors;
            }
            HIP_OK(hipMemcpyAsync(&kept, og.counters + thin::kKept, sizeof kept, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipEventRecord(sc.e[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms, sc.e[0], sc.e[1]));
    }
    og.report(info, n, finite, kept, rounds);
    if (device_ms) *device_ms = ms;
    return 0;
}

int run_neighbours(const gipuma_hip_neighbours_desc *d, uint32_t *count_dev, uint8_t *keep_dev, int64_t info[8], float *device_ms)
{
    const uint32_t n = (uint32_t)d->n_points;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    cloud::OwnGrid og;
    uint32_t counters[support::kCounters] = {};
    float ms = 0.f;

    if (n) {
        // both outputs come out of the kernel with the finite points' entries written
        if (const int rc = og.box.alloc(sc, n)) return rc;
        HIP_OK(hipEventRecord(sc.e[0], st));
        if (count_dev) HIP_OK(hipMemsetAsync(count_dev, 0, sizeof(uint32_t) * n, st));
        if (keep_dev) HIP_OK(hipMemsetAsync(keep_dev, 0, n, st));
        if (const int rc = og.lay(sc, d->points, n, d->radius, d->grid, support::kCounters)) return rc;
        if (og.any) {  // (else: nothing is counted, nothing kept)
            if (const int rc = og.sort(st, d->points, n)) return rc;
            hipLaunchKernelGGL(support::count_kernel, cloud::blocks_for(n), dim3(cloud::kBlock), 0, st, og.sorted, og.cells,
                               og.counters + cloud::kTargets, og.l.g, cloud::kReach * d->radius, (uint32_t)d->max_count,
                               (uint32_t)d->min_neighbours, count_dev, keep_dev, og.counters);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(counters, og.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipEventRecord(sc.e[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms, sc.e[0], sc.e[1]));
    }
    og.report(info, n, counters[cloud::kTargets], counters[support::kKept], counters[support::kSaturated]);
    if (device_ms) *device_ms = ms;
    return 0;
}

int run_knn(const gipuma_hip_knn_desc *d, float *d2_dev, int32_t *idx_dev, uint32_t *count_dev, float *mean_dev, int64_t info[8],
            float *device_ms)
{
    const uint32_t n = (uint32_t)d->n_points, k = (uint32_t)d->k;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    cloud::OwnGrid og;
    uint32_t counters[knn::kCounters] = {};
    float ms = 0.f;

    if (n) {
        // every output comes out of the kernel with the finite points' entries written over the clearing
        if (const int rc = og.box.alloc(sc, n)) return rc;
        HIP_OK(hipEventRecord(sc.e[0], st));
        hipLaunchKernelGGL(knn::clear_kernel, cloud::blocks_for(d2_dev || idx_dev ? n * k : n), dim3(cloud::kBlock), 0, st, n, n * k,
                           d2_dev, idx_dev, count_dev, mean_dev);
        HIP_OK(hipGetLastError());
        if (const int rc = og.lay(sc, d->points, n, d->radius, d->grid, knn::kCounters)) return rc;
        if (og.any) {  // (else: no point has a list)
            if (const int rc = og.sort(st, d->points, n)) return rc;
            const auto kernel = k <= 8 ? knn::topk_kernel<8> : k <= 16 ? knn::topk_kernel<16> : knn::topk_kernel<knn::kMaxK>;
            hipLaunchKernelGGL(kernel, cloud::blocks_for(n), dim3(cloud::kBlock), 0, st, og.sorted, og.cells, og.counters + cloud::kTargets,
                               og.l.g, cloud::kReach * d->radius, (int)k, 1.0 / (double)k, d2_dev, idx_dev, count_dev, mean_dev,
                               og.counters);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(counters, og.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipEventRecord(sc.e[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms, sc.e[0], sc.e[1]));
    }
    og.report(info, n, counters[cloud::kTargets], counters[knn::kComplete], 0);
    if (device_ms) *device_ms = ms;
    return 0;
}

}  // namespace

extern "C" {

int gipuma_hip_cloud_nearest(const gipuma_hip_cloud_desc *d, float *d2_dev, int32_t *idx_dev, int64_t counts[2], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    if (const int rc = cloud::check_args("cloud", d->abi_version, d->n_queries, d->n_targets,
                                  (d->n_queries && (!d->queries || !d2_dev || !idx_dev)) || (d->n_targets && !d->targets), "max_dist",
                                  d->max_dist, nullptr, d->grid, d->device_id))
        return rc;
    memset(last_stats, 0, sizeof last_stats);
    return run(d, d2_dev, idx_dev, counts, device_ms);
}

int gipuma_hip_cloud_last_stats(int64_t stats[6])
{
    if (!stats) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    memcpy(stats, last_stats, sizeof last_stats);
    return 0;
}

int gipuma_hip_cloud_thin(const gipuma_hip_thin_desc *d, uint8_t *keep_dev, int64_t info[8], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    const char *own = d->order != 0 && d->order != 1 ? "order must be 0 (hashed) or 1 (index)" : nullptr;
    if (const int rc = cloud::check_args("thin", d->abi_version, d->n_points, 0, d->n_points && (!d->points || !keep_dev), "radius", d->radius,
                                  own, d->grid, d->device_id))
        return rc;
    return run_thin(d, keep_dev, info, device_ms);
}

int gipuma_hip_cloud_neighbours(const gipuma_hip_neighbours_desc *d, uint32_t *count_dev, uint8_t *keep_dev, int64_t info[8],
                                float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    const char *own = d->min_neighbours < 0 ? "min_neighbours must be >= 0"
                      : d->max_count < 0    ? "max_count must be >= 0 (0: exact counts)"
                      : d->max_count > 0 && d->min_neighbours > d->max_count ? "min_neighbours must not exceed a max_count > 0" : nullptr;
    if (const int rc = cloud::check_args("neighbours", d->abi_version, d->n_points, 0, d->n_points && (!d->points || (!count_dev && !keep_dev)),
                                  "radius", d->radius, own, d->grid, d->device_id))
        return rc;
    return run_neighbours(d, count_dev, keep_dev, info, device_ms);
}

int gipuma_hip_cloud_knn(const gipuma_hip_knn_desc *d, float *d2_dev, int32_t *idx_dev, uint32_t *count_dev, float *mean_dev,
                         int64_t info[8], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    const bool bad_k = d->k < 1 || d->k > knn::kMaxK;
    const bool too_many = !bad_k && (d2_dev || idx_dev) && d->n_points >= ((1ll << 31) + d->k - 1) / d->k;  // n * k >= 2^31
    const char *own = bad_k ? "k must be 1..32" : too_many ? "the lists may hold at most 2^31 - 1 slots (n_points * k)" : nullptr;
    if (const int rc = cloud::check_args("knn", d->abi_version, d->n_points, 0,
                                  d->n_points && (!d->points || (!d2_dev && !idx_dev && !count_dev && !mean_dev)), "radius", d->radius,
                                  own, d->grid, d->device_id, bad_k ? GIPUMA_HIP_ERR_ARG : GIPUMA_HIP_ERR_UNSUPPORTED))
        return rc;
    return run_knn(d, d2_dev, idx_dev, count_dev, mean_dev, info, device_ms);
}

}  // extern "C"
