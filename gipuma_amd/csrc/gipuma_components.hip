// gipuma_components.hip -- the connected components of a cloud's radius graph on gfx950: dropping the small clumps that
// neither the neighbour count nor the statistical filter can see, and segmenting a fused scan into its objects (DESIGN.md
// 18, gipuma_hip_cloud_components, restated on the CPU by tests/components_ref.py).
//
// The contract, defined without any grid (include/gipuma_hip.h): over the finite points, i ~ j iff i != j by index and
// d2(i, j) <= r2 (cloud's d2 of pm_cloud.h, float32 without contraction, bitwise symmetric; the thinning's inclusive radius);
//     label(i) = the smallest index of i's connected component,  size(i) = its cardinality,  keep(i) = size(i) >= min_size
// and (-1, 0, 0) for a point that is not finite, which no component contains.  A minimum and a cardinality of a set do not
// depend on the order its members are visited in, on the grid or on how concurrent unions interleave: the outputs equal a
// sequential union-find over a brute-force edge list in every byte, run after run.
//
// Launches, all on one stream, no host-driven rounds and no host read but OwnGrid's box:
//   cloud::OwnGrid (box_*, count_kernel<false>, scan_kernel, scatter_kernel; gipuma_cloud.hip)   the thinning's set-up
//   comp::init_kernel      parent[pos] = pos, minidx[pos] = INT32_MAX, size[pos] = 0; the caller's outputs (-1, 0, 0), which a
//                          point that is not finite keeps: it is never sorted
//   comp::hook_kernel      one lane per sorted position over the cells of its cloud::Reach (no neighbour is skipped: kReach);
//                          every record p < pos within the radius is united with pos in a lock-free union-find over the
//                          SORTED POSITIONS, so that neighbours' entries lie close together
//   comp::flatten_kernel   a new launch, so every union is visible: each position follows parent[] to its root r, read-only,
//                          and gives minidx[r] its caller's index and size[r] one more
//   comp::write_kernel     label, size and mask to the caller's index; kept points and roots counted
// The scratch on top of OwnGrid's is four 4-byte arrays per point.  No LDS staging, no float atomics, no scratch memory.
#include <hip/hip_runtime.h>

#include <climits>

#include "pm_cloud.h"

using pm_host::fail;

namespace comp {

using namespace cloud;  // (Rec, Grid, Reach, d2_of, kBlock)

enum { kKept = cloud::kStats, kComponents, kCounters };  // the device counters, behind cloud's (kTargets: the finite points)

__global__ __launch_bounds__(kBlock) void init_kernel(uint32_t n, uint32_t *__restrict__ parent, int32_t *__restrict__ minidx,
                                                      uint32_t *__restrict__ size, int32_t *__restrict__ label_out,
                                                      uint32_t *__restrict__ size_out, uint8_t *__restrict__ keep_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    minidx[i] = INT_MAX;
    size[i] = 0u;
    if (label_out) label_out[i] = -1;
    if (size_out) size_out[i] = 0u;
    if (keep_out) keep_out[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The union-find of hook_kernel.  parent[] is a forest over the sorted positions; a ROOT is a position x with parent[x] == x,
// the TREE of x is the set of positions that reach the same root as x.  Inside the kernel parent[] is only ever changed by
// two atomic read-modify-writes, never by a plain store:
//     (H) atomicCAS(&parent[hi], hi, lo) with lo < hi   -- it changes the entry only if hi is a root at that instant
//     (C) atomicMin(&parent[x], gp) with gp < x         -- gp was read as the parent of a position read as the parent of x
// Invariants, at every instant and whatever the atomics' interleaving (each is indivisible at its address):
//   (I1) parent[x] <= x, and an entry only ever decreases.  init gives equality; (H) and (C) store values below x and (C)
//        keeps the smaller of old and new.  Hence a position that has stopped being a root never becomes one again, the
//        forest has no cycle, and every walk x, parent[x], parent[parent[x]], ... strictly decreases until it stands.
//   (I2) two positions that are in one tree at some instant are in one tree at every later instant.  (H) hangs a whole tree
//        below a position of another: trees only merge.  (C): p was read from parent[x], gp from parent[p]; a value read
//        from parent[y] was in y's tree when it was stored (by induction over the stores) and by (I2) still is, so gp is in
//        x's tree when (C) acts, and below x: x's subtree moves to another position of its own tree, no root changes.
//   (I3) a tree lies inside one component of the radius graph.  Only (H) merges trees, and unite(u, v) is only called for
//        an edge's two ends or positions read on the walks from them: both trees hold an end of one edge.
// NEVER INVENTED: (I3).  NEVER LOST: unite() for the edge (pos, p) returns only after a successful (H) between a position
// of pos's tree and one of p's, which merges them, or after its two walks have met in one position, which by (I2) is in
// both trees: they are one.  By (I2) they stay one.  Every edge is seen from the end with the larger position, so when the
// kernel has finished the trees ARE the components, and by (I1) each tree has exactly one root: the roots are one per component.
// STALE LOADS: a find reads parent[] with relaxed agent-scope atomic loads, and the value may be an older one.  Every value
// an entry ever held satisfies (I1) and (I2), so an old value is still a position of the same tree at or below x -- a valid
// place to go on from; taking a former root for a root is caught by (H), which tests the entry itself.  Nothing rests on a
// load being fresh, no lane waits for another lane's store, there is no fence and no flag.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t entry(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a position of x's tree that this lane read as its own parent: a root, unless another lane has hooked it since
__device__ __forceinline__ uint32_t find(uint32_t *parent, uint32_t x)
{
    uint32_t p = entry(&parent[x]);
    // Terminates: p <= x by (I1), whichever value of the entry the load saw; the loop goes on only while p < x and goes on
    // from p, so x strictly decreases and is bounded by 0.  It waits for no store.
    while (p != x) {
        const uint32_t gp = entry(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);  // (C): halve the path; x's entry can only fall to a position of its tree
        x = p;
        p = gp;
    }
    return x;
}

// Unites the trees of u and v; returns a position of the united tree to go on from (the lane's next find starts there).
__device__ __forceinline__ uint32_t unite(uint32_t *parent, uint32_t u, uint32_t v)
{
    u = find(parent, u);
    v = find(parent, v);
    // Terminates: a failed CAS means another lane's atomic has already lowered parent[hi], and returns that value, old <
    // hi by (I1); the lane goes on from it -- from what the atomic returned, not from a new load -- and find only lowers
    // it further.  So hi is replaced by a smaller position and lo stays: u + v strictly decreases with every failed CAS and
    // is bounded by 0.  A successful CAS or u == v ends the loop.  No iteration waits for another lane.
    while (u != v) {
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const uint32_t old = atomicCAS(&parent[hi], hi, lo);  // (H)
        if (old == hi) return lo;
        u = find(parent, old);
        v = lo;
    }
    return u;
}

// *n_sorted: the number of sorted (finite) points, as the histogram left it on the device.  Each edge is seen from both
// ends, so the end with the larger position unites: a row is walked up to pos only.  `mine` is a position of pos's tree,
// the last union's result: the next find starts near the root.
__global__ __launch_bounds__(kBlock) void hook_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ ends,
                                                      const uint32_t *__restrict__ n_sorted, Grid g, float reach, uint32_t *parent)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    if (pos >= *n_sorted) return;
    const Rec a = sorted[pos];
    const Reach r(a, reach, g);
    uint32_t mine = pos;
    for (int z = r.z0; z <= r.z1; ++z)
        for (int y = r.y0; y <= r.y1; ++y) {
            uint32_t p, end;
            r.row(ends, g, y, z, p, end);
            end = end < pos ? end : pos;
            for (; p < end; ++p) {  // (a row is a finite range of positions: p < end <= pos)
                const Rec b = sorted[p];
                if (d2_of(a, b) <= g.r2) mine = unite(parent, mine, p);
            }
        }
}

// A new launch: every union of hook_kernel is visible, parent[] is read-only here and plain loads do.  The walk strictly
// decreases (I1).  root[pos] = r for write_kernel.  minidx[r] = min of the tree's caller indices, size[r] = its cardinality:
// integer min and sum, which do not depend on the order.  The lanes of a wavefront that share lane 0's root -- all of them
// where a component is larger than a wavefront's stretch of the sorted order -- send one atomic each of the two kinds.
__global__ __launch_bounds__(kBlock) void flatten_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ n_sorted,
                                                         const uint32_t *__restrict__ parent, uint32_t *__restrict__ root,
                                                         int32_t *__restrict__ minidx, uint32_t *__restrict__ size)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    const bool in = pos < *n_sorted;  // (the lanes in range are a wavefront's first ones: lane 0 is in range if any is)
    uint32_t r = pos;
    int32_t j = INT_MAX;
    if (in) {
        for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;  // (p < r: strictly decreasing)
        root[pos] = r;
        j = sorted[pos].j;
    }
    const uint32_t lead = (uint32_t)__shfl((int)r, 0);
    const bool with_lead = in && r == lead;
    const uint64_t bl = __ballot(with_lead);
    int32_t m = with_lead ? j : INT_MAX;
    for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && bl) {
        atomicMin(&minidx[lead], m);
        atomicAdd(&size[lead], (uint32_t)__popcll(bl));
    }
    if (in && !with_lead) {
        atomicMin(&minidx[r], j);
        atomicAdd(&size[r], 1u);
    }
}

// The outputs, to the caller's index, each where its pointer is given (they come in cleared); the kept points and the roots
// -- the components -- are counted with one ballot and one atomic per wavefront (integer sums).
__global__ __launch_bounds__(kBlock) void write_kernel(const Rec *__restrict__ sorted, const uint32_t *__restrict__ n_sorted,
                                                       const uint32_t *__restrict__ root, const int32_t *__restrict__ minidx,
                                                       const uint32_t *__restrict__ size, uint32_t min_size,
                                                       int32_t *__restrict__ label_out, uint32_t *__restrict__ size_out,
                                                       uint8_t *__restrict__ keep_out, uint32_t *__restrict__ counters)
{
    const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false, is_root = false;
    if (pos < *n_sorted) {
        const int32_t j = sorted[pos].j;
        const uint32_t r = root[pos], s = size[r];
        kept = s >= min_size;
        is_root = r == pos;
        if (label_out) label_out[j] = minidx[r];
        if (size_out) size_out[j] = s;
        if (keep_out && kept) keep_out[j] = 1;
    }
    const uint64_t bk = __ballot(kept), br = __ballot(is_root);
    if ((threadIdx.x & 63) == 0) {
        if (bk) atomicAdd(&counters[kKept], (uint32_t)__popcll(bk));
        if (br) atomicAdd(&counters[kComponents], (uint32_t)__popcll(br));
    }
}

}  // namespace comp

namespace {

int run_components(const gipuma_hip_components_desc *d, int32_t *label_dev, uint32_t *size_dev, uint8_t *keep_dev, int64_t info[8],
                   float *device_ms)
{
    const uint32_t n = (uint32_t)d->n_points;
    HIP_OK(hipSetDevice(d->device_id));
    pm_host::CallScope sc;
    if (const int rc = sc.open(d->stream, 2)) return rc;
    hipStream_t st = sc.st;
    cloud::OwnGrid og;
    uint32_t counters[comp::kCounters] = {};
    float ms = 0.f;

    if (n) {
        const dim3 blocks = cloud::blocks_for(n), block(cloud::kBlock);
        uint32_t *parent, *size, *root;
        int32_t *minidx;
        if (const int rc = og.box.alloc(sc, n)) return rc;
        if (sc.alloc(parent, n) || sc.alloc(minidx, n) || sc.alloc(size, n) || sc.alloc(root, n)) return GIPUMA_HIP_ERR_DEVICE;
        HIP_OK(hipEventRecord(sc.e[0], st));
        hipLaunchKernelGGL(comp::init_kernel, blocks, block, 0, st, n, parent, minidx, size, label_dev, size_dev, keep_dev);
        HIP_OK(hipGetLastError());
        if (const int rc = og.lay(sc, d->points, n, d->radius, d->grid, comp::kCounters)) return rc;
        if (og.any) {  // (else: no component)
            if (const int rc = og.sort(st, d->points, n)) return rc;
            const uint32_t *n_sorted = og.counters + cloud::kTargets;
            hipLaunchKernelGGL(comp::hook_kernel, blocks, block, 0, st, og.sorted, og.cells, n_sorted, og.l.g, cloud::kReach * d->radius,
                               parent);
            HIP_OK(hipGetLastError());
            hipLaunchKernelGGL(comp::flatten_kernel, blocks, block, 0, st, og.sorted, n_sorted, parent, root, minidx, size);
            HIP_OK(hipGetLastError());
            hipLaunchKernelGGL(comp::write_kernel, blocks, block, 0, st, og.sorted, n_sorted, root, minidx, size, (uint32_t)d->min_size,
                               label_dev, size_dev, keep_dev, og.counters);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(counters, og.counters, sizeof counters, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipEventRecord(sc.e[1], st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipEventElapsedTime(&ms, sc.e[0], sc.e[1]));
    }
    og.report(info, n, counters[cloud::kTargets], counters[comp::kKept], counters[comp::kComponents]);
    if (device_ms) *device_ms = ms;
    return 0;
}

}  // namespace

extern "C" int gipuma_hip_cloud_components(const gipuma_hip_components_desc *d, int32_t *label_dev, uint32_t *size_dev, uint8_t *keep_dev,
                                           int64_t info[8], float *device_ms)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    const char *own = d->min_size < 0 ? "min_size must be >= 0" : nullptr;
    if (const int rc = cloud::check_args("components", d->abi_version, d->n_points, 0,
                                         d->n_points && (!d->points || (!label_dev && !size_dev && !keep_dev)), "radius", d->radius, own,
                                         d->grid, d->device_id))
        return rc;
    return run_components(d, label_dev, size_dev, keep_dev, info, device_ms);
}
