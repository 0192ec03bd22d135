// pm_host_instrument.h -- what gipuma_hip.hip measures about a solve, kept beside the solve: the half-sweep and group timers
// (gipuma_hip_launch_times / gipuma_hip_group_times), the counter report of GIPUMA_HIP_COUNTS=1, and the hooks of the two
// instrumented builds (-DPM_WG_TICKS, -DPM_CHECKED).  Host only; knows the device code by pm::kDbgSlots alone.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pm_host.h"

namespace {

// One event per half-sweep launch of a timed gipuma_hip_solve, and a pair around every pm::group_kernel launch in front of
// one.  begin -> per half-sweep { enter, [group_mark 0, group_mark 1], mark } -> collect.
struct SolveTimers {
    std::vector<hipEvent_t> events;    // of a solve of n half-sweeps: [0] before the first, [h + 1] after half-sweep h, then
                                       // [n + 1 + 2 * h], [n + 2 + 2 * h] around the pm::group_kernel launch of half-sweep h
    std::vector<char> gev_used;        // per half-sweep: it had such a launch
    std::vector<float> half_sweep_ms;  // of the last timed gipuma_hip_solve (gipuma_hip_launch_times)
    std::vector<float> group_ms;       // of the last timed solve (gipuma_hip_group_times)
    bool timed = false;                // the solve that is running, or ran last, is a timed one
    int half_sweeps = 0;               // ... of so many half-sweeps
    int timed_half_sweep = -1;         // >= 0 while a timed solve is launching that half-sweep
    int n_pushed = 0;                  // leading half-sweeps of the last timed solve that read pushed costs
    int n_push_consumed = 0;           // ... counted while a solve runs (launch_sweep)

    hipEvent_t group_event(int h, int after) const { return events[half_sweeps + 1 + 2 * h + after]; }
    int begin(bool timed_solve, int n_half_sweeps, hipStream_t stream)
    {
        timed = timed_solve;
        half_sweeps = n_half_sweeps;
        n_push_consumed = 0;
        if (!timed) return 0;
        while (events.size() < (size_t)3 * half_sweeps + 1) {
            hipEvent_t e;
            HIP_OK(hipEventCreate(&e));
            events.push_back(e);
        }
        gev_used.assign(half_sweeps, 0);
        HIP_OK(hipEventRecord(events[0], stream));
        return 0;
    }
    void enter(int half_sweep) { timed_half_sweep = timed ? half_sweep : -1; }
    int mark(int half_sweep, hipStream_t stream, int rc)  // half-sweep `half_sweep` is enqueued, or failed with `rc`
    {
        timed_half_sweep = -1;
        if (!rc && timed) HIP_OK(hipEventRecord(events[half_sweep + 1], stream));
        return rc;
    }
    int group_mark(int after, hipStream_t stream)  // in front of (0) / behind (1) the pm::group_kernel launch of a half-sweep
    {
        const int h = timed_half_sweep;
        if (h < 0) return 0;
        HIP_OK(hipEventRecord(group_event(h, after), stream));
        if (after) gev_used[h] = 1;
        return 0;
    }
    // after `done` (recorded behind the solve's last launch): the durations, and -- to stderr, GIPUMA_HIP_LAUNCH_TIMES=1 --
    int collect(hipEvent_t done, bool print)
    {
        if (!timed) return 0;
        HIP_OK(hipEventSynchronize(done));
        half_sweep_ms.assign(half_sweeps, 0.0f);
        for (int i = 0; i < half_sweeps; i++) HIP_OK(hipEventElapsedTime(&half_sweep_ms[i], events[i], events[i + 1]));
        group_ms.assign(half_sweeps, 0.0f);
        for (int i = 0; i < half_sweeps; i++)
            if (gev_used[i]) HIP_OK(hipEventElapsedTime(&group_ms[i], group_event(i, 0), group_event(i, 1)));
        n_pushed = n_push_consumed;
        if (print) {
            fprintf(stderr, "gipuma_hip launch_ms:");
            for (float ms : half_sweep_ms) fprintf(stderr, " %.3f", ms);
            fprintf(stderr, "\n");
        }
        return 0;
    }
    void destroy() { for (hipEvent_t e : events) (void)hipEventDestroy(e); }
};

// copies `n` values out, as far as `capacity` reaches (gipuma_hip_launch_times, gipuma_hip_group_times)
inline int copy_times(const std::vector<float> &ms, float *out, int capacity, int *n_out)
{
    const int n = (int)ms.size();
    if (out)
        for (int i = 0; i < n && i < capacity; i++) out[i] = ms[i];
    if (n_out) *n_out = n;
    return 0;
}

// GIPUMA_HIP_COUNTS=1: what the kernels of a solve counted in Problem::dbg, to stderr, and the counters zeroed for the next
// solve.  Per half-sweep: events per pixel of the colour.
inline int report_counts(unsigned long long *dbg_dev, int rows, int cols, int iterations)
{
    std::vector<unsigned long long> h(64 * pm::kDbgSlots);
    HIP_OK(hipMemcpy(h.data(), dbg_dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_OK(hipMemset(dbg_dev, 0, h.size() * sizeof(unsigned long long)));
    const double px = 0.5 * (double)rows * (double)cols;
    static const char *names[] = {"tasks/px", "-", "items/px", "open items/px", "redone cands/px", "cands/px"};
    if (h[62 * pm::kDbgSlots + 1]) {  // the plane-keyed kernels' phase clocks: 100 MHz ticks of each workgroup's first wavefront, summed
        fprintf(stderr, "gipuma_hip plane-keyed phase ticks (state, task list, grouping, batches, wait for the last batch, tile, "
                        "replay + refinement):");
        for (int k = 0; k < 7; k++) fprintf(stderr, " %llu", h[62 * pm::kDbgSlots + k]);
        fprintf(stderr, "\n");
    }
    if (h[61 * pm::kDbgSlots + 0]) {  // pm::group_kernel's batches, summed over the solve's launches
        const double nb = (double)h[61 * pm::kDbgSlots + 0], nt = (double)h[61 * pm::kDbgSlots + 7];
        fprintf(stderr, "gipuma_hip group_kernel batches: %.1f per tile; per batch %.1f strips, %.1f tasks, %.2f groups, "
                        "%.2f rows; per tile %.1f groups, %.1f tasks\n", nb / nt, h[61 * pm::kDbgSlots + 1] / nb,
                h[61 * pm::kDbgSlots + 2] / nb, h[61 * pm::kDbgSlots + 3] / nb, h[61 * pm::kDbgSlots + 4] / nb,
                h[61 * pm::kDbgSlots + 5] / nt, h[61 * pm::kDbgSlots + 6] / nt);
    }
    for (int k = 0; k < 6; k++) {
        fprintf(stderr, "gipuma_hip counts %s:", names[k]);
        for (int ph = 1; ph <= 2 * iterations && ph < 64; ph++)
            fprintf(stderr, " %.3f", (double)h[(size_t)ph * pm::kDbgSlots + k] / px);
        fprintf(stderr, "\n");
    }
    return 0;
}

// (experiment build, -DPM_WG_TICKS) GIPUMA_HIP_WG_TICKS=<file>: the clocks of every workgroup of a fused launch
// (Problem::wg_ticks), appended to the file.  Without the macro, or without the switch, both hooks do nothing.
#ifndef PM_WG_TICKS
struct WgTicks {
    int clear(int) { return 0; }
    int append(hipStream_t, int, int, uint32_t, unsigned) { return 0; }
};
#else
struct WgTicks {
    unsigned long long *dev = nullptr;  // Problem::wg_ticks, 4 words per sweep tile
    std::string path;
    int clear(int tiles)  // in front of a fused launch
    {
        if (!dev) return 0;
        std::vector<unsigned long long> init((size_t)4 * tiles, 0ull);
        for (size_t i = 2; i < init.size(); i += 4) init[i] = ~0ull;
        HIP_OK(hipMemcpy(dev, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
        return 0;
    }
    int append(hipStream_t stream, int gx, int gy, uint32_t phase, unsigned tune)  // behind it
    {
        if (!dev) return 0;
        std::vector<unsigned long long> h((size_t)4 * gx * gy);
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(path.c_str(), "ab")) {
            const unsigned long long hdr[4] = {(unsigned long long)gx, (unsigned long long)gy, (unsigned long long)phase, (unsigned long long)tune};
            fwrite(hdr, sizeof hdr, 1, f);
            fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
            fclose(f);
        }
        return 0;
    }
};
#endif

#ifdef PM_CHECKED
// The bounds-checked TEST build (pm_core.h, -DPM_CHECKED): what the kernels of a session counted in Problem::viol -- one line
// per session, written when it is destroyed, appended to the file GIPUMA_CHECKED_LOG names (stderr without it): the accesses of
// each class that fell outside their buffer (window loads gray / integer-addressed / colour, norm4, cost, pushed costs, flags
// and rings).
inline void checked_collect(const unsigned long long *viol_dev, int cols, int rows, int ch, int box, int n_sel)
{
    unsigned long long h[pm::kDbgSlots] = {};
    if (hipMemcpy(h, viol_dev, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long total = 0;
    for (unsigned long long v : h) total += v;
    const char *path = getenv("GIPUMA_CHECKED_LOG");
    FILE *f = path ? fopen(path, "a") : stderr;
    if (!f) f = stderr;
    fprintf(f, "gipuma_hip CHECKED session %dx%d ch %d box %d views %d: violations %llu (window %llu, window-int %llu, window-c4 %llu, "
               "norm4 %llu, cost %llu, push_cost %llu, flags %llu)\n", cols, rows, ch, box, n_sel, total, h[0], h[1], h[2], h[3], h[4],
            h[5], h[6]);
    if (f != stderr) fclose(f);
}
#endif

}  // namespace
