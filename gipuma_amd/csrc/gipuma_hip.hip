// gipuma_hip.hip -- C-ABI (include/gipuma_hip.h) over the gfx950 kernels in pm_device.h.
//
// Host side of what the reference does in gipuma<T>() (gipuma.cu:1825-1960): validate, make the
// problem resident in HBM, launch init / red-black sweeps / finalize on one HIP stream, time with
// HIP events.  Differences from the reference that are deliberate:
//   * one launch per colour (close+far+refine fused, result-identical, see sweep_kernel) and no
//     host synchronisation between launches (the reference calls cudaDeviceSynchronize after
//     each of its 6 launches per iteration, gipuma.cu:1916-1936);
//   * cameras are packed once into one POD block read through scalar loads, instead of the
//     ~3600 managed allocations the reference dereferences on the device (camera.h:45-51);
//   * no per-pixel RNG state array (48 B/pixel, gipuma.cu:1840): the RNG is counter based.  Per-pixel state of a
//     session: 20 B planes + costs, 1 B history flag, and -- performance only, optional (the solve runs without
//     them when the allocation fails) -- 32 B pushed propagation costs and 16-64 B prefilter sample lists.
//
// This file is compiled THREE times into libgipuma_hip.so.  As itself it is the exact flavour (bit-identical to the CPU
// restatement of the numerical model) and owns the exported C-ABI.  Included by gipuma_hip_fast.hip (PM_APPROX = 1,
// namespace pm -> pm_fast) it is the tolerance-judged flavour behind GIPUMA_HIP_FLAG_FAST; included by gipuma_hip_literal.hip
// (PM_LITERAL = 1, pm_lit) the reference-order flavour behind GIPUMA_HIP_FLAG_LITERAL.  Same host logic in all three, in an
// unnamed namespace: a flavour is known to the others by one table of its session entry points (FlavourApi, generated from the
// list in pm_host_session.h).  An inclusion names the hidden function that returns its table (GIPUMA_HIP_FLAVOUR_API); the
// exact flavour adds the C-ABI, in which a session is a handle on the table and the session of the flavour it was created in.
//
// Host logic by header: pm_host_session.h (entry-point list, experiment switches, session and its device memory, kernel table,
// variant / early-termination / schedule stages), pm_host_images.h (images and their cache), pm_host_instrument.h (timers,
// counters, PM_WG_TICKS and PM_CHECKED hooks).  Here: the other stages of create, the launches, the entry points.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#ifdef GIPUMA_HIP_FLAVOUR_API
#pragma GCC visibility push(hidden)
#endif
#include "../../include/gipuma_hip.h"
#include "pm_device.h"
#include "pm_push.h"
#include "pm_group.h"
#include "pm_host_images.h"

namespace {

// The stages of create (more in pm_host_session.h, pm_host_images.h): each does what its name says or fails, last error set.
// device, stream and events; descriptor -> Problem fields
int open_session(Session *s, const gipuma_hip_desc *d)
{
    s->device = d->device_id;
    HIP_OK(hipSetDevice(s->device));
    s->unfused = (d->flags & GIPUMA_HIP_FLAG_UNFUSED) != 0;
    if (s->exp.tune)  // (the host-internal bits are not the caller's to set)
        s->tune = (unsigned)strtoul(s->exp.tune, nullptr, 0) &
                  ~(Tune::kHistorySkip | Tune::kUntrustedCosts | Tune::kAccumChanged | Tune::kPushConsume);
    if (d->stream) {
        s->stream = (hipStream_t)d->stream;
    } else {
        HIP_OK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        s->own_stream = true;
    }
    for (auto &e : s->ev) HIP_OK(hipEventCreate(&e));
    s->rows = d->rows;
    s->cols = d->cols;
    s->n_sel = d->n_selected;
    s->ch = d->channels;
    s->gx = (d->cols + pm::kTileW - 1) / pm::kTileW;
    s->gy = (d->rows + pm::kSweepTileH - 1) / pm::kSweepTileH;
    s->tiles = s->gx * s->gy;
    s->iterations = d->params.iterations;
    pm::Problem &hp = s->hp;
    hp.rows = d->rows;
    hp.cols = d->cols;
    hp.channels = d->channels;
    hp.pitch = (d->flags & GIPUMA_HIP_FLAG_IMAGES_ON_DEVICE) ? d->pitch : d->cols * d->channels;
    hp.n_sel = d->n_selected;
    hp.box_h = d->params.box_hsize;
    hp.box_v = d->params.box_vsize;
    hp.n_best = d->params.n_best;
    hp.cost_comb = d->params.cost_comb;
    hp.alpha = d->params.alpha;
    hp.tau_color = d->params.tau_color;
    hp.tau_gradient = d->params.tau_gradient;
    hp.gamma = d->params.gamma;
    hp.min_disp = d->params.min_disparity;
    hp.max_disp = d->params.max_disparity;
    hp.good_factor = d->params.good_factor;
    hp.seed = d->seed;
    return 0;
}

void copy9(float *dst, const float *src) { memcpy(dst, src, 9 * sizeof(float)); }
void copy3(float *dst, const float *src) { memcpy(dst, src, 3 * sizeof(float)); }

// cameras -> one POD block
int pack_cameras(Session *s, const gipuma_hip_desc *d)
{
    pm::Problem &hp = s->hp;
    const gipuma_hip_camera &c0 = d->cameras[0];
    copy9(hp.rc.K_inv, c0.K_inv);
    copy9(hp.rc.M_inv, c0.M_inv);
    copy9(hp.rc.R_orig_inv, c0.R_orig_inv);
    copy3(hp.rc.P_col34, c0.P_col34);
    copy3(hp.rc.C, c0.C);
    hp.rc.fx = c0.fx;
    hp.rc.cx = c0.K[2];  // cam.K[2], cam.K[2+3] in getDepthFromPlane3_cu, gipuma.cu:699-701
    hp.rc.cy = c0.K[5];
    hp.rc.alpha = c0.alpha;
    hp.rc.f = c0.f;
    hp.rc.baseline = c0.baseline;
    hp.rc.depth_min = c0.depth_min;
    hp.rc.depth_max = c0.depth_max;
    for (int i = 0; i < d->n_selected; i++) {
        const gipuma_hip_camera &c = d->cameras[d->selected[i]];
        copy9(hp.view[i].K, c.K);
        copy9(hp.view[i].R, c.R);
        copy3(hp.view[i].t, c.t);
#if PM_APPROX && defined(PM_APPROX_HFOLD)
        // A = K R K_ref^-1, u = K t (homography(), approx flavour), formed in double
        double KR[9];
        for (int r = 0; r < 3; r++)
            for (int q = 0; q < 3; q++)
                KR[3 * r + q] = (double)c.K[3 * r] * c.R[q] + (double)c.K[3 * r + 1] * c.R[3 + q] + (double)c.K[3 * r + 2] * c.R[6 + q];
        for (int r = 0; r < 3; r++) {
            for (int q = 0; q < 3; q++)
                hp.view[i].A[3 * r + q] = (float)(KR[3 * r] * c0.K_inv[q] + KR[3 * r + 1] * c0.K_inv[3 + q] + KR[3 * r + 2] * c0.K_inv[6 + q]);
            hp.view[i].u[r] = (float)((double)c.K[3 * r] * c.t[0] + (double)c.K[3 * r + 1] * c.t[1] + (double)c.K[3 * r + 2] * c.t[2]);
        }
#endif
    }
    return 0;
}

// per-pixel state, tile state and the counters of the instrumented builds
int alloc_state(Session *s, const gipuma_hip_desc *)
{
    pm::Problem &hp = s->hp;
    const size_t np = (size_t)s->rows * (size_t)s->cols;
    int rc = 0;
    s->et_hint_bytes = (size_t)s->tiles * 12;
    if ((rc = s->alloc({&hp.et_hint.raw, s->et_hint_bytes, 0}))) return rc;
    if ((rc = s->alloc({&hp.et_stat.raw, 3 * pm::kEtSlot * sizeof(unsigned), 0}))) return rc;
    // Skip rule (S) -- a ring of the last 8 planes a pixel's propagation evaluated, 129 B per pixel -- only where a
    // propagation candidate is expensive and nothing else shares its evaluation: colour sessions (their images are four
    // times the gray ones; measured with the round-3 library: late half-sweeps 6-9 % fewer tasks).  Gray sessions run
    // the plane-keyed propagation kernel instead and keep their footprint (config C: 0.3 % for 248 MB).
    // Performance only: without the memory the rule is off.
    if (s->ch == 4 && !(s->tune & (Tune::kNoSeen | Tune::kNoSkip)))
        if ((rc = s->alloc_optional({{&hp.seen_ring.raw, (size_t)pm::kSeenRing * np * sizeof(float4)}, {&hp.seen_pos.raw, np, 0}}))) return rc;
#ifdef PM_CHECKED  // (the bounds-checked TEST build, pm_core.h)
    if ((rc = s->alloc({&hp.viol.raw, pm::kDbgSlots * sizeof(unsigned long long), 0}))) return rc;
#endif
    if (s->exp.counts && (rc = s->alloc({&hp.dbg.raw, 64 * pm::kDbgSlots * sizeof(unsigned long long), 0}))) return rc;  // experiment aid
#ifdef PM_WG_TICKS
    if (s->exp.wg_ticks) {
        s->wg_ticks.path = s->exp.wg_ticks;
        if ((rc = s->alloc({&hp.wg_ticks.raw, 4 * (size_t)s->tiles * sizeof(unsigned long long)}))) return rc;
        s->wg_ticks.dev = hp.wg_ticks;
    }
#endif
    if ((rc = s->alloc({&hp.changed.raw, np, 1}))) return rc;
    // state planes, zero-filled like LineState::resize (linestate.h:16-24)
    if ((rc = s->alloc({&s->norm4, np * sizeof(float4), 0}))) return rc;
    return s->alloc({&s->cost, np * sizeof(float), 0});
}

int upload_problem(Session *s, const gipuma_hip_desc *)
{
    if (const int rc = s->alloc({&s->dp, sizeof(pm::Problem)})) return rc;
    HIP_OK(hipMemcpyAsync(s->dp, &s->hp, sizeof(pm::Problem), hipMemcpyHostToDevice, s->stream));
    HIP_OK(hipStreamSynchronize(s->stream));  // host image buffers may be released by the caller
    return 0;
}

// The launches of a session: the dense cost evaluation, and the state machine that turns one half-sweep into its launches (push /
// plane-keyed propagation, history rule, column-per-lane kernels) from the schedule that create resolved.

// pm::push_kernel: the planes of `colour` evaluated for their consumers (the pixels of the other colour)
int launch_push(Session *s, int colour, bool hist)
{
    hipLaunchKernelGGL(s->k.push.fn, dim3(s->tiles), dim3(pm::kThreads), s->k.push.lds, s->stream, s->dp, s->norm4, colour,
                       hist ? 1 : 0, s->tune);
    HIP_OK(hipGetLastError());
    s->push_valid = 1 - colour;
    s->push_hist = hist;
    return 0;
}

// pm::group_kernel: the propagation costs of the half-sweep of `colour` that follows, one evaluation per plane
int launch_group(Session *s, int colour, bool hist, unsigned tune)
{
    if (const int rc = s->timers.group_mark(0, s->stream)) return rc;
    hipLaunchKernelGGL(s->k.group.fn, dim3(s->tiles), dim3(pm::kThreads), s->k.group.lds, s->stream, s->dp, s->norm4, s->cost,
                       colour, hist ? 1 : 0, tune & ~(Tune::kPushConsume | Tune::kHistorySkip));
    HIP_OK(hipGetLastError());
    s->push_valid = colour;
    s->push_hist = hist;
    return s->timers.group_mark(1, s->stream);
}

// pm::sweep_group_kernel: propagation costs per plane + accept replay + refinement in one launch (pm_group.h)
int launch_fused(Session *s, int colour, uint32_t phase, unsigned tune)
{
    if (s->hp.tile_order) {  // this launch's dispatch order from the colour's previous durations (identity without any)
        hipLaunchKernelGGL(pm::tile_order_kernel, dim3(8), dim3(pm::kThreads), 0, s->stream, s->dp, colour, tune, s->hp.tile_order.raw);
        HIP_OK(hipGetLastError());
    }
    if (const int rc = s->wg_ticks.clear(s->tiles)) return rc;
    hipLaunchKernelGGL(s->k.fused.fn, dim3(s->tiles), dim3(pm::kThreads), s->k.fused.lds, s->stream, s->dp, s->norm4, s->cost,
                       colour, phase, tune);
    HIP_OK(hipGetLastError());
    return s->wg_ticks.append(s->stream, s->gx, s->gy, phase, tune);
}

int launch_sweep(Session *s, int iteration, int colour, unsigned stages)
{
    const uint32_t phase = 1u + 2u * (uint32_t)iteration + (uint32_t)colour;
    unsigned tune = s->tune | (s->costs_trusted ? 0u : Tune::kUntrustedCosts);
    // history rule (exact skipping (H) in pm_device.h): only inside a strictly alternating sequence of
    // full half-sweeps on trusted costs, as gipuma_hip_solve produces from its second iteration on
    const bool qualifies = stages == GIPUMA_STAGE_ALL && !s->unfused && s->costs_trusted;
    if (qualifies && s->prev1 == 1 - colour && s->prev2 == colour && !(tune & (Tune::kNoHistory | Tune::kNoSkip)))
        tune |= Tune::kHistorySkip;
    // will rule (H) hold for the next half-sweep if it is the other colour's full one?  (then prev1 = colour,
    // prev2 = today's prev1)
    const bool hist_next = qualifies && s->prev1 == 1 - colour && !(tune & (Tune::kNoHistory | Tune::kNoSkip));
    s->prev2 = s->prev1;
    s->prev1 = qualifies ? colour : -1;
    // push propagation: this half-sweep reads the costs of its propagation candidates from push_cost
    // (written by push_kernel after the previous half-sweep, or right now if nobody did), and offers
    // its own planes to the next one
    const int half_sweep = 2 * iteration + colour;
    const bool push_now = qualifies && half_sweep < s->push_launches;
    if (push_now) {
        const bool hist = (tune & Tune::kHistorySkip) != 0;
        if (s->push_valid != colour || s->push_hist != hist) {
            const int rc = launch_push(s, 1 - colour, hist);
            if (rc) return rc;
        }
        tune |= Tune::kPushConsume;
        s->timers.n_push_consumed++;
    }
    // plane-keyed propagation for the later half-sweeps (any skip rule the sweep would apply is applied there): in the
    // sweep's own launch (fused), or by pm::group_kernel in front of it
    const bool group_now = !push_now && qualifies && s->group_from >= 0 && half_sweep >= s->group_from;
    if (group_now && !s->group_fused) {
        const int rc = launch_group(s, colour, (tune & Tune::kHistorySkip) != 0, tune);
        if (rc) return rc;
        tune |= Tune::kPushConsume;
    }
    s->push_valid = -1;  // the planes of `colour` are about to change
    const bool push_next = qualifies && half_sweep + 1 < s->push_launches;
    // task order (performance only): planes are still incoherent in the first two iterations, where
    // grouping the evaluations of one plane saves cache-line fills; afterwards owner order is faster
    if (iteration >= 2 && !(tune & Tune::kSourceMajorTasks)) tune |= Tune::kOwnerMajorTasks;
    // ... and in the leading half-sweeps the evaluations themselves are done column-per-lane (8 lanes per
    // (pixel, plane) pair, pm::sweep_cols_kernel) where the session has that kernel
    const Launch<sweep_fn> &k =
        s->cols_ok && (half_sweep < s->cols_launches || (tune & Tune::kColsAlways)) ? s->k.sweep_cols : s->k.sweep;
    if (s->worder && !s->worder_valid) {
        const int n = s->rows * s->cols;
        hipLaunchKernelGGL(s->k.weight_order, dim3((n + pm::kThreads - 1) / pm::kThreads), dim3(pm::kThreads), 0, s->stream,
                           s->dp, s->worder);
        HIP_OK(hipGetLastError());
        s->worder_valid = true;
    }
    if (group_now && s->group_fused) return launch_fused(s, colour, phase, tune);
    hipLaunchKernelGGL(k.fn, dim3(s->tiles), dim3(pm::kThreads), k.lds, s->stream, s->dp, s->norm4, s->cost, colour, phase,
                       stages, tune);
    HIP_OK(hipGetLastError());
    if (push_next) return launch_push(s, colour, hist_next);
    return 0;
}

int launch_dense(Session *s, bool generate, float4 *planes, float *cost_out)
{
    // random (or arbitrary caller-supplied) planes: column-per-lane evaluation where the session has it
    const Launch<init_fn> &k = (s->cols_ok ? s->k.init_cols : s->k.init)[generate];
    const int gy = (s->rows + pm::kDenseTileH - 1) / pm::kDenseTileH;
    hipLaunchKernelGGL(k.fn, dim3(s->gx * gy), dim3(pm::kThreads), k.lds, s->stream, s->dp, planes, cost_out, s->tune);
    HIP_OK(hipGetLastError());
    return 0;
}

// What gipuma_hip_init_planes and gipuma_hip_seed_planes share: the launches in front of the kernel that writes a new plane
// field, and the session's state once that field and its costs are enqueued.
int new_planes_reset(Session *s)
{
    // (a fresh solve starts with fresh hints, so that repeated solves of a session do the same work)
    HIP_OK(hipMemsetAsync(s->hp.et_hint, 0, s->et_hint_bytes, s->stream));
    HIP_OK(hipMemsetAsync(s->hp.et_stat, 0, 3 * pm::kEtSlot * sizeof(unsigned), s->stream));
    s->worder_valid = false;  // (listed again by the first sweep: part of every solve)
    if (s->hp.tile_clock)  // (no durations yet: the first fused launch of either colour runs in the plain order)
        HIP_OK(hipMemsetAsync(s->hp.tile_clock, 0, 4 * (size_t)s->tiles * sizeof(unsigned long long), s->stream));
    if (s->hp.seen_pos) HIP_OK(hipMemsetAsync(s->hp.seen_pos, 0, (size_t)s->rows * s->cols, s->stream));  // rule (S): new planes
    return 0;
}

void new_planes_installed(Session *s, int rc)
{
    invalidate_history(s);
    s->costs_trusted = rc == 0;
    s->finalized = false;
}

// The session entry points of this flavour (GIPUMA_SESSION_ENTRY_POINTS; cache_clear: pm_host_images.h).

// (leaves the last-error text alone: a failed create reports its own failure)
int destroy(Session *s)
{
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    release_cached_images(s);
#ifdef PM_CHECKED
    if (s->hp.viol) checked_collect(s->hp.viol, s->cols, s->rows, s->ch, s->box, s->n_sel);
#endif
    s->release_memory();
    for (auto &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    s->timers.destroy();
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return 0;
}

// `d` has passed validate and the device check (gipuma_hip_create); destroy cleans up whatever the stages built
int create(const gipuma_hip_desc *d, Session **out)
{
    static int (*const stages[])(Session *, const gipuma_hip_desc *) = {
        open_session,              // device, stream, events; descriptor -> Problem fields
        make_images_resident,      // bind resident planes, or upload them
        classify_and_pack,         // 8-bit verdict, packed views (the image cache)
        pack_cameras,              // cameras -> POD block
        alloc_state,               // per-pixel state
        choose_variant,            // box, combiner, the kernels
        choose_early_termination,  // ... and the prefilter
        choose_schedule,           // push / plane-keyed / column-per-lane half-sweeps, pushed costs, dispatch order
        upload_problem,
    };
    Session *s = new (std::nothrow) Session;
    if (!s) return fail(GIPUMA_HIP_ERR_DEVICE, "out of host memory");
    for (auto stage : stages)
        if (const int rc = stage(s, d)) {
            destroy(s);
            return rc;
        }
    *out = s;
    return 0;
}

int init_planes(Session *s)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    HIP_OK(hipSetDevice(s->device));
    int rc = new_planes_reset(s);
    if (!rc) rc = launch_dense(s, true, s->norm4, s->cost);
    new_planes_installed(s, rc);
    return rc;
}

int seed_planes(Session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift)
{
    if (!s || !prior_dev) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    if (prior_rows < 1 || prior_cols < 1 || shift < 0 || shift > 15)
        return fail(GIPUMA_HIP_ERR_ARG, "seed: prior_rows / prior_cols must be positive and shift in 0..15");
    // (each lane reads the prior's pixel it covers and writes its own plane: only the same pixel may be both)
    if (shift != 0 && prior_dev == (const float *)s->norm4)
        return fail(GIPUMA_HIP_ERR_ARG, "seed: a session's own planes can seed it at shift 0 only");
    HIP_OK(hipSetDevice(s->device));
    int rc = new_planes_reset(s);
    if (!rc) {
        const int n = s->rows * s->cols;
        hipLaunchKernelGGL(pm::seed_kernel, dim3((n + pm::kThreads - 1) / pm::kThreads), dim3(pm::kThreads), 0, s->stream, s->dp,
                           s->norm4, (const float4 *)prior_dev, prior_rows, prior_cols, shift);
        HIP_OK(hipGetLastError());
        rc = launch_dense(s, false, s->norm4, s->cost);
    }
    new_planes_installed(s, rc);
    return rc;
}

int sweep(Session *s, int iteration, int colour, unsigned stages)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    if (iteration < 0 || (colour != GIPUMA_BLACK && colour != GIPUMA_RED) || (stages & ~7u))
        return fail(GIPUMA_HIP_ERR_ARG, "bad iteration/colour/stages");
    if (s->finalized)
        return fail(GIPUMA_HIP_ERR_ARG, "the session holds finalized maps (world normal, depth), not planes: call "
                                        "gipuma_hip_init_planes or gipuma_hip_set_state before sweeping again");
    HIP_OK(hipSetDevice(s->device));
    if (s->unfused) {  // the reference's three launches per colour, gipuma.cu:1915-1923
        for (unsigned st = 1; st <= 4; st <<= 1)
            if (stages & st) {
                int rc = launch_sweep(s, iteration, colour, st);
                if (rc) return rc;
            }
        return 0;
    }
    return stages ? launch_sweep(s, iteration, colour, stages) : 0;
}

int finalize(Session *s)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    HIP_OK(hipSetDevice(s->device));
    const int n = s->rows * s->cols;
    if (s->finalized) return fail(GIPUMA_HIP_ERR_ARG, "already finalized");
    hipLaunchKernelGGL(pm::finalize_kernel, dim3((n + pm::kThreads - 1) / pm::kThreads), dim3(pm::kThreads), 0,
                       s->stream, s->dp, s->norm4, s->cost);
    HIP_OK(hipGetLastError());
    s->finalized = true;
    invalidate_history(s);
    return 0;
}

int eval_cost(Session *s, const float *planes_host, float *cost_out_host)
{
    if (!s || !planes_host || !cost_out_host) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    HIP_OK(hipSetDevice(s->device));
    const size_t np = (size_t)s->rows * (size_t)s->cols;
    float4 *pl = nullptr;
    float *c = nullptr;
    HIP_OK(hipMalloc(&pl, np * sizeof(float4)));
    hipError_t e = hipMalloc(&c, np * sizeof(float));
    if (e != hipSuccess) {
        (void)hipFree(pl);
        return fail(GIPUMA_HIP_ERR_DEVICE, "hipMalloc: %s", hipGetErrorString(e));
    }
    int rc = 0;
    e = hipMemcpyAsync(pl, planes_host, np * sizeof(float4), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) rc = launch_dense(s, false, pl, c);
    if (e == hipSuccess && !rc)
        e = hipMemcpyAsync(cost_out_host, c, np * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(s->stream);
    (void)hipFree(pl);
    (void)hipFree(c);
    if (e != hipSuccess) return fail(GIPUMA_HIP_ERR_DEVICE, "eval_cost: %s", hipGetErrorString(e));
    return rc;
}

int get_state(Session *s, float *norm4_host, float *cost_host)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    HIP_OK(hipSetDevice(s->device));
    const size_t np = (size_t)s->rows * (size_t)s->cols;
    if (norm4_host)
        HIP_OK(hipMemcpyAsync(norm4_host, s->norm4, np * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    if (cost_host)
        HIP_OK(hipMemcpyAsync(cost_host, s->cost, np * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_OK(hipStreamSynchronize(s->stream));
    return 0;
}

int set_state(Session *s, const float *norm4_host, const float *cost_host)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    HIP_OK(hipSetDevice(s->device));
    const size_t np = (size_t)s->rows * (size_t)s->cols;
    if (norm4_host)
        HIP_OK(hipMemcpyAsync(s->norm4, norm4_host, np * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    if (cost_host)
        HIP_OK(hipMemcpyAsync(s->cost, cost_host, np * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (s->hp.seen_pos) HIP_OK(hipMemsetAsync(s->hp.seen_pos, 0, np, s->stream));  // rule (S): a cost may have gone up
    HIP_OK(hipStreamSynchronize(s->stream));
    invalidate_history(s);
    if (norm4_host) s->finalized = false;
    return 0;
}

int state_device_ptrs(Session *s, float **norm4_dev, float **cost_dev)
{
    if (!s) return fail(GIPUMA_HIP_ERR_ARG, "null session");
    if (norm4_dev) *norm4_dev = (float *)s->norm4;
    if (cost_dev) *cost_dev = s->cost;
    return 0;
}

// gipuma_hip_solve (prior_dev == nullptr: random planes) and gipuma_hip_solve_seeded
int solve_from(Session *s, gipuma_hip_timing *timing, const float *prior_dev, int prior_rows, int prior_cols, int shift)
{
    HIP_OK(hipSetDevice(s->device));
    int rc;
    SolveTimers &timers = s->timers;
    HIP_OK(hipEventRecord(s->ev[0], s->stream));
    if ((rc = prior_dev ? seed_planes(s, prior_dev, prior_rows, prior_cols, shift) : init_planes(s))) return rc;
    HIP_OK(hipEventRecord(s->ev[1], s->stream));
    if ((rc = timers.begin(timing || s->exp.launch_times, 2 * s->iterations, s->stream))) return rc;
    for (int h = 0; h < 2 * s->iterations; h++) {  // gipuma.cu:1911-1941: per iteration the black half-sweep, then the red one
        timers.enter(h);
        if ((rc = timers.mark(h, s->stream, sweep(s, h / 2, h % 2 ? GIPUMA_RED : GIPUMA_BLACK, GIPUMA_STAGE_ALL)))) return rc;
    }
    HIP_OK(hipEventRecord(s->ev[2], s->stream));
    if ((rc = finalize(s))) return rc;
    HIP_OK(hipEventRecord(s->ev[3], s->stream));
    if (timing) {
        HIP_OK(hipEventSynchronize(s->ev[3]));
        HIP_OK(hipEventElapsedTime(&timing->ms_init, s->ev[0], s->ev[1]));
        HIP_OK(hipEventElapsedTime(&timing->ms_sweeps, s->ev[1], s->ev[2]));
        HIP_OK(hipEventElapsedTime(&timing->ms_finalize, s->ev[2], s->ev[3]));
        HIP_OK(hipEventElapsedTime(&timing->ms_total, s->ev[0], s->ev[3]));
        timing->n_sweep_launches = s->iterations * (s->unfused ? 6 : 2);
        timing->ms_sweep_avg = timing->n_sweep_launches ? timing->ms_sweeps / (float)timing->n_sweep_launches : 0.0f;
    }
    if ((rc = timers.collect(s->ev[3], s->exp.launch_times))) return rc;
    if (timers.timed && s->hp.dbg) return report_counts(s->hp.dbg, s->rows, s->cols, s->iterations);
    return 0;
}

int solve(Session *s, gipuma_hip_timing *timing)
{
    return s ? solve_from(s, timing, nullptr, 0, 0, 0) : fail(GIPUMA_HIP_ERR_ARG, "null session");
}

int solve_seeded(Session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift, gipuma_hip_timing *timing)
{
    return s && prior_dev ? solve_from(s, timing, prior_dev, prior_rows, prior_cols, shift) : fail(GIPUMA_HIP_ERR_ARG, "null argument");
}

int launch_times(Session *s, float *ms_half_sweep, int capacity, int *n_half_sweeps, int *n_pushed)
{
    if (s && n_pushed) *n_pushed = s->timers.n_pushed;
    return s ? copy_times(s->timers.half_sweep_ms, ms_half_sweep, capacity, n_half_sweeps) : fail(GIPUMA_HIP_ERR_ARG, "null session");
}

int group_times(Session *s, float *ms_group, int capacity, int *n_half_sweeps)
{
    return s ? copy_times(s->timers.group_ms, ms_group, capacity, n_half_sweeps) : fail(GIPUMA_HIP_ERR_ARG, "null session");
}

int schedule(Session *s, int info[4])
{
    if (!s || !info) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    info[0] = s->push_launches;
    info[1] = s->group_from;
    info[2] = s->group_fused ? 1 : 0;
    info[3] = s->cols_launches;
    return 0;
}

const FlavourApi<Session> kApi = {
#define X(name, params) name,
    GIPUMA_SESSION_ENTRY_POINTS(X)
#undef X
};
// (the same table with the session pointers typed void *: formally undefined, what -fsanitize=function would flag in a host
// build; the same calling convention on this ABI, and what a C prototype with void * across units does)
const FlavourApi<void> *opaque_api() { return reinterpret_cast<const FlavourApi<void> *>(&kApi); }

}  // namespace

#ifdef GIPUMA_HIP_FLAVOUR_API
// all that another translation unit sees of this flavour (hidden: not part of the C-ABI)
extern "C" const FlavourApi<void> *GIPUMA_HIP_FLAVOUR_API(void) { return opaque_api(); }
#pragma GCC visibility pop
#else
// The exact flavour: the exported C-ABI.
extern "C" __attribute__((visibility("hidden"))) const FlavourApi<void> *gipuma_hipf_api(void);  // gipuma_hip_fast.hip
extern "C" __attribute__((visibility("hidden"))) const FlavourApi<void> *gipuma_hipl_api(void);  // gipuma_hip_literal.hip

// a session of the C-ABI: the flavour it was created in, and that flavour's session
struct gipuma_hip_session {
    const FlavourApi<void> *api;
    void *impl;
};

namespace {

thread_local std::string g_err;

// a session entry point of the C-ABI goes to the session's flavour; a null session to this one, which reports it
#define FORWARD(s, fn, ...) ((s) ? (s)->api->fn((s)->impl, ##__VA_ARGS__) : kApi.fn(nullptr, ##__VA_ARGS__))

int validate(const gipuma_hip_desc *d)
{
    if (!d) return fail(GIPUMA_HIP_ERR_ARG, "null descriptor");
    if (d->abi_version != GIPUMA_HIP_ABI_VERSION) return fail(GIPUMA_HIP_ERR_ARG, "abi_version mismatch");
    if (d->rows < 1 || d->cols < 1) return fail(GIPUMA_HIP_ERR_ARG, "rows/cols must be positive");
    if ((long long)d->rows * (long long)d->pitch >= (1LL << 29))
        return fail(GIPUMA_HIP_ERR_ARG, "image too large for 32-bit texel offsets");
    if (d->channels != 1 && d->channels != 4)
        return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "channels must be 1 (gray, T=float) or 4 (colour, T=float4)");
    if (d->pitch < d->cols * d->channels) return fail(GIPUMA_HIP_ERR_ARG, "pitch < cols*channels");
    if (d->channels == 4 && (d->pitch & 3)) return fail(GIPUMA_HIP_ERR_ARG, "colour pitch must be a multiple of 4 floats");
    if (d->n_images < 1 || d->n_images > 512 || !d->images || !d->cameras)
        return fail(GIPUMA_HIP_ERR_ARG, "images/cameras missing");
    if (d->n_selected < 0 || d->n_selected > GIPUMA_HIP_MAX_VIEWS || (d->n_selected > 0 && !d->selected))
        return fail(GIPUMA_HIP_ERR_ARG, "n_selected must be 0..32 (gipuma.cu:736)");
    for (int i = 0; i < d->n_selected; i++)
        if (d->selected[i] < 0 || d->selected[i] >= d->n_images || !d->images[d->selected[i]])
            return fail(GIPUMA_HIP_ERR_ARG, "selected view out of range");
    if (!d->images[0]) return fail(GIPUMA_HIP_ERR_ARG, "reference image missing");
    const gipuma_hip_params &p = d->params;
    if (p.box_hsize < 1 || p.box_vsize < 1 || !(p.box_hsize & 1) || !(p.box_vsize & 1))
        return fail(GIPUMA_HIP_ERR_ARG, "box sizes must be odd (main.cpp:269-276)");
    if (p.box_hsize > 49 || p.box_vsize > 49) return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "box size > 49");
    if (p.iterations < 0) return fail(GIPUMA_HIP_ERR_ARG, "iterations < 0");
    return 0;
}

// what the selftests share: the device check (their own code and text for a bad ordinal), a mismatch counter around `launches`
template <class L>
int selftest(int device_id, const char *bad_argument, unsigned long long *mismatches, L launches)
{
    if (device_id < 0 || device_id >= pm_host::device_count()) return fail(GIPUMA_HIP_ERR_NO_DEVICE, "no such HIP device");
    if (bad_argument) return fail(GIPUMA_HIP_ERR_ARG, "%s", bad_argument);
    HIP_OK(hipSetDevice(device_id));
    unsigned long long *d = nullptr;
    HIP_OK(hipMalloc(&d, sizeof *d));
    hipError_t e = hipMemset(d, 0, sizeof *d);
    if (e == hipSuccess) e = launches(d);
    if (e == hipSuccess) e = hipMemcpy(mismatches, d, sizeof *d, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(GIPUMA_HIP_ERR_DEVICE, "selftest: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int gipuma_hip_version(void) { return GIPUMA_HIP_ABI_VERSION; }

const char *gipuma_hip_last_error(void) { return g_err.c_str(); }

// the one last-error text of the library, per thread: every translation unit reports through pm_host::fail, which ends here
// (hidden, not part of the C-ABI)
__attribute__((visibility("hidden"))) void gipuma_set_last_error(const char *text) { g_err = text; }

int gipuma_hip_device_count(void) { return pm_host::device_count(); }

int gipuma_hip_cache_clear(void)
{
    for (const FlavourApi<void> *api : {gipuma_hipf_api(), gipuma_hipl_api(), opaque_api()})  // (each keeps its own packed planes)
        if (const int rc = api->cache_clear()) return rc;
    return 0;
}

int gipuma_hip_selftest_reciprocal(int device_id, unsigned long long *mismatches)
{
    if (!mismatches) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    return selftest(device_id, nullptr, mismatches, [](unsigned long long *d) {
        hipLaunchKernelGGL(pm::rcp_selftest_kernel, dim3(65536), dim3(pm::kThreads), 0, 0, d, 1u, 252u);
        return hipGetLastError();
    });
}

int gipuma_hip_selftest_quotient(int device_id, unsigned z_first, unsigned z_count, unsigned long long *mismatches)
{
    if (!mismatches) return fail(GIPUMA_HIP_ERR_ARG, "null argument");
    const bool in_range = z_first < (1u << 23) && z_count <= (1u << 23) - z_first;
    return selftest(device_id, in_range ? nullptr : "significand range out of 0..2^23", mismatches, [=](unsigned long long *d) {
        hipError_t e = hipSuccess;
        // (launches of at most 2^14 denominators: ~0.1 s each, so that no single launch runs for minutes)
        for (unsigned done = 0; e == hipSuccess && done < z_count; done += 1u << 14) {
            const unsigned n = std::min(z_count - done, 1u << 14);
            hipLaunchKernelGGL(pm::quotient_selftest_kernel, dim3(n), dim3(pm::kThreads), 0, 0, d, z_first + done);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        return e;
    });
}

int gipuma_hip_create(const gipuma_hip_desc *d, gipuma_hip_session **out)
{
    if (!out) return fail(GIPUMA_HIP_ERR_ARG, "null out pointer");
    *out = nullptr;
    int rc = validate(d);
    if (!rc) rc = pm_host::check_device(d->device_id);
    if (rc) return rc;
    if ((d->flags & GIPUMA_HIP_FLAG_FAST) && (d->flags & GIPUMA_HIP_FLAG_LITERAL))
        return fail(GIPUMA_HIP_ERR_ARG, "GIPUMA_HIP_FLAG_FAST and GIPUMA_HIP_FLAG_LITERAL exclude each other");
    gipuma_hip_session *s = new (std::nothrow) gipuma_hip_session;
    if (!s) return fail(GIPUMA_HIP_ERR_DEVICE, "out of host memory");
    s->api = (d->flags & GIPUMA_HIP_FLAG_LITERAL) ? gipuma_hipl_api() : (d->flags & GIPUMA_HIP_FLAG_FAST) ? gipuma_hipf_api() : opaque_api();
    if ((rc = s->api->create(d, &s->impl))) {
        delete s;
        return rc;
    }
    *out = s;
    return 0;
}

int gipuma_hip_destroy(gipuma_hip_session *s)
{
    if (!s) return 0;
    const int rc = s->api->destroy(s->impl);
    delete s;
    return rc;
}

// the session entry points of include/gipuma_hip.h: each goes to the function of its name in the session's flavour
#define C_ABI(name, params, ...) int gipuma_hip_##name params { return FORWARD(s, name, ##__VA_ARGS__); }
C_ABI(init_planes, (gipuma_hip_session *s))
C_ABI(seed_planes, (gipuma_hip_session *s, const float *prior, int rows, int cols, int shift), prior, rows, cols, shift)
C_ABI(sweep, (gipuma_hip_session *s, int iteration, int colour, unsigned stages), iteration, colour, stages)
C_ABI(finalize, (gipuma_hip_session *s))
C_ABI(eval_cost, (gipuma_hip_session *s, const float *planes_host, float *cost_out_host), planes_host, cost_out_host)
C_ABI(get_state, (gipuma_hip_session *s, float *norm4_host, float *cost_host), norm4_host, cost_host)
C_ABI(set_state, (gipuma_hip_session *s, const float *norm4_host, const float *cost_host), norm4_host, cost_host)
C_ABI(state_device_ptrs, (gipuma_hip_session *s, float **norm4_dev, float **cost_dev), norm4_dev, cost_dev)
C_ABI(solve, (gipuma_hip_session *s, gipuma_hip_timing *timing), timing)
C_ABI(solve_seeded, (gipuma_hip_session *s, const float *prior, int rows, int cols, int shift, gipuma_hip_timing *timing), prior, rows, cols, shift, timing)
C_ABI(launch_times, (gipuma_hip_session *s, float *ms, int capacity, int *n_half_sweeps, int *n_pushed), ms, capacity, n_half_sweeps, n_pushed)
C_ABI(group_times, (gipuma_hip_session *s, float *ms_group, int capacity, int *n_half_sweeps), ms_group, capacity, n_half_sweeps)
C_ABI(schedule, (gipuma_hip_session *s, int info[4]), info)
#undef C_ABI

int gipuma_hip_run(const gipuma_hip_desc *desc, float *norm4_out, float *cost_out, gipuma_hip_timing *timing)
{
    gipuma_hip_session *s = nullptr;
    int rc = gipuma_hip_create(desc, &s);
    if (rc) return rc;
    gipuma_hip_timing t{};
    rc = gipuma_hip_solve(s, &t);
    if (!rc) rc = gipuma_hip_get_state(s, norm4_out, cost_out);
    if (timing) *timing = t;
    gipuma_hip_destroy(s);  // (leaves the last-error text alone)
    return rc;
}

}  // extern "C"
#endif
