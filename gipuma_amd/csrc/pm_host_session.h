// pm_host_session.h -- what a session of gipuma_hip.hip is and what gipuma_hip_create decides about it: the one list of the
// session entry points a flavour offers, the experiment switches, the session with the device memory it owns, the kernel
// table, and the stages of create that pick the kernel variant, the schedule and the early-termination parameters.  Host
// only; included once per flavour, after the device headers (pm_device.h, pm_push.h, pm_group.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <optional>
#include <tuple>
#include <vector>

#include "pm_host.h"
#include "pm_host_instrument.h"

// The session entry points of a flavour, the one list of them: FlavourApi and each flavour's table (gipuma_hip.hip, kApi) are
// generated from it, in this order.  `create` is handed a descriptor that gipuma_hip_create has validated.
#define GIPUMA_SESSION_ENTRY_POINTS(X)                                                                                 \
    X(cache_clear, (void))                                                                                             \
    X(create, (const gipuma_hip_desc *desc, Session **out))                                                            \
    X(destroy, (Session *s))                                                                                           \
    X(init_planes, (Session *s))                                                                                       \
    X(sweep, (Session *s, int iteration, int colour, unsigned stages))                                                 \
    X(finalize, (Session *s))                                                                                          \
    X(eval_cost, (Session *s, const float *planes_host, float *cost_out_host))                                         \
    X(get_state, (Session *s, float *norm4_host, float *cost_host))                                                    \
    X(set_state, (Session *s, const float *norm4_host, const float *cost_host))                                        \
    X(state_device_ptrs, (Session *s, float **norm4_dev, float **cost_dev))                                            \
    X(solve, (Session *s, gipuma_hip_timing *timing))                                                                  \
    X(launch_times, (Session *s, float *ms_half_sweep, int capacity, int *n_half_sweeps, int *n_pushed))               \
    X(group_times, (Session *s, float *ms_group, int capacity, int *n_half_sweeps))                                    \
    X(schedule, (Session *s, int info[4]))                                                                             \
    X(seed_planes, (Session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift))                    \
    X(solve_seeded, (Session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift, gipuma_hip_timing *timing))

// a flavour's entry points; FlavourApi<void> is how another translation unit holds them (the session is opaque there)
template <class Session>
struct FlavourApi {
#define X(name, params) int(*name) params;
    GIPUMA_SESSION_ENTRY_POINTS(X)
#undef X
};

namespace {

using pm::Tune;
using pm_host::fail;

// Experiment switches (A/B runs, tests of the work-reduction rules): every GIPUMA_HIP_<name> variable below is read
// ONLY when GIPUMA_HIP_EXPERIMENTS is set to a non-zero value -- a production process never changes its schedule on
// ambient environment variables.  None of them changes a result (tests/test_parity_gpu.py).
const char *exp_text(const char *name)
{
    const char *on = getenv("GIPUMA_HIP_EXPERIMENTS");
    return on && atoi(on) != 0 ? getenv(name) : nullptr;
}
std::optional<int> exp_number(const char *name)
{
    const char *t = exp_text(name);
    return t ? std::optional<int>(atoi(t)) : std::nullopt;
}

// every switch there is, read once when gipuma_hip_create makes the session; the stages of create read this struct (texts
// are the environment's own: parsed by a stage of that create, not kept)
struct Experiments {
    const char *tune = exp_text("GIPUMA_HIP_TUNE");  // pm::Tune bits, any base (the host-internal ones are masked out)
    bool launch_times = exp_number("GIPUMA_HIP_LAUNCH_TIMES").value_or(0) != 0;  // experiment aid: every half-sweep of a solve timed, to stderr
    bool counts = exp_number("GIPUMA_HIP_COUNTS").value_or(0) != 0;  // experiment aid: Problem::dbg, report_counts
    std::optional<int> push_launches = exp_number("GIPUMA_HIP_PUSH_LAUNCHES");  // A/B runs: 0 = never
    std::optional<int> group_from = exp_number("GIPUMA_HIP_GROUP_FROM");        // <first half-sweep> (< 0 = never)
    std::optional<int> group_fused = exp_number("GIPUMA_HIP_GROUP_FUSED");      // 0: two launches in gray too
    std::optional<int> cols_launches = exp_number("GIPUMA_HIP_COLS_LAUNCHES");  // experiment; < 0: the default
    std::optional<int> push_lds_kb = exp_number("GIPUMA_HIP_PUSH_LDS_KB");      // experiment: fewer workgroups per CU
    // tests on small frames; 2 (tests): every workgroup bounds every step, whatever the probes measured
    std::optional<int> et_force = exp_number("GIPUMA_HIP_ET_FORCE");
    std::optional<int> tp_g0 = exp_number("GIPUMA_HIP_TP_G0");    // experiment: phase-1 columns
    const char *et_theta = exp_text("GIPUMA_HIP_ET_THETA");       // experiment: "t0,t1,t2" (any value is exact)
    std::optional<int> lb_k = exp_number("GIPUMA_HIP_LB_K");      // experiment: fixed length, < 0 = off
    std::optional<int> tile_order = exp_number("GIPUMA_HIP_TILE_ORDER");  // 0/1: A/B runs
#ifdef PM_WG_TICKS
    const char *wg_ticks = exp_text("GIPUMA_HIP_WG_TICKS");  // <file>: per-workgroup clocks of the fused launches
#endif
};

typedef void (*init_fn)(const pm::Problem *, float4 *, float *, unsigned);
typedef void (*sweep_fn)(const pm::Problem *, float4 *, float *, int, uint32_t, unsigned, unsigned);
typedef void (*push_fn)(const pm::Problem *, const float4 *, int, int, unsigned);
typedef void (*group_fn)(const pm::Problem *, const float4 *, const float *, int, int, unsigned);
typedef void (*fused_fn)(const pm::Problem *, float4 *, float *, int, uint32_t, unsigned);
typedef void (*order_fn)(const pm::Problem *, uint32_t *);

template <class F>
struct Launch {
    F fn = nullptr;  // nullptr: no instantiation for the session's (box, channels)
    size_t lds = 0;  // dynamic LDS bytes of its launches
};

// the kernels of a session, one per family, chosen once by gipuma_hip_create (kernels_for)
struct Kernels {
    Launch<init_fn> init[2], init_cols[2];  // [generate]: costs of given planes / random planes and their costs
    Launch<sweep_fn> sweep, sweep_cols;
    Launch<push_fn> push;
    Launch<group_fn> group;
    Launch<fused_fn> fused;
    order_fn weight_order = nullptr;
    int lb_max = 0;  // samples the prefilter lists per pixel (pm::lb_max)
};

// GIPUMA_HIP_FLAG_CACHE_IMAGES (pm_host_images.h): an image plane is known by (device, address, rows, cols, pitch, channels)
typedef std::tuple<int, const void *, int, int, int, int> CacheKey;

struct Session {
    const Experiments exp;
    int device = 0;
    int rows = 0, cols = 0, n_sel = 0, iterations = 0;
    pm::Problem hp{};  // (its device buffers are allocated straight into its pointers: alloc({&hp.changed.raw, ...}))
    pm::Problem *dp = nullptr;
    float4 *norm4 = nullptr;
    float *cost = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool u8 = false;         // every image integer valued in [0,255] -> weight table + packed windows
    std::vector<CacheKey> cache_refs;  // shared packed views it holds a use count on (GIPUMA_HIP_FLAG_CACHE_IMAGES)
    bool combine_reg = false;
    bool unfused = false;
    // state invariant cost[p] == cost(p, plane[p]): true once init_planes has run, not assumed after
    // gipuma_hip_set_state (the caller may install any pair); the sweep kernel's skip rule (A) needs it
    bool costs_trusted = false;
    // gipuma_hip_finalize rewrites norm4 in place to (world normal, depth): no sweep may follow until the
    // planes are re-initialised or re-installed
    bool finalized = false;
    // history rule bookkeeping: colours of the last two launches that were full-stage, fused, trusted
    // half-sweeps (-1 otherwise); the rule is valid for colour c iff prev1 == 1-c and prev2 == c
    int prev1 = -1, prev2 = -1;
    size_t et_hint_bytes = 0;  // 12 bytes per sweep tile (Problem::et_hint)
    WgTicks wg_ticks;
    // lower-bound prefilter of refinement candidates (pm::lb_item): the heaviest window samples of every
    // pixel, listed by pm::weight_order_kernel at the start of every solve (init_planes) or before the
    // first sweep that needs them
    uint32_t *worder = nullptr;  // device, Problem::worder
    bool worder_valid = false;
    // push propagation (pm_push.h): after a half-sweep the planes of its colour are evaluated once for
    // all their consumers; the next half-sweep reads those costs instead of evaluating them
    int push_valid = -1;       // colour whose pixels find valid costs in push_cost (-1: nobody)
    bool push_hist = false;    // ... offered under rule (H) (only the planes that changed)
    int box = 0;             // specialised window size, 0 = runtime
    int ch = 1;              // 1 = gray (T=float), 4 = colour (T=float4)
    unsigned tune = 0;
    // what the launches run, resolved once by gipuma_hip_create (gipuma_hip_schedule reports it)
    Kernels k;
    int gx = 0, gy = 0, tiles = 0;  // sweep tiles (pm::kTileW x pm::kSweepTileH) per row, per column, in all
    int push_launches = 0;      // leading half-sweeps (2*iteration + colour) that consume pushed costs (0: none)
    // plane-keyed propagation (pm_group.h): from half-sweep `group_from` on (-1: never) the propagation costs of a
    // half-sweep come from pm::group_kernel launched right before it, or from one launch of pm::sweep_group_kernel
    int group_from = -1;
    bool group_fused = false;
    bool cols_ok = false;       // the column-per-lane kernels run (random planes; the leading half-sweeps)
    int cols_launches = 0;      // leading half-sweeps (2*iteration + colour) evaluated column-per-lane
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    SolveTimers timers;

    // Device memory: every buffer the session owns is allocated here and freed by release_memory, nowhere else.  (Packed
    // views shared through the image cache belong to the cache.)
    std::vector<void *> memory;
    struct Want {
        void **ptr;
        size_t bytes;
        int fill;  // byte value, < 0: none
        template <class T> Want(T **p, size_t n, int byte = -1) : ptr((void **)p), bytes(n), fill(byte) {}
    };
    // All of `wants` -- allocated, recorded, filled with a byte value on the session's stream where asked -- or none of them.
    // Without the memory: `required` fails; else the pointers are null again, the HIP error is cleared and the call succeeds.
    int alloc_all(std::initializer_list<Want> wants, bool required)
    {
        const size_t mark = memory.size();
        for (const Want &w : wants) {
            const hipError_t e = hipMalloc(w.ptr, w.bytes);
            if (e == hipSuccess) {
                memory.push_back(*w.ptr);
                continue;
            }
            (void)hipGetLastError();
            for (; memory.size() > mark; memory.pop_back()) (void)hipFree(memory.back());
            for (const Want &u : wants) *u.ptr = nullptr;
            return required ? fail(GIPUMA_HIP_ERR_DEVICE, "hipMalloc of %zu bytes: %s", w.bytes, hipGetErrorString(e)) : 0;
        }
        for (const Want &w : wants)
            if (w.fill >= 0) HIP_OK(hipMemsetAsync(*w.ptr, w.fill, w.bytes, stream));
        return 0;
    }
    int alloc(const Want &w) { return alloc_all({w}, true); }  // required state
    // performance-only state: where the pointers stay null the caller switches the feature off -- the solve runs without it,
    // same results
    int alloc_optional(std::initializer_list<Want> wants) { return alloc_all(wants, false); }
    void release_memory()
    {
        for (void *p : memory) (void)hipFree(p);
        memory.clear();
    }
};

// what the launches remember about the plane field, reset: costs not trusted, history rule not valid, no pushed costs valid
void invalidate_history(Session *s)
{
    s->costs_trusted = false;
    s->prev1 = s->prev2 = -1;
    s->push_valid = -1;
}

// The kernel table: every kernel instantiation a session can launch is named here and nowhere else, each pointer together
// with its dynamic LDS size.  A family without an instantiation for (BOX, CH) stays nullptr, and the schedule that
// gipuma_hip_create resolves from this table never launches it.  What exists, as built and measured:
//   * colour box 19 runs the generic (box 0) kernels: gipuma_hip_create gives such a session box 0;
//   * colour sessions have push, plane-keyed and column-per-lane kernels for box 15 only;
//   * the fused plane-keyed kernel (pm::sweep_group_kernel) is gray only (the colour one held two workgroups
//     per CU at 256 registers with 121 spilled, was slower, and could not be trusted);
//   * no column-per-lane kernels for box 11 (6 of 8 lanes: slower than one lane per pixel, config B 18.0 vs 19.8 Mpix/s);
//   * the prefilter's weight order (pm::weight_order_kernel) exists for every specialised box, colour 11 / 15 / 25
//     included, and lb_max<BOX>() sizes its planes for colour sessions too;
//   * the no-interior A/B arm (Tune::kNoInterior, gray) has two variants: box 15 on 8-bit images with the register
//     combiner, and box 0 with the generic combiner -- gipuma_hip_create gives every other such session box 0 and the
//     generic combiner, as it gives box 0 to parameters the specialised loops cannot fold exactly (fold_exact).
template <int BOX, int CH>
Kernels kernels_for(bool u8, bool creg, bool no_interior, size_t lds_sweep, size_t lds_dense)
{
    constexpr bool gray_box = CH == 1 && BOX > 0;  // 11 / 15 / 19 / 25
    constexpr bool push_box = gray_box || (CH == 4 && BOX == 15);
    constexpr bool cols_box = (CH == 1 && (BOX == 15 || BOX == 19 || BOX == 25)) || (CH == 4 && BOX == 15);
    Kernels k;
    k.init[0] = {u8 ? pm::init_kernel<BOX, true, false, false, CH> : pm::init_kernel<BOX, false, false, false, CH>, lds_dense};
    k.init[1] = {u8 ? pm::init_kernel<BOX, true, false, true, CH> : pm::init_kernel<BOX, false, false, true, CH>, lds_dense};
    if (u8)
        k.sweep = {creg ? pm::sweep_kernel<BOX, true, true, true, CH> : pm::sweep_kernel<BOX, true, false, true, CH>, lds_sweep};
    else
        k.sweep = {creg ? pm::sweep_kernel<BOX, false, true, true, CH> : pm::sweep_kernel<BOX, false, false, true, CH>, lds_sweep};
    if constexpr (CH == 1 && BOX == 15)
        if (no_interior) k.sweep.fn = pm::sweep_kernel<15, true, true, false, 1>;  // (8-bit, register combiner)
    if constexpr (CH == 1 && BOX == 0)
        if (no_interior) k.sweep.fn = u8 ? pm::sweep_kernel<0, true, false, false, 1> : pm::sweep_kernel<0, false, false, false, 1>;
    if constexpr (cols_box) {
        k.init_cols[0] = {pm::init_cols_kernel<BOX, false, CH>, lds_dense};
        k.init_cols[1] = {pm::init_cols_kernel<BOX, true, CH>, lds_dense};
        k.sweep_cols = {creg ? pm::sweep_cols_kernel<BOX, true, CH> : pm::sweep_cols_kernel<BOX, false, CH>, lds_sweep};
    }
    if constexpr (push_box) {
        if constexpr (CH == 4)
            k.push = {pm::push_kernel_c4<BOX>, sizeof(float) * (size_t)pm::PushLayoutC4<BOX>::total};
        else
            k.push = {pm::push_kernel<BOX>, sizeof(float) * (size_t)pm::PushLayout<BOX>::total};
        k.group = {pm::group_kernel<BOX, CH>, sizeof(float) * (size_t)pm::GroupLayout<BOX, CH>::total};
    }
    if constexpr (gray_box)  // (its tile is the plane-keyed kernel's and the sweep's: the larger of the two layouts)
        k.fused = {pm::sweep_group_kernel<BOX>, std::max(sizeof(float) * (size_t)pm::GroupLayout<BOX>::total, lds_sweep)};
    if constexpr (BOX > 0) {
        k.weight_order = pm::weight_order_kernel<BOX, CH>;
        k.lb_max = pm::lb_max<BOX>();
    }
    return k;
}

constexpr int box_ch(int box, int ch) { return 8 * box + ch; }

// the one place a session's (box, channels) reaches kernels_for
bool session_kernels(Session *s, size_t lds_sweep, size_t lds_dense)
{
    const bool no_interior = (s->tune & Tune::kNoInterior) != 0;
    switch (box_ch(s->box, s->ch)) {
#define KERNELS(B, C)                                                                                 \
    case box_ch(B, C):                                                                                \
        s->k = kernels_for<B, C>(s->u8, s->combine_reg, no_interior, lds_sweep, lds_dense);           \
        return true
    KERNELS(0, 1); KERNELS(11, 1); KERNELS(15, 1); KERNELS(19, 1); KERNELS(25, 1);
    KERNELS(0, 4); KERNELS(11, 4); KERNELS(15, 4); KERNELS(25, 4);
#undef KERNELS
    }
    return false;
}

template <class F>
hipError_t allow_lds(const Launch<F> &k)  // (gfx950: up to 160 KiB of dynamic LDS per workgroup)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
}

size_t lds_bytes(const Session *s, int tile_h, bool with_cv, bool sweep)
{
    const int hw = (s->hp.box_h + 1) / 2, hh = (s->hp.box_v + 1) / 2;
    const int texels = (pm::kTileW + 2 * hw) * (tile_h + 2 * hh);
    size_t n = (s->ch == 4 ? pm::lut_size<4>() : pm::lut_size<1>()) + (size_t)4 * texels +
               (size_t)(s->ch == 4 ? pm::work_floats<4>(texels, sweep) : pm::work_floats<1>(texels, sweep));
    if (with_cv) n += (size_t)s->n_sel * pm::kThreads;
    return n * sizeof(float);
}

// ---- stages of gipuma_hip_create (gipuma_hip.hip runs them in this order, after the images are resident and packed) ----

// kernel variant: the window size compiled in where kernels_for has it -- colour box 19 runs the generic kernels --
// else box 0 (the window size at run time)
int choose_variant(Session *s, const gipuma_hip_desc *)
{
    const pm::Problem &hp = s->hp;
    s->box = 0;
    if (hp.box_h == hp.box_v && !(s->tune & Tune::kGenericBox) &&
        (hp.box_h == 11 || hp.box_h == 15 || hp.box_h == 25 || (hp.box_h == 19 && s->ch == 1)))
        s->box = hp.box_h;
    // the specialised loops fold the gradient term's 1/16 into alpha and tau_gradient (dis_fold, pm_cost.h): exact
    // unless alpha / 16 is subnormal or 16 tau_gradient overflows -- such parameters take the literal generic loop
    const float a16 = hp.alpha * 0.0625f, tg16 = hp.tau_gradient * 16.0f;
    const bool fold_exact = a16 * 16.0f == hp.alpha && (std::isfinite(tg16) || !std::isfinite(hp.tau_gradient));
    if (!fold_exact) s->box = 0;
    s->combine_reg = hp.cost_comb == GIPUMA_COMB_BEST_N && hp.n_best >= 1 && hp.n_best <= 4 &&
                     !(s->tune & Tune::kGenericCombine);
    if ((s->tune & Tune::kNoInterior) && !(s->box == 15 && s->u8 && s->combine_reg)) {
        s->box = 0;  // the no-interior A/B arm only exists for these two variants
        s->combine_reg = false;
    }
    const size_t lds_sweep = lds_bytes(s, pm::kSweepTileH, !s->combine_reg, true);
    const size_t lds_dense = lds_bytes(s, pm::kDenseTileH, true, false);
    if (lds_sweep > 160u * 1024u || lds_dense > 160u * 1024u)  // 160 KiB of LDS per CU on gfx950
        return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "window x views needs more than 160 KiB of LDS per workgroup");
    if (!session_kernels(s, lds_sweep, lds_dense))
        return fail(GIPUMA_HIP_ERR_UNSUPPORTED, "no kernels for this window size and channel count");
    return 0;
}

// early termination of refinement evaluations (pm::multiview_cost): only where every view cost is
// provably finite and below MAXCOST for every plane, so that numValid == n_sel always
// (gipuma.cu:771-775): weights exp(-k/gamma) <= 1 from the table, dis <= (1-alpha)*tau_c + alpha*tau_g
// -- and the lower-bound prefilter of refinement candidates, which rides on it
int choose_early_termination(Session *s, const gipuma_hip_desc *d)
{
    const Experiments &x = s->exp;
    pm::Problem &hp = s->hp;
    const gipuma_hip_params &p = d->params;
    const double samples = (double)((hp.box_h + 1) / 2) * (double)((hp.box_v + 1) / 2);
    const bool sane = p.gamma > 0.0f && p.alpha >= 0.0f && p.alpha <= 1.0f && p.tau_color >= 0.0f &&
                      p.tau_gradient >= 0.0f && std::isfinite(p.tau_color) && std::isfinite(p.tau_gradient) &&
                      samples * ((1.0 - p.alpha) * p.tau_color + (double)p.alpha * p.tau_gradient) * 1.01 <
                          (double)GIPUMA_HIP_MAXCOST;
    // ... and only where a half-sweep is many waves of workgroups: on a frame whose tiles all fit the
    // GPU at once (< 1024 = 256 CUs x 4) the launch lasts as long as its slowest workgroup, and
    // the occasional redo pass of a bounded evaluation lengthens exactly that (configs A, B: -5..-13 %)
    const bool big = s->tiles >= 1024 || x.et_force.has_value();
    // (gray: the pipelined loop on float-encoded offsets; colour: its integer-addressed loop)
    hp.et_enable = sane && big && s->u8 && s->combine_reg && (s->ch == 4 || (hp.magic_addr && s->box > 0));
    if (hp.et_enable && x.et_force.value_or(0) >= 2) hp.et_enable = 2;
    hp.et_theta[0] = 1.0f;
    hp.et_theta[1] = 1.0f;
    // the two-phase refinement (compile-time box) redoes open candidates item by item, which
    // is cheap; the per-wavefront bound repeats the whole wavefront and wants a looser third bound
    const bool two_phase = s->box > 0 && !(s->tune & Tune::kNoTwoPhase);
    hp.et_theta[2] = two_phase ? 1.0f : 1.5f;
    if (x.tp_g0) hp.tp_g0 = *x.tp_g0;
    float theta[3];
    if (x.et_theta && sscanf(x.et_theta, "%f,%f,%f", &theta[0], &theta[1], &theta[2]) == 3) std::copy(theta, theta + 3, hp.et_theta);
    // lower-bound prefilter of refinement candidates: where the two-phase refinement runs on gray planes
    hp.lb_k = x.lb_k.value_or(0);  // 0: chosen by the probe workgroups
    if (hp.et_enable && s->box > 0 && hp.lb_k >= 0 && !(s->tune & (Tune::kNoTwoPhase | Tune::kNoEarlyExit))) {
        // (one plane of rows*cols words per two listed samples: 8 planes for box 15, 16 for box 25, 4 for box 11)
        const size_t lb_planes = s->k.lb_max / 2;
        if (const int rc = s->alloc_optional({{&s->worder, lb_planes * s->rows * s->cols * sizeof(uint32_t)}})) return rc;
        hp.worder = s->worder;
    }
    if (!s->worder) hp.lb_k = -1;
    return 0;
}

#ifndef PM_TILE_ORDER_DEFAULT
#define PM_TILE_ORDER_DEFAULT 0  // (the fused launches' dispatch order from the previous durations: off unless GIPUMA_HIP_TILE_ORDER=1)
#endif
// the schedule of a solve (gipuma_hip_schedule reports it; the launches only read it).  Push (pm_push.h) and plane-keyed
// (pm_group.h) propagation: 8-bit images, register combiner, packed planes -- gray ones with float-encoded offsets
int choose_schedule(Session *s, const gipuma_hip_desc *)
{
    const Experiments &x = s->exp;
    const bool propagate = s->k.push.fn && s->u8 && s->combine_reg && s->n_sel > 0 && (s->ch == 4 || s->hp.magic_addr) &&
                           !(s->tune & (Tune::kNoInterior | Tune::kNoSkip));
    // measured: config C 4 (5 and 6 level), config D 3 (4 level, 6 loses), config B 2 (+1 %), box 19 2 (2 / 3 / 4
    // -> 131.7 / 134.4 / 139.0 ms); colour (config C geometry): 3 where the plane-keyed kernel takes over afterwards (frames
    // of >= 1024 tiles: 2 / 3 / 4 / 6 pushed half-sweeps 195.5 / 195.7 / 197.7 / 205.9 ms per view), else 6 (4: -1.3 %,
    // 8: -0.7 %, 16: -7 %)
    s->push_launches = s->ch == 4 ? (s->tiles >= 1024 ? 3 : 6) : s->box == 15 ? 4 : s->box == 25 ? 3 : 2;
    s->push_launches = x.push_launches.value_or(s->push_launches);
    if (!propagate || s->push_launches < 0) s->push_launches = 0;
    // plane-keyed propagation after the pushed half-sweeps: from the fifth half-sweep on for box 15 (config C 90.6 -> 80.8 ms
    // per view in round 4; any start between the third and the fifth within 0.5 %), from the fourth for box 25 and colour,
    // from the third for box 19.  Box 11 and every frame under 1024 tiles (configs A and B; on config B's 300 tiles, one
    // wave of workgroups, it loses 1.5 %: scripts/history/gpu_r04_sched.sh) keep group_from = -1: their instantiations are
    // reached only through GIPUMA_HIP_GROUP_FROM=<first half-sweep> (< 0 = never) under GIPUMA_HIP_EXPERIMENTS, and are
    // parity-tested there.
    s->group_from = s->tiles < 1024 ? -1 : s->ch == 4 ? 3 : s->box == 15 ? 4 : s->box == 25 ? 3 : s->box == 19 ? 2 : -1;
    s->group_from = x.group_from.value_or(s->group_from);
    if (!propagate || !s->k.group.fn || s->group_from < 0) s->group_from = -1;
    // one launch per half-sweep (pm::sweep_group_kernel) where it exists, gray; colour: pm::group_kernel<15, 4> in front of
    // the sweep kernel.  GIPUMA_HIP_GROUP_FUSED=0: two launches in gray too
    s->group_fused = s->group_from >= 0 && s->k.fused.fn && x.group_fused.value_or(1) != 0;
    // column-per-lane evaluation (8-bit images, gray ones with float-encoded offsets) of random planes and, measured, of the
    // first four half-sweeps for box 15 (groups of 8 lanes, config C), three for box 25 (13 of 16 lanes, config D: 128.7 /
    // 90.9 / 73.7 -> 88.3 / 78.7 / 72.0 ms, the fourth loses) and two for box 19
    s->cols_ok = s->k.sweep_cols.fn && s->u8 && (s->ch == 4 || s->hp.magic_addr) &&
                 !(s->tune & (Tune::kNoColsKernel | Tune::kNoInterior));
    s->cols_launches = s->box == 25 ? 3 : s->box == 19 ? 2 : 4;
    if (x.cols_launches.value_or(-1) >= 0) s->cols_launches = *x.cols_launches;
    if (!s->cols_ok) s->cols_launches = 0;
    if (x.push_lds_kb) s->k.push.lds = std::max(s->k.push.lds, (size_t)*x.push_lds_kb * 1024);
    const size_t np = (size_t)s->rows * (size_t)s->cols, tiles = s->tiles;
    // performance-only state: without the memory for it the solve runs a plainer schedule, same results
    if (s->push_launches > 0 || s->group_from >= 0) {
        if (const int rc = s->alloc_optional({{&s->hp.push_cost.raw, 8 * np * sizeof(float)}})) return rc;
        if (!s->hp.push_cost) {  // every half-sweep evaluates its own propagation candidates
            s->push_launches = 0;
            s->group_from = -1;
            s->group_fused = false;
        }
    }
    if (s->push_launches > 0) HIP_OK(allow_lds(s->k.push));
    if (s->group_from >= 0) HIP_OK(s->group_fused ? allow_lds(s->k.fused) : allow_lds(s->k.group));
    // dispatch order of the fused launches (pm::tile_order_kernel; without the memory the plain order)
    const bool want = x.tile_order.value_or(PM_TILE_ORDER_DEFAULT) != 0;
    if (want && s->group_fused && tiles >= 8 && !(s->tune & Tune::kNoXcdRemap))
        return s->alloc_optional({{&s->hp.tile_clock.raw, 4 * tiles * sizeof(unsigned long long), 0}, {&s->hp.tile_order.raw, tiles * sizeof(int)}});
    return 0;
}

}  // namespace
