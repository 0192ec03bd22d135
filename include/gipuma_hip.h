/*
 * gipuma_hip.h -- C-ABI of the MI355X-native PatchMatch multi-view stereo hot path.
 *
 * This is the drop-in boundary for the one entry point of the reference's device path,
 *
 *     int runcuda(GlobalState &gs);            (reference gipuma.h:2, gipuma.cu:1962-1970)
 *
 * restated as a plain-C interface: POD structs, raw pointers and sizes, no C++/torch/OpenCV
 * types.  Every field below names the reference field it carries (file:line).  The adapter that
 * keeps the reference's C++ signature on top of this ABI lives in
 * gipuma_amd/csrc/adapter/ (see INTEGRATION.md).
 *
 * Conventions
 *   - 3x3 matrices are row-major float[9] (the reference stores them row-major in 16-float
 *     buffers, config.h:150-241 / cameraGeometryUtils.h:160-167).
 *   - images are row-major float32, one value per pixel (gray, channels == 1) holding 0..255
 *     (main.cpp:941), `pitch` elements per row; image 0 is the reference view (config.h:21).
 *   - state planes: norm4[y*cols+x] = (nx, ny, nz, d) with n.X + d = 0 in reference-camera
 *     coordinates (linestate.h:10); cost[y*cols+x] is the aggregated multi-view cost
 *     (linestate.h:11).  After gipuma_hip_finalize / gipuma_hip_run, norm4 holds
 *     (n_world.xyz, depth) exactly like gipuma_compute_disp leaves it (gipuma.cu:1080-1103).
 *   - all entry points return 0 on success or a negative gipuma_hip_status; they never exit
 *     the process (the reference's checkCudaErrors does, helper_cuda.h:890-905).
 */
#ifndef GIPUMA_HIP_H
#define GIPUMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIPUMA_HIP_ABI_VERSION 1
#define GIPUMA_HIP_MAX_VIEWS 32 /* float costVector[32], gipuma.cu:736 */
#define GIPUMA_HIP_MAXCOST 1000.0f /* config.h:22 */

typedef enum {
    GIPUMA_HIP_OK = 0,
    GIPUMA_HIP_ERR_ARG = -1,      /* malformed descriptor */
    GIPUMA_HIP_ERR_DEVICE = -2,   /* HIP runtime error (text in gipuma_hip_last_error) */
    GIPUMA_HIP_ERR_NO_DEVICE = -3,/* no gfx950 device / extension not usable */
    GIPUMA_HIP_ERR_UNSUPPORTED = -4
} gipuma_hip_status;

/* cost combination, algorithmparameters.h:17 */
enum { GIPUMA_COMB_ALL = 0, GIPUMA_COMB_BEST_N = 1, GIPUMA_COMB_ANGLE = 2, GIPUMA_COMB_GOOD = 3 };

/* stages of one checkerboard half-sweep (gipuma.cu:1915-1935) */
enum {
    GIPUMA_STAGE_CLOSE = 1,  /* gipuma_*_spatialPropClose_cu, gipuma.cu:1471-1588 */
    GIPUMA_STAGE_FAR = 2,    /* gipuma_*_spatialPropFar_cu,   gipuma.cu:1353-1468 */
    GIPUMA_STAGE_REFINE = 4, /* gipuma_*_planeRefine_cu,      gipuma.cu:1590-1711 */
    GIPUMA_STAGE_ALL = 7
};
enum { GIPUMA_BLACK = 0 /* (x+y) even, gipuma.cu:1730-1734 */, GIPUMA_RED = 1 };

/* One calibrated view.  Mirrors Camera_cu (camera.h:7-62) after getCameraParameters()
 * (cameraGeometryUtils.h:311-345) has re-expressed every pose relative to the reference
 * camera, so that for view 0:  R = I, t = 0. */
typedef struct gipuma_hip_camera {
    float K[9];          /* Camera_cu::K      (per-view intrinsics, cameraGeometryUtils.h:311) */
    float K_inv[9];      /* Camera_cu::K_inv  (used for the reference view only, gipuma.cu:605) */
    float R[9];          /* Camera_cu::R      (relative rotation) */
    float t[3];          /* Camera_cu::t4 */
    float M_inv[9];      /* Camera_cu::M_inv  = inverse of P'[:, :3]; reference view only */
    float P_col34[3];    /* Camera_cu::P_col34 = P'[:, 3];           reference view only */
    float C[3];          /* Camera_cu::C4 camera centre;             reference view only */
    float R_orig_inv[9]; /* Camera_cu::R_orig_inv, world<-camera;    reference view only (gipuma.cu:1095) */
    float fx, fy;        /* Camera_cu::fx, fy  (of K_0, cameraGeometryUtils.h:314-323) */
    float f;             /* CameraParameters_cu::f / Camera_cu::f */
    float alpha;         /* Camera_cu::alpha = fx / fy */
    float baseline;      /* Camera_cu::baseline (constant 0.54, cameraGeometryUtils.h:305) */
    float depth_min;     /* Camera_cu::depthMin (main.cpp:902) */
    float depth_max;     /* Camera_cu::depthMax (main.cpp:903) */
} gipuma_hip_camera;

/* The subset of AlgorithmParameters (algorithmparameters.h:52-84) the device path reads. */
typedef struct gipuma_hip_params {
    int32_t box_hsize;     /* odd, --blocksize= */
    int32_t box_vsize;
    int32_t iterations;
    int32_t n_best;
    int32_t cost_comb;     /* GIPUMA_COMB_* */
    float alpha;           /* cost_alpha */
    float tau_color;
    float tau_gradient;
    float gamma;
    float min_disparity;   /* = f*baseline/depth_max (main.cpp:905) */
    float max_disparity;   /* = f*baseline/depth_min (main.cpp:906) */
    float good_factor;
} gipuma_hip_params;

/* images[] are device pointers (already resident).  The planes must be COMPLETE when gipuma_hip_create / gipuma_hip_run is
 * called: the library reads them on its own stream (desc.stream, or a non-blocking one it creates), which does not wait for
 * the stream that wrote them -- synchronise that stream (or pass it as desc.stream) first.  A plane read half-written fails
 * the 8-bit test and sends the session down the float kernels: same results once the plane is complete, far slower. */
#define GIPUMA_HIP_FLAG_IMAGES_ON_DEVICE 1u
#define GIPUMA_HIP_FLAG_UNFUSED 2u          /* run close/far/refine as 3 launches like the reference */
/* With IMAGES_ON_DEVICE: the library may keep what it derives from an image plane (the 8-bit check and the
 * window-packed copy the kernels sample) in a process-wide cache keyed by the plane's device address and
 * geometry, and reuse it in later sessions -- a scan's images serve as source view of many reference
 * views (the reference re-uploads every image for every view, main.cpp:960-968).  The caller promises not
 * to change or free those planes before gipuma_hip_cache_clear(). */
#define GIPUMA_HIP_FLAG_CACHE_IMAGES 4u
/* Mode flag (SURVEY.md 8b "mode flags (bit-exact/fast)"): without it every result is bit-identical to the CPU restatement of
 * the stated numerical model (since round 6 correctly rounded x/z, y/z and unfused multiply-adds like the
 * reference's source; the model's bilinear taps).  With it the session runs the TOLERANCE-JUDGED flavour of the same kernels
 * -- the operation-order freedoms the reference takes by being built with --use_fast_math (CMakeLists.txt:23) and nvcc's
 * contraction: the numerical model of rounds 1-5 (x * (1/z) for x / z, fused multiply-adds in the sample loop) with the
 * hardware reciprocal without its correcting step, no proof that the window's denominators are in the exact reciprocal's
 * range, and the nine divisions by the plane offset in getHomography_cu (gipuma.cu:339-356) as one reciprocal and a Markstein
 * step each.  (Measured and rejected, compiled only by A/B builds: a host-folded homography, tree sums -- pm_core.h.)  Same
 * algorithm, schedule and random numbers; results are judged by the fraction of pixels inside 1e-4 relative depth / 1e-3
 * normal of the default mode's and of the reference's (tests/test_fast_mode.py, tests/test_headline_parity.py,
 * DESIGN.md 3a), not bit for bit. */
#define GIPUMA_HIP_FLAG_FAST 8u
/* Mode flag: the REFERENCE-ORDER flavour.  The per-sample arithmetic of the patch cost in the literal operation order of the
 * reference's source -- one bilinear fetch per tap at the coordinates gipuma.cu:251-253 writes, each with its own fraction;
 * correctly rounded x/z and y/z (config.h:44-47); unfused multiply-adds (config.h:150-162, gipuma.cu:272-274, 672).  Results
 * equal the reference's OWN device code (compiled for the CPU with fp32 texture-filter weights, oracle/_ref;
 * tests/golden/ref_*.npz) in every bit of every plane and cost -- up to BASELINE's headline frame (tests/test_headline_parity.py).
 * Since round 6 it runs through the same kernels and schedule as the default mode (packed 8-bit windows, push / column-per-lane
 * / plane-keyed propagation, bounded refinement): about 1.3x the default mode's time.  The default mode differs from it in the
 * taps only (one window, the centre tap's fractions, differences taken on the texels).  Gray and colour (T = float4: the
 * reference's float4 operators and l1_norm, vector_operations.h, gipuma.cu:174-179); excludes GIPUMA_HIP_FLAG_FAST. */
#define GIPUMA_HIP_FLAG_LITERAL 16u

/* Everything runcuda() reads out of GlobalState (globalstate.h:24-45). */
typedef struct gipuma_hip_desc {
    uint32_t abi_version;            /* GIPUMA_HIP_ABI_VERSION */
    int32_t rows, cols;              /* CameraParameters_cu::rows, cols */
    int32_t channels;                /* 1 = gray (T=float, one float per pixel); 4 = colour (T=float4: B, G, R, unused) */
    int32_t pitch;                   /* elements per image row (>= cols*channels) */
    int32_t n_images;                /* reference + source views handed over (<= 512, config.h:2) */
    const float *const *images;      /* GlobalState::imgs[] as linear buffers (no texture HW on gfx950) */
    const gipuma_hip_camera *cameras;/* n_images entries, CameraParameters_cu::cameras[] */
    int32_t n_selected;              /* CameraParameters_cu::viewSelectionSubsetNumber (<= 32) */
    const int32_t *selected;         /* CameraParameters_cu::viewSelectionSubset[], indices into images[] */
    gipuma_hip_params params;        /* GlobalState::params */
    uint32_t seed;                   /* solver seed (extension: the reference seeds from clock64(), gipuma.cu:1019) */
    int32_t device_id;               /* HIP device ordinal */
    void *stream;                    /* hipStream_t to launch on, NULL = the library's own stream */
    uint32_t flags;                  /* GIPUMA_HIP_FLAG_* */
} gipuma_hip_desc;

/* Device-side timings of the last gipuma_hip_run (hipEvent pairs on the launch stream). */
typedef struct gipuma_hip_timing {
    float ms_init;     /* gipuma_init_cu2 */
    float ms_sweeps;   /* all red/black launches (the reference's own timed region minus finalize) */
    float ms_finalize; /* gipuma_compute_disp */
    float ms_total;    /* init + sweeps + finalize */
    int32_t n_sweep_launches;
    float ms_sweep_avg; /* ms_sweeps / n_sweep_launches: the dominant kernel's mean launch time */
} gipuma_hip_timing;

typedef struct gipuma_hip_session gipuma_hip_session;

/* ---- library ---- */
int gipuma_hip_version(void);                 /* GIPUMA_HIP_ABI_VERSION of the built library */
const char *gipuma_hip_last_error(void);      /* thread-local text of the last failure */
int gipuma_hip_device_count(void);            /* usable HIP devices (0 if none) */
/* frees everything kept for GIPUMA_HIP_FLAG_CACHE_IMAGES.  Sessions that use a cached packed image hold a use
 * count on it: while one of them is alive the call frees nothing and returns GIPUMA_HIP_ERR_ARG. */
int gipuma_hip_cache_clear(void);

/* Device self-test of an arithmetic shortcut the kernels rely on: v_rcp_f32 + one Newton step must
 * equal the IEEE-correct 1.0f/z bit for bit for EVERY float with biased exponent 1..252.  Runs the
 * exhaustive comparison (2^32 inputs, ~1 s) on `device_id` and returns the number of mismatches in
 * that range through *mismatches (0 expected); the gpu tests call it. */
int gipuma_hip_selftest_reciprocal(int device_id, unsigned long long *mismatches);
/* The default and the reference-order flavour form x / z, y / z of the warped point (vecdiv4, /root/reference/config.h:44-47;
 * getCorrespondingPoint_cu, gipuma.cu:207-217) as  r = RN(1/z), q = RN(x r), q' = RN(q + RN(x - q z) r)  where the window's
 * operands are provably in range -- the correctly rounded IEEE quotient for every pair of fp32 significands.  This runs the
 * proof by exhaustion for the denominators with significand bits z_first .. z_first + z_count - 1 (of 2^23) against all 2^23
 * numerators and returns the number of pairs whose result differs from the IEEE division (0 expected; the whole range takes
 * about a minute on an MI355X: profiles/r06_selftest_quotient.txt; the gpu tests run a slice). */
int gipuma_hip_selftest_quotient(int device_id, unsigned z_first, unsigned z_count, unsigned long long *mismatches);

/* ---- session: the pieces of gipuma<T>() (gipuma.cu:1825-1960), one call per launch ---- */
/* validates the descriptor, uploads/binds images and cameras, allocates norm4/cost in HBM
 * (replaces gs.lines->resize, linestate.h:16-24, and the setup half of gipuma<T>(), :1840-1861) */
int gipuma_hip_create(const gipuma_hip_desc *desc, gipuma_hip_session **out);
int gipuma_hip_destroy(gipuma_hip_session *s);
/* random plane per pixel + its cost: gipuma_init_cu2<float>, gipuma.cu:996-1051, launch :1906 */
int gipuma_hip_init_planes(gipuma_hip_session *s);
/* one colour of one iteration: the launches at gipuma.cu:1915-1923 (black) / :1927-1935 (red).
 * `stages` is a mask of GIPUMA_STAGE_*; the stages run in the reference order close, far, refine. */
int gipuma_hip_sweep(gipuma_hip_session *s, int iteration, int colour, unsigned stages);
/* plane -> (world normal, depth): gipuma_compute_disp, gipuma.cu:1080-1103, launch :1944 */
int gipuma_hip_finalize(gipuma_hip_session *s);
/* multi-view cost of a GIVEN plane field (pmCostMultiview_cu, gipuma.cu:720-806; what the
 * unused gipuma_initial_cost kernel, :1052-1079, computes).  planes: rows*cols*4 host floats,
 * cost_out: rows*cols host floats. Does not touch the session state. */
int gipuma_hip_eval_cost(gipuma_hip_session *s, const float *planes_host, float *cost_out_host);
/* host copies of the state planes (blocking) */
int gipuma_hip_get_state(gipuma_hip_session *s, float *norm4_host, float *cost_host);
int gipuma_hip_set_state(gipuma_hip_session *s, const float *norm4_host, const float *cost_host);
/* device pointers of the state planes (for callers that keep results in HBM).  A caller that
 * WRITES the planes through these pointers must afterwards call
 * gipuma_hip_set_state(s, NULL, NULL): like any set_state it tells the session that the stored
 * costs are no longer known to be the costs of the stored planes and that its record of which
 * planes changed in the last half-sweeps is void (the sweep kernels skip candidates equal to a
 * pixel's own plane, and neighbours that did not change since the pixel last met them, only
 * while both are known). */
int gipuma_hip_state_device_ptrs(gipuma_hip_session *s, float **norm4_dev, float **cost_dev);
/* init + iterations x (black, red) + finalize on the session, timed with HIP events.
 * Does not synchronise the host unless `timing` is non-NULL. */
int gipuma_hip_solve(gipuma_hip_session *s, gipuma_hip_timing *timing);
/* Device time of every half-sweep (one colour of one iteration: the launches at gipuma.cu:1915-1923 or
 * :1927-1935) of the last gipuma_hip_solve that was given a `timing`, in launch order: up to `capacity`
 * values to ms_half_sweep, their number (2 x iterations) to *n_half_sweeps.  *n_pushed = how many leading
 * half-sweeps read their propagation costs from pm::push_kernel launches that are timed with them
 * (DESIGN.md 5); every later half-sweep is exactly one fused sweep launch.  (The reference times the whole loop
 * with one cudaEvent pair, gipuma.cu:1908-1952.)  Pointers may be NULL. */
int gipuma_hip_launch_times(gipuma_hip_session *s, float *ms_half_sweep, int capacity, int *n_half_sweeps,
                            int *n_pushed);
/* Of the same solve: per half-sweep the device time of the pm::group_kernel launch that evaluated its propagation
 * costs (0 where the half-sweep had none: the pushed ones and every half-sweep of a problem the kernel does not
 * serve), so that the fused sweep launch's own time is ms_half_sweep[i] - ms_group[i].  These launches replace the
 * cost evaluations of gipuma.cu:1437-1462 / :1571-1582.  Pointers may be NULL. */
int gipuma_hip_group_times(gipuma_hip_session *s, float *ms_group, int capacity, int *n_half_sweeps);
/* Which kernels a full solve of this session launches per half-sweep h = 2 * iteration + colour (performance only; the
 * results do not depend on it):  info[0] = half-sweeps h < info[0] read propagation costs pushed by pm::push_kernel;
 * info[1] = from half-sweep info[1] on the costs come from the plane-keyed evaluation (pm_group.h), -1: never;
 * info[2] = 1: that evaluation is fused with the sweep (one pm::sweep_group_kernel launch per half-sweep), 0: a
 * pm::group_kernel launch in front of the sweep launch;  info[3] = half-sweeps h < info[3] run the column-per-lane
 * sweep kernel, 0: none. */
int gipuma_hip_schedule(gipuma_hip_session *s, int info[4]);

/* ---- one-shot: the whole of runcuda() ---- */
/* norm4_out: rows*cols*4 host floats, cost_out: rows*cols host floats (either may be NULL).
 * Results are host-visible on return like the reference's managed memory after
 * cudaDeviceSynchronize (gipuma.cu:1945, main.cpp:976-985). */
int gipuma_hip_run(const gipuma_hip_desc *desc, float *norm4_out, float *cost_out,
                   gipuma_hip_timing *timing);

/* ---- a start from a known depth / normal map instead of random planes ----
 * The prior is a DEVICE buffer of prior_rows x prior_cols float4 in the public result form (n_world.xyz, depth) -- what
 * gipuma_hip_finalize leaves in norm4 and what disp.dmb + normals.dmb hold --, covering the frame at 1 / 2^shift of the
 * session's resolution (shift >= 0; depth is the camera-frame z, and R, C of the reference camera are the same on every
 * pyramid level, so neither needs rescaling between levels).  For pixel (x, y), in float32 without contraction:
 *     (nw, z) = prior[min(y >> shift, prior_rows - 1)][min(x >> shift, prior_cols - 1)]
 *     usable:  nw and z finite,  depth_min <= z <= depth_max of camera 0,  (nw.x nw.x + nw.y nw.y) + nw.z nw.z > 0
 *     plane = (n, d) with n = R_orig nw flipped towards the camera (vecOnHemisphere_cu, gipuma.cu:131-137) and d of the
 *             plane through the pixel's own ray at depth z (getD_cu, gipuma.cu:96-111); the normal is not renormalised
 *     not usable:  exactly the plane gipuma_hip_init_planes draws for (x, y) with the session's seed
 *     cost  = the multi-view cost of that plane
 * Afterwards the session is in the state gipuma_hip_init_planes leaves (costs known, hints and history cleared), so the
 * half-sweeps that follow run the session's schedule (gipuma_hip_schedule) like those of a plain solve.  A
 * finalize -> seed round trip at shift 0 returns the planes up to rounding, not in every bit.  The prior must be
 * COMPLETE when the call is made (as for the images: the session's stream does not wait for the stream that wrote it)
 * and must stay untouched until the seed has run; a session's own norm4 may seed it at shift 0 only.
 * Enqueues on the session's stream and does not synchronise. */
int gipuma_hip_seed_planes(gipuma_hip_session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift);
/* gipuma_hip_solve with gipuma_hip_seed_planes in place of the random initialisation: seed + the session's iterations x
 * (black, red) + finalize.  Half-sweeps are numbered from iteration 0, so the random draws of a pyramid level do not depend
 * on the levels below it.  iterations = 0 is legal and gives the finalized seed.  timing->ms_init is the seed's time.
 * Does not synchronise the host unless `timing` is non-NULL. */
int gipuma_hip_solve_seeded(gipuma_hip_session *s, const float *prior_dev, int prior_rows, int prior_cols, int shift,
                            gipuma_hip_timing *timing);

/* ---- one pyramid level of an image plane ----
 * Reduces the device plane rows x cols (pitch in floats, channels 1 or 4) to (rows >> 1) x (cols >> 1); a last odd row
 * or column is dropped.  Per channel
 *     out[Y][X] = floorf(((in[2Y][2X] + in[2Y][2X+1]) + (in[2Y+1][2X] + in[2Y+1][2X+1])) * 0.25f + 0.5f)
 * For integer-valued 0..255 planes every step is exact in fp32 and the output is integer-valued again: the coarse plane
 * passes the 8-bit test of gipuma_hip_create like its parent.  Coarse pixel X covers fine pixels 2X, 2X+1, so the camera
 * of the level is that of S P with S = [[1/2, 0, -1/4], [0, 1/2, -1/4], [0, 0, 1]] (gipuma_amd/pyramid.py
 * level_projection).  Runs on `stream` and does not synchronise; with stream == NULL it runs on the null stream and
 * returns when the plane is complete. */
int gipuma_hip_downsample(const float *src_dev, int rows, int cols, int pitch, int channels, float *dst_dev,
                          int dst_pitch, int device_id, void *stream);
/* (the name design documents use for it: the factor is part of the contract, not of the symbol) */
#define gipuma_hip_downsample2 gipuma_hip_downsample

/* ---- depth-map fusion: per-view (n_world, depth) planes -> one point cloud ----
 * The step the reference's scripts hand to an external tool after the per-view solves (scripts/dtu_fast.sh:23-26,
 * --disp_thresh / --normal_thresh / --num_consistent).  No parity with that tool is claimed; the contract is
 * DESIGN.md 11.  In short: views are taken in order i = 0..n_views-1; a pixel of view i with a valid depth that no
 * earlier view has marked is back-projected to X = c_i + z (bp_i (x, y, 1)); every other view j projects X with P_j,
 * rounds to the nearest pixel q and counts as consistent when q is inside, its depth z' is valid,
 * |fb_j / h_2 - fb_j / z'| < disp_thresh and n . n' > cos(normal_thresh).  With at least num_consistent such views
 * the mean of the points, the normalised sum of the normals and the rounded mean gray are emitted, and every
 * consistent q is marked in its view.  Points come out in (view, y, x) order, bit for bit reproducible. */
#define GIPUMA_HIP_FUSION_MAX_VIEWS 512 /* MAX_IMAGES, config.h:2 */

/* One view: device planes and float32 constants derived on the host in double from the view's own (not re-centred)
 * P = K [R | -R C], K scaled by cam_scale (gipuma_amd/cameras.py view_constants). */
typedef struct gipuma_hip_fusion_view {
    const float *norm4; /* device, rows*cols*4 floats (n_world.xyz, depth) as gipuma_hip_finalize leaves them */
    const float *gray;  /* device, rows*cols floats 0..255, or NULL (gray 0) */
    float bp[9];        /* R^T K^-1, row-major: world direction of pixel (x, y, 1) */
    float c[3];         /* camera centre C */
    float P[12];        /* [K R | -K R C], row-major 3x4 */
    float fb;           /* f32(f32(K[0][0]) * 0.54f): focal length x baseline (cameraGeometryUtils.h:103-107, :305) */
} gipuma_hip_fusion_view;

typedef struct gipuma_hip_fusion_desc {
    uint32_t abi_version;                /* GIPUMA_HIP_ABI_VERSION */
    int32_t rows, cols;                  /* of every view */
    int32_t n_views;                     /* 2 .. GIPUMA_HIP_FUSION_MAX_VIEWS */
    const gipuma_hip_fusion_view *views; /* host array of n_views entries */
    float disp_thresh;                   /* --disp_thresh, disparity units (pixels) */
    float normal_thresh;                 /* --normal_thresh, degrees; cos_t = f32(cos(normal_thresh * pi / 180)) in double */
    int32_t num_consistent;              /* --num_consistent, >= 1 */
    float depth_min, depth_max;          /* depths outside are invalid; <= 0: no bound */
    int32_t device_id;                   /* HIP device ordinal */
    void *stream;                        /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_fusion_desc;

typedef struct gipuma_hip_fusion gipuma_hip_fusion;

/* Runs the fusion and returns a handle that holds the points in device memory; blocks until they are complete.  The
 * planes must be complete when it is called (as for gipuma_hip_create). */
int gipuma_hip_fuse(const gipuma_hip_fusion_desc *desc, gipuma_hip_fusion **out);
/* total points, points emitted per view (n_views entries) and the device time of the fusion in ms (each may be NULL) */
int gipuma_hip_fusion_count(const gipuma_hip_fusion *f, int64_t *n_points, int64_t *per_view, float *device_ms);
/* points first .. first + count - 1 as binary PLY vertices of 27 bytes each: float x, y, z, nx, ny, nz (little
 * endian) and the gray byte three times (the vertex of storePlyFileBinary, displayUtils.h:78-159) */
int gipuma_hip_fusion_points(const gipuma_hip_fusion *f, void *vertices, int64_t first, int64_t count);
/* the final `used` marks: n_views * rows * cols bytes (0 / 1), view-major */
int gipuma_hip_fusion_used(const gipuma_hip_fusion *f, uint8_t *masks);
int gipuma_hip_fusion_free(gipuma_hip_fusion *f);

/* ---- the cross-view prior: solved (n_world, depth) maps of other cameras -> a start for a new reference view ----
 * Carries the result planes of n_sources already-solved views (1 .. GIPUMA_HIP_MAX_VIEWS, all rows x cols) into the
 * target camera, in the public result form gipuma_hip_seed_planes / gipuma_hip_solve_seeded take at shift 0.  The
 * reference has nothing like it; the contract is this project's own.  Float32 without contraction, valid(z) as in the
 * fusion (finite, > 0, inside depth_min / depth_max where those are > 0):
 *   splat:   every source pixel (x, y) of source k with valid depth z, a finite normal n with n.n > 0 and -- when cost
 *            planes are given -- cost <= max_cost is back-projected, X = c_k + z (bp_k (x, y, 1)), and projected with the
 *            target's P: h = P_t (X, 1).  It is kept when h_2 > 0 and valid(h_2), its nearest pixel
 *            q = floor(h_0 / h_2 + 0.5, h_1 / h_2 + 0.5) is inside the frame and its plane faces the target camera,
 *            n . (bp_t (q, 1)) < 0.  Then  zbuf[q] = min(zbuf[q], bits(h_2) << 32 | k rows cols + y cols + x)  as one
 *            64-bit unsigned atomic minimum: the nearest surface wins, a tie goes to the lower source ordinal, then to
 *            the lower source pixel -- whatever the launch geometry and the order the workgroups run in.
 *   resolve: a target pixel takes its own key (class `direct`) or, when it has none and fill = 1, the smallest key of
 *            its 8 neighbours inside the frame (class `filled`).  The winner's plane is intersected with the pixel's OWN
 *            ray r = bp_t (x, y, 1):  zc = n . (X - c_t) / n . r  (the depth a nearest-pixel splat loses 2-3e-4 of).
 *            zc is used when it is valid and the ray is not grazing, (n . r)^2 > grazing_cos^2 (n . n)(r . r); otherwise
 *            a direct pixel keeps the splatted depth h_2 and a filled one becomes empty.  prior = (n, depth); an
 *            `empty` pixel is (0, 0, 0, 0), which gipuma_hip_seed_planes answers with the random plane of
 *            gipuma_hip_init_planes.
 * target: bp, c and P are read (norm4, gray, fb are not); sources: norm4, bp and c.  The constants are those of
 * gipuma_amd/cameras.py view_constants.  costs: NULL, or a host array of n_sources device planes of rows * cols floats.
 * A frame may have at most 2^30 pixels (pixel indices are int; more is GIPUMA_HIP_ERR_ARG, as in the fusion); within
 * that, n_sources * rows * cols >= 2^32 is refused with GIPUMA_HIP_ERR_UNSUPPORTED (the key's low word). */
typedef struct gipuma_hip_prior_desc {
    uint32_t abi_version;                  /* GIPUMA_HIP_ABI_VERSION */
    int32_t rows, cols;                    /* of every view */
    gipuma_hip_fusion_view target;         /* the new reference camera */
    int32_t n_sources;                     /* 1 .. GIPUMA_HIP_MAX_VIEWS */
    const gipuma_hip_fusion_view *sources; /* host array of n_sources entries, device planes */
    const float *const *costs;             /* NULL, or host array of n_sources device cost planes */
    float max_cost;                        /* with costs: source pixels with cost > max_cost are left out */
    float depth_min, depth_max;            /* depths outside are invalid; <= 0: no bound */
    float grazing_cos;                     /* 0 .. 1; f32(cos(80 degrees)) computed in double is the usual value */
    int32_t fill;                          /* 1: empty pixels look at their 8 neighbours; 0: they stay empty */
    int32_t device_id;                     /* HIP device ordinal */
    void *stream;                          /* hipStream_t to enqueue on; NULL = the null stream, complete on return */
} gipuma_hip_prior_desc;

/* Writes rows * cols float4 to the caller's device buffer prior_dev.  Enqueues on desc->stream and synchronises only
 * when `counts` (the number of direct, filled and empty pixels) or `device_ms` (memset + both kernels, HIP events) is
 * asked for; either may be NULL.  The source planes must be complete on that stream's terms when the call is made.
 * Scratch: the 8-byte-per-pixel key plane is cached per device (grown when a larger frame comes, kept until the process
 * ends) and shared by every call on that device, so two calls on one device must not run side by side: keep them on
 * one stream, or let the first finish. */
int gipuma_hip_prior_from_views(const gipuma_hip_prior_desc *desc, float *prior_dev, int64_t counts[3], float *device_ms);

/* ---- nearest neighbours between two point clouds: the search behind the cloud score ----
 * For every query a_i (n_queries packed float32 xyz) the nearest target b_j (n_targets packed xyz) within max_dist.
 * Float32 without contraction, r2 = max_dist * max_dist:
 *     dx = a_i.x - b_j.x;  dy = a_i.y - b_j.y;  dz = a_i.z - b_j.z;  d2 = (dx*dx + dy*dy) + dz*dz
 *     j is a candidate  iff  b_j is finite in all three coordinates  and  d2 is finite  and  d2 <= r2   (the radius is
 *                            inclusive)
 *     d2_dev[i]  = the minimum of d2 over the candidates;  idx_dev[i] = the lowest j that attains it
 *     no candidate, or a_i not finite:  d2_dev[i] = +inf,  idx_dev[i] = -1
 * +inf means "none" and nothing else: a d2 that overflows is no candidate even where r2 = +inf (max_dist above 1.8e19).
 * A minimum and a lowest index do not depend on the order of the candidates: the result is defined without reference
 * to the uniform grid the kernels search with, and it equals a brute-force search in every bit (tests/cloud_ref.py).
 * The grid -- one cell edge on all axes, `grid` cells along the longest axis of the finite targets' bounding box --
 * changes the time only; 0 lets the library choose it from n_targets, ceil(sqrt(n_targets / 2)) capped at 256.
 * n_queries = 0 writes nothing; n_targets = 0 answers "none" everywhere.  Blocks until the result is complete; the
 * clouds must be complete on desc->stream's terms when the call is made.  Scratch (about 20 bytes per point and 8 per
 * cell) is allocated for the call and freed before it returns, on every error path too. */
typedef struct gipuma_hip_cloud_desc {
    uint32_t abi_version;           /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_queries, n_targets;   /* each < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *queries, *targets; /* device pointers, packed xyz float32 */
    float max_dist;                 /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    int32_t grid;                   /* 0: automatic; 1..256: cells along the longest axis */
    int32_t device_id;              /* HIP device ordinal */
    void *stream;                   /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_cloud_desc;

/* d2_dev, idx_dev: n_queries entries each, device.  counts (queries that found a neighbour, queries that did not) and
 * device_ms (HIP events around the launches) may be NULL. */
int gipuma_hip_cloud_nearest(const gipuma_hip_cloud_desc *desc, float *d2_dev, int32_t *idx_dev, int64_t counts[2],
                             float *device_ms);
/* What the calling thread's last gipuma_hip_cloud_nearest did: the cells along the longest axis, the cells along x, y
 * and z, the queries answered "none" without a search (farther than max_dist from the targets' bounding box) and the
 * queries searched.  All 0 after a call that had no finite target or no query. */
int gipuma_hip_cloud_last_stats(int64_t stats[6]);

/* ---- thinning a cloud to a minimum point spacing: the density normalisation before the score ----
 * P: n_points packed float32 xyz.  d2(i, j) is gipuma_hip_cloud_nearest's, float32 without contraction, and bitwise
 * symmetric in i, j (negation is exact); r2 = radius * radius in float32; the radius is inclusive.
 *     key(i) = (prio(i), i), compared lexicographically, lower first
 *     order 0 (hashed): prio(i) = mix32(mix32(seed + 0x9E3779B9u) ^ ((uint32_t)i + 0x85EBCA6Bu)), uint32 wrap-around,
 *                       mix32(h): h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16
 *     order 1 (index):  prio(i) = 0 -- the caller's own order
 *     a point that is not finite in all three coordinates is never kept and never suppresses another point
 *     the finite points are visited in ascending key;  i is KEPT  iff  no point kept before it has d2(i, j) <= r2
 *     keep_dev[i] = 1 for a kept point, 0 for any other
 * This is the lexicographically first maximal independent set of the radius graph: kept points are pairwise d2 > r2,
 * every finite dropped point has a kept point of lower key within the radius, and the mask is a pure function of
 * (P, radius, seed, order) -- defined without reference to the grid or to the rounds the kernels decide it in, and equal
 * to the sequential pass in every byte (tests/thin_ref.py).  `grid` (cells along the longest axis of the finite points'
 * box) changes the time only; 0 lets the library choose a cell edge of about the radius, at most 256 cells.
 * n_points = 0 writes nothing and reports 0 rounds.  Blocks until the mask is complete; the cloud must be complete on
 * desc->stream's terms when the call is made.  Scratch (about 32 bytes per point and 4 per cell) is allocated for the
 * call and freed before it returns, on every error path too. */
typedef struct gipuma_hip_thin_desc {
    uint32_t abi_version; /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_points;     /* < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *points;  /* device pointer, packed xyz float32 */
    float radius;         /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    uint32_t seed;        /* of the hashed order */
    int32_t order;        /* 0: hashed, 1: index */
    int32_t grid;         /* 0: automatic; 1..256: cells along the longest axis */
    int32_t device_id;    /* HIP device ordinal */
    void *stream;         /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_thin_desc;

/* keep_dev: n_points bytes, device.  info (points kept, finite points dropped, points not finite, rounds, cells along the
 * longest axis, cells along x, y and z) and device_ms (HIP events around everything the call enqueues, the host's reads
 * of the per-round survivor count included) may be NULL. */
int gipuma_hip_cloud_thin(const gipuma_hip_thin_desc *desc, uint8_t *keep_dev, int64_t info[8], float *device_ms);

/* ---- counting a point's neighbours within a radius: dropping the isolated points of a cloud ----
 * P: n_points packed float32 xyz.  d2(i, j) and r2 = radius * radius are the thinning's, float32 without contraction;
 * the neighbour relation is the thinning's radius graph, plain d2 <= r2, inclusive (inf <= inf holds where r2 = +inf).
 *     P_i not finite in all three coordinates:  count(i) = 0, keep(i) = 0 -- never kept, never counted by another point
 *     otherwise:  exact(i) = the number of j != i with P_j finite and d2(i, j) <= r2   (j != i by index: an exact copy
 *                            of P_i is a neighbour)
 *                 count(i) = max_count > 0 ? min(exact(i), max_count) : exact(i)
 *                 keep(i)  = count(i) >= min_neighbours
 * min_neighbours <= max_count is required where max_count > 0, so that saturation never changes keep; it lets a point in
 * a dense region stop counting early.  A count is the cardinality of a set: it is defined without reference to the grid or
 * to the order the kernel visits the points in, and equal to a brute force in every bit (tests/neighbours_ref.py); d2 is
 * bitwise symmetric, so exact counts sum to an even number.  `grid` is the thinning's and changes the time only; 0 lets
 * the library choose a cell edge of about the radius, at most 256 cells.
 * n_points = 0 writes nothing.  Blocks until the outputs are complete; the cloud must be complete on desc->stream's
 * terms when the call is made.  Scratch (about 20 bytes per point and 4 per cell) is allocated for the call and freed
 * before it returns, on every error path too. */
typedef struct gipuma_hip_neighbours_desc {
    uint32_t abi_version;   /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_points;       /* < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *points;    /* device pointer, packed xyz float32 */
    float radius;           /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    int32_t min_neighbours; /* >= 0 */
    int32_t max_count;      /* 0: exact counts; > 0: counts saturate there, and min_neighbours <= max_count */
    int32_t grid;           /* 0: automatic; 1..256: cells along the longest axis */
    int32_t device_id;      /* HIP device ordinal */
    void *stream;           /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_neighbours_desc;

/* count_dev: n_points uint32, device; keep_dev: n_points bytes, device.  Either may be NULL, not both where n_points > 0
 * (GIPUMA_HIP_ERR_ARG).  info (points kept, finite points dropped, points not finite, points whose count reached a
 * max_count > 0, cells along the longest axis, cells along x, y and z) and device_ms (HIP events around everything the
 * call enqueues) may be NULL. */
int gipuma_hip_cloud_neighbours(const gipuma_hip_neighbours_desc *desc, uint32_t *count_dev, uint8_t *keep_dev,
                                int64_t info[8], float *device_ms);

/* ---- the k nearest neighbours of every point inside its own cloud, and their mean distance: statistical outlier removal
 *  ----
 * P: n_points packed float32 xyz.  d2(i, j) and r2 = radius * radius are the thinning's, float32 without contraction; the
 * neighbour relation is the neighbour count's: plain d2 <= r2, inclusive, j != i by index, so an exact copy is a neighbour.
 *     P_i not finite in all three coordinates:  m(i) = 0, every slot (+inf, -1), mean(i) = +inf -- and no point lists i
 *     otherwise:  N(i)    = { j != i : P_j finite and d2(i, j) <= r2 }
 *                 list(i) = the min(k, |N(i)|) smallest pairs (d2(i, j), j) of N(i) in lexicographic order, ascending
 *                 m(i)    = min(k, |N(i)|)
 *                 d2_dev[i*k + s], idx_dev[i*k + s] = list(i)[s] for s < m(i);  (+inf, -1) for m(i) <= s < k
 *                 count_dev[i] = m(i)
 *                 mean_dev[i]  = m(i) == k ? (((sqrt(d2_0) + sqrt(d2_1)) + ...) + sqrt(d2_{k-1})) / (float)k : +inf
 * The sum is float32, in ascending slot order, starting from 0; every sqrt and the division are correctly rounded float32
 * (what numpy's float32 sqrt, + and / do).  The k smallest of a set of distinct pairs, sorted, do not depend on the order
 * the kernel visits the points in or on the grid: all four outputs equal a brute force in every bit, run after run
 * (tests/knn_ref.py).  m(i) == k is the neighbour count's keep(i) with min_neighbours = k.
 * Where r2 = +inf (radius above 1.8e19) inf <= inf holds, as in the thinning: a finite P_j whose d2 overflows is a neighbour.
 * A slot with d2 = +inf and idx >= 0 is such a neighbour -- it is filled, it counts in m(i), it sorts behind every finite d2
 * by its index, and a list that holds one has mean = +inf although m(i) == k.  An EMPTY slot is the one with idx = -1.
 * `grid` is the thinning's and changes the time only.  n_points = 0 writes nothing.  Blocks until the outputs are
 * complete; the cloud must be complete on desc->stream's terms when the call is made.  Scratch (about 20 bytes per point
 * and 4 per cell) is allocated for the call and freed before it returns, on every error path too. */
typedef struct gipuma_hip_knn_desc {
    uint32_t abi_version; /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_points;     /* < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *points;  /* device pointer, packed xyz float32 */
    float radius;         /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    int32_t k;            /* 1..32, else GIPUMA_HIP_ERR_ARG */
    int32_t grid;         /* 0: automatic; 1..256: cells along the longest axis */
    int32_t device_id;    /* HIP device ordinal */
    void *stream;         /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_knn_desc;

/* d2_dev, idx_dev: n_points * k entries each, device; count_dev (uint32), mean_dev: n_points entries each, device.  Each may
 * be NULL, not all four where n_points > 0 (GIPUMA_HIP_ERR_ARG); with d2_dev or idx_dev given, n_points * k must be below
 * 2^31 (GIPUMA_HIP_ERR_UNSUPPORTED).  info (points with a complete list, m == k; finite points with a short one; points not
 * finite; 0; cells along the longest axis, cells along x, y and z) and device_ms (HIP events around everything the call
 * enqueues) may be NULL. */
int gipuma_hip_cloud_knn(const gipuma_hip_knn_desc *desc, float *d2_dev, int32_t *idx_dev, uint32_t *count_dev,
                         float *mean_dev, int64_t info[8], float *device_ms);

/* ---- the connected components of a cloud's radius graph: dropping its small clumps ----
 * P: n_points packed float32 xyz.  d2(i, j) and r2 = radius * radius are the thinning's, float32 without contraction; the
 * edge relation is the neighbour count's radius graph: i ~ j iff i != j by index, both points are finite and d2(i, j) <= r2
 * (inclusive; inf <= inf holds where r2 = +inf; an exact copy is a neighbour).  d2 is bitwise symmetric, so is the relation.
 *     P_i not finite in all three coordinates:  label(i) = -1, size(i) = 0, keep(i) = 0 -- and no component contains i
 *     otherwise:  C(i)     = the connected component of i in the radius graph over the finite points
 *                 label(i) = min { j : j in C(i) }     (the caller's index)
 *                 size(i)  = |C(i)|
 *                 keep(i)  = size(i) >= min_size
 * A component's smallest index and its cardinality are defined without reference to the grid, to the order the kernels
 * visit the points in or to how their concurrent unions interleave: all three outputs equal a sequential union-find over
 * a brute-force edge list in every byte, run after run (tests/components_ref.py).  `grid` is the thinning's and changes the
 * time only.  n_points = 0 writes nothing.  Blocks until the outputs are complete; the cloud must be complete on
 * desc->stream's terms when the call is made.  Scratch (about 36 bytes per point and 4 per cell, 16 of them on top of the
 * neighbour count's) is allocated for the call and freed before it returns, on every error path too. */
typedef struct gipuma_hip_components_desc {
    uint32_t abi_version; /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_points;     /* < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *points;  /* device pointer, packed xyz float32 */
    float radius;         /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    int32_t min_size;     /* >= 0, else GIPUMA_HIP_ERR_ARG */
    int32_t grid;         /* 0: automatic; 1..256: cells along the longest axis */
    int32_t device_id;    /* HIP device ordinal */
    void *stream;         /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_components_desc;

/* label_dev: n_points int32, device; size_dev: n_points uint32, device; keep_dev: n_points bytes, device.  Each may be NULL,
 * not all three where n_points > 0 (GIPUMA_HIP_ERR_ARG).  info (points kept, finite points dropped -- in a component below
 * min_size --, points not finite, components, cells along the longest axis, cells along x, y and z) and device_ms (HIP
 * events around everything the call enqueues) may be NULL. */
int gipuma_hip_cloud_components(const gipuma_hip_components_desc *desc, int32_t *label_dev, uint32_t *size_dev,
                                uint8_t *keep_dev, int64_t info[8], float *device_ms);

/* ---- a cloud's normals and surface variation from its k nearest neighbours ----
 * P: n_points packed float32 xyz.  list(i) and m(i) are gipuma_hip_cloud_knn's: the min(k, |N(i)|) nearest other finite points of
 * i within the radius, ascending in (d2, j), the same relation, ordering and treatment of copies.
 *     P_i not finite, or m(i) < 3 ("short"):  normal(i) = (0, 0, 0), variation(i) = +inf, the six entries of C are 0
 *     otherwise, M = m(i) + 1 (the point itself counts, at d = 0):
 *         d_s = P_list(i)[s] - P_i per coordinate in float32, then widened to float64               (s ascending)
 *         S1 = sum_s d_s,  S2 = sum_s d_s d_s^T       (float64, in slot order, from 0; each product is exact in a double)
 *         C  = M * S2 - S1 S1^T                       (float64, M^2 times the covariance; upper triangle C00 C01 C02 C11 C12 C22)
 *         trace = (C00 + C11) + C22 <= 0 or not finite ("degenerate": all copies, or overflow): the short values; C is written
 *         (w, V) = cyclic Jacobi on C in float64, V from the identity: SIX sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r
 *             the third index; a pair whose a_pq is exactly 0 is skipped; else theta = (a_qq - a_pp) / (2 a_pq),
 *             t = sgn(theta) / (|theta| + sqrt(theta theta + 1)) with sgn(0) = +1, c = 1 / sqrt(t t + 1), s = t c, h = t a_pq, then
 *             a_pp -= h; a_qq += h; a_pq = 0; (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq); and for the rows i = 0, 1, 2 of V
 *             (v_ip, v_iq) = (c v_ip - s v_iq, s v_ip + c v_iq) -- every right-hand side from the values before the rotation
 *         e = the index of the smallest w = (a_00, a_11, a_22), the lowest index on a tie
 *         normal(i)    = float32 of column e of V, negated where the sign rule says so
 *         variation(i) = float32((w_e > 0 ? w_e : 0) / ((w_0 + w_1) + w_2))
 * The sign rule, on the float32 normal n widened to float64: orient 1: dot = (n_0 (v_0 - p_0) + n_1 (v_1 - p_1)) + n_2 (v_2 - p_2)
 * with the viewpoint v and p = P_i; orient 2: dot = (n_0 g_0 + n_1 g_1) + n_2 g_2 with g = guide[i]; negate iff dot < 0.  orient
 * 0, and where the dot is 0 or not finite: negate iff the component of largest magnitude -- the lowest axis on a tie -- is < 0.
 * Every + - * / sqrt is correctly rounded float64 without contraction (what numpy float64 does): all outputs equal the
 * restatement (tests/normals_ref.py) in every bit, at every grid, run after run.  A NaN entry of C is written as 0x7ff8000000000000.
 * `grid` is the thinning's and changes the time only.  n_points = 0 writes nothing.  Blocks until the outputs are complete; the
 * cloud (and the guide) must be complete on desc->stream's terms when the call is made.  Scratch (about 20 bytes per point and 4
 * per cell) is allocated for the call and freed before it returns, on every error path too. */
typedef struct gipuma_hip_normals_desc {
    uint32_t abi_version; /* GIPUMA_HIP_ABI_VERSION */
    int64_t n_points;     /* < 2^31; more: GIPUMA_HIP_ERR_UNSUPPORTED */
    const float *points;  /* device pointer, packed xyz float32 */
    float radius;         /* > 0 and finite, else GIPUMA_HIP_ERR_ARG */
    int32_t k;            /* 3..32, else GIPUMA_HIP_ERR_ARG */
    int32_t grid;         /* 0: automatic; 1..256: cells along the longest axis */
    int32_t orient;       /* 0: largest component positive; 1: towards viewpoint; 2: along guide; else GIPUMA_HIP_ERR_ARG */
    float viewpoint[3];   /* orient 1: finite, else GIPUMA_HIP_ERR_ARG; otherwise not read */
    const float *guide;   /* orient 2: device pointer, n_points packed float32 normals, NULL: GIPUMA_HIP_ERR_ARG; otherwise not read */
    int32_t device_id;    /* HIP device ordinal */
    void *stream;         /* hipStream_t to launch on, NULL = one the library creates for the call */
} gipuma_hip_normals_desc;

/* normal_dev: 3 * n_points float32, device; variation_dev: n_points float32; count_dev: n_points uint32, m(i); scatter_dev:
 * 6 * n_points float64, the upper triangle of C.  Each may be NULL, not all four where n_points > 0 (GIPUMA_HIP_ERR_ARG).
 * info (points estimated; finite points short or degenerate; points not finite; estimated points whose normal was negated; cells
 * along the longest axis, cells along x, y and z) and device_ms (HIP events around everything the call enqueues) may be NULL. */
int gipuma_hip_cloud_normals(const gipuma_hip_normals_desc *desc, float *normal_dev, float *variation_dev, uint32_t *count_dev,
                             double *scatter_dev, int64_t info[8], float *device_ms);

#ifdef __cplusplus
}
#endif
#endif /* GIPUMA_HIP_H */
