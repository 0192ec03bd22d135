"""ctypes mirror of include/gipuma_hip.h and the loader of the HIP library.

The HIP library (gipuma_amd/csrc/libgipuma_hip.so, built by ``__graft_entry__.build()``) is the
only compute path of this package.  There is no CPU fallback: if the library is missing or no
MI355X is visible, calls raise ``GipumaHipError``.
"""
import ctypes as C
import os

ABI_VERSION = 1
MAX_VIEWS = 32
MAXCOST = 1000.0
ERR_ARG, ERR_DEVICE, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -2, -3, -4  # gipuma_hip_status

COMB_ALL, COMB_BEST_N, COMB_ANGLE, COMB_GOOD = 0, 1, 2, 3
STAGE_CLOSE, STAGE_FAR, STAGE_REFINE, STAGE_ALL = 1, 2, 4, 7
BLACK, RED = 0, 1
FLAG_IMAGES_ON_DEVICE = 1
FLAG_UNFUSED = 2
FLAG_CACHE_IMAGES = 4
FLAG_FAST = 8  # tolerance-judged flavour of the kernels (include/gipuma_hip.h); default: bit-exact
FLAG_LITERAL = 16  # reference-order flavour: bit-identical to the reference's own code (fp32 filter model); slow

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgipuma_hip.so")


class GipumaHipError(RuntimeError):
    pass


class Camera(C.Structure):
    """gipuma_hip_camera == the used part of Camera_cu (reference camera.h:7-62)."""
    _fields_ = [
        ("K", C.c_float * 9), ("K_inv", C.c_float * 9), ("R", C.c_float * 9),
        ("t", C.c_float * 3), ("M_inv", C.c_float * 9), ("P_col34", C.c_float * 3),
        ("C", C.c_float * 3), ("R_orig_inv", C.c_float * 9),
        ("fx", C.c_float), ("fy", C.c_float), ("f", C.c_float), ("alpha", C.c_float),
        ("baseline", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float),
    ]


class Params(C.Structure):
    """gipuma_hip_params == the device-read part of AlgorithmParameters
    (reference algorithmparameters.h:52-84)."""
    _fields_ = [
        ("box_hsize", C.c_int32), ("box_vsize", C.c_int32), ("iterations", C.c_int32),
        ("n_best", C.c_int32), ("cost_comb", C.c_int32),
        ("alpha", C.c_float), ("tau_color", C.c_float), ("tau_gradient", C.c_float),
        ("gamma", C.c_float), ("min_disparity", C.c_float), ("max_disparity", C.c_float),
        ("good_factor", C.c_float),
    ]


class Desc(C.Structure):
    """gipuma_hip_desc == what runcuda() reads out of GlobalState (reference globalstate.h:24-45)."""
    _fields_ = [
        ("abi_version", C.c_uint32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("channels", C.c_int32), ("pitch", C.c_int32), ("n_images", C.c_int32),
        ("images", C.POINTER(C.c_void_p)), ("cameras", C.POINTER(Camera)),
        ("n_selected", C.c_int32), ("selected", C.POINTER(C.c_int32)),
        ("params", Params), ("seed", C.c_uint32), ("device_id", C.c_int32),
        ("stream", C.c_void_p), ("flags", C.c_uint32),
    ]


class Timing(C.Structure):
    _fields_ = [
        ("ms_init", C.c_float), ("ms_sweeps", C.c_float), ("ms_finalize", C.c_float),
        ("ms_total", C.c_float), ("n_sweep_launches", C.c_int32), ("ms_sweep_avg", C.c_float),
    ]


FUSION_MAX_VIEWS = 512  # GIPUMA_HIP_FUSION_MAX_VIEWS (MAX_IMAGES, config.h:2)


class FusionView(C.Structure):
    """gipuma_hip_fusion_view: one view's device planes and float32 camera constants (gipuma_amd.cameras.view_constants)"""
    _fields_ = [
        ("norm4", C.c_void_p), ("gray", C.c_void_p), ("bp", C.c_float * 9), ("c", C.c_float * 3),
        ("P", C.c_float * 12), ("fb", C.c_float),
    ]


def fill_view(v, k, norm4=None, gray=None):
    """fills the FusionView `v` from k = cameras.view_constants(P, cam_scale) and the device addresses of its planes"""
    v.norm4, v.gray = norm4, gray
    v.bp[:] = [float(x) for x in k["bp"].reshape(-1)]
    v.c[:] = [float(x) for x in k["c"]]
    v.P[:] = [float(x) for x in k["P"].reshape(-1)]
    v.fb = float(k["fb"])


def device_plane(a, device, keep):
    """The device address of the float32 plane `a` on `device`: a device tensor is passed through (no copy), a host array
    uploaded.  `keep`: the caller's list that holds the tensor alive for as long as the library may read it."""
    import numpy as np
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    keep.append(t)
    return t.data_ptr()


class FusionDesc(C.Structure):
    """gipuma_hip_fusion_desc: views, size and the fusion parameters (--disp_thresh, --normal_thresh, --num_consistent)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("rows", C.c_int32), ("cols", C.c_int32), ("n_views", C.c_int32),
        ("views", C.POINTER(FusionView)), ("disp_thresh", C.c_float), ("normal_thresh", C.c_float),
        ("num_consistent", C.c_int32), ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


class PriorDesc(C.Structure):
    """gipuma_hip_prior_desc: the target camera, the solved source views and the knobs of the cross-view prior"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("rows", C.c_int32), ("cols", C.c_int32), ("target", FusionView),
        ("n_sources", C.c_int32), ("sources", C.POINTER(FusionView)), ("costs", C.POINTER(C.c_void_p)),
        ("max_cost", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float), ("grazing_cos", C.c_float),
        ("fill", C.c_int32), ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


class CloudDesc(C.Structure):
    """gipuma_hip_cloud_desc: two device clouds of packed float32 xyz, the search radius and the grid (0: automatic)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_queries", C.c_int64), ("n_targets", C.c_int64), ("queries", C.c_void_p),
        ("targets", C.c_void_p), ("max_dist", C.c_float), ("grid", C.c_int32), ("device_id", C.c_int32),
        ("stream", C.c_void_p),
    ]


class ThinDesc(C.Structure):
    """gipuma_hip_thin_desc: one device cloud of packed float32 xyz, the minimum spacing, the order's seed and kind (0
    hashed, 1 index) and the grid (0: automatic)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("points", C.c_void_p), ("radius", C.c_float),
        ("seed", C.c_uint32), ("order", C.c_int32), ("grid", C.c_int32), ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


class NeighboursDesc(C.Structure):
    """gipuma_hip_neighbours_desc: one device cloud of packed float32 xyz, the radius, the count a point needs to be kept,
    the count at which counting stops (0: never) and the grid (0: automatic)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("points", C.c_void_p), ("radius", C.c_float),
        ("min_neighbours", C.c_int32), ("max_count", C.c_int32), ("grid", C.c_int32), ("device_id", C.c_int32),
        ("stream", C.c_void_p),
    ]


class ComponentsDesc(C.Structure):
    """gipuma_hip_components_desc: one device cloud of packed float32 xyz, the radius of the edge relation, the size a
    component needs for its points to be kept and the grid (0: automatic)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("points", C.c_void_p), ("radius", C.c_float),
        ("min_size", C.c_int32), ("grid", C.c_int32), ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


class KnnDesc(C.Structure):
    """gipuma_hip_knn_desc: one device cloud of packed float32 xyz, the radius, the list length k (1..32) and the grid (0:
    automatic)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("points", C.c_void_p), ("radius", C.c_float),
        ("k", C.c_int32), ("grid", C.c_int32), ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


class NormalsDesc(C.Structure):
    """gipuma_hip_normals_desc: one device cloud of packed float32 xyz, the radius, the list length k (3..32), the grid (0:
    automatic), the sign rule (0 largest component, 1 viewpoint, 2 guide) with its viewpoint and guide normals"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("points", C.c_void_p), ("radius", C.c_float),
        ("k", C.c_int32), ("grid", C.c_int32), ("orient", C.c_int32), ("viewpoint", C.c_float * 3), ("guide", C.c_void_p),
        ("device_id", C.c_int32), ("stream", C.c_void_p),
    ]


# every symbol include/gipuma_hip.h declares: (name, restype, argtypes)
_FP = C.POINTER(C.c_float)
SYMBOLS = [
    ("gipuma_hip_version", C.c_int, []),
    ("gipuma_hip_last_error", C.c_char_p, []),
    ("gipuma_hip_device_count", C.c_int, []),
    ("gipuma_hip_cache_clear", C.c_int, []),
    ("gipuma_hip_selftest_reciprocal", C.c_int, [C.c_int, C.POINTER(C.c_ulonglong)]),
    ("gipuma_hip_selftest_quotient", C.c_int, [C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong)]),
    ("gipuma_hip_create", C.c_int, [C.POINTER(Desc), C.POINTER(C.c_void_p)]),
    ("gipuma_hip_destroy", C.c_int, [C.c_void_p]),
    ("gipuma_hip_init_planes", C.c_int, [C.c_void_p]),
    ("gipuma_hip_sweep", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint]),
    ("gipuma_hip_finalize", C.c_int, [C.c_void_p]),
    ("gipuma_hip_eval_cost", C.c_int, [C.c_void_p, _FP, _FP]),
    ("gipuma_hip_get_state", C.c_int, [C.c_void_p, _FP, _FP]),
    ("gipuma_hip_set_state", C.c_int, [C.c_void_p, _FP, _FP]),
    ("gipuma_hip_state_device_ptrs", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("gipuma_hip_solve", C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    ("gipuma_hip_launch_times", C.c_int, [C.c_void_p, _FP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("gipuma_hip_group_times", C.c_int, [C.c_void_p, _FP, C.c_int, C.POINTER(C.c_int)]),
    ("gipuma_hip_schedule", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("gipuma_hip_run", C.c_int, [C.POINTER(Desc), _FP, _FP, C.POINTER(Timing)]),
    ("gipuma_hip_seed_planes", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("gipuma_hip_solve_seeded", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Timing)]),
    ("gipuma_hip_downsample", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p]),
    ("gipuma_hip_fuse", C.c_int, [C.POINTER(FusionDesc), C.POINTER(C.c_void_p)]),
    ("gipuma_hip_fusion_count", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _FP]),
    ("gipuma_hip_fusion_points", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("gipuma_hip_fusion_used", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gipuma_hip_fusion_free", C.c_int, [C.c_void_p]),
    ("gipuma_hip_prior_from_views", C.c_int, [C.POINTER(PriorDesc), C.c_void_p, C.POINTER(C.c_int64), _FP]),
    ("gipuma_hip_cloud_nearest", C.c_int, [C.POINTER(CloudDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), _FP]),
    ("gipuma_hip_cloud_last_stats", C.c_int, [C.POINTER(C.c_int64)]),
    ("gipuma_hip_cloud_thin", C.c_int, [C.POINTER(ThinDesc), C.c_void_p, C.POINTER(C.c_int64), _FP]),
    ("gipuma_hip_cloud_neighbours", C.c_int, [C.POINTER(NeighboursDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), _FP]),
    ("gipuma_hip_cloud_knn", C.c_int, [C.POINTER(KnnDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                       _FP]),
    ("gipuma_hip_cloud_components", C.c_int, [C.POINTER(ComponentsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                              _FP]),
    ("gipuma_hip_cloud_normals", C.c_int, [C.POINTER(NormalsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int64), _FP]),
]

_lib = None


def load_library(path=None):
    """dlopen the HIP library and bind every declared symbol.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    exp = os.environ.get("GIPUMA_HIP_EXPERIMENTS", "0") not in ("", "0")
    p = path or (os.environ.get("GIPUMA_HIP_LIB") if exp else None) or LIB_PATH  # A/B: a differently built library
    if not os.path.exists(p):
        raise GipumaHipError(
            "HIP extension not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
            "g.build()'`); gipuma_amd has no CPU fallback" % p)
    try:
        lib = C.CDLL(p)
    except OSError as e:  # e.g. libamdhip64 not loadable
        raise GipumaHipError("cannot load %s: %s" % (p, e))
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.gipuma_hip_version() != ABI_VERSION:
        raise GipumaHipError("ABI mismatch: library %d, bindings %d"
                             % (lib.gipuma_hip_version(), ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


def check(lib, rc, what):
    if rc != 0:
        msg = lib.gipuma_hip_last_error()
        raise GipumaHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
