"""Coarse-to-fine solve of one reference view: solve at half resolution, where an iteration costs a
quarter, carry the (world normal, depth) map up as the start of the next level, polish at full resolution.

    pyr = ScanPyramid(dev_images, levels=2)              # the coarse planes of the whole scan, once
    norm4, cost, times = solve_view(pyr, P_all, used, ap_view, level_iterations=[8, 2], seed=1)
    pyr.close()

Level l of an image is l applications of the library's 2x2 mean (gipuma_hip_downsample: coarse pixel X covers the fine
pixels 2X, 2X+1, a last odd row or column is dropped), so x_coarse = (x_fine - 1/2) / 2 and the camera of a level is
not a new formula: it is get_camera_parameters of S^l P for every view, S = [[1/2, 0, -1/4], [0, 1/2, -1/4], [0, 0, 1]].
R and C of every camera are the same on all levels; depth is the camera-frame z; so a level's result seeds the next
one as it is (Session.solve_seeded, shift 1).  View selection and the depth range are decided once, on the finest
level, and reused on every level.
"""
import numpy as np

from . import abi
from .cameras import get_camera_parameters
from .problem import AlgorithmParameters, GlobalState, Session

S_HALF = np.array([[0.5, 0.0, -0.25], [0.0, 0.5, -0.25], [0.0, 0.0, 1.0]], dtype=np.float64)


def level_projection(P, level):
    """S^level P in float64: the projection matrix onto pyramid level `level` of the image P projects onto"""
    P = np.asarray(P, dtype=np.float64)
    for _ in range(int(level)):
        P = S_HALF @ P
    return P


def level_cameras(P_list, level, cam_scale=1.0):
    """the camera set of a pyramid level.  Level 0: get_camera_parameters(P_list, cam_scale), the plain solve's cameras.
    Coarser levels: --cam_scale first, as diag(1/s, 1/s, 1) P, then S^level, then the same decomposition."""
    if level == 0:
        return get_camera_parameters(list(P_list), cam_scale=cam_scale)
    D = np.diag([1.0 / cam_scale, 1.0 / cam_scale, 1.0])
    return get_camera_parameters([level_projection(D @ np.asarray(P, dtype=np.float64), level) for P in P_list])


def downsample(tensor, out=None):
    """one pyramid level of a device plane, (rows, cols) gray or (rows, cols, 4) colour float32, through the C-ABI
    (pyr::downsample2_kernel) on torch's current stream; returns the ((rows >> 1), (cols >> 1)[, 4]) device tensor"""
    import torch
    if not tensor.is_cuda or tensor.dtype != torch.float32 or tensor.dim() not in (2, 3) or tensor.stride(-1) != 1:
        raise ValueError("downsample takes a float32 device plane (rows, cols) or (rows, cols, 4)")
    channels = 1 if tensor.dim() == 2 else int(tensor.shape[2])
    if channels == 4 and tensor.stride(1) != 4:
        raise ValueError("a colour plane's texels must be contiguous")
    rows, cols, pitch = int(tensor.shape[0]), int(tensor.shape[1]), int(tensor.stride(0))
    if out is None:
        shape = (rows >> 1, cols >> 1) + ((4,) if tensor.dim() == 3 else ())
        out = torch.empty(shape, dtype=torch.float32, device=tensor.device)
    lib = abi.load_library()
    stream = torch.cuda.current_stream(tensor.device).cuda_stream
    abi.check(lib, lib.gipuma_hip_downsample(tensor.data_ptr(), rows, cols, pitch, channels, out.data_ptr(),
                                             int(out.stride(0)), tensor.device.index, stream or None),
              "gipuma_hip_downsample")
    return out


class ScanPyramid:
    """The pyramid levels of a whole scan's device images, built once and shared by every reference view like the
    images themselves.  planes[l][i]: image i on level l (level 0: the caller's tensors).  It owns the coarse planes:
    close() clears the library's image cache first (with GIPUMA_HIP_FLAG_CACHE_IMAGES the cache is keyed by device
    address, and torch hands a freed plane's address out again), so every session on them must be closed by then."""

    def __init__(self, dev_images, levels):
        import torch
        if levels < 1:
            raise ValueError("levels must be >= 1")
        self.levels = int(levels)
        self.planes = [list(dev_images)]
        self.device = dev_images[0].device
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(self.device))
        for _ in range(1, self.levels):
            self.planes.append([downsample(t) for t in self.planes[-1]])
        e1.record(torch.cuda.current_stream(self.device))
        # complete before a session reads them on a stream of its own (include/gipuma_hip.h, IMAGES_ON_DEVICE)
        torch.cuda.synchronize(self.device)
        self.device_ms = e0.elapsed_time(e1)  # paid once per scan, not per view

    def size(self, level):
        t = self.planes[level][0]
        return int(t.shape[0]), int(t.shape[1])

    def close(self):
        if len(self.planes) > 1:
            abi.load_library().gipuma_hip_cache_clear()
        self.planes = self.planes[:1]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def level_problem(pyramid, level, P_list, used, ap, iterations, seed, cam_scale=1.0, flags=abi.FLAG_CACHE_IMAGES):
    """GlobalState of reference view used[0] with the sources used[1:] on one pyramid level.  `ap` carries the depth
    range decided on the finest level (batch.plan_views); the same blocksize is used on every level."""
    cs = level_cameras([P_list[i] for i in used], level, cam_scale)
    ap_l = AlgorithmParameters(**{k: getattr(ap, k) for k in vars(ap)})
    ap_l.iterations = int(iterations)
    return GlobalState.on_resident_planes(pyramid.planes[level], used, cs, ap_l, seed=seed, flags=flags)


def solve_view(pyramid, P_list, used, ap, level_iterations, seed=1, mode="exact", cam_scale=1.0, timing=True,
               flags=abi.FLAG_CACHE_IMAGES):
    """The hierarchy for one reference view: the coarsest level by a plain solve, every finer level by solve_seeded
    from the device planes of the level below (no host round trip).  `level_iterations`: one entry per level of the
    pyramid, coarsest first.  Returns (norm4, cost, times) of the finest level; times: per level, coarsest first,
    dict(level, rows, cols, iterations, ms_init (the seed's time above the coarsest level), ms_sweeps, ms_finalize,
    ms_total) -- device times when `timing`, else None."""
    if len(level_iterations) != pyramid.levels:
        raise ValueError("need one iteration count per level (%d), coarsest first" % pyramid.levels)
    fast, literal = mode == "fast", mode == "literal"
    prev, times = None, []
    try:
        for k, level in enumerate(range(pyramid.levels - 1, -1, -1)):
            gs = level_problem(pyramid, level, P_list, used, ap, level_iterations[k], seed, cam_scale, flags)
            s = Session(gs, fast=fast, literal=literal)
            try:
                if prev is None:
                    t = s.solve(timing=timing)
                else:
                    if not timing:
                        prev.sync()  # (a timed solve has waited already; the finer session's stream would not)
                    t = s.solve_seeded(prev.state_device_ptrs()[0], 1, timing=timing, prior_rows=prev.gs.rows,
                                       prior_cols=prev.gs.cols)
                    if not timing:
                        s.sync()  # the prior is read: the coarser session may go
            except Exception:
                s.close()
                raise
            if prev is not None:
                prev.close()
            prev = s
            times.append(dict(level=level, rows=gs.rows, cols=gs.cols, iterations=int(level_iterations[k]),
                              ms_init=t.ms_init, ms_sweeps=t.ms_sweeps, ms_finalize=t.ms_finalize,
                              ms_total=t.ms_total) if timing else None)
        norm4, cost = prev.get_state()
    finally:
        if prev is not None:
            prev.close()
    return norm4, cost, times
