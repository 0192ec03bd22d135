"""The cross-view prior: the solved (normal, depth) maps of neighbouring views, carried into a new
reference camera as the start of its solve -- PatchMatch's view propagation across the views of a scan.

    prior = prior_from_views(P_all[ref], [norm4 of the solved neighbours], [their P], cam_scale, depth_min, depth_max)
    session.solve_seeded(prior, 0)                # a few iterations instead of the full count from random planes

Every source pixel is splatted into the target camera through a 64-bit z-buffer (the nearest surface wins), and every
target pixel intersects the winner's plane with its own ray (gipuma_amd/csrc/gipuma_prior.hip, gfx950; the contract is
in include/gipuma_hip.h).  Pixels no source reaches come out as (0, 0, 0, 0), which the seed answers with the random plane
of a plain solve.  There is no CPU fallback.
"""
import ctypes as C

from . import abi
from .cameras import cos_f32, view_constants


def grazing_cos(degrees=80.0):
    """f32(cos(degrees)), computed in double"""
    return float(cos_f32(degrees))


def prior_from_views(target_P, source_norm4s, source_Ps, cam_scale=1.0, depth_min=-1.0, depth_max=-1.0, costs=None,
                     max_cost=None, fill=True, grazing_deg=80.0, out=None, return_info=False, device_id=0):
    """The prior of the camera `target_P` from S solved views.  source_norm4s: (rows, cols, 4) float32 result planes
    (n_world.xyz, depth), device tensors (passed by pointer, no copy) or host arrays (uploaded); source_Ps: their 3x4
    projection matrices; costs (with max_cost): one (rows, cols) cost plane per source, pixels beyond max_cost are left
    out.  Returns the (rows, cols, 4) device tensor that Session.solve_seeded(prior, 0) / seed_planes(prior, 0) take
    (`out`: write into this contiguous float32 device tensor instead of a new one).  Runs on torch's current stream.
    With return_info: (prior, dict(direct, filled, empty, device_ms)), and the call has completed; without, the prior is
    complete once that stream is -- synchronise it before a session reads the prior on its own stream."""
    # (torch first: it brings a HIP runtime of its own, gipuma_amd.fusion.fuse)
    import torch
    lib = abi.load_library()
    S = len(source_norm4s)
    if len(source_Ps) != S:
        raise ValueError("need one P per source view")
    if not 1 <= S <= abi.MAX_VIEWS:
        raise ValueError("the prior takes 1..%d source views, got %d" % (abi.MAX_VIEWS, S))
    if (costs is None) != (max_cost is None):
        raise ValueError("costs and max_cost go together")
    if costs is not None and len(costs) != S:
        raise ValueError("need one cost plane per source view")
    shape = tuple(source_norm4s[0].shape)
    if len(shape) != 3 or shape[2] != 4:
        raise ValueError("norm4 planes are (rows, cols, 4)")
    for k in range(S):
        if tuple(source_norm4s[k].shape) != shape or (costs is not None and tuple(costs[k].shape) != shape[:2]):
            raise ValueError("every view must have the same size: %s" % (shape[:2],))
    if lib.gipuma_hip_device_count() < 1:
        raise abi.GipumaHipError("the cross-view prior needs a HIP device; gipuma_amd has no CPU fallback")
    dev, keep = torch.device("cuda", device_id), []  # keep: the device planes handed over
    views = (abi.FusionView * S)()
    for k in range(S):
        abi.fill_view(views[k], view_constants(source_Ps[k], cam_scale), abi.device_plane(source_norm4s[k], dev, keep))
    cost_ptrs = None
    if costs is not None:
        cost_ptrs = (C.c_void_p * S)(*[abi.device_plane(c, dev, keep) for c in costs])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError("out must be a contiguous float32 device tensor of shape %s" % (shape,))
    d = abi.PriorDesc()
    d.abi_version = abi.ABI_VERSION
    d.rows, d.cols, d.n_sources = shape[0], shape[1], S
    abi.fill_view(d.target, view_constants(target_P, cam_scale))
    d.sources = C.cast(views, C.POINTER(abi.FusionView))
    d.costs = C.cast(cost_ptrs, C.POINTER(C.c_void_p)) if cost_ptrs is not None else None
    d.max_cost = float(max_cost) if max_cost is not None else 0.0
    d.depth_min, d.depth_max = depth_min, depth_max
    d.grazing_cos = grazing_cos(grazing_deg)
    d.fill = 1 if fill else 0
    d.device_id = device_id
    stream = torch.cuda.current_stream(dev)
    d.stream = stream.cuda_stream or None
    counts, ms = (C.c_int64 * 3)(), C.c_float()
    abi.check(lib, lib.gipuma_hip_prior_from_views(C.byref(d), out.data_ptr(), counts if return_info else None,
                                                   C.byref(ms) if return_info else None), "gipuma_hip_prior_from_views")
    for t in keep:  # (uploaded planes may be released once the stream has passed this point)
        t.record_stream(stream)
    if not return_info:
        return out
    return out, dict(direct=int(counts[0]), filled=int(counts[1]), empty=int(counts[2]), device_ms=float(ms.value))


def greedy_order(refs, sources_of):
    """The order in which a scan's reference views are solved with --view_prior: next is the unsolved view with the most
    already-solved views among its selected sources, ties in the order of `refs` (the scan's order).  refs: names;
    sources_of: {name: the selected source names}.  Deterministic; the first view is refs[0]."""
    todo, solved, order = list(refs), set(), []
    while todo:
        best = max(range(len(todo)), key=lambda i: (sum(1 for s in sources_of[todo[i]] if s in solved), -i))
        name = todo.pop(best)
        order.append(name)
        solved.add(name)
    return order
