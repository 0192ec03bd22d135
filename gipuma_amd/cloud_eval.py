"""Score a point cloud against a reference cloud on the GPU: accuracy and completeness, after thinning
the cloud to a minimum point spacing, dropping its isolated points, dropping its
statistical outliers, dropping its small clumps and dropping the points whose normal
disagrees with the surface around them when asked to.

    python -m gipuma_amd.cloud_eval --cloud fused.ply --reference gt.ply --max_dist 20 --thresholds 0.5,1,2 \\
        [--reduce 0.2 [--reduce_reference] [--seed N]] [--neighbour_radius 1 --min_neighbours 8] \\
        [--outlier_radius 1 --outlier_k 16 --outlier_std 2] [--component_radius 1 --min_component 100] \\
        [--normal_radius 1 --normal_k 16 --max_normal_angle 30] [--write_cloud scored.ply [--estimated_normals]] \\
        [--output report.json]

DTU -- the data set this project is calibrated on -- scores a reconstruction cloud against cloud: accuracy is the distance
from each reconstructed point to the nearest reference point, completeness the same the other way round, distances beyond
a cut-off discarded.  Both directions are one nearest-neighbour search each (gipuma_hip_cloud_nearest,
gipuma_amd/csrc/gipuma_cloud.hip: gfx950 kernels over a uniform grid, equal to a brute-force search in every bit).  There
is no CPU fallback.  The means of the score are means over points, so they are weighted by how densely the fusion happened
to sample each surface; DTU removes that by thinning the reconstruction to a minimum spacing first (its 0.2 mm resampling).
--reduce does the same here (gipuma_hip_cloud_thin: points visited in a hashed order, a point kept unless a kept point lies
within the spacing), and `thin` offers it for the delivered cloud.  What a fused cloud still carries then are floaters:
points, or small clumps of points, far from any surface.  --neighbour_radius / --min_neighbours drop every point with
fewer than that many other points within the radius (gipuma_hip_cloud_neighbours; `drop_isolated`, `neighbour_counts`),
after the thinning: a count means the same everywhere only once the density is normalised.  A count cannot see the loose
halo a few spacings off a surface, or the smeared rim of a depth step: such points have neighbours enough, only farther away
than a surface point's.  --outlier_radius / --outlier_k / --outlier_std drop every point whose mean distance to its k
nearest neighbours within the radius (gipuma_hip_cloud_knn; `knn`, `nearest_k`, `drop_outliers`) exceeds the cloud's mean of
that figure by more than outlier_std standard deviations, and every point with fewer than k neighbours there.  Neither
filter sees a CLUMP: forty points fused at a wrong depth have thirty-nine neighbours each, closer than a surface point's.
--component_radius / --min_component drop every connected component of the radius graph -- points joined where they lie
within the radius of each other -- that has fewer than min_component points (gipuma_hip_cloud_components,
gipuma_amd/csrc/gipuma_components.hip; `components`, `component_labels`, `drop_small_components`), after the three;
`component_labels` also segments a cloud into its objects.  None of the four reads the normals a fused cloud carries, which
are averaged plane hypotheses, not the normals of the surface the points form.  `normals` / `estimate_normals`
(gipuma_hip_cloud_normals, gipuma_amd/csrc/gipuma_normals.hip) estimate the geometric normal and the surface variation of
every point from its k nearest neighbours within a radius; --normal_radius / --normal_k / --max_normal_angle drop every
point of the cloud whose own normal (the PLY's nx, ny, nz) is more than that angle off the estimate, and every point with
fewer than three neighbours there (`normal_agreement`, `drop_disagreeing_normals`), after the four; --estimated_normals
writes the estimates in place of the file's normals.  --write_cloud writes the cloud as it is scored.  Not part of the score here: DTU's observability masks and ground-plane removal.
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import abi, dmb
from .cameras import cos_f32

THRESHOLDS = (0.5, 1.0, 2.0)
_STATS = ("grid", "cells_x", "cells_y", "cells_z", "early_out", "searched")
ORDERS = {"hashed": 0, "index": 1}
_THIN_INFO = ("kept", "dropped", "not_finite", "rounds", "grid", "cells_x", "cells_y", "cells_z")
_KNN_INFO = ("complete", "short", "not_finite", "unused", "grid", "cells_x", "cells_y", "cells_z")
_COMPONENT_INFO = ("kept", "dropped", "not_finite", "components", "grid", "cells_x", "cells_y", "cells_z")
_NORMAL_INFO = ("estimated", "short", "not_finite", "flipped", "grid", "cells_x", "cells_y", "cells_z")
_NEIGHBOUR_INFO = ("kept", "dropped", "not_finite", "saturated", "grid", "cells_x", "cells_y", "cells_z")


def _device_cloud(a, device, keep):
    """the device address of the (n, 3) float32 cloud `a` (abi.device_plane: a device tensor goes by pointer) and n"""
    if len(a.shape) != 2 or a.shape[1] != 3:
        raise ValueError("a cloud is an (n, 3) array of xyz, got %s" % (tuple(a.shape),))
    n = int(a.shape[0])
    return (abi.device_plane(a, device, keep) if n else None), n


def _open(what, desc_type, device_id):
    """every call's prelude: (torch, lib, a `desc_type` with abi_version and device_id set, the torch device, the list that
    keeps the device clouds handed over alive until the caller returns); `what` needs a HIP device, without one this raises"""
    # (torch first: it brings a HIP runtime of its own, and a process that loaded the library's first cannot start torch's)
    import torch
    lib = abi.load_library()
    if lib.gipuma_hip_device_count() < 1:
        raise abi.GipumaHipError("%s needs a HIP device; gipuma_amd has no CPU fallback" % what)
    return torch, lib, desc_type(abi_version=abi.ABI_VERSION, device_id=device_id), torch.device("cuda", device_id), []


def _figures(names, values):
    return {k: int(v) for k, v in zip(names, values)}


def _call(torch, lib, name, d, dev, outs, names):
    """lib.<name>(d, *addresses of `outs` (NULL for None or an empty tensor), int64 figures, device_ms): (figures dict, ms)"""
    torch.cuda.synchronize(dev)  # (the library works on a stream of its own: the clouds must be complete)
    figures, ms = (C.c_int64 * len(names))(), C.c_float()
    abi.check(lib, getattr(lib, name)(C.byref(d), *[t.data_ptr() if t is not None and t.numel() else None for t in outs],
                                      figures, C.byref(ms)), name)
    return _figures(names, figures), ms.value


def _indices(keep):
    """the ascending int64 indices (numpy) of the points a device mask keeps"""
    import torch
    return torch.nonzero(keep).reshape(-1).cpu().numpy().astype(np.int64)


def nearest(queries, targets, max_dist, grid=0, device_id=0, return_info=False):
    """For every query the nearest target within max_dist (the contract of gipuma_hip_cloud_nearest).  queries, targets:
    (n, 3) numpy arrays or torch tensors; device tensors are passed by pointer.  Returns (d2, idx, device_ms): float32
    squared distances (+inf: none), int32 target indices (-1: none), both numpy, and the device time in ms; with
    return_info also dict(found, none, grid, cells_x, cells_y, cells_z, early_out, searched)."""
    torch, lib, d, dev, held = _open("the cloud search", abi.CloudDesc, device_id)
    d.queries, d.n_queries = _device_cloud(queries, dev, held)
    d.targets, d.n_targets = _device_cloud(targets, dev, held)
    d.max_dist, d.grid = float(max_dist), int(grid)
    d2, idx = (torch.empty(d.n_queries, dtype=t, device=dev) for t in (torch.float32, torch.int32))
    counts, ms = _call(torch, lib, "gipuma_hip_cloud_nearest", d, dev, (d2, idx), ("found", "none"))
    out = d2.cpu().numpy(), idx.cpu().numpy(), ms
    if not return_info:
        return out
    stats = (C.c_int64 * len(_STATS))()
    abi.check(lib, lib.gipuma_hip_cloud_last_stats(stats), "gipuma_hip_cloud_last_stats")
    return out + (dict(counts, **_figures(_STATS, stats)),)


def thin_mask(points, radius, seed=0, order="hashed", grid=0, device_id=0):
    """The contract of gipuma_hip_cloud_thin on the (n, 3) cloud `points` (a numpy array or a torch tensor; a device
    tensor is passed by pointer): (keep, device_ms, info) -- keep a torch uint8 tensor on the device, one byte per point,
    info dict(kept, dropped, not_finite, rounds, grid, cells_x, cells_y, cells_z)."""
    if order not in ORDERS:
        raise ValueError("order is 'hashed' or 'index', got %r" % (order,))
    torch, lib, d, dev, held = _open("thinning a cloud", abi.ThinDesc, device_id)
    d.points, d.n_points = _device_cloud(points, dev, held)
    d.radius, d.seed, d.order, d.grid = float(radius), int(seed) & 0xFFFFFFFF, ORDERS[order], int(grid)
    keep = torch.empty(d.n_points, dtype=torch.uint8, device=dev)
    info, ms = _call(torch, lib, "gipuma_hip_cloud_thin", d, dev, (keep,), _THIN_INFO)
    return keep, ms, info


def thin(points, radius, seed=0, order="hashed", grid=0, device_id=0, return_info=False):
    """Thins a cloud to a minimum point spacing: the points are visited in ascending (prio(i), i) -- a hash
    of seed and index, or with order="index" the caller's own order -- and a point is kept unless a point kept before it
    lies within `radius` (inclusive).  Returns the ascending int64 indices of the kept points (numpy); with return_info
    also device_ms and dict(kept, dropped, not_finite, rounds, grid, cells_x, cells_y, cells_z)."""
    keep, ms, info = thin_mask(points, radius, seed, order, grid, device_id)
    return (_indices(keep), ms, info) if return_info else _indices(keep)


def neighbours(points, radius, min_neighbours=0, max_count=0, grid=0, device_id=0, counts=True, keep=True):
    """The contract of gipuma_hip_cloud_neighbours on the (n, 3) cloud `points` (a numpy array or a torch tensor; a device
    tensor is passed by pointer): (count, keep, device_ms, info) -- count a torch int32 tensor on the device holding the
    uint32 counts' bits, keep a torch uint8 tensor on the device, one entry per point each, or None where `counts` /
    `keep` is False; info dict(kept, dropped, not_finite, saturated, grid, cells_x, cells_y, cells_z)."""
    torch, lib, d, dev, held = _open("counting a cloud's neighbours", abi.NeighboursDesc, device_id)
    d.points, d.n_points = _device_cloud(points, dev, held)
    d.radius, d.min_neighbours, d.max_count, d.grid = float(radius), int(min_neighbours), int(max_count), int(grid)
    count_t = torch.empty(d.n_points, dtype=torch.int32, device=dev) if counts else None
    keep_t = torch.empty(d.n_points, dtype=torch.uint8, device=dev) if keep else None
    info, ms = _call(torch, lib, "gipuma_hip_cloud_neighbours", d, dev, (count_t, keep_t), _NEIGHBOUR_INFO)
    return count_t, keep_t, ms, info


def neighbour_counts(points, radius, max_count=0, grid=0, device_id=0, return_info=False):
    """For every point of the cloud the number of OTHER finite points within `radius` (inclusive; an exact copy counts;
    DESIGN.md 16), 0 for a point that is not finite; with max_count > 0 the counts saturate there.  Returns uint32 counts
    (numpy); with return_info also device_ms and dict(kept, dropped, not_finite, saturated, grid, cells_x, cells_y,
    cells_z) -- min_neighbours is 0 here, so every finite point is `kept`."""
    count, _, ms, info = neighbours(points, radius, 0, max_count, grid, device_id, keep=False)
    out = count.cpu().numpy().view(np.uint32)
    return (out, ms, info) if return_info else out


def drop_isolated(points, radius, min_neighbours, grid=0, device_id=0, return_info=False):
    """Drops the isolated points of a cloud: a point is kept iff it is finite and at least `min_neighbours`
    other finite points lie within `radius` (inclusive).  Counting stops at max(min_neighbours, 1), so points in dense
    regions stop early.  Returns the ascending int64 indices of the kept points (numpy), like `thin`; with return_info also
    device_ms and dict(kept, dropped, not_finite, saturated, grid, cells_x, cells_y, cells_z)."""
    _, keep, ms, info = neighbours(points, radius, min_neighbours, max(int(min_neighbours), 1), grid, device_id, counts=False)
    return (_indices(keep), ms, info) if return_info else _indices(keep)


def knn(points, radius, k, grid=0, device_id=0, d2=True, idx=True, count=True, mean=True):
    """The contract of gipuma_hip_cloud_knn on the (n, 3) cloud `points` (a numpy array or a torch tensor; a device tensor
    is passed by pointer): (d2, idx, count, mean, device_ms, info) -- torch tensors on the device, d2 float32 (n, k) and
    idx int32 (n, k), ascending in (d2, idx) with (+inf, -1) in the empty slots, count int32 (n,) holding the uint32 m's
    bits, mean float32 (n,), each None where its switch is False; info dict(complete, short, not_finite, grid, cells_x,
    cells_y, cells_z)."""
    torch, lib, d, dev, held = _open("a cloud's nearest neighbours", abi.KnnDesc, device_id)
    d.points, d.n_points = _device_cloud(points, dev, held)
    d.radius, d.k, d.grid = float(radius), int(k), int(grid)
    rows = (d.n_points, max(d.k, 0))
    outs = (torch.empty(rows, dtype=torch.float32, device=dev) if d2 else None,
            torch.empty(rows, dtype=torch.int32, device=dev) if idx else None,
            torch.empty(d.n_points, dtype=torch.int32, device=dev) if count else None,
            torch.empty(d.n_points, dtype=torch.float32, device=dev) if mean else None)
    info, ms = _call(torch, lib, "gipuma_hip_cloud_knn", d, dev, outs, _KNN_INFO)
    del info["unused"]
    return outs + (ms, info)


def nearest_k(points, radius, k, grid=0, device_id=0, return_info=False):
    """For every point of the cloud its (at most) k nearest OTHER finite points within `radius` (inclusive; an exact copy is
    one): (d2 (n, k) float32, idx (n, k) int32, m (n,) uint32), numpy -- row i ascending in (d2, idx), its
    first m[i] slots filled, the others (+inf, -1); with return_info also device_ms and dict(complete, short, not_finite,
    grid, cells_x, cells_y, cells_z)."""
    d2, idx, m, _, ms, info = knn(points, radius, k, grid, device_id, mean=False)
    out = d2.cpu().numpy(), idx.cpu().numpy(), m.cpu().numpy().view(np.uint32)
    return out + (ms, info) if return_info else out


def outlier_threshold(mean, std_ratio):
    """(keep mask, mu, sigma, t) of the statistical filter from the float32 `mean` of gipuma_hip_cloud_knn (+inf: fewer
    than k neighbours): mu and sigma are the mean and the population standard deviation of the finite entries -- the
    points with a complete list -- in numpy float64, in index order; t = float32(mu + std_ratio * sigma); a point is kept
    iff its list is complete and mean <= t.  No complete list: nothing kept, mu = sigma = t = NaN."""
    mean = np.asarray(mean, dtype=np.float32)
    complete = np.isfinite(mean)
    if not complete.any():
        return np.zeros(len(mean), dtype=bool), float("nan"), float("nan"), float("nan")
    of = mean[complete].astype(np.float64)
    mu, sigma = float(of.mean()), float(of.std())
    with np.errstate(over="ignore"):
        t = np.float32(mu + float(std_ratio) * sigma)
    return complete & (mean <= t), mu, sigma, float(t)


def drop_outliers(points, radius, k, std_ratio, grid=0, device_id=0, return_info=False):
    """Drops the statistical outliers of a cloud: with mean(i) the mean distance from point i to its k
    nearest other finite points within `radius`, and mu, sigma the mean and standard deviation of that figure over the
    points that have k such neighbours, a point is kept iff it has k neighbours within `radius` and mean(i) <= mu +
    std_ratio * sigma.  A point with fewer is dropped and takes no part in mu, sigma: this is drop_isolated's rule with
    min_neighbours = k.  Returns the ascending int64 indices of the kept points (numpy), like `thin`; with return_info also
    device_ms and dict(complete, short, not_finite, grid, cells_x, cells_y, cells_z, mu, sigma, threshold).  Only the
    means are asked of the library, where +inf says "fewer than k"; a radius whose float32 square is +inf (above 1.8e19) is
    refused, because there a complete list may hold an overflowed d2 and say +inf as well."""
    if not (std_ratio >= 0 and np.isfinite(std_ratio)):
        raise ValueError("std_ratio must be >= 0 and finite, got %r" % (std_ratio,))
    with np.errstate(over="ignore"):
        if np.isposinf(np.float32(radius) * np.float32(radius)):
            raise ValueError("the filter needs a radius whose float32 square is finite, got %r" % (radius,))
    _, _, _, mean, ms, info = knn(points, radius, k, grid, device_id, d2=False, idx=False, count=False)
    keep, mu, sigma, t = outlier_threshold(mean.cpu().numpy(), std_ratio)
    kept = np.nonzero(keep)[0].astype(np.int64)
    return (kept, ms, dict(info, mu=mu, sigma=sigma, threshold=t)) if return_info else kept


def components(points, radius, min_size=0, grid=0, device_id=0, label=True, size=True, keep=True):
    """The contract of gipuma_hip_cloud_components on the (n, 3) cloud `points` (a numpy array or a torch tensor; a device
    tensor is passed by pointer): (label, size, keep, device_ms, info) -- label a torch int32 tensor on the device (the
    smallest index of the point's connected component in the radius graph, -1 for a point that is not finite), size a torch
    int32 tensor holding the uint32 cardinalities' bits, keep a torch uint8 tensor (size >= min_size), one entry per point
    each, or None where its switch is False; info dict(kept, dropped, not_finite, components, grid, cells_x, cells_y,
    cells_z)."""
    torch, lib, d, dev, held = _open("a cloud's connected components", abi.ComponentsDesc, device_id)
    d.points, d.n_points = _device_cloud(points, dev, held)
    d.radius, d.min_size, d.grid = float(radius), int(min_size), int(grid)
    outs = (torch.empty(d.n_points, dtype=torch.int32, device=dev) if label else None,
            torch.empty(d.n_points, dtype=torch.int32, device=dev) if size else None,
            torch.empty(d.n_points, dtype=torch.uint8, device=dev) if keep else None)
    info, ms = _call(torch, lib, "gipuma_hip_cloud_components", d, dev, outs, _COMPONENT_INFO)
    return outs + (ms, info)


def component_labels(points, radius, grid=0, device_id=0, return_info=False):
    """The connected components of the cloud's radius graph: two finite points are joined where they lie
    within `radius` of each other (inclusive; an exact copy is joined).  Returns (label int32, size uint32), numpy: the
    smallest index of the point's component and the component's number of points, (-1, 0) for a point that is not finite;
    with return_info also device_ms and dict(kept, dropped, not_finite, components, grid, cells_x, cells_y, cells_z) --
    min_size is 0 here, so every finite point is `kept`."""
    label, size, _, ms, info = components(points, radius, 0, grid, device_id, keep=False)
    out = label.cpu().numpy(), size.cpu().numpy().view(np.uint32)
    return out + (ms, info) if return_info else out


def drop_small_components(points, radius, min_size, grid=0, device_id=0, return_info=False):
    """Drops the small clumps of a cloud: a point is kept iff it is finite and its connected component in
    the radius graph has at least `min_size` points.  Returns the ascending int64 indices of the kept points (numpy), like
    `thin`; with return_info also device_ms and dict(kept, dropped, not_finite, components, grid, cells_x, cells_y,
    cells_z) -- components counts all of them, the dropped ones too."""
    _, _, keep, ms, info = components(points, radius, min_size, grid, device_id, label=False, size=False)
    return (_indices(keep), ms, info) if return_info else _indices(keep)


def normals(points, radius, k, orient=0, viewpoint=None, guide=None, grid=0, device_id=0, normal=True, variation=True, count=True,
            scatter=False):
    """The contract of gipuma_hip_cloud_normals on the (n, 3) cloud `points` (a numpy array or a torch tensor; a device
    tensor is passed by pointer): (normal, variation, count, scatter, device_ms, info) -- torch tensors on the device, normal
    float32 (n, 3), variation float32 (n,), count int32 (n,) holding the uint32 m's bits, scatter float64 (n, 6), the upper
    triangle of C, each None where its switch is False; info dict(estimated, short, not_finite, flipped, grid, cells_x,
    cells_y, cells_z).  orient 0: the component of largest magnitude positive; 1: towards `viewpoint` (3 numbers); 2: along
    the (n, 3) normals `guide`."""
    if int(orient) == 1 and viewpoint is None:
        raise ValueError("orient 1 needs a viewpoint")
    torch, lib, d, dev, held = _open("a cloud's normals", abi.NormalsDesc, device_id)
    d.points, d.n_points = _device_cloud(points, dev, held)
    d.radius, d.k, d.grid, d.orient = float(radius), int(k), int(grid), int(orient)
    if viewpoint is not None:
        d.viewpoint = (C.c_float * 3)(*[float(v) for v in viewpoint])
    if guide is not None:
        d.guide, n_guide = _device_cloud(guide, dev, held)
        if n_guide != d.n_points:
            raise ValueError("the guide holds %d normals for %d points" % (n_guide, d.n_points))
    outs = (torch.empty((d.n_points, 3), dtype=torch.float32, device=dev) if normal else None,
            torch.empty(d.n_points, dtype=torch.float32, device=dev) if variation else None,
            torch.empty(d.n_points, dtype=torch.int32, device=dev) if count else None,
            torch.empty((d.n_points, 6), dtype=torch.float64, device=dev) if scatter else None)
    info, ms = _call(torch, lib, "gipuma_hip_cloud_normals", d, dev, outs, _NORMAL_INFO)
    return outs + (ms, info)


def estimate_normals(points, radius, k, orient=0, viewpoint=None, guide=None, grid=0, device_id=0, return_info=False):
    """The geometric normal and the surface variation of every point of the cloud from its (at most) k nearest other finite
    points within `radius`: the eigenvector of the smallest eigenvalue of their covariance, the point
    included, and that eigenvalue's share of the three.  Returns (normal (n, 3) float32, variation (n,) float32), numpy;
    ((0, 0, 0), +inf) for a point that is not finite, has fewer than three neighbours there or whose neighbourhood is a single
    place; with return_info also device_ms and dict(estimated, short, not_finite, flipped, grid, cells_x, cells_y, cells_z)."""
    nrm, var, _, _, ms, info = normals(points, radius, k, orient, viewpoint, guide, grid, device_id, count=False)
    out = nrm.cpu().numpy(), var.cpu().numpy()
    return out + (ms, info) if return_info else out


def normal_agreement(estimated, given):
    """|n . g| / |g| per point in float64 (host side): how well the normals `given` agree with the `estimated` ones, 1 for
    parallel or anti-parallel, 0 for perpendicular -- and 0 where the estimate is the zero vector (no estimate) or g is zero
    or not finite."""
    e = np.ascontiguousarray(estimated, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    g = np.ascontiguousarray(given, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    if len(e) != len(g):
        raise ValueError("%d estimates for %d given normals" % (len(e), len(g)))
    with np.errstate(all="ignore"):
        norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        a = np.abs((e[:, 0] * g[:, 0] + e[:, 1] * g[:, 1]) + e[:, 2] * g[:, 2]) / norm
    bad = ~np.isfinite(g).all(axis=1) | ~(norm > 0) | ~np.isfinite(norm) | ~e.any(axis=1) | ~np.isfinite(a)
    return np.where(bad, 0.0, a)


def _host_normals(given):
    import torch
    return given.detach().cpu().numpy() if isinstance(given, torch.Tensor) else np.asarray(given)


def drop_disagreeing_normals(points, given, radius, k, max_angle_deg, grid=0, device_id=0, return_info=False):
    """Drops the points of a cloud whose own normal disagrees with the surface around them: a point is kept
    iff it has an estimated normal (estimate_normals: at least three neighbours within `radius`, not all in one place) and
    normal_agreement(estimate, given) >= float32(cos(max_angle_deg * pi / 180)), the cosine made in double.  `given`: the (n,
    3) normals the cloud carries.  Returns the ascending int64 indices of the kept points (numpy), like `thin`; with
    return_info also device_ms and dict(estimated, short, not_finite, flipped, grid, cells_x, cells_y, cells_z)."""
    if not (0 <= max_angle_deg <= 90):
        raise ValueError("max_angle_deg must be 0..90, got %r" % (max_angle_deg,))
    nrm, _, _, _, ms, info = normals(points, radius, k, 0, None, None, grid, device_id, variation=False, count=False)
    est = nrm.cpu().numpy()
    keep = est.any(axis=1) & (normal_agreement(est, _host_normals(given)) >= float(cos_f32(max_angle_deg)))
    kept = np.nonzero(keep)[0].astype(np.int64)
    return (kept, ms, info) if return_info else kept


def direction_score(d2, thresholds):
    """One direction of the score from its squared distances (float32, +inf: none): ({mean, median, found, none} over the
    points that found a neighbour, [share of ALL points with d <= tau for tau in thresholds] -- "none" is a miss)."""
    d2 = np.asarray(d2, dtype=np.float32)
    hit = np.isfinite(d2)
    d = np.sqrt(d2[hit].astype(np.float64))
    stats = {"mean": float(d.mean()) if len(d) else float("nan"), "median": float(np.median(d)) if len(d) else float("nan"),
             "found": int(hit.sum()), "none": int(len(d2) - hit.sum())}
    return stats, [float((d <= t).sum() / len(d2)) if len(d2) else 0.0 for t in thresholds]


def combine(acc, prec, comp, rec, thresholds):
    """the report of score() from the two directions' direction_score results"""
    out = {"accuracy": acc, "completeness": comp, "thresholds": [float(t) for t in thresholds], "precision": prec,
           "recall": rec, "fscore": [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)]}
    return out


def _taken(a, idx, device_id):
    """the rows `idx` (numpy int64) of the cloud `a`, as a float32 device tensor"""
    import torch
    dev = torch.device("cuda", device_id)
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(device=dev, dtype=torch.float32)[torch.from_numpy(idx).to(dev)]


def _reduced(a, radius, seed, device_id):
    """the cloud `a` thinned to `radius` (thin, hashed order), as a device tensor, the kept indices and (device_ms, rounds)"""
    idx, ms, info = thin(a, radius, seed=seed, device_id=device_id, return_info=True)
    return _taken(a, idx, device_id), idx, (ms, info["rounds"])


def score(cloud, reference, max_dist=20.0, thresholds=THRESHOLDS, grid=0, device_id=0, reduce=0.0, reduce_reference=False,
          seed=0, neighbour_radius=0.0, min_neighbours=0, return_indices=False, outlier_radius=0.0, outlier_k=0, outlier_std=0.0,
          component_radius=0.0, min_component=0, normal_radius=0.0, normal_k=0, max_normal_angle=0.0, cloud_normals=None):
    """Both directions of the score.  accuracy: {mean, median, found, none} of d = sqrt(d2) (float64, on the host) over
    the cloud's points that found a reference point within max_dist; completeness: the same over the reference's points;
    precision / recall per threshold: the share of ALL cloud / reference points with d <= tau; fscore = 2PR / (P + R), 0
    when both are 0.  Empty clouds give NaN means and 0 counts.  Also the point counts, both device times and the grids.
    reduce > 0: the cloud is thinned to that spacing (thin, hashed order with `seed`) before both searches, with
    reduce_reference the reference too -- DTU thins the reconstruction only.  The report then also carries reduce,
    cloud_points_before, reference_points_before, thin_rounds and thin_device_ms (cloud first, then the reference).
    neighbour_radius > 0: the cloud -- never the reference -- then loses its isolated points (drop_isolated with
    min_neighbours), after the thinning and before both searches; the report then also carries neighbour_radius,
    min_neighbours, cloud_points_before_filter and filter_device_ms.  outlier_radius > 0: the cloud -- never the reference
    -- then loses its statistical outliers (drop_outliers with outlier_k and outlier_std), after both, before both
    searches; the report then also carries outlier_radius, outlier_k, outlier_std, outlier_threshold,
    cloud_points_before_outliers and outlier_device_ms.  component_radius > 0: the cloud -- never the reference -- then
    loses its small clumps (drop_small_components with min_component), after the three, before both searches; the report
    then also carries component_radius, min_component, components, cloud_points_before_components and
    component_device_ms.  normal_radius > 0: the cloud -- never the reference -- then loses the points whose normal in
    `cloud_normals` (an (n, 3) array, row for row the cloud's) disagrees with the estimate (drop_disagreeing_normals with
    normal_k and max_normal_angle), after the four, before both searches; the report then also carries normal_radius,
    normal_k, max_normal_angle, cloud_points_before_normals and normal_device_ms.  return_indices: (report, the ascending indices into `cloud` of
    the points scored, or None where all were)."""
    thresholds = [float(t) for t in thresholds]
    if not (reduce >= 0 and np.isfinite(reduce)):
        raise ValueError("reduce must be >= 0 and finite, got %r" % (reduce,))
    if not (neighbour_radius >= 0 and np.isfinite(neighbour_radius)):
        raise ValueError("neighbour_radius must be >= 0 and finite, got %r" % (neighbour_radius,))
    if int(min_neighbours) != min_neighbours or min_neighbours < 0:
        raise ValueError("min_neighbours must be an integer >= 0, got %r" % (min_neighbours,))
    if not (outlier_radius >= 0 and np.isfinite(outlier_radius)):
        raise ValueError("outlier_radius must be >= 0 and finite, got %r" % (outlier_radius,))
    if outlier_radius > 0 and (int(outlier_k) != outlier_k or not 1 <= outlier_k <= 32):
        raise ValueError("outlier_k must be an integer 1..32, got %r" % (outlier_k,))
    if outlier_radius > 0 and not (outlier_std >= 0 and np.isfinite(outlier_std)):
        raise ValueError("outlier_std must be >= 0 and finite, got %r" % (outlier_std,))
    if not (component_radius >= 0 and np.isfinite(component_radius)):
        raise ValueError("component_radius must be >= 0 and finite, got %r" % (component_radius,))
    if int(min_component) != min_component or not 0 <= min_component < 2 ** 31:
        raise ValueError("min_component must be an integer 0 .. 2^31 - 1, got %r" % (min_component,))
    if not (normal_radius >= 0 and np.isfinite(normal_radius)):
        raise ValueError("normal_radius must be >= 0 and finite, got %r" % (normal_radius,))
    if normal_radius > 0 and (int(normal_k) != normal_k or not 3 <= normal_k <= 32):
        raise ValueError("normal_k must be an integer 3..32, got %r" % (normal_k,))
    if normal_radius > 0 and not (0 <= max_normal_angle <= 90):
        raise ValueError("max_normal_angle must be 0..90 degrees, got %r" % (max_normal_angle,))
    if normal_radius > 0 and (cloud_normals is None or tuple(cloud_normals.shape) != (int(cloud.shape[0]), 3)):
        raise ValueError("normal_radius needs cloud_normals, an (n, 3) array of the cloud's own normals")
    before, thinned, indices = (int(cloud.shape[0]), int(reference.shape[0])), [], None
    if reduce > 0:
        cloud, indices, t = _reduced(cloud, reduce, seed, device_id)
        thinned.append(t)
        if reduce_reference:
            reference, _, t = _reduced(reference, reduce, seed, device_id)
            thinned.append(t)
    if neighbour_radius > 0:  # (after the thinning: a count means the same everywhere once the density is normalised)
        before_filter = int(cloud.shape[0])
        kept, filter_ms, _ = drop_isolated(cloud, neighbour_radius, min_neighbours, device_id=device_id, return_info=True)
        cloud, indices = _taken(cloud, kept, device_id), kept if indices is None else indices[kept]
    if outlier_radius > 0:  # (after both: the mean distance to k neighbours is a figure of the normalised, cleaned cloud)
        before_outliers = int(cloud.shape[0])
        kept, outlier_ms, o_info = drop_outliers(cloud, outlier_radius, int(outlier_k), outlier_std, device_id=device_id,
                                                 return_info=True)
        cloud, indices = _taken(cloud, kept, device_id), kept if indices is None else indices[kept]
    if component_radius > 0:  # (last: the clumps that are left when single points and loose halos have gone)
        before_components = int(cloud.shape[0])
        kept, component_ms, comp_info = drop_small_components(cloud, component_radius, int(min_component), device_id=device_id,
                                                           return_info=True)
        cloud, indices = _taken(cloud, kept, device_id), kept if indices is None else indices[kept]
    if normal_radius > 0:  # (the points fused at a wrong plane among good neighbours: only the normals tell them apart)
        before_normals = int(cloud.shape[0])
        given = _host_normals(cloud_normals)
        kept, normal_ms, _ = drop_disagreeing_normals(cloud, given if indices is None else given[indices], normal_radius, int(normal_k),
                                                      max_normal_angle, device_id=device_id, return_info=True)
        cloud, indices = _taken(cloud, kept, device_id), kept if indices is None else indices[kept]
    a_d2, _, a_ms, a_info = nearest(cloud, reference, max_dist, grid, device_id, return_info=True)
    c_d2, _, c_ms, c_info = nearest(reference, cloud, max_dist, grid, device_id, return_info=True)
    out = combine(*direction_score(a_d2, thresholds), *direction_score(c_d2, thresholds), thresholds)
    out.update({"max_dist": float(max_dist), "cloud_points": int(len(a_d2)), "reference_points": int(len(c_d2)),
                "accuracy_device_ms": a_ms, "completeness_device_ms": c_ms,
                "accuracy_search": {k: a_info[k] for k in _STATS}, "completeness_search": {k: c_info[k] for k in _STATS}})
    if reduce > 0:
        out.update({"reduce": float(reduce), "cloud_points_before": before[0], "reference_points_before": before[1],
                    "thin_rounds": [r for _, r in thinned], "thin_device_ms": [ms for ms, _ in thinned]})
    if neighbour_radius > 0:
        out.update({"neighbour_radius": float(neighbour_radius), "min_neighbours": int(min_neighbours),
                    "cloud_points_before_filter": before_filter, "filter_device_ms": filter_ms})
    if outlier_radius > 0:
        out.update({"outlier_radius": float(outlier_radius), "outlier_k": int(outlier_k), "outlier_std": float(outlier_std),
                    "outlier_threshold": o_info["threshold"], "cloud_points_before_outliers": before_outliers,
                    "outlier_device_ms": outlier_ms})
    if component_radius > 0:
        out.update({"component_radius": float(component_radius), "min_component": int(min_component),
                    "components": comp_info["components"], "cloud_points_before_components": before_components,
                    "component_device_ms": component_ms})
    if normal_radius > 0:
        out.update({"normal_radius": float(normal_radius), "normal_k": int(normal_k), "max_normal_angle": float(max_normal_angle),
                    "cloud_points_before_normals": before_normals, "normal_device_ms": normal_ms})
    return (out, indices) if return_indices else out


def check_outlier_args(pa, args, radius, k, std):
    """the three options of the statistical filter (this command's and batch's --fuse_* ones): they need each other, the
    radius goes through float32; off: radius 0.0, k 0, std 0.0"""
    r, kk, s = float(np.float32(getattr(args, radius))), getattr(args, k), getattr(args, std)
    if not (r >= 0 and np.isfinite(r)):
        pa.error("--%s must be >= 0 and finite (0: off)" % radius)
    if len({r > 0, kk is not None, s is not None}) != 1:
        pa.error("--%s, --%s and --%s need each other" % (radius, k, std))
    if kk is not None and not 1 <= kk <= 32:
        pa.error("--%s must be 1..32" % k)
    if s is not None and not (s >= 0 and np.isfinite(s)):
        pa.error("--%s must be >= 0 and finite" % std)
    setattr(args, radius, r), setattr(args, k, kk or 0), setattr(args, std, s or 0.0)


def check_component_args(pa, args, radius, size):
    """the two options of the component filter (this command's and batch's --fuse_* ones): they need each other, the
    radius goes through float32; off: radius 0.0, size 0"""
    r, n = float(np.float32(getattr(args, radius))), getattr(args, size)
    if not (r >= 0 and np.isfinite(r)):
        pa.error("--%s must be >= 0 and finite (0: off)" % radius)
    if (r > 0) != (n is not None):
        pa.error("--%s and --%s need each other" % (radius, size))
    if n is not None and not 0 <= n < 2 ** 31:
        pa.error("--%s must be 0 .. 2^31 - 1" % size)
    setattr(args, radius, r), setattr(args, size, n or 0)


def check_normal_args(pa, args, radius, k, angle, angle_optional=False):
    """the three options of the normal filter (this command's and batch's --fuse_* ones): they need each other, the radius
    goes through float32; off: radius 0.0, k 0, angle None.  angle_optional (--estimated_normals): the radius and k may come
    without the angle -- the estimate alone, nothing is dropped.  The filter is on iff the angle is given."""
    r, kk, a = float(np.float32(getattr(args, radius))), getattr(args, k), getattr(args, angle)
    if not (r >= 0 and np.isfinite(r)):
        pa.error("--%s must be >= 0 and finite (0: off)" % radius)
    if (r > 0) != (kk is not None) or (a is not None and not r > 0) or (a is None and r > 0 and not angle_optional):
        pa.error("--%s, --%s and --%s need each other" % (radius, k, angle))
    if kk is not None and not 3 <= kk <= 32:
        pa.error("--%s must be 3..32" % k)
    if a is not None and not (0 <= a <= 90):
        pa.error("--%s must be 0..90 degrees" % angle)
    setattr(args, radius, r), setattr(args, k, kk or 0)


def parse_args(argv):
    pa = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pa.add_argument("--cloud", required=True, help="the reconstruction, a PLY file (ascii or binary_little_endian)")
    pa.add_argument("--reference", required=True, help="the reference cloud, a PLY file")
    pa.add_argument("--max_dist", type=float, default=20.0, help="distances beyond it are discarded")
    pa.add_argument("--thresholds", default=",".join("%g" % t for t in THRESHOLDS),
                    help="comma separated distances of the precision / recall / F-score")
    pa.add_argument("--grid", type=int, default=0, help="cells along the longest axis (0: automatic, 1..256)")
    pa.add_argument("--reduce", type=float, default=0.0,
                    help="thin the cloud to this minimum point spacing before scoring (0: off; DTU uses 0.2)")
    pa.add_argument("--reduce_reference", action="store_true", help="with --reduce: thin the reference as well")
    pa.add_argument("--seed", type=int, default=0, help="with --reduce: seed of the order the points are visited in")
    pa.add_argument("--neighbour_radius", type=float, default=0.0,
                    help="with --min_neighbours: after --reduce, drop the cloud's points that have fewer than that many "
                         "other points within this radius (0: off)")
    pa.add_argument("--min_neighbours", type=int, default=None, help="with --neighbour_radius: the count a point needs to stay")
    pa.add_argument("--outlier_radius", type=float, default=0.0,
                    help="with --outlier_k and --outlier_std: after --reduce and --neighbour_radius, drop the cloud's points "
                         "whose mean distance to their k nearest neighbours within this radius is above the cloud's mean of it "
                         "by more than that many standard deviations, and those with fewer than k neighbours there (0: off)")
    pa.add_argument("--outlier_k", type=int, default=None, help="with --outlier_radius: the number of nearest neighbours, 1..32")
    pa.add_argument("--outlier_std", type=float, default=None, help="with --outlier_radius: the standard deviations allowed, >= 0")
    pa.add_argument("--component_radius", type=float, default=0.0,
                    help="with --min_component: after --reduce, --neighbour_radius and --outlier_radius, drop the cloud's "
                         "points whose connected component -- points joined where they lie within this radius of each other "
                         "-- has fewer than that many points (0: off)")
    pa.add_argument("--min_component", type=int, default=None,
                    help="with --component_radius: the points a component needs for them to stay")
    pa.add_argument("--normal_radius", type=float, default=0.0,
                    help="with --normal_k and --max_normal_angle: after the four other stages, drop the cloud's points whose "
                         "own normal (nx, ny, nz of --cloud) is more than that angle off the normal estimated from their k "
                         "nearest neighbours within this radius, and those with fewer than three neighbours there (0: off); "
                         "with --estimated_normals alone: the radius of the estimate")
    pa.add_argument("--normal_k", type=int, default=None, help="with --normal_radius: the number of nearest neighbours, 3..32")
    pa.add_argument("--max_normal_angle", type=float, default=None,
                    help="with --normal_radius: the angle allowed between a point's normal and the estimate, 0..90 degrees")
    pa.add_argument("--write_cloud", default=None,
                    help="write the cloud as it is scored, after --reduce, --neighbour_radius, --outlier_radius, "
                         "--component_radius and / or --normal_radius, as a binary PLY with "
                         "every vertex property of --cloud")
    pa.add_argument("--estimated_normals", action="store_true",
                    help="with --write_cloud, --normal_radius and --normal_k: the written nx, ny, nz are the normals estimated "
                         "on the scored cloud, along the file's own normals where it has them")
    pa.add_argument("--device", type=int, default=0)
    pa.add_argument("--output", default=None, help="write the report (JSON) here")
    args = pa.parse_args(argv)
    args.max_dist = float(np.float32(args.max_dist))  # a float field, like the solver's
    if not (args.max_dist > 0 and np.isfinite(args.max_dist)):
        pa.error("--max_dist must be > 0 and finite")
    try:
        args.thresholds = [float(t) for t in args.thresholds.split(",") if t]
    except ValueError:
        pa.error("--thresholds takes comma separated numbers")
    if not args.thresholds or any(not (t >= 0 and np.isfinite(t)) for t in args.thresholds):
        pa.error("--thresholds needs at least one distance, each >= 0 and finite")
    if not 0 <= args.grid <= 256:
        pa.error("--grid must be 0 (automatic) or 1..256")
    args.reduce = float(np.float32(args.reduce))
    if not (args.reduce >= 0 and np.isfinite(args.reduce)):
        pa.error("--reduce must be >= 0 and finite (0: off)")
    if args.reduce_reference and not args.reduce > 0:
        pa.error("--reduce_reference needs --reduce")
    if not 0 <= args.seed < 2 ** 32:
        pa.error("--seed must be 0 .. 2^32 - 1")
    args.neighbour_radius = float(np.float32(args.neighbour_radius))
    if not (args.neighbour_radius >= 0 and np.isfinite(args.neighbour_radius)):
        pa.error("--neighbour_radius must be >= 0 and finite (0: off)")
    if (args.neighbour_radius > 0) != (args.min_neighbours is not None):
        pa.error("--neighbour_radius and --min_neighbours need each other")
    if args.min_neighbours is not None and not 0 <= args.min_neighbours < 2 ** 31:
        pa.error("--min_neighbours must be 0 .. 2^31 - 1")
    args.min_neighbours = args.min_neighbours or 0
    check_outlier_args(pa, args, "outlier_radius", "outlier_k", "outlier_std")
    check_component_args(pa, args, "component_radius", "min_component")
    check_normal_args(pa, args, "normal_radius", "normal_k", "max_normal_angle", angle_optional=args.estimated_normals)
    if args.estimated_normals and (args.write_cloud is None or not args.normal_radius > 0):
        pa.error("--estimated_normals needs --write_cloud, --normal_radius and --normal_k")
    return args


def _with_estimated_normals(vertices, own, radius, k, device_id):
    """the vertices with nx, ny, nz (added behind the other properties where the file has none) set to the estimates on these
    very vertices, along the normals `own` where there are any, else with the largest component positive"""
    xyz = np.stack([vertices[c].astype(np.float32) for c in ("x", "y", "z")], axis=-1)
    est, _ = estimate_normals(xyz, radius, k, orient=0 if own is None else 2, guide=own, device_id=device_id)
    extra = [(c, "<f4") for c in ("nx", "ny", "nz") if c not in vertices.dtype.names]
    out = np.empty(len(vertices), dtype=np.dtype(vertices.dtype.descr + extra))
    for name in vertices.dtype.names:
        out[name] = vertices[name]
    for a, c in enumerate(("nx", "ny", "nz")):
        out[c] = est[:, a]
    return out


def main(argv=None):
    args = parse_args(argv)
    filtering = args.max_normal_angle is not None  # (else --normal_radius and --normal_k serve --estimated_normals alone)
    vertices = dmb.read_ply_vertices(args.cloud) if args.write_cloud or filtering else None  # (refused before anything is computed)
    has_normals = vertices is not None and all(c in (vertices.dtype.names or ()) for c in ("nx", "ny", "nz"))
    if filtering and not has_normals:
        raise ValueError("%s: --normal_radius compares the cloud's own normals: the file has no nx, ny, nz" % args.cloud)
    own = np.stack([vertices[c].astype(np.float32) for c in ("nx", "ny", "nz")], axis=-1) if has_normals else None
    report, indices = score(dmb.read_ply_xyz(args.cloud), dmb.read_ply_xyz(args.reference), args.max_dist, args.thresholds,
                            grid=args.grid, device_id=args.device, reduce=args.reduce, reduce_reference=args.reduce_reference,
                            seed=args.seed, neighbour_radius=args.neighbour_radius, min_neighbours=args.min_neighbours,
                            return_indices=True, outlier_radius=args.outlier_radius, outlier_k=args.outlier_k,
                            outlier_std=args.outlier_std, component_radius=args.component_radius,
                            min_component=args.min_component, **(dict(normal_radius=args.normal_radius, normal_k=args.normal_k,
                            max_normal_angle=args.max_normal_angle, cloud_normals=own) if filtering else {}))
    report.update({"cloud": args.cloud, "reference": args.reference})
    if args.write_cloud:
        scored = vertices if indices is None else vertices[indices]
        if args.estimated_normals:
            scored = _with_estimated_normals(scored, own if indices is None or own is None else own[indices], args.normal_radius,
                                             args.normal_k, args.device)
        dmb.write_ply_vertices(args.write_cloud, scored)
    if args.output:
        with open(args.output, "w") as f:
            json.dump(report, f, indent=1)
    print("accuracy %.4f (median %.4f, %d of %d points), completeness %.4f (median %.4f, %d of %d points), F-score %s at %s; "
          "%.2f + %.2f ms on device"
          % (report["accuracy"]["mean"], report["accuracy"]["median"], report["accuracy"]["found"], report["cloud_points"],
             report["completeness"]["mean"], report["completeness"]["median"], report["completeness"]["found"],
             report["reference_points"], "/".join("%.4f" % f for f in report["fscore"]),
             "/".join("%g" % t for t in args.thresholds), report["accuracy_device_ms"], report["completeness_device_ms"]))
    after_components = report.get("cloud_points_before_normals", report["cloud_points"])
    after_outliers = report.get("cloud_points_before_components", after_components)  # (what the earlier stages left)
    if args.reduce > 0:
        print("thinned to a spacing of %g first: cloud %d -> %d points, reference %d -> %d, %s rounds, %s ms on device"
              % (args.reduce, report["cloud_points_before"], report.get("cloud_points_before_filter", report.get("cloud_points_before_outliers", after_outliers)),
                 report["reference_points_before"],
                 report["reference_points"], "/".join("%d" % r for r in report["thin_rounds"]),
                 "/".join("%.2f" % m for m in report["thin_device_ms"])))
    if args.neighbour_radius > 0:
        print("points with fewer than %d others within %g dropped: cloud %d -> %d points, %.2f ms on device"
              % (args.min_neighbours, args.neighbour_radius, report["cloud_points_before_filter"],
                 report.get("cloud_points_before_outliers", after_outliers), report["filter_device_ms"]))
    if args.outlier_radius > 0:
        print("points with a mean distance above %g to their %d nearest within %g (%g standard deviations) dropped: cloud %d -> %d "
              "points, %.2f ms on device"
              % (report["outlier_threshold"], args.outlier_k, args.outlier_radius, args.outlier_std,
                 report["cloud_points_before_outliers"], after_outliers, report["outlier_device_ms"]))
    if args.component_radius > 0:
        print("%d components of points within %g of each other, those of fewer than %d points dropped: cloud %d -> %d points, "
              "%.2f ms on device"
              % (report["components"], args.component_radius, args.min_component, report["cloud_points_before_components"],
                 after_components, report["component_device_ms"]))
    if filtering:
        print("points whose normal is more than %g degrees off the one estimated from their %d nearest within %g dropped: cloud %d -> "
              "%d points, %.2f ms on device"
              % (args.max_normal_angle, args.normal_k, args.normal_radius, report["cloud_points_before_normals"],
                 report["cloud_points"], report["normal_device_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
