"""CPU restatement of the neighbour count's contract (include/gipuma_hip.h), written from the contract, not
from the kernel: a brute force in numpy float32 over every pair, chunked over the queries, every - * + on float32 operands
in the contract's order -- so the kernel (gipuma_amd/csrc/gipuma_cloud.hip, namespace support), whatever grid it walks,
must equal it in every bit.  `neighbours_sparse` is the same contract on the pairs a k-d tree hands over, for clouds the
brute force is too slow for.  Not a test module."""
import collections

import numpy as np

from tests.cloud_ref import PAIR_MARGIN, squared
from tests.thin_ref import _d2

f32 = np.float32
Result = collections.namedtuple("Result", "count keep kept dropped not_finite saturated exact")


def from_exact(p, exact, min_neighbours, max_count):
    """what gipuma_hip_cloud_neighbours reports, from the exact counts (int64, 0 for a point that is not finite)"""
    if min_neighbours < 0 or max_count < 0 or (max_count > 0 and min_neighbours > max_count):
        raise ValueError("min_neighbours >= 0, max_count >= 0, and min_neighbours <= max_count where that is > 0")
    ok = np.isfinite(p).all(axis=1)
    assert not exact[~ok].any()
    count = np.minimum(exact, max_count) if max_count > 0 else exact
    keep = ok & (count >= min_neighbours)
    saturated = int((ok & (exact >= max_count)).sum()) if max_count > 0 else 0
    kept, finite = int(keep.sum()), int(ok.sum())
    return Result(count.astype(np.uint32), keep.astype(np.uint8), kept, finite - kept, len(p) - finite, saturated, exact)


def neighbours(points, radius, min_neighbours=0, max_count=0, chunk=512):
    """Result(count uint32, keep uint8, kept, dropped, not_finite, saturated, exact int64): the brute force"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.isfinite(p).all(axis=1)
    exact = np.zeros(len(p), dtype=np.int64)
    for i0 in range(0, len(p), chunk):
        rows = np.arange(i0, min(i0 + chunk, len(p)))
        near = (_d2(p[rows, None, :], p[None, :, :]) <= r2) & ok[rows, None] & ok[None, :]
        # (j != i by index: a finite point is within any radius of itself -- d2 = 0 <= r2 -- and is taken out again)
        assert near[np.arange(len(rows)), rows][ok[rows]].all()
        exact[rows] = near.sum(axis=1) - ok[rows]
    return from_exact(p, exact, min_neighbours, max_count)


def neighbours_sparse(points, radius, min_neighbours=0, max_count=0, max_pairs=1 << 23):
    """`neighbours` for large clouds of ORDINARY magnitudes: the same Result, or None where the tree's pair list would
    exceed max_pairs (counted before any pair is listed).

    The candidate pairs come from scipy.spatial.cKDTree.query_pairs on the float64 coordinates of the finite points, with
    radius * (1 + PAIR_MARGIN); on those pairs only, d2 is computed in numpy float32 in the contract's order and compared
    with r2 as the brute force does.  Why no pair is missing: cloud_ref.nearest_sparse's argument, word for word -- a pair
    with float32 d2 <= r2 has a real distance below radius (1 + 2^-21) where nothing under- or overflows, and the tree is
    asked for twenty times that margin.  d2 is bitwise symmetric, so each unordered pair is tested once and counts for
    both of its points."""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.nonzero(np.isfinite(p).all(axis=1))[0]
    exact = np.zeros(len(p), dtype=np.int64)
    if len(ok) >= 2:
        reach = float(radius) * (1.0 + PAIR_MARGIN)
        tree = cKDTree(p[ok].astype(np.float64))
        if (tree.count_neighbors(tree, reach) - len(ok)) // 2 > max_pairs:  # (ordered pairs, each point with itself included)
            return None
        pairs = tree.query_pairs(reach, output_type="ndarray")
        i, j = ok[pairs[:, 0]], ok[pairs[:, 1]]
        near = _d2(p[i], p[j]) <= r2
        exact = np.bincount(i[near], minlength=len(p)) + np.bincount(j[near], minlength=len(p))
    return from_exact(p, exact.astype(np.int64), min_neighbours, max_count)
