"""CPU restatement of the k-nearest-neighbour contract and of the statistical outlier filter on it (DESIGN.md 17,
include/gipuma_hip.h), written from the contract, not from the kernel: a brute force in numpy float32 over every pair,
chunked over the queries, every - * + on float32 operands in the contract's order, each row ordered by (d2, j) with
np.lexsort -- so the kernel (gipuma_amd/csrc/gipuma_cloud.hip, namespace knn), whatever grid it walks and whatever order it
meets the records in, must equal it in every bit.  `knn_sparse` is the same contract on the pairs a k-d tree hands over, for
clouds the brute force is too slow for.  Not a test module."""
import collections

import numpy as np

from tests.cloud_ref import PAIR_MARGIN, squared
from tests.thin_ref import _d2

f32 = np.float32
MAX_K = 32
Result = collections.namedtuple("Result", "d2 idx m mean complete short not_finite")
Filter = collections.namedtuple("Filter", "keep mu sigma threshold short")


def _check(radius, k):
    if not (f32(radius) > 0 and np.isfinite(f32(radius))):
        raise ValueError("radius must be > 0 and finite")
    if int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError("k must be 1..32")


def mean_of(d2, m, k):
    """mean(i): the float32 sum of the roots in ascending slot order, starting from 0, over (float)k -- an explicit loop
    over the slots (np.sum adds pairwise: not the contract's order) -- or +inf where the list is short"""
    s = np.zeros(len(d2), dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(k):
            s = s + np.sqrt(d2[:, t])
        mean = s / f32(k)
    assert s.dtype == f32 and mean.dtype == f32
    return np.where(m == k, mean, f32(np.inf)).astype(f32)


def _result(p, d2, idx, m, k):
    ok = np.isfinite(p).all(axis=1)
    assert not m[~ok].any()
    complete = int((m == k).sum())
    return Result(d2, idx, m.astype(np.uint32), mean_of(d2, m, k), complete, int(ok.sum()) - complete, int(len(p) - ok.sum()))


def knn(points, radius, k, chunk=256):
    """Result(d2 (n, k) float32, idx (n, k) int32, m uint32, mean float32, complete, short, not_finite): the brute force"""
    _check(radius, k)
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n, r2 = len(p), squared(radius)
    ok = np.isfinite(p).all(axis=1)
    d2 = np.full((n, k), np.inf, dtype=f32)
    idx = np.full((n, k), -1, dtype=np.int32)
    m = np.zeros(n, dtype=np.int64)
    for i0 in range(0, n, chunk):
        rows = np.arange(i0, min(i0 + chunk, n))
        D = _d2(p[rows, None, :], p[None, :, :])
        with np.errstate(invalid="ignore"):
            near = (D <= r2) & ok[rows, None] & ok[None, :]
        near[np.arange(len(rows)), rows] = False  # j != i by index
        # neighbours first, then by (d2, j): a neighbour whose d2 is +inf (inf <= inf) still comes before every non-neighbour
        J = np.broadcast_to(np.arange(n), D.shape)
        order = np.lexsort((J, D, ~near), axis=-1)[:, :k]
        taken = np.take_along_axis(near, order, axis=1)
        width = order.shape[1]  # (n < k: fewer columns than slots)
        d2[rows, :width] = np.where(taken, np.take_along_axis(D, order, axis=1), f32(np.inf))
        idx[rows, :width] = np.where(taken, order, -1)
        m[rows] = np.minimum(near.sum(axis=1), k)
    return _result(p, d2, idx, m, k)


def shorter(r, points, k):
    """the Result for a smaller k from one for a larger k: the k smallest of the K smallest"""
    assert k <= r.d2.shape[1]
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    return _result(p, np.ascontiguousarray(r.d2[:, :k]), np.ascontiguousarray(r.idx[:, :k]), np.minimum(r.m.astype(np.int64), k), k)


def knn_sparse(points, radius, k, max_pairs=1 << 23):
    """`knn` for large clouds of ORDINARY magnitudes: the same Result, or None where the tree's pair list would exceed
    max_pairs (counted before any pair is listed).

    The candidate pairs come from scipy.spatial.cKDTree.query_pairs on the float64 coordinates of the finite points, with
    radius * (1 + PAIR_MARGIN); on those pairs only, d2 is computed in numpy float32 in the contract's order and compared
    with r2 as the brute force does.  Why no pair is missing: neighbours_ref.neighbours_sparse's argument, which is
    cloud_ref.nearest_sparse's, word for word.  d2 is bitwise symmetric, so each unordered pair is computed once and
    listed for both of its points; the lists are then ordered by (i, d2, j) and cut at k."""
    from scipy.spatial import cKDTree
    _check(radius, k)
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n, r2 = len(p), squared(radius)
    ok = np.nonzero(np.isfinite(p).all(axis=1))[0]
    d2 = np.full((n, k), np.inf, dtype=f32)
    idx = np.full((n, k), -1, dtype=np.int32)
    m = np.zeros(n, dtype=np.int64)
    if len(ok) >= 2:
        reach = float(radius) * (1.0 + PAIR_MARGIN)
        tree = cKDTree(p[ok].astype(np.float64))
        if (tree.count_neighbors(tree, reach) - len(ok)) // 2 > max_pairs:
            return None
        pairs = tree.query_pairs(reach, output_type="ndarray")
        a, b = ok[pairs[:, 0]], ok[pairs[:, 1]]
        D = _d2(p[a], p[b])
        near = D <= r2
        i, j, D = np.concatenate([a[near], b[near]]), np.concatenate([b[near], a[near]]), np.concatenate([D[near], D[near]])
        order = np.lexsort((j, D, i))
        i, j, D = i[order], j[order], D[order]
        counts = np.bincount(i, minlength=n)
        slot = np.arange(len(i)) - (np.cumsum(counts) - counts)[i]  # the rank inside the point's own list
        first = slot < k
        d2[i[first], slot[first]] = D[first]
        idx[i[first], slot[first]] = j[first]
        m = np.minimum(counts, k)
    return _result(p, d2, idx, m, k)


def drop_outliers(r, k, std_ratio, radius):
    """Filter(keep bool, mu, sigma, threshold, short) from a Result: S = {m == k}; mu, sigma the mean and the population
    standard deviation of mean(i) over S in numpy float64, from the float32 array in index order; t = float32(mu +
    std_ratio * sigma); keep(i) = i in S and mean(i) <= t.  S empty: nothing kept (mu, sigma, t are NaN).  Turned down, as
    cloud_eval.drop_outliers turns it down: a std_ratio that is negative or not finite, and a radius whose float32 square
    is +inf -- there a complete list may hold an overflowed d2 and its mean says +inf like a short one's."""
    if not (std_ratio >= 0 and np.isfinite(std_ratio)):
        raise ValueError("std_ratio must be >= 0 and finite")
    if not np.isfinite(squared(radius)):
        raise ValueError("the filter needs a radius whose float32 square is finite")
    S = r.m == k
    if not S.any():
        return Filter(np.zeros(len(r.m), dtype=bool), float("nan"), float("nan"), float("nan"), r.short)
    of = r.mean[S].astype(np.float64)
    mu, sigma = float(np.mean(of)), float(np.std(of))
    t = f32(mu + float(std_ratio) * sigma)
    return Filter(S & (r.mean <= t), mu, sigma, float(t), r.short)
