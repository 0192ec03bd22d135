"""CPU restatement of the cloud search's contract (include/gipuma_hip.h) in numpy float32, written from the
contract, not from the kernels: a brute-force search over every (query, target) pair, chunked over the queries, every
- * + on float32 operands in the contract's order -- so the kernels (gipuma_amd/csrc/gipuma_cloud.hip), whatever grid they
search with, must equal it in every bit.  `nearest_sparse` is the same contract on the candidate pairs a k-d tree hands
over, for clouds the brute force is too slow for.  Not a test module."""
import collections

import numpy as np

f32 = np.float32
Result = collections.namedtuple("Result", "d2 idx found none")
PAIR_MARGIN = 1e-5  # nearest_sparse's and thin_ref.thin_sparse's tree radius: the contract's radius times 1 + this


def squared(x):
    """r2: the float32 product, which may overflow to +inf or underflow to a subnormal or to 0"""
    with np.errstate(over="ignore", under="ignore"):
        return f32(x) * f32(x)


def nearest(queries, targets, max_dist, chunk=256):
    """queries (n_a, 3), targets (n_b, 3), max_dist: float32.  Result(d2 float32 (+inf: none), idx int32 (-1: none), found,
    none)."""
    a = np.ascontiguousarray(queries, dtype=f32).reshape(-1, 3)
    b = np.ascontiguousarray(targets, dtype=f32).reshape(-1, 3)
    r2 = squared(max_dist)
    d2_out = np.full(len(a), np.inf, dtype=f32)
    idx_out = np.full(len(a), -1, dtype=np.int32)
    b_ok = np.isfinite(b).all(axis=1)
    if len(b):
        for i0 in range(0, len(a), chunk):
            q = a[i0:i0 + chunk]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                dx = q[:, None, 0] - b[None, :, 0]
                dy = q[:, None, 1] - b[None, :, 1]
                dz = q[:, None, 2] - b[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                # (a d2 of +inf -- an overflow -- is no candidate even where r2 is +inf too: +inf means "none" only)
                cand = b_ok[None, :] & np.isfinite(d2) & (d2 <= r2) & np.isfinite(q).all(axis=1)[:, None]
            assert d2.dtype == f32
            masked = np.where(cand, d2, f32(np.inf))
            j = masked.argmin(axis=1)  # (the first, i.e. lowest, index that attains the minimum)
            hit = cand.any(axis=1)     # (a row without a candidate is all +inf: its argmin names no one and is not used)
            rows = np.nonzero(hit)[0]
            d2_out[i0 + rows] = masked[rows, j[rows]]
            idx_out[i0 + rows] = j[rows]
    found = int((idx_out >= 0).sum())
    return Result(d2_out, idx_out, found, len(a) - found)


def nearest_sparse(queries, targets, max_dist, max_pairs=1 << 23):
    """`nearest` for large clouds of ORDINARY magnitudes: the same Result, or None where the pair list would exceed
    max_pairs (counted by the trees before any pair is listed).

    The candidate pairs come from scipy.spatial.cKDTree on the float64 coordinates of the finite points, queried with
    max_dist * (1 + PAIR_MARGIN); on those pairs only, d2 is computed in numpy float32 in the contract's order, compared
    with r2 as `nearest` does, and the lexicographic minimum over (d2, j) is taken per query.

    Why no pair the brute force accepts is missing.  Let float32 d2 <= r2 for a pair of finite points whose coordinates,
    differences and squares neither underflow nor overflow.  d2 is a sum of non-negative terms and carries five roundings
    of relative size 2^-24 (an axis' difference enters squared and counts twice, its square once, the two sums once each),
    r2 = fl(max_dist^2) one more: the real squared distance is at most max_dist^2 (1 + 2^-24) / (1 - 2^-24)^5, the real
    distance below max_dist (1 + 2^-22) < max_dist (1 + 2^-21).  The tree measures in float64 (roundings of 2^-53) and is
    asked for 1 + 1e-5, twenty times 2^-21: every such pair is on its list.  Pairs on the list beyond r2 fail d2 <= r2 here as
    they do in the brute force.  The argument needs ordinary magnitudes; tests/test_cloud_scale.py checks the equality
    with `nearest` on every case of tests/test_cloud_eval.py."""
    from scipy.spatial import cKDTree
    a = np.ascontiguousarray(queries, dtype=f32).reshape(-1, 3)
    b = np.ascontiguousarray(targets, dtype=f32).reshape(-1, 3)
    r2 = squared(max_dist)
    d2_out = np.full(len(a), np.inf, dtype=f32)
    idx_out = np.full(len(a), -1, dtype=np.int32)
    qi = np.nonzero(np.isfinite(a).all(axis=1))[0]
    tj = np.nonzero(np.isfinite(b).all(axis=1))[0]
    if len(qi) and len(tj):
        reach = float(max_dist) * (1.0 + PAIR_MARGIN)
        ta, tb = cKDTree(a[qi].astype(np.float64)), cKDTree(b[tj].astype(np.float64))
        if ta.count_neighbors(tb, reach) > max_pairs:
            return None
        pairs = ta.sparse_distance_matrix(tb, reach, output_type="ndarray")
        i, j = qi[pairs["i"]], tj[pairs["j"]]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dx = a[i, 0] - b[j, 0]
            dy = a[i, 1] - b[j, 1]
            dz = a[i, 2] - b[j, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == f32
        cand = np.isfinite(d2) & (d2 <= r2)
        i, j, d2 = i[cand], j[cand], d2[cand]
        by = np.lexsort((j, d2, i))  # (the last key is the primary one: per query, ascending (d2, j))
        i, j, d2 = i[by], j[by], d2[by]
        first = np.ones(len(i), dtype=bool)
        first[1:] = i[1:] != i[:-1]
        d2_out[i[first]] = d2[first]
        idx_out[i[first]] = j[first]
    found = int((idx_out >= 0).sum())
    return Result(d2_out, idx_out, found, len(a) - found)
