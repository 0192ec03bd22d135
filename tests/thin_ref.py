"""CPU restatement of the thinning contract (include/gipuma_hip.h), written from the contract, not from the
kernels: the hash of the order in numpy uint32, the sequential greedy pass in numpy float32 with a brute-force d2 against
the list of kept points, and a simulation of the synchronous rounds the kernels decide the same mask in, which gives the
round count.  Every - * + is on float32 operands in the contract's order, so the kernels
(gipuma_amd/csrc/gipuma_cloud.hip, namespace thin), whatever grid they walk, must equal it in every byte.  `thin_sparse` is
the round simulation on the edges a k-d tree hands over, for clouds the brute force is too slow for.  Not a test module."""
import collections

import numpy as np

from tests.cloud_ref import PAIR_MARGIN, squared

f32 = np.float32
u32 = np.uint32
ORDERS = {"hashed": 0, "index": 1}
Result = collections.namedtuple("Result", "keep kept dropped not_finite rounds undecided")


def mix32(h):
    """mix32 of gipuma_amd/csrc/pm_hash.h on a uint32 array, with uint32 wrap-around"""
    h = np.asarray(h, dtype=u32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> u32(16)
        h *= u32(0x7feb352d)
        h ^= h >> u32(15)
        h *= u32(0x846ca68b)
        h ^= h >> u32(16)
    return h


def prio(n, seed=0, order="hashed"):
    """prio(i) for i = 0 .. n - 1, uint32"""
    if ORDERS[order] == 1:
        return np.zeros(n, dtype=u32)
    with np.errstate(over="ignore"):
        salt = mix32(np.array([seed], dtype=u32) + u32(0x9E3779B9))[0]
        return mix32(salt ^ (np.arange(n, dtype=u32) + u32(0x85EBCA6B)))


def visiting_order(points, seed=0, order="hashed"):
    """the indices of the finite points in ascending key (prio(i), i)"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    pr = prio(len(p), seed, order)
    by_key = np.lexsort((np.arange(len(p)), pr))  # (the last key is the primary one)
    return by_key[np.isfinite(p).all(axis=1)[by_key]]


def _d2(a, b):
    """the contract's d2 of the point(s) a against the points b, float32"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx = a[..., 0] - b[..., 0]
        dy = a[..., 1] - b[..., 1]
        dz = a[..., 2] - b[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == f32
    return d2


def sequential(points, radius, seed=0, order="hashed"):
    """The contract as it is worded: visit the finite points in ascending key, keep a point iff no point kept before it
    has d2 <= r2.  Returns keep (uint8, one byte per point)."""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    keep = np.zeros(len(p), dtype=np.uint8)
    kept = np.empty((len(p), 3), dtype=f32)
    m = 0
    for i in visiting_order(p, seed, order):
        if m and (_d2(p[i], kept[:m]) <= r2).any():
            continue
        kept[m] = p[i]
        m += 1
        keep[i] = 1
    return keep


def lower_key_edges(points, radius, seed=0, order="hashed", chunk=512):
    """every pair (i, j), j != i, both finite, d2(i, j) <= r2 and key(j) < key(i): two int64 arrays (brute force)"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.isfinite(p).all(axis=1)
    rank = np.empty(len(p), dtype=np.int64)  # the position in the order of the keys: key(j) < key(i) iff rank[j] < rank[i]
    rank[np.lexsort((np.arange(len(p)), prio(len(p), seed, order)))] = np.arange(len(p))
    ei, ej = [], []
    for i0 in range(0, len(p), chunk):
        rows = np.arange(i0, min(i0 + chunk, len(p)))
        near = (_d2(p[rows, None, :], p[None, :, :]) <= r2) & ok[rows, None] & ok[None, :] & (rank[None, :] < rank[rows, None])
        i, j = np.nonzero(near)
        ei.append(rows[i])
        ej.append(j)
    return (np.concatenate(ei), np.concatenate(ej)) if ei else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def lower_key_edges_sparse(points, radius, seed=0, order="hashed", max_pairs=1 << 22):
    """`lower_key_edges` for large clouds of ORDINARY magnitudes: the same set of pairs (in another order), or None where
    the tree's pair list would exceed max_pairs (counted before any pair is listed).

    The candidate pairs come from scipy.spatial.cKDTree.query_pairs on the float64 coordinates of the finite points, with
    radius * (1 + PAIR_MARGIN); on those pairs only, d2 is computed in numpy float32 in the contract's order and
    compared with r2 as the brute force does.  Why no edge is missing: cloud_ref.nearest_sparse's argument, word for word
    -- a pair with float32 d2 <= r2 has a real distance below radius (1 + 2^-21) where nothing under- or overflows, and
    the tree is asked for twenty times that margin.  d2 is bitwise symmetric, so each unordered pair is tested once and
    directed from the higher key to the lower."""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.nonzero(np.isfinite(p).all(axis=1))[0]
    none = np.zeros(0, np.int64)
    if len(ok) < 2:
        return none, none
    rank = np.empty(len(p), dtype=np.int64)  # the position in the order of the keys: key(j) < key(i) iff rank[j] < rank[i]
    rank[np.lexsort((np.arange(len(p)), prio(len(p), seed, order)))] = np.arange(len(p))
    reach = float(radius) * (1.0 + PAIR_MARGIN)
    tree = cKDTree(p[ok].astype(np.float64))
    if (tree.count_neighbors(tree, reach) - len(ok)) // 2 > max_pairs:  # (ordered pairs, each point with itself included)
        return None
    pairs = tree.query_pairs(reach, output_type="ndarray")
    i, j = ok[pairs[:, 0]], ok[pairs[:, 1]]
    near = _d2(p[i], p[j]) <= r2
    i, j = i[near], j[near]
    swap = rank[i] < rank[j]
    return np.where(swap, j, i).astype(np.int64), np.where(swap, i, j).astype(np.int64)


def rounds(points, radius, seed=0, order="hashed", edges=None):
    """The synchronous rounds of DESIGN.md 15: in a round an undecided point is dropped if a lower-key neighbour was kept
    in an EARLIER round, else kept if no lower-key neighbour was undecided when the round began, else it stays.  Returns
    (keep uint8, the number of rounds, the undecided count after each round).  edges: lower_key_edges' result when the
    caller has it already."""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n = len(p)
    ei, ej = lower_key_edges(p, radius, seed, order) if edges is None else edges
    undecided = np.isfinite(p).all(axis=1)
    keep = np.zeros(n, dtype=bool)
    left = []
    while undecided.any():
        drop = np.bincount(ei, weights=keep[ej], minlength=n) > 0
        blocked = np.bincount(ei, weights=undecided[ej], minlength=n) > 0
        now_dropped = undecided & drop
        now_kept = undecided & ~drop & ~blocked
        assert (now_dropped | now_kept).any(), "a round decided nothing"
        keep |= now_kept
        undecided &= ~(now_dropped | now_kept)
        left.append(int(undecided.sum()))
    return keep.astype(np.uint8), len(left), left


def thin(points, radius, seed=0, order="hashed", edges=None):
    """Result(keep, kept, dropped, not_finite, rounds, undecided) -- what gipuma_hip_cloud_thin reports, from the round
    simulation; `sequential` is the contract it must equal (tests/test_cloud_thin.py compares the two on every case)."""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    keep, n_rounds, left = rounds(p, radius, seed, order, edges)
    finite = int(np.isfinite(p).all(axis=1).sum())
    kept = int(keep.sum())
    return Result(keep, kept, finite - kept, len(p) - finite, n_rounds, left)


def thin_sparse(points, radius, seed=0, order="hashed", max_pairs=1 << 22):
    """`thin` with the edges of lower_key_edges_sparse and the round simulation unchanged; None where that declines."""
    edges = lower_key_edges_sparse(points, radius, seed, order, max_pairs)
    return None if edges is None else thin(points, radius, seed, order, edges)
