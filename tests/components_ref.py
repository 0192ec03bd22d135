"""CPU restatement of the connected components' contract (include/gipuma_hip.h), written from the contract,
not from the kernels: a brute force in numpy float32 over every pair, chunked, every - * + on float32 operands in the
contract's order, gives the edge list, and a plain sequential union-find, written out below, the components -- so the
kernels (gipuma_amd/csrc/gipuma_components.hip), whatever grid they walk and however their unions interleave, must equal it
in every byte.  `components_sparse` is the same union-find on the pairs a k-d tree hands over, for clouds the brute force is
too slow for.  Not a test module."""
import collections

import numpy as np

from tests.cloud_ref import PAIR_MARGIN, squared
from tests.thin_ref import _d2

f32 = np.float32
Result = collections.namedtuple("Result", "label size keep kept dropped not_finite components")


def union_find(n, edges_i, edges_j):
    """parent[] after a sequential union-find over the edges (i, j), flattened: parent[x] is the root of x.  The smaller
    root becomes the parent, so a root is the smallest member of its set -- the label itself."""
    parent = list(range(n))
    for a, b in zip(edges_i.tolist(), edges_j.tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)
    for x in range(n):  # (parent[x] <= x: the entries below x are already roots' indices)
        parent[x] = parent[parent[x]]
    return np.asarray(parent, dtype=np.int64)


def from_edges(p, edges_i, edges_j, min_size):
    """what gipuma_hip_cloud_components reports, from the edge list over the caller's indices (finite points only)"""
    if min_size < 0:
        raise ValueError("min_size >= 0")
    n = len(p)
    ok = np.isfinite(p).all(axis=1)
    assert ok[edges_i].all() and ok[edges_j].all()
    root = union_find(n, edges_i, edges_j)
    assert (root <= np.arange(n)).all() and np.array_equal(root[root], root)
    label = np.where(ok, root, -1).astype(np.int32)
    size = np.where(ok, np.bincount(root[ok], minlength=n)[root] if n else 0, 0).astype(np.uint32)
    keep = ok & (size >= min_size)
    kept, finite = int(keep.sum()), int(ok.sum())
    return Result(label, size, keep.astype(np.uint8), kept, finite - kept, n - finite, int((ok & (root == np.arange(n))).sum()))


def edges(points, radius, chunk=512):
    """the brute force's edges (i < j), both ends finite and d2 <= r2"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.isfinite(p).all(axis=1)
    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for i0 in range(0, len(p), chunk):
        rows = np.arange(i0, min(i0 + chunk, len(p)))
        with np.errstate(invalid="ignore", over="ignore"):
            near = (_d2(p[rows, None, :], p[None, :, :]) <= r2) & ok[rows, None] & ok[None, :]
        a, b = np.nonzero(near)
        a = rows[a]
        ii.append(a[a < b]), jj.append(b[a < b])
    return np.concatenate(ii), np.concatenate(jj)


def components(points, radius, min_size=0):
    """Result(label int32, size uint32, keep uint8, kept, dropped, not_finite, components): the brute force"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    return from_edges(p, *edges(p, radius), min_size)


def sparse_edges(points, radius, max_pairs=1 << 23):
    """`edges` for clouds of ORDINARY magnitudes, or None where the tree's pair list would exceed max_pairs.  The
    candidate pairs come from scipy.spatial.cKDTree.query_pairs on the float64 coordinates of the finite points, with
    radius * (1 + PAIR_MARGIN); on those pairs only, d2 is computed in numpy float32 in the contract's order and compared
    with r2 as the brute force does.  Why no pair is missing: cloud_ref.nearest_sparse's argument -- a pair with float32
    d2 <= r2 has a real distance below radius (1 + 2^-21) where nothing under- or overflows, and the tree is asked for
    twenty times that margin."""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    r2 = squared(radius)
    ok = np.nonzero(np.isfinite(p).all(axis=1))[0]
    if len(ok) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    reach = float(radius) * (1.0 + PAIR_MARGIN)
    tree = cKDTree(p[ok].astype(np.float64))
    if (tree.count_neighbors(tree, reach) - len(ok)) // 2 > max_pairs:
        return None
    pairs = tree.query_pairs(reach, output_type="ndarray")
    i, j = ok[pairs[:, 0]], ok[pairs[:, 1]]
    near = _d2(p[i], p[j]) <= r2
    i, j = i[near], j[near]
    return np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)


def components_sparse(points, radius, min_size=0, max_pairs=1 << 23):
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    e = sparse_edges(p, radius, max_pairs)
    return None if e is None else from_edges(p, *e, min_size)


def csgraph_labels(points, edges_i, edges_j):
    """(label int32) re-derived as minima from scipy.sparse.csgraph.connected_components' partition of the same edges, or
    None where scipy.sparse does not import: a second opinion on the union-find, on the partition only"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n = len(p)
    ok = np.isfinite(p).all(axis=1)
    if n == 0:
        return np.zeros(0, np.int32)
    _, part = connected_components(coo_matrix((np.ones(len(edges_i), np.int8), (edges_i, edges_j)), shape=(n, n)), directed=False)
    first = np.full(part.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, part, np.arange(n))
    return np.where(ok, first[part], -1).astype(np.int32)
