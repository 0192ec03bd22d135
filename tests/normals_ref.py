"""CPU restatement of the normal-estimation contract (include/gipuma_hip.h), written from the contract, not
from the kernel.  The lists are tests/knn_ref.py's (imported: the brute force, or the k-d tree's pairs for large clouds); the
rest is numpy float64 `+ - * / sqrt` in the contract's order, as explicit loops over the slots and over the rotations, every
point at once -- so the kernel (gipuma_amd/csrc/gipuma_normals.hip), whatever grid it walks, must equal it in every bit.  Not a
test module."""
import collections

import numpy as np

from tests import knn_ref

f32, f64 = np.float32, np.float64
MIN_K, MAX_K = 3, 32
SWEEPS = 6
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))  # (p, q, r): r the third index
TRIANGLE = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the six entries of C, as `scatter` holds them
CANONICAL_NAN = np.uint64(0x7ff8000000000000)
Result = collections.namedtuple("Result", "normal variation m scatter estimated short not_finite flipped is_estimated is_flipped w vector")


def _check(radius, k, orient, viewpoint, guide):
    if not (f32(radius) > 0 and np.isfinite(f32(radius))):
        raise ValueError("radius must be > 0 and finite")
    if int(k) != k or not MIN_K <= k <= MAX_K:
        raise ValueError("k must be 3..32")
    if orient not in (0, 1, 2):
        raise ValueError("orient must be 0, 1 or 2")
    if orient == 1 and (viewpoint is None or not np.isfinite(np.asarray(viewpoint, dtype=f32)).all()):
        raise ValueError("orient 1 needs a finite viewpoint")
    if orient == 2 and guide is None:
        raise ValueError("orient 2 needs the guide normals")


def scatter_of(p, idx, m, k):
    """(C (n, 3, 3) float64, rows with m >= 3 only; the others 0): d in float32, widened; S1, S2 in slot order from 0"""
    n = len(p)
    s1 = np.zeros((n, 3), dtype=f64)
    s2 = np.zeros((n, 3, 3), dtype=f64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(k):
            on = s < m
            j = np.where(on, idx[:, s], 0)
            d = p[j] - p  # float32
            assert d.dtype == f32
            d = np.where(on[:, None], d, f32(0)).astype(f64)
            # (a slot that is not filled adds nothing; adding +0.0 changes no bit of a sum that started from +0.0)
            s1 = np.where(on[:, None], s1 + d, s1)
            for a, b in TRIANGLE:
                s2[:, a, b] = np.where(on, s2[:, a, b] + d[:, a] * d[:, b], s2[:, a, b])
        M = (m.astype(np.int64) + 1).astype(f64)
        C = np.zeros((n, 3, 3), dtype=f64)
        for a, b in TRIANGLE:
            C[:, a, b] = M * s2[:, a, b] - s1[:, a] * s1[:, b]
    C[m < MIN_K] = 0.0
    return C


def jacobi(C, sweeps=SWEEPS):
    """(w (n, 3), V (n, 3, 3)) of the upper triangles C (n, 3, 3): the contract's cyclic Jacobi, rotation by rotation"""
    n = len(C)
    A = {ab: C[:, ab[0], ab[1]].copy() for ab in TRIANGLE}
    V = np.zeros((n, 3, 3), dtype=f64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    key = lambda a, b: (min(a, b), max(a, b))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[(p, q)], A[key(r, p)], A[key(r, q)]
                on = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                u = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -u, u)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                A[(p, p)] = np.where(on, app - h, app)
                A[(q, q)] = np.where(on, aqq + h, aqq)
                A[(p, q)] = np.where(on, 0.0, apq)
                A[key(r, p)] = np.where(on, c * arp - s * arq, arp)
                A[key(r, q)] = np.where(on, s * arp + c * arq, arq)
                for i in range(3):
                    x, y = V[:, i, p].copy(), V[:, i, q].copy()
                    V[:, i, p] = np.where(on, c * x - s * y, x)
                    V[:, i, q] = np.where(on, s * x + c * y, y)
    return np.stack([A[(0, 0)], A[(1, 1)], A[(2, 2)]], axis=1), V


def _rule0(nrm):
    """flip iff the component of largest magnitude, the lowest axis on a tie, is negative"""
    big = nrm[:, 0].copy()
    for a in (1, 2):
        take = np.abs(nrm[:, a]) > np.abs(big)
        big = np.where(take, nrm[:, a], big)
    return big < 0


def from_lists(points, idx, m, k, orient=0, viewpoint=None, guide=None, sweeps=SWEEPS):
    """Result from the lists (idx (n, k) int32, m (n,)) of knn_ref"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    n = len(p)
    m = np.asarray(m).astype(np.int64)
    ok = np.isfinite(p).all(axis=1)
    C = scatter_of(p, idx, m, k)
    with np.errstate(all="ignore"):
        trace = (C[:, 0, 0] + C[:, 1, 1]) + C[:, 2, 2]
        est = (m >= MIN_K) & (trace > 0.0) & (trace < np.inf)
        w, V = jacobi(np.where(est[:, None, None], C, 0.0), sweeps)
        b1 = w[:, 1] < w[:, 0]
        w1 = np.where(b1, w[:, 1], w[:, 0])
        b2 = w[:, 2] < w1
        we = np.where(b2, w[:, 2], w1)
        e = np.where(b2, 2, np.where(b1, 1, 0))
        vector = np.take_along_axis(V, e[:, None, None].repeat(3, axis=1), axis=2)[:, :, 0]  # (float64, before the sign)
        nrm = vector.astype(f32)
        variation = (np.where(we > 0.0, we, 0.0) / ((w[:, 0] + w[:, 1]) + w[:, 2])).astype(f32)
        n64 = nrm.astype(f64)
        dot = np.zeros(n, dtype=f64)
        if orient == 1:
            v = np.asarray(viewpoint, dtype=f32).astype(f64)
            q = p.astype(f64)
            dot = (n64[:, 0] * (v[0] - q[:, 0]) + n64[:, 1] * (v[1] - q[:, 1])) + n64[:, 2] * (v[2] - q[:, 2])
        if orient == 2:
            g = np.ascontiguousarray(guide, dtype=f32).reshape(-1, 3).astype(f64)
            dot = (n64[:, 0] * g[:, 0] + n64[:, 1] * g[:, 1]) + n64[:, 2] * g[:, 2]
        by_dot = (dot != 0.0) & (np.abs(dot) < np.inf)
        flip = np.where(by_dot, dot < 0.0, _rule0(nrm)) & est
    nrm = np.where(flip[:, None], -nrm, nrm)
    nrm[~est] = 0.0
    variation[~est] = np.inf
    scatter = np.stack([C[:, a, b] for a, b in TRIANGLE], axis=1)
    bits = scatter.view(np.uint64).copy()
    bits[np.isnan(scatter)] = CANONICAL_NAN
    scatter = bits.view(f64)
    estimated = int(est.sum())
    return Result(nrm.astype(f32), variation.astype(f32), m.astype(np.uint32), scatter, estimated, int(ok.sum()) - estimated,
                  int(n - ok.sum()), int(flip.sum()), est, flip, w, vector)


def normals(points, radius, k, orient=0, viewpoint=None, guide=None, lists=None, sweeps=SWEEPS):
    """Result(normal (n, 3) float32, variation float32, m uint32, scatter (n, 6) float64, estimated, short, not_finite, flipped,
    the masks, the eigenvalues, the float64 eigenvector before the sign): the brute force's lists (or `lists`, a knn_ref.Result at this k), then the contract"""
    _check(radius, k, orient, viewpoint, guide)
    r = lists if lists is not None else knn_ref.knn(points, radius, k)
    assert r.idx.shape[1] == k
    return from_lists(points, r.idx, r.m, k, orient, viewpoint, guide, sweeps)


def normals_sparse(points, radius, k, orient=0, viewpoint=None, guide=None):
    """`normals` on knn_ref.knn_sparse's lists (large clouds of ordinary magnitudes), or None where that gives None"""
    _check(radius, k, orient, viewpoint, guide)
    r = knn_ref.knn_sparse(points, radius, k)
    return None if r is None else from_lists(points, r.idx, r.m, k, orient, viewpoint, guide)


def agreement(estimated, given):
    """|n . g| / |g| per point in float64, 0 where the estimate is the zero vector or g is zero or not finite"""
    e = np.ascontiguousarray(estimated, dtype=f32).reshape(-1, 3).astype(f64)
    g = np.ascontiguousarray(given, dtype=f32).reshape(-1, 3).astype(f64)
    with np.errstate(all="ignore"):
        norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        dot = np.abs((e[:, 0] * g[:, 0] + e[:, 1] * g[:, 1]) + e[:, 2] * g[:, 2])
        a = dot / norm
    bad = ~np.isfinite(g).all(axis=1) | ~(norm > 0) | ~np.isfinite(norm) | ~e.any(axis=1) | ~np.isfinite(a)
    return np.where(bad, 0.0, a)


def keep_agreeing(r, given, max_angle_deg):
    """the filter's mask: estimated and agreement >= float32(cos(max_angle_deg pi / 180)), the cosine made in double"""
    if not (0 <= max_angle_deg <= 90):
        raise ValueError("max_angle_deg must be 0..90")
    cos_t = f32(np.cos(float(max_angle_deg) * np.pi / 180.0))
    return r.is_estimated & (agreement(r.normal, given) >= float(cos_t))
