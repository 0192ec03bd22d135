"""CPU restatement of the cloud search's contract (include/gipuma_hip.h) in numpy float32, written from the
contract, not from the kernels: a brute-force search over every (query, target) pair, chunked over the queries, every
- * + on float32 operands in the contract's order -- so the kernels (gipuma_amd/csrc/gipuma_cloud.hip), whatever grid they
search with, must equal it in every bit.  Not a test module."""
import collections

import numpy as np

f32 = np.float32
Result = collections.namedtuple("Result", "d2 idx found none")


def nearest(queries, targets, max_dist, chunk=256):
    """queries (n_a, 3), targets (n_b, 3), max_dist: float32.  Result(d2 float32 (+inf: none), idx int32 (-1: none), found,
    none)."""
    a = np.ascontiguousarray(queries, dtype=f32).reshape(-1, 3)
    b = np.ascontiguousarray(targets, dtype=f32).reshape(-1, 3)
    r2 = f32(max_dist) * f32(max_dist)
    d2_out = np.full(len(a), np.inf, dtype=f32)
    idx_out = np.full(len(a), -1, dtype=np.int32)
    b_ok = np.isfinite(b).all(axis=1)
    if len(b):
        for i0 in range(0, len(a), chunk):
            q = a[i0:i0 + chunk]
            with np.errstate(invalid="ignore", over="ignore"):
                dx = q[:, None, 0] - b[None, :, 0]
                dy = q[:, None, 1] - b[None, :, 1]
                dz = q[:, None, 2] - b[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                cand = b_ok[None, :] & (d2 <= r2) & np.isfinite(q).all(axis=1)[:, None]
            assert d2.dtype == f32
            masked = np.where(cand, d2, f32(np.inf))
            j = masked.argmin(axis=1)  # (the first, i.e. lowest, index that attains the minimum)
            hit = cand.any(axis=1)
            rows = np.nonzero(hit)[0]
            d2_out[i0 + rows] = masked[rows, j[rows]]
            idx_out[i0 + rows] = j[rows]
    found = int((idx_out >= 0).sum())
    return Result(d2_out, idx_out, found, len(a) - found)
