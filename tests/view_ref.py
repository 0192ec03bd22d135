"""The view geometry both CPU restatements share (tests/fusion_ref.py, tests/prior_ref.py), written from the contract
(include/gipuma_hip.h) in numpy float32: every + - * on float32 operands in the contract's order, no
fused multiply-adds.  k: gipuma_amd.cameras.view_constants of a camera.  Not a test module."""
import numpy as np


def valid(z, depth_min, depth_max):
    """finite, > 0, and inside depth_min / depth_max where those are > 0"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > 0)
        if depth_min > 0:
            ok &= z >= depth_min
        if depth_max > 0:
            ok &= z <= depth_max
    return ok


def rays(k, xf, yf):
    """r_i = (bp[i][0] x + bp[i][1] y) + bp[i][2]"""
    bp = k["bp"]
    return [(bp[i, 0] * xf + bp[i, 1] * yf) + bp[i, 2] for i in range(3)]


def backproject(k, z, xf, yf):
    """X_i = c[i] + z * ((bp[i][0] x + bp[i][1] y) + bp[i][2])"""
    return [k["c"][i] + z * r for i, r in enumerate(rays(k, xf, yf))]


def project(k, X):
    """h_i = ((P[i][0] X_0 + P[i][1] X_1) + P[i][2] X_2) + P[i][3]"""
    P = k["P"]
    return [((P[i, 0] * X[0] + P[i, 1] * X[1]) + P[i, 2] * X[2]) + P[i, 3] for i in range(3)]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
