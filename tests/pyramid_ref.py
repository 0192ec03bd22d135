"""numpy float32 restatement of the pyramid contract (include/gipuma_hip.h): the 2x2 mean of
gipuma_hip_downsample and the seed of gipuma_hip_seed_planes, plus the coarse-to-fine composition made of the
restatement and the CPU oracle.  Every operation is one float32 +, -, *, / or sqrt in the order the contract writes it
(numpy rounds each one correctly and fuses nothing), so the kernels have to agree in every bit.  Test infrastructure."""
import ctypes as C

import numpy as np

from gipuma_amd import abi, pyramid
from gipuma_amd.problem import AlgorithmParameters, GlobalState
from tests import oracle_lib
from tests.oracle_lib import OracleState

f32 = np.float32


def downsample2(a):
    """(rows, cols) or (rows, cols, 4) float32 -> the next pyramid level; a last odd row or column is dropped"""
    a = np.asarray(a, dtype=f32)
    r, c = a.shape[0] >> 1, a.shape[1] >> 1
    p00, p01 = a[0:2 * r:2, 0:2 * c:2], a[0:2 * r:2, 1:2 * c:2]
    p10, p11 = a[1:2 * r:2, 0:2 * c:2], a[1:2 * r:2, 1:2 * c:2]
    return np.floor(((p00 + p01) + (p10 + p11)) * f32(0.25) + f32(0.5)).astype(f32)


def _matvec(m, v):
    """matvecmul4 (config.h:163-176): rows of m times the vector field v (..., 3), sums left to right"""
    m = [f32(x) for x in m]
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([m[0] * x + m[1] * y + m[2] * z, m[3] * x + m[4] * y + m[5] * z, m[6] * x + m[7] * y + m[8] * z],
                    axis=-1).astype(f32)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def view_vectors(cam, rows, cols):
    """getViewVector_cu (gipuma.cu:80-89, 122-130) for every pixel"""
    xs, ys = np.meshgrid(np.arange(cols, dtype=f32), np.arange(rows, dtype=f32))
    pc = [f32(v) for v in cam.P_col34]
    pt = np.stack([xs - pc[0], ys - pc[1], np.full_like(xs, f32(1.0) - pc[2])], axis=-1)
    v = _matvec(cam.M_inv, pt)
    v = np.stack([v[..., k] - f32(cam.C[k]) for k in range(3)], axis=-1)
    ns = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    inv = f32(1.0) / np.sqrt(ns)
    return (v * inv[..., None]).astype(f32)


def plane_d(cam, n, depth, rows, cols):
    """getD_cu (gipuma.cu:96-111) for every pixel: n (rows, cols, 3), depth (rows, cols)"""
    xs, ys = np.meshgrid(np.arange(cols, dtype=f32), np.arange(rows, dtype=f32))
    pc = [f32(v) for v in cam.P_col34]
    pt = np.stack([depth * xs - pc[0], depth * ys - pc[1], depth - pc[2]], axis=-1)
    return -_dot(n, _matvec(cam.M_inv, pt))


def seed_planes(gs, prior, shift):
    """the contract of gipuma_hip_seed_planes on host arrays.  Returns (planes, cost, info): info holds the masks
    `fallback` (pixels that got the random plane) and `flipped` (usable pixels whose normal was negated)."""
    rows, cols = gs.rows, gs.cols
    prior = np.asarray(prior, dtype=f32)
    cam = gs.cameras.c_array[0]
    yi = np.minimum(np.arange(rows) >> shift, prior.shape[0] - 1)
    xi = np.minimum(np.arange(cols) >> shift, prior.shape[1] - 1)
    q = prior[yi][:, xi]
    nw, z = q[..., :3], q[..., 3]
    with np.errstate(all="ignore"):
        ok = np.isfinite(q).all(-1) & (f32(cam.depth_min) <= z) & (z <= f32(cam.depth_max)) & \
            ((nw[..., 0] * nw[..., 0] + nw[..., 1] * nw[..., 1]) + nw[..., 2] * nw[..., 2] > 0)
        Ri = list(cam.R_orig_inv)
        n = _matvec([Ri[0], Ri[3], Ri[6], Ri[1], Ri[4], Ri[7], Ri[2], Ri[5], Ri[8]], nw)
        flip = _dot(n, view_vectors(cam, rows, cols)) > 0
        n = np.where(flip[..., None], -n, n)
        d = plane_d(cam, n, z, rows, cols)
    planes = np.concatenate([n, d[..., None]], axis=-1).astype(f32)
    o = OracleState(gs)
    o.init_planes()  # the planes gipuma_hip_init_planes draws with the session's seed
    planes[~ok] = o.norm4[~ok]
    cost = o.eval_cost(planes)
    return planes, cost, dict(fallback=~ok, flipped=flip & ok)


def solve_seeded(gs, prior, shift, flavour=None):
    """restated seed + the oracle's sweeps (iterations numbered from 0) + its finalize"""
    L = oracle_lib.lib()
    if flavour is not None:
        L.gipuma_oracle_set_flavour(flavour)
    try:
        planes, cost, info = seed_planes(gs, prior, shift)
        o = OracleState(gs)
        o.norm4, o.cost = np.ascontiguousarray(planes), np.ascontiguousarray(cost)
        for it in range(gs.params.iterations):
            o.sweep(it, abi.BLACK)
            o.sweep(it, abi.RED)
        o.finalize()
    finally:
        if flavour is not None:
            L.gipuma_oracle_set_flavour(-1)
    return o.norm4, o.cost, info


def level_images(images, level):
    out = [np.asarray(im, dtype=f32) for im in images]
    for _ in range(level):
        out = [downsample2(im) for im in out]
    return out


def level_problem(gs, info, level, iterations):
    """host GlobalState of a synth problem (gs, info = synth.build_problem(...)) on a pyramid level: the restated
    planes, the cameras of S^level P, the finest level's view selection, depth range, parameters and seed"""
    cs = pyramid.level_cameras(info["P_matrices"], level, info["cam_scale"])
    ap = AlgorithmParameters(**{k: getattr(gs.params, k) for k in vars(gs.params)})
    ap.iterations = int(iterations)
    return GlobalState(level_images(gs.images, level), cs, gs.selected, ap, seed=int(gs.desc.seed))


def solve_hierarchy(gs, info, level_iterations, flavour=None):
    """pyramid.solve_view made of the restatement and the oracle; level_iterations coarsest first.
    Returns (norm4, cost, fallback share of the finest level's seed)."""
    levels = len(level_iterations)
    g = level_problem(gs, info, levels - 1, level_iterations[0])
    L = oracle_lib.lib()
    if flavour is not None:
        L.gipuma_oracle_set_flavour(flavour)
    try:
        n4, cost = OracleState(g).run()
    finally:
        if flavour is not None:
            L.gipuma_oracle_set_flavour(-1)
    share = 0.0
    for k in range(1, levels):
        g = level_problem(gs, info, levels - 1 - k, level_iterations[k])
        n4, cost, inf = solve_seeded(g, n4, 1, flavour)
        share = float(inf["fallback"].mean())
    return n4, cost, share
