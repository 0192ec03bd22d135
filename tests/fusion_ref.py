"""CPU restatement of the depth-map fusion contract (include/gipuma_hip.h) in numpy float32, written from
the contract, not from the kernels: every + - * / sqrt floor on float32 operands, in the contract's order, no fused
multiply-adds -- so the kernels (gipuma_amd/csrc/gipuma_fuse.hip) must equal it in every bit.  Not a test module."""
import collections

import numpy as np

from gipuma_amd import dmb
from tests.view_ref import backproject, dot, project, valid  # noqa: F401 (backproject: used by tests/test_fusion.py)

f32 = np.float32
# why a (pixel, partner) pair or a pixel is turned down, in the order the contract tests
REASONS = ("invalid", "used", "behind", "outside", "partner_invalid", "disparity", "normal", "too_few")


Result = collections.namedtuple("Result", "points per_view used tally emitted")


def fuse(norm4s, grays, consts, disp_thresh, cos_t, num_consistent, depth_min=-1.0, depth_max=-1.0):
    """norm4s: V (rows, cols, 4) float32; grays: (rows, cols) or None; consts: gipuma_amd.cameras.view_constants per view;
    cos_t: float32 (gipuma_amd.fusion.cos_threshold).  Returns Result(points (PLY vertices, (view, y, x) order),
    per_view counts, used (V, rows, cols) uint8, tally {reason: count}, emitted (V, rows, cols) uint8: the pixels each view
    emitted)."""
    V = len(norm4s)
    rows, cols = norm4s[0].shape[:2]
    disp_thresh, cos_t = f32(disp_thresh), f32(cos_t)
    depth_min, depth_max = f32(depth_min), f32(depth_max)
    planes = [np.ascontiguousarray(n, dtype=f32).reshape(-1, 4) for n in norm4s]
    gplanes = [None if g is None else np.ascontiguousarray(g, dtype=f32).reshape(-1) for g in grays]
    used = np.zeros((V, rows * cols), dtype=np.uint8)
    emitted = np.zeros((V, rows * cols), dtype=np.uint8)
    tally = collections.Counter({r: 0 for r in REASONS})
    yy, xx = np.mgrid[0:rows, 0:cols]
    xs, ys = xx.reshape(-1).astype(f32), yy.reshape(-1).astype(f32)
    out, per_view = [], []
    for i in range(V):
        z_all = planes[i][:, 3]
        val = valid(z_all, depth_min, depth_max)
        tally["invalid"] += int((~val).sum())
        tally["used"] += int((val & (used[i] != 0)).sum())
        idx = np.nonzero(val & (used[i] == 0))[0]
        if not len(idx):  # (every tally of a pair counts over idx: nothing to add, nothing to mark)
            out.append(np.zeros(0, dtype=dmb._PLY_VERTEX))
            per_view.append(0)
            continue
        z = z_all[idx]
        n = [planes[i][idx, k] for k in range(3)]
        X = backproject(consts[i], z, xs[idx], ys[idx])
        S = list(X)
        N = list(n)
        SG = gplanes[i][idx].copy() if gplanes[i] is not None else np.zeros(len(idx), dtype=f32)
        count = np.zeros(len(idx), dtype=np.int64)
        hits = []
        for j in range(V):
            if j == i:
                continue
            fb = consts[j]["fb"]
            h = project(consts[j], X)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                front = h[2] > 0
                qx = np.floor(h[0] / h[2] + f32(0.5))
                qy = np.floor(h[1] / h[2] + f32(0.5))
                inside = front & (qx >= 0) & (qx <= f32(cols - 1)) & (qy >= 0) & (qy <= f32(rows - 1))
            tally["behind"] += int((~front).sum())
            tally["outside"] += int((front & ~inside).sum())
            qxs, qys = np.where(inside, qx, f32(0)), np.where(inside, qy, f32(0))
            q = qys.astype(np.int64) * cols + qxs.astype(np.int64)
            m = planes[j][q]
            pv = inside & valid(m[:, 3], depth_min, depth_max)
            tally["partner_invalid"] += int((inside & ~pv).sum())
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                dok = np.abs(fb / h[2] - fb / m[:, 3]) < disp_thresh
                nok = dot(n, [m[:, k] for k in range(3)]) > cos_t
            tally["disparity"] += int((pv & ~dok).sum())
            tally["normal"] += int((pv & dok & ~nok).sum())
            ok = pv & dok & nok
            count += ok
            with np.errstate(invalid="ignore", over="ignore"):
                Xj = backproject(consts[j], m[:, 3], qxs, qys)
                for k in range(3):
                    S[k] = np.where(ok, S[k] + Xj[k], S[k])
                    N[k] = np.where(ok, N[k] + m[:, k], N[k])
                if gplanes[j] is not None:
                    SG = np.where(ok, SG + gplanes[j][q], SG)
            hits.append((j, ok, q))
        emit = count >= num_consistent
        tally["too_few"] += int((~emit).sum())
        e = np.nonzero(emit)[0]
        k1 = (count[e] + 1).astype(f32)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            length = np.sqrt(dot([N[k][e] for k in range(3)], [N[k][e] for k in range(3)]))
            v = np.zeros(len(e), dtype=dmb._PLY_VERTEX)
            for k, name in enumerate(("x", "y", "z")):
                v[name] = S[k][e] / k1
            for k, name in enumerate(("nx", "ny", "nz")):
                v[name] = N[k][e] / length
            g = np.minimum(f32(255), np.floor(SG[e] / k1 + f32(0.5))).astype(np.uint8)
        v["red"] = v["green"] = v["blue"] = g
        for j, ok, q in hits:
            used[j][q[emit & ok]] = 1
        emitted[i][idx[e]] = 1
        out.append(v)
        per_view.append(len(e))
    return Result(np.concatenate(out), per_view, used.reshape(V, rows, cols), dict(tally),
                  emitted.reshape(V, rows, cols))
