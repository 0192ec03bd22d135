"""CPU restatement of the cross-view prior (include/gipuma_hip.h) in numpy float32, written from the
contract, not from the kernels: every + - * / floor on float32 operands in the contract's order, no fused multiply-adds,
the z-buffer as an unsigned 64-bit minimum -- so the kernels (gipuma_amd/csrc/gipuma_prior.hip) must equal it in every
bit.  Not a test module."""
import collections

import numpy as np

from tests.view_ref import backproject, dot, project, rays, valid

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# why a source pixel is left out of the splat, in the order the contract tests
REASONS = ("invalid_depth", "bad_normal", "cost", "behind", "outside", "back_facing")


Result = collections.namedtuple("Result", "prior counts zbuf tally info")


def grazing_cos(degrees=80.0):
    """f32(cos(degrees)) computed in double (what gipuma_amd.prior hands to the library)"""
    import math
    return f32(math.cos(float(degrees) * math.pi / 180.0))


def prior_from_views(target, source_norm4s, sources, depth_min=-1.0, depth_max=-1.0, costs=None, max_cost=None,
                     grazing=None, fill=True):
    """target / sources: gipuma_amd.cameras.view_constants of the cameras; source_norm4s: (rows, cols, 4) float32 result
    planes; costs: None or one (rows, cols) plane per source.  Returns Result(prior (rows, cols, 4), counts
    [direct, filled, empty], zbuf, tally {reason: source pixels}, info dict(cls (rows, cols) 0 / 1 / 2, source (rows,
    cols) winner's ordinal or -1, grazing (rows, cols) bool: the plane intersection was turned down))."""
    S = len(source_norm4s)
    rows, cols = source_norm4s[0].shape[:2]
    npix = rows * cols
    assert S * npix < 2 ** 32
    depth_min, depth_max = f32(depth_min), f32(depth_max)
    g = grazing_cos() if grazing is None else f32(grazing)
    g2 = g * g
    planes = [np.ascontiguousarray(n, dtype=f32).reshape(-1, 4) for n in source_norm4s]
    yy, xx = np.mgrid[0:rows, 0:cols]
    xs, ys = xx.reshape(-1).astype(f32), yy.reshape(-1).astype(f32)
    zbuf = np.full(npix, EMPTY, dtype=np.uint64)
    tally = collections.Counter({r: 0 for r in REASONS})
    with np.errstate(all="ignore"):
        for k in range(S):
            m = planes[k]
            n, z = [m[:, i] for i in range(3)], m[:, 3]
            ok = valid(z, depth_min, depth_max)
            tally["invalid_depth"] += int((~ok).sum())
            nok = np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2]) & (dot(n, n) > 0)
            tally["bad_normal"] += int((ok & ~nok).sum())
            ok &= nok
            if costs is not None:
                cok = np.ascontiguousarray(costs[k], dtype=f32).reshape(-1) <= f32(max_cost)
                tally["cost"] += int((ok & ~cok).sum())
                ok &= cok
            X = backproject(sources[k], z, xs, ys)
            h = project(target, X)
            front = (h[2] > 0) & valid(h[2], depth_min, depth_max)
            tally["behind"] += int((ok & ~front).sum())
            ok &= front
            qx = np.floor(h[0] / h[2] + f32(0.5))
            qy = np.floor(h[1] / h[2] + f32(0.5))
            inside = (qx >= 0) & (qx < f32(cols)) & (qy >= 0) & (qy < f32(rows))
            tally["outside"] += int((ok & ~inside).sum())
            ok &= inside
            r = rays(target, qx, qy)
            facing = dot(n, r) < 0
            tally["back_facing"] += int((ok & ~facing).sum())
            ok &= facing
            idx = np.nonzero(ok)[0]
            key = (h[2][idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(k * npix) + idx.astype(np.uint64))
            q = qy[idx].astype(np.int64) * cols + qx[idx].astype(np.int64)
            np.minimum.at(zbuf, q, key)
        # resolve
        zb = zbuf.reshape(rows, cols)
        key = zb.copy()
        cls = np.zeros((rows, cols), dtype=np.int8)
        if fill:
            pad = np.full((rows + 2, cols + 2), EMPTY, dtype=np.uint64)
            pad[1:-1, 1:-1] = zb
            best = np.full((rows, cols), EMPTY, dtype=np.uint64)
            for dy in (0, 1, 2):
                for dx in (0, 1, 2):
                    if dy == 1 and dx == 1:
                        continue
                    best = np.minimum(best, pad[dy:dy + rows, dx:dx + cols])
            hole = zb == EMPTY
            key[hole] = best[hole]
            cls[hole] = 1
        empty = key == EMPTY
        cls[empty] = 2
        key = key.reshape(-1)
        low = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        high = (key >> np.uint64(32)).astype(np.uint32).view(f32)
        have = ~empty.reshape(-1)
        low = np.where(have, low, 0)
        ks, idx = low // npix, low % npix
        m = np.stack(planes)[ks, idx]
        n, z = [m[:, i] for i in range(3)], m[:, 3]
        sxs, sys_ = (idx % cols).astype(f32), (idx // cols).astype(f32)
        # (every pixel with the constants of its own winner: bp as (3, 3, npix), c as (3, npix))
        winner = dict(bp=np.stack([s["bp"] for s in sources])[ks].transpose(1, 2, 0), c=np.stack([s["c"] for s in sources])[ks].T)
        X = backproject(winner, z, sxs, sys_)
        r = rays(target, xs, ys)
        den = dot(n, r)
        ct = target["c"]
        num = dot(n, [X[i] - ct[i] for i in range(3)])
        zc = num / den
        good = (den * den > g2 * (dot(n, n) * dot(r, r))) & valid(zc, depth_min, depth_max)
    cls = cls.reshape(-1)
    direct, filled = have & (cls == 0), have & (cls == 1)
    prior = np.zeros((npix, 4), dtype=f32)
    keep = direct | (filled & good)
    for i in range(3):
        prior[keep, i] = n[i][keep]
    prior[direct, 3] = np.where(good, zc, high)[direct]
    prior[filled & good, 3] = zc[filled & good]
    cls = np.where(filled & ~good, 2, cls).astype(np.int8)
    counts = [int((cls == v).sum()) for v in (0, 1, 2)]
    info = dict(cls=cls.reshape(rows, cols), source=np.where(cls != 2, ks, -1).reshape(rows, cols),
                grazing=(have & ~good).reshape(rows, cols))
    return Result(prior.reshape(rows, cols, 4), counts, zbuf.reshape(rows, cols), dict(tally), info)
