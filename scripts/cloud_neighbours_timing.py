"""dropping the isolated points of the fused cloud of a 49-view 1600x1200 synthetic DTU scan: the cloud is
thinned to a minimum spacing of 0.2 first, then drop_isolated at radius 1.0 with min_neighbours 8 and the exact counts
(max_count 0) at the same radius: points before and after, device events, three runs each, and whether the three masks /
count arrays are the same bytes.  For orientation the wall time of scipy's cKDTree.query_ball_point(return_length=True,
workers=16) on the same cloud, when scipy is there.

    python scripts/cloud_neighbours_timing.py out.json
"""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import cameras, cloud_eval, fusion, synth

ROWS, COLS, SPACING, RADIUS, MIN_NEIGHBOURS, RUNS = 1200, 1600, 0.2, 1.0, 8, 3
t0 = time.time()
allP = synth.dtu_projection_matrices()
Ps = [allP[k] for k in sorted(allP)][:49]  # views 1 .. 49, the scan of DESIGN.md 11 (the calibration file holds 64 cameras)
cs = cameras.get_camera_parameters(Ps, cam_scale=1.0)
surface = synth.Surface(600.0, 25.0, 160.0, pixel_footprint=600.0 / cs.f, seed=1234)  # in view 0's camera frame
_, R0, _ = cameras.decompose_projection(Ps[0])
rng = np.random.default_rng(1)
v, u = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
pix = np.stack([u, v, np.ones_like(u)], -1)
norm4s, grays = [], []
for i, P in enumerate(Ps):
    img, depth = synth.render(surface, cs.K[i], cs.R[i], cs.t[i], ROWS, COLS, device="cuda")
    d = depth.cpu().numpy().astype(np.float64)
    Xr = (d[..., None] * (pix @ np.linalg.inv(cs.K[i]).T) - cs.t[i]) @ cs.R[i]
    hx, hy = surface.grad(torch.from_numpy(Xr[..., 0]), torch.from_numpy(Xr[..., 1]))
    nr = np.stack([-hx.numpy(), -hy.numpy(), np.ones_like(u)], -1)
    nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
    nr[((-cs.R[i].T @ cs.t[i] - Xr) * nr).sum(-1) < 0] *= -1.0
    noisy = d * (1.0 + 0.0005 * rng.standard_normal(d.shape))  # ground-truth depth + 0.05 % noise, as for DESIGN.md 11
    norm4s.append(torch.from_numpy(np.concatenate([nr @ R0, noisy[..., None]], axis=-1).astype(np.float32)).cuda())
    grays.append(img.float().cuda())
    if i % 7 == 6:
        print("%d views rendered, %.1f s" % (i + 1, time.time() - t0), flush=True)
print("scan of %d views rendered in %.1f s" % (len(Ps), time.time() - t0), flush=True)

points, info = fusion.fuse(norm4s, grays, Ps, 1.0, 0.1, 30.0, 3, 300.0, 800.0, return_info=True)
cloud = torch.from_numpy(np.ascontiguousarray(np.stack([points["x"], points["y"], points["z"]], -1))).cuda()
del norm4s, grays, points
print("fused %d points in %.2f ms" % (len(cloud), info["device_ms"]), flush=True)

idx, thin_ms, thin_info = cloud_eval.thin(cloud, SPACING, return_info=True)
out = {"points_fused": int(len(cloud)), "fusion_device_ms": info["device_ms"], "spacing": SPACING, "thin_device_ms": thin_ms,
       "thin_rounds": thin_info["rounds"], "radius": RADIUS, "min_neighbours": MIN_NEIGHBOURS}
cloud = cloud[torch.from_numpy(idx).cuda()].contiguous()
out["points_before"] = int(len(cloud))
print("thinned to %d points in %.2f ms" % (len(cloud), thin_ms), flush=True)

cloud_eval.neighbours(cloud[:100000], RADIUS, MIN_NEIGHBOURS, MIN_NEIGHBOURS)  # warm-up: code objects loaded
for what, max_count in (("drop_isolated", MIN_NEIGHBOURS), ("exact_counts", 0)):  # (drop_isolated's own max_count)
    runs, digests = [], []
    for _ in range(RUNS):
        count, keep, ms, i = cloud_eval.neighbours(cloud, RADIUS, MIN_NEIGHBOURS, max_count, counts=max_count == 0, keep=max_count != 0)
        digests.append(hashlib.sha256((count if keep is None else keep).cpu().numpy().tobytes()).hexdigest())
        runs.append({"device_ms": ms, **i})
        print(what, json.dumps(runs[-1]), flush=True)
    out[what] = {"max_count": max_count, "points_after": runs[0]["kept"], "saturated": runs[0]["saturated"],
                 "grid": [runs[0][k] for k in ("grid", "cells_x", "cells_y", "cells_z")],
                 "device_ms": [r["device_ms"] for r in runs], "outputs_identical": len(set(digests)) == 1,
                 "info_identical": all(r == {**runs[0], "device_ms": r["device_ms"]} for r in runs),
                 "output_sha256": digests[0], "runs": runs}
    if max_count == 0:
        c = count.cpu().numpy().view(np.uint32)
        out[what].update({"count_mean": float(c.mean()), "count_max": int(c.max()), "count_sum_even": int(c.astype(np.int64).sum()) % 2 == 0,
                          "below_min_neighbours": int((c < MIN_NEIGHBOURS).sum())})
try:
    from scipy.spatial import cKDTree
    host = cloud.cpu().numpy().astype(np.float64)
    t1 = time.time()
    tree = cKDTree(host)
    t2 = time.time()
    lengths = tree.query_ball_point(host, RADIUS, return_length=True, workers=16)
    out["ckdtree"] = {"build_s": t2 - t1, "query_s": time.time() - t2, "workers": 16,
                      "count_mean": float(lengths.mean() - 1)}  # (float64, the point itself included: not the contract)
    print("cKDTree", json.dumps(out["ckdtree"]), flush=True)
except ImportError:
    out["ckdtree"] = None
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "cloud_neighbours_dtu49.json", "w"), indent=1)
print("done")
