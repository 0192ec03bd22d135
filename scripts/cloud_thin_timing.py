"""thinning the fused cloud of a 49-view 1600x1200 synthetic DTU scan to a minimum spacing of 0.2 and of 1.0:
points before and after, rounds, device events, three runs each, and whether the three masks are the same bytes

    python scripts/cloud_thin_timing.py out.json
"""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import cameras, cloud_eval, fusion, synth

ROWS, COLS, RADII, RUNS = 1200, 1600, (0.2, 1.0), 3
t0 = time.time()
allP = synth.dtu_projection_matrices()
Ps = [allP[k] for k in sorted(allP)]
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

out = {"points_before": int(len(cloud)), "fusion_device_ms": info["device_ms"], "seed": 0, "order": "hashed", "thin": []}
cloud_eval.thin_mask(cloud[:100000], 1.0)  # warm-up: code objects loaded
for radius in RADII:
    runs, digests = [], []
    for _ in range(RUNS):
        keep, ms, i = cloud_eval.thin_mask(cloud, radius)
        digests.append(hashlib.sha256(keep.cpu().numpy().tobytes()).hexdigest())
        runs.append({"device_ms": ms, **i})
        print(radius, json.dumps(runs[-1]), flush=True)
    out["thin"].append({"radius": radius, "points_after": runs[0]["kept"], "rounds": runs[0]["rounds"],
                        "grid": [runs[0][k] for k in ("grid", "cells_x", "cells_y", "cells_z")],
                        "device_ms": [r["device_ms"] for r in runs], "masks_identical": len(set(digests)) == 1,
                        "counts_identical": all(r == {**runs[0], "device_ms": r["device_ms"]} for r in runs),
                        "mask_sha256": digests[0], "runs": runs})
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "cloud_thin_dtu49.json", "w"), indent=1)
print("done")
