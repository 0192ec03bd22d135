"""the normals and the surface variation of every point of the fused cloud of a 49-view 1600x1200 synthetic DTU scan (DESIGN.md
19): the cloud is thinned to a minimum spacing of 0.2 first, then gipuma_hip_cloud_normals at radius 1.0 with k = 8, 16 and 32,
oriented along the fused normals (orient 2): estimated and short points, flips, device events, three runs each, SHA-256 of the
outputs per run (which must be identical), and the agreement of the fused normals with the estimates.  For orientation, in the
same job, gipuma_hip_cloud_knn with the means alone at the same k: the difference is what the gather and the
eigen-solve cost.  No time here is a pass criterion.

    python scripts/cloud_normals_timing.py out.json
"""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import cameras, cloud_eval, fusion, synth

ROWS, COLS, SPACING, RADIUS, KS, RUNS = 1200, 1600, 0.2, 1.0, (8, 16, 32), 3
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
fused_normals = torch.from_numpy(np.ascontiguousarray(np.stack([points["nx"], points["ny"], points["nz"]], -1))).cuda()
del norm4s, grays, points
print("fused %d points in %.2f ms" % (len(cloud), info["device_ms"]), flush=True)

idx, thin_ms, thin_info = cloud_eval.thin(cloud, SPACING, return_info=True)
out = {"points_fused": int(len(cloud)), "fusion_device_ms": info["device_ms"], "spacing": SPACING, "thin_device_ms": thin_ms,
       "thin_rounds": thin_info["rounds"], "radius": RADIUS}
cloud = cloud[torch.from_numpy(idx).cuda()].contiguous()
fused_normals = fused_normals[torch.from_numpy(idx).cuda()].contiguous()
out["points_before"] = int(len(cloud))
print("thinned to %d points in %.2f ms" % (len(cloud), thin_ms), flush=True)

for k in KS:  # warm-up: every code object loaded
    cloud_eval.normals(cloud[:100000], RADIUS, k, 2, None, fused_normals[:100000])
    cloud_eval.knn(cloud[:100000], RADIUS, k, d2=False, idx=False, count=False)
given = fused_normals.cpu().numpy()
for k in KS:
    runs, digests = [], []
    for _ in range(RUNS):
        normal, variation, m, _, ms, i = cloud_eval.normals(cloud, RADIUS, k, 2, None, fused_normals)
        digests.append([hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (normal, variation, m)])
        runs.append({"device_ms": ms, **i})
        print("k", k, json.dumps(runs[-1]), flush=True)
    est = normal.cpu().numpy()
    has = est.any(axis=1)
    agree = cloud_eval.normal_agreement(est, given)[has]
    var = variation.cpu().numpy()[has].astype(np.float64)
    out["k%d" % k] = {"k": k, "estimated": runs[0]["estimated"], "short": runs[0]["short"], "flipped": runs[0]["flipped"],
                      "grid": [runs[0][g] for g in ("grid", "cells_x", "cells_y", "cells_z")],
                      "device_ms": [r["device_ms"] for r in runs], "outputs_identical": all(d == digests[0] for d in digests),
                      "info_identical": all(r == {**runs[0], "device_ms": r["device_ms"]} for r in runs),
                      "output_sha256": dict(zip(("normal", "variation", "m"), digests[0])), "runs": runs,
                      "agreement_with_fused_normals": {"mean": float(agree.mean()), "median": float(np.median(agree)),
                                                       "below_cos_30_degrees": int((agree < np.cos(np.pi / 6)).sum())},
                      "variation": {"mean": float(var.mean()), "median": float(np.median(var))}}
    del normal, variation, m
    out["k%d" % k]["knn_device_ms_mean_only"] = [cloud_eval.knn(cloud, RADIUS, k, d2=False, idx=False, count=False)[4] for _ in range(RUNS)]
    print("k", k, "knn, mean only", out["k%d" % k]["knn_device_ms_mean_only"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "cloud_normals_dtu49.json", "w"), indent=1)
print("done")
