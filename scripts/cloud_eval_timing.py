"""the cloud score on a 49-view 1600x1200 synthetic DTU scan: the fused cloud against the cloud back-projected
from the ground-truth depths, both directions, device events; scipy's k-d tree on 16 threads as the CPU baseline

    python scripts/cloud_eval_timing.py out.json [clouds.npz]      # clouds.npz: keeps both clouds for the trace workload
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import cameras, cloud_eval, fusion, synth

ROWS, COLS, MAX_DIST = 1200, 1600, 20.0
t0 = time.time()
allP = synth.dtu_projection_matrices()
Ps = [allP[k] for k in sorted(allP)]
cs = cameras.get_camera_parameters(Ps, cam_scale=1.0)
surface = synth.Surface(600.0, 25.0, 160.0, pixel_footprint=600.0 / cs.f, seed=1234)  # in view 0's camera frame
_, R0, _ = cameras.decompose_projection(Ps[0])
rng = np.random.default_rng(1)
v, u = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
pix = np.stack([u, v, np.ones_like(u)], -1)
norm4s, grays, reference = [], [], []
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
    # the reference cloud: every 10th pixel of every view's exact depth, back-projected -- 49 x 1.92 M pixels would be ten
    # times the fused cloud; a tenth is a reference of the fused cloud's size
    k = cameras.view_constants(P, 1.0)
    keep = (np.arange(ROWS * COLS) % 10) == (i % 10)
    ray = pix.reshape(-1, 3)[keep] @ np.asarray(k["bp"], dtype=np.float64).reshape(3, 3).T
    reference.append((np.asarray(k["c"], dtype=np.float64) + d.reshape(-1)[keep, None] * ray).astype(np.float32))
reference = np.concatenate(reference)
print("scan of %d views rendered in %.1f s" % (len(Ps), time.time() - t0), flush=True)

points, info = fusion.fuse(norm4s, grays, Ps, 1.0, 0.1, 30.0, 3, 300.0, 800.0, return_info=True)
cloud = np.ascontiguousarray(np.stack([points["x"], points["y"], points["z"]], -1))
del norm4s, grays
print("fused %d points in %.2f ms; reference %d points" % (len(cloud), info["device_ms"], len(reference)), flush=True)
if len(sys.argv) > 2:
    np.savez(sys.argv[2], cloud=cloud, reference=reference)

out = {"cloud_points": int(len(cloud)), "reference_points": int(len(reference)), "max_dist": MAX_DIST,
       "fusion_device_ms": info["device_ms"], "runs": []}
a, b = torch.from_numpy(cloud).cuda(), torch.from_numpy(reference).cuda()
cloud_eval.score(a[:100000], b[:100000], MAX_DIST)  # warm-up: code objects loaded
for _ in range(3):
    s = cloud_eval.score(a, b, MAX_DIST)
    out["runs"].append({k: s[k] for k in ("accuracy_device_ms", "completeness_device_ms", "accuracy", "completeness", "precision",
                                          "recall", "fscore", "thresholds", "accuracy_search", "completeness_search")})
    print(json.dumps(out["runs"][-1]), flush=True)
for k in ("accuracy_device_ms", "completeness_device_ms"):
    out[k + "_range"] = [min(r[k] for r in out["runs"]), max(r[k] for r in out["runs"])]
out["automatic_grid"] = {"accuracy": out["runs"][0]["accuracy_search"], "completeness": out["runs"][0]["completeness_search"]}
del a, b

from scipy.spatial import cKDTree
base = {}
for name, q, t in (("accuracy", cloud, reference), ("completeness", reference, cloud)):
    t1 = time.perf_counter()
    tree = cKDTree(t)
    t2 = time.perf_counter()
    dist, _ = tree.query(q, distance_upper_bound=MAX_DIST, workers=16)
    t3 = time.perf_counter()
    base[name] = {"build_seconds": t2 - t1, "query_seconds": t3 - t2, "found": int(np.isfinite(dist).sum()),
                  "mean": float(dist[np.isfinite(dist)].mean())}
    print(name, base[name], flush=True)
out["ckdtree_workers_16"] = base
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "cloud_eval_dtu49.json", "w"), indent=1)
print("done")
