"""the connected components of the fused cloud of a 49-view 1600x1200 synthetic DTU scan: the cloud is thinned
to a minimum spacing of 0.2 first (the cloud of DESIGN.md 16), then labelled at radius 0.3 and 1.0, three runs each: device
events, components, the largest one, the points kept at min_size 100 and whether the three runs' outputs are the same bytes.
In the same job the neighbour count at the same radius (exact counts: the same walk without the unions; drop_isolated with
min_neighbours 8: the walk that stops early), and for orientation the wall time of scipy's cKDTree.query_pairs plus
csgraph.connected_components on the same cloud, when scipy is there.

    python scripts/cloud_components_timing.py out.json [name=path/to/libgipuma_hip.so ...]

Every further library named is timed as well, in the same process on the same cloud, after the tree's own: a differently
built one (its components and the existing calls), or an earlier commit's (the existing calls only: the search both ways,
the thinning at 0.2 and 1.0, drop_isolated, the k nearest at k = 8), with medians of three and the outputs' hashes.
"""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import abi, cameras, cloud_eval, fusion, synth

ROWS, COLS, SPACING, RADII, MIN_SIZE, MIN_NEIGHBOURS, RUNS = 1200, 1600, 0.2, (0.3, 1.0), 100, 8, 3
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
print("scan of %d views rendered in %.1f s" % (len(Ps), time.time() - t0), flush=True)

points, info = fusion.fuse(norm4s, grays, Ps, 1.0, 0.1, 30.0, 3, 300.0, 800.0, return_info=True)
fused = torch.from_numpy(np.ascontiguousarray(np.stack([points["x"], points["y"], points["z"]], -1))).cuda()
del norm4s, grays, points
idx, thin_ms, thin_info = cloud_eval.thin(fused, SPACING, return_info=True)
cloud = fused[torch.from_numpy(idx).cuda()].contiguous()
out = {"points_fused": int(len(fused)), "spacing": SPACING, "points": int(len(cloud)), "min_size": MIN_SIZE, "runs_per_call": RUNS}
print("fused %d points, thinned to %d" % (len(fused), len(cloud)), flush=True)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update((t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes())
    return h.hexdigest()


def timed(call):
    """RUNS runs of call() -> (device_ms, figures dict, digest): the times, their median, the figures and whether they repeat"""
    runs = [call() for _ in range(RUNS)]
    ms = [r[0] for r in runs]
    return {"device_ms": ms, "median_ms": float(np.median(ms)), "spread_ms": max(ms) - min(ms), **runs[0][1],
            "output_sha256": runs[0][2], "outputs_identical": len({r[2] for r in runs}) == 1,
            "figures_identical": all(r[1] == runs[0][1] for r in runs)}


def components_at(radius):
    label, size, keep, ms, i = cloud_eval.components(cloud, radius, MIN_SIZE)
    return ms, {"components": i["components"], "kept": i["kept"], "dropped": i["dropped"], "largest": int(size.max()),
                "grid": [i[k] for k in ("grid", "cells_x", "cells_y", "cells_z")]}, sha(label, size, keep)


def neighbours_at(radius, max_count):
    count, keep, ms, i = cloud_eval.neighbours(cloud, radius, MIN_NEIGHBOURS, max_count, counts=max_count == 0, keep=max_count != 0)
    return ms, {"kept": i["kept"]}, sha(count if keep is None else keep)


def thin_at(radius):
    keep, ms, i = cloud_eval.thin_mask(cloud if radius > SPACING else fused, radius)
    return ms, {"kept": i["kept"], "rounds": i["rounds"]}, sha(keep)


def knn8():
    _, _, _, mean, ms, i = cloud_eval.knn(cloud, 1.0, 8, d2=False, idx=False, count=False)
    return ms, {"complete": i["complete"]}, sha(mean)


def search(a, b):
    d2, j, ms, i = cloud_eval.nearest(a, b, 20.0, return_info=True)
    return ms, {"found": i["found"]}, sha(d2, j)


def existing_calls():
    half = cloud[::2].contiguous()
    return {"search cloud -> half": timed(lambda: search(cloud, half)), "search half -> cloud": timed(lambda: search(half, cloud)),
            "thin 0.2": timed(lambda: thin_at(0.2)), "thin 1.0": timed(lambda: thin_at(1.0)),
            "drop_isolated 1.0": timed(lambda: neighbours_at(1.0, MIN_NEIGHBOURS)), "knn k=8 1.0": timed(knn8)}


def component_calls():
    res = {}
    for radius in RADII:
        res["components %g" % radius] = timed(lambda: components_at(radius))
        res["exact_counts %g" % radius] = timed(lambda: neighbours_at(radius, 0))
        res["drop_isolated %g" % radius] = timed(lambda: neighbours_at(radius, MIN_NEIGHBOURS))
        c, n = res["components %g" % radius], res["exact_counts %g" % radius]
        c["over_the_same_walk_ms"] = c["median_ms"] - n["median_ms"]
        print(radius, json.dumps(c), flush=True)
    return res


cloud_eval.components(cloud[:100000], 1.0)  # warm-up: code objects loaded
cloud_eval.neighbours(cloud[:100000], 1.0, 1, 1)
out["tree"] = {**component_calls(), **existing_calls()}
for spec in sys.argv[2:]:
    name, path = spec.split("=", 1)
    declared = abi.SYMBOLS[:]
    try:
        lib = abi.load_library(path)
        has_components = True
    except AttributeError:  # an earlier commit's library: without the new entry point
        abi.SYMBOLS[:] = [s for s in declared if s[0] != "gipuma_hip_cloud_components"]
        lib, has_components = abi.load_library(path), False
        abi.SYMBOLS[:] = declared
    abi._lib = lib
    cloud_eval.neighbours(cloud[:100000], 1.0, 1, 1)  # warm-up of this library's code objects
    out[name] = {**(component_calls() if has_components else {}), **existing_calls()}
    out[name]["equal_to_tree"] = {k: r["output_sha256"] == out["tree"][k]["output_sha256"] and
                                  all(r[f] == out["tree"][k][f] for f in r if f in ("kept", "components", "found", "complete", "rounds"))
                                  for k, r in out[name].items()}
    print(name, json.dumps({k: r["median_ms"] for k, r in out[name].items() if k != "equal_to_tree"}), flush=True)
abi._lib = None
try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    host = cloud.cpu().numpy().astype(np.float64)
    t1 = time.time()
    pairs = cKDTree(host).query_pairs(RADII[0], output_type="ndarray")
    t2 = time.time()
    n_comp, _ = connected_components(coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(host),) * 2), directed=False)
    out["scipy"] = {"radius": RADII[0], "pairs": int(len(pairs)), "pairs_s": t2 - t1, "components_s": time.time() - t2,
                    "components": int(n_comp)}  # (float64 distances: not the contract; the count is not compared)
    print("scipy", json.dumps(out["scipy"]), flush=True)
except ImportError:
    out["scipy"] = None
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "cloud_components_dtu49.json", "w"), indent=1)
print("done")
