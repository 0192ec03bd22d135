"""per-view and whole-scan timing of the cross-view prior on config C (1600x1200, box 15, best-3), device events"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gipuma_amd import batch, dmb, prior, synth
from gipuma_amd.problem import Session

out = {}
t0 = time.time()
scan = synth.build_scan("C", device="cuda")
n = len(scan.images)
gt = scan.gt_depth
print("scan of %d views rendered in %.1f s" % (n, time.time() - t0), flush=True)

def share(d, g, tol):
    return float((np.abs(d - g) / g < tol).mean())

solved = {}
for j in range(1, 9):
    with Session(scan.problem(j)) as s:
        t = s.solve(timing=True)
        n4, _ = s.get_state()
    solved[j] = torch.from_numpy(n4).cuda()
    print("view %d plain %.2f ms, within 1e-3 %.4f" % (j, t.ms_total, share(n4[..., 3], gt[j], 1e-3)), flush=True)
torch.cuda.synchronize()
gs0 = scan.problem(0)
dmin, dmax = float(gs0.params.depthMin), float(gs0.params.depthMax)

def make_prior(S):
    ids = list(range(1, 1 + S))
    return prior.prior_from_views(scan.P_matrices[0], [solved[j] for j in ids], [scan.P_matrices[j] for j in ids],
                                  scan.cam_scale, dmin, dmax, return_info=True)

out["prior_device_ms"] = {}
for S in (2, 4, 8):
    make_prior(S)
    runs = [make_prior(S)[1] for _ in range(9)]
    out["prior_device_ms"][str(S)] = dict(median=statistics.median(r["device_ms"] for r in runs),
                                          min=min(r["device_ms"] for r in runs), max=max(r["device_ms"] for r in runs),
                                          direct=runs[0]["direct"], filled=runs[0]["filled"], empty=runs[0]["empty"])
    print("prior S=%d: %r" % (S, out["prior_device_ms"][str(S)]), flush=True)

start, pinfo = make_prior(4)
raw = start.cpu().numpy()[..., 3]
out["raw_prior_within_1e-3"] = share(raw, gt[0], 1e-3)
plain = Session(gs0)
seeded = {it: Session(scan.problem(0, iterations=it)) for it in (1, 2, 3)}
plain.solve(timing=True)
for it in seeded:
    seeded[it].solve_seeded(start, 0, timing=True)
ms = {"plain": [], **{"seeded_%d" % it: [] for it in seeded}, "prior_S4": []}
for rep in range(5):  # alternating
    ms["plain"].append(plain.solve(timing=True).ms_total)
    for it in seeded:
        _, pi = make_prior(4)
        ms["prior_S4"].append(pi["device_ms"])
        ms["seeded_%d" % it].append(seeded[it].solve_seeded(start, 0, timing=True).ms_total)
out["per_view_ms"] = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}
q = {"plain": plain.get_state()[0][..., 3]}
for it in seeded:
    q["seeded_%d" % it] = seeded[it].get_state()[0][..., 3]
out["view0_quality"] = {k: dict(within_1e3=share(v, gt[0], 1e-3), within_1e2=share(v, gt[0], 1e-2)) for k, v in q.items()}
plain.close()
for s in seeded.values():
    s.close()
print(json.dumps(out["per_view_ms"]), flush=True)
print(json.dumps(out["view0_quality"]), flush=True)

# the whole scan through the batch runner
tmp = tempfile.mkdtemp()
os.makedirs(os.path.join(tmp, "img")); os.makedirs(os.path.join(tmp, "p"))
for i, im in enumerate(scan.images):
    name = "v%02d.pgm" % i
    with open(os.path.join(tmp, "img", name), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.astype(np.uint8).tobytes())
    np.savetxt(os.path.join(tmp, "p", name + ".P"), np.asarray(scan.P_matrices[i]), fmt="%.17g")
base = ["--images-folder", os.path.join(tmp, "img"), "--p-folder", os.path.join(tmp, "p"), "--blocksize=15", "--iterations=8",
        "--n_best=3", "--depth_min=300", "--depth_max=800", "--min_angle=10", "--max_angle=30", "--max_views=10"]
out["batch"] = {}
runs = [("warmup", ["--views", "v00.pgm"]), ("plain_in_flight_2", []), ("plain_in_flight_1", ["--in_flight", "1"]),
        ("view_prior_4_it1", ["--view_prior", "4"]), ("view_prior_4_it2", ["--view_prior", "4", "--prior_iterations", "2"]),
        ("plain_in_flight_2_again", [])]
for tag, extra in runs:
    o = os.path.join(tmp, tag)
    tw = time.perf_counter()
    assert batch.main(base + ["--output-folder", o] + extra) == 0
    wall = time.perf_counter() - tw
    rep = json.load(open(os.path.join(o, "batch_rank0.json")))
    views = [v for v in rep["views"] if "skipped" not in v]
    per = {}
    for v in views:
        i = int(v["ref"][1:3])
        d = dmb.read_dmb(os.path.join(o, v["ref"][:-4], "disp.dmb"))
        per[v["ref"]] = dict(within_1e3=share(d, gt[i], 1e-3), within_1e2=share(d, gt[i], 1e-2), device_ms=v.get("device_ms"),
                             iterations=v.get("iterations"), prior=v.get("prior"), n_sources=len(v["sources"]))
    out["batch"][tag] = dict(batch_seconds=rep["batch_seconds"], wall_seconds_with_load=wall, load_seconds=rep["load_seconds"],
                             n_views=len(views), order=rep.get("order"), views=per,
                             mean_within_1e3=float(np.mean([p["within_1e3"] for p in per.values()])),
                             mean_within_1e2=float(np.mean([p["within_1e2"] for p in per.values()])),
                             sum_device_ms=(sum(p["device_ms"] for p in per.values()) if all(p["device_ms"] for p in per.values()) else None))
    print(tag, rep["batch_seconds"], out["batch"][tag]["mean_within_1e3"], out["batch"][tag]["sum_device_ms"], flush=True)
out_path = sys.argv[1] if len(sys.argv) > 1 else "prior_timing.json"
json.dump(out, open(out_path, "w"), indent=1)
print("done")
