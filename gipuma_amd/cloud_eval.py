"""Score a point cloud against a reference cloud on the GPU: accuracy and completeness.

    python -m gipuma_amd.cloud_eval --cloud fused.ply --reference gt.ply --max_dist 20 --thresholds 0.5,1,2 \\
        [--output report.json]

DTU -- the data set this project is calibrated on -- scores a reconstruction cloud against cloud: accuracy is the distance
from each reconstructed point to the nearest reference point, completeness the same the other way round, distances beyond
a cut-off discarded.  Both directions are one nearest-neighbour search each (gipuma_hip_cloud_nearest,
gipuma_amd/csrc/gipuma_cloud.hip: gfx950 kernels over a uniform grid, equal to a brute-force search in every bit).  There
is no CPU fallback.  Not part of the score here: DTU's density normalisation of the clouds (its 0.2 mm resampling),
observability masks and ground-plane removal.
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import abi, dmb

THRESHOLDS = (0.5, 1.0, 2.0)
_STATS = ("grid", "cells_x", "cells_y", "cells_z", "early_out", "searched")


def _device_cloud(a, device, keep):
    """the device address of the (n, 3) float32 cloud `a` (abi.device_plane: a device tensor goes by pointer) and n"""
    if len(a.shape) != 2 or a.shape[1] != 3:
        raise ValueError("a cloud is an (n, 3) array of xyz, got %s" % (tuple(a.shape),))
    n = int(a.shape[0])
    return (abi.device_plane(a, device, keep) if n else None), n


def nearest(queries, targets, max_dist, grid=0, device_id=0, return_info=False):
    """For every query the nearest target within max_dist (the contract of gipuma_hip_cloud_nearest).  queries, targets:
    (n, 3) numpy arrays or torch tensors; device tensors are passed by pointer.  Returns (d2, idx, device_ms): float32
    squared distances (+inf: none), int32 target indices (-1: none), both numpy, and the device time in ms; with
    return_info also dict(found, none, grid, cells_x, cells_y, cells_z, early_out, searched)."""
    # (torch first: it brings a HIP runtime of its own, and a process that loaded the library's first cannot start torch's)
    import torch
    lib = abi.load_library()
    if lib.gipuma_hip_device_count() < 1:
        raise abi.GipumaHipError("the cloud search needs a HIP device; gipuma_amd has no CPU fallback")
    dev, keep = torch.device("cuda", device_id), []  # keep: the device clouds handed over, alive until the call returns
    d = abi.CloudDesc()
    d.abi_version = abi.ABI_VERSION
    d.queries, d.n_queries = _device_cloud(queries, dev, keep)
    d.targets, d.n_targets = _device_cloud(targets, dev, keep)
    d.max_dist, d.grid, d.device_id = float(max_dist), int(grid), device_id
    d2 = torch.empty(d.n_queries, dtype=torch.float32, device=dev)
    idx = torch.empty(d.n_queries, dtype=torch.int32, device=dev)
    # (the library works on a stream of its own: the clouds must be complete)
    torch.cuda.synchronize(dev)
    counts, ms = (C.c_int64 * 2)(), C.c_float()
    abi.check(lib, lib.gipuma_hip_cloud_nearest(C.byref(d), d2.data_ptr() if d.n_queries else None,
                                                idx.data_ptr() if d.n_queries else None, counts, C.byref(ms)),
              "gipuma_hip_cloud_nearest")
    out = d2.cpu().numpy(), idx.cpu().numpy(), ms.value
    if not return_info:
        return out
    stats = (C.c_int64 * len(_STATS))()
    abi.check(lib, lib.gipuma_hip_cloud_last_stats(stats), "gipuma_hip_cloud_last_stats")
    return out + (dict(found=int(counts[0]), none=int(counts[1]), **{k: int(v) for k, v in zip(_STATS, stats)}),)


def direction_score(d2, thresholds):
    """One direction of the score from its squared distances (float32, +inf: none): ({mean, median, found, none} over the
    points that found a neighbour, [share of ALL points with d <= tau for tau in thresholds] -- "none" is a miss)."""
    d2 = np.asarray(d2, dtype=np.float32)
    hit = np.isfinite(d2)
    d = np.sqrt(d2[hit].astype(np.float64))
    stats = {"mean": float(d.mean()) if len(d) else float("nan"), "median": float(np.median(d)) if len(d) else float("nan"),
             "found": int(hit.sum()), "none": int(len(d2) - hit.sum())}
    return stats, [float((d <= t).sum() / len(d2)) if len(d2) else 0.0 for t in thresholds]


def combine(acc, prec, comp, rec, thresholds):
    """the report of score() from the two directions' direction_score results"""
    out = {"accuracy": acc, "completeness": comp, "thresholds": [float(t) for t in thresholds], "precision": prec,
           "recall": rec, "fscore": [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)]}
    return out


def score(cloud, reference, max_dist=20.0, thresholds=THRESHOLDS, grid=0, device_id=0):
    """Both directions of the score.  accuracy: {mean, median, found, none} of d = sqrt(d2) (float64, on the host) over
    the cloud's points that found a reference point within max_dist; completeness: the same over the reference's points;
    precision / recall per threshold: the share of ALL cloud / reference points with d <= tau; fscore = 2PR / (P + R), 0
    when both are 0.  Empty clouds give NaN means and 0 counts.  Also the point counts, both device times and the grids."""
    thresholds = [float(t) for t in thresholds]
    a_d2, _, a_ms, a_info = nearest(cloud, reference, max_dist, grid, device_id, return_info=True)
    c_d2, _, c_ms, c_info = nearest(reference, cloud, max_dist, grid, device_id, return_info=True)
    out = combine(*direction_score(a_d2, thresholds), *direction_score(c_d2, thresholds), thresholds)
    out.update({"max_dist": float(max_dist), "cloud_points": int(len(a_d2)), "reference_points": int(len(c_d2)),
                "accuracy_device_ms": a_ms, "completeness_device_ms": c_ms,
                "accuracy_search": {k: a_info[k] for k in _STATS}, "completeness_search": {k: c_info[k] for k in _STATS}})
    return out


def parse_args(argv):
    pa = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pa.add_argument("--cloud", required=True, help="the reconstruction, a PLY file (ascii or binary_little_endian)")
    pa.add_argument("--reference", required=True, help="the reference cloud, a PLY file")
    pa.add_argument("--max_dist", type=float, default=20.0, help="distances beyond it are discarded")
    pa.add_argument("--thresholds", default=",".join("%g" % t for t in THRESHOLDS),
                    help="comma separated distances of the precision / recall / F-score")
    pa.add_argument("--grid", type=int, default=0, help="cells along the longest axis (0: automatic, 1..256)")
    pa.add_argument("--device", type=int, default=0)
    pa.add_argument("--output", default=None, help="write the report (JSON) here")
    args = pa.parse_args(argv)
    args.max_dist = float(np.float32(args.max_dist))  # a float field, like the solver's
    if not (args.max_dist > 0 and np.isfinite(args.max_dist)):
        pa.error("--max_dist must be > 0 and finite")
    try:
        args.thresholds = [float(t) for t in args.thresholds.split(",") if t]
    except ValueError:
        pa.error("--thresholds takes comma separated numbers")
    if not args.thresholds or any(not (t >= 0 and np.isfinite(t)) for t in args.thresholds):
        pa.error("--thresholds needs at least one distance, each >= 0 and finite")
    if not 0 <= args.grid <= 256:
        pa.error("--grid must be 0 (automatic) or 1..256")
    return args


def main(argv=None):
    args = parse_args(argv)
    report = score(dmb.read_ply_xyz(args.cloud), dmb.read_ply_xyz(args.reference), args.max_dist, args.thresholds,
                   grid=args.grid, device_id=args.device)
    report.update({"cloud": args.cloud, "reference": args.reference})
    if args.output:
        with open(args.output, "w") as f:
            json.dump(report, f, indent=1)
    print("accuracy %.4f (median %.4f, %d of %d points), completeness %.4f (median %.4f, %d of %d points), F-score %s at %s; "
          "%.2f + %.2f ms on device"
          % (report["accuracy"]["mean"], report["accuracy"]["median"], report["accuracy"]["found"], report["cloud_points"],
             report["completeness"]["mean"], report["completeness"]["median"], report["completeness"]["found"],
             report["reference_points"], "/".join("%.4f" % f for f in report["fscore"]),
             "/".join("%g" % t for t in args.thresholds), report["accuracy_device_ms"], report["completeness_device_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
