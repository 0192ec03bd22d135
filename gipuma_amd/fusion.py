"""Depth-map fusion: the per-view (normal, depth) maps of a scan -> one point cloud.

    python -m gipuma_amd.fusion --input-folder results/ --images-folder scan9/ --p-folder calib/ \\
        --cam_scale=1 --depth_min=300 --depth_max=800 --disp_thresh=0.1 --normal_thresh=30 --num_consistent=3 \\
        --output fused.ply

The step every runner script of the reference ends with (scripts/dtu_fast.sh:23-26, :56-57: an external CUDA tool with
the same three knobs).  No parity with that tool is claimed: the contract is this project's own (DESIGN.md 11,
include/gipuma_hip.h), computed by gfx950 kernels (gipuma_amd/csrc/gipuma_fuse.hip).  There is no CPU fallback.

Input: per reference image <name> of --images-folder, the dumps normals.dmb / disp.dmb of one solve, in
<input-folder>/<stem>/ (the batch runner, gipuma_amd.batch) or <input-folder>/<YYYYMMDD_HHMMSS>_<stem>/ (the C++ CLI,
main.cpp:717-718; the newest if there are several); the gray image itself (batch.read_image); <p-folder>/<name>.P.
Output: the binary PLY (xyz, normal, gray x 3) and a JSON report next to it (<output without .ply>.json).
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

from . import abi, dmb
from .cameras import BASELINE, cos_f32, read_p_file, view_constants  # noqa: F401 (names kept importable from here)


def cos_threshold(normal_thresh):
    """cos_t = f32(cos(normal_thresh * pi / 180)) in double, normal_thresh a float32 (what gipuma_hip_fuse computes)"""
    return cos_f32(np.float32(normal_thresh))


def fuse(norm4s, grays, Ps, cam_scale=1.0, disp_thresh=0.1, normal_thresh=30.0, num_consistent=3, depth_min=-1.0,
         depth_max=-1.0, device_id=0, return_info=False):
    """Fuses V views (in the order given) on the GPU.  norm4s: (rows, cols, 4) float32 planes (n_world.xyz, depth);
    grays: (rows, cols) planes 0..255 or None; Ps: 3x4 projection matrices.  Planes may be numpy arrays or torch
    tensors (device tensors are passed by pointer).  Returns the points as a structured array of dmb's PLY vertex, in
    (view, y, x) order; with return_info also dict(per_view=[points emitted per view], device_ms=..., used=(V, rows, cols)
    uint8 marks)."""
    # (torch first: it brings a HIP runtime of its own, and a process that loaded the library's first cannot start torch's)
    import torch
    lib = abi.load_library()
    V = len(norm4s)
    if len(grays) != V or len(Ps) != V:
        raise ValueError("need one gray plane (or None) and one P per view")
    if not 2 <= V <= abi.FUSION_MAX_VIEWS:
        raise ValueError("fusion takes 2..%d views, got %d" % (abi.FUSION_MAX_VIEWS, V))
    shape = tuple(norm4s[0].shape)
    if len(shape) != 3 or shape[2] != 4:
        raise ValueError("norm4 planes are (rows, cols, 4)")
    for n4, g in zip(norm4s, grays):
        if tuple(n4.shape) != shape or (g is not None and tuple(g.shape) != shape[:2]):
            raise ValueError("every view must have the same size: %s" % (shape[:2],))
    if lib.gipuma_hip_device_count() < 1:
        raise abi.GipumaHipError("depth-map fusion needs a HIP device; gipuma_amd has no CPU fallback")
    dev, keep = torch.device("cuda", device_id), []  # keep: the device planes handed over, alive until the call returns
    views = (abi.FusionView * V)()
    for v in range(V):
        abi.fill_view(views[v], view_constants(Ps[v], cam_scale), abi.device_plane(norm4s[v], dev, keep),
                      abi.device_plane(grays[v], dev, keep) if grays[v] is not None else None)
    # (the library works on a stream of its own: the planes must be complete)
    torch.cuda.synchronize(dev)
    d = abi.FusionDesc()
    d.abi_version = abi.ABI_VERSION
    d.rows, d.cols, d.n_views = shape[0], shape[1], V
    d.views = C.cast(views, C.POINTER(abi.FusionView))
    d.disp_thresh, d.normal_thresh, d.num_consistent = disp_thresh, normal_thresh, num_consistent
    d.depth_min, d.depth_max = depth_min, depth_max
    d.device_id = device_id
    h = C.c_void_p()
    abi.check(lib, lib.gipuma_hip_fuse(C.byref(d), C.byref(h)), "gipuma_hip_fuse")
    try:
        n, per_view, ms = C.c_int64(), (C.c_int64 * V)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_fusion_count(h, C.byref(n), per_view, C.byref(ms)), "gipuma_hip_fusion_count")
        points = np.empty(n.value, dtype=dmb._PLY_VERTEX)
        abi.check(lib, lib.gipuma_hip_fusion_points(h, points.ctypes.data, 0, n.value), "gipuma_hip_fusion_points")
        if not return_info:
            return points
        used = np.empty((V, shape[0], shape[1]), dtype=np.uint8)
        abi.check(lib, lib.gipuma_hip_fusion_used(h, used.ctypes.data), "gipuma_hip_fusion_used")
        return points, dict(per_view=list(per_view), device_ms=ms.value, used=used)
    finally:
        lib.gipuma_hip_fusion_free(h)


def result_folder(input_folder, name):
    """the folder holding the dumps of reference image `name`: <input>/<stem>/ (batch runner) or the newest
    <input>/<YYYYMMDD_HHMMSS>_<stem>/ (C++ CLI, which cuts the last four characters of the name); None if neither"""
    stems = {os.path.splitext(name)[0], name[:-4] if len(name) > 4 else name}
    for stem in sorted(stems):
        folder = os.path.join(input_folder, stem)
        if os.path.isfile(os.path.join(folder, "disp.dmb")):
            return folder
    pat = re.compile(r"^\d{8}_\d{6}_(.*)$")
    stamped = sorted(e for e in os.listdir(input_folder)
                     if pat.match(e) and pat.match(e).group(1) in stems
                     and os.path.isfile(os.path.join(input_folder, e, "disp.dmb")))
    return os.path.join(input_folder, stamped[-1]) if stamped else None


def read_norm4(folder):
    """(n_world.xyz, depth) of one solve from its normals.dmb / disp.dmb"""
    n = dmb.read_dmb(os.path.join(folder, "normals.dmb"))
    d = dmb.read_dmb(os.path.join(folder, "disp.dmb"))
    if n.ndim != 3 or n.shape[2] != 3 or n.shape[:2] != d.shape:
        raise ValueError("%s: normals.dmb and disp.dmb do not match" % folder)
    return np.ascontiguousarray(np.concatenate([n, d[:, :, None]], axis=2), dtype=np.float32)


def main(argv=None):
    from .batch import IMAGE_EXTENSIONS, read_image
    pa = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pa.add_argument("--input-folder", required=True, help="the per-view results (disp.dmb, normals.dmb)")
    pa.add_argument("--images-folder", required=True)
    pa.add_argument("--p-folder", required=True)
    pa.add_argument("--views", default="all", help="comma separated image names to fuse (default: every image with a result)")
    pa.add_argument("--cam_scale", type=float, default=1.0)
    pa.add_argument("--depth_min", type=float, default=-1.0)
    pa.add_argument("--depth_max", type=float, default=-1.0)
    pa.add_argument("--disp_thresh", type=float, default=0.1)
    pa.add_argument("--normal_thresh", type=float, default=30.0)
    pa.add_argument("--num_consistent", type=int, default=3)
    pa.add_argument("--device", type=int, default=0)
    pa.add_argument("--output", default="fused.ply")
    args = pa.parse_args(argv)
    for k in ("cam_scale", "depth_min", "depth_max", "disp_thresh", "normal_thresh"):  # float fields, like the solver's
        setattr(args, k, float(np.float32(getattr(args, k))))
    names = sorted(n for n in os.listdir(args.images_folder) if n.lower().endswith(IMAGE_EXTENSIONS))
    if args.views == "all":
        chosen = [(n, result_folder(args.input_folder, n)) for n in names]
        chosen = [(n, f) for n, f in chosen if f is not None]
    else:
        wanted = [v for v in args.views.split(",") if v]
        missing = [v for v in wanted if v not in names]
        if missing:
            raise SystemExit("no image %s in %s" % (", ".join(missing), args.images_folder))
        chosen = [(n, result_folder(args.input_folder, n)) for n in names if n in wanted]  # (in the scan's order)
        missing = [n for n, f in chosen if f is None]
        if missing:
            raise SystemExit("no result (disp.dmb) for %s in %s" % (", ".join(missing), args.input_folder))
    if len(chosen) < 2:
        raise SystemExit("need the results of at least 2 views in %s, found %d" % (args.input_folder, len(chosen)))
    norm4s, grays, Ps = [], [], []
    for n, folder in chosen:
        norm4s.append(read_norm4(folder))
        grays.append(read_image(os.path.join(args.images_folder, n)))
        Ps.append(read_p_file(os.path.join(args.p_folder, n + ".P")))
        if norm4s[-1].shape[:2] != norm4s[0].shape[:2] or grays[-1].shape != norm4s[-1].shape[:2]:
            raise SystemExit("%s: result %s / image %s differ from the first view's %s" % (
                n, norm4s[-1].shape[:2], grays[-1].shape, norm4s[0].shape[:2]))
    t0 = time.perf_counter()
    points, info = fuse(norm4s, grays, Ps, args.cam_scale, args.disp_thresh, args.normal_thresh, args.num_consistent,
                        args.depth_min, args.depth_max, device_id=args.device, return_info=True)
    wall = time.perf_counter() - t0
    dmb.write_points_ply(args.output, points)
    report = {"points": int(len(points)), "device_ms": info["device_ms"], "wall_seconds": wall,
              "rows": int(norm4s[0].shape[0]), "cols": int(norm4s[0].shape[1]),
              "parameters": {k: getattr(args, k) for k in ("cam_scale", "depth_min", "depth_max", "disp_thresh",
                                                           "normal_thresh", "num_consistent")},
              "views": [{"name": n, "folder": f, "emitted": int(c)} for (n, f), c in zip(chosen, info["per_view"])]}
    with open(os.path.splitext(args.output)[0] + ".json", "w") as f:
        json.dump(report, f, indent=1)
    print("fused %d views into %d points (%.2f ms on device) -> %s" % (len(chosen), len(points), info["device_ms"],
                                                                     args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
