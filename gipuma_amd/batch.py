"""Batch runner: every image of a scan as reference view, sharded over the GPUs of a node
(replaces the per-view process loop of the reference's scripts/dtu_fast.sh:30-55).

    python -m gipuma_amd.batch --images-folder scan9/ --p-folder calib/ --output-folder results/ \\
        --blocksize=15 --iterations=8 --n_best=3 --depth_min=300 --depth_max=800 \\
        --min_angle=10 --max_angle=30 --max_views=10
    python -m torch.distributed.run --nproc-per-node 8 -m gipuma_amd.batch ...      # 8 GPUs

MI355X-first differences from the shell loop:
  * one process per GPU handles MANY reference views; the scan's images are decoded and uploaded
    to HBM once per process (a 49-view DTU scan is 0.4 GB of the 288 GB) and every session binds
    them by device pointer -- no per-view process start, disk read or PCIe upload;
  * reference views are sharded round-robin over the ranks (gipuma_amd.shard); there is no
    inter-GPU communication;
  * several reference views are kept in flight per GPU (--in_flight, default 2): one session and HIP
    stream each, the solves enqueued asynchronously -- launch tails of one view fill with workgroups of
    another (bench.py `value_views_in_flight`: +2 % with 2 / 3 views on config C since the fused launches of
    round 4 -- they leave little to overlap --, far more on frames whose tiles do not fill the GPU, e.g. config B);
  * results land in <output>/<refname>/{disp.dmb, normals.dmb, cost.dmb} -- the dumps the
    reference writes (main.cpp:1001-1015) and the depth-map fusion reads (gipuma_amd.fusion);
  * --levels N (default 1: today's single-level solve): coarse-to-fine over an N-level pyramid of the scan (DESIGN.md 12,
    gipuma_amd.pyramid) -- the coarse planes are made once per scan, every view solves its coarsest level plainly and
    seeds each finer level from the one below; --level_iterations a,b,.. (coarsest first; default for --levels 2:
    <iterations>,2).  Views are solved one at a time; with --in_flight 1 the report carries per-level device times;
  * --view_prior N (default 0: off): a view whose selected sources have been solved earlier in this run starts from their
    results instead of from random planes (gipuma_amd.prior) -- the (normal, depth) maps of up to N solved
    sources are carried into its camera on the GPU and it runs --prior_iterations iterations from that start; views are
    taken greedily, the one with the most solved sources next, and solved one at a time; the solved maps stay in HBM for
    the run (49 views at 1600x1200: 1.9 GB).  With several ranks each rank draws on its own solved views only;
  * --fuse: the results of this run are also fused on the GPU, from memory, into <output>/fused.ply (with
    --disp_thresh / --normal_thresh / --num_consistent and the depth range) -- what the reference's
    scripts leave to an external CUDA tool after the loop (scripts/dtu_fast.sh:56-57).  One process only: with
    WORLD_SIZE > 1 run `python -m gipuma_amd.fusion` on the output folder instead;
  * --eval_cloud gt.ply (with --fuse): the fused cloud is scored against that reference cloud on the GPU -- accuracy,
    completeness, precision / recall / F-score within --eval_max_dist (gipuma_amd.cloud_eval) -- and the
    score joins the report as `cloud_score`.  --eval_reduce 0.2 thins the fused cloud to that minimum point spacing
    first, as DTU's evaluation does;
  * --fuse_neighbour_radius r --fuse_min_neighbours N (with --fuse): the fused cloud loses its isolated points -- those
    with fewer than N other points within r (gipuma_amd.cloud_eval.drop_isolated) -- before fused.ply is
    written and before --eval_cloud scores it;
  * --fuse_outlier_radius r --fuse_outlier_k K --fuse_outlier_std s (with --fuse): the fused cloud then loses its
    statistical outliers -- the points whose mean distance to their K nearest neighbours within r exceeds the cloud's
    mean of that figure by more than s standard deviations, and those with fewer than K neighbours there (DESIGN.md 17,
    gipuma_amd.cloud_eval.drop_outliers) -- after --fuse_neighbour_radius, before fused.ply is written and scored;
  * --fuse_component_radius r --fuse_min_component N (with --fuse): the fused cloud then loses its small clumps -- every
    connected component of its radius graph (points joined where they lie within r of each other) with fewer than N
    points (gipuma_amd.cloud_eval.drop_small_components) -- after --fuse_outlier_radius, before fused.ply
    is written and scored;
  * --fuse_normal_radius r --fuse_normal_k K --fuse_max_normal_angle a (with --fuse): the fused cloud then loses the
    points whose fused normal is more than a degrees off the normal estimated from their K nearest neighbours within r,
    and those with fewer than three neighbours there (gipuma_amd.cloud_eval.drop_disagreeing_normals) --
    after --fuse_component_radius, before fused.ply is written and scored.

Images: what the reference's scripts hand to imread (main.cpp:739-751) -- PNG, JPG (through PIL), binary PGM / PPM.
Calibration: <p-folder>/<image name>.P (fileIoUtils.h:83-110).
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

from . import abi, dmb
from .cameras import get_camera_parameters, read_p_file, select_views
from .problem import AlgorithmParameters, GlobalState, Session
from .shard import views_for_rank


def read_pgm(path):
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"P5":
        raise ValueError("%s: only binary PGM (P5) is read here" % path)
    tokens, pos = [], 2
    while len(tokens) < 3:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        tokens.append(int(data[pos:end]))
        pos = end
    cols, rows, maxv = tokens
    if maxv != 255:
        raise ValueError("%s: 8-bit images only" % path)
    img = np.frombuffer(data, dtype=np.uint8, count=rows * cols, offset=pos + 1).reshape(rows, cols)
    return img.astype(np.float32)


IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".pgm", ".ppm", ".pnm")


def read_image(path):
    """imread(path, IMREAD_GRAYSCALE) as float32 (main.cpp:741, :941).  PGM: the bytes.  Everything else through PIL:
    single-channel files as they are (16-bit: the high byte); colour PNG / PPM by the rule of the C++ front-end
    (gipuma_host.cpp read_image_gray: libpng's 15-bit 9797 / 19234 / 3737 for PNG, OpenCV's 14-bit BGR2GRAY for PPM);
    JPEG decoded to luma by libjpeg itself (PIL draft mode 'L'), which is what OpenCV's JPEG reader does for
    IMREAD_GRAYSCALE.  One known deviation: a 16-bit RGB / RGBA PNG reaches this function as PIL's 8-bit RGB, so its gray
    is formed on the high bytes; libpng (and the C++ front-end, read_png_rgb8) forms it on the 16-bit samples and then
    takes the high byte -- the last bit may differ for such files."""
    with open(path, "rb") as f:
        head = f.read(4)
    if head[:2] == b"P5":
        return read_pgm(path)
    from PIL import Image
    im = Image.open(path)
    if im.format == "JPEG":
        im.draft("L", im.size)
        return np.asarray(im.convert("L"), dtype=np.uint8).astype(np.float32)
    if im.mode in ("I;16", "I;16B", "I;16L", "I"):
        return (np.asarray(im, dtype=np.uint32) >> 8).astype(np.uint8).astype(np.float32)
    if im.mode in ("L", "1", "LA"):
        return np.asarray(im.convert("L"), dtype=np.uint8).astype(np.float32)
    if im.mode == "P" and im.palette is not None and im.palette.mode == "L":
        return np.asarray(im.convert("L"), dtype=np.uint8).astype(np.float32)
    rgb = np.asarray(im.convert("RGB"), dtype=np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    if im.format == "PPM":
        return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.float32)
    return ((9797 * r + 19234 * g + 3737 * b) >> 15).astype(np.float32)


def plan_views(P_all, names, ref_idx, cols, rows, ap, cam_scale=1.0):
    """the reference's per-view recipe: reference first, every other image as a candidate,
    selectViews keeps those inside the angle cone (main.cpp:430-499); returns the camera set
    restricted to [reference] + selected views and their global indices"""
    order = [ref_idx] + [i for i in range(len(names)) if i != ref_idx]
    cs_all = get_camera_parameters([P_all[i] for i in order], cam_scale=cam_scale)
    ap_view = AlgorithmParameters(**{k: getattr(ap, k) for k in vars(ap)})
    subset, dmin, dmax = select_views(cs_all, cols, rows, ap.min_angle, ap.max_angle, ap.max_views,
                                      ap.depthMin, ap.depthMax)
    used = [order[0]] + [order[i] for i in subset]
    cs = get_camera_parameters([P_all[i] for i in used], cam_scale=cam_scale)
    ap_view.depthMin, ap_view.depthMax = dmin, dmax
    return cs, used, ap_view


# Iterations of a view that starts from its neighbours' results: the smallest of 1, 2, 3 that met the quality margins on
# the three 320x240 scenes (tests/test_prior.py).  At 1600x1200 it does NOT hold them: see DESIGN.md 13 and the help text.
PRIOR_ITERATIONS = 1


class Scan:
    """What every solve strategy works on: the whole scan resident in the HBM of one device (loaded here, once), the
    parameters, and what the run collects (the report's entries; with --fuse the solved maps)."""

    def __init__(self, args, dev_index):
        import torch
        self.args = args
        self.names = sorted(n for n in os.listdir(args.images_folder) if n.lower().endswith(IMAGE_EXTENSIONS))
        if len(self.names) < 2:
            raise SystemExit("need at least 2 images (png / jpg / pgm / ppm) in %s" % args.images_folder)
        self.P_all = [read_p_file(os.path.join(args.p_folder, n + ".P")) for n in self.names]
        t0 = time.perf_counter()
        self.dev = [torch.from_numpy(read_image(os.path.join(args.images_folder, n))).to("cuda:%d" % dev_index)
                    for n in self.names]
        torch.cuda.synchronize()
        self.load_seconds = time.perf_counter() - t0
        self.rows, self.cols = (int(n) for n in self.dev[0].shape)
        self.ap = AlgorithmParameters(iterations=args.iterations, n_best=args.n_best, gamma=args.cost_gamma,
                                      depthMin=args.depth_min, depthMax=args.depth_max, min_angle=args.min_angle,
                                      max_angle=args.max_angle, max_views=args.max_views)
        self.ap.set_blocksize(args.blocksize)
        self.flavour = dict(fast=args.mode == "fast", literal=args.mode == "literal")  # of every Session (--mode)
        self.report = []
        self.solved = {}  # reference name -> norm4 (host), for --fuse

    def plans(self, mine):
        """(name, *plan_views) of every view of `mine` with a source inside the angle cone; the others go to the report"""
        for ref_name in mine:
            plan = plan_views(self.P_all, self.names, self.names.index(ref_name), self.cols, self.rows, self.ap, self.args.cam_scale)
            if len(plan[1]) < 2:
                self.report.append({"ref": ref_name, "skipped": "no source view inside the angle cone"})
            else:
                yield (ref_name,) + plan

    def record(self, ref_name, used, tw0, t, n4, cost, levels=None, extra=None):
        """writes the dumps of one solved view and its entry of the report"""
        wall_ms = (time.perf_counter() - tw0) * 1e3  # session set-up + solve (+ what ran beside it) + download
        folder = os.path.join(self.args.output_folder, os.path.splitext(ref_name)[0])
        os.makedirs(folder, exist_ok=True)
        dmb.write_dmb(os.path.join(folder, "disp.dmb"), n4[..., 3])
        dmb.write_dmb(os.path.join(folder, "normals.dmb"), n4[..., :3])
        dmb.write_dmb(os.path.join(folder, "cost.dmb"), cost)
        if self.args.fuse:
            self.solved[ref_name] = n4
        npix = self.rows * self.cols
        entry = {"ref": ref_name, "sources": [self.names[i] for i in used[1:]], "wall_ms": wall_ms,
                 "mpix_per_s_wall": npix / (wall_ms * 1e-3) / 1e6}
        if t is not None:  # one view at a time: the device time is that view's alone
            entry.update({"device_ms": t.ms_total, "mpix_per_s": npix / (t.ms_total * 1e-3) / 1e6})
        if levels is not None:  # (--levels > 1, one view at a time: device times per level, coarsest first)
            ms = sum(lv["ms_total"] for lv in levels)
            entry.update({"levels": levels, "device_ms": ms, "mpix_per_s": npix / (ms * 1e-3) / 1e6})
        if extra is not None:  # (--view_prior: the prior's sources, class counts and device time; the iterations run)
            entry.update(extra)
        self.report.append(entry)


def solve_plain(scan, mine, in_flight):
    """The views of `mine` in order, `in_flight` of them at a time: one session and stream each, the solves enqueued
    asynchronously (in_flight 1: one at a time, with per-view device times)."""
    pending = collections.deque()  # (session, reference name, used, start time, timing or None)

    def retire():
        s, ref_name, used, tw0, t = pending.popleft()
        try:
            n4, cost = s.get_state()  # waits for the session's stream
        finally:
            s.close()
        scan.record(ref_name, used, tw0, t, n4, cost)

    try:
        for ref_name, cs, used, ap_view in scan.plans(mine):
            gs = GlobalState.on_resident_planes(scan.dev, used, cs, ap_view, seed=scan.args.seed)
            tw0 = time.perf_counter()
            s = Session(gs, **scan.flavour)
            try:
                t = s.solve(timing=in_flight == 1)  # (untimed: asynchronous, returns once the launches are enqueued)
            except Exception:
                s.close()
                raise
            pending.append((s, ref_name, used, tw0, t if in_flight == 1 else None))
            while len(pending) >= in_flight:
                retire()
        while pending:
            retire()
    finally:  # (an error above: do not leave sessions of this batch behind)
        for leftover in pending:
            leftover[0].close()


def solve_levels(scan, mine, pyr, level_iterations, timing):
    """--levels: the views of `mine` one at a time, each coarse-to-fine over the scan's pyramid.  View selection and the
    depth range are decided by plan_views, on the finest level; every level reuses them."""
    from . import pyramid
    for ref_name, _, used, ap_view in scan.plans(mine):
        tw0 = time.perf_counter()
        n4, cost, times = pyramid.solve_view(pyr, scan.P_all, used, ap_view, level_iterations, seed=scan.args.seed,
                                             mode=scan.args.mode, cam_scale=scan.args.cam_scale, timing=timing)
        scan.record(ref_name, used, tw0, None, n4, cost, times if timing else None)


def solve_with_view_prior(scan, mine):
    """--view_prior: the views of `mine` in gipuma_amd.prior.greedy_order, one at a time.  A view with at least
    --prior_min_views solved sources starts from the prior of the first --view_prior of them (in selection order) and runs
    --prior_iterations iterations; any other view runs the plain solve.  Returns the order."""
    import torch
    from . import prior as view_prior
    args, names, P_all = scan.args, scan.names, scan.P_all
    device = scan.dev[0].device
    planned = list(scan.plans(mine))  # (the views without a source are in the report by now, ahead of the solved ones)
    plans = {p[0]: p[1:] for p in planned}
    order = view_prior.greedy_order([p[0] for p in planned], {n: [names[i] for i in plans[n][1][1:]] for n in plans})
    kept = {}  # reference name -> (norm4, cost or None) on the device, for the views solved after it
    for ref_name in order:
        cs, used, ap_view = plans[ref_name]
        have = [names[i] for i in used[1:] if names[i] in kept][:args.view_prior]
        tw0 = time.perf_counter()
        start, pinfo = None, None
        if len(have) >= args.prior_min_views:
            with_cost = args.prior_max_cost is not None
            start, pinfo = view_prior.prior_from_views(
                P_all[used[0]], [kept[n][0] for n in have], [P_all[names.index(n)] for n in have], args.cam_scale,
                ap_view.depthMin, ap_view.depthMax, costs=[kept[n][1] for n in have] if with_cost else None,
                max_cost=args.prior_max_cost, return_info=True, device_id=device.index)
            ap_view.iterations = args.prior_iterations
        with Session(GlobalState.on_resident_planes(scan.dev, used, cs, ap_view, seed=args.seed), **scan.flavour) as s:
            t = s.solve(timing=True) if start is None else s.solve_seeded(start, 0, timing=True)
            n4, cost = s.get_state()
        # (kept in HBM for the views solved later: uploaded again from the host copy the dumps need anyway, 31 MB per
        #  1600x1200 view -- a device-to-device copy out of the session would save that upload)
        kept[ref_name] = (torch.from_numpy(n4).to(device),
                          torch.from_numpy(cost).to(device) if args.prior_max_cost is not None else None)
        torch.cuda.synchronize()
        scan.record(ref_name, used, tw0, t, n4, cost,
                    extra={"iterations": int(ap_view.iterations), "prior": None if pinfo is None else dict(sources=have, **pinfo)})
    return order


def parse_args(argv):
    """the command line, checked; args.level_iterations comes back as the list of counts, coarsest first"""
    pa = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pa.add_argument("--images-folder", required=True)
    pa.add_argument("--p-folder", required=True)
    pa.add_argument("--output-folder", required=True)
    pa.add_argument("--views", default="all", help="comma separated image names to use as reference (default all)")
    pa.add_argument("--blocksize", type=int, default=19)
    pa.add_argument("--iterations", type=int, default=8)
    pa.add_argument("--n_best", type=int, default=2)
    pa.add_argument("--cost_gamma", type=float, default=10.0)
    pa.add_argument("--depth_min", type=float, default=-1.0)
    pa.add_argument("--depth_max", type=float, default=-1.0)
    pa.add_argument("--min_angle", type=float, default=5.0)
    pa.add_argument("--max_angle", type=float, default=45.0)
    pa.add_argument("--max_views", type=int, default=9)
    pa.add_argument("--cam_scale", type=float, default=1.0)
    pa.add_argument("--seed", type=int, default=1)
    pa.add_argument("--in_flight", type=int, default=2,
                    help="reference views kept in flight per GPU (1: one at a time, with per-view device times)")
    pa.add_argument("--mode", choices=["exact", "fast", "literal"], default="exact",
                    help="exact: bit-identical to the numerical model (default); fast: tolerance-judged kernels "
                         "(GIPUMA_HIP_FLAG_FAST); literal: the reference's own operation order, bit-identical to the "
                         "reference's code, about 20x slower (GIPUMA_HIP_FLAG_LITERAL)")
    pa.add_argument("--levels", type=int, default=1,
                    help="pyramid levels of a coarse-to-fine solve (1: the plain solve; gipuma_amd.pyramid)")
    pa.add_argument("--level_iterations", default="",
                    help="with --levels > 1: iterations per level, coarsest first (default: <iterations>,2,..,2)")
    pa.add_argument("--view_prior", type=int, default=0,
                    help="start a view from the results of up to N of its selected source views that this run (this rank: "
                         "ranks do not exchange results) has solved already (0: off; gipuma_amd.prior)")
    pa.add_argument("--prior_iterations", type=int, default=PRIOR_ITERATIONS,
                    help="with --view_prior: iterations of a view that starts from a prior (the others run --iterations; "
                         "0: the view's result is the prior itself with the random fallback, finalized).  The default, "
                         "%d, is the smallest count that matched the plain solve on the 320x240 test scenes; at 1600x1200 "
                         "it loses quality (config C, share within 1e-2 of ground truth: plain 0.999, 1 it. 0.984, 2 it. "
                         "0.994, 3 it. 0.999, and the loss compounds from view to view): use 3 there (DESIGN.md 13)"
                         % PRIOR_ITERATIONS)
    pa.add_argument("--prior_min_views", type=int, default=2,
                    help="with --view_prior: solved source views a view needs to start from their prior")
    pa.add_argument("--prior_max_cost", type=float, default=None,
                    help="with --view_prior: leave source pixels with a cost above this out of the prior (default: keep all)")
    pa.add_argument("--fuse", action="store_true",
                    help="fuse the views solved in this run into <output-folder>/fused.ply (gipuma_amd.fusion)")
    pa.add_argument("--disp_thresh", type=float, default=0.1, help="with --fuse")
    pa.add_argument("--normal_thresh", type=float, default=30.0, help="with --fuse, degrees")
    pa.add_argument("--num_consistent", type=int, default=3, help="with --fuse")
    pa.add_argument("--eval_cloud", default=None,
                    help="with --fuse: a reference cloud (PLY) to score the fused cloud against (gipuma_amd.cloud_eval)")
    pa.add_argument("--eval_max_dist", type=float, default=20.0,
                    help="with --eval_cloud: distances beyond it are discarded")
    pa.add_argument("--eval_reduce", type=float, default=0.0,
                    help="with --eval_cloud: thin the fused cloud to this minimum point spacing before it is scored "
                         "(0: off; DTU uses 0.2; DESIGN.md 15)")
    pa.add_argument("--fuse_neighbour_radius", type=float, default=0.0,
                    help="with --fuse and --fuse_min_neighbours: drop the fused points that have fewer than that many other "
                         "points within this radius, before fused.ply is written and scored (0: off; DESIGN.md 16)")
    pa.add_argument("--fuse_min_neighbours", type=int, default=None,
                    help="with --fuse_neighbour_radius: the count a fused point needs to stay")
    pa.add_argument("--fuse_outlier_radius", type=float, default=0.0,
                    help="with --fuse, --fuse_outlier_k and --fuse_outlier_std: after --fuse_neighbour_radius, drop the fused "
                         "points whose mean distance to their k nearest neighbours within this radius is above the cloud's "
                         "mean of it by more than that many standard deviations, and those with fewer than k neighbours "
                         "there (0: off; DESIGN.md 17)")
    pa.add_argument("--fuse_outlier_k", type=int, default=None, help="with --fuse_outlier_radius: the number of nearest neighbours, 1..32")
    pa.add_argument("--fuse_outlier_std", type=float, default=None,
                    help="with --fuse_outlier_radius: the standard deviations allowed, >= 0")
    pa.add_argument("--fuse_component_radius", type=float, default=0.0,
                    help="with --fuse and --fuse_min_component: after --fuse_outlier_radius, drop the fused points whose "
                         "connected component -- points joined where they lie within this radius of each other -- has fewer "
                         "than that many points (0: off; DESIGN.md 18)")
    pa.add_argument("--fuse_min_component", type=int, default=None,
                    help="with --fuse_component_radius: the points a component needs for them to stay")
    pa.add_argument("--fuse_normal_radius", type=float, default=0.0,
                    help="with --fuse, --fuse_normal_k and --fuse_max_normal_angle: after --fuse_component_radius, drop the "
                         "fused points whose fused normal is more than that angle off the normal estimated from their k "
                         "nearest neighbours within this radius, and those with fewer than three neighbours there (0: off; "
                         "DESIGN.md 19)")
    pa.add_argument("--fuse_normal_k", type=int, default=None, help="with --fuse_normal_radius: the number of nearest neighbours, 3..32")
    pa.add_argument("--fuse_max_normal_angle", type=float, default=None,
                    help="with --fuse_normal_radius: the angle allowed between the fused normal and the estimate, 0..90 degrees")
    args = pa.parse_args(argv)
    # the reference parses these with sscanf("%f") into float fields (main.cpp:300-360)
    for k in ("cost_gamma", "depth_min", "depth_max", "min_angle", "max_angle", "cam_scale", "disp_thresh",
              "normal_thresh", "eval_max_dist", "eval_reduce", "fuse_neighbour_radius"):
        setattr(args, k, float(np.float32(getattr(args, k))))
    if args.eval_cloud is not None and not args.fuse:
        pa.error("--eval_cloud scores the fused cloud: it needs --fuse")
    if args.eval_cloud is not None and not (args.eval_max_dist > 0 and np.isfinite(args.eval_max_dist)):
        pa.error("--eval_max_dist must be > 0 and finite")
    if not (args.eval_reduce >= 0 and np.isfinite(args.eval_reduce)):
        pa.error("--eval_reduce must be >= 0 and finite (0: off)")
    if args.eval_reduce > 0 and args.eval_cloud is None:
        pa.error("--eval_reduce thins the cloud that --eval_cloud scores: it needs --eval_cloud")
    if not (args.fuse_neighbour_radius >= 0 and np.isfinite(args.fuse_neighbour_radius)):
        pa.error("--fuse_neighbour_radius must be >= 0 and finite (0: off)")
    if (args.fuse_neighbour_radius > 0) != (args.fuse_min_neighbours is not None):
        pa.error("--fuse_neighbour_radius and --fuse_min_neighbours need each other")
    if args.fuse_min_neighbours is not None and not 0 <= args.fuse_min_neighbours < 2 ** 31:
        pa.error("--fuse_min_neighbours must be 0 .. 2^31 - 1")
    if args.fuse_neighbour_radius > 0 and not args.fuse:
        pa.error("--fuse_neighbour_radius filters the fused cloud: it needs --fuse")
    args.fuse_min_neighbours = args.fuse_min_neighbours or 0
    from .cloud_eval import check_outlier_args
    check_outlier_args(pa, args, "fuse_outlier_radius", "fuse_outlier_k", "fuse_outlier_std")
    if args.fuse_outlier_radius > 0 and not args.fuse:
        pa.error("--fuse_outlier_radius filters the fused cloud: it needs --fuse")
    from .cloud_eval import check_component_args
    check_component_args(pa, args, "fuse_component_radius", "fuse_min_component")
    if args.fuse_component_radius > 0 and not args.fuse:
        pa.error("--fuse_component_radius filters the fused cloud: it needs --fuse")
    from .cloud_eval import check_normal_args
    check_normal_args(pa, args, "fuse_normal_radius", "fuse_normal_k", "fuse_max_normal_angle")
    args.fuse_max_normal_angle = args.fuse_max_normal_angle or 0.0
    if args.fuse_normal_radius > 0 and not args.fuse:
        pa.error("--fuse_normal_radius filters the fused cloud: it needs --fuse")
    if args.levels < 1:
        raise SystemExit("--levels must be >= 1")
    args.level_iterations = [int(v) for v in args.level_iterations.split(",") if v] or \
        [args.iterations] + [2] * (args.levels - 1)
    if args.levels > 1 and len(args.level_iterations) != args.levels:
        raise SystemExit("--level_iterations needs %d values, coarsest first" % args.levels)
    if args.view_prior < 0 or args.view_prior > abi.MAX_VIEWS:
        raise SystemExit("--view_prior must be 0..%d" % abi.MAX_VIEWS)
    if args.view_prior and args.levels > 1:
        raise SystemExit("--view_prior cannot be combined with --levels > 1: a view starts either from its coarser level "
                         "or from its solved neighbours")
    if args.view_prior and (args.prior_iterations < 0 or args.prior_min_views < 1):
        raise SystemExit("--prior_iterations must be >= 0 and --prior_min_views >= 1")
    if args.view_prior and args.view_prior < args.prior_min_views:
        raise SystemExit("--view_prior %d is below --prior_min_views %d: no view would ever start from a prior"
                         % (args.view_prior, args.prior_min_views))
    if args.fuse and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--fuse works within one process (there is no exchange of results between ranks): run "
                         "`python -m gipuma_amd.fusion --input-folder %s ...` once every rank is done" % args.output_folder)
    return args


def fuse_solved(scan):
    """--fuse: the views solved in this run, from memory, into <output-folder>/fused.ply; returns the report's entry"""
    from . import fusion
    args, names = scan.args, scan.names
    # the views solved here, in the scan's order (that of the fusion CLI on the dumps); skipped ones are left out
    fused_views = [n for n in names if n in scan.solved]
    if len(fused_views) < 2:
        raise SystemExit("--fuse needs at least 2 solved views, this run solved %d" % len(fused_views))
    points, info = fusion.fuse([scan.solved[n] for n in fused_views], [scan.dev[names.index(n)] for n in fused_views],
                               [scan.P_all[names.index(n)] for n in fused_views], args.cam_scale, args.disp_thresh,
                               args.normal_thresh, args.num_consistent, args.depth_min, args.depth_max,
                               device_id=scan.dev[0].device.index, return_info=True)
    filtered = {}
    if args.fuse_neighbour_radius > 0:  # (the isolated points go before the cloud is written and scored)
        from . import cloud_eval
        kept, ms, _ = cloud_eval.drop_isolated(np.stack([points["x"], points["y"], points["z"]], axis=-1), args.fuse_neighbour_radius,
                                               args.fuse_min_neighbours, device_id=scan.dev[0].device.index, return_info=True)
        filtered = {"points_before_filter": int(len(points)), "filter_device_ms": ms}
        points = points[kept]
    if args.fuse_outlier_radius > 0:  # (then the statistical outliers, of the cloud the count has cleaned)
        from . import cloud_eval
        kept, ms, o = cloud_eval.drop_outliers(np.stack([points["x"], points["y"], points["z"]], axis=-1), args.fuse_outlier_radius,
                                               args.fuse_outlier_k, args.fuse_outlier_std, device_id=scan.dev[0].device.index,
                                               return_info=True)
        filtered.update({"points_before_outliers": int(len(points)), "outlier_threshold": o["threshold"], "outlier_device_ms": ms})
        points = points[kept]
    if args.fuse_component_radius > 0:  # (then the small clumps, which neither of the two can see)
        from . import cloud_eval
        kept, ms, c = cloud_eval.drop_small_components(np.stack([points["x"], points["y"], points["z"]], axis=-1),
                                                       args.fuse_component_radius, args.fuse_min_component,
                                                       device_id=scan.dev[0].device.index, return_info=True)
        filtered.update({"points_before_components": int(len(points)), "components": c["components"], "component_device_ms": ms})
        points = points[kept]
    if args.fuse_normal_radius > 0:  # (then the points fused at a wrong plane among good neighbours: the first stage that reads the normals)
        from . import cloud_eval
        kept, ms, _ = cloud_eval.drop_disagreeing_normals(np.stack([points["x"], points["y"], points["z"]], axis=-1),
                                                          np.stack([points["nx"], points["ny"], points["nz"]], axis=-1),
                                                          args.fuse_normal_radius, args.fuse_normal_k, args.fuse_max_normal_angle,
                                                          device_id=scan.dev[0].device.index, return_info=True)
        filtered.update({"points_before_normals": int(len(points)), "normal_device_ms": ms})
        points = points[kept]
    dmb.write_points_ply(os.path.join(args.output_folder, "fused.ply"), points)
    scan.fused_xyz = np.stack([points["x"], points["y"], points["z"]], axis=-1)  # (for --eval_cloud)
    return {"points": int(len(points)), "device_ms": info["device_ms"],
            "views": [{"name": n, "emitted": int(c)} for n, c in zip(fused_views, info["per_view"])], **filtered}


def score_fused(scan):
    """--eval_cloud: the fused cloud of this run against the reference cloud; returns the report's `cloud_score`"""
    from . import cloud_eval
    args = scan.args
    out = cloud_eval.score(scan.fused_xyz, dmb.read_ply_xyz(args.eval_cloud), args.eval_max_dist,
                           device_id=scan.dev[0].device.index, reduce=args.eval_reduce)
    out["reference"] = args.eval_cloud
    return out


def write_report(scan, head, pyr, order, fused, cloud_score=None):
    """batch_rank<rank>.json: `head`, the options of the strategy that ran, the throughput and the per-view entries"""
    args, t_batch = scan.args, head["batch_seconds"]
    n_done = sum(1 for r in scan.report if "skipped" not in r)
    out = {**head,
           **({"levels": args.levels, "level_iterations": args.level_iterations, "pyramid_device_ms": pyr.device_ms}
              if pyr is not None else {}),
           **({"view_prior": args.view_prior, "prior_iterations": args.prior_iterations,
               "prior_min_views": args.prior_min_views, "prior_max_cost": args.prior_max_cost, "order": order}
              if args.view_prior else {}),
           "mpix_per_s_batch": n_done * scan.rows * scan.cols / max(t_batch, 1e-9) / 1e6,
           "views": scan.report, **({"fusion": fused} if fused is not None else {}),
           **({"cloud_score": cloud_score} if cloud_score is not None else {})}
    with open(os.path.join(args.output_folder, "batch_rank%d.json" % head["rank"]), "w") as f:
        json.dump(out, f, indent=1)


def main(argv=None):
    args = parse_args(argv)
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise abi.GipumaHipError("gipuma_amd.batch needs a GPU; there is no CPU fallback")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    scan = Scan(args, dev_index)
    refs = scan.names if args.views == "all" else [v for v in args.views.split(",") if v]
    mine = views_for_rank(refs, rank, world) if len(refs) >= world else refs[rank:rank + 1]
    os.makedirs(args.output_folder, exist_ok=True)
    in_flight = max(1, args.in_flight)
    pyr = None
    if args.levels > 1:
        from . import pyramid
        pyr = pyramid.ScanPyramid(scan.dev, args.levels)  # the coarse planes of the whole scan, once
    t_batch0 = time.perf_counter()
    order = None  # (--view_prior: the order the views were solved in)
    try:
        if args.view_prior:
            order = solve_with_view_prior(scan, mine)
        elif pyr is not None:
            solve_levels(scan, mine, pyr, args.level_iterations, timing=in_flight == 1)
        else:
            solve_plain(scan, mine, in_flight)
    finally:
        if pyr is not None:
            pyr.close()  # (clears the image cache before the coarse planes are released)
        # an error above must not leave the image cache behind: its entries are keyed by the device addresses of the
        # scan's tensors, which torch hands out again once they are freed (the library refuses while a session still
        # uses them)
        abi.load_library().gipuma_hip_cache_clear()
    t_batch = time.perf_counter() - t_batch0
    fused = fuse_solved(scan) if args.fuse else None
    write_report(scan, {"rank": rank, "world": world, "device": dev_index, "load_seconds": scan.load_seconds,
                        "in_flight": in_flight, "batch_seconds": t_batch}, pyr, order, fused,
                 score_fused(scan) if args.eval_cloud is not None else None)
    print("rank %d/%d: %d reference views on cuda:%d" % (rank, world, len(scan.report), dev_index))
    return 0


if __name__ == "__main__":
    sys.exit(main())
