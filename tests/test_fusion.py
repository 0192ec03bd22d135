"""Depth-map fusion (gipuma_amd.fusion).  CPU: known answers of the restatement (tests/fusion_ref.py), the
camera constants, the PLY writer, the CLI's folders and the C-ABI's argument checks.  GPU: the kernels equal the
restatement in every bit, are deterministic, put fused points on the surface, and the batch runner's --fuse equals the
CLI on the dumps."""
import collections
import contextlib
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gipuma_amd import abi, cameras, dmb, fusion, synth
from tests import fusion_ref
from tests.abi_layout import assert_mirrors_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# synthetic scans
# ----------------------------------------------------------------------------------------------------------------------
def _pinhole(f, cx, cy, R, Cc):
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return K @ np.concatenate([R, (-R @ np.asarray(Cc, dtype=np.float64))[:, None]], axis=1)


def _plane_views(Ps, depths, rows, cols, normal=(0.0, 0.0, -1.0)):
    """norm4 planes of constant depth and normal"""
    out = []
    for z in depths:
        n4 = np.empty((rows, cols, 4), dtype=f32)
        n4[..., :3] = normal
        n4[..., 3] = z
        out.append(n4)
    return out


def _dtu_views(n, cols, rows, ref=15):
    allP = synth.dtu_projection_matrices()
    order = [ref] + [k for k in sorted(allP) if k != ref]
    cs_all = cameras.get_camera_parameters([allP[k] for k in order], cam_scale=1600.0 / cols)
    cand, _, _ = cameras.select_views(cs_all, cols, rows, 10.0, 30.0, max_views=10 ** 6)
    pick = [cand[(i * len(cand)) // n] for i in range(n)]
    return [allP[ref]] + [allP[order[i]] for i in pick]


class Scan:
    pass


def make_scan(n_views, cols, rows, seed, perturb=True, facing=False, gray_missing=None):
    """DTU cameras at cam_scale 1600/cols looking at synth.Surface; depth and world normals (oriented towards each
    camera) from the analytic surface; with `perturb`, deterministic damage from `seed` that reaches every branch of the
    contract; `facing`: one more camera behind the surface looking back at the others (points beyond it are behind it)."""
    s = Scan()
    s.cam_scale = 1600.0 / cols
    Ps = _dtu_views(n_views - 1 - (1 if facing else 0), cols, rows)
    K0, R0, C0 = cameras.decompose_projection(Ps[0])
    if facing:
        Rf = np.diag([1.0, -1.0, -1.0]) @ R0
        Ps.append(K0 @ np.concatenate([Rf, (-Rf @ (C0 + R0.T @ np.array([0.0, 0.0, 760.0])))[:, None]], axis=1))
    cs = cameras.get_camera_parameters(Ps, cam_scale=s.cam_scale)
    s.surface = synth.Surface(600.0, 25.0, 160.0, pixel_footprint=600.0 / cs.f, seed=seed)
    s.R0, s.t0 = R0, -R0 @ C0
    s.Ps, s.norm4s, s.grays = Ps, [], []
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    pix = np.stack([u, v, np.ones_like(u)], -1)
    for i in range(len(Ps)):
        img, depth = synth.render(s.surface, cs.K[i], cs.R[i], cs.t[i], rows, cols)
        d = depth.numpy().astype(np.float64)
        Xr = (d[..., None] * (pix @ np.linalg.inv(cs.K[i]).T) - cs.t[i]) @ cs.R[i]   # reference-camera coordinates
        hx, hy = s.surface.grad(torch.from_numpy(Xr[..., 0]), torch.from_numpy(Xr[..., 1]))
        nr = np.stack([-hx.numpy(), -hy.numpy(), np.ones_like(u)], -1)
        nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
        o = -cs.R[i].T @ cs.t[i]
        nr[((o - Xr) * nr).sum(-1) < 0] *= -1.0
        n4 = np.concatenate([nr @ R0, d[..., None]], axis=-1).astype(f32)
        if perturb:
            r = rng.random((rows, cols))
            z = n4[..., 3]
            z[r < 0.03] = 0.0                                                  # holes
            z[(r >= 0.03) & (r < 0.04)] = np.nan
            z[(r >= 0.04) & (r < 0.05)] = 900.0                                # beyond depth_max
            z[(r >= 0.05) & (r < 0.055)] = 200.0                               # before depth_min
            out = (r >= 0.055) & (r < 0.09)                                    # depth outliers
            z[out] *= (1.0 + np.sign(rng.random(out.sum()) - 0.5) * rng.uniform(0.06, 0.2, out.sum())).astype(f32)
            flip = (r >= 0.09) & (r < 0.11)                                    # normals the wrong way
            n4[flip, :3] *= -1.0
            z[(r >= 0.11) & (r < 0.12)] = 795.0                                # beyond the facing camera
        s.norm4s.append(n4)
        s.grays.append(None if i == gray_missing else img.numpy())
    return s


def _consts(s):
    return [fusion.view_constants(P, s.cam_scale) for P in s.Ps]


def _ref(s, disp, nc, depth=(300.0, 800.0), normal_thresh=30.0):
    return fusion_ref.fuse(s.norm4s, s.grays, _consts(s), disp, fusion.cos_threshold(normal_thresh), nc, *depth)


def _surface_distance(s, xyz):
    """vertical distance of world points to the analytic surface, in the reference camera's frame"""
    Xr = np.asarray(xyz, dtype=np.float64) @ s.R0.T + s.t0
    h = s.surface.h(torch.from_numpy(Xr[:, 0]), torch.from_numpy(Xr[:, 1])).numpy()
    return np.abs(Xr[:, 2] - h)


def _xyz(points):
    return np.stack([points["x"], points["y"], points["z"]], -1)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's known answers
# ----------------------------------------------------------------------------------------------------------------------
def test_two_views_with_the_same_camera_fuse_every_valid_pixel_to_itself():
    P = _pinhole(100.0, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0))
    rng = np.random.default_rng(3)
    n4 = _plane_views([P], [0.0], 30, 40)[0]
    n4[..., 3] = rng.uniform(300.0, 700.0, (30, 40))
    n4[rng.random((30, 40)) < 0.1, 3] = 0.0
    consts = [fusion.view_constants(P)] * 2
    r = fusion_ref.fuse([n4, n4.copy()], [None, None], consts, 0.1, fusion.cos_threshold(30), 1)
    valid = n4[..., 3] > 0
    assert r.per_view == [int(valid.sum()), 0]
    ys, xs = np.nonzero(valid)
    X = fusion_ref.backproject(consts[0], n4[ys, xs, 3], xs.astype(f32), ys.astype(f32))
    assert np.array_equal(_xyz(r.points), np.stack(X, -1))
    assert np.array_equal(r.used[1], valid.astype(np.uint8)) and not r.used[0].any()


def test_disparity_difference_on_a_fronto_parallel_plane_in_closed_form():
    """cameras translated along x by b; view 0 sees the plane at Z0, view 1's map says Z1: the disparity difference is
    |fb/Z0 - fb/Z1| with fb = f32(f 0.54) -- consistent just above that threshold, not just below"""
    f, b, Z0, Z1 = 100.0, 4.0, 400.0, 410.0
    Ps = [_pinhole(f, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0)), _pinhole(f, 20.0, 15.0, np.eye(3), (b, 0.0, 0.0))]
    n4s = _plane_views(Ps, [Z0, Z1], 30, 40)
    fb = float(f32(f32(f) * f32(0.54)))
    diff = abs(fb / Z0 - fb / Z1)
    for thresh, expect in ((diff * 1.001, True), (diff * 0.999, False)):
        r = fusion_ref.fuse(n4s, [None, None], [fusion.view_constants(P) for P in Ps], thresh, fusion.cos_threshold(30), 1)
        assert (r.per_view[0] > 0) == expect
        if expect:  # every pixel whose partner x - f b / Z0 = x - 1 lies inside view 1
            assert r.per_view[0] == 30 * 39
        else:
            assert r.tally["disparity"] > 0 and sum(r.per_view) == 0


def test_num_consistent_at_the_threshold_and_one_above():
    P = _pinhole(100.0, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0))
    n4s = _plane_views([P] * 3, [500.0] * 3, 30, 40)
    consts = [fusion.view_constants(P)] * 3
    at = fusion_ref.fuse(n4s, [None] * 3, consts, 0.1, fusion.cos_threshold(30), 2)
    above = fusion_ref.fuse(n4s, [None] * 3, consts, 0.1, fusion.cos_threshold(30), 3)
    assert at.per_view == [1200, 0, 0] and above.per_view == [0, 0, 0] and above.tally["too_few"] == 3 * 1200


def test_used_marks_emit_each_surface_point_once():
    """three cameras 1 and 2 units apart see the plane Z = 50 with f = 100: 2 and 4 pixels of disparity.  Every surface
    point seen by two or more views is emitted exactly once"""
    rows, cols = 12, 40
    Ps = [_pinhole(100.0, 20.0, 6.0, np.eye(3), (b, 0.0, 0.0)) for b in (0.0, 1.0, 2.0)]
    n4s = _plane_views(Ps, [50.0] * 3, rows, cols)
    r = fusion_ref.fuse(n4s, [None] * 3, [fusion.view_constants(P) for P in Ps], 0.1, fusion.cos_threshold(30), 1)
    xyz = _xyz(r.points)
    assert len(np.unique(np.round(xyz, 3), axis=0)) == len(xyz) == rows * cols
    assert r.per_view == [rows * (cols - 2), rows * 2, 0]


def test_view_constants_back_project_like_get3dpoint():
    """c + z bp (x, y, 1) == get3Dpoint through the camera that is not re-centred (dmb.ply_points), to float32 rounding"""
    P = synth.dtu_projection_matrices()[15]
    k = fusion.view_constants(P, 1.0)
    K, R, Cc = cameras.decompose_projection(P)
    Pn = K @ np.concatenate([R, (-R @ Cc)[:, None]], axis=1)
    rng = np.random.default_rng(5)
    depth = rng.uniform(300.0, 800.0, (40, 60)).astype(f32)
    want = dmb.ply_points(depth, np.linalg.inv(Pn[:, :3]), Pn[:, 3])
    yy, xx = np.mgrid[0:40, 0:60]
    got = np.stack(fusion_ref.backproject(k, depth, xx.astype(f32), yy.astype(f32)), -1)
    assert np.allclose(got, want, rtol=0, atol=2e-6 * np.abs(want).max() + 1e-3)
    assert k["fb"] == f32(f32(K[0, 0]) * f32(0.54))


def test_write_points_ply_round_trips():
    v = np.zeros(5, dtype=dmb._PLY_VERTEX)
    for name in ("x", "y", "z", "nx", "ny", "nz"):
        v[name] = np.arange(5, dtype=f32) * 1.5 - 2
    v["red"] = v["green"] = v["blue"] = np.arange(5) * 50
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "p.ply")
        dmb.write_points_ply(p, v)
        back = dmb.read_ply_binary(p)
        assert back.tobytes() == v.tobytes() and os.path.getsize(p) == len(open(p, "rb").read().split(b"end_header\n")[0]) + 11 + 27 * 5


def _write_results(root, name, n4, layout):
    if layout == "batch":
        folder = os.path.join(root, os.path.splitext(name)[0])
    else:
        folder = os.path.join(root, "%s_%s" % (layout, name[:-4]))
    os.makedirs(folder, exist_ok=True)
    dmb.write_dmb(os.path.join(folder, "disp.dmb"), n4[..., 3])
    dmb.write_dmb(os.path.join(folder, "normals.dmb"), n4[..., :3])
    return folder


def _write_scan(tmp, names, rows, cols):
    img, cal = os.path.join(tmp, "img"), os.path.join(tmp, "cal")
    os.makedirs(img)
    os.makedirs(cal)
    P = synth.dtu_projection_matrices()
    for k, n in enumerate(names):
        with open(os.path.join(img, n), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (cols, rows) + bytes(rows * cols))
        with open(os.path.join(cal, n + ".P"), "w") as f:
            for row in P[sorted(P)[k]]:
                f.write(" ".join("%.6f" % x for x in row) + "\n")
    return img, cal


def test_cli_finds_both_result_layouts_and_rejects_bad_input(tmp_path):
    names = ["a_000.pgm", "a_001.pgm", "a_002.pgm"]
    img, cal = _write_scan(str(tmp_path), names, 6, 8)
    res = str(tmp_path / "res")
    n4 = np.ones((6, 8, 4), dtype=f32)
    assert _write_results(res, names[0], n4, "batch") == fusion.result_folder(res, names[0])
    _write_results(res, names[1], n4, "20260101_120000")
    newest = _write_results(res, names[1], n4, "20260102_080000")
    assert fusion.result_folder(res, names[1]) == newest
    assert fusion.result_folder(res, names[2]) is None
    base = ["--input-folder", res, "--images-folder", img, "--p-folder", cal, "--output", str(tmp_path / "f.ply")]
    with pytest.raises(SystemExit, match="no result"):       # a listed view without a result
        fusion.main(base + ["--views", ",".join(names)])
    with pytest.raises(SystemExit, match="no image"):
        fusion.main(base + ["--views", "a_000.pgm,zzz.pgm"])
    _write_results(res, names[2], np.ones((5, 8, 4), dtype=f32), "batch")
    with pytest.raises(SystemExit, match="differ"):          # sizes that do not match
        fusion.main(base)
    with pytest.raises(ValueError, match="same size"):
        fusion.fuse([n4, n4[:5]], [None, None], [np.eye(3, 4)] * 2)


def _desc(views, n, **kw):
    d = abi.FusionDesc()
    d.abi_version, d.rows, d.cols, d.n_views = abi.ABI_VERSION, 4, 4, n
    d.views = C.cast(views, C.POINTER(abi.FusionView))
    d.disp_thresh, d.normal_thresh, d.num_consistent = 0.1, 30.0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_fuse_validates_its_arguments_and_needs_a_device():
    """argument errors before anything else; then, on a box without a device, a loud error and no CPU fallback"""
    lib = abi.load_library()
    host = np.zeros((4, 4, 4), dtype=f32)
    views = (abi.FusionView * 3)()
    for v in views:
        v.norm4 = host.ctypes.data
    h = C.c_void_p()
    for kw in (dict(n_views=1), dict(n_views=513), dict(num_consistent=0), dict(abi_version=2), dict(rows=0)):
        assert lib.gipuma_hip_fuse(C.byref(_desc(views, 3, **kw)), C.byref(h)) == abi.ERR_ARG, kw
    views[1].norm4 = None
    assert lib.gipuma_hip_fuse(C.byref(_desc(views, 3)), C.byref(h)) == abi.ERR_ARG
    assert b"norm4" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_fuse(None, C.byref(h)) == abi.ERR_ARG and lib.gipuma_hip_fusion_free(None) == 0
    if lib.gipuma_hip_device_count() == 0:
        views[1].norm4 = host.ctypes.data
        assert lib.gipuma_hip_fuse(C.byref(_desc(views, 3)), C.byref(h)) == abi.ERR_NO_DEVICE
        assert b"no CPU fallback" in lib.gipuma_hip_last_error()
        with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
            fusion.fuse([host, host], [None, None], [np.eye(3, 4)] * 2)
    else:  # (host pointers never reach the device: the device path goes through fusion.fuse)
        P = _pinhole(10.0, 2.0, 2.0, np.eye(3), (0.0, 0.0, 0.0))
        n4 = _plane_views([P], [5.0], 4, 4)[0]
        assert len(fusion.fuse([n4, n4], [None, None], [P, P], num_consistent=1)) == 16


def test_fusion_structs_match_the_header_layout():
    fields = {"gipuma_hip_fusion_view": (abi.FusionView, ["norm4", "gray", "bp", "c", "P", "fb"]),
              "gipuma_hip_fusion_desc": (abi.FusionDesc, ["abi_version", "rows", "cols", "n_views", "views", "disp_thresh",
                                                          "normal_thresh", "num_consistent", "depth_min", "depth_max",
                                                          "device_id", "stream"])}
    for s, (py, fs) in fields.items():
        assert_mirrors_header(py, s, fs)


def test_fusion_kernels_use_global_not_flat_memory_instructions():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "f.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--offload-device-only", "-o", out, "gipuma_fuse.hip"],
                              cwd=os.path.join(ROOT, "gipuma_amd", "csrc"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    for k in ("evaluate_kernel", "scan_kernel", "scatter_kernel"):
        assert "_ZN4fuse%d%s" % (len(k), k) in asm
    ops = [l.split()[0] for l in asm.splitlines() if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_")]
    assert "global_load_dwordx4" in ops and not [o for o in ops if "atomic" in o]


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
SCANS = {  # name: (views, cols, rows, seed, facing camera, view without gray)
    "dtu5_160": (5, 160, 120, 11, True, 2),
    "dtu8_320": (8, 320, 240, 12, True, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("num_consistent", [1, 3])
@pytest.mark.parametrize("scan", sorted(SCANS))
def test_kernels_equal_the_restatement_bit_for_bit(hip, scan, num_consistent):
    V, cols, rows, seed, facing, nogray = SCANS[scan]
    s = make_scan(V, cols, rows, seed, facing=facing, gray_missing=nogray)
    disp = 0.1 / s.cam_scale  # 0.1 at full DTU size
    pts, info = fusion.fuse(s.norm4s, s.grays, s.Ps, s.cam_scale, disp, 30.0, num_consistent, 300.0, 800.0,
                            return_info=True)
    ref = _ref(s, disp, num_consistent)
    assert info["per_view"] == ref.per_view
    assert pts.tobytes() == ref.points.tobytes()
    assert np.array_equal(info["used"], ref.used)
    assert len(pts) > 0 and all(ref.tally[r] > 0 for r in fusion_ref.REASONS), ref.tally


@pytest.mark.gpu
def test_fusion_is_deterministic_from_host_arrays_and_device_tensors(hip):
    s = make_scan(6, 320, 240, 21, facing=True)
    a = fusion.fuse(s.norm4s, s.grays, s.Ps, s.cam_scale, 0.02, 30.0, 2, 300.0, 800.0)
    dev = [torch.from_numpy(n).cuda() for n in s.norm4s]
    gdev = [torch.from_numpy(g).cuda() for g in s.grays]
    b = fusion.fuse(dev, gdev, s.Ps, s.cam_scale, 0.02, 30.0, 2, 300.0, 800.0)
    assert len(a) > 0 and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_fused_ground_truth_lies_on_the_surface(hip):
    """unperturbed maps: most pixels of the first view are emitted; every point lies on the analytic surface and every
    normal agrees with it"""
    s = make_scan(5, 320, 240, 31, perturb=False)
    pts, info = fusion.fuse(s.norm4s, s.grays, s.Ps, s.cam_scale, 0.1 / s.cam_scale, 30.0, 3, 300.0, 800.0,
                            return_info=True)
    dist = _surface_distance(s, _xyz(pts))
    Xr = _xyz(pts).astype(np.float64) @ s.R0.T + s.t0
    hx, hy = s.surface.grad(torch.from_numpy(Xr[:, 0]), torch.from_numpy(Xr[:, 1]))
    nr = np.stack([-hx.numpy(), -hy.numpy(), np.ones(len(pts))], -1)
    nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
    nw = np.stack([pts["nx"], pts["ny"], pts["nz"]], -1).astype(np.float64) @ s.R0.T
    ang = np.degrees(np.arccos(np.clip(np.abs((nr * nw).sum(-1)), 0, 1)))
    print("fused %d points, first view %.3f of its pixels; distance max %.4f, normal max %.3f deg"
          % (len(pts), info["per_view"][0] / (320 * 240), dist.max(), ang.max()))
    # bounds from the first run on an MI355X (equal to the restatement's): 0.863 of the first view's pixels, distance at
    # most 0.0101 (scene units; the pixel footprint is about 2), normals within 0.041 degrees
    assert info["per_view"][0] > 0.8 * 320 * 240
    assert dist.max() < 0.05 and ang.max() < 0.5


@pytest.fixture(scope="module")
def batch_scan(tmp_path_factory):
    """a tiny scan on disk, solved by the batch runner with --fuse (as tests/test_batch_eval.py writes it)"""
    from gipuma_amd import batch
    tmp = tmp_path_factory.mktemp("fuse_batch")
    cfg = synth.tiny_config(cols=96, rows=64, n_src=4, blocksize=9, iterations=3, n_best=2)
    gs, info = synth.build_problem(cfg)
    img_dir, p_dir, out = tmp / "img", tmp / "calib", tmp / "out"
    img_dir.mkdir()
    p_dir.mkdir()
    P = synth.dtu_projection_matrices()
    for im, vid in zip(gs.images, info["view_ids"]):
        name = "rect_%03d.pgm" % vid
        with open(img_dir / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (gs.cols, gs.rows) + im.astype(np.uint8).tobytes())
        with open(p_dir / (name + ".P"), "w") as f:
            for r in P[vid]:
                f.write(" ".join("%.6f" % v for v in r) + "\n")
    cam_scale = "%.9g" % np.float32(cfg["cam_scale"])
    fuse_args = ["--depth_min=300", "--depth_max=800", "--cam_scale=" + cam_scale, "--disp_thresh=0.02",
                 "--normal_thresh=30", "--num_consistent=2"]
    rc = batch.main(["--images-folder", str(img_dir), "--p-folder", str(p_dir), "--output-folder", str(out),
                     "--blocksize=9", "--iterations=3", "--n_best=2", "--min_angle=2", "--max_angle=60",
                     "--max_views=10", "--fuse"] + fuse_args)
    assert rc == 0
    return dict(img=str(img_dir), calib=str(p_dir), out=str(out), fuse_args=fuse_args, info=info, tmp=tmp,
                cam_scale=float(np.float32(cam_scale)))


@pytest.mark.gpu
def test_batch_fuse_equals_the_cli_and_the_restatement_on_the_dumps(hip, batch_scan):
    out = batch_scan["out"]
    fused = open(os.path.join(out, "fused.ply"), "rb").read()
    cli_ply = str(batch_scan["tmp"] / "cli.ply")
    assert fusion.main(["--input-folder", out, "--images-folder", batch_scan["img"], "--p-folder", batch_scan["calib"],
                        "--output", cli_ply] + batch_scan["fuse_args"]) == 0
    assert open(cli_ply, "rb").read() == fused
    rep = json.load(open(str(batch_scan["tmp"] / "cli.json")))
    assert rep["points"] == len(dmb.read_ply_binary(cli_ply)) > 0 and rep["device_ms"] > 0
    from gipuma_amd.batch import read_image
    names = sorted(n for n in os.listdir(batch_scan["img"]))
    n4s = [fusion.read_norm4(fusion.result_folder(out, n)) for n in names]
    grays = [read_image(os.path.join(batch_scan["img"], n)) for n in names]
    Ps = [cameras.read_p_file(os.path.join(batch_scan["calib"], n + ".P")) for n in names]
    ref = fusion_ref.fuse(n4s, grays, [fusion.view_constants(P, batch_scan["cam_scale"]) for P in Ps], f32(0.02),
                          fusion.cos_threshold(30.0), 2, 300.0, 800.0)
    ref_ply = str(batch_scan["tmp"] / "ref.ply")
    dmb.write_points_ply(ref_ply, ref.points)
    assert open(ref_ply, "rb").read() == fused
    rep = json.load(open(os.path.join(out, "batch_rank0.json")))
    assert rep["fusion"]["points"] == len(ref.points)
    # (--fuse alone: the keys of --view_prior, the solve order among them, are not in the report)
    assert not {"order", "view_prior", "prior_iterations", "prior_min_views", "prior_max_cost"} & set(rep)


@pytest.mark.gpu
def test_fusion_removes_the_solver_outliers(hip, batch_scan):
    """95th percentile of the distance to the surface: fused points below all per-view points of the solves"""
    out, info = batch_scan["out"], batch_scan["info"]
    s = Scan()
    s.surface = info["surface"]
    K0, s.R0, C0 = cameras.decompose_projection(info["P_matrices"][0])
    s.t0 = -s.R0 @ C0
    fused = dmb.read_ply_binary(os.path.join(out, "fused.ply"))
    every = []
    for n in sorted(os.listdir(batch_scan["img"])):
        n4 = fusion.read_norm4(fusion.result_folder(out, n))
        k = fusion.view_constants(cameras.read_p_file(os.path.join(batch_scan["calib"], n + ".P")), batch_scan["cam_scale"])
        ys, xs = np.nonzero((n4[..., 3] >= 300) & (n4[..., 3] <= 800))
        every.append(np.stack(fusion_ref.backproject(k, n4[ys, xs, 3], xs.astype(f32), ys.astype(f32)), -1))
    p_all = np.percentile(_surface_distance(s, np.concatenate(every)), 95)
    p_fused = np.percentile(_surface_distance(s, _xyz(fused)), 95)
    print("p95 distance to the surface: all per-view points %.3f, fused %.3f (%d points)" % (p_all, p_fused, len(fused)))
    assert p_fused < p_all


# ----------------------------------------------------------------------------------------------------------------------
# the limits of the kernels and of the host loop ("limits pinned"): frames that do not fill their last
# workgroup, more workgroups than one chunk of the scan, an output that outgrows its buffer, views that emit nothing,
# 512 views, point ranges, a caller's stream.  Every scene is built once, restated once (tests/fusion_ref.py) and judged
# by a condition function that says what the scene is there for -- checked on the restatement alone without a device,
# and again by the GPU test that compares the kernels with it.
# ----------------------------------------------------------------------------------------------------------------------
WORKGROUP = 256  # fuse::kBlock: pixels per workgroup of evaluate_kernel / scatter_kernel
SCAN_CHUNK = 1024  # fuse::kScan: workgroup counts per chunk of scan_kernel


def _workgroups(npix):
    return -(-npix // WORKGROUP)


def _group_counts(mask):
    """points per workgroup of one view's emitted mask"""
    flat = mask.reshape(-1)
    pad = np.zeros(_workgroups(flat.size) * WORKGROUP, dtype=np.int64)
    pad[:flat.size] = flat
    return pad.reshape(-1, WORKGROUP).sum(1)


Case = collections.namedtuple("Case", "norm4s grays Ps cam_scale disp normal_thresh num_consistent ref")


def _case(norm4s, grays, Ps, cam_scale, disp, normal_thresh, nc, depth=(300.0, 800.0)):
    consts = [fusion.view_constants(P, cam_scale) for P in Ps]
    ref = fusion_ref.fuse(norm4s, grays, consts, disp, fusion.cos_threshold(normal_thresh), nc, *depth)
    return Case(norm4s, grays, Ps, cam_scale, disp, normal_thresh, nc, ref)


@functools.lru_cache(maxsize=None)
def _scan_case(n_views, cols, rows, seed, nc):
    s = make_scan(n_views, cols, rows, seed)
    return _case(s.norm4s, s.grays, s.Ps, s.cam_scale, 0.1 / s.cam_scale, 30.0, nc)


def _fuse_case(c, **kw):
    return fusion.fuse(c.norm4s, c.grays, c.Ps, c.cam_scale, c.disp, c.normal_thresh, c.num_consistent, 300.0, 800.0,
                       return_info=True, **kw)


def _assert_equals_ref(pts, per_view, used, ref, what):
    """points, per-view counts and used masks in every byte; the message names the first record that differs"""
    assert list(per_view) == ref.per_view, "%s: per_view %r, restated %r" % (what, list(per_view), ref.per_view)
    if pts.tobytes() != ref.points.tobytes():
        a, b = np.frombuffer(pts.tobytes(), np.uint8).reshape(-1, 27), np.frombuffer(ref.points.tobytes(), np.uint8).reshape(-1, 27)
        k = int(np.nonzero((a != b).any(1))[0][0])
        view = int(np.searchsorted(np.cumsum(ref.per_view), k, side="right"))
        raise AssertionError("%s: %d of %d records differ, first at %d (view %d): %r, restated %r"
                             % (what, int((a != b).any(1).sum()), len(a), k, view, pts[k], ref.points[k]))
    bad = [v for v in range(len(ref.used)) if not np.array_equal(used[v], ref.used[v])]
    assert not bad, "%s: the used masks of views %r differ" % (what, bad)


# -- frames that do not fill their last workgroup ------------------------------------------------------------------------
RAGGED = {  # name: (cols, rows, seed, range of rows * cols % 256, the last workgroup must hold emitted points)
    "161x113": (161, 113, 41, (1, 63), True),     # 17 pixels in the last workgroup: one partial wavefront, three empty
    "67x45": (67, 45, 42, (193, 255), True),      # 199: the last wavefront of the last workgroup is the partial one
    "7x5": (7, 5, 43, (1, 63), False),            # less than one wavefront
    "333x1": (333, 1, 44, (65, 127), False),      # a single row, two workgroups
}


def _ragged_case(name):
    cols, rows, seed = RAGGED[name][:3]
    return _scan_case(4, cols, rows, seed, 1)


def _ragged_condition(name, ref):
    cols, rows, _, (lo, hi), in_last = RAGGED[name]
    npix = rows * cols
    assert lo <= npix % WORKGROUP <= hi
    assert sum(ref.per_view) > 0 and len(set(ref.per_view)) > 1
    if in_last:  # points inside the last, partly filled workgroup -- and the workgroups differ in their counts
        last = (_workgroups(npix) - 1) * WORKGROUP
        assert ref.emitted[0].reshape(-1)[last:].any()
        assert len(set(_group_counts(ref.emitted[0]))) > 1


# -- more workgroups than one chunk of scan_kernel ---------------------------------------------------------------------
CHUNKED = {  # name: (cols, rows, seed, workgroups, chunks)
    "512x512": (512, 512, 51, 1024, 1),       # the chunk exactly full
    "530x495": (530, 495, 52, 1025, 2),       # the second chunk: one workgroup, 206 pixels
    "540x490": (540, 490, 53, 1034, 2),       # ten workgroups into the second chunk, the last with 152 pixels
    "800x660": (800, 660, 54, 2063, 3),       # 528 000 pixels
}


def _chunked_case(name):
    cols, rows, seed = CHUNKED[name][:3]
    return _scan_case(3, cols, rows, seed, 1)


def _chunked_condition(name, ref):
    cols, rows, _, groups, chunks = CHUNKED[name]
    npix = rows * cols
    assert _workgroups(npix) == groups and -(-groups // SCAN_CHUNK) == chunks
    counts = _group_counts(ref.emitted[0])
    assert len(counts) == groups and len(set(counts)) > 1
    for k in range(chunks):  # view 0 emits in every chunk: each carry is non-zero and each chunk's offsets are used
        assert counts[k * SCAN_CHUNK:(k + 1) * SCAN_CHUNK].sum() > 0, (name, k)


# -- an output that outgrows its buffer --------------------------------------------------------------------------------
PAIR_DEPTHS = (400.0, 450.0, 500.0, 550.0, 600.0)


@functools.lru_cache(maxsize=None)
def _pairs_case(cols, rows):
    """ten views in five pairs, all through one pinhole camera; both views of a pair see the fronto-parallel plane at the
    pair's depth.  fb = 54.000004: neighbouring pairs are 0.008 .. 0.015 apart in disparity, disp_thresh is 0.005 -- a view
    agrees with its partner only.  The first of a pair emits every pixel and marks every pixel of the second."""
    P = _pinhole(100.0, cols / 2.0, rows / 2.0, np.eye(3), (0.0, 0.0, 0.0))
    Ps = [P] * 10
    n4s = _plane_views(Ps, [z for z in PAIR_DEPTHS for _ in (0, 1)], rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols]
    grays = [((xx * 3 + yy * 5 + 37 * (v // 2) + 11 * (v % 2)) % 200).astype(f32) for v in range(10)]
    return _case(n4s, grays, Ps, 1.0, 0.005, 30.0, 1)


def _pairs_condition(cols, rows, ref):
    """capacity starts at npix: view 0 fills it exactly; views 2, 4 and 8 each need a larger buffer (2, 4, 8 npix)"""
    npix = rows * cols
    assert ref.per_view == [npix, 0] * 5 and sum(ref.per_view) == 5 * npix > 4 * npix
    capacity, total, grown = npix, 0, []
    for v, n in enumerate(ref.per_view):
        if total + n > capacity:
            grown.append(v)
            while capacity < total + n:
                capacity *= 2
        total += n
    assert grown == [2, 4, 8]
    g = ref.points["red"].reshape(5, npix)  # the pairs' grays differ: a block in the wrong place cannot compare equal
    assert all(not np.array_equal(g[a], g[b]) for a in range(5) for b in range(a))
    assert [ref.used[v].all() for v in range(10)] == [False, True] * 5


# -- views that emit nothing -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _silent_case(which):
    """three views of the plane Z = 500 through one camera.  "normal": normal_thresh = 0, cos_t = 1.0 and no n . n' > 1;
    "count": num_consistent = 3 with two partners"""
    P = _pinhole(100.0, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0))
    n4s = _plane_views([P] * 3, [500.0] * 3, 30, 40)
    grays = [np.full((30, 40), 10.0 * v, dtype=f32) for v in range(3)]
    return _case(n4s, grays, [P] * 3, 1.0, 0.1, 0.0 if which == "normal" else 30.0, 1 if which == "normal" else 3)


def _silent_condition(which, ref):
    assert ref.per_view == [0, 0, 0] and len(ref.points) == 0 and not ref.used.any() and not ref.emitted.any()
    if which == "normal":
        assert fusion.cos_threshold(0.0) == f32(1.0) and ref.tally["normal"] == 3 * 2 * 1200 and ref.tally["too_few"] == 3 * 1200
    else:
        assert ref.tally["normal"] == 0 and ref.tally["too_few"] == 3 * 1200


# -- many views --------------------------------------------------------------------------------------------------------
MANY = {100: (24, 18), 512: (13, 9)}  # views: (cols, rows)


@functools.lru_cache(maxsize=None)
def _many_case(V):
    """V pinhole cameras (f = 100) translated along x in steps of 0.02, all seeing the plane Z = 500: 0.004 pixels of
    disparity per step.  With 100 views every partner pixel is the pixel itself; with 512 the partner is up to two
    columns away, and the columns that no earlier view reaches are emitted by later views."""
    cols, rows = MANY[V]
    Ps = [_pinhole(100.0, cols / 2.0, rows / 2.0, np.eye(3), (0.02 * k, 0.0, 0.0)) for k in range(V)]
    n4s = _plane_views(Ps, [500.0] * V, rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols]
    grays = [((xx * 7 + yy * 13 + v * 3) % 256).astype(f32) for v in range(V)]
    return _case(n4s, grays, Ps, 1.0, 0.05, 30.0, 3)


def _many_condition(V, ref):
    cols, rows = MANY[V]
    assert len(ref.per_view) == V
    if V == 100:
        assert ref.per_view == [cols * rows] + [0] * 99
    else:
        assert V == abi.FUSION_MAX_VIEWS
        assert sum(ref.per_view) == 153 and ref.per_view[0] == cols * rows and max(np.nonzero(ref.per_view)[0]) >= 256
    assert all(u.any() for u in ref.used[1:])  # view 0 marked a pixel in every other view: all V - 1 passed the tests


@functools.lru_cache(maxsize=None)
def _dtu40_case():
    """40 views of DTU geometry (beyond the solver's 32): _dtu_views repeats cameras when asked for more than the scan's
    selection holds, each repeat with damage of its own"""
    return _scan_case(40, 80, 60, 61, 3)


def _dtu40_condition(ref):
    assert len(ref.per_view) == 40 > abi.MAX_VIEWS and sum(1 for n in ref.per_view if n) >= 8
    assert all(ref.tally[r] > 0 for r in fusion_ref.REASONS if r != "behind"), ref.tally


# -- CPU: each scene reaches what it is there for ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_scenes_emit_in_their_last_workgroup(name):
    _ragged_condition(name, _ragged_case(name).ref)


@pytest.mark.parametrize("name", sorted(CHUNKED))
def test_chunked_scenes_emit_in_every_chunk_of_the_scan(name):
    _chunked_condition(name, _chunked_case(name).ref)


@pytest.mark.parametrize("cols,rows", [(67, 45)])
def test_pairs_scene_outgrows_the_point_buffer_three_times(cols, rows):
    _pairs_condition(cols, rows, _pairs_case(cols, rows).ref)


@pytest.mark.parametrize("which", ["normal", "count"])
def test_silent_scenes_emit_nothing(which):
    _silent_condition(which, _silent_case(which).ref)


@pytest.mark.parametrize("V", sorted(MANY))
def test_many_view_scenes_reach_every_view(V):
    _many_condition(V, _many_case(V).ref)


def test_forty_dtu_views_scene_reaches_the_contract_s_branches():
    _dtu40_condition(_dtu40_case().ref)


def test_the_restatement_s_emitted_mask_counts_the_points_in_scan_order():
    ref = _ragged_case("67x45").ref
    assert [int(e.sum()) for e in ref.emitted] == ref.per_view
    assert ref.emitted.dtype == np.uint8 and ref.emitted.shape == ref.used.shape and set(np.unique(ref.emitted)) == {0, 1}
    # a view that finds no valid unused pixel (every second one of the pairs scene) leaves without a record or a tally
    pairs = _pairs_case(67, 45).ref
    assert [int(e.sum()) for e in pairs.emitted] == pairs.per_view and pairs.tally["used"] == 5 * 67 * 45


def test_513_views_are_refused():
    lib = abi.load_library()
    assert abi.FUSION_MAX_VIEWS == 512
    assert "#define GIPUMA_HIP_FUSION_MAX_VIEWS 512" in open(os.path.join(ROOT, "include", "gipuma_hip.h")).read()
    host = np.zeros((4, 4, 4), dtype=f32)
    views = (abi.FusionView * 513)()
    for v in views:
        v.norm4 = host.ctypes.data
    h = C.c_void_p()
    assert lib.gipuma_hip_fuse(C.byref(_desc(views, 513)), C.byref(h)) == abi.ERR_ARG and not h.value
    assert b"512" in lib.gipuma_hip_last_error()
    with pytest.raises(ValueError, match="2..512 views"):
        fusion.fuse([host] * 513, [None] * 513, [np.eye(3, 4)] * 513)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_frames_equal_the_restatement(hip, name):
    """pix < npix false in the last workgroup, a last wavefront partly outside the frame, workgroups without a pixel in
    three of their wavefronts, a frame below one wavefront, a single row"""
    c = _ragged_case(name)
    _ragged_condition(name, c.ref)
    pts, info = _fuse_case(c)
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHUNKED))
def test_scan_chunks_equal_the_restatement(hip, name):
    """1024, 1025, 1034 and 2063 workgroups: scan_kernel's carry over one, two and three chunks of 1024 counts"""
    c = _chunked_case(name)
    _chunked_condition(name, c.ref)
    pts, info = _fuse_case(c)
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(67, 45)])
def test_growing_the_point_buffer_keeps_the_earlier_views_points(hip, cols, rows):
    """five times a frame's worth of points: the buffer is grown at the third, fifth and ninth view; every second view
    emits nothing and its scatter is skipped"""
    c = _pairs_case(cols, rows)
    _pairs_condition(cols, rows, c.ref)
    pts, info = _fuse_case(c)
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, "pairs %dx%d" % (cols, rows))
    assert len(pts) == 5 * rows * cols


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["normal", "count"])
def test_views_that_emit_nothing_give_an_empty_cloud(hip, which):
    c = _silent_case(which)
    _silent_condition(which, c.ref)
    pts, info = _fuse_case(c)
    assert len(pts) == 0 and pts.dtype == dmb._PLY_VERTEX and info["per_view"] == [0, 0, 0] and not info["used"].any()
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, which)


@pytest.mark.gpu
@pytest.mark.parametrize("V", sorted(MANY))
def test_many_views_equal_the_restatement(hip, V):
    """100 and 512 (the header's limit) views: the view table beyond a handful of entries, used planes up to
    511 * npix + pix.  The 512-view call is about 1500 launches and 512 stream waits on a 117-pixel frame; its time on
    an MI355X has not been measured yet (the restatement takes 0.6 s)"""
    c = _many_case(V)
    _many_condition(V, c.ref)
    pts, info = _fuse_case(c)
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, "%d views" % V)


@pytest.mark.gpu
def test_forty_dtu_views_equal_the_restatement(hip):
    c = _dtu40_case()
    _dtu40_condition(c.ref)
    pts, info = _fuse_case(c)
    _assert_equals_ref(pts, info["per_view"], info["used"], c.ref, "40 DTU views")


@contextlib.contextmanager
def _fused(lib, c, stream=None, planes=None):
    """gipuma_hip_fuse through the C-ABI, the descriptor built as fusion.fuse builds it, the handle kept: yields
    (handle, number of points).  stream: a torch stream whose handle goes into desc.stream -- then `planes` (norm4, gray
    device tensors written on that stream) are passed as they are and nothing is synchronised before the call."""
    dev, keep = torch.device("cuda", 0), []
    V = len(c.norm4s)
    n4s, grays = planes if planes is not None else (c.norm4s, c.grays)
    views = (abi.FusionView * V)()
    for v in range(V):
        abi.fill_view(views[v], fusion.view_constants(c.Ps[v], c.cam_scale), abi.device_plane(n4s[v], dev, keep),
                      abi.device_plane(grays[v], dev, keep) if grays[v] is not None else None)
    d = abi.FusionDesc()
    d.abi_version = abi.ABI_VERSION
    d.rows, d.cols, d.n_views = c.norm4s[0].shape[0], c.norm4s[0].shape[1], V
    d.views = C.cast(views, C.POINTER(abi.FusionView))
    d.disp_thresh, d.normal_thresh, d.num_consistent = c.disp, c.normal_thresh, c.num_consistent
    d.depth_min, d.depth_max, d.device_id = 300.0, 800.0, 0
    if stream is None:
        torch.cuda.synchronize(dev)
    else:
        assert stream.cuda_stream
        d.stream = stream.cuda_stream
    h = C.c_void_p()
    abi.check(lib, lib.gipuma_hip_fuse(C.byref(d), C.byref(h)), "gipuma_hip_fuse")
    try:
        n = C.c_int64()
        abi.check(lib, lib.gipuma_hip_fusion_count(h, C.byref(n), None, None), "gipuma_hip_fusion_count")
        yield h, n.value
    finally:
        lib.gipuma_hip_fusion_free(h)


def _read(lib, h, first, count):
    out = np.zeros(count, dtype=dmb._PLY_VERTEX)
    abi.check(lib, lib.gipuma_hip_fusion_points(h, out.ctypes.data, first, count), "gipuma_hip_fusion_points")
    return out


def _results(lib, h, n, V, rows, cols):
    per_view, used = (C.c_int64 * V)(), np.empty((V, rows, cols), dtype=np.uint8)
    abi.check(lib, lib.gipuma_hip_fusion_count(h, None, per_view, None), "gipuma_hip_fusion_count")
    abi.check(lib, lib.gipuma_hip_fusion_used(h, used.ctypes.data), "gipuma_hip_fusion_used")
    return _read(lib, h, 0, n), list(per_view), used


@pytest.mark.gpu
def test_point_ranges_read_the_same_records_and_check_their_bounds(hip):
    lib = hip
    c = _ragged_case("67x45")
    with _fused(lib, c) as (h, n):
        whole = _read(lib, h, 0, n)
        assert n == len(c.ref.points) > 100 and whole.tobytes() == c.ref.points.tobytes()
        a, b = n // 7, n // 7 + (2 * n) // 3  # three uneven pieces
        pieces = [_read(lib, h, 0, a), _read(lib, h, a, b - a), _read(lib, h, b, n - b)]
        assert 0 < a < b < n and len({len(p) for p in pieces}) == 3
        assert np.concatenate(pieces).tobytes() == whole.tobytes()
        for k in (0, 1, 2, n - 3, n - 2, n - 1):  # record by record at both ends
            assert _read(lib, h, k, 1).tobytes() == whole[k:k + 1].tobytes(), k
        points = lib.gipuma_hip_fusion_points
        for first in (0, 1, n - 1, n):  # nothing to read: no destination needed, the end itself is a valid start
            assert points(h, None, first, 0) == 0
        assert points(h, None, 0, 1) == abi.ERR_ARG
        spare = np.zeros(4, dtype=dmb._PLY_VERTEX)
        int64_max = (1 << 63) - 1
        for first, count in ((-1, 1), (-1, 0), (0, -1), (n - 1, 2), (n, 1), (0, n + 1), (n + 1, 0), (int64_max, 1),
                             (int64_max, 0), (1, int64_max)):
            assert points(h, spare.ctypes.data, first, count) == abi.ERR_ARG, (first, count)
            assert b"out of bounds" in lib.gipuma_hip_last_error()
        assert not spare.tobytes().strip(b"\0")  # ... and nothing was written
        assert points(None, spare.ctypes.data, 0, 1) == abi.ERR_ARG
        assert lib.gipuma_hip_fusion_count(h, None, None, None) == 0
        assert lib.gipuma_hip_fusion_count(None, None, None, None) == abi.ERR_ARG
    with _fused(lib, _silent_case("normal")) as (h, n):  # an empty cloud: the only valid range is (0, 0)
        assert n == 0 and lib.gipuma_hip_fusion_points(h, None, 0, 0) == 0
        assert lib.gipuma_hip_fusion_points(h, spare.ctypes.data, 0, 1) == abi.ERR_ARG
        assert lib.gipuma_hip_fusion_points(h, None, 1, 0) == abi.ERR_ARG


@pytest.mark.gpu
def test_fusion_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the planes were written just before, the device not synchronised: the library
    runs behind them on that stream.  Two frame sizes one after the other on the same stream; each equals the restatement
    and the call on a stream of the library's own"""
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("161x113", "67x45"):
        c = _ragged_case(name)
        V, (rows, cols) = len(c.norm4s), c.norm4s[0].shape[:2]
        staged = [torch.from_numpy(n).cuda() for n in c.norm4s], [torch.from_numpy(g).cuda() for g in c.grays]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the planes the library reads: device copies queued on the caller's stream
            planes = [t.clone() for t in staged[0]], [t.clone() for t in staged[1]]
        with _fused(lib, c, stream, planes) as (h, n):
            on_stream = _results(lib, h, n, V, rows, cols)
        with _fused(lib, c) as (h, n):
            default = _results(lib, h, n, V, rows, cols)
        _assert_equals_ref(*on_stream, c.ref, "%s on the caller's stream" % name)
        _assert_equals_ref(*default, c.ref, "%s on the library's stream" % name)
        assert on_stream[0].tobytes() == default[0].tobytes()
