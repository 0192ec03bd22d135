"""Depth-map fusion (gipuma_amd.fusion).  CPU: known answers of the restatement (tests/fusion_ref.py), the
camera constants, the PLY writer, the CLI's folders and the C-ABI's argument checks.  GPU: the kernels equal the
restatement in every bit, are deterministic, put fused points on the surface, and the batch runner's --fuse equals the
CLI on the dumps."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gipuma_amd import abi, cameras, dmb, fusion, synth
from tests import fusion_ref

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
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "gipuma_hip.h"),
             'int main(void){']
    for s, (_, fs) in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fs:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append('return 0;}')
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "l.c")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", os.path.join(td, "l"), src])
        got = dict(l.split() for l in subprocess.check_output([os.path.join(td, "l")]).decode().split("\n") if l)
    for s, (py, fs) in fields.items():
        assert int(got[s]) == C.sizeof(py) and [f for f, _ in py._fields_] == fs
        for f in fs:
            assert int(got["%s.%s" % (s, f)]) == getattr(py, f).offset, (s, f)


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
