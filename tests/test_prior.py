"""The cross-view prior (gipuma_amd.prior): the solved maps of neighbouring views carried into a new
reference camera.  CPU: known answers of the restatement (tests/prior_ref.py), the C-ABI's argument checks and struct
layout, the kernels' instructions, the batch runner's argument handling and processing order.  GPU: the kernels equal the
restatement in every bit and are deterministic; a session seeded from the prior equals restated prior + restated seed +
oracle; a view solved from its neighbours reaches the quality of the plain solve; batch --view_prior."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from gipuma_amd import abi, batch, cameras, dmb, fusion, prior, synth
from gipuma_amd.problem import GlobalState, Session, runcuda
from tests import prior_ref, pyramid_ref
from tests.abi_layout import assert_mirrors_header
from tests.oracle_lib import OracleState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(a, b, what):
    a, b = bits(a), bits(b)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r"
                             % (what, len(bad), a.size, tuple(bad[0]), a.view(np.float32)[tuple(bad[0])],
                                b.view(np.float32)[tuple(bad[0])]))


def _pinhole(f, cx, cy, R, Cc):
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return K @ np.concatenate([R, (-R @ np.asarray(Cc, dtype=np.float64))[:, None]], axis=1)


def _plane(rows, cols, z, normal=(0.0, 0.0, -1.0)):
    n4 = np.empty((rows, cols, 4), dtype=f32)
    n4[..., :3] = normal
    n4[..., 3] = z
    return n4


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's known answers
# ----------------------------------------------------------------------------------------------------------------------
def test_a_source_with_the_target_s_own_camera_returns_the_source_map():
    """same pixel, same normal bits, depth within 4 ulp on every valid pixel; invalid pixels stay empty without fill"""
    rows, cols = 30, 40
    k = fusion.view_constants(_pinhole(100.0, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0)))
    rng = np.random.default_rng(3)
    n4 = _plane(rows, cols, 0.0)
    n4[..., 3] = rng.uniform(300.0, 700.0, (rows, cols))
    n4[..., :2] = rng.uniform(-0.3, 0.3, (rows, cols, 2))  # tilted, still facing the camera
    hole = rng.random((rows, cols)) < 0.1
    n4[hole, 3] = 0.0
    r = prior_ref.prior_from_views(k, [n4], [k], fill=False)
    valid = ~hole
    assert r.counts == [int(valid.sum()), 0, int(hole.sum())]
    assert np.array_equal(r.info["cls"] == 0, valid) and (r.info["source"][valid] == 0).all()
    yy, xx = np.mgrid[0:rows, 0:cols]
    assert np.array_equal((r.zbuf[valid] & np.uint64(0xFFFFFFFF)).astype(np.int64), (yy * cols + xx)[valid])  # same pixel
    assert np.array_equal(bits(r.prior[valid][:, :3]), bits(n4[valid][:, :3]))
    assert _ulps(r.prior[valid][:, 3], n4[valid][:, 3]).max() <= 4
    assert not r.prior[hole].any() and not r.info["grazing"].any()


def test_a_fronto_parallel_plane_from_a_translated_camera_has_the_analytic_depth():
    """the plane Z = 500 seen from a camera moved 40 along the axis and 3 sideways: depth 460 on every covered pixel, the
    normal's bits kept; the plane intersection removes the rounding to the pixel centre (<= 2e-6 relative, fp32)"""
    rows, cols = 30, 40
    src = fusion.view_constants(_pinhole(100.0, 20.0, 15.0, np.eye(3), (0.0, 0.0, 0.0)))
    tgt = fusion.view_constants(_pinhole(100.0, 20.0, 15.0, np.eye(3), (3.0, 0.0, 40.0)))
    r = prior_ref.prior_from_views(tgt, [_plane(rows, cols, 500.0)], [src], fill=True)
    got = r.info["cls"] != 2
    assert got.mean() > 0.8 and r.counts[0] > 0
    assert np.abs(r.prior[got][:, 3] / f32(460.0) - 1).max() <= 2e-6
    assert (r.prior[got][:, :3] == np.array([0.0, 0.0, -1.0], dtype=f32)).all()
    # a tilted plane: n . X = -d through (0, 0, 500); the target ray of pixel (x, y) meets it at the closed-form depth
    n = np.array([0.2, -0.1, -1.0])
    z_src = np.empty((rows, cols))
    yy, xx = np.mgrid[0:rows, 0:cols]
    ray = np.stack([(xx - 20.0) / 100.0, (yy - 15.0) / 100.0, np.ones_like(xx, dtype=np.float64)], -1)
    z_src = (n @ np.array([0.0, 0.0, 500.0])) / (ray @ n)
    n4 = _plane(rows, cols, 0.0, n)
    n4[..., 3] = z_src
    r = prior_ref.prior_from_views(tgt, [n4], [src], fill=False)
    want = (n @ (np.array([0.0, 0.0, 500.0]) - np.array([3.0, 0.0, 40.0]))) / (ray @ n)
    got = r.info["cls"] == 0
    assert got.mean() > 0.8
    assert np.abs(r.prior[got][:, 3] / want[got] - 1).max() <= 1e-5


def test_the_nearer_of_two_surfaces_wins_and_a_duplicated_source_resolves_to_ordinal_zero():
    rows, cols = 12, 16
    k = fusion.view_constants(_pinhole(100.0, 8.0, 6.0, np.eye(3), (0.0, 0.0, 0.0)))
    far, near = _plane(rows, cols, 500.0), _plane(rows, cols, 400.0)
    near[:, :8, 3] = 0.0  # the near surface covers the right half only
    r = prior_ref.prior_from_views(k, [far, near], [k, k], fill=False)
    assert (r.info["source"][:, 8:] == 1).all() and (r.info["source"][:, :8] == 0).all()
    assert (r.prior[:, 8:, 3] == 400.0).all() and (r.prior[:, :8, 3] == 500.0).all()
    r = prior_ref.prior_from_views(k, [far, far.copy()], [k, k], fill=False)
    assert (r.info["source"] == 0).all() and r.counts == [rows * cols, 0, 0]


def test_a_one_pixel_crack_is_filled_with_fill_and_empty_without():
    rows, cols = 12, 16
    k = fusion.view_constants(_pinhole(100.0, 8.0, 6.0, np.eye(3), (0.0, 0.0, 0.0)))
    n4 = _plane(rows, cols, 450.0)
    n4[5, 7, 3] = np.nan
    n4[0, 0, 3] = -1.0  # a corner: three neighbours inside the frame
    r = prior_ref.prior_from_views(k, [n4], [k], fill=True)
    assert r.counts == [rows * cols - 2, 2, 0] and r.info["cls"][5, 7] == 1 and r.info["cls"][0, 0] == 1
    assert abs(float(r.prior[5, 7, 3]) / 450.0 - 1) < 1e-6 and tuple(r.prior[5, 7, :3]) == (0.0, 0.0, -1.0)
    # the smallest key of the 8 neighbours: equal depths, source 0 -> the lowest source pixel, (4, 6)
    assert int(r.zbuf[4, 6]) == min(int(r.zbuf[y, x]) for y in (4, 5, 6) for x in (6, 7, 8) if (y, x) != (5, 7))
    r = prior_ref.prior_from_views(k, [n4], [k], fill=False)
    assert r.counts == [rows * cols - 2, 0, 2] and not r.prior[5, 7].any() and not r.prior[0, 0].any()


def test_back_facing_pixels_and_pixels_beyond_max_cost_are_dropped():
    rows, cols = 12, 16
    k = fusion.view_constants(_pinhole(100.0, 8.0, 6.0, np.eye(3), (0.0, 0.0, 0.0)))
    n4 = _plane(rows, cols, 450.0)
    n4[3, 4, :3] = (0.0, 0.0, 1.0)   # faces away
    n4[6, 9, :3] = 0.0               # no normal
    n4[7, 9, 0] = np.inf
    cost = np.full((rows, cols), 0.2, dtype=f32)
    cost[8, 2] = 0.9
    cost[9, 2] = np.nan
    cost[10, 2] = 0.5                # the bound itself passes
    r = prior_ref.prior_from_views(k, [n4], [k], costs=[cost], max_cost=0.5, fill=False)
    assert r.tally["back_facing"] == 1 and r.tally["bad_normal"] == 2 and r.tally["cost"] == 2
    for y, x in ((3, 4), (6, 9), (7, 9), (8, 2), (9, 2)):
        assert r.info["cls"][y, x] == 2 and not r.prior[y, x].any()
    assert r.info["cls"][10, 2] == 0 and r.counts == [rows * cols - 5, 0, 5]
    # depth bounds apply to the source depth and to the depth in the target
    r = prior_ref.prior_from_views(k, [n4], [k], depth_min=460.0, fill=False)
    assert r.counts[0] == 0 and r.tally["invalid_depth"] == rows * cols


# ----------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI, instructions, batch arguments
# ----------------------------------------------------------------------------------------------------------------------
def _desc(views, n, **kw):
    d = abi.PriorDesc()
    d.abi_version, d.rows, d.cols, d.n_sources = abi.ABI_VERSION, 4, 4, n
    d.sources = C.cast(views, C.POINTER(abi.FusionView))
    d.grazing_cos, d.fill = prior.grazing_cos(), 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_prior_from_views_validates_its_arguments_and_needs_a_device():
    lib = abi.load_library()
    host = np.zeros((4, 4, 4), dtype=f32)
    out = np.zeros((4, 4, 4), dtype=f32)
    views = (abi.FusionView * 32)()
    for v in views:
        v.norm4 = host.ctypes.data
    call = lambda d, o=out.ctypes.data: lib.gipuma_hip_prior_from_views(C.byref(d), o, None, None)  # noqa: E731
    for kw in (dict(n_sources=0), dict(n_sources=33), dict(abi_version=2), dict(rows=0), dict(cols=-1), dict(fill=2),
               dict(grazing_cos=1.5), dict(grazing_cos=float("nan")), dict(rows=1 << 16, cols=1 << 15)):
        assert call(_desc(views, 3, **kw)) == abi.ERR_ARG, kw
    assert call(_desc(views, 3), None) == abi.ERR_ARG
    assert call(_desc(None, 3)) == abi.ERR_ARG
    assert lib.gipuma_hip_prior_from_views(None, out.ctypes.data, None, None) == abi.ERR_ARG
    costs = (C.c_void_p * 3)(host.ctypes.data, None, host.ctypes.data)
    assert call(_desc(views, 3, costs=C.cast(costs, C.POINTER(C.c_void_p)), max_cost=0.5)) == abi.ERR_ARG
    assert b"cost" in lib.gipuma_hip_last_error()
    views[1].norm4 = None
    assert call(_desc(views, 3)) == abi.ERR_ARG and b"norm4" in lib.gipuma_hip_last_error()
    views[1].norm4 = host.ctypes.data
    # the key's low word: S rows cols must stay below 2^32
    assert call(_desc(views, 4, rows=1 << 15, cols=1 << 15)) == abi.ERR_UNSUPPORTED
    assert call(_desc(views, 32, rows=1 << 14, cols=1 << 13)) == abi.ERR_UNSUPPORTED
    if lib.gipuma_hip_device_count() == 0:
        assert call(_desc(views, 3)) == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        assert call(_desc(views, 3, rows=1 << 15, cols=1 << 15)) == abi.ERR_NO_DEVICE  # 3 x 2^30 < 2^32
        with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
            prior.prior_from_views(np.eye(3, 4), [host], [np.eye(3, 4)])
    with pytest.raises(ValueError, match="same size"):
        prior.prior_from_views(np.eye(3, 4), [host, host[:3]], [np.eye(3, 4)] * 2)
    with pytest.raises(ValueError, match="go together"):
        prior.prior_from_views(np.eye(3, 4), [host], [np.eye(3, 4)], costs=[host[..., 0]])


def test_prior_struct_matches_the_header_layout():
    fs = ["abi_version", "rows", "cols", "target", "n_sources", "sources", "costs", "max_cost", "depth_min", "depth_max",
          "grazing_cos", "fill", "device_id", "stream"]
    assert_mirrors_header(abi.PriorDesc, "gipuma_hip_prior_desc", fs)


def test_prior_kernels_use_global_memory_instructions_one_64_bit_minimum_and_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "p.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--offload-device-only", "-o", out, "gipuma_prior.hip"],
                              cwd=os.path.join(ROOT, "gipuma_amd", "csrc"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    for k in ("splat_kernel", "resolve_kernel"):
        assert "_ZN5prior%d%s" % (len(k), k) in asm
    ops = [l.split()[0] for l in asm.splitlines() if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")]
    assert ops.count("global_atomic_umin_x2") == 1 and "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert [o for o in ops if o.startswith("s_load_")]  # the view constants of the splat: scalar loads
    sizes = [l.split()[-1] for l in asm.splitlines() if ".amdhsa_private_segment_fixed_size" in l]
    assert sizes == ["0", "0"]
    assert "spill_count: 0" in asm and not [l for l in asm.splitlines() if "spill_count:" in l and not l.strip().endswith(" 0")]


def test_batch_refuses_view_prior_with_levels():
    base = ["--images-folder", "nowhere", "--p-folder", "nowhere", "--output-folder", "nowhere"]
    with pytest.raises(SystemExit, match="--view_prior cannot be combined with --levels"):
        batch.main(base + ["--view_prior", "4", "--levels", "2"])
    with pytest.raises(SystemExit, match="--view_prior must be"):
        batch.main(base + ["--view_prior", "33"])
    with pytest.raises(SystemExit, match="below --prior_min_views"):
        batch.main(base + ["--view_prior", "1"])


def test_build_scan_s_first_view_is_build_problem_s():
    """the scan helper renders what build_problem renders: same images, ground truth, cameras, parameters and selection"""
    for scene in ("smooth", "steps", "patchy"):
        cfg = synth.tiny_config(cols=64, rows=48, n_src=3)
        scan = synth.build_scan(cfg, scene=scene)
        gs, info = synth.build_problem(cfg, scene=scene)
        g0 = scan.problem(0)
        assert len(scan.images) == len(gs.images) and all(np.array_equal(a, b) for a, b in zip(scan.images, gs.images))
        assert np.array_equal(scan.gt_depth[0], info["gt_depth"]) and scan.view_ids == info["view_ids"]
        assert bytes(g0.desc.params) == bytes(gs.desc.params) and bytes(g0.cameras.c_array) == bytes(gs.cameras.c_array)
        assert g0.selected == gs.selected and g0.desc.seed == gs.desc.seed
        # the ground-truth normals have unit length
        n = scan.gt_norm4[1][..., :3].astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-6


def test_greedy_order_on_a_hand_made_selection_graph():
    """a: (b, c)  b: (a, c)  c: (d, e)  d: (c, e)  e: (a, b, d)  f: ()
    start a (all zero, scan order); then b (1 solved: a) before c (0); then e has (a, b) = 2, c has 0 -> e; then
    d (e) = 1 ties with c (0)? no: c (d, e) = 1, d (c, e) = 1 -> scan order: c; then d; f last (never any)"""
    sel = dict(a=["b", "c"], b=["a", "c"], c=["d", "e"], d=["c", "e"], e=["a", "b", "d"], f=[])
    assert prior.greedy_order(list("abcdef"), sel) == ["a", "b", "e", "c", "d", "f"]
    assert prior.greedy_order(list("fedcba"), sel) == ["f", "e", "d", "c", "b", "a"]
    assert prior.greedy_order([], {}) == [] and prior.greedy_order(["x"], dict(x=["y"])) == ["x"]
    chain = {str(i): [str(i - 1), str(i + 1)] for i in range(6)}
    assert prior.greedy_order([str(i) for i in range(6)], chain) == ["0", "1", "2", "3", "4", "5"]


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=4)
def _scan(cols, rows, n_src, scene="smooth", blocksize=11, cfg="tiny"):
    if cfg == "tiny":
        return synth.build_scan(synth.tiny_config(cols=cols, rows=rows, n_src=n_src, blocksize=blocksize, iterations=8, n_best=3),
                                scene=scene)
    return synth.build_scan(cfg, cols=cols, rows=rows, n_src=n_src, blocksize=blocksize, n_best=3, scene=scene)


def _perturbed_sources(scan, S, seed):
    """S source maps for target view 0: the ground truth of views 1.. (cycled: duplicates give exact ties), damaged so that
    every branch of the contract is reached, plus -- as the last source when S >= 3 -- a camera behind the surface looking
    back (its surface faces away from the target; its depth-795 pixels lie behind the target camera).  Returns
    (norm4s, Ps, costs)."""
    rng = np.random.default_rng(seed)
    n_real = len(scan.images) - 1
    rows, cols = scan.gt_depth[0].shape
    norm4s, Ps, costs = [], [], []
    for k in range(S):
        j = 1 + k % n_real
        n4 = scan.gt_norm4[j].copy()
        if k < n_real:  # (a second pass over the views repeats the maps bit for bit: ties)
            r = rng.random((rows, cols))
            z = n4[..., 3]
            z[r < 0.03] = 0.0
            z[(r >= 0.03) & (r < 0.04)] = np.nan
            z[(r >= 0.04) & (r < 0.045)] = np.inf
            z[(r >= 0.045) & (r < 0.05)] = 900.0
            z[(r >= 0.05) & (r < 0.055)] = 200.0
            near = (r >= 0.055) & (r < 0.09)                       # occluders: nearer than the surface
            z[near] *= rng.uniform(0.6, 0.9, near.sum()).astype(f32)
            n4[(r >= 0.09) & (r < 0.10), :3] *= f32(-1.0)          # back-facing
            n4[(r >= 0.10) & (r < 0.105), :3] = 0.0
            n4[(r >= 0.105) & (r < 0.11), 1] = np.nan
            g = (r >= 0.11) & (r < 0.16)                           # normals at a grazing angle to the rays
            v = rng.normal(size=(int(g.sum()), 3))
            n4[g, :3] = (n4[g, :3] * 0.05 + v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)
            z[(r >= 0.16) & (r < 0.20)] *= f32(1.3)                # behind the surface: lose against it
            hole = slice(rows // 3, rows // 3 + 6), slice(cols // 4, cols // 4 + 9)
            z[hole] = 0.0                                          # a hole no neighbour fills
        norm4s.append(n4)
        Ps.append(scan.P_matrices[j])
        # (a map repeated bit for bit carries its first copy's costs too, or the cost filter would break the tie)
        costs.append(costs[k - n_real] if k >= 2 * n_real else rng.uniform(0.0, 1.0, (rows, cols)).astype(f32))
    if S >= 3:
        K0, R0, C0 = cameras.decompose_projection(scan.P_matrices[0])
        Rf = np.diag([1.0, -1.0, -1.0]) @ R0
        Ps[-1] = K0 @ np.concatenate([Rf, (-Rf @ (C0 + R0.T @ np.array([0.0, 0.0, 760.0])))[:, None]], axis=1)
        n4 = scan.gt_norm4[0].copy()
        n4[..., :3] *= f32(-1.0)
        n4[..., 3] = (f32(760.0) - scan.gt_depth[0])[:, ::-1]
        n4[rng.random((rows, cols)) < 0.1, 3] = 795.0
        norm4s[-1] = n4
    return norm4s, Ps, costs


PRIOR_CASES = [  # (cols, rows, views of the scan, S, grazing degrees, fill, costs)
    ("161x113-S4", 161, 113, 4, 4, 80.0, True, True),
    ("161x113-S4-nofill-noguard", 161, 113, 4, 4, 90.0, False, False),
    ("161x113-S4-guard-always", 161, 113, 4, 4, 0.0, True, False),
    ("320x240-S1", 320, 240, 4, 1, 80.0, True, False),
    ("96x64-S32", 96, 64, 4, 32, 80.0, True, True),
    ("1600x1200-S4", 1600, 1200, 3, 4, 80.0, True, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,cols,rows,n_src,S,grazing,fill,with_cost", PRIOR_CASES, ids=[c[0] for c in PRIOR_CASES])
def test_prior_equals_the_restatement_bit_for_bit(hip, name, cols, rows, n_src, S, grazing, fill, with_cost):
    """every bit of the prior plane and the three counts; host arrays and device tensors; three runs byte-identical"""
    torch = _torch()
    scan = _scan(cols, rows, n_src)
    n4s, Ps, costs = _perturbed_sources(scan, S, seed=cols + S)
    kw = dict(depth_min=300.0, depth_max=800.0, fill=fill)
    ck = dict(costs=costs, max_cost=0.9) if with_cost else {}
    ref = prior_ref.prior_from_views(fusion.view_constants(scan.P_matrices[0], scan.cam_scale), n4s,
                                     [fusion.view_constants(P, scan.cam_scale) for P in Ps],
                                     grazing=prior.grazing_cos(grazing), **kw, **ck)
    got, info = prior.prior_from_views(scan.P_matrices[0], n4s, Ps, scan.cam_scale, grazing_deg=grazing, return_info=True,
                                       **kw, **ck)
    print("%s: counts %r, tally %r, %.3f ms" % (name, ref.counts, ref.tally, info["device_ms"]))
    assert [info["direct"], info["filled"], info["empty"]] == ref.counts and sum(ref.counts) == rows * cols
    assert_same(got.cpu().numpy(), ref.prior, name)
    assert info["device_ms"] > 0
    dev = [torch.from_numpy(n).cuda() for n in n4s]
    dck = dict(costs=[torch.from_numpy(c).cuda() for c in costs], max_cost=0.9) if with_cost else {}
    out = torch.full((rows, cols, 4), -5.0, dtype=torch.float32, device="cuda:0")
    runs = []
    for _ in range(3):
        back = prior.prior_from_views(scan.P_matrices[0], dev, Ps, scan.cam_scale, grazing_deg=grazing, out=out, **kw, **dck)
        assert back is out
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy().tobytes())
        out.fill_(-5.0)
    assert runs[0] == runs[1] == runs[2] == ref.prior.tobytes()
    # the case reaches what it is there for
    if S >= 3:
        want = set(prior_ref.REASONS) - (set() if with_cost else {"cost"})
        assert all(ref.tally[r] > 0 for r in want), ref.tally
        assert ref.counts[0] > 0 and ref.counts[2] > 0 and (ref.counts[1] > 0 if fill and grazing else ref.counts[1] == 0)
        assert len(np.unique(ref.info["source"][ref.info["cls"] != 2])) >= 3
    if grazing == 80.0:
        assert ref.info["grazing"].any() and not ref.info["grazing"][ref.info["cls"] != 2].all()
    if grazing == 0.0:  # cos 0 = 1: no intersection passes, every direct pixel keeps its splatted depth
        assert ref.info["grazing"][ref.info["cls"] != 2].all() and ref.counts[1] == 0
    if S == 32:  # the second and later passes over the views repeat maps bit for bit: the lower ordinal wins the ties
        assert (ref.info["source"] >= 4).any() and not ((ref.info["source"] >= 8) & (ref.info["source"] < 31)).any()


# ----------------------------------------------------------------------------------------------------------------------
# GPU: a caller's stream (desc.stream was NULL in every call above: torch's default stream has the handle 0)
# ----------------------------------------------------------------------------------------------------------------------
STREAM_FRAMES = [(96, 64), (161, 113)]  # (cols, rows) of the two calls queued back to back: the second is the larger


@functools.lru_cache(maxsize=None)
def _stream_case(cols, rows):
    """4 perturbed sources of the scan at this size and the restated prior (default knobs, depth 300..800)"""
    scan = _scan(cols, rows, 4)
    n4s, Ps, _ = _perturbed_sources(scan, 4, seed=cols + 4)
    ref = prior_ref.prior_from_views(fusion.view_constants(scan.P_matrices[0], scan.cam_scale), n4s,
                                     [fusion.view_constants(P, scan.cam_scale) for P in Ps], 300.0, 800.0)
    return scan, n4s, Ps, ref


def _stream_condition(ref, rows, cols):
    """direct, filled and empty pixels, several sources among the winners, both outcomes of the grazing guard"""
    assert sum(ref.counts) == rows * cols and all(n > 0 for n in ref.counts), ref.counts
    assert len(np.unique(ref.info["source"][ref.info["cls"] != 2])) >= 3
    assert ref.info["grazing"].any() and not ref.info["grazing"][ref.info["cls"] != 2].all()


def test_the_stream_cases_reach_every_class_and_the_second_frame_is_the_larger():
    (c0, r0), (c1, r1) = STREAM_FRAMES
    assert c0 * r0 < c1 * r1 and (c1 * r1) % 256 == 17  # grows the key plane; a ragged last workgroup
    for cols, rows in STREAM_FRAMES:
        _stream_condition(_stream_case(cols, rows)[3], rows, cols)


# The child of test_prior_enqueued_twice_on_a_caller_s_stream: a fresh process, so the device's cached key plane starts
# empty whatever ran before, and the second call must replace it.  argv: the .npz of the inputs, the .npz to write.
_STREAM_CHILD = r"""
import sys
import numpy as np
import torch
from gipuma_amd import abi, prior, pyramid
src, dst = sys.argv[1:3]
data = np.load(src)
assert abi.load_library().gipuma_hip_device_count() >= 1
stream = torch.cuda.Stream()
assert stream.cuda_stream != 0
staged = [[torch.from_numpy(data["n4_%d_%d" % (c, k)]).cuda() for k in range(4)] for c in (0, 1)]
busy = torch.zeros(1 << 26, dtype=torch.float32, device="cuda:0")
pyramid.downsample(torch.zeros(4, 4, device="cuda:0"))  # the library's kernels are loaded; the prior's scratch is untouched
torch.cuda.synchronize()
outs, queued = [], []
with torch.cuda.stream(stream):
    for _ in range(400):  # device work ahead of the calls: the first has not run when the second is made
        busy.add_(1.0)
    for c in (0, 1):
        planes = [t.clone() for t in staged[c]]  # the sources: written on this stream, after the work above
        outs.append(prior.prior_from_views(data["P_target_%d" % c], planes, list(data["Ps_%d" % c]), float(data["cam_scale_%d" % c]),
                                           300.0, 800.0))
        queued.append(not stream.query())
    stream.synchronize()
np.savez(dst, queued=queued, busy=float(busy[0].item()), out_0=outs[0].cpu().numpy(), out_1=outs[1].cpu().numpy())
"""


@pytest.mark.gpu
def test_prior_enqueued_twice_on_a_caller_s_stream(hip, tmp_path):
    """without counts or time the call only enqueues: two calls back to back on one non-default stream, 96x64 then 161x113
    -- the second replaces the cached key plane while the first is still queued -- synchronised once after both; both
    priors equal the restatement in every bit.  In a child process: the cache of this one only grows, and an earlier
    test's 1600x1200 frame would keep the second call from growing it"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays, refs = {}, []
    for c, (cols, rows) in enumerate(STREAM_FRAMES):
        scan, n4s, Ps, ref = _stream_case(cols, rows)
        _stream_condition(ref, rows, cols)
        refs.append(ref)
        arrays.update({"n4_%d_%d" % (c, k): n4s[k] for k in range(4)})
        arrays.update({"P_target_%d" % c: np.asarray(scan.P_matrices[0]), "Ps_%d" % c: np.stack([np.asarray(P) for P in Ps]),
                       "cam_scale_%d" % c: np.float64(scan.cam_scale)})
    np.savez(src, **arrays)
    subprocess.run([sys.executable, "-c", _STREAM_CHILD, src, dst], cwd=ROOT, check=True, timeout=300)
    got = np.load(dst)
    assert got["busy"] == 400.0
    # the first call returned with the stream still busy: it enqueued and did not synchronise.  (Nothing of the kind holds
    # after the second: releasing the smaller key plane waits for the device.)
    assert bool(got["queued"][0])
    for c, (cols, rows) in enumerate(STREAM_FRAMES):
        assert_same(got["out_%d" % c], refs[c].prior, "call %d (%dx%d) on the caller's stream" % (c, cols, rows))


@pytest.mark.gpu
def test_prior_with_counts_on_a_caller_s_stream_has_completed(hip):
    """return_info on a non-default stream: the library synchronises that stream for the counts, so counts and plane are
    the restatement's as soon as the call returns; once more without (enqueue only), read after synchronising"""
    torch = _torch()
    cols, rows = STREAM_FRAMES[1]
    scan, n4s, Ps, ref = _stream_case(cols, rows)
    _stream_condition(ref, rows, cols)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    staged = [torch.from_numpy(n).cuda() for n in n4s]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        planes = [t.clone() for t in staged]
        got, info = prior.prior_from_views(scan.P_matrices[0], planes, Ps, scan.cam_scale, 300.0, 800.0, return_info=True)
        assert stream.query()  # nothing left in flight
        assert [info["direct"], info["filled"], info["empty"]] == ref.counts and info["device_ms"] > 0
        again = prior.prior_from_views(scan.P_matrices[0], planes, Ps, scan.cam_scale, 300.0, 800.0)
    stream.synchronize()
    assert_same(got.cpu().numpy(), ref.prior, "prior with counts on the caller's stream")
    assert_same(again.cpu().numpy(), ref.prior, "prior enqueued on the caller's stream")


# ----------------------------------------------------------------------------------------------------------------------
# GPU: a session seeded from the prior
# ----------------------------------------------------------------------------------------------------------------------
SEEDED_CASES = [
    ("box11", dict(blocksize=11), 2, None),
    ("box15", dict(blocksize=15), 2, None),
    ("box15-literal", dict(blocksize=15), 1, 7),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,over,iterations,flavour", SEEDED_CASES, ids=[c[0] for c in SEEDED_CASES])
def test_solve_seeded_from_the_prior_equals_restatement_plus_oracle(hip, name, over, iterations, flavour):
    """config C's cameras at 832x640 (the size of the pyramid's seeded cases), 4 sources: Session.solve_seeded(prior, 0) ==
    pyramid_ref.seed_planes(restated prior, shift 0) + the oracle's sweeps + finalize, every pixel, planes and costs"""
    scan = _scan(832, 640, 4, blocksize=over["blocksize"], cfg="C")
    n4s, Ps, _ = _perturbed_sources(scan, 4, seed=5)
    gs = scan.problem(0, iterations=iterations)
    dmin, dmax = float(gs.params.depthMin), float(gs.params.depthMax)
    ref = prior_ref.prior_from_views(fusion.view_constants(scan.P_matrices[0], scan.cam_scale), n4s,
                                     [fusion.view_constants(P, scan.cam_scale) for P in Ps], dmin, dmax)
    start = prior.prior_from_views(scan.P_matrices[0], n4s, Ps, scan.cam_scale, dmin, dmax)
    _torch().cuda.synchronize()
    literal = flavour == 7
    with Session(gs, literal=literal) as s:
        sched = s.schedule()
        s.solve_seeded(start, 0)
        n4, c = s.get_state()
        assert s.schedule() == sched
    r_n4, r_c, inf = pyramid_ref.solve_seeded(gs, ref.prior, 0, flavour)
    print("%s: prior counts %r, %.4f of the pixels seeded by the random fallback" % (name, ref.counts, inf["fallback"].mean()))
    assert ref.counts[2] > 0 and inf["fallback"].mean() >= ref.counts[2] / float(gs.rows * gs.cols)
    assert_same(n4, r_n4, "%s norm4" % name)
    assert_same(c, r_c, "%s cost" % name)


def _share(d, gt, tol):
    return float((np.abs(d - gt) / gt < tol).mean())


def solve_from_neighbours(scan, iterations_list, n_prior=4):
    """the four sources solved plainly (the configuration's iterations), the reference view from their prior with each of
    `iterations_list`; returns (plain depth of view 0, {iterations: seeded depth}, restated prior Result, device info)"""
    n = len(scan.images)
    solved = [runcuda(scan.problem(j))[0] for j in range(1, n)][:n_prior]
    Ps = scan.P_matrices[1:1 + n_prior]
    gs = scan.problem(0)
    dmin, dmax = float(gs.params.depthMin), float(gs.params.depthMax)
    plain, _ = runcuda(gs)
    ref = prior_ref.prior_from_views(fusion.view_constants(scan.P_matrices[0], scan.cam_scale), solved,
                                     [fusion.view_constants(P, scan.cam_scale) for P in Ps], dmin, dmax)
    start, info = prior.prior_from_views(scan.P_matrices[0], solved, Ps, scan.cam_scale, dmin, dmax, return_info=True)
    assert_same(start.cpu().numpy(), ref.prior, "prior of the solved views")
    out = {}
    for it in iterations_list:
        with Session(scan.problem(0, iterations=it)) as s:
            s.solve_seeded(start, 0)
            out[it] = s.get_state()[0][..., 3]
    return plain[..., 3], out, ref, info


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["smooth", "steps", "patchy"])
def test_a_view_solved_from_its_neighbours_reaches_the_quality_of_the_plain_solve(hip, scene):
    """DTU geometry, 320x240, box 11, 4 sources, best-3, seed 1: the four sources solved plainly (8 iterations), the reference
    view from their prior with batch's default --prior_iterations.  Share of pixels within 1e-3 / 1e-2 relative depth of
    ground truth against the plain 8-iteration solve of the same view, with the margins of
    test_two_levels_reach_the_quality_of_the_plain_solve (-0.02 at 1e-3, -0.005 at 1e-2); at most 5 % of the prior's
    pixels are empty (the restatement's own count on the solved inputs).
    Measured on an MI355X (plain | seeded with 1, 2, 3 iterations), share within 1e-3 / 1e-2:  see DESIGN.md 13."""
    scan = _scan(320, 240, 4, scene=scene)
    gt = scan.gt_depth[0]
    its = sorted({1, 2, 3, batch.PRIOR_ITERATIONS})
    plain, seeded, ref, info = solve_from_neighbours(scan, its)
    empty = ref.counts[2] / float(gt.size)
    print("%s: prior direct / filled / empty %r (empty %.4f), %.3f ms; raw prior within 1e-3: %.4f"
          % (scene, ref.counts, empty, info["device_ms"], _share(ref.prior[..., 3], gt, 1e-3)))
    print("%s: plain %.4f / %.4f" % (scene, _share(plain, gt, 1e-3), _share(plain, gt, 1e-2)))
    for it in its:
        print("%s: seeded, %d iterations %.4f / %.4f" % (scene, it, _share(seeded[it], gt, 1e-3), _share(seeded[it], gt, 1e-2)))
    assert empty <= 0.05
    got = seeded[batch.PRIOR_ITERATIONS]
    assert _share(got, gt, 1e-3) >= _share(plain, gt, 1e-3) - 0.02
    assert _share(got, gt, 1e-2) >= _share(plain, gt, 1e-2) - 0.005


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the batch runner
# ----------------------------------------------------------------------------------------------------------------------
def _write_scan(folder, scan):
    os.makedirs(os.path.join(folder, "img"))
    os.makedirs(os.path.join(folder, "p"))
    for i, im in enumerate(scan.images):
        name = "v%02d.pgm" % i
        with open(os.path.join(folder, "img", name), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.astype(np.uint8).tobytes())
        np.savetxt(os.path.join(folder, "p", name + ".P"), np.asarray(scan.P_matrices[i]), fmt="%.17g")
    return ["--images-folder", os.path.join(folder, "img"), "--p-folder", os.path.join(folder, "p"),
            "--blocksize=11", "--iterations=3", "--n_best=3", "--depth_min=300", "--depth_max=800", "--min_angle=2",
            "--max_angle=60", "--max_views=10", "--cam_scale=%r" % scan.cam_scale]


@pytest.mark.gpu
def test_batch_view_prior(hip, tmp_path):
    """a 5-view scan, every view a reference: the dumps of every view equal the composition (restated prior from the earlier
    dumps' planes + restated seed + oracle) bit for bit, the order is the greedy one, the report carries the prior's counts;
    --view_prior 0 writes what batch writes without the option, byte for byte; --view_prior 4 --fuse produces a cloud; with
    the references given in another order than the scan's, --view_prior --fuse still reports the greedy solve order under
    "order" (the fusion takes its views in the scan's order, which is not the order they were solved in)"""
    scan = _scan(160, 120, 4)
    tmp = str(tmp_path)
    args = _write_scan(tmp, scan)
    outs = {}
    for tag, extra in (("plain", []), ("off", ["--view_prior", "0"]),
                       ("prior", ["--view_prior", "4", "--prior_iterations", "2", "--prior_max_cost", "0.6", "--fuse",
                                  "--disp_thresh=%r" % (0.5 / scan.cam_scale), "--num_consistent=2"])):
        outs[tag] = os.path.join(tmp, tag)
        assert batch.main(args + ["--output-folder", outs[tag]] + extra) == 0
    names = sorted(os.listdir(os.path.join(tmp, "img")))
    assert len(names) == 5
    for n in names:
        for f in ("disp.dmb", "normals.dmb", "cost.dmb"):
            a = open(os.path.join(outs["plain"], n[:-4], f), "rb").read()
            assert a == open(os.path.join(outs["off"], n[:-4], f), "rb").read(), (n, f)
    rep_off = json.load(open(os.path.join(outs["off"], "batch_rank0.json")))
    assert "order" not in rep_off and all("prior" not in v for v in rep_off["views"])
    rep = json.load(open(os.path.join(outs["prior"], "batch_rank0.json")))
    assert rep["view_prior"] == 4 and rep["prior_iterations"] == 2 and rep["fusion"]["points"] > 0
    assert len(dmb.read_ply_binary(os.path.join(outs["prior"], "fused.ply"))) == rep["fusion"]["points"]
    # the same plan, made of the restatements and the oracle
    P_all = [cameras.read_p_file(os.path.join(tmp, "p", n + ".P")) for n in names]
    host = [batch.read_image(os.path.join(tmp, "img", n)) for n in names]
    cam_scale = float(f32(scan.cam_scale))
    ap = batch.AlgorithmParameters(iterations=3, n_best=3, depthMin=300.0, depthMax=800.0, min_angle=2.0, max_angle=60.0,
                                   max_views=10)
    ap.set_blocksize(11)
    plans = {n: batch.plan_views(P_all, names, i, 160, 120, ap, cam_scale) for i, n in enumerate(names)}
    order = prior.greedy_order(names, {n: [names[i] for i in plans[n][1][1:]] for n in names})
    assert rep["order"] == order == [v["ref"] for v in rep["views"]]
    done, seeded = {}, 0
    for n, entry in zip(order, rep["views"]):
        cs, used, ap_view = plans[n]
        have = [names[i] for i in used[1:] if names[i] in done][:4]
        folder = os.path.join(outs["prior"], n[:-4])
        if len(have) >= 2:
            seeded += 1
            ref = prior_ref.prior_from_views(
                fusion.view_constants(P_all[used[0]], cam_scale), [done[m][0] for m in have],
                [fusion.view_constants(P_all[names.index(m)], cam_scale) for m in have], ap_view.depthMin, ap_view.depthMax,
                costs=[done[m][1] for m in have], max_cost=0.6)
            assert entry["prior"]["sources"] == have and entry["iterations"] == 2 and entry["prior"]["device_ms"] > 0
            assert [entry["prior"][k] for k in ("direct", "filled", "empty")] == ref.counts
            ap_view.iterations = 2
            gs = GlobalState([host[i] for i in used], cs, list(range(1, len(used))), ap_view, seed=1)
            r_n4, r_c, _ = pyramid_ref.solve_seeded(gs, ref.prior, 0)
        else:
            assert entry["prior"] is None and entry["iterations"] == 3
            gs = GlobalState([host[i] for i in used], cs, list(range(1, len(used))), ap_view, seed=1)
            r_n4, r_c = OracleState(gs).run()
        assert_same(dmb.read_dmb(os.path.join(folder, "disp.dmb")), r_n4[..., 3], "%s disp.dmb" % n)
        assert_same(dmb.read_dmb(os.path.join(folder, "normals.dmb")), r_n4[..., :3], "%s normals.dmb" % n)
        assert_same(dmb.read_dmb(os.path.join(folder, "cost.dmb")), r_c, "%s cost.dmb" % n)
        done[n] = (np.ascontiguousarray(r_n4), np.ascontiguousarray(r_c))
    assert seeded >= 3 and order[0] == names[0]
    # the references last to first: the greedy order starts at the scan's last view, the fusion still at its first
    out_rev = os.path.join(tmp, "prior_rev")
    assert batch.main(args + ["--output-folder", out_rev, "--views", ",".join(reversed(names)), "--view_prior", "4",
                              "--prior_iterations", "2", "--fuse", "--disp_thresh=%r" % (0.5 / scan.cam_scale),
                              "--num_consistent=2"]) == 0
    rep_rev = json.load(open(os.path.join(out_rev, "batch_rank0.json")))
    order_rev = prior.greedy_order(names[::-1], {n: [names[i] for i in plans[n][1][1:]] for n in names})
    assert order_rev[0] == names[-1] and order_rev != names
    assert rep_rev["order"] == order_rev == [v["ref"] for v in rep_rev["views"]]
    assert [v["name"] for v in rep_rev["fusion"]["views"]] == names and rep_rev["fusion"]["points"] > 0
