"""Thinning a cloud to a minimum point spacing (gipuma_hip_cloud_thin, gipuma_amd.cloud_eval.thin).  Every
case is a cloud, a radius, a seed, an order and a condition -- stated on the restatement (tests/thin_ref.py) alone -- that
it reaches the path it is named for; that condition runs without a device, and so do the comparison of the restatement's
two forms (the sequential pass of the contract, the synchronous rounds of the kernels), a k-d tree's second opinion on the
two properties the contract implies, the C-ABI's argument checks and the command lines.  GPU: the mask as bytes, the four
counts (the number of rounds included) and the returned indices equal the restatement at every grid; the descriptor's
stream; device tensors; the score with `reduce`."""
import ctypes as C
import functools

import numpy as np
import pytest

from gipuma_amd import abi, cloud_eval
from tests import thin_ref
from tests.abi_layout import assert_mirrors_header

f32 = np.float32
GRIDS = (0, 1, 2, 7, 256)


class Case:
    def __init__(self, points, radius, check, seed=0, order="hashed", grids=GRIDS):
        self.points = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
        self.radius, self.check, self.seed, self.order, self.grids = f32(radius), check, seed, order, grids

    @functools.cached_property
    def ref(self):
        return thin_ref.thin(self.points, self.radius, self.seed, self.order)


def _uniform(n=3000, seed=101, box=20.0):
    return np.random.default_rng(seed).uniform(0.0, box, (n, 3)).astype(f32)


def _sphere(n=6000, radius=50.0, sigma=0.2, seed=202):
    """the first of DESIGN.md 14's two noisy samplings of a sphere"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= radius / np.linalg.norm(v, axis=1, keepdims=True)
    return v + rng.normal(scale=sigma, size=(n, 3))


def _lattice_twice():
    g = np.arange(8, dtype=np.float64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([lattice, lattice])


def _shares(kept, dropped):
    def check(c):
        n = len(c.points)
        assert c.ref.kept >= kept * n and c.ref.dropped >= dropped * n, (c.ref.kept, c.ref.dropped)
        assert c.ref.rounds >= 3  # chains of dependent decisions: more than the two rounds of isolated pairs
    return check


def _case_collinear(order):
    x = np.zeros((300, 3))
    x[:, 0] = 0.6 * np.arange(300)  # a neighbour at 0.6 on either side, the next ones at 1.2

    def check(c):
        r = c.ref
        if order == "index":
            # every point waits for its left neighbour: one decision per round, the worklist goes down one by one
            assert (r.kept, r.rounds) == (150, 300) and np.array_equal(r.keep, np.arange(300) % 2 == 0)
            assert r.undecided == list(range(299, -1, -1))
        else:
            assert r.rounds < 20 and 100 <= r.kept <= 150  # (a maximal set takes a half to a third of the points)
    return Case(x, 1.0, check, order=order)


def _case_lattice(which):
    def check(c):
        r = c.ref
        if which == "pairs":  # the two copies of a site are 0 apart, two sites 1: exactly one of each pair
            assert np.array_equal(r.keep[:512] + r.keep[512:], np.ones(512, np.uint8)) and (r.kept, r.rounds) == (512, 2)
            assert r.keep[:512].any() and r.keep[512:].any()  # (the hash, not the index, picks the copy)
        else:  # d2 == r2 exactly between adjacent sites: the inclusive radius drops them
            assert (r.kept, r.rounds) == (256, 22) and not r.keep[512:].any()
            sites = c.points[:512][r.keep[:512] == 1].astype(np.float64)
            d = np.abs(sites[:, None] - sites[None]).sum(-1)
            assert not (d == 1).any()
    return Case(_lattice_twice(), 0.5 if which == "pairs" else 1.0, check, order="hashed" if which == "pairs" else "index")


def _case_pair(inside):
    def check(c):
        assert c.ref.kept == (1 if inside else 2) and c.ref.rounds == (2 if inside else 1)
    return Case([[0, 0, 0], [3, 4, 0]], f32(5) if inside else np.nextafter(f32(5), f32(0)), check)


def _case_identical():
    def check(c):
        r = c.ref
        first = int(thin_ref.visiting_order(c.points, c.seed, c.order)[0])
        assert (r.kept, r.rounds) == (1, 2) and r.keep[first] == 1 and first != 0
    return Case(np.repeat(_uniform(1, seed=707), 500, axis=0), 1.0, check)


def _case_radius(which):
    def check(c):
        if which == "tiny":
            assert (c.ref.kept, c.ref.rounds) == (len(c.points), 1)
        else:
            assert c.ref.kept == 1
    return Case(_uniform(), 1e-3 if which == "tiny" else 1000.0, check)


def _case_count(n):
    def check(c):
        assert c.ref.kept + c.ref.dropped == n
        if n <= 1:
            assert (c.ref.kept, c.ref.rounds) == (n, n)  # nothing: no round; one point: kept in the first
        else:
            assert 0 < c.ref.dropped and 0 < c.ref.kept
    return Case(_uniform(n, seed=303, box=4.0), 1.0, check)


def _case_non_finite():
    pts = _uniform()
    rng = np.random.default_rng(808)
    rows = rng.choice(len(pts), len(pts) // 100, replace=False)
    pts[rows, rng.integers(0, 3, len(rows))] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=f32), len(rows))

    def check(c):
        r = c.ref
        assert r.not_finite == 30 and not r.keep[rows].any() and r.kept + r.dropped == len(pts) - 30
        # never a suppressor: the finite points' mask is the one of the cloud without the others (hashed by the same index)
        clean = c.points.copy()
        clean[rows] = 1e6 + 100.0 * np.arange(len(rows), dtype=f32)[:, None]  # far away from everything and each other
        ok = np.ones(len(pts), bool)
        ok[rows] = False
        assert np.array_equal(thin_ref.sequential(clean, c.radius, c.seed, c.order)[ok], r.keep[ok])
    return Case(pts, 1.5, check)


def _case_flat(kind):
    rng = np.random.default_rng(707)
    if kind == "coplanar":
        pts = rng.uniform(0.0, 10.0, (2000, 3))
        pts[:, 2] = 4.0
    else:
        pts = np.array([1.0, 2.0, 3.0]) + np.sort(rng.uniform(0.0, 10.0, 500))[:, None] * np.array([1.0, 0.0, 0.0])

    def check(c):
        ext = c.points.max(axis=0) - c.points.min(axis=0)
        assert (ext == 0).sum() == (1 if kind == "coplanar" else 2)  # axes of zero extent: one cell each
        assert c.ref.kept >= 0.05 * len(pts) and c.ref.dropped >= 0.3 * len(pts)
    return Case(pts, 0.3 if kind == "coplanar" else 0.05, check)


def _case_crowded():
    rng = np.random.default_rng(909)
    pts = np.concatenate([rng.uniform(0.0, 0.01, (20000, 3)), [[1000.0, 0.0, 0.0], [0.0, 1000.0, 0.0]]])

    def check(c):
        p = c.points.astype(np.float64)
        ext = p.max(axis=0) - p.min(axis=0)
        h = ext.max() / 4
        cells = np.floor(ext / h).astype(int) + 1
        assert int(np.prod(np.minimum(cells, 4))) == 16  # the grid of 4: 4 x 4 x 1 cells
        assert len({tuple(r) for r in np.floor((p[:20000] - p.min(axis=0)) / h).astype(int)}) == 1  # 20 000 points in one
        assert c.ref.kept >= 0.1 * len(pts) and c.ref.dropped >= 0.1 * len(pts) and c.ref.keep[20000:].all()
    return Case(pts, 5e-4, check, grids=(0, 4))


def _case_large_coordinates():
    scale = 0.02 / np.sqrt(4 * np.pi * 50.0 ** 2 / 6000)  # mean spacing of 6000 points on the sphere -> 0.02
    pts = (_sphere() * scale + 65536.0).astype(f32)

    def check(c):
        assert c.ref.kept >= 0.2 * len(pts) and c.ref.dropped >= 0.2 * len(pts)
        assert np.spacing(f32(65536.0)) > 0.25 * c.radius  # a coordinate's own rounding step is a quarter of the radius
    return Case(pts, 0.03, check)


BUILDERS = {
    **{"uniform_seed%d" % s: functools.partial(lambda s: Case(_uniform(), 1.5, _shares(0.25, 0.50), seed=s), s)
       for s in (0, 1, 12345)},
    "uniform_index": lambda: Case(_uniform(), 1.5, _shares(0.25, 0.50), order="index"),
    "sphere": lambda: Case(_sphere(), 2.0, _shares(0.30, 0.30)),
    "collinear_index": lambda: _case_collinear("index"),
    "collinear_hashed": lambda: _case_collinear("hashed"),
    "lattice_pairs": lambda: _case_lattice("pairs"),
    "lattice_inclusive": lambda: _case_lattice("inclusive"),
    "radius_inclusive": lambda: _case_pair(True),
    "radius_just_short": lambda: _case_pair(False),
    "identical": _case_identical,
    "radius_tiny": lambda: _case_radius("tiny"),
    "radius_huge": lambda: _case_radius("huge"),
    **{"points_%d" % n: functools.partial(_case_count, n) for n in (0, 1, 63, 64, 65, 257)},
    "non_finite": _case_non_finite,
    "flat_coplanar": lambda: _case_flat("coplanar"),
    "flat_collinear": lambda: _case_flat("collinear"),
    "crowded_cell": _case_crowded,
    "large_coordinates": _case_large_coordinates,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_prio_known_answers():
    assert thin_ref.prio(5, 0).tolist() == [363934122, 2569593342, 3816931001, 608282661, 4132357579]
    assert thin_ref.prio(3, 7).tolist() == [827110146, 3547762833, 3223061855]
    assert thin_ref.prio(4, 9, "index").tolist() == [0, 0, 0, 0]
    assert thin_ref.visiting_order([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [2, 2, 2]], 0).tolist() == [0, 3, 2]  # (by prio)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    r = c.ref
    assert r.kept + r.dropped + r.not_finite == len(c.points) and r.kept == int(r.keep.sum())
    assert r.rounds == len(r.undecided) and (not r.undecided or r.undecided[-1] == 0)
    assert all(a > b for a, b in zip([r.kept + r.dropped] + r.undecided, r.undecided))  # every round decides something


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_the_sequential_pass_equals_the_rounds(name):
    c = case(name)
    assert np.array_equal(thin_ref.sequential(c.points, c.radius, c.seed, c.order), c.ref.keep)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_kept_points_are_apart_and_dropped_points_are_covered(name):
    """the two properties the contract implies, judged by a k-d tree in float64.  Pairs whose distance is within 1e-5 of
    the radius (relative) are left to the restatement: float32's d2 carries five roundings of 2^-24."""
    from scipy.spatial import cKDTree
    c = case(name)
    r, radius = c.ref, float(c.radius)
    ok = np.isfinite(c.points).all(axis=1)
    kept = np.nonzero(r.keep == 1)[0]
    dropped = np.nonzero((r.keep == 0) & ok)[0]
    assert not (r.keep[~ok]).any()
    if len(kept) == 0:
        assert ok.sum() == 0
        return
    tree = cKDTree(c.points[kept].astype(np.float64))
    assert len(tree.query_pairs(radius * (1 - 1e-5))) == 0
    rank = np.empty(len(c.points), dtype=np.int64)
    rank[np.lexsort((np.arange(len(c.points)), thin_ref.prio(len(c.points), c.seed, c.order)))] = np.arange(len(c.points))
    near = tree.query_ball_point(c.points[dropped].astype(np.float64), radius * (1 + 1e-5))
    for i, js in zip(dropped, near):
        assert js and rank[kept[js]].min() < rank[i], "dropped point %d has no kept point of lower key within the radius" % i


def test_two_seeds_give_different_masks_and_one_seed_the_same():
    a, b = case("uniform_seed0"), case("uniform_seed1")
    assert np.array_equal(a.points, b.points) and not np.array_equal(a.ref.keep, b.ref.keep)
    assert np.array_equal(thin_ref.thin(a.points, a.radius, 0).keep, a.ref.keep)


def _desc(**kw):
    d = abi.ThinDesc()
    d.abi_version, d.n_points, d.points, d.radius, d.seed, d.order = abi.ABI_VERSION, 4, 0x1000, 1.0, 0, 0
    d.grid, d.device_id, d.stream = 0, 0, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last ones for want of a device when there is
    none -- with a device they are not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(keep=out, **kw):
        return lib.gipuma_hip_cloud_thin(C.byref(_desc(**kw)), keep, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(radius=bad) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    for bad in (2, -1):
        assert rc(order=bad) == abi.ERR_ARG and b"order" in lib.gipuma_hip_last_error()
    assert rc(points=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(keep=None) == abi.ERR_ARG
    assert rc(n_points=-1) == abi.ERR_ARG
    assert rc(n_points=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_thin(None, out, None, None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        assert rc() == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        assert rc(n_points=0, points=None, keep=None) == abi.ERR_NO_DEVICE  # valid, too
        with pytest.raises(abi.GipumaHipError):
            cloud_eval.thin(np.zeros((2, 3), f32), 1.0)
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG
    with pytest.raises(ValueError):
        cloud_eval.thin(np.zeros((2, 3), f32), 1.0, order="random")


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.ThinDesc, "gipuma_hip_thin_desc")
    assert "gipuma_hip_cloud_thin" in [s[0] for s in abi.SYMBOLS]


CLI = ["--cloud", "c.ply", "--reference", "r.ply"]


@pytest.mark.parametrize("argv", [CLI + ["--reduce", "-0.2"], CLI + ["--reduce", "nan"], CLI + ["--reduce", "inf"],
                                  CLI + ["--reduce_reference"], CLI + ["--reduce", "0.2", "--seed", "-1"],
                                  CLI + ["--reduce", "0.2", "--seed", str(2 ** 32)]])
def test_cli_reduce_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_reduce_arguments():
    a = cloud_eval.parse_args(CLI)
    assert a.reduce == 0.0 and a.reduce_reference is False and a.seed == 0
    a = cloud_eval.parse_args(CLI + ["--reduce", "0.2", "--reduce_reference", "--seed", "7"])
    assert a.reduce == float(f32(0.2)) and a.reduce_reference is True and a.seed == 7


def test_batch_eval_reduce_arguments(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    assert batch.parse_args(base).eval_reduce == 0.0
    a = batch.parse_args(base + ["--fuse", "--eval_cloud", "gt.ply", "--eval_reduce", "0.2"])
    assert a.eval_reduce == float(f32(0.2)) and a.eval_cloud == "gt.ply"
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + ["--fuse", "--eval_reduce", "0.2"])
    assert e.value.code == 2 and "--eval_cloud" in capsys.readouterr().err
    for bad in ("-1", "nan"):
        with pytest.raises(SystemExit):
            batch.parse_args(base + ["--fuse", "--eval_cloud", "gt.ply", "--eval_reduce", bad])
    capsys.readouterr()


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _assert_equals_ref(keep, info, c, what):
    r = c.ref
    assert keep.dtype == np.uint8 and np.array_equal(keep, r.keep), \
        "%s: the mask differs at %d points" % (what, int((keep != r.keep).sum()))
    assert (info["kept"], info["dropped"], info["not_finite"], info["rounds"]) == (r.kept, r.dropped, r.not_finite, r.rounds), what


GPU_RUNS = [(name, g) for name in sorted(BUILDERS) for g in (BUILDERS[name]().grids if name == "crowded_cell" else GRIDS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_kernels_equal_the_restatement_byte_for_byte(hip, name, grid):
    c = case(name)
    c.check(c)
    what = "%s at grid %d" % (name, grid)
    keep, ms, info = cloud_eval.thin_mask(c.points, c.radius, c.seed, c.order, grid=grid)
    _assert_equals_ref(keep.cpu().numpy(), info, c, what)
    idx, ms, info = cloud_eval.thin(c.points, c.radius, c.seed, c.order, grid=grid, return_info=True)
    assert idx.dtype == np.int64 and np.array_equal(idx, np.nonzero(c.ref.keep)[0]), what
    assert (info["kept"], info["dropped"], info["not_finite"], info["rounds"]) == \
        (c.ref.kept, c.ref.dropped, c.ref.not_finite, c.ref.rounds), what
    ok = c.points[np.isfinite(c.points).all(axis=1)]
    if len(ok):
        assert ms > 0
        ext = ok.max(axis=0) - ok.min(axis=0)
        if grid and ext.max() > 0:
            assert info["grid"] == grid and max(info["cells_x"], info["cells_y"], info["cells_z"]) == grid
            assert all(info["cells_" + k] == 1 for k, e in zip("xyz", ext) if e == 0)  # an axis of zero extent: one cell
        if name == "crowded_cell" and grid == 4:
            assert info["cells_x"] * info["cells_y"] * info["cells_z"] == 16
    else:
        assert info["grid"] == 0 and info["rounds"] == 0


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_runs_repeat(hip):
    import torch
    c, other = case("sphere"), case("uniform_seed1")
    pts = torch.from_numpy(c.points).cuda()
    masks = []
    for _ in range(2):  # (the order inside a cell varies from run to run; the mask and the rounds do not)
        keep, ms, info = cloud_eval.thin_mask(pts, c.radius, c.seed, c.order)
        assert keep.is_cuda
        masks.append(keep.cpu().numpy().tobytes())
        _assert_equals_ref(keep.cpu().numpy(), info, c, "device tensor")
    assert masks[0] == masks[1]
    upts = torch.from_numpy(other.points).cuda()
    k0 = cloud_eval.thin_mask(upts, other.radius, 0)[0].cpu().numpy()
    k1 = cloud_eval.thin_mask(upts, other.radius, 1)[0].cpu().numpy()
    assert np.array_equal(k0, case("uniform_seed0").ref.keep) and np.array_equal(k1, other.ref.keep) and not np.array_equal(k0, k1)


@pytest.mark.gpu
def test_thinning_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the cloud was written just before, the device not synchronised: the library
    runs behind it on that stream.  Two cloud sizes one after the other on the same stream."""
    import torch
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("uniform_seed12345", "points_257"):
        c = case(name)
        staged = torch.from_numpy(c.points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the cloud the library reads: a device copy queued on the caller's stream
            pts = staged.clone()
            keep = torch.empty(len(c.points), dtype=torch.uint8, device="cuda")
        d = _desc(n_points=len(c.points), points=pts.data_ptr(), radius=float(c.radius), seed=c.seed, stream=stream.cuda_stream)
        info, ms = (C.c_int64 * 8)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_thin(C.byref(d), keep.data_ptr(), info, C.byref(ms)), "thin")
        got = dict(kept=info[0], dropped=info[1], not_finite=info[2], rounds=info[3])
        _assert_equals_ref(keep.cpu().numpy(), got, c, "%s on the caller's stream" % name)
        assert ms.value > 0
    abi.check(lib, lib.gipuma_hip_cloud_thin(C.byref(_desc(n_points=0, points=None)), None, None, None), "thin of nothing")


SCORE_KEYS = {"accuracy", "completeness", "thresholds", "precision", "recall", "fscore", "max_dist", "cloud_points",
              "reference_points", "accuracy_device_ms", "completeness_device_ms", "accuracy_search", "completeness_search"}
NEW_KEYS = {"reduce", "cloud_points_before", "reference_points_before", "thin_rounds", "thin_device_ms"}
TIMES = {"accuracy_device_ms", "completeness_device_ms"}  # (a time is not a result: positive, never equal)


@pytest.mark.gpu
def test_score_with_reduce_is_the_score_of_the_thinned_cloud(hip):
    rng = np.random.default_rng(17)
    cloud = rng.uniform(0.0, 30.0, (4000, 3)).astype(f32)
    ref = rng.uniform(0.0, 30.0, (5000, 3)).astype(f32)
    plain = cloud_eval.score(cloud, ref, max_dist=2.0)
    assert set(plain) == SCORE_KEYS  # without the option: key for key what it was
    idx, ridx = cloud_eval.thin(cloud, 1.0, seed=3), cloud_eval.thin(ref, 1.0, seed=3)
    assert np.array_equal(idx, np.nonzero(thin_ref.sequential(cloud, 1.0, 3))[0]) and 0 < len(idx) < 4000
    for both in (False, True):
        got = cloud_eval.score(cloud, ref, max_dist=2.0, reduce=1.0, reduce_reference=both, seed=3)
        want = cloud_eval.score(cloud[idx], ref[ridx] if both else ref, max_dist=2.0)
        assert set(got) == SCORE_KEYS | NEW_KEYS
        for k in SCORE_KEYS - TIMES:
            assert got[k] == want[k], k
        assert all(got[k] > 0 for k in TIMES)
        assert got["reduce"] == 1.0 and got["cloud_points_before"] == 4000 and got["reference_points_before"] == 5000
        assert got["cloud_points"] == len(idx) and got["reference_points"] == (len(ridx) if both else 5000)
        assert len(got["thin_rounds"]) == len(got["thin_device_ms"]) == (2 if both else 1)
        assert all(r >= 1 for r in got["thin_rounds"]) and all(m > 0 for m in got["thin_device_ms"])
    assert plain["cloud_points"] == 4000 and plain["accuracy"] != got["accuracy"]
