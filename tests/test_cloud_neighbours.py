"""Counting a point's neighbours within a radius and dropping the isolated points (DESIGN.md 16,
gipuma_hip_cloud_neighbours, gipuma_amd.cloud_eval.neighbour_counts / drop_isolated).  Every case is a cloud, a radius, a
min_neighbours, a max_count and a condition -- stated on the restatement (tests/neighbours_ref.py) alone -- that it
reaches the path it is named for; that condition runs without a device, and so do the comparison of the restatement's two
forms (the brute force, the k-d tree's pairs), the C-ABI's argument checks, the command lines and the PLY round trip of
--write_cloud.  GPU: the counts as uint32, the mask as bytes and the four info counts equal the restatement at every grid;
either output alone; the descriptor's stream; device tensors; the score with the filter."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
# torch before the `hip` fixture loads the library (see tests/test_cloud_scale.py): this module must also run on its own
import torch  # noqa: F401

from gipuma_amd import abi, cloud_eval, dmb
from tests import neighbours_ref
from tests import test_cloud_scale as scale
from tests import test_cloud_thin as thin_cases
from tests.abi_layout import assert_mirrors_header

f32 = np.float32
GRIDS = thin_cases.GRIDS
assert GRIDS == (0, 1, 2, 7, 256)


# ----------------------------------------------------------------------------------------------------------------------
# The clouds (by name: several cases share one, and its brute force) and the cases
# ----------------------------------------------------------------------------------------------------------------------
N_SPHERE = 6000
CLUMPS = np.array([[0.0, 0.0, 0.0], [20.0, -10.0, 5.0], [-15.0, 20.0, -10.0]])  # inside the sphere, 20 and more from it


def _sphere_with_floaters():
    """the noisy sphere, then the single floaters (>= 8 from the surface), then three clumps of three floaters"""
    f = np.random.default_rng(7).uniform(-80.0, 80.0, (60, 3))
    f = f[np.abs(np.linalg.norm(f, axis=1) - 50.0) >= 8.0]
    clumps = (CLUMPS[:, None, :] + np.array([[0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [0.0, 0.6, 0.0]])[None]).reshape(-1, 3)
    return np.concatenate([thin_cases._sphere(), f, clumps])


def _moved_away(points, rows):
    """the cloud with `rows` put far away from everything and from each other"""
    p = points.copy()
    p[rows] = 1e6 + 100.0 * np.arange(len(rows), dtype=f32)[:, None]
    return p


CLOUDS = {
    "uniform": thin_cases._uniform,
    "sphere_floaters": _sphere_with_floaters,
    "lattice_twice": thin_cases._lattice_twice,
    "pair": lambda: [[0, 0, 0], [3, 4, 0]],
    "identical": lambda: thin_cases.case("identical").points,
    **{"points_%d" % n: functools.partial(lambda n: thin_cases.case("points_%d" % n).points, n) for n in (0, 1, 63, 64, 65, 257)},
    "non_finite": lambda: thin_cases.case("non_finite").points,
    "non_finite_moved": lambda: _moved_away(cloud("non_finite"), np.nonzero(~np.isfinite(cloud("non_finite")).all(axis=1))[0]),
    "flat_coplanar": lambda: thin_cases.case("flat_coplanar").points,
    "flat_collinear": lambda: thin_cases.case("flat_collinear").points,
    "crowded_cell": lambda: thin_cases.case("crowded_cell").points,
    "large_coordinates": lambda: thin_cases.case("large_coordinates").points,
    **{"scale_" + name: functools.partial(lambda name: scale.thin_case(name).points, name) for name in scale.THIN_BUILDERS},
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    return np.ascontiguousarray(CLOUDS[name](), dtype=f32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def exact(name, radius):
    """the brute force's exact counts of a cloud at a radius, computed once for every case that shares them"""
    e = neighbours_ref.neighbours(cloud(name), radius).exact
    e.setflags(write=False)
    return e


class Case:
    def __init__(self, name, radius, min_neighbours, max_count, check, grids=GRIDS):
        self.name, self.radius, self.min_neighbours, self.max_count = name, f32(radius), min_neighbours, max_count
        self.check, self.grids = check, grids

    @property
    def points(self):
        return cloud(self.name)

    @functools.cached_property
    def ref(self):
        return neighbours_ref.from_exact(self.points, exact(self.name, self.radius), self.min_neighbours, self.max_count)


def _case_uniform(max_count):
    def check(c):
        r, n = c.ref, len(c.points)
        assert (int(r.exact.min()), int(r.exact.max())) == (0, 14) and 4.5 < r.exact.mean() < 5.5
        assert r.kept >= 0.2 * n and r.dropped >= 0.2 * n and r.not_finite == 0, (r.kept, r.dropped)
        if max_count:  # saturation stops the count, never changes the mask
            assert r.saturated == r.kept and int(r.count.max()) == max_count and (r.count < r.exact).any()
            assert np.array_equal(r.keep, case("uniform").ref.keep)
        else:
            assert r.saturated == 0 and np.array_equal(r.count, r.exact)
    return Case("uniform", 1.5, 4, max_count, check)


def _case_sphere_floaters():
    def check(c):
        r, p = c.ref, c.points
        floaters, clumps = np.arange(N_SPHERE, len(p) - 9), np.arange(len(p) - 9, len(p))
        assert len(floaters) == 54 and (np.abs(np.linalg.norm(p[floaters].astype(np.float64), axis=1) - 50.0) >= 8.0).all()
        assert not r.exact[floaters].any() and not r.keep[floaters].any()  # every single floater stands alone
        assert (r.exact[clumps] == 2).all() and not r.keep[clumps].any()  # a clump's members count each other only
        assert r.keep[:N_SPHERE].sum() >= 0.99 * N_SPHERE and r.exact[:N_SPHERE].min() >= 1
        assert r.dropped >= 63 and r.kept == int(r.keep[:N_SPHERE].sum())
    return Case("sphere_floaters", 6.0, 6, 0, check)


def _case_lattice(which):
    def check(c):
        e = c.ref.exact
        if which == "copies":  # two sites are 1 apart, the two copies of a site 0: the copy and nothing else
            assert (e == 1).all() and c.ref.kept == 1024
        else:  # d2 == r2 exactly between adjacent sites: the inclusive radius counts them, twice each, and the copy
            g = np.arange(8)
            inner = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
            inner = ((inner > 0) & (inner < 7)).all(axis=1)
            assert (e[:512][inner] == 13).all() and (e[512:][inner] == 13).all() and e.min() == 7 and e.max() == 13
            assert c.ref.kept == 2 * int(inner.sum()) == 432
    return Case("lattice_twice", 0.5 if which == "copies" else 1.0, 1 if which == "copies" else 13, 0, check)


def _case_pair(inside):
    def check(c):
        assert c.ref.exact.tolist() == ([1, 1] if inside else [0, 0]) and c.ref.kept == (2 if inside else 0)
    return Case("pair", f32(5) if inside else np.nextafter(f32(5), f32(0)), 1, 0, check)


def _case_identical(max_count):
    def check(c):
        assert (c.ref.exact == 499).all() and (c.ref.count == (max_count or 499)).all()
        assert (c.ref.kept, c.ref.saturated) == (500, 500 if max_count else 0)
    return Case("identical", 1.0, max_count or 499, max_count, check)


def _case_radius(which):
    def check(c):
        n = len(c.points)
        assert (c.ref.exact == (0 if which == "tiny" else n - 1)).all() and c.ref.kept == (0 if which == "tiny" else n)
    return Case("uniform", 1e-3 if which == "tiny" else 1000.0, 1, 0, check)


def _case_count(n):
    def check(c):
        assert len(c.points) == n and c.ref.kept + c.ref.dropped == n
        if n >= 63:
            assert 0 < c.ref.kept and 0 < c.ref.dropped
        else:
            assert c.ref.kept == 0 and c.ref.dropped == n  # nothing, or one point without a neighbour
    return Case("points_%d" % n, 1.0, 12 if n == 257 else 4 if n >= 63 else 1, 0, check)


def _case_non_finite():
    def check(c):
        r, p = c.ref, c.points
        bad = ~np.isfinite(p).all(axis=1)
        assert bad.sum() == 30 == r.not_finite and not r.count[bad].any() and not r.keep[bad].any()
        assert c.min_neighbours == 0 and np.array_equal(r.keep, (~bad).astype(np.uint8)) and r.dropped == 0
        # never counted by others: the finite points count what they count in the cloud without the others
        assert np.array_equal(exact("non_finite_moved", c.radius)[~bad], r.exact[~bad]) and r.exact[~bad].max() >= 4
    return Case("non_finite", 1.5, 0, 0, check)


def _case_flat(kind):
    def check(c):
        ext = c.points.max(axis=0) - c.points.min(axis=0)
        assert (ext == 0).sum() == (1 if kind == "coplanar" else 2)  # axes of zero extent: one cell each
        assert c.ref.kept >= 0.2 * len(c.points) and c.ref.dropped >= 0.05 * len(c.points), (c.ref.kept, c.ref.dropped)
    return Case("flat_" + kind, 0.3 if kind == "coplanar" else 0.05, 5 if kind == "coplanar" else 4, 0, check)


def _case_crowded(max_count):
    def check(c):
        thin_cases.case("crowded_cell").check(thin_cases.case("crowded_cell"))  # 20 000 points in one of 16 cells
        r = c.ref
        assert not r.exact[20000:].any() and not r.keep[20000:].any()
        assert r.kept >= 0.2 * 20000 and r.dropped >= 0.1 * 20000, (r.kept, r.dropped)
        assert r.saturated == (r.kept if max_count else 0)
    return Case("crowded_cell", 5e-4, 8, max_count, check, grids=(0, 4))


def _case_large_coordinates():
    def check(c):
        assert np.spacing(f32(65536.0)) > 0.25 * c.radius  # a coordinate's own rounding step is a quarter of the radius
        assert c.ref.kept >= 0.2 * len(c.points) and c.ref.dropped >= 0.2 * len(c.points), (c.ref.kept, c.ref.dropped)
    return Case("large_coordinates", 0.03, 7, 0, check)


def _case_scale(name):
    """the thinning's extreme scales (tests/test_cloud_scale.py): its clouds, its radii and its expectation of one cell"""
    t = scale.thin_case(name)

    def check(c):
        t.check(t)
        r, n = c.ref, len(c.points)
        assert tuple(g for g in GRIDS if scale.thin_layout(c, g)[1]) == tuple(t.one_cell)
        if name == "r2_infinite":  # inf <= inf: every finite point counts all the others, the two at +-3e38 included
            assert np.isposinf(neighbours_ref.squared(c.radius)) and (r.exact == n - 1).all() and np.abs(c.points).max() > 2.9e38
        elif name == "r2_zero":  # only the exact copy is within a radius whose square is 0
            assert neighbours_ref.squared(c.radius) == 0 and (r.exact == 1).all()
        else:
            assert r.kept >= 20 and r.dropped >= 20, (r.kept, r.dropped)
    return Case("scale_" + name, t.radius, {"r2_infinite": 401, "r2_zero": 1}.get(name, 14 if name.endswith("41") else 2), 0, check)


BUILDERS = {
    "uniform": lambda: _case_uniform(0),
    "uniform_saturated": lambda: _case_uniform(4),
    "sphere_floaters": _case_sphere_floaters,
    "lattice_copies": lambda: _case_lattice("copies"),
    "lattice_inclusive": lambda: _case_lattice("inclusive"),
    "radius_inclusive": lambda: _case_pair(True),
    "radius_just_short": lambda: _case_pair(False),
    "identical": lambda: _case_identical(0),
    "identical_saturated": lambda: _case_identical(10),
    "radius_tiny": lambda: _case_radius("tiny"),
    "radius_huge": lambda: _case_radius("huge"),
    **{"points_%d" % n: functools.partial(_case_count, n) for n in (0, 1, 63, 64, 65, 257)},
    "non_finite": _case_non_finite,
    "flat_coplanar": lambda: _case_flat("coplanar"),
    "flat_collinear": lambda: _case_flat("collinear"),
    "crowded_cell": lambda: _case_crowded(0),
    "crowded_cell_saturated": lambda: _case_crowded(8),
    "large_coordinates": _case_large_coordinates,
}
SCALE_BUILDERS = {"scale_" + name: functools.partial(_case_scale, name) for name in scale.THIN_BUILDERS}
ALL_BUILDERS = {**BUILDERS, **SCALE_BUILDERS}


@functools.lru_cache(maxsize=None)
def case(name):
    return ALL_BUILDERS[name]()


# the large cloud: test_cloud_scale's 300 001 targets, against the sparse restatement
LARGE_RADIUS, LARGE_MIN = 0.3, 2


@functools.lru_cache(maxsize=None)
def large_ref(max_count):
    return neighbours_ref.neighbours_sparse(scale.large_clouds()[1], LARGE_RADIUS, LARGE_MIN, max_count)


def _check_large(max_count):
    r = large_ref(max_count)
    assert r.not_finite == 0 and r.kept + r.dropped == scale.N_LARGE
    assert r.kept >= 0.2 * scale.N_LARGE and r.dropped >= 0.2 * scale.N_LARGE, (r.kept, r.dropped)
    assert not r.exact[list(scale.OUTLIERS)].any()  # (nothing within 10 of them)
    assert r.saturated == (int((r.exact >= max_count).sum()) if max_count else 0) and (max_count == 0 or 0 < r.saturated < r.kept)
    assert np.array_equal(r.keep, large_ref(0).keep)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    r = c.ref
    assert r.count.dtype == np.uint32 and r.keep.dtype == np.uint8 and len(r.count) == len(r.keep) == len(c.points)
    assert r.kept + r.dropped + r.not_finite == len(c.points) and r.kept == int(r.keep.sum())
    assert int(r.exact.sum()) % 2 == 0  # d2 is bitwise symmetric: every neighbour pair counts twice
    if c.max_count == 0:
        assert int(r.count.astype(np.int64).sum()) % 2 == 0 and r.saturated == 0
    else:
        assert c.min_neighbours <= c.max_count and int(r.count.max(initial=0)) <= c.max_count


def test_the_sparse_restatement_equals_the_brute_force_on_every_small_case():
    """(the extreme scales are not of the ordinary magnitudes the sparse form's argument needs: they are judged against
    the brute force alone, as in tests/test_cloud_scale.py)"""
    for name in sorted(BUILDERS):
        c = case(name)
        s = neighbours_ref.neighbours_sparse(c.points, c.radius, c.min_neighbours, c.max_count)
        assert s is not None, name
        for got, want in zip(s, c.ref):
            assert np.array_equal(got, want) and np.asarray(got).dtype == np.asarray(want).dtype, name


def test_the_large_cloud_reaches_its_paths():
    for max_count in (0, 8):
        _check_large(max_count)
    assert int(large_ref(0).exact.sum()) % 2 == 0


def test_the_restatement_turns_down_what_the_library_turns_down():
    for bad in ((-1, 0), (0, -1), (5, 4)):
        with pytest.raises(ValueError):
            neighbours_ref.neighbours(cloud("pair"), 1.0, *bad)
    assert neighbours_ref.neighbours(cloud("pair"), 5.0, 4, 4).kept == 0  # min_neighbours == max_count is allowed


def _desc(**kw):
    d = abi.NeighboursDesc()
    d.abi_version, d.n_points, d.points, d.radius, d.min_neighbours, d.max_count = abi.ABI_VERSION, 4, 0x1000, 1.0, 2, 0
    d.grid, d.device_id, d.stream = 0, 0, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last ones for want of a device when there is
    none -- with a device they are not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(count=out, keep=out, **kw):
        return lib.gipuma_hip_cloud_neighbours(C.byref(_desc(**kw)), count, keep, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(radius=bad) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    assert rc(min_neighbours=-1) == abi.ERR_ARG and b"min_neighbours" in lib.gipuma_hip_last_error()
    assert rc(max_count=-1) == abi.ERR_ARG and b"max_count" in lib.gipuma_hip_last_error()
    assert rc(min_neighbours=5, max_count=4) == abi.ERR_ARG and b"min_neighbours" in lib.gipuma_hip_last_error()
    assert rc(points=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(count=None, keep=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(n_points=-1) == abi.ERR_ARG
    assert rc(n_points=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_neighbours(None, out, out, None, None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        for valid in (dict(), dict(count=None), dict(keep=None), dict(min_neighbours=4, max_count=4),
                      dict(n_points=0, points=None, count=None, keep=None)):
            assert rc(**valid) == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        for call in (lambda: cloud_eval.neighbour_counts(np.zeros((2, 3), f32), 1.0),
                     lambda: cloud_eval.drop_isolated(np.zeros((2, 3), f32), 1.0, 1)):
            with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
                call()
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.NeighboursDesc, "gipuma_hip_neighbours_desc",
                          ["abi_version", "n_points", "points", "radius", "min_neighbours", "max_count", "grid", "device_id", "stream"])
    assert "gipuma_hip_cloud_neighbours" in [s[0] for s in abi.SYMBOLS]


CLI = ["--cloud", "c.ply", "--reference", "r.ply"]


@pytest.mark.parametrize("argv", [CLI + ["--neighbour_radius", "1"], CLI + ["--min_neighbours", "3"],
                                  CLI + ["--neighbour_radius", "0", "--min_neighbours", "3"],
                                  CLI + ["--neighbour_radius", "-1", "--min_neighbours", "3"],
                                  CLI + ["--neighbour_radius", "nan", "--min_neighbours", "3"],
                                  CLI + ["--neighbour_radius", "inf", "--min_neighbours", "3"],
                                  CLI + ["--neighbour_radius", "1", "--min_neighbours", "-1"],
                                  CLI + ["--neighbour_radius", "1", "--min_neighbours", str(2 ** 31)],
                                  CLI + ["--neighbour_radius", "1", "--min_neighbours", "2.5"]])
def test_cli_filter_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_filter_arguments():
    a = cloud_eval.parse_args(CLI)
    assert a.neighbour_radius == 0.0 and a.min_neighbours == 0 and a.write_cloud is None
    a = cloud_eval.parse_args(CLI + ["--neighbour_radius", "0.1", "--min_neighbours", "8", "--write_cloud", "out.ply"])
    assert a.neighbour_radius == float(f32(0.1)) and a.min_neighbours == 8 and a.write_cloud == "out.ply"  # (through float32)
    a = cloud_eval.parse_args(CLI + ["--neighbour_radius", "1", "--min_neighbours", "0", "--reduce", "0.2"])
    assert a.neighbour_radius == 1.0 and a.min_neighbours == 0 and a.reduce == float(f32(0.2))
    assert cloud_eval.parse_args(CLI + ["--reduce", "0.2", "--write_cloud", "out.ply"]).write_cloud == "out.ply"


def test_batch_filter_arguments(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    a = batch.parse_args(base)
    assert a.fuse_neighbour_radius == 0.0 and a.fuse_min_neighbours == 0
    a = batch.parse_args(base + ["--fuse", "--fuse_neighbour_radius", "0.1", "--fuse_min_neighbours", "8"])
    assert a.fuse_neighbour_radius == float(f32(0.1)) and a.fuse_min_neighbours == 8
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + ["--fuse_neighbour_radius", "1", "--fuse_min_neighbours", "8"])
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    for bad in (["--fuse_neighbour_radius", "1"], ["--fuse_min_neighbours", "8"],
                ["--fuse_neighbour_radius", "-1", "--fuse_min_neighbours", "8"],
                ["--fuse_neighbour_radius", "nan", "--fuse_min_neighbours", "8"],
                ["--fuse_neighbour_radius", "1", "--fuse_min_neighbours", "-1"]):
        with pytest.raises(SystemExit) as e:
            batch.parse_args(base + ["--fuse"] + bad)
        assert e.value.code == 2
    capsys.readouterr()


def _own_vertices(n=50, seed=5):
    rng = np.random.default_rng(seed)
    v = np.zeros(n, dtype=dmb._PLY_VERTEX)
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        v[k] = rng.normal(size=n).astype(f32)
    for k in ("red", "green", "blue"):
        v[k] = rng.integers(0, 256, n)
    return v


def test_ply_round_trip_of_the_project_s_own_vertex(tmp_path):
    v = _own_vertices()
    assert v.dtype.itemsize == 27
    src, out = str(tmp_path / "fused.ply"), str(tmp_path / "out.ply")
    dmb.write_points_ply(src, v)
    got = dmb.read_ply_vertices(src)
    assert got.dtype.names == v.dtype.names and got.tobytes() == v.tobytes()
    dmb.write_ply_vertices(out, got)
    assert open(out, "rb").read() == open(src, "rb").read()  # every vertex kept: the file it came from, byte for byte
    rows = np.array([3, 4, 17, 49])
    dmb.write_ply_vertices(out, got[rows])
    assert dmb.read_ply_binary(out).tobytes() == v[rows].tobytes()
    assert np.array_equal(dmb.read_ply_xyz(out), np.stack([v["x"], v["y"], v["z"]], -1)[rows])
    dmb.write_ply_vertices(out, got[:0])
    assert len(dmb.read_ply_vertices(out)) == 0 and dmb.read_ply_vertices(out).dtype == got.dtype


def test_ply_round_trip_of_an_ascii_file_and_of_extra_properties(tmp_path):
    src, out = str(tmp_path / "a.ply"), str(tmp_path / "out.ply")
    open(src, "w").write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty double x\nproperty float y\n"
                         "property float z\nproperty uchar red\nproperty int label\nproperty short s\nelement face 1\n"
                         "property list uchar int vertex_indices\nend_header\n"
                         "0.1 2 3 255 -70000 -3\n4 5.5 6 0 8 9\n7 8 9.25 17 2147483647 32767\n3 0 1 2\n")
    v = dmb.read_ply_vertices(src)
    assert [(n, v.dtype[n].str) for n in v.dtype.names] == [("x", "<f8"), ("y", "<f4"), ("z", "<f4"), ("red", "|u1"),
                                                            ("label", "<i4"), ("s", "<i2")]
    assert v["x"].tolist() == [0.1, 4.0, 7.0] and v["label"].tolist() == [-70000, 8, 2147483647] and v["red"].tolist() == [255, 0, 17]
    assert np.array_equal(dmb.read_ply_xyz(src), np.stack([v["x"], v["y"], v["z"]], -1).astype(f32))
    dmb.write_ply_vertices(out, v[[0, 2]])  # an ascii input is written binary, the other element is not carried over
    head = open(out, "rb").read().split(b"end_header\n")[0].decode()
    assert head == ("ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty double x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty int label\nproperty short s\n")
    back = dmb.read_ply_vertices(out)
    assert back.dtype == v.dtype and back.tobytes() == v[[0, 2]].tobytes()
    assert os.path.getsize(out) == len(head) + len("end_header\n") + 2 * (8 + 4 + 4 + 1 + 4 + 2)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_a_list_property_in_vertex_is_refused(tmp_path, fmt):
    src = str(tmp_path / "l.ply")
    open(src, "wb").write(("ply\nformat %s 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                           "property list uchar int seen_by\nend_header\n" % fmt).encode() +
                          (b"1 2 3 1 7\n" if fmt == "ascii" else np.array([1, 2, 3], "<f4").tobytes() + b"\x01" + np.array([7], "<i4").tobytes()))
    with pytest.raises(ValueError, match="list property"):
        dmb.read_ply_vertices(src)
    for text in ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n4 5\n",
                 "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float x\nend_header\n1 2\n",
                 "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty uchar r\nend_header\n1 300\n"):
        open(src, "w").write(text)
        with pytest.raises(ValueError):
            dmb.read_ply_vertices(src)
    with pytest.raises(ValueError):
        dmb.write_ply_vertices(src, np.zeros((3, 3), f32))


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _assert_equals_ref(count, keep, info, r, what):
    if count is not None:
        count = count.cpu().numpy().view(np.uint32)
        assert np.array_equal(count, r.count), "%s: the counts differ at %d points" % (what, int((count != r.count).sum()))
    if keep is not None:
        keep = keep.cpu().numpy()
        assert keep.dtype == np.uint8 and np.array_equal(keep, r.keep), \
            "%s: the mask differs at %d points" % (what, int((keep != r.keep).sum()))
    assert (info["kept"], info["dropped"], info["not_finite"], info["saturated"]) == (r.kept, r.dropped, r.not_finite, r.saturated), what


GPU_RUNS = [(name, g) for name in sorted(ALL_BUILDERS) for g in ((0, 4) if name.startswith("crowded_cell") else GRIDS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_the_kernel_equals_the_restatement_in_every_bit(hip, name, grid):
    c = case(name)
    assert grid in c.grids
    c.check(c)
    what = "%s at grid %d" % (name, grid)
    count, keep, ms, info = cloud_eval.neighbours(c.points, c.radius, c.min_neighbours, c.max_count, grid=grid)
    _assert_equals_ref(count, keep, info, c.ref, what)
    ok = c.points[np.isfinite(c.points).all(axis=1)]
    if len(ok):
        assert ms > 0
        G, one_cell = scale.thin_layout(c, grid)  # the thinning's documented rule, not asked of the library
        assert info["grid"] == G, "%s: the library reports %d cells" % (what, info["grid"])
        if one_cell:
            assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)
        elif grid:
            with np.errstate(over="ignore"):
                ext = ok.max(axis=0) - ok.min(axis=0)
            assert max(info["cells_x"], info["cells_y"], info["cells_z"]) == grid
            assert all(info["cells_" + k] == 1 for k, e in zip("xyz", ext) if e == 0)  # an axis of zero extent: one cell
        if name.startswith("crowded_cell") and grid == 4:
            assert info["cells_x"] * info["cells_y"] * info["cells_z"] == 16
    else:
        assert info["grid"] == 0 and info["kept"] == 0
    if c.max_count == 0:  # the public functions: the exact counts, and the kept indices with the early stop
        got = cloud_eval.neighbour_counts(c.points, c.radius, grid=grid)
        assert got.dtype == np.uint32 and np.array_equal(got, c.ref.count), what
        idx, ms, info = cloud_eval.drop_isolated(c.points, c.radius, c.min_neighbours, grid=grid, return_info=True)
        assert idx.dtype == np.int64 and np.array_equal(idx, np.nonzero(c.ref.keep)[0]), what
        assert (info["kept"], info["dropped"], info["not_finite"]) == (c.ref.kept, c.ref.dropped, c.ref.not_finite), what


@pytest.mark.gpu
@pytest.mark.parametrize("max_count", (0, 8))
def test_large_cloud_equals_the_sparse_restatement(hip, max_count):
    _check_large(max_count)
    b = scale.large_clouds()[1]
    count, keep, ms, info = cloud_eval.neighbours(b, LARGE_RADIUS, LARGE_MIN, max_count)
    _assert_equals_ref(count, keep, info, large_ref(max_count), "300 001 points, max_count %d" % max_count)
    assert float(scale._longest_extent(b)) / LARGE_RADIUS > 256 and info["grid"] == 256  # floor(longest / radius), capped


@pytest.mark.gpu
def test_either_output_alone(hip):
    for name in ("uniform", "uniform_saturated"):
        c = case(name)
        count, keep, _, info = cloud_eval.neighbours(c.points, c.radius, c.min_neighbours, c.max_count, keep=False)
        assert keep is None
        _assert_equals_ref(count, None, info, c.ref, name + ", counts only")
        count, keep, _, info = cloud_eval.neighbours(c.points, c.radius, c.min_neighbours, c.max_count, counts=False)
        assert count is None
        _assert_equals_ref(None, keep, info, c.ref, name + ", mask only")


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_runs_repeat(hip):
    c = case("sphere_floaters")
    pts = torch.from_numpy(c.points).cuda()
    runs = []
    for _ in range(2):  # (the order inside a cell varies from run to run; a count does not)
        count, keep, ms, info = cloud_eval.neighbours(pts, c.radius, c.min_neighbours, c.max_count)
        assert count.is_cuda and keep.is_cuda
        _assert_equals_ref(count, keep, info, c.ref, "device tensor")
        runs.append(count.cpu().numpy().tobytes() + keep.cpu().numpy().tobytes())
    assert runs[0] == runs[1]
    assert np.array_equal(cloud_eval.drop_isolated(pts, c.radius, c.min_neighbours), np.nonzero(c.ref.keep)[0])


@pytest.mark.gpu
def test_counting_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the cloud was written just before, the device not synchronised: the library
    runs behind it on that stream.  Two cloud sizes one after the other on the same stream."""
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("uniform", "points_257"):
        c = case(name)
        staged = torch.from_numpy(c.points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the cloud the library reads: a device copy queued on the caller's stream
            pts = staged.clone()
            count = torch.empty(len(c.points), dtype=torch.int32, device="cuda")
            keep = torch.empty(len(c.points), dtype=torch.uint8, device="cuda")
        d = _desc(n_points=len(c.points), points=pts.data_ptr(), radius=float(c.radius), min_neighbours=c.min_neighbours,
                  max_count=c.max_count, stream=stream.cuda_stream)
        info, ms = (C.c_int64 * 8)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_neighbours(C.byref(d), count.data_ptr(), keep.data_ptr(), info, C.byref(ms)), "neighbours")
        got = dict(kept=info[0], dropped=info[1], not_finite=info[2], saturated=info[3])
        _assert_equals_ref(count, keep, got, c.ref, "%s on the caller's stream" % name)
        assert ms.value > 0
    info = (C.c_int64 * 8)(*([7] * 8))
    abi.check(lib, lib.gipuma_hip_cloud_neighbours(C.byref(_desc(n_points=0, points=None)), None, None, info, None), "nothing")
    assert list(info) == [0] * 8


@pytest.mark.gpu
def test_a_thinned_cloud_has_no_neighbours_within_the_thinning_radius(hip):
    c = case("uniform")
    idx = cloud_eval.thin(c.points, 1.5)
    assert 0 < len(idx) < len(c.points)
    counts = cloud_eval.neighbour_counts(c.points[idx], 1.5)  # kept points are pairwise d2 > r2
    assert counts.dtype == np.uint32 and len(counts) == len(idx) and not counts.any()
    assert cloud_eval.neighbour_counts(c.points[idx], 3.0).any()


@pytest.mark.gpu
def test_score_with_the_filter_is_the_score_of_the_filtered_cloud(hip):
    keys, thin_keys, times = thin_cases.SCORE_KEYS, thin_cases.NEW_KEYS, thin_cases.TIMES
    new_keys = {"neighbour_radius", "min_neighbours", "cloud_points_before_filter", "filter_device_ms"}
    rng = np.random.default_rng(17)
    cloud_pts = rng.uniform(0.0, 30.0, (4000, 3)).astype(f32)
    ref = rng.uniform(0.0, 30.0, (5000, 3)).astype(f32)
    plain = cloud_eval.score(cloud_pts, ref, max_dist=2.0)
    assert set(plain) == keys  # without the new arguments: key for key what it was
    assert set(cloud_eval.score(cloud_pts, ref, max_dist=2.0, reduce=1.0, seed=3)) == keys | thin_keys
    for reduce in (0.0, 1.0):
        idx = cloud_eval.thin(cloud_pts, reduce, seed=3) if reduce else np.arange(4000)
        kept = cloud_eval.drop_isolated(cloud_pts[idx], 2.0, 3)
        assert 0.1 * len(idx) < len(kept) < 0.9 * len(idx)
        got, indices = cloud_eval.score(cloud_pts, ref, max_dist=2.0, reduce=reduce, seed=3, neighbour_radius=2.0, min_neighbours=3,
                                        return_indices=True)
        want = cloud_eval.score(cloud_pts[idx][kept], ref, max_dist=2.0)  # the reference is never filtered
        assert set(got) == keys | new_keys | (thin_keys if reduce else set())
        for k in keys - times:
            assert got[k] == want[k], k
        assert np.array_equal(indices, idx[kept]) and indices.dtype == np.int64
        assert (got["neighbour_radius"], got["min_neighbours"], got["cloud_points_before_filter"]) == (2.0, 3, len(idx))
        assert got["cloud_points"] == len(kept) and got["reference_points"] == 5000 and got["filter_device_ms"] > 0
        if reduce:
            assert got["cloud_points_before"] == 4000 and len(got["thin_rounds"]) == 1
        assert got["accuracy"] != plain["accuracy"]


@pytest.mark.gpu
def test_the_command_line_writes_the_cloud_it_scores(hip, tmp_path, capsys):
    """--reduce, the filter and --write_cloud in one call of main(): the file holds the surviving vertices of the input,
    every property of theirs, in the input's order; the report is the API's"""
    import json
    c = case("sphere_floaters")
    v = _own_vertices(len(c.points))
    v["x"], v["y"], v["z"] = c.points[:, 0], c.points[:, 1], c.points[:, 2]
    src, ref, out, rep = (str(tmp_path / n) for n in ("cloud.ply", "ref.ply", "out.ply", "report.json"))
    dmb.write_points_ply(src, v)
    dmb.write_points_ply(ref, v[:N_SPHERE:2])
    assert cloud_eval.main(["--cloud", src, "--reference", ref, "--max_dist", "5", "--reduce", "1.5", "--seed", "3",
                            "--neighbour_radius", "6", "--min_neighbours", "4", "--write_cloud", out, "--output", rep]) == 0
    assert "dropped" in capsys.readouterr().out
    idx = cloud_eval.thin(c.points, 1.5, seed=3)
    idx = idx[cloud_eval.drop_isolated(c.points[idx], 6.0, 4)]
    assert 1000 < len(idx) < N_SPHERE and idx.max() < N_SPHERE  # thinned, and no floater is left
    assert dmb.read_ply_binary(out).tobytes() == v[idx].tobytes()
    report = json.load(open(rep))
    assert report["cloud_points"] == len(idx) and report["cloud_points_before"] == len(v) and report["min_neighbours"] == 4
    assert report["cloud_points_before_filter"] == len(cloud_eval.thin(c.points, 1.5, seed=3))
    # without the filter and the thinning the file is the input's vertices, all of them
    assert cloud_eval.main(["--cloud", src, "--reference", ref, "--write_cloud", out]) == 0
    assert open(out, "rb").read() == open(src, "rb").read()
    capsys.readouterr()
