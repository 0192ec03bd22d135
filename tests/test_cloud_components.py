"""The connected components of a cloud's radius graph and dropping its small clumps (DESIGN.md 18,
gipuma_hip_cloud_components, gipuma_amd.cloud_eval.component_labels / drop_small_components).  Every case is a cloud, a
radius, a min_size and a condition -- stated on the restatement (tests/components_ref.py) alone -- that it reaches the path
it is named for; that condition runs without a device, and so do the comparison of the restatement's forms (the brute
force, the k-d tree's pairs, scipy's csgraph), the C-ABI's argument checks, the command lines and the unit's assembly.
GPU: label as int32, size as uint32, the mask as bytes and the four info counts equal the restatement at every grid; any
subset of the outputs; the descriptor's stream; device tensors; three runs; the score, the command line and the batch with
the filter."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
# torch before the `hip` fixture loads the library (see tests/test_cloud_scale.py): this module must also run on its own
import torch  # noqa: F401

from gipuma_amd import abi, cloud_eval, dmb
from tests import components_ref, knn_ref, neighbours_ref
from tests import test_cloud_neighbours as neighbour_cases
from tests import test_cloud_scale as scale
from tests import test_cloud_thin as thin_cases
from tests.abi_layout import assert_mirrors_header

f32 = np.float32
GRIDS = thin_cases.GRIDS
assert GRIDS == (0, 1, 2, 7, 256)
N_SPHERE = neighbour_cases.N_SPHERE
N_CLUMP = 40
CLUMP_AT = np.array([10.0, 5.0, -20.0])  # inside the sphere of radius 50: about 27 from its surface
SPHERE_RADIUS = 5.0  # the sphere's mean spacing is 2.3: at 5 its 6 000 points are one component (asserted)


# ----------------------------------------------------------------------------------------------------------------------
# The clouds
# ----------------------------------------------------------------------------------------------------------------------
def _sphere_floaters_clump():
    """DESIGN.md 16's cloud -- the noisy sphere, 54 single floaters, three clumps of three -- and then one tight clump of
    40 points within 0.5 of each other"""
    clump = CLUMP_AT + np.random.default_rng(40).uniform(-0.25, 0.25, (N_CLUMP, 3))
    return np.concatenate([neighbour_cases._sphere_with_floaters(), clump])


def _chain(n, order):
    """n collinear points at spacing 1 (d2 == r2 exactly at radius 1), stored in `order`"""
    x = np.zeros((n, 3))
    x[:, 0] = np.arange(n)
    if order == "descending":
        x = x[::-1]
    elif order == "shuffled":  # index 0 holds the middle of the line
        perm = np.random.default_rng(11).permutation(n)
        perm[np.nonzero(perm == n // 2)[0][0]], perm[0] = perm[0], n // 2
        x = x[perm]
    return x


def _chain_with_gap():
    """the shuffled chain with every point from 1024 on moved by 2^-13, one rounding step there and exact for all of them:
    the one gap 1023 -> nextafter(1024) is wider than the radius, every other stays 1"""
    x = _chain(2000, "shuffled").astype(f32)
    x[x[:, 0] >= 1024, 0] += f32(2.0 ** -13)
    return x


def _spirals(n=5000, turns=140, radius=0.9, pitch=2.2):
    """two interleaved helices around one axis, half a turn apart: at the same place of the circle they are half a pitch --
    1.1 -- apart along the axis, across it 1.8.  The automatic grid at radius 1 is capped at 256 cells of edge 1.2 along the
    axis, 2 x 2 across: a layer holds more than half a turn of either helix, so the two pass through all four of its cells."""
    t = np.linspace(0.0, 2.0 * np.pi * turns, n)
    z = t * (pitch / (2.0 * np.pi))
    a = np.stack([radius * np.cos(t), radius * np.sin(t), z], -1)
    b = np.stack([radius * np.cos(t + np.pi), radius * np.sin(t + np.pi), z], -1)
    out = np.empty((2 * n, 3))
    out[0::2], out[1::2] = a, b
    return out


def _bridge():
    """two clumps 1.6 apart and, exactly between them, a point that is not finite in one coordinate"""
    rng = np.random.default_rng(5)
    left, right = rng.uniform(-0.3, 0.3, (20, 3)), rng.uniform(-0.3, 0.3, (20, 3)) + [2.2, 0.0, 0.0]
    return np.concatenate([left, [[1.1, np.nan, 0.0]], right, [[1.1, 0.0, np.inf]]])


CLOUDS = {
    "sphere_floaters_clump": _sphere_floaters_clump,
    "pair": lambda: [[0, 0, 0], [3, 4, 0]],
    "chain_shuffled": lambda: _chain(2000, "shuffled"),
    "chain_gap": _chain_with_gap,
    "chain_ascending": lambda: _chain(100000, "ascending"),
    "chain_descending": lambda: _chain(100000, "descending"),
    "spirals": _spirals,
    "identical": lambda: thin_cases.case("identical").points,
    "crowded_cell": lambda: thin_cases.case("crowded_cell").points,
    **{"points_%d" % n: functools.partial(lambda n: thin_cases.case("points_%d" % n).points, n) for n in (0, 1, 63, 64, 65, 257)},
    "lattice_twice": thin_cases._lattice_twice,
    "non_finite": lambda: thin_cases.case("non_finite").points,
    "non_finite_moved": lambda: neighbour_cases.cloud("non_finite_moved"),
    "bridge": _bridge,
    "flat_coplanar": lambda: thin_cases.case("flat_coplanar").points,
    "uniform": thin_cases._uniform,
    "large_coordinates": lambda: thin_cases.case("large_coordinates").points,
    **{"scale_" + name: functools.partial(lambda name: scale.thin_case(name).points, name) for name in scale.THIN_BUILDERS},
}
SPARSE_ONLY = ("chain_ascending", "chain_descending", "crowded_cell")  # too many pairs for the brute force to be quick


@functools.lru_cache(maxsize=None)
def cloud(name):
    return np.ascontiguousarray(CLOUDS[name](), dtype=f32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def edges(name, radius):
    """a cloud's edge list at a radius, computed once for every case that shares it: the brute force's, or -- for the three
    clouds named above -- the k-d tree's, which test_the_sparse_restatement_... proves equal on every other case"""
    e = components_ref.sparse_edges(cloud(name), radius) if name in SPARSE_ONLY else components_ref.edges(cloud(name), radius)
    assert e is not None, name
    for a in e:
        a.setflags(write=False)
    return e


class Case:
    def __init__(self, name, radius, min_size, check, grids=GRIDS):
        self.name, self.radius, self.min_size, self.check, self.grids = name, f32(radius), min_size, check, grids

    @property
    def points(self):
        return cloud(self.name)

    @functools.cached_property
    def ref(self):
        return components_ref.from_edges(self.points, *edges(self.name, self.radius), self.min_size)


def _sizes(r):
    """the sizes of the components, descending"""
    return sorted((int(s) for s in r.size[(r.label == np.arange(len(r.label)))]), reverse=True)


def _case_motivating():
    def check(c):
        p, r = c.points, c.ref
        clump = np.arange(len(p) - N_CLUMP, len(p))
        others = np.arange(N_SPHERE, len(p) - N_CLUMP)
        assert len(others) == 63 and np.linalg.norm(CLUMP_AT) <= 50.0 - 8.0
        # the neighbour count of DESIGN.md 16 keeps the clump: 39 neighbours each
        n = neighbours_ref.neighbours(p, 6.0, 6)
        assert (n.exact[clump] == N_CLUMP - 1).all() and n.keep[clump].all() and not n.keep[others].any()
        # so does the statistical filter of DESIGN.md 17 (k = 8 within 6, two standard deviations): the clump's members are
        # closer to each other than the sphere's, their mean distance is below the cloud's mean
        k = knn_ref.knn(p, 6.0, 8)
        keep, mu, _, _ = cloud_eval.outlier_threshold(k.mean, 2.0)
        assert keep[clump].all() and (k.mean[clump] < mu).all() and keep[:N_SPHERE].sum() >= 0.9 * N_SPHERE
        # the components: the sphere is one, and min_size 100 drops the 40 + 63 and nothing else
        assert (r.label[:N_SPHERE] == 0).all() and (r.size[:N_SPHERE] == N_SPHERE).all()
        assert (r.label[clump] == clump[0]).all() and (r.size[clump] == N_CLUMP).all()
        assert _sizes(r) == [N_SPHERE, N_CLUMP] + [3] * 3 + [1] * 54
        assert np.array_equal(np.nonzero(r.keep)[0], np.arange(N_SPHERE)) and (r.kept, r.dropped) == (N_SPHERE, N_CLUMP + 63)
    return Case("sphere_floaters_clump", SPHERE_RADIUS, 100, check)


def _case_pair(inside):
    def check(c):
        assert c.ref.label.tolist() == ([0, 0] if inside else [0, 1]) and c.ref.components == (1 if inside else 2)
    return Case("pair", f32(5) if inside else np.nextafter(f32(5), f32(0)), 2, check)


def _case_chain(name, n):
    def check(c):
        r = c.ref
        assert (r.label == 0).all() and (r.size == n).all() and r.components == 1
        if name == "chain_shuffled":
            assert c.points[0, 0] == n // 2 and not (np.diff(c.points[:, 0]) == 1).all()
        assert components_ref.squared(c.radius) == 1.0  # d2 == r2 exactly between two neighbours of the line
    return Case(name, 1.0, n, check)


def _case_chain_gap():
    def check(c):
        r, x = c.ref, c.points[:, 0]
        assert np.sort(x)[1024] == np.nextafter(f32(1024), f32(2048)) and (np.diff(np.sort(x.astype(np.float64))) == 1).sum() == 1998
        assert r.components == 2 and _sizes(r) == [1024, 976] and (r.label[x < 1024] == 0).all()
        assert (r.label[x >= 1024] == np.nonzero(x >= 1024)[0][0]).all()
    return Case("chain_gap", 1.0, 0, check)


def _case_spirals():
    def check(c):
        r, p = c.ref, c.points
        assert r.components == 2 and (r.label[0::2] == 0).all() and (r.label[1::2] == 1).all() and (r.size == 5000).all()
        G, one = scale.thin_layout(c, 0)  # the automatic grid: every cell of it holds a point of either spiral
        assert not one and G == 256
        lo, ext = p.min(axis=0).astype(np.float64), (p.max(axis=0) - p.min(axis=0)).astype(np.float64)
        h = ext.max() / G
        cells = np.minimum(np.floor(ext / h).astype(int) + 1, G)
        hit = {tuple(v) for v in np.minimum(np.floor((p - lo) / h).astype(int), cells - 1)}
        assert len(hit) == int(np.prod(cells)) == 4 * 256, (len(hit), cells)
    return Case("spirals", 1.0, 0, check)


def _case_identical():
    def check(c):
        assert (c.ref.label == 0).all() and (c.ref.size == 500).all() and c.ref.components == 1
    return Case("identical", 1.0, 500, check)


def _case_crowded(joined):
    def check(c):
        thin_cases.case("crowded_cell").check(thin_cases.case("crowded_cell"))  # 20 000 points in one of 16 cells
        r = c.ref
        assert (r.size[20000:] == 1).all()
        if joined:  # every lane hooks into one tree
            assert (r.label[:20000] == 0).all() and (r.size[:20000] == 20000).all() and r.components == 3
        else:
            assert r.components >= 5000 and _sizes(r)[0] >= 5 and r.kept >= 2000 and r.dropped >= 2000, (r.components, r.kept)
    return Case("crowded_cell", 1e-3 if joined else 2e-4, 2, check, grids=(0, 4))


def _case_count(n):
    def check(c):
        assert len(c.points) == n and sum(_sizes(c.ref)) == n and c.ref.kept + c.ref.dropped == n
        if n >= 63:
            assert 1 < c.ref.components < n and 0 < c.ref.kept and 0 < c.ref.dropped
    return Case("points_%d" % n, 0.5, 3, check)


def _case_lattice(which):
    def check(c):
        r = c.ref
        if which == "copies":  # a site and its copy, 0 apart; two sites are 1 apart
            assert r.components == 512 and (r.size == 2).all() and np.array_equal(r.label, np.tile(np.arange(512), 2))
        else:  # d2 == r2 exactly between adjacent sites
            assert r.components == 1 and (r.size == 1024).all() and not r.label.any()
    return Case("lattice_twice", 0.5 if which == "copies" else 1.0, 2, check)


def _case_non_finite():
    def check(c):
        r, p = c.ref, c.points
        bad = ~np.isfinite(p).all(axis=1)
        assert bad.sum() == 30 == r.not_finite and (r.label[bad] == -1).all() and not r.size[bad].any() and not r.keep[bad].any()
        assert c.min_size == 0 and np.array_equal(r.keep, (~bad).astype(np.uint8)) and r.dropped == 0  # never kept, even at 0
        # never joining: the finite points' components are those of the cloud with the others moved far away
        moved = components_ref.from_edges(cloud("non_finite_moved"), *edges("non_finite_moved", c.radius), 0)
        assert np.array_equal(moved.label[~bad], r.label[~bad]) and np.array_equal(moved.size[~bad], r.size[~bad])
        assert 1 < r.components < (~bad).sum() and _sizes(r)[0] >= 5
    return Case("non_finite", 1.5, 0, check)


def _case_bridge():
    def check(c):
        r = c.ref
        assert r.not_finite == 2 and r.components == 2 and _sizes(r) == [20, 20]
        assert (r.label[:20] == 0).all() and (r.label[21:41] == 21).all() and r.label[20] == r.label[41] == -1
        # a finite point in the same place WOULD join them
        p = c.points.copy()
        p[20] = [1.1, 0.0, 0.0]
        assert components_ref.components(p, c.radius).components == 1
    return Case("bridge", 1.0, 0, check)


def _case_coplanar():
    def check(c):
        ext = c.points.max(axis=0) - c.points.min(axis=0)
        assert (ext == 0).sum() == 1 and 1 < c.ref.components < 2000 and _sizes(c.ref)[0] >= 10  # an axis of zero extent: one cell
    return Case("flat_coplanar", 0.15, 4, check)


UNIFORM_LARGEST = 2887  # (asserted below)


def _case_uniform(min_size):
    def check(c):
        r, s = c.ref, _sizes(c.ref)
        assert s[0] == UNIFORM_LARGEST and s[-1] == 1 and len(set(s)) >= 8 and r.components == len(s) >= 50  # mixed sizes
        assert r.kept == sum(v for v in s if v >= min_size) and r.kept + r.dropped == 3000
        assert (r.kept == 0) == (min_size > UNIFORM_LARGEST) and (r.dropped == 0) == (min_size <= 1)
    return Case("uniform", 1.5, min_size, check)


def _case_large_coordinates():
    def check(c):
        assert np.spacing(f32(65536.0)) > 0.25 * c.radius  # a coordinate's own rounding step is a quarter of the radius
        assert 1 < c.ref.components and _sizes(c.ref)[0] >= 50 and c.ref.kept > 0 and c.ref.dropped > 0, _sizes(c.ref)[:3]
    return Case("large_coordinates", 0.03, 10, check)


def _case_scale(name):
    """the thinning's extreme scales (tests/test_cloud_scale.py): its clouds, its radii and its expectation of one cell"""
    t = scale.thin_case(name)

    def check(c):
        t.check(t)
        r, n = c.ref, len(c.points)
        assert tuple(g for g in GRIDS if scale.thin_layout(c, g)[1]) == tuple(t.one_cell)
        if name == "r2_infinite":  # inf <= inf: one component holding every finite point, the two at +-3e38 included
            assert np.isposinf(components_ref.squared(c.radius)) and r.components == 1 and (r.size == n).all()
        elif name == "r2_zero":  # only the exact copy is within a radius whose square is 0
            assert components_ref.squared(c.radius) == 0 and r.components == 512 and (r.size == 2).all()
        else:
            assert 1 <= r.components < n and _sizes(r)[0] >= 5
    return Case("scale_" + name, t.radius, 2, check)


BUILDERS = {
    "motivating": _case_motivating,
    "radius_inclusive": lambda: _case_pair(True),
    "radius_just_short": lambda: _case_pair(False),
    "chain_shuffled": lambda: _case_chain("chain_shuffled", 2000),
    "chain_gap": _case_chain_gap,
    "chain_ascending": lambda: _case_chain("chain_ascending", 100000),
    "chain_descending": lambda: _case_chain("chain_descending", 100000),
    "spirals": _case_spirals,
    "identical": _case_identical,
    "crowded_joined": lambda: _case_crowded(True),
    "crowded_many": lambda: _case_crowded(False),
    **{"points_%d" % n: functools.partial(_case_count, n) for n in (0, 1, 63, 64, 65, 257)},
    "lattice_copies": lambda: _case_lattice("copies"),
    "lattice_inclusive": lambda: _case_lattice("inclusive"),
    "non_finite": _case_non_finite,
    "bridge": _case_bridge,
    "flat_coplanar": _case_coplanar,
    **{"uniform_min%d" % m: functools.partial(_case_uniform, m) for m in (1, 2, 5, UNIFORM_LARGEST + 1)},
    "large_coordinates": _case_large_coordinates,
}
SCALE_BUILDERS = {"scale_" + name: functools.partial(_case_scale, name) for name in scale.THIN_BUILDERS}
ALL_BUILDERS = {**BUILDERS, **SCALE_BUILDERS}


@functools.lru_cache(maxsize=None)
def case(name):
    return ALL_BUILDERS[name]()


LARGE_RADIUS, LARGE_MIN = 0.3, 3


@functools.lru_cache(maxsize=None)
def large_ref():
    return components_ref.components_sparse(scale.large_clouds()[1], LARGE_RADIUS, LARGE_MIN)


def _check_properties(r, n):
    """what holds of every result: label <= index and idempotent, size constant on a component, the sizes sum up"""
    ok = r.label >= 0
    i = np.arange(n)
    assert r.label.dtype == np.int32 and r.size.dtype == np.uint32 and r.keep.dtype == np.uint8
    assert len(r.label) == len(r.size) == len(r.keep) == n
    assert (r.label[ok] <= i[ok]).all() and np.array_equal(r.label[r.label[ok]], r.label[ok])
    assert np.array_equal(r.size[r.label[ok]], r.size[ok]) and not r.size[~ok].any() and (r.size[ok] >= 1).all()
    roots = ok & (r.label == i)
    assert int(r.size[roots].astype(np.int64).sum()) == int(ok.sum()) and int(roots.sum()) == r.components
    assert r.kept + r.dropped + r.not_finite == n and r.kept == int(r.keep.sum()) and r.not_finite == int((~ok).sum())


def _check_large():
    r = large_ref()
    assert r is not None and r.not_finite == 0
    _check_properties(r, scale.N_LARGE)
    assert r.kept >= 0.1 * scale.N_LARGE and r.dropped >= 0.1 * scale.N_LARGE and r.components >= 10000, (r.kept, r.dropped)
    assert (r.size[list(scale.OUTLIERS)] == 1).all()  # (nothing within 10 of them)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    _check_properties(c.ref, len(c.points))


def test_the_sparse_restatement_and_csgraph_equal_the_brute_force_on_every_small_case():
    """(the extreme scales are not of the ordinary magnitudes the sparse form's argument needs: they are judged against
    the brute force alone; the three clouds the brute force is too slow for are judged by the sparse form, proven here)"""
    for name in sorted(BUILDERS):
        c = case(name)
        if c.name in SPARSE_ONLY:
            continue
        s = components_ref.components_sparse(c.points, c.radius, c.min_size)
        assert s is not None, name
        for got, want in zip(s, c.ref):
            assert np.array_equal(got, want) and np.asarray(got).dtype == np.asarray(want).dtype, name
    for name in sorted(ALL_BUILDERS):
        c = case(name)
        second = components_ref.csgraph_labels(c.points, *edges(c.name, c.radius))
        assert second is None or np.array_equal(second, c.ref.label), name


def test_the_large_cloud_reaches_its_paths():
    _check_large()
    second = components_ref.csgraph_labels(scale.large_clouds()[1], *components_ref.sparse_edges(scale.large_clouds()[1], LARGE_RADIUS))
    assert second is None or np.array_equal(second, large_ref().label)


def test_the_restatement_turns_down_what_the_library_turns_down():
    with pytest.raises(ValueError):
        components_ref.components(cloud("pair"), 1.0, -1)


def _desc(**kw):
    d = abi.ComponentsDesc()
    d.abi_version, d.n_points, d.points, d.radius, d.min_size = abi.ABI_VERSION, 4, 0x1000, 1.0, 2
    d.grid, d.device_id, d.stream = 0, 0, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last ones for want of a device when there is
    none -- with a device they are not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(label=out, size=out, keep=out, **kw):
        return lib.gipuma_hip_cloud_components(C.byref(_desc(**kw)), label, size, keep, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(radius=bad) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    assert rc(min_size=-1) == abi.ERR_ARG and b"min_size" in lib.gipuma_hip_last_error()
    assert rc(min_size=-1, radius=0.0) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()  # (the thinning's order)
    assert rc(min_size=-1, grid=300) == abi.ERR_ARG and b"min_size" in lib.gipuma_hip_last_error()
    assert rc(points=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(label=None, size=None, keep=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(n_points=-1) == abi.ERR_ARG
    assert rc(n_points=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_components(None, out, out, out, None, None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        for valid in (dict(), dict(label=None), dict(size=None, keep=None), dict(label=None, size=None), dict(min_size=0),
                      dict(n_points=0, points=None, label=None, size=None, keep=None)):
            assert rc(**valid) == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        for call in (lambda: cloud_eval.component_labels(np.zeros((2, 3), f32), 1.0),
                     lambda: cloud_eval.drop_small_components(np.zeros((2, 3), f32), 1.0, 1),
                     lambda: cloud_eval.components(np.zeros((2, 3), f32), 1.0)):
            with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
                call()
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.ComponentsDesc, "gipuma_hip_components_desc",
                          ["abi_version", "n_points", "points", "radius", "min_size", "grid", "device_id", "stream"])
    assert "gipuma_hip_cloud_components" in [s[0] for s in abi.SYMBOLS]


CLI = ["--cloud", "c.ply", "--reference", "r.ply"]


@pytest.mark.parametrize("argv", [CLI + ["--component_radius", "1"], CLI + ["--min_component", "3"],
                                  CLI + ["--component_radius", "0", "--min_component", "3"],
                                  CLI + ["--component_radius", "-1", "--min_component", "3"],
                                  CLI + ["--component_radius", "nan", "--min_component", "3"],
                                  CLI + ["--component_radius", "inf", "--min_component", "3"],
                                  CLI + ["--component_radius", "1", "--min_component", "-1"],
                                  CLI + ["--component_radius", "1", "--min_component", str(2 ** 31)],
                                  CLI + ["--component_radius", "1", "--min_component", "2.5"]])
def test_cli_component_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_component_arguments():
    a = cloud_eval.parse_args(CLI)
    assert a.component_radius == 0.0 and a.min_component == 0
    a = cloud_eval.parse_args(CLI + ["--component_radius", "0.1", "--min_component", "100", "--write_cloud", "out.ply"])
    assert a.component_radius == float(f32(0.1)) and a.min_component == 100 and a.write_cloud == "out.ply"  # (through float32)
    a = cloud_eval.parse_args(CLI + ["--component_radius", "1", "--min_component", "0", "--reduce", "0.2", "--neighbour_radius", "1",
                                     "--min_neighbours", "2", "--outlier_radius", "1", "--outlier_k", "4", "--outlier_std", "2"])
    assert (a.component_radius, a.min_component, a.neighbour_radius, a.outlier_k) == (1.0, 0, 1.0, 4)


def test_batch_component_arguments(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    on = ["--fuse_component_radius", "0.1", "--fuse_min_component", "8"]
    a = batch.parse_args(base)
    assert a.fuse_component_radius == 0.0 and a.fuse_min_component == 0
    a = batch.parse_args(base + ["--fuse"] + on)
    assert a.fuse_component_radius == float(f32(0.1)) and a.fuse_min_component == 8
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + on)
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    for bad in (on[:2], on[2:], ["--fuse_component_radius", "-1"] + on[2:], ["--fuse_component_radius", "nan"] + on[2:],
                on[:2] + ["--fuse_min_component", "-1"], on[:2] + ["--fuse_min_component", str(2 ** 31)]):
        with pytest.raises(SystemExit) as e:
            batch.parse_args(base + ["--fuse"] + bad)
        assert e.value.code == 2
    capsys.readouterr()


def test_score_turns_down_bad_component_arguments_before_anything_runs():
    a = np.zeros((2, 3), f32)
    for bad in (dict(component_radius=-1.0), dict(component_radius=float("nan")), dict(component_radius=1.0, min_component=-1),
                dict(component_radius=1.0, min_component=2.5)):
        with pytest.raises(ValueError):
            cloud_eval.score(a, a, **bad)


def test_the_kernels_use_global_memory_instructions_integer_atomics_and_no_contraction():
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "c.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--offload-device-only", "-o", out, "gipuma_components.hip"],
                              cwd=os.path.join(root, "gipuma_amd", "csrc"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    for k in ("init_kernel", "hook_kernel", "flatten_kernel", "write_kernel"):
        assert "_ZN4comp%d%s" % (len(k), k) in asm
    assert "_ZN5cloud" not in asm.replace("N5cloud3RecE", "").replace("NS0_4GridE", "")  # the set-up kernels are defined once, elsewhere
    ops = [l.split()[0] for l in asm.splitlines() if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")]
    assert not [o for o in ops if o.startswith("v_fma") or o.startswith("v_mad_f32") or o.startswith("v_fmac")]  # no contraction
    atomics = {o for o in ops if "atomic" in o}
    assert atomics <= {"global_atomic_add", "global_atomic_cmpswap", "global_atomic_smin", "global_atomic_umin"}, atomics
    assert "global_atomic_cmpswap" in atomics and atomics & {"global_atomic_smin", "global_atomic_umin"}


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _assert_equals_ref(label, size, keep, info, r, what):
    if label is not None:
        label = label.cpu().numpy()
        assert label.dtype == np.int32 and np.array_equal(label, r.label), \
            "%s: the labels differ at %d points" % (what, int((label != r.label).sum()))
    if size is not None:
        size = size.cpu().numpy().view(np.uint32)
        assert np.array_equal(size, r.size), "%s: the sizes differ at %d points" % (what, int((size != r.size).sum()))
    if keep is not None:
        keep = keep.cpu().numpy()
        assert keep.dtype == np.uint8 and np.array_equal(keep, r.keep), \
            "%s: the mask differs at %d points" % (what, int((keep != r.keep).sum()))
    assert (info["kept"], info["dropped"], info["not_finite"], info["components"]) == (r.kept, r.dropped, r.not_finite, r.components), what


GPU_RUNS = [(name, g) for name in sorted(ALL_BUILDERS) for g in ((0, 4) if name.startswith("crowded") else GRIDS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_the_kernels_equal_the_restatement_in_every_byte(hip, name, grid):
    c = case(name)
    assert grid in c.grids
    c.check(c)
    what = "%s at grid %d" % (name, grid)
    label, size, keep, ms, info = cloud_eval.components(c.points, c.radius, c.min_size, grid=grid)
    _assert_equals_ref(label, size, keep, info, c.ref, what)
    ok = c.points[np.isfinite(c.points).all(axis=1)]
    if len(c.points):
        assert ms > 0
    if len(ok):
        G, one_cell = scale.thin_layout(c, grid)  # the thinning's documented rule, not asked of the library
        assert info["grid"] == G, "%s: the library reports %d cells" % (what, info["grid"])
        if one_cell:
            assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)
        elif grid:
            with np.errstate(over="ignore"):
                ext = ok.max(axis=0) - ok.min(axis=0)
            assert max(info["cells_x"], info["cells_y"], info["cells_z"]) == grid
            assert all(info["cells_" + k] == 1 for k, e in zip("xyz", ext) if e == 0)  # an axis of zero extent: one cell
        if name.startswith("crowded") and grid == 4:
            assert info["cells_x"] * info["cells_y"] * info["cells_z"] == 16
    else:
        assert info["grid"] == 0 and info["kept"] == 0 and info["components"] == 0
    if grid == 0:  # the public functions
        got = cloud_eval.component_labels(c.points, c.radius)
        assert got[0].dtype == np.int32 and got[1].dtype == np.uint32
        assert np.array_equal(got[0], c.ref.label) and np.array_equal(got[1], c.ref.size), what
        idx, ms, info = cloud_eval.drop_small_components(c.points, c.radius, c.min_size, return_info=True)
        assert idx.dtype == np.int64 and np.array_equal(idx, np.nonzero(c.ref.keep)[0]), what
        assert (info["kept"], info["dropped"], info["components"]) == (c.ref.kept, c.ref.dropped, c.ref.components), what


@pytest.mark.gpu
def test_large_cloud_equals_the_sparse_restatement(hip):
    _check_large()
    b = scale.large_clouds()[1]
    label, size, keep, ms, info = cloud_eval.components(b, LARGE_RADIUS, LARGE_MIN)
    _assert_equals_ref(label, size, keep, info, large_ref(), "300 001 points")
    assert float(scale._longest_extent(b)) / LARGE_RADIUS > 256 and info["grid"] == 256  # floor(longest / radius), capped


@pytest.mark.gpu
def test_any_subset_of_the_outputs_alone(hip):
    c = case("uniform_min5")
    for mask in range(1, 8):
        on = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
        label, size, keep, _, info = cloud_eval.components(c.points, c.radius, c.min_size, label=on[0], size=on[1], keep=on[2])
        assert [t is not None for t in (label, size, keep)] == on
        _assert_equals_ref(label, size, keep, info, c.ref, "outputs %s" % on)


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_three_runs_give_the_same_bytes(hip):
    for name in ("motivating", "crowded_many"):
        c = case(name)
        pts = torch.from_numpy(c.points).cuda()
        runs = []
        for _ in range(3):  # (the order inside a cell and the unions' interleaving vary from run to run; the result does not)
            label, size, keep, ms, info = cloud_eval.components(pts, c.radius, c.min_size)
            assert label.is_cuda and size.is_cuda and keep.is_cuda
            _assert_equals_ref(label, size, keep, info, c.ref, name + ", device tensor")
            runs.append(label.cpu().numpy().tobytes() + size.cpu().numpy().tobytes() + keep.cpu().numpy().tobytes())
        assert runs[0] == runs[1] == runs[2]
        assert np.array_equal(cloud_eval.drop_small_components(pts, c.radius, c.min_size), np.nonzero(c.ref.keep)[0])


@pytest.mark.gpu
def test_components_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the cloud was written just before, the device not synchronised: the library
    runs behind it on that stream.  Two cloud sizes one after the other on the same stream, then n = 0."""
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("uniform_min2", "points_257"):
        c = case(name)
        staged = torch.from_numpy(c.points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the cloud the library reads: a device copy queued on the caller's stream
            pts = staged.clone()
            label = torch.empty(len(c.points), dtype=torch.int32, device="cuda")
            size = torch.empty(len(c.points), dtype=torch.int32, device="cuda")
            keep = torch.empty(len(c.points), dtype=torch.uint8, device="cuda")
        d = _desc(n_points=len(c.points), points=pts.data_ptr(), radius=float(c.radius), min_size=c.min_size, stream=stream.cuda_stream)
        info, ms = (C.c_int64 * 8)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_components(C.byref(d), label.data_ptr(), size.data_ptr(), keep.data_ptr(), info, C.byref(ms)),
                  "components")
        got = dict(kept=info[0], dropped=info[1], not_finite=info[2], components=info[3])
        _assert_equals_ref(label, size, keep, got, c.ref, "%s on the caller's stream" % name)
        assert ms.value > 0
    info = (C.c_int64 * 8)(*([7] * 8))
    abi.check(lib, lib.gipuma_hip_cloud_components(C.byref(_desc(n_points=0, points=None)), None, None, None, info, None), "nothing")
    assert list(info) == [0] * 8


@pytest.mark.gpu
def test_a_thinned_cloud_is_all_components_of_one_at_the_thinning_radius(hip):
    c = case("uniform_min1")
    idx = cloud_eval.thin(c.points, 1.5)
    assert 0 < len(idx) < len(c.points)
    label, size = cloud_eval.component_labels(c.points[idx], 1.5)  # kept points are pairwise d2 > r2
    assert np.array_equal(label, np.arange(len(idx))) and (size == 1).all()
    assert cloud_eval.component_labels(c.points[idx], 3.0)[1].max() > 1


@pytest.mark.gpu
def test_the_filters_before_it_keep_the_clump_and_the_component_filter_drops_it(hip):
    c = case("motivating")
    p, clump = c.points, np.arange(len(c.points) - N_CLUMP, len(c.points))
    assert np.isin(clump, cloud_eval.drop_isolated(p, 6.0, 6)).all()
    assert np.isin(clump, cloud_eval.drop_outliers(p, 6.0, 8, 2.0)).all()
    assert np.array_equal(cloud_eval.drop_small_components(p, SPHERE_RADIUS, 100), np.arange(N_SPHERE))


@pytest.mark.gpu
def test_score_with_the_filter_is_the_score_of_the_filtered_cloud(hip):
    keys, thin_keys, times = thin_cases.SCORE_KEYS, thin_cases.NEW_KEYS, thin_cases.TIMES
    new_keys = {"component_radius", "min_component", "components", "cloud_points_before_components", "component_device_ms"}
    earlier = {"neighbour_radius", "min_neighbours", "cloud_points_before_filter", "filter_device_ms", "outlier_radius", "outlier_k",
               "outlier_std", "outlier_threshold", "cloud_points_before_outliers", "outlier_device_ms"}
    rng = np.random.default_rng(17)
    cloud_pts = rng.uniform(0.0, 30.0, (4000, 3)).astype(f32)
    ref = rng.uniform(0.0, 30.0, (5000, 3)).astype(f32)
    plain = cloud_eval.score(cloud_pts, ref, max_dist=2.0)
    assert set(plain) == keys  # without the new arguments: key for key what it was
    # the component filter alone
    kept = cloud_eval.drop_small_components(cloud_pts, 1.5, 4)
    assert 0.1 * 4000 < len(kept) < 0.9 * 4000
    got, indices = cloud_eval.score(cloud_pts, ref, max_dist=2.0, component_radius=1.5, min_component=4, return_indices=True)
    want = cloud_eval.score(cloud_pts[kept], ref, max_dist=2.0)
    assert set(got) == keys | new_keys and np.array_equal(indices, kept)
    for k in keys - times:
        assert got[k] == want[k], k
    # all four stages, composed by hand
    idx = cloud_eval.thin(cloud_pts, 1.0, seed=3)
    idx = idx[cloud_eval.drop_isolated(cloud_pts[idx], 2.0, 2)]
    before_outliers = len(idx)
    idx = idx[cloud_eval.drop_outliers(cloud_pts[idx], 2.5, 3, 1.0)]
    before = len(idx)
    labels, _, _, info = cloud_eval.component_labels(cloud_pts[idx], 1.6, return_info=True)
    idx = idx[cloud_eval.drop_small_components(cloud_pts[idx], 1.6, 6)]
    assert 0.1 * before < len(idx) < 0.9 * before < 0.9 * before_outliers
    got, indices = cloud_eval.score(cloud_pts, ref, max_dist=2.0, reduce=1.0, seed=3, neighbour_radius=2.0, min_neighbours=2,
                                    outlier_radius=2.5, outlier_k=3, outlier_std=1.0, component_radius=1.6, min_component=6,
                                    return_indices=True)
    want = cloud_eval.score(cloud_pts[idx], ref, max_dist=2.0)  # the reference is never filtered
    assert set(got) == keys | thin_keys | earlier | new_keys
    for k in keys - times:
        assert got[k] == want[k], k
    assert np.array_equal(indices, idx) and indices.dtype == np.int64
    assert (got["component_radius"], got["min_component"], got["cloud_points_before_components"]) == (float(f32(1.6)), 6, before) or \
        (got["component_radius"], got["min_component"], got["cloud_points_before_components"]) == (1.6, 6, before)
    assert got["components"] == info["components"] == len(np.unique(labels)) and got["component_device_ms"] > 0
    assert got["cloud_points"] == len(idx) and got["cloud_points_before_outliers"] == before_outliers


@pytest.mark.gpu
def test_the_command_line_writes_the_cloud_it_scores(hip, tmp_path, capsys):
    """--reduce, the neighbour filter, the component filter and --write_cloud in one call of main(): the file holds the
    surviving vertices of the input, every property of theirs, in the input's order; the summary's figures chain up"""
    c = case("motivating")
    v = neighbour_cases._own_vertices(len(c.points))
    v["x"], v["y"], v["z"] = c.points[:, 0], c.points[:, 1], c.points[:, 2]
    src, ref, out, rep = (str(tmp_path / n) for n in ("cloud.ply", "ref.ply", "out.ply", "report.json"))
    dmb.write_points_ply(src, v)
    dmb.write_points_ply(ref, v[:N_SPHERE:2])
    assert cloud_eval.main(["--cloud", src, "--reference", ref, "--max_dist", "5", "--reduce", "0.3", "--seed", "3",
                            "--neighbour_radius", "6", "--min_neighbours", "2", "--component_radius", "5", "--min_component", "100",
                            "--write_cloud", out, "--output", rep]) == 0
    lines = capsys.readouterr().out.splitlines()
    idx = cloud_eval.thin(c.points, 0.3, seed=3)
    after_thin = len(idx)
    idx = idx[cloud_eval.drop_isolated(c.points[idx], 6.0, 2)]
    after_count = len(idx)
    assert (idx >= len(c.points) - N_CLUMP).sum() >= 3  # the count leaves what the thinning left of the clump
    idx = idx[cloud_eval.drop_small_components(c.points[idx], 5.0, 100)]
    assert 5000 < len(idx) < after_count < after_thin and idx.max() < N_SPHERE  # no floater and no clump is left
    assert dmb.read_ply_binary(out).tobytes() == v[idx].tobytes()
    report = json.load(open(rep))
    assert report["cloud_points"] == len(idx) and report["cloud_points_before_components"] == after_count
    assert report["cloud_points_before_filter"] == after_thin and report["min_component"] == 100
    assert len(lines) == 4 and "-> %d points" % after_thin in lines[1] and "-> %d points" % after_count in lines[2]
    assert "components" in lines[3] and "cloud %d -> %d points" % (after_count, len(idx)) in lines[3]


@pytest.mark.gpu
def test_batch_fuses_and_drops_the_small_components(hip, tmp_path):
    """batch --fuse --fuse_component_radius on the suite's small synthetic scan (as tests/test_fusion.py writes it): fused.ply
    is the unfiltered run's cloud without its small components, and the report says so.  The radius is the median distance
    to the nearest neighbour in the unfiltered cloud: about half of the points have nobody within it."""
    from gipuma_amd import batch, synth
    cfg = synth.tiny_config(cols=96, rows=64, n_src=4, blocksize=9, iterations=3, n_best=2)
    gs, info = synth.build_problem(cfg)
    img_dir, p_dir = tmp_path / "img", tmp_path / "calib"
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
    base = ["--images-folder", str(img_dir), "--p-folder", str(p_dir), "--blocksize=9", "--iterations=3", "--n_best=2",
            "--min_angle=2", "--max_angle=60", "--max_views=10", "--depth_min=300", "--depth_max=800",
            "--cam_scale=%.9g" % np.float32(cfg["cam_scale"]), "--disp_thresh=0.02", "--normal_thresh=30", "--num_consistent=2", "--fuse"]
    plain_dir, filtered_dir = str(tmp_path / "plain"), str(tmp_path / "filtered")
    assert batch.main(base + ["--output-folder", plain_dir]) == 0
    plain = dmb.read_ply_binary(os.path.join(plain_dir, "fused.ply"))
    xyz = np.stack([plain["x"], plain["y"], plain["z"]], -1)
    assert len(xyz) >= 100
    d2 = cloud_eval.nearest_k(xyz, 1e6, 1)[0][:, 0]
    radius = float(f32(np.sqrt(np.median(d2.astype(np.float64)))))
    label, size = cloud_eval.component_labels(xyz, radius)
    r = components_ref.components(xyz, radius, 3)
    assert np.array_equal(label, r.label) and np.array_equal(size, r.size) and 0 < r.kept and 0 < r.dropped
    assert batch.main(base + ["--output-folder", filtered_dir, "--fuse_component_radius", repr(radius), "--fuse_min_component", "3"]) == 0
    got = dmb.read_ply_binary(os.path.join(filtered_dir, "fused.ply"))
    assert got.tobytes() == plain[r.keep == 1].tobytes()
    fusion = json.load(open(os.path.join(filtered_dir, "batch_rank0.json")))["fusion"]
    assert fusion["points_before_components"] == len(plain) and fusion["points"] == len(got) == r.kept
    assert fusion["components"] == r.components and fusion["component_device_ms"] > 0
    assert "points_before_components" not in json.load(open(os.path.join(plain_dir, "batch_rank0.json")))["fusion"]
