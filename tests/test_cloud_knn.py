"""The k nearest neighbours of every point inside its own cloud and the statistical outlier filter on them (DESIGN.md 17,
gipuma_hip_cloud_knn, gipuma_amd.cloud_eval.knn / nearest_k / drop_outliers).  Every case is a cloud, a radius, a k and a
condition -- stated on the restatement (tests/knn_ref.py) alone -- that it reaches the path it is named for; that condition
runs without a device, and so do the comparison of the restatement's two forms (the brute force, the k-d tree's pairs), the
C-ABI's argument checks and the command lines.  GPU: d2 and mean as uint32 bit patterns, idx, m and the info counts equal
the restatement at every grid; each output alone; the descriptor's stream; device tensors; agreement with the search and
the neighbour count; the filter; the score with the filter."""
import ctypes as C
import functools

import numpy as np
import pytest
# torch before the `hip` fixture loads the library (see tests/test_cloud_scale.py): this module must also run on its own
import torch  # noqa: F401

from gipuma_amd import abi, cloud_eval, dmb
from tests import cloud_ref, knn_ref
from tests import test_cloud_neighbours as neighbour_cases
from tests import test_cloud_scale as scale
from tests import test_cloud_thin as thin_cases
from tests.abi_layout import assert_mirrors_header
from tests.thin_ref import _d2

f32 = np.float32
GRIDS = thin_cases.GRIDS
assert GRIDS == (0, 1, 2, 7, 256)


# ----------------------------------------------------------------------------------------------------------------------
# The clouds (by name: several cases share one, and its brute force at k = 32) and the cases
# ----------------------------------------------------------------------------------------------------------------------
def _lattice7():
    g = np.arange(7, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


LATTICE_PERMUTATION = np.random.default_rng(1717).permutation(343)
N_HALO = 40


def _halo():
    """points 3.5 outside the noisy sphere (R = 50, 6000 points: a spacing of about 2.3), one and a half spacings off it"""
    v = np.random.default_rng(2727).normal(size=(N_HALO, 3))
    return v * (53.5 / np.linalg.norm(v, axis=1, keepdims=True))


CLOUDS = {
    "uniform": thin_cases._uniform,
    "lattice": _lattice7,
    "lattice_permuted": lambda: _lattice7()[LATTICE_PERMUTATION],
    "identical": lambda: np.concatenate([np.repeat(thin_cases._uniform(1, seed=707), 40, axis=0), [[500.0, 500.0, 500.0]]]),
    "dense": lambda: np.random.default_rng(3737).uniform(0.0, 6.0, (2000, 3)),
    "crowded": lambda: np.concatenate([np.random.default_rng(909).uniform(0.0, 0.01, (300, 3)),
                                       [[1000.0, 0.0, 0.0], [0.0, 1000.0, 0.0]]]),
    "pair": lambda: [[0, 0, 0], [3, 4, 0]],
    "non_finite": lambda: thin_cases.case("non_finite").points,
    "flat_coplanar": lambda: thin_cases.case("flat_coplanar").points,
    "flat_collinear": lambda: thin_cases.case("flat_collinear").points,
    **{"points_%d" % n: functools.partial(lambda n: thin_cases._uniform(n, seed=303, box=4.0), n) for n in (0, 1, 2, 4, 5)},
    "large_coordinates": lambda: thin_cases.case("large_coordinates").points,
    **{"scale_" + name: functools.partial(lambda name: scale.thin_case(name).points, name) for name in scale.THIN_BUILDERS},
    # the neighbour filter's sphere, 54 single floaters and three clumps of three, then the halo
    "sphere_halo": lambda: np.concatenate([neighbour_cases.cloud("sphere_floaters"), _halo()]),
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    return np.ascontiguousarray(CLOUDS[name](), dtype=f32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def longest(name, radius):
    """the brute force of a cloud at a radius with 32 slots, computed once: every shorter list is its first k slots"""
    return knn_ref.knn(cloud(name), radius, knn_ref.MAX_K)


class Case:
    def __init__(self, name, radius, k, check, grids=GRIDS):
        self.name, self.radius, self.k, self.check, self.grids = name, f32(radius), k, check, grids

    @property
    def points(self):
        return cloud(self.name)

    @functools.cached_property
    def ref(self):
        return knn_ref.shorter(longest(self.name, self.radius), self.points, self.k)


def _case_uniform(k):
    def check(c):
        r, n = c.ref, len(c.points)
        counts = neighbour_cases.exact("uniform", c.radius)
        assert (int(counts.min()), int(counts.max())) == (0, 14) and np.array_equal(r.m, np.minimum(counts, k))
        if k in (4, 8):  # complete and short lists in one run
            assert r.complete >= 0.05 * n and r.short >= 0.2 * n, (r.complete, r.short)
        if k == 32:
            assert r.complete == 0 and r.short == n
        assert c.k in (1, 4, 8, 9, 16, 17, 32)  # either side of every boundary between the kernel's list lengths
    return Case("uniform", 1.5, k, check)


def _case_lattice(permuted, k):
    def check(c):
        r, p = c.ref, c.points
        inner = ((p > 0) & (p < 6)).all(axis=1)
        # 6 sites at d2 = 1, 12 at d2 = 2, the radius ends before d2 = 3: many equal d2, the order is the index's alone
        want = [1.0] * 6 + [2.0] * 12
        assert (r.d2[inner] == np.array(want[:k], dtype=f32)).all() and (r.m[inner] == k).all() and inner.sum() == 125
        # a corner site has 6 sites within the radius, a site on an edge 9, on a face 13: short lists of three lengths at k = 18
        assert r.m.min() == 6 and r.short == (8 if k == 8 else 343 - 125) and set(r.m.tolist()) == ({6, 8} if k == 8 else {6, 9, 13, 18})
        first, second = r.idx[inner][:, :min(k, 6)], r.idx[inner][:, 6:]
        assert (np.diff(first, axis=1) > 0).all() and (np.diff(second, axis=1) > 0).all()
        if permuted:  # the same lists of d2 at the same sites, other index lists: not the plain lattice's mapped over
            plain = case("lattice_k%d" % k).ref
            assert np.array_equal(r.d2, plain.d2[LATTICE_PERMUTATION])
            mapped = np.argsort(LATTICE_PERMUTATION)[plain.idx[LATTICE_PERMUTATION][inner]]  # the plain lists, renumbered
            assert np.array_equal(np.sort(mapped[:, :6], axis=1), r.idx[inner][:, :6])  # the same six sites, in the new order
            assert not np.array_equal(mapped, r.idx[inner])
    return Case("lattice_permuted" if permuted else "lattice", 1.5, k, check)


def _case_identical(k):
    def check(c):
        r = c.ref
        assert not r.d2[:40].any() and (r.m[:40] == k).all() and r.m[40] == 0 and not r.mean[:40].any()
        for i in (0, 1, k - 1, k, k + 1, 39):  # the lowest indices other than the point's own
            assert r.idx[i].tolist() == [j for j in range(k + 1) if j != i][:k]
        assert r.idx[40].tolist() == [-1] * k and np.isposinf(r.d2[40]).all() and np.isposinf(r.mean[40])
    return Case("identical", 1.0, k, check)


def _case_dense():
    def check(c):
        r, p = c.ref, c.points.astype(np.float64)
        counts = knn_ref.knn(c.points, c.radius, 32).m
        assert (counts == 32).mean() > 0.9 and r.complete == len(p)  # far more than k = 8 neighbours nearly everywhere
        # the automatic grid is 3 cells an axis (floor(5.99 / 1.5)): the neighbours of a point in the middle stand in at
        # least three cell rows along y and along z, so that late rows must displace what early rows put into the list
        i = int(np.argmin(np.linalg.norm(p - 3.0, axis=1)))
        h = (p.max(axis=0) - p.min(axis=0)).max() / 3
        near = np.nonzero(_d2(c.points[i], c.points) <= cloud_ref.squared(c.radius))[0]
        cells = np.floor((p[near] - p.min(axis=0)) / h).astype(int)
        assert len(near) > 100 and len(set(cells[:, 1])) >= 3 and len(set(cells[:, 2])) >= 3
        rows_of_list = {tuple(np.floor((p[j] - p.min(axis=0)) / h).astype(int)[:0:-1]) for j in r.idx[i]}  # (z, y)
        earlier = sum((int(z), int(y)) < min(rows_of_list) for y, z in cells[:, 1:])  # the walk goes z outermost, then y
        assert earlier >= 8  # the list was full of records from earlier rows before its first final entry came: all displaced
    return Case("dense", 1.5, 8, check)


def _case_crowded():
    def check(c):
        r, p = c.ref, c.points.astype(np.float64)
        h = (p.max(axis=0) - p.min(axis=0)).max() / 4
        assert len({tuple(x) for x in np.floor((p[:300] - p.min(axis=0)) / h).astype(int)}) == 1  # 300 points in one cell
        counts = neighbour_cases.neighbours_ref.neighbours(c.points, c.radius).exact
        assert counts[:300].max() > 64 and r.complete >= 150 and r.short >= 10 and r.m[300:].tolist() == [0, 0], (r.complete, r.short)
    return Case("crowded", 4e-3, 32, check, grids=(0, 4))


def _case_pair(inside):
    def check(c):
        r = c.ref
        if inside:  # d2 == r2 == 25 exactly
            assert r.d2.tolist() == [[25.0], [25.0]] and r.idx.tolist() == [[1], [0]] and r.mean.tolist() == [5.0, 5.0]
        else:  # r2 an ulp below
            assert cloud_ref.squared(c.radius) < f32(25) and r.idx.tolist() == [[-1], [-1]] and r.short == 2
    return Case("pair", f32(5) if inside else np.nextafter(f32(5), f32(0)), 1, check)


def _case_non_finite():
    def check(c):
        r, p = c.ref, c.points
        bad = ~np.isfinite(p).all(axis=1)
        assert bad.sum() == 30 == r.not_finite and {float(x) for x in p[bad][~np.isfinite(p[bad])]} >= {np.inf, -np.inf}
        assert np.isnan(p[bad]).any() and all((~np.isfinite(p[bad][:, a])).any() for a in range(3))  # each coordinate
        assert not r.m[bad].any() and (r.idx[bad] == -1).all() and np.isposinf(r.d2[bad]).all() and np.isposinf(r.mean[bad]).all()
        assert not np.isin(r.idx, np.nonzero(bad)[0]).any() and r.complete > 100 and r.short > 100  # no finite point lists them
    return Case("non_finite", 1.5, 4, check)


def _case_flat(kind):
    def check(c):
        ext = c.points.max(axis=0) - c.points.min(axis=0)
        assert (ext == 0).sum() == (1 if kind == "coplanar" else 2)  # axes of zero extent: one cell each
        assert c.ref.complete >= 0.2 * len(c.points) and c.ref.short >= 0.05 * len(c.points), (c.ref.complete, c.ref.short)
    return Case("flat_" + kind, 0.3 if kind == "coplanar" else 0.05, 4, check)


def _case_count(n):
    def check(c):  # every point within the radius of every other: n - 1 neighbours each
        r = c.ref
        assert len(c.points) == n and (r.m == min(4, max(n - 1, 0))).all() and (r.complete, r.short) == ((n, 0) if n == 5 else (0, n))
        assert np.isposinf(r.mean).all() if n < 5 else np.isfinite(r.mean).all()
    return Case("points_%d" % n, 10.0, 4, check)


def _case_large_coordinates():
    def check(c):
        assert np.spacing(f32(65536.0)) > 0.25 * c.radius  # a coordinate's own rounding step is a quarter of the radius
        assert c.ref.complete >= 0.1 * len(c.points) and c.ref.short >= 0.1 * len(c.points), (c.ref.complete, c.ref.short)
        ties = (np.diff(c.ref.d2.view(np.uint32), axis=1) == 0) & (c.ref.idx[:, 1:] >= 0)
        assert ties.sum() > 100  # the coarse coordinates make equal d2 common: the index decides
    return Case("large_coordinates", 0.03, 8, check)


def _case_scale(name):
    """the thinning's extreme scales (tests/test_cloud_scale.py): its clouds, its radii and its expectation of one cell"""
    t = scale.thin_case(name)

    def check(c):
        t.check(t)
        r, n = c.ref, len(c.points)
        assert tuple(g for g in GRIDS if scale.thin_layout(c, g)[1]) == tuple(t.one_cell)
        if name == "r2_infinite":
            # inf <= inf: the two points at +-3e38 are neighbours of everything at d2 = +inf.  The 400 ordinary points never
            # list them (8 finite d2 come first); the far two list the eight lowest indices, every slot FILLED at d2 = +inf:
            # m == k and mean = +inf -- the meaning of a slot with d2 = +inf and idx >= 0 that the header states
            assert np.isposinf(cloud_ref.squared(c.radius)) and r.complete == n == 402 and np.isfinite(r.mean[:400]).all()
            assert r.idx[400:].tolist() == [list(range(8))] * 2 and np.isposinf(r.d2[400:]).all() and np.isposinf(r.mean[400:]).all()
        elif name == "r2_zero":  # only the exact copy is within a radius whose square is 0
            assert cloud_ref.squared(c.radius) == 0 and (r.m == 1).all() and r.idx[:512, 0].tolist() == list(range(512, 1024))
        elif name.endswith("41"):  # a quarter of the edge: 300 points crowd each other
            assert r.complete >= 20 and r.short >= 20, (r.complete, r.short)
        else:  # a sixteenth of the edge: one or two neighbours on average, lists of every short length
            assert r.short == n and set(r.m.tolist()) >= {0, 1, 2, 3, 4}
    return Case("scale_" + name, t.radius, 8, check)


UNIFORM_K = (1, 4, 8, 9, 16, 17, 32)
BUILDERS = {
    **{"uniform_k%d" % k: functools.partial(_case_uniform, k) for k in UNIFORM_K},
    **{"lattice_k%d" % k: functools.partial(_case_lattice, False, k) for k in (8, 18)},
    **{"lattice_permuted_k%d" % k: functools.partial(_case_lattice, True, k) for k in (8, 18)},
    **{"identical_k%d" % k: functools.partial(_case_identical, k) for k in (8, 32)},
    "dense": _case_dense,
    "crowded": _case_crowded,
    "radius_inclusive": lambda: _case_pair(True),
    "radius_just_short": lambda: _case_pair(False),
    "non_finite": _case_non_finite,
    "flat_coplanar": lambda: _case_flat("coplanar"),
    "flat_collinear": lambda: _case_flat("collinear"),
    **{"points_%d" % n: functools.partial(_case_count, n) for n in (0, 1, 2, 4, 5)},  # n in {1, 2, k, k + 1}, and none
    "large_coordinates": _case_large_coordinates,
}
SCALE_BUILDERS = {"scale_" + name: functools.partial(_case_scale, name) for name in scale.THIN_BUILDERS}
ALL_BUILDERS = {**BUILDERS, **SCALE_BUILDERS}


@functools.lru_cache(maxsize=None)
def case(name):
    return ALL_BUILDERS[name]()


# the large cloud: test_cloud_scale's 300 001 targets, against the sparse restatement
LARGE_RADIUS, LARGE_K = 0.45, 8  # (a radius below 1 / 256 of the extent: the automatic grid is capped)


@functools.lru_cache(maxsize=None)
def large_ref():
    return knn_ref.knn_sparse(scale.large_clouds()[1], LARGE_RADIUS, LARGE_K)


def _check_large():
    r = large_ref()
    assert r is not None and r.not_finite == 0 and r.complete + r.short == scale.N_LARGE
    assert r.complete >= 0.05 * scale.N_LARGE and r.short >= 0.2 * scale.N_LARGE, (r.complete, r.short)
    assert not r.m[list(scale.OUTLIERS)].any()  # (nothing within 10 of them)
    assert scale.N_LARGE > 1000 * 256  # a launch of more than 1 000 workgroups


# the filter: the sphere's own points, 54 floaters, three clumps of three, the halo
FILTER_RADIUS, FILTER_K, FILTER_STD = 6.0, 8, 2.0
N_SPHERE = neighbour_cases.N_SPHERE


@functools.lru_cache(maxsize=None)
def filter_ref():
    r = knn_ref.shorter(longest("sphere_halo", f32(FILTER_RADIUS)), cloud("sphere_halo"), FILTER_K)
    return r, knn_ref.drop_outliers(r, FILTER_K, FILTER_STD, FILTER_RADIUS)


def _check_filter():
    """returns the share of the sphere's own points that survive: a property of the case, printed and recorded in DESIGN.md
    17, not fixed beforehand"""
    r, f = filter_ref()
    n = len(cloud("sphere_halo"))
    floaters, halo = np.arange(N_SPHERE, N_SPHERE + 63), np.arange(N_SPHERE + 63, n)
    assert len(halo) == N_HALO and n == N_SPHERE + 63 + N_HALO
    assert (r.m[floaters] < FILTER_K).all() and not f.keep[floaters].any()  # every floater is dropped as short
    by_threshold = halo[(r.m[halo] == FILTER_K) & ~f.keep[halo]]
    assert len(by_threshold) >= 1 and (r.mean[by_threshold] > f32(f.threshold)).all()  # not by the short rule
    assert f.sigma > 0 and f.mu < f.threshold and f.short == r.short >= 63
    share = float(f.keep[:N_SPHERE].mean())
    print("the filter at radius %g, k %d, std_ratio %g: mu %.4f sigma %.4f threshold %.4f; %d of %d halo points dropped (%d by the "
          "threshold), %.4f of the sphere's own points survive"
          % (FILTER_RADIUS, FILTER_K, FILTER_STD, f.mu, f.sigma, f.threshold, int((~f.keep[halo]).sum()), N_HALO, len(by_threshold),
             share))
    return share


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    r, n, k = c.ref, len(c.points), c.k
    assert r.d2.shape == r.idx.shape == (n, k) and (r.d2.dtype, r.idx.dtype, r.m.dtype, r.mean.dtype) == (f32, np.int32, np.uint32, f32)
    assert r.complete + r.short + r.not_finite == n and r.complete == int((r.m == k).sum())
    filled = np.arange(k)[None, :] < r.m[:, None]
    assert ((r.idx >= 0) == filled).all() and np.isposinf(r.d2[~filled]).all()
    with np.errstate(invalid="ignore"):  # ascending in (d2, idx) over the filled slots; never the point itself
        d, j = r.d2[:, :-1], r.idx[:, :-1]
        assert (~filled[:, 1:] | (d < r.d2[:, 1:]) | ((d == r.d2[:, 1:]) & (j < r.idx[:, 1:]))).all()
    assert not (r.idx == np.arange(n)[:, None]).any()
    assert np.array_equal(np.isposinf(r.mean), (r.m < k) | np.isposinf(r.d2[:, k - 1]))
    direct = knn_ref.knn(c.points, c.radius, k)  # the brute force at this k itself, not cut from the one at 32
    for got, want in zip(direct, r):
        assert np.array_equal(got, want), name


def test_the_sparse_restatement_equals_the_brute_force_on_every_small_case():
    """(the extreme scales are not of the ordinary magnitudes the sparse form's argument needs: they are judged against
    the brute force alone, as in tests/test_cloud_scale.py)"""
    for name in sorted(BUILDERS):
        c = case(name)
        s = knn_ref.knn_sparse(c.points, c.radius, c.k)
        assert s is not None, name
        for got, want in zip(s, c.ref):
            assert np.array_equal(np.asarray(got).view(np.uint32) if np.asarray(got).dtype == f32 else got,
                                  np.asarray(want).view(np.uint32) if np.asarray(want).dtype == f32 else want), name
            assert np.asarray(got).dtype == np.asarray(want).dtype, name
    s = knn_ref.knn_sparse(cloud("sphere_halo"), FILTER_RADIUS, FILTER_K)
    for got, want in zip(s, filter_ref()[0]):
        assert np.array_equal(got, want)
    assert knn_ref.drop_outliers(s, FILTER_K, FILTER_STD, FILTER_RADIUS)[1:] == filter_ref()[1][1:]


def test_the_large_cloud_reaches_its_paths():
    _check_large()


def test_the_filter_case_reaches_its_paths():
    assert 0.5 < _check_filter() <= 1.0
    r, _ = filter_ref()
    nothing = knn_ref.drop_outliers(knn_ref.knn(cloud("pair"), 1.0, 1), 1, 1.0, 1.0)  # S is empty: nothing kept
    assert not nothing.keep.any() and np.isnan(nothing.threshold) and nothing.short == 2
    strict = knn_ref.drop_outliers(r, FILTER_K, 0.0, FILTER_RADIUS)  # std_ratio 0: the threshold is the mean itself
    assert strict.threshold == float(f32(strict.mu)) and 0 < strict.keep.sum() < (r.m == FILTER_K).sum()


def test_the_restatement_turns_down_what_the_library_turns_down():
    for k in (0, 33, -1, 2.5):
        with pytest.raises(ValueError):
            knn_ref.knn(cloud("pair"), 1.0, k)
        with pytest.raises(ValueError):
            knn_ref.knn_sparse(cloud("pair"), 1.0, k)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            knn_ref.knn(cloud("pair"), radius, 1)
    r = knn_ref.knn(cloud("pair"), 5.0, 1)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            knn_ref.drop_outliers(r, 1, bad, 5.0)
        with pytest.raises(ValueError):
            cloud_eval.drop_outliers(cloud("pair"), 5.0, 1, bad)
    with pytest.raises(ValueError):  # r2 = +inf: a complete list's mean may say +inf, like a short one's
        knn_ref.drop_outliers(r, 1, 1.0, 1e20)
    with pytest.raises(ValueError):
        cloud_eval.drop_outliers(cloud("pair"), 1e20, 1, 1.0)
    assert knn_ref.knn(cloud("pair"), 5.0, 32).m.tolist() == [1, 1]  # k = 32 is allowed


def _desc(**kw):
    d = abi.KnnDesc()
    d.abi_version, d.n_points, d.points, d.radius, d.k = abi.ABI_VERSION, 4, 0x1000, 1.0, 8
    d.grid, d.device_id, d.stream = 0, 0, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last ones for want of a device when there is
    none -- with a device they are not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(d2=out, idx=out, count=out, mean=out, **kw):
        return lib.gipuma_hip_cloud_knn(C.byref(_desc(**kw)), d2, idx, count, mean, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(radius=bad) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    for bad in (0, 33, -1):
        assert rc(k=bad) == abi.ERR_ARG and b"k must be 1..32" in lib.gipuma_hip_last_error()
    # n * k >= 2^31 with a list asked for: 2^28 points at k = 8 are too many, one fewer is not; without the lists neither
    for lists in (dict(), dict(d2=None), dict(idx=None)):
        assert rc(n_points=1 << 28, k=8, **lists) == abi.ERR_UNSUPPORTED and b"slots" in lib.gipuma_hip_last_error()
    assert rc(n_points=(1 << 31) - 1, k=1) != abi.ERR_UNSUPPORTED and rc(n_points=(1 << 28) - 1, k=8) != abi.ERR_UNSUPPORTED
    assert rc(n_points=1 << 28, k=8, d2=None, idx=None) != abi.ERR_UNSUPPORTED
    assert rc(n_points=(1 << 26) + 1, k=32) == abi.ERR_UNSUPPORTED and rc(n_points=1 << 26, k=32) == abi.ERR_UNSUPPORTED
    assert rc(n_points=1 << 28, k=8, radius=0.0) == abi.ERR_ARG  # (the thinning's order: the radius comes first)
    assert rc(points=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(d2=None, idx=None, count=None, mean=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(n_points=-1) == abi.ERR_ARG
    assert rc(n_points=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_knn(None, out, out, out, out, None, None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        for valid in (dict(), dict(k=1), dict(k=32), dict(d2=None, idx=None, count=None), dict(idx=None, count=None, mean=None),
                      dict(n_points=0, points=None, d2=None, idx=None, count=None, mean=None)):
            assert rc(**valid) == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        for call in (lambda: cloud_eval.nearest_k(np.zeros((2, 3), f32), 1.0, 1),
                     lambda: cloud_eval.drop_outliers(np.zeros((2, 3), f32), 1.0, 1, 1.0)):
            with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
                call()
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.KnnDesc, "gipuma_hip_knn_desc",
                          ["abi_version", "n_points", "points", "radius", "k", "grid", "device_id", "stream"])
    assert "gipuma_hip_cloud_knn" in [s[0] for s in abi.SYMBOLS]
    assert [f[0] for f in abi.KnnDesc._fields_ if f[0] != "k"] == \
        [f[0] for f in abi.NeighboursDesc._fields_ if f[0] not in ("min_neighbours", "max_count")]  # laid out like the count's


CLI = ["--cloud", "c.ply", "--reference", "r.ply"]
ON = ["--outlier_radius", "1", "--outlier_k", "8", "--outlier_std", "2"]


def _without(argv, option):
    i = argv.index(option)
    return argv[:i] + argv[i + 2:]


def _with(argv, option, value):
    i = argv.index(option)
    return argv[:i + 1] + [value] + argv[i + 2:]


@pytest.mark.parametrize("argv", [CLI + _without(ON, o) for o in ON[::2]] + [CLI + ON[2 * i:2 * i + 2] for i in range(3)] +
                         [CLI + _with(ON, "--outlier_radius", v) for v in ("0", "-1", "nan", "inf")] +
                         [CLI + _with(ON, "--outlier_k", v) for v in ("0", "33", "-1", "2.5")] +
                         [CLI + _with(ON, "--outlier_std", v) for v in ("-1", "nan", "inf")])
def test_cli_outlier_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_outlier_arguments():
    a = cloud_eval.parse_args(CLI)
    assert (a.outlier_radius, a.outlier_k, a.outlier_std) == (0.0, 0, 0.0) and a.write_cloud is None
    a = cloud_eval.parse_args(CLI + ["--outlier_radius", "0.1", "--outlier_k", "32", "--outlier_std", "0", "--write_cloud", "out.ply"])
    assert (a.outlier_radius, a.outlier_k, a.outlier_std) == (float(f32(0.1)), 32, 0.0) and a.write_cloud == "out.ply"  # (through float32)
    a = cloud_eval.parse_args(CLI + ON + ["--reduce", "0.2", "--neighbour_radius", "1", "--min_neighbours", "3"])
    assert (a.outlier_radius, a.outlier_k, a.outlier_std, a.reduce, a.min_neighbours) == (1.0, 8, 2.0, float(f32(0.2)), 3)


def test_batch_outlier_arguments(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    on = ["--fuse_outlier_radius", "0.1", "--fuse_outlier_k", "16", "--fuse_outlier_std", "1.5"]
    a = batch.parse_args(base)
    assert (a.fuse_outlier_radius, a.fuse_outlier_k, a.fuse_outlier_std) == (0.0, 0, 0.0)
    a = batch.parse_args(base + ["--fuse"] + on)
    assert (a.fuse_outlier_radius, a.fuse_outlier_k, a.fuse_outlier_std) == (float(f32(0.1)), 16, 1.5)
    a = batch.parse_args(base + ["--fuse", "--fuse_neighbour_radius", "1", "--fuse_min_neighbours", "8"] + on)
    assert a.fuse_min_neighbours == 8 and a.fuse_outlier_k == 16
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + on)
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    for bad in ([_without(on, o) for o in on[::2]] + [_with(on, "--fuse_outlier_radius", v) for v in ("-1", "nan")] +
                [_with(on, "--fuse_outlier_k", v) for v in ("0", "33")] + [_with(on, "--fuse_outlier_std", "-1")]):
        with pytest.raises(SystemExit) as e:
            batch.parse_args(base + ["--fuse"] + bad)
        assert e.value.code == 2
    capsys.readouterr()


def test_score_without_the_new_arguments_builds_the_report_it_builds_today(monkeypatch):
    """score() with the search replaced by the search's restatement, so that it runs without a device: the keys are those
    of before the filter (tests/test_cloud_thin.py lists them), and the new arguments are refused where they are wrong
    before anything is computed"""
    def nearest(queries, targets, max_dist, grid=0, device_id=0, return_info=False):
        r = cloud_ref.nearest(queries, targets, max_dist)
        return r.d2, r.idx, 0.5, dict(found=r.found, none=r.none, **{k: 1 for k in cloud_eval._STATS})

    monkeypatch.setattr(cloud_eval, "nearest", nearest)
    rng = np.random.default_rng(17)
    a, b = rng.uniform(0.0, 5.0, (60, 3)).astype(f32), rng.uniform(0.0, 5.0, (70, 3)).astype(f32)
    plain = cloud_eval.score(a, b, max_dist=2.0)
    assert set(plain) == thin_cases.SCORE_KEYS and plain["cloud_points"] == 60
    assert cloud_eval.score(a, b, max_dist=2.0, outlier_radius=0.0, outlier_k=0, outlier_std=0.0) == plain
    report, indices = cloud_eval.score(a, b, max_dist=2.0, return_indices=True)
    assert report == plain and indices is None
    for bad in (dict(outlier_radius=-1.0), dict(outlier_radius=float("nan")), dict(outlier_radius=1.0, outlier_k=0, outlier_std=1.0),
                dict(outlier_radius=1.0, outlier_k=33, outlier_std=1.0), dict(outlier_radius=1.0, outlier_k=8, outlier_std=-1.0)):
        with pytest.raises(ValueError):
            cloud_eval.score(a, b, max_dist=2.0, **bad)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _assert_equals_ref(d2, idx, m, mean, info, r, what):
    """d2 and mean as uint32 bit patterns; each output may be None (not asked for)"""
    if d2 is not None:
        assert d2.dtype == torch.float32 and tuple(d2.shape) == r.d2.shape, what
        diff = _bits(d2) != r.d2.view(np.uint32)
        assert not diff.any(), "%s: d2 differs in %d slots" % (what, int(diff.sum()))
    if idx is not None:
        assert idx.dtype == torch.int32 and tuple(idx.shape) == r.idx.shape, what
        diff = idx.cpu().numpy() != r.idx
        assert not diff.any(), "%s: idx differs in %d slots" % (what, int(diff.sum()))
    if m is not None:
        assert np.array_equal(_bits(m), r.m), "%s: m differs at %d points" % (what, int((_bits(m) != r.m).sum()))
    if mean is not None:
        got, want = _bits(mean), r.mean.view(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), "%s: mean differs at %d points, first %d: %08x for %08x" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    assert (info["complete"], info["short"], info["not_finite"]) == (r.complete, r.short, r.not_finite), what


GPU_RUNS = [(name, g) for name in sorted(ALL_BUILDERS) for g in ((0, 4) if name == "crowded" else GRIDS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_the_kernel_equals_the_restatement_in_every_bit(hip, name, grid):
    c = case(name)
    assert grid in c.grids
    c.check(c)
    what = "%s at grid %d" % (name, grid)
    d2, idx, m, mean, ms, info = cloud_eval.knn(c.points, c.radius, c.k, grid=grid)
    _assert_equals_ref(d2, idx, m, mean, info, c.ref, what)
    ok = c.points[np.isfinite(c.points).all(axis=1)]
    if len(ok):
        assert ms > 0
        G, one_cell = scale.thin_layout(c, grid)  # the thinning's documented rule, not asked of the library
        assert info["grid"] == G, "%s: the library reports %d cells" % (what, info["grid"])
        if one_cell:
            assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)
        elif grid:
            assert max(info["cells_x"], info["cells_y"], info["cells_z"]) == grid
        if name == "crowded" and grid == 4:
            assert info["cells_x"] * info["cells_y"] * info["cells_z"] == 16
        if name == "dense" and grid == 0:
            assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (3, 3, 3)
    else:
        assert info["grid"] == 0 and info["complete"] == 0
    got = cloud_eval.nearest_k(c.points, c.radius, c.k, grid=grid)  # the public function: numpy, m as uint32
    assert [a.dtype for a in got] == [f32, np.int32, np.uint32] and got[0].shape == got[1].shape == (len(c.points), c.k)
    assert np.array_equal(got[0].view(np.uint32), c.ref.d2.view(np.uint32)) and np.array_equal(got[1], c.ref.idx), what
    assert np.array_equal(got[2], c.ref.m), what


@pytest.mark.gpu
def test_large_cloud_equals_the_sparse_restatement(hip):
    _check_large()
    b = scale.large_clouds()[1]
    d2, idx, m, mean, ms, info = cloud_eval.knn(b, LARGE_RADIUS, LARGE_K)
    _assert_equals_ref(d2, idx, m, mean, info, large_ref(), "300 001 points")
    assert float(scale._longest_extent(b)) / LARGE_RADIUS > 256 and info["grid"] == 256  # floor(longest / radius), capped


@pytest.mark.gpu
def test_each_output_alone(hip):
    for name in ("uniform_k8", "uniform_k17"):
        c = case(name)
        for alone in range(4):
            switches = [i == alone for i in range(4)]
            outs = cloud_eval.knn(c.points, c.radius, c.k, d2=switches[0], idx=switches[1], count=switches[2], mean=switches[3])
            assert [o is not None for o in outs[:4]] == switches
            _assert_equals_ref(*outs[:4], outs[5], c.ref, "%s, output %d alone" % (name, alone))


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_runs_repeat(hip):
    c = case("dense")
    pts = torch.from_numpy(c.points).cuda()
    runs = []
    for _ in range(2):  # (the order inside a cell varies from run to run; the k smallest pairs do not)
        d2, idx, m, mean, ms, info = cloud_eval.knn(pts, c.radius, c.k)
        assert d2.is_cuda and idx.is_cuda and m.is_cuda and mean.is_cuda
        _assert_equals_ref(d2, idx, m, mean, info, c.ref, "device tensor")
        runs.append(b"".join(t.cpu().numpy().tobytes() for t in (d2, idx, m, mean)))
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_lists_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the cloud was written just before, the device not synchronised: the library
    runs behind it on that stream.  Two cloud sizes one after the other on the same stream."""
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("uniform_k9", "non_finite"):
        c = case(name)
        n, k = len(c.points), c.k
        staged = torch.from_numpy(c.points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the cloud the library reads: a device copy queued on the caller's stream
            pts = staged.clone()
            d2 = torch.empty((n, k), dtype=torch.float32, device="cuda")
            idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
            m = torch.empty(n, dtype=torch.int32, device="cuda")
            mean = torch.empty(n, dtype=torch.float32, device="cuda")
        d = _desc(n_points=n, points=pts.data_ptr(), radius=float(c.radius), k=k, stream=stream.cuda_stream)
        info, ms = (C.c_int64 * 8)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_knn(C.byref(d), d2.data_ptr(), idx.data_ptr(), m.data_ptr(), mean.data_ptr(), info,
                                                C.byref(ms)), "knn")
        got = dict(complete=info[0], short=info[1], not_finite=info[2])
        _assert_equals_ref(d2, idx, m, mean, got, c.ref, "%s on the caller's stream" % name)
        assert ms.value > 0 and info[3] == 0
    info = (C.c_int64 * 8)(*([7] * 8))
    abi.check(lib, lib.gipuma_hip_cloud_knn(C.byref(_desc(n_points=0, points=None)), None, None, None, None, info, None), "nothing")
    assert list(info) == [0] * 8
    outs = cloud_eval.knn(cloud("points_0"), 1.0, 4)  # n = 0 through the public function: empty tensors, nothing written
    assert tuple(outs[0].shape) == (0, 4) and tuple(outs[2].shape) == (0,) and outs[5]["complete"] == 0


@pytest.mark.gpu
def test_agreement_with_the_neighbour_count_and_the_search(hip):
    p, radius = cloud("uniform"), f32(1.5)
    counts = cloud_eval.neighbour_counts(p, radius)
    for k in (4, 32):
        assert np.array_equal(cloud_eval.nearest_k(p, radius, k)[2], np.minimum(counts, k))
        kept = cloud_eval.drop_isolated(p, radius, k)  # the two filters nest: a complete list is the count's keep at min_neighbours = k
        _, _, m = cloud_eval.nearest_k(p, radius, k)
        assert np.array_equal(np.nonzero(m == k)[0], kept)
    d2, idx, m = cloud_eval.nearest_k(p, radius, 1)
    for i in (0, 1, 777, 1500, 2999):  # slot 0 at k = 1 is the search's answer in the cloud without the point
        want_d2, want_idx, _ = cloud_eval.nearest(p[i:i + 1], np.delete(p, i, axis=0), radius)
        j = int(want_idx[0])
        assert d2[i, 0].view(np.uint32) == want_d2[0].view(np.uint32) and idx[i, 0] == (j if j < i else j + (j >= 0))


@pytest.mark.gpu
def test_the_filter_equals_the_restatement(hip):
    share = _check_filter()
    r, f = filter_ref()
    p = cloud("sphere_halo")
    for grid in (0, 7):
        kept, ms, info = cloud_eval.drop_outliers(p, FILTER_RADIUS, FILTER_K, FILTER_STD, grid=grid, return_info=True)
        assert kept.dtype == np.int64 and np.array_equal(kept, np.nonzero(f.keep)[0])
        mask = np.zeros(len(p), dtype=np.uint8)
        mask[kept] = 1
        assert mask.tobytes() == f.keep.astype(np.uint8).tobytes()
        assert (info["mu"], info["sigma"], info["threshold"], info["short"]) == (f.mu, f.sigma, f.threshold, f.short)
        assert ms > 0 and info["complete"] == r.complete and info["not_finite"] == 0
    assert np.array_equal(cloud_eval.drop_outliers(torch.from_numpy(p).cuda(), FILTER_RADIUS, FILTER_K, FILTER_STD), kept)
    assert abs(float(np.isin(np.arange(N_SPHERE), kept).mean()) - share) < 1e-12
    # no complete list: nothing is kept
    kept, _, info = cloud_eval.drop_outliers(cloud("pair"), 1.0, 1, 1.0, return_info=True)
    assert len(kept) == 0 and kept.dtype == np.int64 and np.isnan(info["threshold"]) and info["short"] == 2


@pytest.mark.gpu
def test_score_with_the_filter_is_the_score_of_the_filtered_cloud(hip):
    keys, thin_keys, times = thin_cases.SCORE_KEYS, thin_cases.NEW_KEYS, thin_cases.TIMES
    count_keys = {"neighbour_radius", "min_neighbours", "cloud_points_before_filter", "filter_device_ms"}
    new_keys = {"outlier_radius", "outlier_k", "outlier_std", "outlier_threshold", "cloud_points_before_outliers", "outlier_device_ms"}
    rng = np.random.default_rng(17)
    cloud_pts = rng.uniform(0.0, 30.0, (4000, 3)).astype(f32)
    ref = rng.uniform(0.0, 30.0, (5000, 3)).astype(f32)
    plain = cloud_eval.score(cloud_pts, ref, max_dist=2.0)
    assert set(plain) == keys  # without the new arguments: key for key what it was
    assert set(cloud_eval.score(cloud_pts, ref, max_dist=2.0, neighbour_radius=2.0, min_neighbours=3)) == keys | count_keys
    for reduce, count in ((0.0, False), (1.0, False), (1.0, True)):
        idx = cloud_eval.thin(cloud_pts, reduce, seed=3) if reduce else np.arange(4000)
        if count:
            idx = idx[cloud_eval.drop_isolated(cloud_pts[idx], 2.0, 3)]
        kept, _, o = cloud_eval.drop_outliers(cloud_pts[idx], 3.0, 4, 0.5, return_info=True)
        assert 0.1 * len(idx) < len(kept) < 0.9 * len(idx)
        got, indices = cloud_eval.score(cloud_pts, ref, max_dist=2.0, reduce=reduce, seed=3, return_indices=True, outlier_radius=3.0,
                                        outlier_k=4, outlier_std=0.5, **(dict(neighbour_radius=2.0, min_neighbours=3) if count else {}))
        want = cloud_eval.score(cloud_pts[idx][kept], ref, max_dist=2.0)  # the reference is never filtered
        assert set(got) == keys | new_keys | (thin_keys if reduce else set()) | (count_keys if count else set())
        for k in keys - times:
            assert got[k] == want[k], k
        assert np.array_equal(indices, idx[kept]) and indices.dtype == np.int64  # the three stages compose
        assert (got["outlier_radius"], got["outlier_k"], got["outlier_std"], got["outlier_threshold"]) == (3.0, 4, 0.5, o["threshold"])
        assert got["cloud_points_before_outliers"] == len(idx) and got["cloud_points"] == len(kept) and got["outlier_device_ms"] > 0
        assert got["reference_points"] == 5000 and got["accuracy"] != plain["accuracy"]


@pytest.mark.gpu
def test_the_command_line_writes_the_cloud_it_scores(hip, tmp_path, capsys):
    """--reduce, both filters and --write_cloud in one call of main(): the file holds the surviving vertices of the input,
    every property of theirs, in the input's order; the report is the API's"""
    import json
    p = cloud("sphere_halo")
    v = neighbour_cases._own_vertices(len(p))
    v["x"], v["y"], v["z"] = p[:, 0], p[:, 1], p[:, 2]
    src, ref, out, rep = (str(tmp_path / n) for n in ("cloud.ply", "ref.ply", "out.ply", "report.json"))
    dmb.write_points_ply(src, v)
    dmb.write_points_ply(ref, v[:N_SPHERE:2])
    assert cloud_eval.main(["--cloud", src, "--reference", ref, "--max_dist", "5", "--reduce", "1.5", "--seed", "3",
                            "--neighbour_radius", "6", "--min_neighbours", "4", "--outlier_radius", "6", "--outlier_k", "8",
                            "--outlier_std", "1", "--write_cloud", out, "--output", rep]) == 0
    text = capsys.readouterr().out
    assert "standard deviations" in text and "dropped" in text
    thinned = cloud_eval.thin(p, 1.5, seed=3)
    counted = thinned[cloud_eval.drop_isolated(p[thinned], 6.0, 4)]
    idx = counted[cloud_eval.drop_outliers(p[counted], 6.0, 8, 1.0)]
    assert 1000 < len(idx) < len(counted) < len(thinned)
    assert dmb.read_ply_binary(out).tobytes() == v[idx].tobytes()
    report = json.load(open(rep))
    assert report["cloud_points"] == len(idx) and report["cloud_points_before"] == len(v) and report["outlier_k"] == 8
    assert report["cloud_points_before_filter"] == len(thinned) and report["cloud_points_before_outliers"] == len(counted)
    assert "%d -> %d points" % (len(counted), len(idx)) in text and "%d -> %d points" % (len(thinned), len(counted)) in text
