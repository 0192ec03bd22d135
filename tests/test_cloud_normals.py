"""A cloud's normals and surface variation from its k nearest neighbours, and the filter on the agreement of a cloud's own
normals with them (gipuma_hip_cloud_normals, gipuma_amd.cloud_eval.normals / estimate_normals /
normal_agreement / drop_disagreeing_normals).  Every case is a cloud, a radius, a k, a sign rule and a condition -- stated on
the restatement (tests/normals_ref.py) alone -- that it reaches the path it is named for; that condition runs without a
device, and so do the comparison of the restatement with numpy.linalg.eigh, six against seven sweeps, the C-ABI's argument
checks, the command lines and the assembly test.  GPU: normal and variation as uint32 bit patterns, m, the six entries of C as
uint64 patterns and the info counts equal the restatement at every grid; each output alone; the descriptor's stream; device
tensors; agreement with the lists and the neighbour count; the filter; the score with the filter; the command lines.

Measured on the restatement over the cases below (printed by test_the_restatement_agrees_with_eigh and
test_six_sweeps_are_a_fixed_point): the worst angle(normal, eigh's vector) * gap is 2.65 * 2^-52 and the worst variation error
0.84 * 2^-52 on top of the float32 rounding; the eigenvalues' bits stand after at most four sweeps, and six and seven sweeps
give the same bits on every case, the 300 001 points included."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
# torch before the `hip` fixture loads the library (see tests/test_cloud_scale.py): this module must also run on its own
import torch  # noqa: F401

from gipuma_amd import abi, cloud_eval, dmb
from tests import knn_ref, normals_ref
from tests import test_cloud_knn as knn_cases
from tests import test_cloud_neighbours as neighbour_cases
from tests import test_cloud_scale as scale
from tests import test_cloud_thin as thin_cases
from tests.abi_layout import assert_mirrors_header

f32, f64 = np.float32, np.float64
GRIDS = thin_cases.GRIDS
assert GRIDS == (0, 1, 2, 7, 256)
EPS = 2.0 ** -52
EIGH_BOUND = 64 * EPS  # allowed; 2.4 * 2^-52 was measured with these formulas on 20 000 random neighbourhoods: a 27-fold margin
N_SPHERE = neighbour_cases.N_SPHERE
SPHERE_RADIUS, SPHERE_K = 6.0, 8


# ----------------------------------------------------------------------------------------------------------------------
# The clouds (by name: several cases share one, and its brute force) and the cases
# ----------------------------------------------------------------------------------------------------------------------
def _plane():
    """2 000 distinct integer sites of a 2048 x 2048 plane at z = 5: d_z is exactly 0"""
    rng = np.random.default_rng(1919)
    sites = rng.choice(2048 * 2048, 2000, replace=False)
    return np.stack([sites % 2048, sites // 2048, np.full(2000, 5)], -1).astype(f64)


def _plane_matrix():
    """a rotation (about (1, 2, 3) by 0.7) rounded to multiples of 2^-7, as float32: with integer sites and an offset of
    65 536 every product and every sum below is exact in float32, so the moved points lie in one plane EXACTLY -- the plane
    spanned by the matrix's first two columns -- although a float32 near 65 536 has a spacing of 2^-7"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    return (np.round(R * 128) / 128).astype(f32)


def _plane_far():
    R, p = _plane_matrix(), _plane().astype(f32)
    out = np.zeros_like(p)
    for a in range(3):  # float32, term by term: exact (19-bit products, sums below 2^17 on a grid of 2^-7)
        out[:, a] = ((f32(65536.0) + R[a, 0] * p[:, 0]) + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]
    exact = 65536.0 + p.astype(f64) @ R.astype(f64).T
    assert out.dtype == f32 and np.array_equal(out.astype(f64), exact)
    return out


def _plane_axis():
    R = _plane_matrix().astype(f64)
    n = np.cross(R[:, 0], R[:, 1])
    return n / np.linalg.norm(n)


def _collinear():
    """500 points on the line t * (1, 2, 2), t multiples of 2^-10 below 10: exact in float32, exactly collinear"""
    t = np.sort(np.random.default_rng(2020).choice(10240, 500, replace=False)) / 1024.0
    return t[:, None] * np.array([1.0, 2.0, 2.0])


COLLINEAR_AXIS = np.array([1.0, 2.0, 2.0]) / 3.0
SCALES = ("radius_2^41", "radius_2^-41", "r2_infinite", "r2_zero")  # radius 2^41, 2^-41, 1e20, 1e-30

CLOUDS = {
    "plane": _plane,
    "plane_far": _plane_far,
    "collinear": _collinear,
    "sphere_floaters": lambda: neighbour_cases.cloud("sphere_floaters"),
    **{"points_%d" % n: functools.partial(lambda n: thin_cases._uniform(n, seed=303, box=4.0), n) for n in (0, 1, 3, 4, 5)},
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name in CLOUDS:
        return np.ascontiguousarray(CLOUDS[name](), dtype=f32).reshape(-1, 3)
    return knn_cases.cloud(name)


@functools.lru_cache(maxsize=None)
def lists(name, radius, k):
    """the brute force's lists of a cloud, computed once for every case that shares them (test_cloud_knn's at k = 32, cut)"""
    if name in CLOUDS:
        return knn_ref.knn(cloud(name), radius, k)
    return knn_ref.shorter(knn_cases.longest(name, f32(radius)), cloud(name), k)


class Case:
    def __init__(self, name, radius, k, check, orient=0, viewpoint=None, guide=None, eigh=True):
        self.name, self.radius, self.k, self.check = name, f32(radius), k, check
        self.orient, self.viewpoint, self.guide, self.eigh = orient, viewpoint, guide, eigh

    @property
    def points(self):
        return cloud(self.name)

    @functools.cached_property
    def ref(self):
        return self.restated()

    def restated(self, sweeps=normals_ref.SWEEPS):
        return normals_ref.normals(self.points, self.radius, self.k, self.orient, self.viewpoint,
                                   None if self.guide is None else self.guide(), lists(self.name, float(self.radius), self.k), sweeps)


def _unit(r, rows, tol=1e-6):
    return (np.abs(np.linalg.norm(r.normal[rows].astype(f64), axis=1) - 1.0) < tol).all()


def _case_uniform(k):
    def check(c):
        r, n = c.ref, len(c.points)
        counts = neighbour_cases.exact("uniform", c.radius)
        assert np.array_equal(r.m, np.minimum(counts, k)) and np.array_equal(r.is_estimated, counts >= 3)
        assert r.estimated >= 0.3 * n and r.short >= 0.1 * n and r.not_finite == 0, (r.estimated, r.short)  # both in one run
        assert c.k in (3, 4, 8, 9, 16, 17, 32) and _unit(r, r.is_estimated)  # either side of every boundary between the list lengths
        assert 0 < r.flipped < r.estimated and (r.normal[r.is_estimated][np.arange(r.estimated), np.abs(r.normal[r.is_estimated]).argmax(axis=1)] > 0).all()
    return Case("uniform", 1.5, k, check)


def _case_plane():
    def check(c):
        r = c.ref
        assert r.estimated >= 0.95 * len(c.points) and r.short >= 1
        est = r.is_estimated
        assert (r.normal[est].view(np.uint32) == np.array([0.0, 0.0, 1.0], f32).view(np.uint32)).all()  # (0, 0, 1) in every bit
        assert not r.variation[est].any() and not r.scatter[:, [2, 4, 5]].any() and r.flipped == 0
    return Case("plane", 100.0, 8, check)


def _case_plane_far():
    def check(c):
        r, axis = c.ref, _plane_axis()
        assert r.estimated >= 0.95 * len(c.points)  # (the rounded matrix stretches by up to 0.5 %: nearly the plane's neighbourhoods)
        assert c.points.min() > 65536 - 2900 and np.spacing(f32(65536.0)) == 2.0 ** -7
        est = r.is_estimated
        w = np.sort(r.w[est], axis=1)
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
        angle = np.linalg.norm(np.cross(r.vector[est], axis), axis=1)
        assert (angle * gap <= EIGH_BOUND).all(), float((angle * gap).max() / EPS)
        assert (r.variation[est] < 1e-6).all() and (np.abs(r.normal[est].astype(f64) @ axis) > 1 - 1e-6).all()
    return Case("plane_far", 100.0, 8, check)


def _radial():
    p = cloud("sphere_floaters").astype(f64)
    return (p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-30)).astype(f32)  # (a floater stands at the origin: a zero guide)


def _case_sphere(kind):
    def check(c):
        r, p = c.ref, c.points.astype(f64)
        own = np.arange(len(p)) < N_SPHERE
        assert r.is_estimated[own].all() and not r.is_estimated[~own].any()  # every floater is short (the clumps: m = 2)
        along = (r.normal.astype(f64) * p).sum(axis=1) / np.maximum(np.linalg.norm(p, axis=1), 1e-30)  # (a floater stands at the origin)
        assert (np.abs(along[own]) > 0.8).all()  # the estimate is within 37 degrees of the radial direction everywhere
        if kind == "centre":  # every estimated normal points inward
            assert (along[own] < 0).all() and 0 < r.flipped < N_SPHERE
        elif kind == "outside":
            # A viewpoint outside sees the cap facing it from outside and the rest of the sphere from inside: towards it the
            # normal is outward on the cap p . v > |p|^2 and inward elsewhere -- asserted clear of the rim by the 37 degrees above:
            # cos(radial, v - p) = |p| (side - 1) / |v - p| is beyond sin(37 degrees) = 0.6 where |side - 1| > 20
            v = np.asarray(c.viewpoint, f64)
            toward = ((v - p) * r.normal.astype(f64)).sum(axis=1)
            assert (toward[own] > 0).all()
            side = (p * v).sum(axis=1) / np.maximum((p * p).sum(axis=1), 1e-30)
            assert (along[own & (side > 21)] > 0).all() and (along[own & (side < -19)] < 0).all()
            assert (own & (side > 21)).sum() > 500 and (own & (side < -19)).sum() > 500
        else:  # the radial direction as guide: outward everywhere, the viewpoint-at-the-centre result negated bit for bit
            assert (along[own] > 0).all()
            inward = case("sphere_centre").ref
            assert np.array_equal((-inward.normal[own]).view(np.uint32), r.normal[own].view(np.uint32))
            assert r.flipped == N_SPHERE - inward.flipped
    extra = {"centre": dict(orient=1, viewpoint=(0.0, 0.0, 0.0)), "outside": dict(orient=1, viewpoint=(1500.0, 400.0, -300.0)),
             "guide": dict(orient=2, guide=_radial)}[kind]
    return Case("sphere_floaters", SPHERE_RADIUS, SPHERE_K, check, **extra)


def _case_lattice(permuted, k):
    def check(c):
        r, p = c.ref, c.points
        inner = ((p > 0) & (p < 6)).all(axis=1)
        assert r.is_estimated.all() and inner.sum() == 125
        if k == 18:  # a full neighbourhood (6 + 12 sites): C is a multiple of the identity, nothing rotates, the tie goes to axis 0
            s = r.scatter[inner]
            assert (s[:, [1, 2, 4]] == 0).all() and (s[:, 0] == s[:, 3]).all() and (s[:, 0] == s[:, 5]).all()
            assert (r.normal[inner] == np.array([1, 0, 0], f32)).all() and (r.variation[inner] == f32(1.0 / 3.0)).all()
            ties = (r.w[:, 0] == r.w[:, 1]) | (r.w[:, 1] == r.w[:, 2]) | (r.w[:, 0] == r.w[:, 2])
            assert ties.sum() >= 200  # faces and edges tie two eigenvalues
            if permuted:  # integer sums are exact in any order: the permutation changes nothing but the order
                plain = case("lattice_k18").ref
                for got, want in ((r.normal, plain.normal), (r.variation, plain.variation), (r.scatter, plain.scatter), (r.m, plain.m)):
                    assert np.array_equal(got, want[knn_cases.LATTICE_PERMUTATION])
    return Case("lattice_permuted" if permuted else "lattice", 1.5, k, check, eigh=False)  # (its ties are the point)


def _case_collinear():
    def check(c):
        r = c.ref
        assert r.estimated >= 0.9 * len(c.points) and r.estimated + r.short == len(c.points)
        est = r.is_estimated
        assert (np.abs(r.normal[est].astype(f64) @ COLLINEAR_AXIS) < 1e-6).all() and _unit(r, est)
        assert (r.variation[est] < 1e-6).all()
    return Case("collinear", 0.3, 8, check)  # (two eigenvalues are 0 up to rounding: the gap condition leaves the eigh test no point)


def _case_identical():
    def check(c):
        r = c.ref
        assert r.estimated == 0 and r.short == 41 and (r.m[:40] == 8).all() and r.m[40] == 0  # all degenerate; the far point short
        assert not r.normal.any() and np.isposinf(r.variation).all() and not r.scatter.any()
    return Case("identical", 1.0, 8, check)


def _case_non_finite():
    def check(c):
        r, p = c.ref, c.points
        bad = ~np.isfinite(p).all(axis=1)
        assert bad.sum() == 30 == r.not_finite and all((~np.isfinite(p[bad][:, a])).any() for a in range(3)) and np.isnan(p[bad]).any()
        assert not r.m[bad].any() and not r.normal[bad].any() and np.isposinf(r.variation[bad]).all() and not r.scatter[bad].any()
        assert r.estimated > 100 and r.short > 100 and np.isfinite(r.normal).all()
    return Case("non_finite", 1.5, 4, check)


def _case_count(n):
    def check(c):  # every point within the radius of every other: n - 1 neighbours each
        r = c.ref
        assert len(c.points) == n and (r.m == min(3, max(n - 1, 0))).all()
        assert (r.estimated, r.short) == ((n, 0) if n >= 4 else (0, n))  # the triple has m = 2: short
    return Case("points_%d" % n, 10.0, 3, check)


def _case_pair():
    def check(c):
        assert c.ref.m.tolist() == [1, 1] and c.ref.short == 2 and not c.ref.normal.any()
    return Case("pair", 5.0, 3, check)


def _case_scale(name):
    t = scale.thin_case(name)

    def check(c):
        t.check(t)
        r, n = c.ref, len(c.points)
        assert tuple(g for g in GRIDS if scale.thin_layout(c, g)[1]) == tuple(t.one_cell) == GRIDS  # one cell at every grid
        if name == "r2_infinite":
            # the 400 ordinary points list ordinary neighbours.  The two at +-3e38 list the points 0 .. 7 at differences near
            # 3e38, whose squares are about 1e77 in a double: finite, estimated.  Nothing here overflows a double; a float32
            # difference that overflows (between the far two) is in no list
            assert r.estimated == n == 402 and np.isfinite(r.scatter).all() and r.scatter[400:].max() > 1e77
        elif name == "r2_zero":
            assert (r.m == 1).all() and r.short == n and r.estimated == 0  # only the copy is a neighbour
        else:
            assert r.estimated >= 0.9 * n and np.isfinite(r.normal).all() and _unit(r, r.is_estimated)
    return Case("scale_" + name, t.radius, 8, check)


def _overflow_cloud():
    """four points whose float32 differences overflow to +-inf: the sums are inf, C is inf - inf, the trace is not finite"""
    return np.array([[3e38, 0, 0], [-3e38, 1, 0], [3e38, 0, 2], [-3e38, 3, 3], [-3e38, 0, 1]], dtype=f32)


CLOUDS["overflow"] = _overflow_cloud


def _case_overflow():
    def check(c):
        r = c.ref
        assert np.isposinf(knn_ref.squared(c.radius)) and (r.m == 4).all()
        assert r.estimated == 0 and r.short == 5 and not r.normal.any() and np.isposinf(r.variation).all()  # degenerate
        assert np.isnan(r.scatter).any() and (r.scatter.view(np.uint64)[np.isnan(r.scatter)] == normals_ref.CANONICAL_NAN).all()
    return Case("overflow", 1e20, 4, check)


GUIDES = np.array([[0, 0, -1], [0, 0, 0], [np.nan, 0, 0], [1, 1, 0], [0, 0, 1], [0, np.inf, 1]], dtype=f32)


def _case_guide():
    def check(c):
        r, row = c.ref, np.arange(len(c.points)) % len(GUIDES)
        est = r.is_estimated
        # against the plane's (0, 0, 1): opposed, zero, NaN, exactly perpendicular, along, infinite -- only the first flips;
        # where the dot is 0 or not finite rule 0 applies and keeps (0, 0, 1)
        assert np.array_equal(r.is_flipped, est & (row == 0)) and r.flipped == int((est & (row == 0)).sum()) > 300
        assert (r.normal[est & (row != 0)] == np.array([0, 0, 1], f32)).all() and (r.normal[est & (row == 0)][:, 2] == -1).all()
    return Case("plane", 100.0, 8, check, orient=2, guide=lambda: GUIDES[np.arange(2000) % len(GUIDES)])


BUILDERS = {
    **{"uniform_k%d" % k: functools.partial(_case_uniform, k) for k in (3, 4, 8, 9, 16, 17, 32)},
    "plane": _case_plane,
    "plane_far": _case_plane_far,
    **{"sphere_" + kind: functools.partial(_case_sphere, kind) for kind in ("centre", "outside", "guide")},
    **{"lattice_k%d" % k: functools.partial(_case_lattice, False, k) for k in (8, 18)},
    **{"lattice_permuted_k%d" % k: functools.partial(_case_lattice, True, k) for k in (8, 18)},
    "collinear": _case_collinear,
    "identical": _case_identical,
    "non_finite": _case_non_finite,
    **{"points_%d" % n: functools.partial(_case_count, n) for n in (0, 1, 3, 4, 5)},
    "pair": _case_pair,
    **{"scale_" + name: functools.partial(_case_scale, name) for name in SCALES},
    "overflow": _case_overflow,
    "guide": _case_guide,
}
GAP_SHARE_CASES = ("sphere_centre", "plane_far", "uniform_k8")  # the sphere, the tilted plane, the uniform box


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# the large cloud: test_cloud_scale's 300 001 points, against the sparse restatement (test_cloud_knn's radius and k)
LARGE_RADIUS, LARGE_K = knn_cases.LARGE_RADIUS, knn_cases.LARGE_K
assert (LARGE_RADIUS, LARGE_K) == (0.45, 8)


@functools.lru_cache(maxsize=None)
def large_ref():
    r = knn_cases.large_ref()  # knn_ref's cKDTree path, as test_cloud_knn.py takes it
    return normals_ref.from_lists(scale.large_clouds()[1], r.idx, r.m, LARGE_K)


def _check_large():
    r = large_ref()
    assert r.not_finite == 0 and r.estimated + r.short == scale.N_LARGE
    assert r.estimated >= 0.2 * scale.N_LARGE and r.short >= 0.2 * scale.N_LARGE, (r.estimated, r.short)
    assert scale.N_LARGE > 1000 * 256  # a launch of more than 1 000 workgroups


# the filter: the sphere with its radial normals, 200 of them tilted by 60 degrees, and the 63 floaters
FILTER_ANGLE, N_TILTED = 30.0, 200


@functools.lru_cache(maxsize=None)
def filter_normals():
    """(the cloud's own normals, the tilted rows): radial everywhere, 200 of the sphere's rows turned 60 degrees towards a tangent"""
    g = _radial().astype(f64)
    rows = np.sort(np.random.default_rng(3030).choice(N_SPHERE, N_TILTED, replace=False))
    tangent = np.cross(g[rows], np.array([0.3, -0.5, 0.8]))
    tangent /= np.linalg.norm(tangent, axis=1, keepdims=True)
    g[rows] = np.cos(np.pi / 3) * g[rows] + np.sin(np.pi / 3) * tangent
    return g.astype(f32), rows


@functools.lru_cache(maxsize=None)
def filter_ref():
    r = normals_ref.normals(cloud("sphere_floaters"), SPHERE_RADIUS, SPHERE_K, lists=lists("sphere_floaters", SPHERE_RADIUS, SPHERE_K))
    return r, normals_ref.keep_agreeing(r, filter_normals()[0], FILTER_ANGLE)


def _check_filter():
    """returns the share of the untouched points that survive: a property of the case, printed, not fixed beforehand"""
    (r, keep), (given, rows) = filter_ref(), filter_normals()
    n = len(cloud("sphere_floaters"))
    assert n == N_SPHERE + 63 and not keep[rows].any() and not keep[N_SPHERE:].any()  # every tilted point and every floater is dropped
    assert not r.is_estimated[N_SPHERE:].any()  # the floaters: as short
    agree = normals_ref.agreement(r.normal, given)
    assert (agree[rows] < 0.75).all() and agree[rows].min() > 0.2  # 60 degrees, give or take the estimate's own error
    untouched = np.setdiff1d(np.arange(N_SPHERE), rows)
    share = float(keep[untouched].mean())
    print("the normal filter at radius %g, k %d, %g degrees: all %d tilted points and all 63 floaters dropped, %.4f of the %d untouched "
          "points survive (their worst agreement %.4f)" % (SPHERE_RADIUS, SPHERE_K, FILTER_ANGLE, N_TILTED, share, len(untouched),
                                                          agree[untouched].min()))
    return share


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    r, n = c.ref, len(c.points)
    assert r.normal.shape == (n, 3) and r.scatter.shape == (n, 6)
    assert (r.normal.dtype, r.variation.dtype, r.m.dtype, r.scatter.dtype) == (f32, f32, np.uint32, f64)
    assert r.estimated + r.short + r.not_finite == n and r.estimated == int(r.is_estimated.sum()) and r.flipped <= r.estimated
    assert not r.normal[~r.is_estimated].any() and np.isposinf(r.variation[~r.is_estimated]).all()
    assert (r.m[r.is_estimated] >= 3).all() and not r.scatter[r.m < 3].any()
    v = r.variation[r.is_estimated]
    assert ((v >= 0) & (v <= f32(1.0 / 3.0) * (1 + 1e-6))).all() and _unit(r, r.is_estimated)
    assert np.array_equal(r.m, knn_ref.knn(c.points, c.radius, c.k).m)  # the brute force at this k itself


def test_the_large_cloud_reaches_its_paths():
    _check_large()


def test_the_filter_case_reaches_its_paths():
    assert 0.9 < _check_filter() <= 1.0


def _eigh_figures(r):
    """(angle * gap, variation error in units of the bound's two terms, the share excluded by the gap) over the estimated points"""
    est = np.nonzero(r.is_estimated)[0]
    s = r.scatter[est]
    full = np.zeros((len(est), 3, 3))
    for e, (a, b) in enumerate(normals_ref.TRIANGLE):
        full[:, a, b] = full[:, b, a] = s[:, e]
    lam, vec = np.linalg.eigh(full)
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    on = gap > 1e-6
    angle = np.linalg.norm(np.cross(r.vector[est][on], vec[on][:, :, 0]), axis=1)  # sin of the angle: the angle, at this size
    want = np.maximum(lam[on, 0], 0.0) / ((lam[on, 0] + lam[on, 1]) + lam[on, 2])
    err = np.abs(r.variation[est][on].astype(f64) - want) - 2.0 ** -24 * want  # half a float32 ulp, the conversion's rounding, is taken off
    return angle * gap[on], err, 1.0 - float(on.mean()) if len(est) else 0.0


def test_the_restatement_agrees_with_eigh():
    """For every estimated point whose relative gap g = (l1 - l0) / l2 is above 1e-6: angle(the restatement's float64 vector,
    numpy.linalg.eigh's first vector of the same C) * g <= 64 * 2^-52.  The variation, a float32, is bounded the same way:
    |variation - l0 / (l0 + l1 + l2)| <= 2^-24 of that value (half a float32 ulp: the correctly rounded conversion) + 64 * 2^-52
    (both methods' eigenvalues carry errors of a few 2^-52 of the trace, and the variation is an eigenvalue over the trace).
    Only the lattice is left out whole; everywhere else the gap condition decides point by point (it leaves none of the
    collinear points, and the copies have no estimate)."""
    worst_angle, worst_variation = 0.0, 0.0
    for name in sorted(BUILDERS) + ["large"]:
        if name != "large" and not case(name).eigh:
            continue  # the lattice, excluded whole: its ties are the point
        r = large_ref() if name == "large" else case(name).ref
        if not r.estimated:
            continue
        angle_gap, err, excluded = _eigh_figures(r)
        if len(angle_gap):
            worst_angle, worst_variation = max(worst_angle, float(angle_gap.max())), max(worst_variation, float(err.max()))
            assert angle_gap.max() <= EIGH_BOUND, (name, float(angle_gap.max() / EPS))
            assert err.max() <= EIGH_BOUND, (name, float(err.max() / EPS))
        if name in GAP_SHARE_CASES:
            assert excluded <= 0.05, (name, excluded)
            print("%s: %.4f of the estimated points excluded by the gap condition" % (name, excluded))
    print("worst angle * gap %.2f * 2^-52, worst variation error beyond the float32 rounding %.2f * 2^-52" % (worst_angle / EPS, worst_variation / EPS))
    assert [n for n in BUILDERS if not case(n).eigh] == [n for n in BUILDERS if n.startswith("lattice")]  # (excluded, and says so)


def test_six_sweeps_are_a_fixed_point():
    """six and seven sweeps of the restatement give the same bits on every case; the number of sweeps after which the
    off-diagonal entries are exactly 0 is printed (DESIGN.md 19 records it)"""
    needed = 0
    for name in sorted(BUILDERS) + ["large"]:
        if name == "large":
            k = knn_cases.large_ref()
            six, seven = large_ref(), normals_ref.from_lists(scale.large_clouds()[1], k.idx, k.m, LARGE_K, sweeps=7)
        else:
            six, seven = case(name).ref, case(name).restated(sweeps=7)
        assert np.array_equal(six.normal.view(np.uint32), seven.normal.view(np.uint32)), name
        assert np.array_equal(six.variation.view(np.uint32), seven.variation.view(np.uint32)), name
        est = six.is_estimated
        if est.any() and name != "large":
            full = np.zeros((int(est.sum()), 3, 3))
            for e, (a, b) in enumerate(normals_ref.TRIANGLE):
                full[:, a, b] = six.scatter[est][:, e]
            for sweeps in range(1, 7):
                w, _ = normals_ref.jacobi(full, sweeps)
                if np.array_equal(w, six.w[est]):
                    needed = max(needed, sweeps)
                    break
            else:
                raise AssertionError(name)
    print("the eigenvalues' bits stand after at most %d sweeps" % needed)
    assert needed <= 5


def test_the_restatement_turns_down_what_the_library_turns_down():
    p = cloud("points_5")
    for k in (2, 33, 0, 2.5):
        with pytest.raises(ValueError):
            normals_ref.normals(p, 1.0, k)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            normals_ref.normals(p, radius, 3)
    for bad in (dict(orient=3), dict(orient=2), dict(orient=1), dict(orient=1, viewpoint=(0.0, float("nan"), 0.0))):
        with pytest.raises(ValueError):
            normals_ref.normals(p, 1.0, 3, **bad)
    for bad in (-1.0, 91.0, float("nan")):
        with pytest.raises(ValueError):
            cloud_eval.drop_disagreeing_normals(p, p, 1.0, 3, bad)
    with pytest.raises(ValueError, match="viewpoint"):  # (not the descriptor's zeros: the wrapper is as strict as the restatement)
        cloud_eval.normals(p, 1.0, 3, orient=1)


def test_normal_agreement():
    e = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1], [0.6, 0, 0.8]], f32)
    g = np.array([[0, 0, -2], [1, 0, 0], [0, 0, 0], [0, 0, 1], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, 3]], f32)
    got = cloud_eval.normal_agreement(e, g)
    assert got.dtype == f64 and got[:6].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and abs(got[6] - float(f32(0.8))) < 1e-15
    assert np.array_equal(got, normals_ref.agreement(e, g))
    given, _ = filter_normals()
    r, _ = filter_ref()
    assert np.array_equal(cloud_eval.normal_agreement(r.normal, given), normals_ref.agreement(r.normal, given))
    with pytest.raises(ValueError):
        cloud_eval.normal_agreement(e, g[:3])


def _desc(**kw):
    d = abi.NormalsDesc()
    d.abi_version, d.n_points, d.points, d.radius, d.k = abi.ABI_VERSION, 4, 0x1000, 1.0, 8
    d.grid, d.orient, d.guide, d.device_id, d.stream = 0, 0, None, 0, None
    for k, v in kw.items():
        setattr(d, k, (C.c_float * 3)(*v) if k == "viewpoint" else v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last ones for want of a device when there is
    none -- with a device they are not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(normal=out, variation=out, count=out, scatter=out, **kw):
        return lib.gipuma_hip_cloud_normals(C.byref(_desc(**kw)), normal, variation, count, scatter, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(radius=bad) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    for bad in (2, 33, 0, -1):
        assert rc(k=bad) == abi.ERR_ARG and b"k must be 3..32" in lib.gipuma_hip_last_error()
    for bad in (3, -1):
        assert rc(orient=bad) == abi.ERR_ARG and b"orient" in lib.gipuma_hip_last_error()
    assert rc(orient=2) == abi.ERR_ARG and b"guide" in lib.gipuma_hip_last_error()
    for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("-inf"))):
        assert rc(orient=1, viewpoint=bad) == abi.ERR_ARG and b"viewpoint" in lib.gipuma_hip_last_error()
    assert rc(k=2, radius=0.0) == abi.ERR_ARG and b"radius" in lib.gipuma_hip_last_error()  # (the thinning's order)
    assert rc(k=2, grid=300) == abi.ERR_ARG and b"k must" in lib.gipuma_hip_last_error()
    assert rc(points=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(normal=None, variation=None, count=None, scatter=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(n_points=-1) == abi.ERR_ARG
    assert rc(n_points=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_normals(None, out, out, out, out, None, None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        for valid in (dict(), dict(k=3), dict(k=32), dict(normal=None, variation=None, count=None), dict(variation=None, scatter=None),
                      dict(orient=1, viewpoint=(1, 2, 3)), dict(orient=2, guide=0x5000), dict(viewpoint=(float("nan"), 0, 0)),
                      dict(n_points=0, points=None, normal=None, variation=None, count=None, scatter=None)):
            assert rc(**valid) == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        for call in (lambda: cloud_eval.estimate_normals(np.zeros((4, 3), f32), 1.0, 3),
                     lambda: cloud_eval.drop_disagreeing_normals(np.zeros((4, 3), f32), np.zeros((4, 3), f32), 1.0, 3, 30.0),
                     lambda: cloud_eval.normals(np.zeros((4, 3), f32), 1.0, 3)):
            with pytest.raises(abi.GipumaHipError, match="no CPU fallback"):
                call()
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.NormalsDesc, "gipuma_hip_normals_desc",
                          ["abi_version", "n_points", "points", "radius", "k", "grid", "orient", "viewpoint", "guide", "device_id", "stream"])
    assert "gipuma_hip_cloud_normals" in [s[0] for s in abi.SYMBOLS]
    new = ("orient", "viewpoint", "guide")  # laid out like the lists' descriptor, the new fields after `grid`
    assert [f[0] for f in abi.NormalsDesc._fields_ if f[0] not in new] == [f[0] for f in abi.KnnDesc._fields_]
    assert [f[0] for f in abi.NormalsDesc._fields_][5:9] == ["grid"] + list(new)


CLI = ["--cloud", "c.ply", "--reference", "r.ply"]
ON = ["--normal_radius", "1", "--normal_k", "8", "--max_normal_angle", "30"]
_without, _with = knn_cases._without, knn_cases._with


@pytest.mark.parametrize("argv", [CLI + _without(ON, o) for o in ON[::2]] + [CLI + ON[2 * i:2 * i + 2] for i in range(3)] +
                         [CLI + _with(ON, "--normal_radius", v) for v in ("0", "-1", "nan", "inf")] +
                         [CLI + _with(ON, "--normal_k", v) for v in ("2", "33", "-1", "2.5")] +
                         [CLI + _with(ON, "--max_normal_angle", v) for v in ("-1", "91", "nan")] +
                         [CLI + ON + ["--estimated_normals"], CLI + ["--estimated_normals", "--write_cloud", "o.ply"],
                          CLI + ["--estimated_normals", "--write_cloud", "o.ply", "--normal_radius", "1"],
                          CLI + ["--estimated_normals", "--write_cloud", "o.ply", "--normal_radius", "1", "--normal_k", "2"]])
def test_cli_normal_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_normal_arguments():
    a = cloud_eval.parse_args(CLI)
    assert (a.normal_radius, a.normal_k, a.max_normal_angle, a.estimated_normals) == (0.0, 0, None, False)
    a = cloud_eval.parse_args(CLI + ["--normal_radius", "0.1", "--normal_k", "32", "--max_normal_angle", "0", "--write_cloud", "out.ply"])
    assert (a.normal_radius, a.normal_k, a.max_normal_angle) == (float(f32(0.1)), 32, 0.0) and a.write_cloud == "out.ply"  # (through float32)
    a = cloud_eval.parse_args(CLI + ON + ["--write_cloud", "o.ply", "--estimated_normals", "--component_radius", "1", "--min_component", "3"])
    assert (a.normal_radius, a.normal_k, a.max_normal_angle, a.estimated_normals) == (1.0, 8, 30.0, True)
    a = cloud_eval.parse_args(CLI + ON[:4] + ["--write_cloud", "o.ply", "--estimated_normals"])  # the estimate alone: nothing is dropped
    assert (a.normal_radius, a.normal_k, a.max_normal_angle, a.estimated_normals) == (1.0, 8, None, True)


def test_batch_normal_arguments(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    on = ["--fuse_normal_radius", "0.1", "--fuse_normal_k", "16", "--fuse_max_normal_angle", "25"]
    a = batch.parse_args(base)
    assert (a.fuse_normal_radius, a.fuse_normal_k, a.fuse_max_normal_angle) == (0.0, 0, 0.0)
    a = batch.parse_args(base + ["--fuse"] + on + ["--fuse_component_radius", "1", "--fuse_min_component", "8"])
    assert (a.fuse_normal_radius, a.fuse_normal_k, a.fuse_max_normal_angle, a.fuse_min_component) == (float(f32(0.1)), 16, 25.0, 8)
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + on)
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    for bad in ([_without(on, o) for o in on[::2]] + [_with(on, "--fuse_normal_radius", v) for v in ("-1", "nan")] +
                [_with(on, "--fuse_normal_k", v) for v in ("2", "33")] + [_with(on, "--fuse_max_normal_angle", "91")]):
        with pytest.raises(SystemExit) as e:
            batch.parse_args(base + ["--fuse"] + bad)
        assert e.value.code == 2
    capsys.readouterr()


def test_a_cloud_file_without_normals_is_refused_before_anything_is_computed(tmp_path, monkeypatch):
    v = np.zeros(5, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
    src = str(tmp_path / "bare.ply")
    dmb.write_ply_vertices(src, v)
    monkeypatch.setattr(cloud_eval, "score", lambda *a, **k: pytest.fail("computed"))
    with pytest.raises(ValueError, match="nx, ny, nz"):
        cloud_eval.main(["--cloud", src, "--reference", src] + ON)


def test_score_without_the_new_arguments_builds_the_report_it_builds_today(monkeypatch):
    """score() with the search replaced by the search's restatement, so that it runs without a device: the keys are those of
    before the filter, and the new arguments are refused where they are wrong before anything is computed"""
    from tests import cloud_ref

    def nearest(queries, targets, max_dist, grid=0, device_id=0, return_info=False):
        r = cloud_ref.nearest(queries, targets, max_dist)
        return r.d2, r.idx, 0.5, dict(found=r.found, none=r.none, **{k: 1 for k in cloud_eval._STATS})

    monkeypatch.setattr(cloud_eval, "nearest", nearest)
    rng = np.random.default_rng(17)
    a, b = rng.uniform(0.0, 5.0, (60, 3)).astype(f32), rng.uniform(0.0, 5.0, (70, 3)).astype(f32)
    plain = cloud_eval.score(a, b, max_dist=2.0)
    assert set(plain) == thin_cases.SCORE_KEYS and plain["cloud_points"] == 60
    assert cloud_eval.score(a, b, max_dist=2.0, normal_radius=0.0, normal_k=0, max_normal_angle=0.0, cloud_normals=None) == plain
    for bad in (dict(normal_radius=-1.0), dict(normal_radius=float("nan")), dict(normal_radius=1.0, normal_k=2, max_normal_angle=30.0, cloud_normals=a),
                dict(normal_radius=1.0, normal_k=33, max_normal_angle=30.0, cloud_normals=a),
                dict(normal_radius=1.0, normal_k=8, max_normal_angle=91.0, cloud_normals=a),
                dict(normal_radius=1.0, normal_k=8, max_normal_angle=30.0), dict(normal_radius=1.0, normal_k=8, max_normal_angle=30.0, cloud_normals=b)):
        with pytest.raises(ValueError):
            cloud_eval.score(a, b, max_dist=2.0, **bad)


def test_the_kernels_use_global_memory_instructions_integer_atomics_and_no_float32_contraction():
    """(the float64 fused operations in the assembly are the compiler's own correctly rounded `/` and sqrt: expected, allowed)"""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "c.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--offload-device-only", "-o", out, "gipuma_normals.hip"],
                              cwd=os.path.join(root, "gipuma_amd", "csrc"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    assert "_ZN3nrm12clear_kernel" in asm
    for K in (8, 16, 32):
        assert "_ZN3nrm15estimate_kernelILi%dEEE" % K in asm
    assert "_ZN5cloud" not in asm.replace("N5cloud3RecE", "").replace("NS1_4GridE", "").replace("NS0_4GridE", "")  # the set-up kernels are defined once, elsewhere
    ops = [l.split()[0] for l in asm.splitlines() if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")]
    assert not [o for o in ops if o.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_pk_fma_f32"))]
    assert {o for o in ops if "atomic" in o} == {"global_atomic_add"}
    assert ".private_segment_fixed_size: 0" in asm and ".private_segment_fixed_size: " not in asm.replace(".private_segment_fixed_size: 0\n", "")


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _assert_equals_ref(normal, variation, m, scatter, info, r, what):
    """normal and variation as uint32 bit patterns, the entries of C as uint64 ones; each output may be None (not asked for)"""
    if normal is not None:
        assert normal.dtype == torch.float32 and tuple(normal.shape) == r.normal.shape, what
        got, want = normal.cpu().numpy().view(np.uint32), r.normal.view(np.uint32)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert not len(bad), "%s: the normal differs at %d points, first %d: %s for %s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    if variation is not None:
        got, want = variation.cpu().numpy().view(np.uint32), r.variation.view(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), "%s: the variation differs at %d points, first %d: %08x for %08x" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    if m is not None:
        assert np.array_equal(m.cpu().numpy().view(np.uint32), r.m), what
    if scatter is not None:
        assert scatter.dtype == torch.float64 and tuple(scatter.shape) == r.scatter.shape, what
        bad = np.nonzero((scatter.cpu().numpy().view(np.uint64) != r.scatter.view(np.uint64)).any(axis=1))[0]
        assert not len(bad), "%s: C differs at %d points, first %d" % (what, len(bad), bad[0])
    assert (info["estimated"], info["short"], info["not_finite"], info["flipped"]) == (r.estimated, r.short, r.not_finite, r.flipped), what


def _run(c, grid=0, **kw):
    return cloud_eval.normals(c.points, c.radius, c.k, c.orient, c.viewpoint, None if c.guide is None else c.guide(), grid=grid, **kw)


GPU_RUNS = [(name, g) for name in sorted(BUILDERS) for g in GRIDS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_the_kernel_equals_the_restatement_in_every_bit(hip, name, grid):
    c = case(name)
    c.check(c)
    what = "%s at grid %d" % (name, grid)
    normal, variation, m, scatter, ms, info = _run(c, grid, scatter=True)
    _assert_equals_ref(normal, variation, m, scatter, info, c.ref, what)
    if np.isfinite(c.points).all(axis=1).any():
        assert ms > 0
        G, one_cell = scale.thin_layout(c, grid)  # the thinning's documented rule, not asked of the library
        assert info["grid"] == G, "%s: the library reports %d cells" % (what, info["grid"])
        if one_cell:
            assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)
    else:
        assert info["grid"] == 0 and info["estimated"] == 0
    got = cloud_eval.estimate_normals(c.points, c.radius, c.k, c.orient, c.viewpoint, None if c.guide is None else c.guide(), grid=grid)
    assert [a.dtype for a in got] == [f32, f32] and got[0].shape == (len(c.points), 3)  # the public function: numpy
    assert np.array_equal(got[0].view(np.uint32), c.ref.normal.view(np.uint32)), what
    assert np.array_equal(got[1].view(np.uint32), c.ref.variation.view(np.uint32)), what


@pytest.mark.gpu
def test_large_cloud_equals_the_sparse_restatement(hip):
    _check_large()
    b = scale.large_clouds()[1]
    normal, variation, m, scatter, ms, info = cloud_eval.normals(b, LARGE_RADIUS, LARGE_K, scatter=True)
    _assert_equals_ref(normal, variation, m, scatter, info, large_ref(), "300 001 points")
    assert info["grid"] == 256


@pytest.mark.gpu
def test_each_output_alone(hip):
    for name in ("uniform_k8", "uniform_k17", "sphere_guide"):
        c = case(name)
        for alone in range(4):
            switches = [i == alone for i in range(4)]
            outs = _run(c, normal=switches[0], variation=switches[1], count=switches[2], scatter=switches[3])
            assert [o is not None for o in outs[:4]] == switches
            _assert_equals_ref(*outs[:4], outs[5], c.ref, "%s, output %d alone" % (name, alone))


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_runs_repeat(hip):
    c = case("sphere_guide")
    pts, guide = torch.from_numpy(c.points).cuda(), torch.from_numpy(c.guide()).cuda()
    runs = []
    for _ in range(2):  # (the order inside a cell varies from run to run; the lists and what follows from them do not)
        outs = cloud_eval.normals(pts, c.radius, c.k, 2, None, guide, scatter=True)
        assert all(t.is_cuda for t in outs[:4])
        _assert_equals_ref(*outs[:4], outs[5], c.ref, "device tensors")
        runs.append(b"".join(t.cpu().numpy().tobytes() for t in outs[:4]))
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_normals_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the cloud was written just before, the device not synchronised: the library runs
    behind it on that stream.  Two cloud sizes one after the other on the same stream; then n = 0."""
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("uniform_k9", "sphere_centre"):
        c = case(name)
        n = len(c.points)
        staged = torch.from_numpy(c.points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the cloud the library reads: a device copy queued on the caller's stream
            pts = staged.clone()
            normal = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            variation = torch.empty(n, dtype=torch.float32, device="cuda")
            m = torch.empty(n, dtype=torch.int32, device="cuda")
            scatter = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        d = _desc(n_points=n, points=pts.data_ptr(), radius=float(c.radius), k=c.k, orient=c.orient, viewpoint=c.viewpoint or (0, 0, 0),
                  stream=stream.cuda_stream)
        info, ms = (C.c_int64 * 8)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_normals(C.byref(d), normal.data_ptr(), variation.data_ptr(), m.data_ptr(), scatter.data_ptr(),
                                                    info, C.byref(ms)), "normals")
        got = dict(estimated=info[0], short=info[1], not_finite=info[2], flipped=info[3])
        _assert_equals_ref(normal, variation, m, scatter, got, c.ref, "%s on the caller's stream" % name)
        assert ms.value > 0
    info = (C.c_int64 * 8)(*([7] * 8))
    abi.check(lib, lib.gipuma_hip_cloud_normals(C.byref(_desc(n_points=0, points=None)), None, None, None, None, info, None), "nothing")
    assert list(info) == [0] * 8


@pytest.mark.gpu
def test_agreement_with_the_lists_and_the_neighbour_count(hip):
    p, radius = cloud("uniform"), f32(1.5)
    for k in (4, 32):
        normal, _, m, _, _, info = cloud_eval.normals(p, radius, k, variation=False)
        assert np.array_equal(m.cpu().numpy().view(np.uint32), cloud_eval.nearest_k(p, radius, k)[2])
        estimated = np.nonzero(normal.cpu().numpy().any(axis=1))[0]
        assert len(estimated) == info["estimated"] and np.isin(estimated, cloud_eval.drop_isolated(p, radius, 3)).all()


@pytest.mark.gpu
def test_the_filter_equals_the_restatement(hip):
    share = _check_filter()
    (r, keep), (given, rows) = filter_ref(), filter_normals()
    p = cloud("sphere_floaters")
    for grid in (0, 7):
        kept, ms, info = cloud_eval.drop_disagreeing_normals(p, given, SPHERE_RADIUS, SPHERE_K, FILTER_ANGLE, grid=grid, return_info=True)
        assert kept.dtype == np.int64
        mask = np.zeros(len(p), dtype=np.uint8)
        mask[kept] = 1
        assert mask.tobytes() == keep.astype(np.uint8).tobytes()
        assert ms > 0 and (info["estimated"], info["short"]) == (r.estimated, r.short)
    assert np.array_equal(cloud_eval.drop_disagreeing_normals(torch.from_numpy(p).cuda(), torch.from_numpy(given).cuda(), SPHERE_RADIUS,
                                                              SPHERE_K, FILTER_ANGLE), kept)
    assert not np.isin(rows, kept).any() and not (kept >= N_SPHERE).any()
    assert abs(float(np.isin(np.setdiff1d(np.arange(N_SPHERE), rows), kept).mean()) - share) < 1e-12


@pytest.mark.gpu
def test_score_with_the_filter_is_the_score_of_the_filtered_cloud(hip):
    keys, times = thin_cases.SCORE_KEYS, thin_cases.TIMES
    new_keys = {"normal_radius", "normal_k", "max_normal_angle", "cloud_points_before_normals", "normal_device_ms"}
    given, _ = filter_normals()
    p = cloud("sphere_floaters")
    ref = p[:N_SPHERE:2]
    plain = cloud_eval.score(p, ref, max_dist=5.0)
    assert set(plain) == keys  # without the new arguments: key for key what it was
    others = dict(reduce=1.5, seed=3, neighbour_radius=6.0, min_neighbours=4, outlier_radius=6.0, outlier_k=8, outlier_std=2.0,
                  component_radius=5.0, min_component=100)
    for four in (False, True):
        idx = np.arange(len(p))
        if four:
            idx = cloud_eval.thin(p, 1.5, seed=3)
            idx = idx[cloud_eval.drop_isolated(p[idx], 6.0, 4)]
            idx = idx[cloud_eval.drop_outliers(p[idx], 6.0, 8, 2.0)]
            idx = idx[cloud_eval.drop_small_components(p[idx], 5.0, 100)]
        kept = cloud_eval.drop_disagreeing_normals(p[idx], given[idx], SPHERE_RADIUS, SPHERE_K, FILTER_ANGLE)
        assert 0.5 * len(idx) < len(kept) < len(idx)
        got, indices = cloud_eval.score(p, ref, max_dist=5.0, return_indices=True, normal_radius=SPHERE_RADIUS, normal_k=SPHERE_K,
                                        max_normal_angle=FILTER_ANGLE, cloud_normals=given, **(others if four else {}))
        want = cloud_eval.score(p[idx][kept], ref, max_dist=5.0)  # the reference is never filtered
        assert keys | new_keys <= set(got) and (four or set(got) == keys | new_keys)
        for k in keys - times:
            assert got[k] == want[k], k
        assert np.array_equal(indices, idx[kept]) and indices.dtype == np.int64  # the five stages compose
        assert (got["normal_radius"], got["normal_k"], got["max_normal_angle"]) == (SPHERE_RADIUS, SPHERE_K, FILTER_ANGLE)
        assert got["cloud_points_before_normals"] == len(idx) and got["cloud_points"] == len(kept) and got["normal_device_ms"] > 0
        if four:
            assert got["cloud_points_before_components"] >= len(idx)


def _filter_vertices():
    p = cloud("sphere_floaters")
    given, _ = filter_normals()
    v = neighbour_cases._own_vertices(len(p))
    for a, (c, n) in enumerate(zip("xyz", ("nx", "ny", "nz"))):
        v[c], v[n] = p[:, a], given[:, a]
    return p, given, v


@pytest.mark.gpu
def test_the_command_line_writes_the_cloud_it_scores_and_the_estimates(hip, tmp_path, capsys):
    p, given, v = _filter_vertices()
    src, ref, out, rep = (str(tmp_path / n) for n in ("cloud.ply", "ref.ply", "out.ply", "report.json"))
    dmb.write_points_ply(src, v)
    dmb.write_points_ply(ref, v[:N_SPHERE:2])
    common = ["--cloud", src, "--reference", ref, "--max_dist", "5", "--component_radius", "5", "--min_component", "100"]
    assert cloud_eval.main(common + ["--normal_radius", "6", "--normal_k", "8", "--max_normal_angle", "30", "--write_cloud", out,
                                     "--output", rep]) == 0
    text = capsys.readouterr().out
    clumps = cloud_eval.drop_small_components(p, 5.0, 100)
    idx = clumps[cloud_eval.drop_disagreeing_normals(p[clumps], given[clumps], 6.0, 8, 30.0)]
    assert 5000 < len(idx) < len(clumps) == N_SPHERE
    assert dmb.read_ply_binary(out).tobytes() == v[idx].tobytes()  # what is scored: every property, the file's own normals
    report = json.load(open(rep))
    assert report["cloud_points"] == len(idx) and report["cloud_points_before_normals"] == len(clumps) and report["normal_k"] == 8
    assert report["cloud_points_before_components"] == len(p)
    assert "degrees off" in text and "%d -> %d points" % (len(clumps), len(idx)) in text and "%d -> %d points" % (len(p), len(clumps)) in text
    # --estimated_normals: the estimates of the scored cloud, along the file's normals
    assert cloud_eval.main(common + ["--normal_radius", "6", "--normal_k", "8", "--max_normal_angle", "30", "--write_cloud", out,
                                     "--estimated_normals"]) == 0
    got = dmb.read_ply_binary(out)
    est, _ = cloud_eval.estimate_normals(p[idx], 6.0, 8, orient=2, guide=given[idx])
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], -1).view(np.uint32), est.view(np.uint32))
    for c in ("x", "y", "z", "red", "green", "blue"):
        assert np.array_equal(got[c], v[idx][c])
    assert ((est.astype(f64) * p[idx]).sum(axis=1) > 0).all()  # outward, like the file's
    # the estimate alone, on a file without normals: nothing is dropped, nx, ny, nz are added, rule 0
    bare = str(tmp_path / "bare.ply")
    dmb.write_ply_vertices(bare, v[["x", "y", "z", "red"]][:N_SPHERE])
    assert cloud_eval.main(["--cloud", bare, "--reference", ref, "--max_dist", "5", "--normal_radius", "6", "--normal_k", "8",
                            "--write_cloud", out, "--estimated_normals"]) == 0
    got = dmb.read_ply_vertices(out)
    assert got.dtype.names == ("x", "y", "z", "red", "nx", "ny", "nz") and len(got) == N_SPHERE
    est, _ = cloud_eval.estimate_normals(p[:N_SPHERE], 6.0, 8)
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], -1).view(np.uint32), est.view(np.uint32))
    capsys.readouterr()


@pytest.mark.gpu
def test_batch_fuses_and_drops_the_disagreeing_normals(hip, tmp_path):
    """batch --fuse --fuse_normal_radius on the suite's small synthetic scan (as tests/test_cloud_components.py writes it):
    fused.ply is the unfiltered run's cloud without the points whose fused normal is more than 10 degrees off the estimate
    (or that have no estimate), and the report says so.  The radius is four times the median distance to the nearest
    neighbour in the unfiltered cloud."""
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
    given = np.stack([plain["nx"], plain["ny"], plain["nz"]], -1)
    assert len(xyz) >= 100
    d2 = cloud_eval.nearest_k(xyz, 1e6, 1)[0][:, 0]
    radius = float(f32(4.0 * np.sqrt(np.median(d2.astype(np.float64)))))
    r = normals_ref.normals(xyz, radius, 8)
    keep = normals_ref.keep_agreeing(r, given, 10.0)
    print("the fused cloud: %d points, %d estimated, %d kept at 10 degrees" % (len(xyz), r.estimated, int(keep.sum())))
    assert 0 < keep.sum()
    assert batch.main(base + ["--output-folder", filtered_dir, "--fuse_normal_radius", repr(radius), "--fuse_normal_k", "8",
                              "--fuse_max_normal_angle", "10"]) == 0
    got = dmb.read_ply_binary(os.path.join(filtered_dir, "fused.ply"))
    assert got.tobytes() == plain[keep].tobytes()
    fusion = json.load(open(os.path.join(filtered_dir, "batch_rank0.json")))["fusion"]
    assert fusion["points_before_normals"] == len(plain) and fusion["points"] == len(got) == int(keep.sum())
    assert fusion["normal_device_ms"] > 0
    assert "points_before_normals" not in json.load(open(os.path.join(plain_dir, "batch_rank0.json")))["fusion"]
