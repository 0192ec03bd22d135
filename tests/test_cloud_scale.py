"""The cloud search and the thinning where tests/test_cloud_eval.py and tests/test_cloud_thin.py do not
go: clouds of 300 001 points -- the second trips of the box kernels' loops, the automatic grid at its cap -- and scales at
which the grid's proofs do not hold and one cell is taken instead (a cell edge or a thinning radius outside 2^-40 .. 2^40,
an infinite extent, an infinite r2), with radii whose square under- or overflows and distances that are subnormal.

The large clouds are judged against the sparse restatements (cloud_ref.nearest_sparse, thin_ref.thin_sparse: the
contract on a k-d tree's candidate pairs), which a CPU test here proves equal to the brute force in every field on every
case of the two older modules.  The extreme scales are judged against the brute force itself.  As there, every case
states on the restatement alone -- without a device -- that it reaches its path; here also on which grids one cell is
expected, worked out from the documented rule (`laid_out` below), not by asking the library."""
import functools
import math

import numpy as np
import pytest
# torch before the `hip` fixture loads the library: torch brings a HIP runtime of its own, and a process that loaded the
# library's first cannot start torch's (gipuma_amd.cloud_eval.nearest) -- this module must also run on its own
import torch  # noqa: F401

from tests import cloud_ref, thin_ref
from tests import test_cloud_eval as search_cases
from tests import test_cloud_thin as thin_cases

f32 = np.float32
GRIDS = search_cases.GRIDS
assert GRIDS == thin_cases.GRIDS == (0, 1, 2, 7, 256)
H_MIN, H_MAX = f32(2.0 ** -40), f32(2.0 ** 40)  # the range of cell edges (and thinning radii) the grid is used for, inclusive
SUBNORMAL_BELOW = np.finfo(f32).tiny        # 2^-126


# ----------------------------------------------------------------------------------------------------------------------
# The documented layout rule (include/gipuma_hip.h), in float32 as the library's host code states it
# ----------------------------------------------------------------------------------------------------------------------
def _longest_extent(points):
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    with np.errstate(over="ignore"):
        ext = p.max(axis=0) - p.min(axis=0)  # (float32: 6e38 is +inf)
    assert ext.dtype == f32
    return f32(max(f32(0), ext.max()))


def laid_out(longest, G, shortcut_holds):
    """(the G the library reports, whether it fell back to one cell): h = longest / G in float32; one cell where h is
    outside 2^-40 .. 2^40 (both ends included; an infinite extent ends up here) or the client's own condition fails"""
    with np.errstate(over="ignore", under="ignore"):
        h = f32(longest) / f32(G)
    fallback = not (H_MIN <= h <= H_MAX) or not shortcut_holds
    return (1 if fallback else G), fallback


def search_layout(c, grid):
    """the search: G = grid, or min(256, ceil(sqrt(n_targets / 2))); its condition is a finite r2"""
    G = grid if grid else min(256, max(1, math.ceil(math.sqrt(len(c.targets) / 2.0))))
    return laid_out(_longest_extent(c.targets), G, bool(np.isfinite(cloud_ref.squared(c.max_dist))))


def thin_layout(c, grid):
    """the thinning: G = grid, or floor(longest / radius) within 1 .. 256; its condition is a radius in 2^-40 .. 2^40"""
    longest = _longest_extent(c.points)
    q = float(longest) / float(c.radius)
    G = grid if grid else (256 if q >= 256 else 1 if q < 1 else int(q))
    return laid_out(longest, G, bool(H_MIN <= c.radius <= H_MAX))


# ----------------------------------------------------------------------------------------------------------------------
# A. The sparse restatements equal the brute force (CPU)
# ----------------------------------------------------------------------------------------------------------------------
# Declined cases: a listed pair costs about 24 bytes from the tree and 40 of work arrays, so the caps (2^23 pairs for the
# search, 2^22 for the thinning) bound a call at about half a gigabyte.  The two `radius_huge` cases pair every point with
# every other (35 000 000 and 4 498 500 pairs); nothing else comes near the caps.
def test_the_sparse_search_equals_the_brute_force_on_every_case():
    declined = []
    for name in sorted(search_cases.BUILDERS):
        c = search_cases.case(name)
        s = cloud_ref.nearest_sparse(c.queries, c.targets, c.max_dist)
        if s is None:
            declined.append(name)
            continue
        assert np.array_equal(s.d2.view(np.uint32), c.ref.d2.view(np.uint32)), name
        assert np.array_equal(s.idx, c.ref.idx) and s.idx.dtype == c.ref.idx.dtype, name
        assert (s.found, s.none) == (c.ref.found, c.ref.none), name
    assert declined == ["radius_huge"]


def test_the_sparse_thinning_equals_the_brute_force_on_every_case():
    declined = []
    for name in sorted(thin_cases.BUILDERS):
        c = thin_cases.case(name)
        s = thin_ref.thin_sparse(c.points, c.radius, c.seed, c.order)
        if s is None:
            declined.append(name)
            continue
        assert s.keep.dtype == np.uint8 and np.array_equal(s.keep, c.ref.keep), name
        assert (s.kept, s.dropped, s.not_finite, s.rounds) == (c.ref.kept, c.ref.dropped, c.ref.not_finite, c.ref.rounds), name
        assert s.undecided == c.ref.undecided, name
    assert declined == ["radius_huge"]


def test_the_restatement_answers_none_where_every_d2_overflows():
    """max_dist = 1e20: r2 is +inf in float32.  The query and the two finite targets are 6e38 apart, their d2 is +inf too,
    and inf <= inf must not make them candidates: +inf means "none".  (Target 0 is NaN: no index may come back.)"""
    r = cloud_ref.nearest([[3e38, 0, 0]], [[np.nan, 0, 0], [-3e38, 0, 0], [-3e38, 1, 0]], 1e20)
    assert np.isposinf(r.d2[0]) and r.idx[0] == -1 and (r.found, r.none) == (0, 1)


# ----------------------------------------------------------------------------------------------------------------------
# B. Large clouds
# ----------------------------------------------------------------------------------------------------------------------
N_LARGE = 300001
# where the six outlier targets stand, and the loop trip each owns: box_partial_kernel runs 1024 workgroups of 256 lanes,
# so point i is read by workgroup (i / 256) % 1024 in trip i / 262144; box_final_kernel's lane t reads the partial boxes
# t, t + 256, t + 512, t + 768 in its four trips.
OUTLIERS = (0,               # the control: first trip of both loops
            70000,           # workgroup 273: box_final_kernel's second trip
            200000,          # workgroup 781: box_final_kernel's fourth trip
            262143,          # the last point of box_partial_kernel's first trip
            262149,          # box_partial_kernel's second trip
            N_LARGE - 1)     # the ragged tail of that second trip
FACES = tuple((k, s) for k in range(3) for s in (-1, 1))
N_SPHERE_QUERIES = 20000


@functools.lru_cache(maxsize=None)
def large_clouds():
    """(queries, targets, the float32 box of the bulk): _sphere_pair's two noisy samplings of a sphere (R = 50, sigma = 0.2)
    at 300 001 points, moved into [0, 100]^3.  Six targets are replaced by outliers, each 10 beyond one face of the bulk's
    box along that face's axis (at the box's centre otherwise), so that each ALONE defines one face of the targets' box.
    The queries: the first 20 000 of the other sampling, then one per outlier, 0.25 farther out than its target."""
    a, b = search_cases._sphere_pair(n=N_LARGE)
    b = (b + 50.0).astype(f32)
    bulk = np.ones(N_LARGE, dtype=bool)
    bulk[list(OUTLIERS)] = False
    lo, hi = b[bulk].min(axis=0).astype(np.float64), b[bulk].max(axis=0).astype(np.float64)
    far = np.empty((6, 3), dtype=np.float64)
    for m, (k, s) in enumerate(FACES):
        b[OUTLIERS[m]] = 0.5 * (lo + hi)
        b[OUTLIERS[m], k] = (hi[k] + 10.0) if s > 0 else (lo[k] - 10.0)
        far[m] = b[OUTLIERS[m]]
        far[m, k] += 0.25 * s
    a = np.concatenate([a[:N_SPHERE_QUERIES] + 50.0, far]).astype(f32)
    return a, b, (lo, hi)


@functools.lru_cache(maxsize=None)
def large_search_ref():
    a, b, _ = large_clouds()
    return cloud_ref.nearest_sparse(a, b, 0.5)


@functools.lru_cache(maxsize=None)
def large_thin_ref():
    return thin_ref.thin_sparse(large_clouds()[1], 0.3)


def _check_large_search():
    a, b, (lo, hi) = large_clouds()
    r = large_search_ref()
    assert len(a) == N_SPHERE_QUERIES + 6 and len(b) == N_LARGE and N_LARGE > 262144 + 256
    for m, (k, s) in enumerate(FACES):  # each outlier alone defines its face: the rest of the cloud ends 10 short of it
        rest = np.delete(b[:, k], OUTLIERS[m])
        assert b[OUTLIERS[m], k] == (b[:, k].max() if s > 0 else b[:, k].min())
        assert abs(float(b[OUTLIERS[m], k]) - float(rest.max() if s > 0 else rest.min())) > 9.9
    assert np.array_equal(r.idx[N_SPHERE_QUERIES:], np.array(OUTLIERS, dtype=np.int32))
    assert (np.abs(np.sqrt(r.d2[N_SPHERE_QUERIES:].astype(np.float64)) - 0.25) < 1e-4).all()
    sphere = r.idx[:N_SPHERE_QUERIES] >= 0
    assert sphere.sum() > 0.5 * N_SPHERE_QUERIES and (~sphere).any(), int(sphere.sum())
    assert r.found == int(np.isfinite(r.d2).sum()) == int((r.idx >= 0).sum())


def _check_large_thin():
    r = large_thin_ref()
    assert r.not_finite == 0 and r.kept + r.dropped == N_LARGE
    assert r.kept >= 0.2 * N_LARGE and r.dropped >= 0.2 * N_LARGE and r.rounds >= 3, (r.kept, r.dropped, r.rounds)
    assert r.keep[list(OUTLIERS)].all()  # (nothing within 10 of them)


def test_the_large_search_reaches_its_paths():
    _check_large_search()


def test_the_large_thinning_reaches_its_paths():
    _check_large_thin()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", (0, 7))
def test_large_search_equals_the_sparse_restatement(hip, grid):
    """A box that misses an outlier target -- a box loop cut short -- puts that outlier's query 10.25 from the box: it takes
    the early-out and answers "none", where the restatement finds the outlier at 0.25."""
    from gipuma_amd import cloud_eval
    _check_large_search()
    a, b, _ = large_clouds()
    r = large_search_ref()
    d2, idx, ms, info = cloud_eval.nearest(a, b, 0.5, grid=grid, return_info=True)
    wrong = np.nonzero(idx != r.idx)[0]
    assert len(wrong) == 0, "idx differs at %d queries, the first ones %s" % (len(wrong), wrong[:8].tolist())
    assert np.array_equal(d2.view(np.uint32), r.d2.view(np.uint32))
    assert (info["found"], info["none"]) == (r.found, r.none)
    assert info["grid"] == (256 if grid == 0 else grid)  # 300 001 targets: the automatic grid at its cap
    assert info["early_out"] + info["searched"] <= len(a)


@pytest.mark.gpu
def test_large_thinning_equals_the_sparse_restatement(hip):
    from gipuma_amd import cloud_eval
    _check_large_thin()
    b = large_clouds()[1]
    r = large_thin_ref()
    keep, ms, info = cloud_eval.thin_mask(b, 0.3, 0, "hashed", grid=0)
    keep = keep.cpu().numpy()
    assert keep.dtype == np.uint8 and np.array_equal(keep, r.keep), "the mask differs at %d points" % int((keep != r.keep).sum())
    assert (info["kept"], info["dropped"], info["not_finite"], info["rounds"]) == (r.kept, r.dropped, r.not_finite, r.rounds)
    longest = float(_longest_extent(b))
    assert longest / 0.3 > 256 and info["grid"] == 256  # floor(longest / radius), capped


# ----------------------------------------------------------------------------------------------------------------------
# C. Extreme scales: the search
# ----------------------------------------------------------------------------------------------------------------------
def _unit_clouds(n_targets=300, n_queries=200, seed=4242, spread=0.2):
    """targets in [0, 1]^3 with (0,0,0) and (1,1,1) among them -- the extent is exactly 1 on every axis --, queries in
    [-spread, 1 + spread]^3, the first twenty of them next to a target; float32, to be scaled by a power of two (exact)"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.0, 1.0, (n_targets, 3))
    b[0], b[1] = 0.0, 1.0
    a = rng.uniform(-spread, 1.0 + spread, (n_queries, 3))
    a[:20] = b[5:25] + rng.uniform(-0.02, 0.02, (20, 3))
    return a.astype(f32), b.astype(f32)


class SearchCase(search_cases.Case):
    def __init__(self, queries, targets, max_dist, check, one_cell):
        super().__init__(queries, targets, max_dist, check)
        self.one_cell = one_cell  # the grids of GRIDS at which the case expects the one-cell fallback


def _found_and_none(c):
    assert c.ref.found >= 20 and c.ref.none >= 20, (c.ref.found, c.ref.none)


def _case_extent(exp, one_cell):
    """longest extent 2^exp, max_dist a tenth of it"""
    a, b = _unit_clouds()
    scale = f32(2.0 ** exp)

    def check(c):
        _found_and_none(c)
        assert _longest_extent(c.targets) == scale
    return SearchCase(a * scale, b * scale, f32(0.1) * scale, check, one_cell)


def _bulk_pair():
    rng = np.random.default_rng(515)
    b = rng.uniform(0.0, 10.0, (500, 3)).astype(f32)
    a = rng.uniform(-1.0, 11.0, (300, 3)).astype(f32)
    return a, b


def _case_infinite_extent():
    a, b = _bulk_pair()
    far = np.array([[3e38, 5.0, 5.0], [-3e38, 5.0, 5.0]], dtype=f32)
    a2 = np.concatenate([a, np.array([[2.9e38, 5.0, 5.0]], dtype=f32)])  # inside the box, 1e37 from a target: d2 overflows

    def check(c):
        assert np.isfinite(c.targets).all() and np.isposinf(_longest_extent(c.targets))
        plain = cloud_ref.nearest(a, b, c.max_dist)  # the queries near the bulk answer as they do without the far pair
        assert np.array_equal(c.ref.idx[:300], plain.idx) and np.array_equal(c.ref.d2[:300].view(np.uint32), plain.d2.view(np.uint32))
        assert plain.found >= 20 and plain.none >= 20
        assert not np.isin(c.ref.idx, (500, 501)).any() and c.ref.idx[300] == -1  # nothing finds the far pair
    return SearchCase(a2, np.concatenate([b, far]), 1.0, check, GRIDS)


def _case_r2_underflows(max_dist):
    """max_dist 1e-20: r2 = 1e-40 is subnormal; 1e-30: r2 = 0.  Thirty queries are exact copies of targets."""
    a, b = _bulk_pair()
    a[10:40] = b[100:130]

    def check(c):
        r2 = cloud_ref.squared(c.max_dist)
        assert (0 < r2 < SUBNORMAL_BELOW) if max_dist == 1e-20 else (r2 == 0 and c.max_dist > 0)
        assert np.array_equal(np.nonzero(c.ref.idx >= 0)[0], np.arange(10, 40))  # exactly the copies ...
        assert np.array_equal(c.ref.idx[10:40], np.arange(100, 130)) and (c.ref.d2[10:40] == 0).all()  # ... at d2 = 0
    return SearchCase(a, b, max_dist, check, ())


def _case_subnormal_d2():
    """extent 1e-19, max_dist 3e-20: r2 = 9e-40, and every d2 within it, is subnormal.  The contract is IEEE float32 with
    subnormals -- what numpy computes --, so kernels that flushed them to zero would find every target at d2 = 0."""
    a, b = _unit_clouds(n_targets=60, spread=1.0)
    a, b = (a.astype(np.float64) * 1e-19).astype(f32), (b.astype(np.float64) * 1e-19).astype(f32)

    def check(c):
        _found_and_none(c)
        hit = c.ref.d2[c.ref.idx >= 0]
        assert 0 < cloud_ref.squared(c.max_dist) < SUBNORMAL_BELOW and (hit < SUBNORMAL_BELOW).all()
        assert (hit > 0).all() and len(np.unique(hit)) > 0.9 * len(hit)  # not flushed: distinct non-zero values
        assert 0.9e-19 < _longest_extent(c.targets) < 1.1e-19
    return SearchCase(a, b, 3e-20, check, GRIDS)


def _case_r2_infinite():
    a, b = search_cases._uniform_pair()

    def check(c):
        assert np.isposinf(cloud_ref.squared(c.max_dist)) and np.isfinite(c.max_dist)
        huge = search_cases.case("radius_huge").ref  # max_dist 1000 on the same clouds: the global nearest target
        assert c.ref.none == 0 and huge.none == 0
        assert np.array_equal(c.ref.idx, huge.idx) and np.array_equal(c.ref.d2.view(np.uint32), huge.d2.view(np.uint32))
    return SearchCase(a, b, 1e20, check, GRIDS)


def _case_r2_infinite_far_pair():
    """the hand-made pair of test_the_restatement_answers_none_where_every_d2_overflows, and a second query that does
    find a target: d2 = +inf is no candidate, a finite d2 is one at any distance"""
    def check(c):
        assert c.ref.idx.tolist() == [-1, 1] and np.isposinf(c.ref.d2[0]) and c.ref.d2[1] == f32(0.0625)
    return SearchCase([[3e38, 0, 0], [-3e38, 0.25, 0]], [[np.nan, 0, 0], [-3e38, 0, 0], [-3e38, 1, 0]], 1e20, check, GRIDS)


SEARCH_BUILDERS = {
    # h = 2^-38 / G: grids 1 and 2 stay on the grid (h >= 2^-40), 7, 256 and the automatic 13 fall back
    "extent_2^-38": lambda: _case_extent(-38, (0, 7, 256)),
    # h = 2^48 / G: 256 gives 2^40 exactly and stays on the grid (the bound is inclusive), every other grid falls back
    "extent_2^48": lambda: _case_extent(48, (0, 1, 2, 7)),
    "extent_infinite": _case_infinite_extent,
    "r2_subnormal": lambda: _case_r2_underflows(1e-20),
    "r2_zero": lambda: _case_r2_underflows(1e-30),
    "d2_subnormal": _case_subnormal_d2,
    "r2_infinite": _case_r2_infinite,
    "r2_infinite_far_pair": _case_r2_infinite_far_pair,
}


@functools.lru_cache(maxsize=None)
def search_case(name):
    return SEARCH_BUILDERS[name]()


@pytest.mark.parametrize("name", sorted(SEARCH_BUILDERS))
def test_the_search_case_reaches_its_path_and_its_layout(name):
    c = search_case(name)
    c.check(c)
    assert c.ref.found == int((c.ref.idx >= 0).sum()) == int(np.isfinite(c.ref.d2).sum())
    assert tuple(g for g in GRIDS if search_layout(c, g)[1]) == tuple(c.one_cell)


SEARCH_RUNS = [(name, g) for name in sorted(SEARCH_BUILDERS) for g in GRIDS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", SEARCH_RUNS, ids=["%s-grid%d" % r for r in SEARCH_RUNS])
def test_search_at_extreme_scales_equals_the_brute_force(hip, name, grid):
    from gipuma_amd import cloud_eval
    c = search_case(name)
    c.check(c)
    got = cloud_eval.nearest(c.queries, c.targets, c.max_dist, grid=grid, return_info=True)
    search_cases._assert_equals_ref(got, c, "%s at grid %d" % (name, grid))
    info = got[3]
    G, one_cell = search_layout(c, grid)
    assert one_cell == (grid in c.one_cell)
    assert info["grid"] == G, "%s at grid %d: the library reports %d cells" % (name, grid, info["grid"])
    if one_cell:
        assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)


# ----------------------------------------------------------------------------------------------------------------------
# C. Extreme scales: the thinning
# ----------------------------------------------------------------------------------------------------------------------
class ThinCase(thin_cases.Case):
    def __init__(self, points, radius, check, one_cell):
        super().__init__(points, radius, check)
        self.one_cell = one_cell


def _kept_and_dropped(c):
    assert c.ref.kept >= 20 and c.ref.dropped >= 20, (c.ref.kept, c.ref.dropped)


def _case_thin_scaled(radius_exp, extent_over_radius, n, one_cell):
    """n points in a cube of edge extent_over_radius, its two corners among them, scaled by 2^radius_exp: radius
    2^radius_exp exactly, longest extent exactly extent_over_radius times that"""
    pts = np.random.default_rng(616).uniform(0.0, extent_over_radius, (n, 3))
    pts[0], pts[1] = 0.0, extent_over_radius
    scale = f32(2.0 ** radius_exp)

    def check(c):
        _kept_and_dropped(c)
        assert c.radius == scale and _longest_extent(c.points) == f32(extent_over_radius) * scale
    return ThinCase(pts.astype(f32) * scale, scale, check, one_cell)


def _case_thin_r2_infinite():
    pts = np.concatenate([thin_cases._uniform(400, seed=717), np.array([[3e38, 10, 10], [-3e38, 10, 10]], dtype=f32)])

    def check(c):
        assert np.isposinf(cloud_ref.squared(c.radius)) and np.isfinite(c.points).all() and np.isposinf(_longest_extent(c.points))
        # d2 = inf <= inf between the far pair too: every point is a neighbour of every other, the first in key order stays
        first = int(thin_ref.visiting_order(c.points, c.seed, c.order)[0])
        assert (c.ref.kept, c.ref.dropped, c.ref.rounds) == (1, 401, 2) and c.ref.keep[first] == 1
    return ThinCase(pts, 1e20, check, GRIDS)


def _case_thin_r2_zero():
    def check(c):
        assert c.radius > 0 and cloud_ref.squared(c.radius) == 0
        r = c.ref  # only exact copies suppress each other: one of each pair
        assert np.array_equal(r.keep[:512] + r.keep[512:], np.ones(512, np.uint8)) and (r.kept, r.rounds) == (512, 2)
    return ThinCase(thin_cases._lattice_twice(), 1e-30, check, GRIDS)


THIN_BUILDERS = {
    # the radius is outside 2^-40 .. 2^40: one cell at every grid (a quarter of the edge: 300 points crowd each other)
    "radius_2^41": lambda: _case_thin_scaled(41, 4, 300, GRIDS),
    "radius_2^-41": lambda: _case_thin_scaled(-41, 4, 300, GRIDS),
    # the radius is ON the bound and counts as inside; the extent is 16 radii, so the automatic grid is 16 and its cell edge
    # is the radius, on the bound too.  A forced grid goes by h = extent / G alone: 2^44 / G is within 2^40 for 256 only
    # (and for the automatic 16), 2^-36 / G is within 2^-40 for every grid but 256.
    "radius_2^40": lambda: _case_thin_scaled(40, 16, 1500, (1, 2, 7)),
    "radius_2^-40": lambda: _case_thin_scaled(-40, 16, 1500, (256,)),
    "r2_infinite": _case_thin_r2_infinite,
    "r2_zero": _case_thin_r2_zero,
}


@functools.lru_cache(maxsize=None)
def thin_case(name):
    return THIN_BUILDERS[name]()


@pytest.mark.parametrize("name", sorted(THIN_BUILDERS))
def test_the_thinning_case_reaches_its_path_and_its_layout(name):
    c = thin_case(name)
    c.check(c)
    r = c.ref
    assert r.kept + r.dropped + r.not_finite == len(c.points) and r.kept == int(r.keep.sum())
    assert np.array_equal(thin_ref.sequential(c.points, c.radius, c.seed, c.order), r.keep)
    assert tuple(g for g in GRIDS if thin_layout(c, g)[1]) == tuple(c.one_cell)
    if name.startswith("radius_2^") and name.endswith("40"):
        assert thin_layout(c, 0) == (16, False)  # the automatic grid: a cell edge of exactly the radius


THIN_RUNS = [(name, g) for name in sorted(THIN_BUILDERS) for g in GRIDS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", THIN_RUNS, ids=["%s-grid%d" % r for r in THIN_RUNS])
def test_thinning_at_extreme_scales_equals_the_brute_force(hip, name, grid):
    from gipuma_amd import cloud_eval
    c = thin_case(name)
    c.check(c)
    keep, ms, info = cloud_eval.thin_mask(c.points, c.radius, c.seed, c.order, grid=grid)
    thin_cases._assert_equals_ref(keep.cpu().numpy(), info, c, "%s at grid %d" % (name, grid))
    G, one_cell = thin_layout(c, grid)
    assert one_cell == (grid in c.one_cell)
    assert info["grid"] == G, "%s at grid %d: the library reports %d cells" % (name, grid, info["grid"])
    if one_cell:
        assert (info["cells_x"], info["cells_y"], info["cells_z"]) == (1, 1, 1)
