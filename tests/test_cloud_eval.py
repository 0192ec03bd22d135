"""The cloud search (gipuma_hip_cloud_nearest, gipuma_amd.cloud_eval.nearest).  Every case is a pair of
clouds, a radius and a condition -- stated on the restatement (tests/cloud_ref.py) alone -- that it reaches the path it is
named for; that condition runs without a device.  GPU: the kernels equal the restatement in d2 (as raw 32-bit patterns),
idx and both counts, at every grid; the descriptor's stream; the C-ABI's argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest

from gipuma_amd import abi
from tests import cloud_ref
from tests.abi_layout import assert_mirrors_header

f32 = np.float32
GRIDS = (0, 1, 2, 7, 256)  # 256 on a small cloud filling a cube: 2^24 cells, the scan's carry over 1024 chunks


class Case:
    def __init__(self, queries, targets, max_dist, check, grids=GRIDS, early_out=None):
        self.queries = np.ascontiguousarray(queries, dtype=f32).reshape(-1, 3)
        self.targets = np.ascontiguousarray(targets, dtype=f32).reshape(-1, 3)
        self.max_dist, self.check, self.grids, self.early_out = f32(max_dist), check, grids, early_out

    @functools.cached_property
    def ref(self):
        return cloud_ref.nearest(self.queries, self.targets, self.max_dist)


def _uniform_pair():
    """case 1's clouds: 5000 queries and 7000 targets, each uniform in a 100^3 box.  The two boxes are 10 apart on every
    axis: inside one common box a query misses with probability exp(-0.007 * 4/3 pi 5^3) = 2.6 % only."""
    rng = np.random.default_rng(101)
    return (rng.uniform(10.0, 110.0, (5000, 3)).astype(f32), rng.uniform(0.0, 100.0, (7000, 3)).astype(f32))


def _sphere_pair(n=6000, radius=50.0, sigma=0.2, seed=202):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        v = rng.normal(size=(n, 3))
        v *= radius / np.linalg.norm(v, axis=1, keepdims=True)
        out.append(v + rng.normal(scale=sigma, size=(n, 3)))
    return out


def _occupied_share(targets, G):
    """share of the cells of a G-cell grid over the targets' box that hold a target (in float64: a property of the data)"""
    t = np.asarray(targets, dtype=np.float64)
    lo, ext = t.min(axis=0), t.max(axis=0) - t.min(axis=0)
    h = ext.max() / G
    c = np.minimum(np.floor((t - lo) / h), np.floor(ext / h)).astype(np.int64)
    n = np.floor(ext / h).astype(np.int64) + 1
    return len({tuple(r) for r in c}) / float(np.prod(n)), c


def _both_classes(share):
    def check(c):
        assert c.ref.found >= share * len(c.queries) and c.ref.none >= share * len(c.queries), (c.ref.found, c.ref.none)
    return check


def _case_found_and_none():
    a, b = _uniform_pair()
    return Case(a, b, 5.0, _both_classes(0.10))


def _case_sphere():
    a, b = _sphere_pair()

    def check(c):
        assert c.ref.found > 0.5 * len(a) and c.ref.none > 0
        assert _occupied_share(b, 55)[0] < 0.05  # (55: the automatic grid of 6000 targets) a surface: most cells are empty
    return Case(a, b, 2.0, check)


def _case_ties():
    g = np.arange(8, dtype=np.float64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c7 = np.arange(7, dtype=np.float64) + 0.5
    centres = np.stack(np.meshgrid(c7, c7, c7, indexing="ij"), -1).reshape(-1, 3)
    a, b = np.concatenate([lattice, centres]), np.concatenate([lattice, lattice])

    def check(c):
        r = c.ref
        assert r.none == 0 and (r.idx < 512).all()  # the lower copy wins every tie
        assert (r.d2[:512] == 0).all() and np.array_equal(r.idx[:512], np.arange(512))
        assert (r.d2[512:] == f32(0.75)).all()  # eight corners at the same distance ...
        corner = np.floor(centres).astype(np.int64)
        assert np.array_equal(r.idx[512:], (corner[:, 0] * 8 + corner[:, 1]) * 8 + corner[:, 2])  # ... the lowest index
    return Case(a, b, 1.0, check)


def _case_inclusive(inside):
    def check(c):
        if inside:
            assert c.ref.d2[0] == 25 and c.ref.idx[0] == 0 and (c.ref.found, c.ref.none) == (1, 0)
        else:
            assert np.isinf(c.ref.d2[0]) and c.ref.idx[0] == -1 and (c.ref.found, c.ref.none) == (0, 1)
    return Case([[3, 4, 0]], [[0, 0, 0]], f32(5) if inside else np.nextafter(f32(5), f32(0)), check)


SHIFTS = {"0.9": 0.9 * 5.0, "1.1": 1.1 * 5.0, "1e4": 1e4}


def _case_outside(axis, side, shift):
    """case 1's targets moved so that their box begins SHIFTS[shift] past one face of the queries' box.  Query 0 is put
    on that face, straight across from the nearest target: at 0.9 max_dist it finds it."""
    a, b = _uniform_pair()
    a, b = a.astype(np.float64), b.astype(np.float64)
    gap = SHIFTS[shift]
    face = a[:, axis].max() if side > 0 else a[:, axis].min()
    if side > 0:
        b[:, axis] += face + gap - b[:, axis].min()
        t = b[:, axis].argmin()
    else:
        b[:, axis] += face - gap - b[:, axis].max()
        t = b[:, axis].argmax()
    a[0] = b[t]
    a[0, axis] = face

    def check(c):
        if shift == "0.9":
            assert c.ref.found >= 1 and c.ref.idx[0] == t and c.ref.none > 0.9 * len(a)
        else:
            assert c.ref.found == 0
    # (float32 rounding of the moved clouds: the gap of 5.5 stays above 5 by far)
    return Case(a, b, 5.0, check, early_out=None if shift == "0.9" else len(a))


def _case_large_coordinates():
    a, b = _sphere_pair()
    scale = 0.02 / np.sqrt(4 * np.pi * 50.0 ** 2 / 6000)  # mean spacing of 6000 points on the sphere -> 0.02
    a, b = (a * scale + 65536.0).astype(f32), (b * scale + 65536.0).astype(f32)

    def check(c):
        assert c.ref.found > 0.5 * len(a)
        assert len(np.unique(c.ref.d2)) < 200  # distances on the coordinates' 2^-7 lattice: exact ties abound
        h = float((b.max(axis=0) - b.min(axis=0)).max()) / 55
        assert np.spacing(f32(65536.0)) > 0.1 * h  # a coordinate's own rounding step against the automatic grid's cell
    return Case(a, b, 0.05, check)


def _degenerate(kind):
    rng = np.random.default_rng(707)
    base = rng.uniform(0.0, 10.0, (500, 3))
    a = rng.uniform(-1.0, 11.0, (300, 3))
    if kind == "one_target":
        b = base[:1]
        a[:20] = b[0] + rng.uniform(-0.5, 0.5, (20, 3))
    elif kind == "identical":
        b = np.repeat(base[:1], 500, axis=0)
        a[:20] = b[0] + rng.uniform(-0.5, 0.5, (20, 3))
    elif kind == "collinear":
        b = np.array([1.0, 2.0, 3.0]) + np.linspace(0.0, 10.0, 500)[:, None] * np.array([1.0, 0.5, -0.25])
        a[:100] = b[::5] + rng.uniform(-0.5, 0.5, (100, 3))
    elif kind == "coplanar":
        b = rng.uniform(0.0, 10.0, (2000, 3))
        b[:, 2] = 4.0
        a[:, 2] = rng.uniform(2.5, 5.5, 300)
    elif kind == "no_target":
        b = np.zeros((0, 3))
    elif kind == "no_query":
        a, b = np.zeros((0, 3)), base
    else:  # "queries_<n>"
        b = base
        a = rng.uniform(0.0, 10.0, (int(kind.split("_")[1]), 3))
        a[0] = b[7] + 0.25

    def check(c):
        r = c.ref
        assert r.found + r.none == len(a)
        if kind == "no_target":
            assert r.found == 0 and r.none == 300
        elif kind == "no_query":
            assert (r.found, r.none) == (0, 0)
        else:
            assert r.found > 0
            if not kind.startswith("queries_") or len(a) > 1:
                assert r.none > 0
        if kind == "identical":
            assert (r.idx[r.idx >= 0] == 0).all()  # 500 exact ties: the lowest index
    return Case(a, b, 1.0, check)


def _case_non_finite():
    a, b = _uniform_pair()
    rng = np.random.default_rng(808)
    bad = {}
    for name, pts in (("a", a), ("b", b)):
        rows = rng.choice(len(pts), len(pts) // 100, replace=False)
        pts[rows, rng.integers(0, 3, len(rows))] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=f32), len(rows))
        bad[name] = rows

    def check(c):
        r = c.ref
        assert len(bad["a"]) == 50 and len(bad["b"]) == 70 and not np.isfinite(b[bad["b"]]).all(axis=1).any()
        assert (r.idx[bad["a"]] == -1).all() and np.isinf(r.d2[bad["a"]]).all()  # never found
        assert not np.isin(r.idx, bad["b"]).any() and r.found > 0.5 * len(a)      # never a neighbour
    return Case(a, b, 5.0, check)


def _case_crowded():
    rng = np.random.default_rng(909)
    b = np.concatenate([rng.uniform(0.0, 0.01, (20000, 3)), [[1000.0, 0.0, 0.0]]])
    a = rng.uniform(-0.02, 0.03, (300, 3))

    def check(c):
        share, cells = _occupied_share(b, 16)
        assert len({tuple(r) for r in cells[:20000]}) == 1  # 20 000 targets in one cell of the 16-cell grid
        assert c.ref.found > 100 and c.ref.none > 10
    return Case(a, b, 0.02, check, grids=(16,))


def _case_radius(which):
    a, b = _uniform_pair()

    def check(c):
        if which == "huge":
            assert c.ref.none == 0
        else:
            assert c.ref.found <= 0.01 * len(a)
    return Case(a, b, 1000.0 if which == "huge" else 1e-3, check)


BUILDERS = {
    "found_and_none": _case_found_and_none,
    "sphere": _case_sphere,
    "ties": _case_ties,
    "radius_inclusive": lambda: _case_inclusive(True),
    "radius_just_short": lambda: _case_inclusive(False),
    **{"outside_%s%s_%s" % ("xyz"[k], "+" if s > 0 else "-", sh): functools.partial(_case_outside, k, s, sh)
       for k in range(3) for s in (1, -1) for sh in SHIFTS},
    "large_coordinates": _case_large_coordinates,
    **{"degenerate_" + k: functools.partial(_degenerate, k)
       for k in ("one_target", "identical", "collinear", "coplanar", "no_target", "no_query", "queries_1", "queries_63",
                 "queries_64", "queries_65", "queries_257")},
    "non_finite": _case_non_finite,
    "crowded_cell": _case_crowded,
    "radius_huge": lambda: _case_radius("huge"),
    "radius_tiny": lambda: _case_radius("tiny"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ----------------------------------------------------------------------------------------------------------------------
# CPU: every case reaches its path, judged on the restatement alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_the_case_reaches_the_path_it_is_named_for(name):
    c = case(name)
    c.check(c)
    assert c.ref.found == int((c.ref.idx >= 0).sum()) == int(np.isfinite(c.ref.d2).sum())


def test_the_restatement_on_a_hand_made_pair():
    r = cloud_ref.nearest([[0, 0, 0], [10, 0, 0], [np.nan, 0, 0]], [[1, 0, 0], [-1, 0, 0], [0, np.inf, 0], [10, 2, 0]], 2.0)
    assert r.d2.tolist() == [1.0, 4.0, np.inf] and r.idx.tolist() == [0, 3, -1] and (r.found, r.none) == (2, 1)


def _desc(**kw):
    d = abi.CloudDesc()
    d.abi_version, d.n_queries, d.n_targets, d.queries, d.targets = abi.ABI_VERSION, 4, 4, 0x1000, 0x2000
    d.max_dist, d.grid, d.device_id, d.stream = 1.0, 0, 0, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_the_device():
    """(the pointers are never followed: every call here is turned down, the last one for want of a device when there is
    none -- with a device it is not made)"""
    lib = abi.load_library()
    out = 0x3000

    def rc(d2=out, idx=out, **kw):
        return lib.gipuma_hip_cloud_nearest(C.byref(_desc(**kw)), d2, idx, None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(max_dist=bad) == abi.ERR_ARG and b"max_dist" in lib.gipuma_hip_last_error()
    for bad in (257, -1):
        assert rc(grid=bad) == abi.ERR_ARG and b"grid" in lib.gipuma_hip_last_error()
    assert rc(queries=None) == abi.ERR_ARG and b"null pointer" in lib.gipuma_hip_last_error()
    assert rc(targets=None) == abi.ERR_ARG
    assert rc(d2=None) == abi.ERR_ARG and rc(idx=None) == abi.ERR_ARG
    assert rc(n_queries=-1) == abi.ERR_ARG
    assert rc(n_queries=1 << 31) == abi.ERR_UNSUPPORTED and rc(n_targets=1 << 31) == abi.ERR_UNSUPPORTED
    assert rc(abi_version=99) == abi.ERR_ARG and b"abi_version" in lib.gipuma_hip_last_error()
    assert lib.gipuma_hip_cloud_nearest(None, out, out, None, None) == abi.ERR_ARG
    assert lib.gipuma_hip_cloud_last_stats(None) == abi.ERR_ARG
    if lib.gipuma_hip_device_count() == 0:
        assert rc() == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.gipuma_hip_last_error()
        assert rc(n_queries=0, queries=None, d2=None, idx=None) == abi.ERR_NO_DEVICE  # valid, too
        from gipuma_amd import cloud_eval
        with pytest.raises(abi.GipumaHipError):
            cloud_eval.nearest(np.zeros((2, 3), f32), np.zeros((2, 3), f32), 1.0)
    else:
        assert rc(device_id=lib.gipuma_hip_device_count()) == abi.ERR_ARG


def test_the_descriptor_mirrors_the_header():
    assert_mirrors_header(abi.CloudDesc, "gipuma_hip_cloud_desc")


def test_the_kernels_use_global_not_flat_memory_instructions_and_no_float_atomics():
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "c.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--offload-device-only", "-o", out, "gipuma_cloud.hip"],
                              cwd=os.path.join(root, "gipuma_amd", "csrc"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    for k in ("box_partial_kernel", "box_final_kernel", "count_kernel", "scan_kernel", "scatter_kernel", "search_kernel"):
        assert "_ZN5cloud%d%s" % (len(k), k) in asm
    ops = [l.split()[0] for l in asm.splitlines() if l.startswith("\t") and l.split()]
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")]
    assert "global_load_dwordx4" in ops  # a sorted point is one 16-byte load
    assert {o for o in ops if "atomic" in o} == {"global_atomic_add"}  # integer counters only
    assert not [o for o in ops if o.startswith("v_fma") or o.startswith("v_mad_f32") or o.startswith("v_fmac")]  # no contraction


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _assert_equals_ref(got, c, what):
    d2, idx, ms, info = got
    r = c.ref
    assert np.array_equal(idx, r.idx), "%s: idx differs at %d queries" % (what, int((idx != r.idx).sum()))
    assert np.array_equal(d2.view(np.uint32), r.d2.view(np.uint32)), "%s: d2 differs" % what
    assert (info["found"], info["none"]) == (r.found, r.none), what
    assert info["early_out"] + info["searched"] <= len(c.queries)


GPU_RUNS = [(name, g) for name in sorted(BUILDERS) for g in (BUILDERS[name]().grids if name == "crowded_cell" else GRIDS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid", GPU_RUNS, ids=["%s-grid%d" % r for r in GPU_RUNS])
def test_kernels_equal_the_restatement_bit_for_bit(hip, name, grid):
    from gipuma_amd import cloud_eval
    c = case(name)
    c.check(c)
    got = cloud_eval.nearest(c.queries, c.targets, c.max_dist, grid=grid, return_info=True)
    _assert_equals_ref(got, c, "%s at grid %d" % (name, grid))
    info = got[3]
    if len(c.queries) and np.isfinite(c.targets).all(axis=1).any():
        ext = c.targets[np.isfinite(c.targets).all(axis=1)]
        ext = ext.max(axis=0) - ext.min(axis=0)
        if grid and ext.max() > 0:
            assert info["grid"] == grid and max(info["cells_x"], info["cells_y"], info["cells_z"]) == grid
            assert all(info["cells_" + k] == 1 for k, e in zip("xyz", ext) if e == 0)  # an axis of zero extent: one cell
    if c.early_out is not None:  # every query beyond max_dist from the targets' box: answered without a search
        assert (info["early_out"], info["searched"]) == (c.early_out, 0)
    if name.endswith("_0.9"):
        assert info["searched"] >= 1  # (query 0 at least; queries far off sideways still take the early-out)


@pytest.mark.gpu
def test_device_tensors_go_by_pointer_and_runs_repeat(hip):
    import torch
    from gipuma_amd import cloud_eval
    c = case("sphere")
    a, b = torch.from_numpy(c.queries).cuda(), torch.from_numpy(c.targets).cuda()
    for _ in range(2):  # (the order inside a cell varies from run to run; the result does not)
        _assert_equals_ref(cloud_eval.nearest(a, b, c.max_dist, return_info=True), c, "device tensors")


@pytest.mark.gpu
def test_search_on_a_caller_s_stream(hip):
    """desc.stream = a torch stream on which the clouds were written just before, the device not synchronised: the library
    runs behind them on that stream.  Two cloud sizes one after the other on the same stream."""
    import torch
    lib = hip
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream == 0
    for name in ("found_and_none", "degenerate_queries_257"):
        c = case(name)
        staged = torch.from_numpy(c.queries).cuda(), torch.from_numpy(c.targets).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the clouds the library reads: device copies queued on the caller's stream
            a, b = staged[0].clone(), staged[1].clone()
            d2 = torch.empty(len(c.queries), dtype=torch.float32, device="cuda")
            idx = torch.empty(len(c.queries), dtype=torch.int32, device="cuda")
        d = _desc(n_queries=len(c.queries), n_targets=len(c.targets), queries=a.data_ptr(), targets=b.data_ptr(),
                  max_dist=float(c.max_dist), stream=stream.cuda_stream)
        counts, ms = (C.c_int64 * 2)(), C.c_float()
        abi.check(lib, lib.gipuma_hip_cloud_nearest(C.byref(d), d2.data_ptr(), idx.data_ptr(), counts, C.byref(ms)), "cloud")
        stats = (C.c_int64 * 6)()
        assert lib.gipuma_hip_cloud_last_stats(stats) == 0
        info = dict(found=counts[0], none=counts[1], early_out=stats[4], searched=stats[5])
        _assert_equals_ref((d2.cpu().numpy(), idx.cpu().numpy(), ms.value, info), c, "%s on the caller's stream" % name)
        assert ms.value > 0
