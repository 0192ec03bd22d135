"""Plane-keyed (pm_group.h) and push (pm_push.h) propagation on CRAFTED plane fields (tests/crafted.py).

Both kernels shape their work from the field they are handed -- hash chains, groups, strips, batches, rounds -- and the
natural fields of the other tests (random planes, a few iterations on a smooth scene) never make a particular limit of that
machinery bind.  Here the field is chosen: one plane everywhere (groups of 128 tasks: several rounds, byte-indexed weights
on boxes 19 / 25), a few planes all over the tile (every group's bounding box is the tile), block-constant planes (many
small groups of mixed strip length), all planes different (the task list exactly full), nothing to do at all, planes that
collide in the hash table across slot 2047 -> 0, and planes whose windows are not safe for the cheap division.

The CPU part states, per case, what the first launch has to do (a census of tasks and groups per tile) and asserts that the
case contains what it is there for.  The GPU part installs the field in a session whose costs stay trusted, runs four
launches (black, red, black, red) under every schedule and compares planes and costs with the CPU oracle, as uint32, after
every launch.  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

from gipuma_amd import abi, synth
from gipuma_amd.problem import AlgorithmParameters, GlobalState, Session
from tests import crafted, oracle_lib
from tests.oracle_lib import OracleState
from tests.test_parity_gpu import _with_env, assert_same

gpu = pytest.mark.gpu

FRAMES = [(21, 9), (32, 16), (33, 17), (70, 40), (96, 64)]
OTHER_BOX_FIELDS = ["one", "interleaved-8", "interleaved-40", "blocks-4x4", "blocks-8x4", "collide-12"]
COLOUR_FIELDS = ["one", "blocks-4x4", "nothing"]

# name -> (push launches, plane-keyed from, fused, first iteration number)
SCHEDULES = {
    "plain": (0, -1, 1, 0),
    "push": (100, -1, 1, 0),
    "split": (0, 0, 0, 0),
    "fused": (0, 0, 1, 0),
    "fused-it2": (0, 0, 1, 2),   # launches numbered from iteration 2: the owner-major task order
}


# ------------------------------------------------------------------------------------------------
# problems: one 96 x 64 rendering per (box, colour), cropped to the frame; the views chosen per case
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(box, colour):
    return synth.build_problem(synth.tiny_config(cols=96, rows=64, n_src=4, blocksize=box, iterations=2, n_best=3),
                               colour=colour)[0]


@functools.lru_cache(maxsize=None)
def problem(box, cols, rows, views=4, n_best=3, colour=False, float_images=False):
    gs = _base(box, colour)
    ap = AlgorithmParameters(**{k: getattr(gs.params, k) for k in vars(gs.params)})
    ap.n_best = n_best
    imgs = [np.ascontiguousarray(im[:rows, :cols]) for im in gs.images]
    if float_images:  # not 8-bit: no weight table, no packed planes
        imgs = [im + np.float32(0.25) * (i + 1) for i, im in enumerate(imgs)]
    if views == 32:   # the reference's costVector[32] limit: 33 cameras, the four sources repeated
        from gipuma_amd.cameras import CameraSet
        cs = CameraSet(33)
        many = []
        for i in range(33):
            src = 0 if i == 0 else 1 + (i - 1) % 4
            C.memmove(C.byref(cs.c_array[i]), C.byref(gs.cameras.c_array[src]), C.sizeof(abi.Camera))
            many.append(imgs[src])
        cs.f = gs.cameras.f
        return GlobalState(many, cs, list(range(1, 33)), ap, seed=7)
    sel = {1: [3], 4: [1, 2, 3, 4], 9: [1, 2, 3, 4, 1, 2, 3, 4, 1]}[views]
    return GlobalState(imgs, gs.cameras, sel, ap, seed=7)


# ------------------------------------------------------------------------------------------------
# 2. the census of every named case (no GPU)
# ------------------------------------------------------------------------------------------------
def _census(name, box=15, cols=96, rows=64):
    gs = problem(box, cols, rows)
    tiles = crafted.census(crafted.make_field(name, gs, abi.BLACK), abi.BLACK, box)
    return gs, tiles, crafted.summary(tiles, box)


def _stops(name, box):
    """stop reasons of every fill of every batch of every tile (crafted.batch_replay) of the 96 x 64 frame"""
    gs = problem(15, 96, 64)   # (the field does not depend on the window; the strips and the sample buffer do)
    return crafted.batch_stops(crafted.census(crafted.make_field(name, gs, abi.BLACK), abi.BLACK, box), box)


@pytest.mark.parametrize("name", crafted.FIELDS)
def test_census_contains_what_the_case_is_there_for(name):
    """per named field, on the 96 x 64 frame (12 full tiles), the structure of the first black launch.  The figures are
    conditions the generators are built to meet, not measurements of a kernel."""
    gs, tiles, s = _census(name)
    print(name, s)
    full = [t for t in tiles if t["n_pixels"] == 256]
    assert len(full) == 12
    if name == "one":
        # rule (D): one task per pixel; two groups (one per x parity) of 128 tasks: the loop of several rounds, and on
        # boxes 19 / 25 more than 32 tasks: byte-indexed weights
        assert all(t["n_tasks"] == 256 and sorted(g[0] for g in t["groups"]) == [128, 128] for t in tiles)
        for box in (11, 15, 19, 25):
            assert _stops(name, box)["rounds"] == 24 and _stops(name, box)["tasks<=32"] == 0
    elif name.startswith("interleaved-"):
        m = int(name.split("-")[1])
        assert all(len(t["groups"]) == 2 * m for t in tiles)
        assert s["full_tile_groups"] >= 3 and s["strip_lengths"] == [15]      # 23 strips x 15 rows for box 15
        if m == 40:
            # groups of at most 64 tasks whose boxes fill the tile: 23 + 23 strips fit the 64 lanes, a third group does not
            assert s["max_group_tasks"] <= 32 and s["max_tasks"] == crafted.MAX_TASKS
            st = s["stops"]
            assert st["rounds"] == 0 and st["strips+tasks"] > 0 and st["tasks"] > 0    # the strip and the task sums bind
            # the sample buffer ALONE stops a fill on boxes 19 and 25: e.g. three groups of 21 strips x 20 rows on box 25
            # are 63 <= 64 strips and at most 64 tasks, but 63 x 21 = 1323 > 1280 samples
            for box in (19, 25):
                assert _stops(name, box)["samples"] > 0, box
        else:
            assert s["max_group_tasks"] > 64 and s["stops"]["rounds"] == 2 * m * 12
    elif name.startswith("blocks-"):
        assert s["max_groups"] > crafted.BATCH_GROUPS and len(s["strip_lengths"]) >= 4   # mixed strip lengths: both cursor ends
        assert s["full_tile_groups"] == 0
        st = s["stops"]
        assert st["mixed-ends"] > 0 and st["tasks<=32"] > 0 and st["tasks33-64"] > 0
        if name == "blocks-2x2":
            assert s["max_groups"] > 400 and s["max_group_tasks"] <= 8
            assert st["groups"] > 0 and st["strips"] > 0       # the 8-group limit, and the 64 strips alone
        if name == "blocks-4x4":
            assert s["max_group_tasks"] <= 32          # boxes 19 / 25: batches of at most 32 tasks, two lanes per task
            assert st["tasks"] > 0 and st["strips"] > 0        # the sum of several groups' tasks; of their strips
            for box in (19, 25):
                b = _stops(name, box)
                assert b["tasks<=32"] > 0 and b["tasks33-64"] > 0 and b["tasks"] > 0 and b["mixed-ends"] > 0, box
            assert _stops(name, 19)["samples"] > 0             # box 19: 1024 samples alone, in the short-end fill
            assert _stops(name, 11)["groups"] > 0
        if name == "blocks-8x4":
            assert 33 <= s["max_group_tasks"] <= 64    # boxes 19 / 25: one lane per task in a batch of 33..64
            assert st["tasks"] > 0 and _stops(name, 19)["samples"] > 0
        if name == "blocks-16x8":
            assert s["max_group_tasks"] > 64 and st["rounds"] > 0   # a several-round group next to small ones
    elif name == "distinct":
        # every interior pixel has 8 tasks: the task list is exactly full.  A plane is held by ONE source pixel, whose (up to)
        # eight consumers have two x parities: groups of at most 4 tasks, and as many groups as (source pixel, parity)
        # pairs -- 2048 groups of one task cannot occur, the fullest hash table a tile can produce is this one
        assert s["max_tasks"] == crafted.MAX_TASKS and s["max_group_tasks"] == 4
        assert s["max_groups"] >= 700 and s["stops"]["groups"] > 0 and s["stops"]["strips"] > 0
    elif name == "nothing":
        assert s["max_tasks"] == 0                     # rule (A) removes every task: the early return, MAXCOST replay
    elif name.startswith("collide-"):
        k = int(name.split("-")[1])
        assert k >= 8
        q = crafted.colliding_planes(gs, k, 7 + 4)
        assert len({p.tobytes() for p in q}) == k and set(crafted.plane_hash(q).tolist()) == {crafted.COLLIDE_RAW}
        for t in tiles:  # every tile: all k planes in both classes, a walk of at least k - 1 steps, across 2047 -> 0
            assert len(t["groups"]) == 2 * k and t["probe"] >= k - 1 and t["wrapped"]
        assert s["max_group_tasks"] > 64               # the `one` share: matches inside the chain
        assert s["stops"]["rounds"] == 24 and s["stops"]["tasks"] > 0
    elif name in ("degenerate", "degenerate-nan"):
        planes, kinds = crafted.degenerate_pool(gs, 7 + 5, name.endswith("nan"))
        assert all(len(t["groups"]) == 2 * len(kinds) for t in tiles)   # zero+ and zero- are two groups per parity
        by = dict(zip(kinds, planes))
        assert np.array_equal(by["zero+"], by["zero-"]) and by["zero+"].tobytes() != by["zero-"].tobytes()
        for kind in ("d-zero", "d-tiny"):
            assert crafted.unsafe_views(gs, by[kind], 0, 31, 0, 15), kind
        assert not crafted.unsafe_views(gs, by["plain"], 0, 31, 0, 15)
        L, cam = oracle_lib.lib(), gs.cameras.c_array[0]
        depth = {k: L.gipuma_oracle_depth_from_plane(C.byref(cam), oracle_lib.fptr(by[k]), 48, 32) for k in kinds}
        assert depth["too-far"] > gs.params.depthMax and 0 < depth["too-near"] < gs.params.depthMin and depth["behind"] < 0
        assert gs.params.depthMin < depth["plain"] < gs.params.depthMax
    else:
        raise AssertionError("no condition written for " + name)


def test_census_of_ragged_and_tiny_frames():
    """the frames of the GPU cases that are not whole tiles: partial tiles, and a frame below one tile and the window"""
    for cols, rows, n_tiles in ((21, 9, 1), (32, 16, 1), (33, 17, 4), (70, 40, 9)):
        gs, tiles, s = _census("one", cols=cols, rows=rows)
        assert len(tiles) == n_tiles and sum(t["n_pixels"] for t in tiles) == (cols * rows + 1) // 2
        assert all(len(t["groups"]) <= 2 for t in tiles)
    gs, tiles, s = _census("one", cols=33, rows=17)
    assert sorted(t["n_pixels"] for t in tiles) == [1, 8, 16, 256]


def test_plane_hash_restatement():
    """pm::plane_hash by hand for one plane: uint32 products wrap"""
    p = np.array([1.0, 0.0, -1.0, 2.5], dtype=np.float32)
    b = [int(v) for v in p.view(np.uint32)]
    h = (b[0] * 0x9E3779B1) & 0xFFFFFFFF
    for w, k in ((b[1], 0x85EBCA77), (b[2], 0xC2B2AE3D), (b[3], 0x27D4EB2F)):
        h = ((h ^ w) * k) & 0xFFFFFFFF
    h ^= h >> 15
    assert int(crafted.plane_hash(p, 1)) == (h + 1) & 2047


# ------------------------------------------------------------------------------------------------
# 3. the GPU part
# ------------------------------------------------------------------------------------------------
_hip_rt = []


def _hip_runtime():
    """the HIP runtime the library under test is bound to: the soname in its dynamic section, opened with RTLD_NOLOAD
    (the dynamic linker keeps one object per soname, so this is the very object whose allocations the session holds --
    nothing new is loaded or initialised)"""
    if not _hip_rt:
        import os
        import re
        lib_path = abi.load_library()._name
        with open(lib_path, "rb") as f:
            m = re.search(rb"libamdhip64\.so(\.\d+)*", f.read())
        assert m, "the library under test does not name a HIP runtime"
        soname = m.group(0).decode()
        try:
            rt = C.CDLL(soname, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        except OSError:  # (a loader that does not find a loaded object by its soname: the file mapped under that name)
            with open("/proc/self/maps") as f:
                paths = sorted({ln.split()[-1] for ln in f if os.path.basename(ln.split()[-1]).startswith(soname)})
            assert len(paths) == 1, paths
            rt = C.CDLL(paths[0])
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipMemcpy.restype = C.c_int
        rt.hipDeviceSynchronize.restype = C.c_int
        _hip_rt.append(rt)
    return _hip_rt[0]


def install_state(s, planes, cost):
    """Overwrite a session's planes and costs IN PLACE, through gipuma_hip_state_device_ptrs, and leave its bookkeeping
    alone.  include/gipuma_hip.h asks a caller that writes through these pointers to call gipuma_hip_set_state(s, NULL, NULL)
    afterwards, which marks the costs untrusted -- and launch_sweep then runs neither push nor plane-keyed propagation,
    the kernels these tests are about.  The call is left out on purpose: the session comes straight from init_planes()
    (costs trusted, history void, rule (S) rings and early-termination hints fresh), and the costs installed ARE the
    costs of the planes installed (the oracle's, bit-identical to the kernels'), so everything the session believes
    about its state is true by construction."""
    planes = np.ascontiguousarray(planes, dtype=np.float32)
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    s.sync()
    d_n4, d_c = s.state_device_ptrs()
    rt = _hip_runtime()
    assert rt.hipMemcpy(d_n4, planes.ctypes.data, planes.nbytes, 1) == 0   # 1 = hipMemcpyHostToDevice
    assert rt.hipMemcpy(d_c, cost.ctypes.data, cost.nbytes, 1) == 0
    assert rt.hipDeviceSynchronize() == 0
    n4, c = s.get_state()
    assert np.array_equal(crafted.bits(n4), crafted.bits(planes)) and np.array_equal(crafted.bits(c), crafted.bits(cost))


def _launches(it0):
    return [(it0, abi.BLACK), (it0, abi.RED), (it0 + 1, abi.BLACK), (it0 + 1, abi.RED)]


_ORACLE = {}


def oracle_run(key, gs, field, it0, flavour=None):
    """(costs of the field, the oracle's state after each of the four launches), computed once per case and shared"""
    k = key + (it0, flavour)
    if k not in _ORACLE:
        L = oracle_lib.lib()
        if flavour is not None:
            L.gipuma_oracle_set_flavour(flavour)
        try:
            o = OracleState(gs)
            cost = o.eval_cost(field)
            o.norm4, o.cost = np.ascontiguousarray(field.copy()), np.ascontiguousarray(cost.copy())
            states = []
            for it, colour in _launches(it0):
                o.sweep(it, colour)
                states.append((o.norm4.copy(), o.cost.copy()))
        finally:
            if flavour is not None:
                L.gipuma_oracle_set_flavour(-1)
        for a in (cost,) + tuple(x for st in states for x in st):
            a.setflags(write=False)
        _ORACLE[k] = (cost, states)
    return _ORACLE[k]


def session_run(gs, field, cost, schedule, et=1, expect_group=True, expect_push=True, **mode):
    """the four launches of one schedule on a session that holds (field, cost); the state after each.  The schedule the
    session reports must be the one asked for: a case must not pass because its kernel was quietly not chosen."""
    push, group_from, fused, it0 = SCHEDULES[schedule]
    env = {"GIPUMA_HIP_PUSH_LAUNCHES": push, "GIPUMA_HIP_GROUP_FROM": group_from, "GIPUMA_HIP_GROUP_FUSED": fused,
           "GIPUMA_HIP_ET_FORCE": et}

    def run():
        out = []
        with Session(gs, **mode) as s:
            sch = s.schedule()
            assert sch["push_launches"] == (push if expect_push else 0), (schedule, sch)
            assert sch["group_from"] == (group_from if expect_group else -1), (schedule, sch)
            if group_from >= 0 and expect_group and gs.channels == 1:
                assert sch["group_fused"] == bool(fused), (schedule, sch)
            s.init_planes()
            install_state(s, field, cost)
            for it, colour in _launches(it0):
                s.sweep(it, colour)
                out.append(s.get_state())
        return out
    return _with_env(env, run)


def check_case(key, gs, name, schedules=tuple(SCHEDULES), et=1, flavour=None, **kw):
    field = crafted.make_field(name, gs, abi.BLACK)
    runs = {}
    for sch in schedules:
        cost, want = oracle_run(key + (name,), gs, field, SCHEDULES[sch][3], flavour)
        runs[sch] = got = session_run(gs, field, cost, sch, et=et, **kw)
        for k, ((n4, c), (o4, oc)) in enumerate(zip(got, want)):
            assert_same(n4, o4, "%s %s launch %d norm4" % (name, sch, k))
            assert_same(c, oc, "%s %s launch %d cost" % (name, sch, k))
    same_numbering = [s for s in schedules if SCHEDULES[s][3] == 0]
    for sch in same_numbering[1:]:  # (implied by the above; stated because it is the property the schedules promise)
        for k in range(4):
            assert_same(runs[sch][k][0], runs[same_numbering[0]][k][0], "%s %s vs %s launch %d" % (name, sch, same_numbering[0], k))
            assert_same(runs[sch][k][1], runs[same_numbering[0]][k][1], "%s %s vs %s launch %d cost" % (name, sch, same_numbering[0], k))
    return field, runs


@gpu
@pytest.mark.parametrize("cols,rows", FRAMES)
@pytest.mark.parametrize("name", crafted.FIELDS)
def test_box15_every_field_every_schedule(hip, name, cols, rows):
    """box 15, 4 views, best-3: every field on every frame under every schedule, against the oracle after each launch.
    (degenerate-nan: a NaN plane distance in the sources.  No NaN that is compared here is the RESULT of an operation, whose
    payload and sign a CPU and a GPU may choose differently: a NaN depth fails the range test of the propagation and a NaN
    cost fails the strict < of every accept test, so nobody adopts the NaN plane, and its holder -- whose installed cost is
    a NaN too or not, no candidate's NaN cost can replace it -- either keeps plane and cost, copied bit for bit, or takes a
    finite candidate: getDepthFromPlane3 returns 1000 for a NaN d and fminf / fmaxf drop a NaN operand in the refinement's
    clamps.  The test asserts exactly that: every NaN after a launch sits where the installed state had the same bits.)"""
    gs = problem(15, cols, rows)
    field, runs = check_case((15, cols, rows, 4), gs, name)
    if name == "degenerate-nan":
        cost = oracle_run((15, cols, rows, 4, name), gs, field, 0)[0]
        assert np.isnan(field).any()
        for sch, states in runs.items():
            for n4, c in states:
                m4, mc = np.isnan(n4), np.isnan(c)
                assert np.array_equal(crafted.bits(n4)[m4], crafted.bits(field)[m4]), sch
                assert np.array_equal(crafted.bits(c)[mc], crafted.bits(cost)[mc]), sch
    if name == "nothing":  # the scenario bites: the first launch found no task, and refinement still moved the planes
        assert (crafted.bits(runs["fused"][0][0]) != crafted.bits(field)).any()


@gpu
@pytest.mark.parametrize("cols,rows", [(64, 1), (1, 40)])
@pytest.mark.parametrize("name", ["one", "distinct"])
def test_box15_one_pixel_wide_frames(hip, name, cols, rows):
    check_case((15, cols, rows, 4), problem(15, cols, rows), name)


@gpu
@pytest.mark.parametrize("cols,rows", FRAMES)
@pytest.mark.parametrize("name", OTHER_BOX_FIELDS)
@pytest.mark.parametrize("box", [11, 19, 25])
def test_other_boxes(hip, box, name, cols, rows):
    """boxes 11 (36 chain weights), 19 and 25 (two lanes per task up to 32 tasks, byte-indexed weights above)"""
    check_case((box, cols, rows, 4), problem(box, cols, rows), name)


@gpu
@pytest.mark.parametrize("cols,rows", FRAMES)
@pytest.mark.parametrize("name", COLOUR_FIELDS)
def test_colour_box15(hip, name, cols, rows):
    """pm::group_kernel<15, 4> in front of the colour sweep kernel (colour sessions never fuse), pm::push_kernel_c4; rule (S)
    rings fresh from the init"""
    check_case((15, cols, rows, 4, "colour"), problem(15, cols, rows, colour=True), name)


@gpu
@pytest.mark.parametrize("views,n_best,cols,rows", [(1, 3, 33, 17), (1, 3, 96, 64), (9, 3, 33, 17), (9, 3, 70, 40),
                                                      (32, 4, 33, 17)])
@pytest.mark.parametrize("name", ["one", "interleaved-40", "blocks-4x4", "degenerate"])
def test_view_counts(hip, name, views, n_best, cols, rows):
    """one view with n_best 3; 9 views: a partial last block of four homographies; 32 views: eight blocks"""
    check_case((15, cols, rows, views, n_best), problem(15, cols, rows, views=views, n_best=n_best), name)


@gpu
@pytest.mark.parametrize("box,name,cols,rows", [(15, "interleaved-3", 96, 64), (15, "blocks-2x2", 70, 40), (15, "collide-12", 33, 17),
                                               (15, "degenerate", 96, 64), (25, "one", 70, 40), (19, "blocks-8x4", 96, 64),
                                               (11, "interleaved-8", 33, 17)])
def test_every_workgroup_bounds_every_step(hip, box, name, cols, rows):
    """GIPUMA_HIP_ET_FORCE=2: bounded evaluation in every workgroup, on a subset"""
    check_case((box, cols, rows, 4), problem(box, cols, rows), name, et=2)


@gpu
@pytest.mark.parametrize("box,name,cols,rows", [(15, "one", 96, 64), (15, "interleaved-40", 70, 40), (15, "blocks-4x4", 33, 17),
                                               (15, "collide-12", 96, 64), (15, "degenerate", 70, 40), (15, "nothing", 32, 16),
                                               (15, "distinct", 96, 64), (25, "blocks-8x4", 70, 40), (19, "one", 33, 17),
                                               (11, "blocks-4x4", 96, 64)])
def test_literal_mode(hip, box, name, cols, rows):
    """the reference-order flavour of the same kernels against the oracle's flavour 7"""
    check_case((box, cols, rows, 4), problem(box, cols, rows), name, flavour=7, literal=True)


@gpu
@pytest.mark.parametrize("box,name,cols,rows", [(15, "one", 96, 64), (15, "interleaved-8", 70, 40), (15, "blocks-4x4", 33, 17),
                                               (15, "collide-12", 96, 64), (15, "nothing", 32, 16), (25, "one", 70, 40)])
def test_fast_mode_schedules_agree(hip, box, name, cols, rows):
    """the tolerance-judged flavour has no bit-exact reference (tests/test_fast_mode.py judges it by tolerance on
    free-running solves and has no launch-by-launch comparison to join): its schedules must equal ONE ANOTHER bit for bit.
    The installed costs are the fast session's own evaluation of the field."""
    gs = problem(box, cols, rows)
    field = crafted.make_field(name, gs, abi.BLACK)
    with Session(gs, fast=True) as s:
        cost = s.eval_cost(field)
    runs = {sch: session_run(gs, field, cost, sch, fast=True) for sch in ("plain", "push", "split", "fused")}
    for sch in ("push", "split", "fused"):
        for k in range(4):
            assert_same(runs[sch][k][0], runs["plain"][k][0], "fast %s %s vs plain launch %d norm4" % (name, sch, k))
            assert_same(runs[sch][k][1], runs["plain"][k][1], "fast %s %s vs plain launch %d cost" % (name, sch, k))


@gpu
@pytest.mark.parametrize("what", ["n_best_5", "float_images"])
@pytest.mark.parametrize("name", ["one", "blocks-4x4"])
def test_unsupported_combinations_fall_back_by_themselves(hip, name, what):
    """n_best = 5 (the LDS combiner) and images that are not 8-bit: asked for plane-keyed and push propagation, the session
    must report that it runs neither, and still give the oracle's bits"""
    gs = problem(15, 70, 40, n_best=5) if what == "n_best_5" else problem(15, 70, 40, float_images=True)
    check_case((15, 70, 40, what), gs, name, schedules=("split", "fused", "push"), expect_group=False, expect_push=False)


@gpu
def test_fused_interleaved_3_is_deterministic(hip):
    """six groups of 128 tasks per tile, four wavefronts on the two-ended cursor: the most contention a tile can have;
    three runs, byte-identical (and the oracle's)"""
    gs = problem(15, 96, 64)
    field = crafted.make_field("interleaved-3", gs, abi.BLACK)
    cost, want = oracle_run((15, 96, 64, 4, "interleaved-3"), gs, field, 0)
    runs = [session_run(gs, field, cost, "fused") for _ in range(3)]
    for r in runs:
        for k in range(4):
            assert r[k][0].tobytes() == runs[0][k][0].tobytes() and r[k][1].tobytes() == runs[0][k][1].tobytes()
            assert_same(r[k][0], want[k][0], "launch %d norm4" % k)
            assert_same(r[k][1], want[k][1], "launch %d cost" % k)
