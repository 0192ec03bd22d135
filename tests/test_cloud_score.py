"""The cloud score (gipuma_amd.cloud_eval): its arithmetic on hand-made distances, the header-driven PLY
reader, the command lines' argument checks, a k-d tree as a second opinion on the restatement (tests/cloud_ref.py).  GPU:
a cloud against itself and against a translated copy, and a small scan solved, fused and scored by the batch runner."""
import json
import math

import numpy as np
import pytest

from gipuma_amd import cameras, cloud_eval, dmb, synth
from tests import cloud_ref

f32 = np.float32
INF = np.inf


# ----------------------------------------------------------------------------------------------------------------------
# the score's arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def test_score_arithmetic_on_hand_made_distances():
    # cloud: distances 0, 0.5, 1, 3 and one "none"; reference: 0.25, 2 and two "none"
    acc, prec = cloud_eval.direction_score(np.array([0.0, 0.25, 1.0, 9.0, INF], f32), (0.5, 1.0, 2.0))
    comp, rec = cloud_eval.direction_score(np.array([0.0625, 4.0, INF, INF], f32), (0.5, 1.0, 2.0))
    assert acc == {"mean": pytest.approx(4.5 / 4), "median": pytest.approx(0.75), "found": 4, "none": 1}
    assert comp == {"mean": pytest.approx(2.25 / 2), "median": pytest.approx(1.125), "found": 2, "none": 2}
    assert prec == [pytest.approx(2 / 5), pytest.approx(3 / 5), pytest.approx(3 / 5)]  # of ALL points: "none" is a miss
    assert rec == [pytest.approx(1 / 4), pytest.approx(1 / 4), pytest.approx(2 / 4)]   # (the threshold is inclusive)
    out = cloud_eval.combine(acc, prec, comp, rec, (0.5, 1.0, 2.0))
    assert out["fscore"][0] == pytest.approx(2 * 0.4 * 0.25 / 0.65) and out["fscore"][2] == pytest.approx(2 * 0.6 * 0.5 / 1.1)
    assert out["accuracy"] is acc and out["completeness"] is comp and out["thresholds"] == [0.5, 1.0, 2.0]


def test_score_of_empty_and_unmatched_clouds_does_not_raise():
    empty, p0 = cloud_eval.direction_score(np.zeros(0, f32), (1.0,))
    assert math.isnan(empty["mean"]) and math.isnan(empty["median"]) and (empty["found"], empty["none"]) == (0, 0)
    assert p0 == [0.0]
    lost, p1 = cloud_eval.direction_score(np.full(3, INF, f32), (1.0,))
    assert math.isnan(lost["mean"]) and (lost["found"], lost["none"]) == (0, 3) and p1 == [0.0]
    assert cloud_eval.combine(empty, p0, lost, p1, (1.0,))["fscore"] == [0.0]  # P = R = 0


# ----------------------------------------------------------------------------------------------------------------------
# read_ply_xyz
# ----------------------------------------------------------------------------------------------------------------------
def _own_ply(path, n=37):
    rng = np.random.default_rng(5)
    v = np.zeros(n, dtype=dmb._PLY_VERTEX)
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        v[k] = rng.normal(size=n).astype(f32)
    v["red"] = v["green"] = v["blue"] = rng.integers(0, 256, n)
    dmb.write_points_ply(path, v)
    return v


def test_read_ply_xyz_reads_this_project_s_own_files(tmp_path):
    p = str(tmp_path / "own.ply")
    v = _own_ply(p)
    xyz = dmb.read_ply_xyz(p)
    assert xyz.dtype == f32 and xyz.shape == (37, 3)
    assert np.array_equal(xyz, np.stack([v["x"], v["y"], v["z"]], -1))
    dmb.write_points_ply(p, v[:0])
    assert dmb.read_ply_xyz(p).shape == (0, 3)


ASCII = ("ply\nformat ascii 1.0\ncomment a scanner's file\nelement face 1\nproperty list uchar int vertex_indices\n"
         "element vertex 3\nproperty double z\nproperty uchar intensity\nproperty double x\nproperty list uchar int tags\n"
         "property float y\nend_header\n3 0 1 2\n1.5 255 2.5 2 7 8 3.5\n-1 0 -2 0 -3\n1e3 9 0.125 1 4 -0.5\n")


def test_read_ply_xyz_ascii_with_other_properties_lists_and_elements(tmp_path):
    p = str(tmp_path / "a.ply")
    open(p, "w").write(ASCII)
    assert dmb.read_ply_xyz(p).tolist() == [[2.5, 3.5, 1.5], [-2.0, -3.0, -1.0], [0.125, -0.5, 1000.0]]


def _binary_double(path, n=11, count=None, extra=b""):
    """binary little endian: a `range` element with a list first, then vertices of (uchar, double x, double y, short, double z)"""
    rng = np.random.default_rng(6)
    dt = np.dtype([("c", "u1"), ("x", "<f8"), ("y", "<f8"), ("s", "<i2"), ("z", "<f8")])
    v = np.zeros(n, dtype=dt)
    for k in "xyz":
        v[k] = rng.normal(size=n) * 100
    head = ("ply\nformat binary_little_endian 1.0\nelement range 2\nproperty list uchar short span\nproperty int id\n"
            "element vertex %d\nproperty uchar c\nproperty double x\nproperty double y\nproperty short s\n"
            "property double z\nend_header\n" % (n if count is None else count)).encode()
    ranges = b"\x02" + np.array([5, 6], "<i2").tobytes() + np.array([1], "<i4").tobytes() + b"\x00" + np.array([2], "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(head + ranges + v.tobytes() + extra)
    return v


def test_read_ply_xyz_binary_doubles_behind_another_element(tmp_path):
    p = str(tmp_path / "d.ply")
    v = _binary_double(p, extra=b"trailing element data")
    assert np.array_equal(dmb.read_ply_xyz(p), np.stack([v["x"], v["y"], v["z"]], -1).astype(f32))


def test_read_ply_xyz_refuses_malformed_files(tmp_path):
    p = str(tmp_path / "bad.ply")
    _own_ply(p)
    whole = open(p, "rb").read()
    open(p, "wb").write(whole[:-5])  # truncated
    with pytest.raises(ValueError, match="cannot hold"):
        dmb.read_ply_xyz(p)
    open(p, "wb").write(whole.replace(b"property float y\n", b"property float why\n"))  # no y
    with pytest.raises(ValueError, match="no property y"):
        dmb.read_ply_xyz(p)
    open(p, "wb").write(whole.replace(b"binary_little_endian", b"binary_big_endian"))
    with pytest.raises(ValueError, match="binary_big_endian"):
        dmb.read_ply_xyz(p)
    _binary_double(p, n=4, count=10 ** 15)  # a count the file cannot hold: refused before 37 PB are asked for
    with pytest.raises(ValueError, match="cannot hold"):
        dmb.read_ply_xyz(p)
    open(p, "w").write(ASCII.replace("element vertex 3", "element vertex 3000000000000"))
    with pytest.raises(ValueError, match="cannot hold"):
        dmb.read_ply_xyz(p)
    open(p, "w").write(ASCII[:-len("1e3 9 0.125 1 4 -0.5\n")] + "1e3 9 0.125 1\n" + " " * 40)  # a vertex cut short
    with pytest.raises(ValueError, match="incomplete"):
        dmb.read_ply_xyz(p)
    open(p, "wb").write(whole[:whole.index(b"property float nx")])  # no end_header
    with pytest.raises(ValueError, match="end_header"):
        dmb.read_ply_xyz(p)
    open(p, "wb").write(whole.replace(b"property float x", b"property int x"))
    with pytest.raises(ValueError, match="float or double"):
        dmb.read_ply_xyz(p)
    open(p, "wb").write(b"P5\n1 1\n255\n0")
    with pytest.raises(ValueError, match="not a PLY"):
        dmb.read_ply_xyz(p)


# ----------------------------------------------------------------------------------------------------------------------
# command lines
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--reference", "r.ply"], ["--cloud", "c.ply"],
    ["--cloud", "c.ply", "--reference", "r.ply", "--max_dist", "0"],
    ["--cloud", "c.ply", "--reference", "r.ply", "--max_dist", "nan"],
    ["--cloud", "c.ply", "--reference", "r.ply", "--thresholds", "1,x"],
    ["--cloud", "c.ply", "--reference", "r.ply", "--thresholds", ""],
    ["--cloud", "c.ply", "--reference", "r.ply", "--thresholds", "1,-2"],
    ["--cloud", "c.ply", "--reference", "r.ply", "--grid", "257"]])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cloud_eval.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_arguments():
    a = cloud_eval.parse_args(["--cloud", "c.ply", "--reference", "r.ply", "--thresholds", "0.5,1,2", "--max_dist", "0.1"])
    assert a.thresholds == [0.5, 1.0, 2.0] and a.max_dist == float(f32(0.1)) and a.output is None and a.grid == 0


def test_batch_refuses_eval_cloud_without_fuse(capsys):
    from gipuma_amd import batch
    base = ["--images-folder", "i", "--p-folder", "p", "--output-folder", "o"]
    with pytest.raises(SystemExit) as e:
        batch.parse_args(base + ["--eval_cloud", "gt.ply"])
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        batch.parse_args(base + ["--fuse", "--eval_cloud", "gt.ply", "--eval_max_dist", "0"])
    a = batch.parse_args(base + ["--fuse", "--eval_cloud", "gt.ply"])
    assert a.eval_cloud == "gt.ply" and a.eval_max_dist == 20.0
    assert batch.parse_args(base).eval_cloud is None


# ----------------------------------------------------------------------------------------------------------------------
# a second opinion on the restatement
# ----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_a_kd_tree():
    from scipy.spatial import cKDTree
    from tests.test_cloud_eval import case
    c = case("found_and_none")
    max_dist = float(c.max_dist)
    dist, j = cKDTree(c.targets.astype(np.float64)).query(c.queries.astype(np.float64), distance_upper_bound=max_dist * 2)
    band = np.abs(dist - max_dist) <= 1e-5 * max_dist
    r = c.ref
    assert np.array_equal((r.idx >= 0)[~band], (dist <= max_dist)[~band])  # the same queries find a neighbour
    both = (r.idx >= 0) & (dist <= max_dist)
    # d2 in float32: three squares of differences of coordinates up to 110 (rounded to 2^-17 each), two sums -- a few
    # 2^-24 of the coordinates' squares; on the distance itself 1e-4 absolute is ample and far below the cloud's spacing
    assert np.abs(np.sqrt(r.d2[both].astype(np.float64)) - dist[both]).max() < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_cloud_scored_against_itself_and_against_a_translated_copy(hip):
    rng = np.random.default_rng(17)
    cloud = rng.uniform(0.0, 30.0, (4000, 3)).astype(f32)
    cloud[100:200] = cloud[:100]  # duplicates: the lower index answers
    d2, idx, ms = cloud_eval.nearest(cloud, cloud, 1.0)
    assert (d2 == 0).all() and (idx <= np.arange(4000)).all() and (idx[100:200] == np.arange(100)).all() and ms > 0
    s = cloud_eval.score(cloud, cloud, max_dist=1.0, thresholds=(0.0, 0.5))
    assert s["precision"] == [1.0, 1.0] and s["recall"] == [1.0, 1.0] and s["fscore"] == [1.0, 1.0]
    assert s["accuracy"] == {"mean": 0.0, "median": 0.0, "found": 4000, "none": 0} == s["completeness"]
    # coordinates on a 1/4 lattice: the translation is exact in float32
    lattice = np.round(cloud * 4) / 4
    moved = lattice + np.array([0.25, 0.0, 0.0], f32)
    s = cloud_eval.score(moved, lattice, max_dist=1.0, thresholds=(0.25,))
    d2 = cloud_eval.nearest(moved, lattice, 1.0)[0]
    assert (np.sqrt(d2.astype(np.float64)) <= 0.25).all() and s["accuracy"]["none"] == 0 == s["completeness"]["none"]
    assert s["precision"] == [1.0] and s["recall"] == [1.0] and 0 < s["accuracy"]["mean"] <= 0.25
    assert s["cloud_points"] == s["reference_points"] == 4000 and s["accuracy_device_ms"] > 0


@pytest.mark.gpu
def test_batch_fuse_eval_cloud_scores_the_fused_cloud(hip, tmp_path):
    """a small synthetic scan solved, fused and scored by the batch runner against the cloud back-projected from its
    ground-truth depth; the counts equal the restatement's.  No bound on the score itself: nobody has measured one."""
    from gipuma_amd import batch
    cfg = synth.tiny_config(cols=96, rows=64, n_src=4, blocksize=9, iterations=3, n_best=2)
    scan = synth.build_scan(cfg)
    img_dir, p_dir, out = tmp_path / "img", tmp_path / "calib", tmp_path / "out"
    img_dir.mkdir()
    p_dir.mkdir()
    reference = []
    y, x = np.mgrid[0:cfg["rows"], 0:cfg["cols"]].astype(np.float64)
    for im, vid, P, z in zip(scan.images, scan.view_ids, scan.P_matrices, scan.gt_depth):
        name = "rect_%03d.pgm" % vid
        with open(img_dir / name, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (cfg["cols"], cfg["rows"]) + im.astype(np.uint8).tobytes())
        with open(p_dir / (name + ".P"), "w") as f:
            for r in P:
                f.write(" ".join("%.6f" % v for v in r) + "\n")
        k = cameras.view_constants(P, scan.cam_scale)
        ray = np.stack([x, y, np.ones_like(x)], -1) @ np.asarray(k["bp"], dtype=np.float64).reshape(3, 3).T
        reference.append((np.asarray(k["c"], dtype=np.float64) + z.astype(np.float64)[..., None] * ray).reshape(-1, 3))
    reference = np.concatenate(reference)
    gt = np.zeros(len(reference), dtype=dmb._PLY_VERTEX)
    gt["x"], gt["y"], gt["z"] = reference.T
    dmb.write_points_ply(str(tmp_path / "gt.ply"), gt)
    rc = batch.main(["--images-folder", str(img_dir), "--p-folder", str(p_dir), "--output-folder", str(out),
                     "--blocksize=9", "--iterations=3", "--n_best=2", "--min_angle=2", "--max_angle=60", "--max_views=10",
                     "--depth_min=300", "--depth_max=800", "--cam_scale=%.9g" % np.float32(cfg["cam_scale"]),
                     "--disp_thresh=0.02", "--normal_thresh=30", "--num_consistent=2", "--fuse",
                     "--eval_cloud", str(tmp_path / "gt.ply"), "--eval_max_dist", "20"])
    assert rc == 0
    rep = json.load(open(out / "batch_rank0.json"))
    s = rep["cloud_score"]
    fused = dmb.read_ply_xyz(str(out / "fused.ply"))
    ref_xyz = dmb.read_ply_xyz(str(tmp_path / "gt.ply"))
    assert s["cloud_points"] == len(fused) == rep["fusion"]["points"] > 0 and s["reference_points"] == len(ref_xyz)
    acc, comp = cloud_ref.nearest(fused, ref_xyz, 20.0), cloud_ref.nearest(ref_xyz, fused, 20.0)
    assert (s["accuracy"]["found"], s["accuracy"]["none"]) == (acc.found, acc.none)
    assert (s["completeness"]["found"], s["completeness"]["none"]) == (comp.found, comp.none)
    assert acc.found > 0 and comp.found > 0
    for side, r in (("accuracy", acc), ("completeness", comp)):
        assert math.isfinite(s[side]["mean"]) and math.isfinite(s[side]["median"])
        assert s[side]["mean"] == pytest.approx(float(np.sqrt(r.d2[r.idx >= 0].astype(np.float64)).mean()), rel=1e-12)
    print("cloud_score of the 96x64 scan: accuracy %r, completeness %r, F %r" % (s["accuracy"], s["completeness"], s["fscore"]))
    assert s["accuracy_device_ms"] > 0 and s["completeness_device_ms"] > 0 and s["reference"].endswith("gt.ply")
