"""bench.py's result line and its --dump-outputs files: the plain run prints the headline fields only, and what it
writes is what the timed path hands its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_whole_arrays_within_the_budget(tmp_path):
    import bench
    n4 = np.arange(6 * 5 * 4, dtype=np.float32).reshape(6, 5, 4)
    cost = np.arange(6 * 5, dtype=np.float32).reshape(6, 5)
    bench.dump_outputs(str(tmp_path), {"norm4": n4, "cost": cost}, 1 << 20)
    assert sorted(os.listdir(tmp_path)) == ["cost.npy", "norm4.npy"]
    assert np.array_equal(np.load(tmp_path / "norm4.npy"), n4)
    assert np.array_equal(np.load(tmp_path / "cost.npy"), cost)


def test_dump_outputs_samples_the_same_pixels_of_every_array_over_the_budget(tmp_path):
    import bench
    rows, cols = 40, 30
    n4 = np.random.default_rng(1).random((rows, cols, 4), dtype=np.float32)
    cost = np.random.default_rng(2).random((rows, cols), dtype=np.float32)
    budget = 2000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"norm4": n4, "cost": cost}, budget, "_rank1")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["cost_rank1.npy", "norm4_rank1.npy", "pixel_index_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget + 3 * 128  # (+ the .npy headers)
    idx = np.load(tmp_path / "a" / "pixel_index_rank1.npy")
    assert idx.dtype == np.float64 and len(idx) > 0 and np.all(np.diff(idx) > 0)
    flat = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "norm4_rank1.npy"), n4.reshape(-1, 4)[flat])
    assert np.array_equal(np.load(tmp_path / "a" / "cost_rank1.npy"), cost.reshape(-1)[flat])
    for f in files:  # a fixed sample: the same from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_path_computes(hip, tmp_path):
    """a plain run (no --full) on config A: the headline fields, none of the --full ones, and norm4 / cost of its last
    step equal to a solve of the same problem through runcuda(), bit for bit"""
    from gipuma_amd import synth
    from gipuma_amd.problem import runcuda
    from gipuma_amd.shard import views_for_rank
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "A", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("roofline", "quality", "cpu_baseline", "value_exhaustive", "value_fast"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["cost.npy", "norm4.npy"]
    gs, _ = synth.build_problem("A", ref_view=views_for_rank(synth.DTU_REF_VIEWS, 0, 1)[0])
    n4, cost = runcuda(gs)
    got_n4, got_cost = np.load(out / "norm4.npy"), np.load(out / "cost.npy")
    assert got_n4.dtype == np.float32 and got_n4.shape == (gs.rows, gs.cols, 4)
    assert np.array_equal(got_n4.view(np.uint32), n4.view(np.uint32))
    assert np.array_equal(got_cost.view(np.uint32), cost.view(np.uint32))
