"""bench.py's two kinds of run: a plain one (the headline figure alone) with --dump-outputs, whose image must be the oracle's image of the
same frames bit for bit and must repeat exactly from run to run, and a --full one, which still carries everything beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "compute", "counters_per_frame", "frame_batched", "cpu_baseline", "cpu_baseline_reference")


def bench(*args, gpus=1, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), *args], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_frame(tmp_path, rt, oracle):
    runs = []
    for name in ("a", "b"):
        d = bench("--config", "C1", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path / name))
        assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY), sorted(d)
        assert d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / name)) == ["image.npy"]
        runs.append(np.load(tmp_path / name / "image.npy"))
    a, b = runs
    assert a.dtype == np.float32 and a.shape == (256, 256, 4)
    assert (a.view(np.uint32) == b.view(np.uint32)).all(), "two runs with the same arguments dumped different images"
    # the image a caller receives after warm-up + timed frames 1 .. 8 of C1
    sc = rt.scenes
    cfg = sc.CONFIGS["C1"]
    scene, g = cfg["scene"](), sc.GlibcRand(0)
    want = np.zeros((256, 256, 4), np.float32)
    for f in range(1, 9):
        oracle.render(scene, cfg["params"]().replace(frames=f, random=g.rand()), want, threads=16)
    neq = (a.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{int(neq.sum())} of {neq.size} pixels of the dumped image differ from the oracle"


@pytest.mark.gpu
def test_two_ranks_dump_the_image_of_one(tmp_path):
    """--gpus 2 (the test mapping of tests/test_gpu_bench_launcher.py: both ranks on device 0): rank 0 dumps the gathered image, and it
    is the one-rank image bit for bit."""
    args = ("--config", "C1", "--steps", "4", "--warmup", "1", "--dump-outputs")
    assert bench(*args, str(tmp_path / "one"))["n_gpus"] == 1
    assert bench(*args, str(tmp_path / "two"), gpus=2, RTGL_BENCH_SHARED_DEVICE="1")["n_gpus"] == 2
    one, two = np.load(tmp_path / "one" / "image.npy"), np.load(tmp_path / "two" / "image.npy")
    assert one.shape == two.shape == (256, 256, 4) and (one.view(np.uint32) == two.view(np.uint32)).all()


def test_large_outputs_are_dumped_as_a_fixed_sample(tmp_path):
    """(no GPU) above 64 MiB: the same seeded pixels every time, in pixel order."""
    sys.path.insert(0, ROOT)
    import bench as b
    img = np.arange(2160 * 3840 * 4, dtype=np.float32).reshape(2160, 3840, 4)
    b.dump_outputs(str(tmp_path / "a"), img)
    b.dump_outputs(str(tmp_path / "b"), img)
    sa, sb = np.load(tmp_path / "a" / "image_sample.npy"), np.load(tmp_path / "b" / "image_sample.npy")
    assert sa.dtype == np.float32 and sa.shape[1] == 4 and sa.nbytes <= b.DUMP_LIMIT_BYTES
    assert (sa == sb).all() and (np.diff(sa[:, 0]) > 0).all()


@pytest.mark.gpu
def test_full_run_carries_the_other_figures():
    d = bench("--config", "C1", "--steps", "8", "--warmup", "2", "--full", "--cpu-rows", "16")
    assert all(k in d for k in HEADLINE) and all(k in d for k in FULL_ONLY), sorted(d)
    assert d["counters_per_frame"]["paths"] == 256 * 256 and d["roofline"]["avg_launch_ms"] > 0
    assert d["frame_batched"]["value"] > 0 and d["frame_batched"]["steps"] == 8
