"""bench.py's plain run and --dump-outputs: the headline line alone, --steps timed steps, and the last frame of the timed loop
written as float32 -- the same frame whatever the number of frames per step, and the frame the library renders for that view."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
MOVED = ("sub_results", "roofline", "roofline_hbm", "cpu_baseline", "kernel_ms_rank0", "static_camera", "host_path")


def test_dump_frame_writes_the_channels_as_float32(tmp_path):
    rng = np.random.default_rng(3)
    words = rng.integers(0, 1 << 24, (36, 52), dtype=np.uint32)
    bench.dump_frame(str(tmp_path), words.view(np.int32))
    rgb = np.load(tmp_path / "frame_rgb.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (36, 52, 3)
    back = (rgb[..., 0].astype(np.uint32) << 16) | (rgb[..., 1].astype(np.uint32) << 8) | rgb[..., 2].astype(np.uint32)
    assert np.array_equal(back, words)
    assert not (tmp_path / "frame_pixel_index.npy").exists()


def test_dump_frame_samples_a_frame_over_the_limit(tmp_path):
    H, W = 2400, 2400                                   # 5.76 M pixels: 69 MB of R, G, B floats
    words = (np.arange(H * W, dtype=np.uint32) % (1 << 24)).reshape(H, W)
    bench.dump_frame(str(tmp_path), words)
    rgb = np.load(tmp_path / "frame_rgb.npy")
    idx = np.load(tmp_path / "frame_pixel_index.npy")
    assert rgb.dtype == np.float32 and idx.dtype == np.float64
    assert rgb.shape == (bench.DUMP_SAMPLE_PIXELS, 3) and idx.shape == (bench.DUMP_SAMPLE_PIXELS,)
    assert rgb.nbytes + idx.nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.all(np.diff(idx) > 0)
    flat = words.reshape(-1)[idx.astype(np.int64)]
    assert np.array_equal(rgb[:, 2].astype(np.uint32), flat & 0xFF)
    bench.dump_frame(str(tmp_path / "again"), words)    # the sample is seeded: the same pixels every time
    assert np.array_equal(np.load(tmp_path / "again" / "frame_pixel_index.npy"), idx)


def run_bench(args, timeout=600):
    env = dict(os.environ, MIRT_BENCH_TARGET_S="0.1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_frame_of_the_timed_loop(tmp_path):
    """Two plain runs of the default workload with different step counts (so different frames per step): each line holds the
    headline only and its own --steps, and both dump the same last frame -- the one a single render of the loop's last view gives."""
    lines = []
    for steps, sub in ((3, "a"), (7, "b")):
        line = run_bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / sub)])
        assert all(k in line for k in HEADLINE), line
        assert not any(k in line for k in MOVED), sorted(line)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
        lines.append(line)
    a, b = (np.load(tmp_path / s / "frame_rgb.npy") for s in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (1080, 1920, 3)
    assert np.array_equal(a, b)

    import mirt
    kind, scene, W, H, cam, focal, rot11 = bench.WORKLOADS[bench.DEFAULT_WORKLOAD]
    mirt.init(0)
    try:
        tris = mirt.scene_soup(scene[1], scene[2], scene[3])
        mirt.scene_upload(tris)
        view = mirt.make_view(cam, mirt.rot_from_yaw((bench.ORBIT_VIEWS - 1) * bench.ORBIT_STEP, rot11), focal, W, H)
        words = mirt.raytrace(view, bench.LIGHT, bench.INDIRECT, want_rgb=False, want_index=False)["xrgb"]
    finally:
        mirt.shutdown()
    want = np.stack([(words >> 16) & 0xFF, (words >> 8) & 0xFF, words & 0xFF], axis=-1).astype(np.float32)
    assert np.array_equal(a[1:-1, 1:-1], want[1:-1, 1:-1])            # (the ray tracer leaves the border words as they were)
    assert np.count_nonzero(a) > 0
