"""bench.py --dump-outputs: what the timed path handed back in its last step, as .npy files a second build can be compared with."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_whole_frames_that_fit(tmp_path):
    bench = _bench_module()
    rng = np.random.default_rng(1)
    acc = rng.random((180, 320, 4), dtype=np.float32)
    img = rng.integers(0, 256, (180, 320, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"accum": acc, "image": img})
    assert sorted(os.listdir(tmp_path)) == ["accum.npy", "image.npy"]
    a, i = np.load(tmp_path / "accum.npy"), np.load(tmp_path / "image.npy")
    assert a.dtype == np.float32 and i.dtype == np.float32
    assert np.array_equal(a, acc) and np.array_equal(i, img.astype(np.float32))


def test_dump_samples_the_same_pixels_of_a_frame_over_the_budget(tmp_path):
    """1920x1080 RGBA float accumulation + 8-bit image do not fit the budget as float32: a fixed, seeded pixel sample, the same
    from run to run and for every array, with its pixel indices"""
    bench = _bench_module()
    rng = np.random.default_rng(2)
    acc = rng.random((1080, 1920, 4), dtype=np.float32)
    img = rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8)
    d1, d2 = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(d1), {"accum": acc, "image": img})
    bench.dump_outputs(str(d2), {"accum": acc, "image": img})
    assert _dir_bytes(d1) <= bench.DUMP_BUDGET_BYTES
    idx = np.load(d1 / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(d2 / "pixel_index.npy"))
    idx = idx.astype(np.int64)
    assert len(idx) > 0.7 * 1080 * 1920 and (np.diff(idx) > 0).all()
    assert np.array_equal(np.load(d1 / "accum.npy"), acc.reshape(-1, 4)[idx])
    assert np.array_equal(np.load(d1 / "image.npy"), img.reshape(-1, 4)[idx].astype(np.float32))


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_frame(tmp_path):
    """the dumped arrays are the frame a direct whole-frame render of frames 0 .. warmup+steps-1 ends with, bit for bit, whether the
    frame was rendered as one launch or as two sub-shares stacked in one buffer"""
    from raytracingo_amd import capi, scene
    W, H, N, warmup, steps = 320, 180, 2, 2, 3
    capi.load()
    t = scene.tables("cornell", W, H)
    ctx = capi.Context(0)
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)
    for f in range(warmup + steps):
        ctx.launch(capi.make_frame(W, H, N, f, True, False, None, (4, 1, 0)))
    ctx.sync()
    want_acc, want_img = ctx.read_accum(H, W), ctx.read_image(H, W)
    ctx.close()
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--width", str(W),
            "--height", str(H), "--sample", str(N), "--spin-up", "4", "--no-cpu-baseline"]
    for extra in ([], ["--launches-per-frame", "2"]):
        d = tmp_path / ("s%d" % len(extra))
        r = subprocess.run(base + extra + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["steps"] == steps and j["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["accum.npy", "image.npy"]
        acc, img = np.load(d / "accum.npy"), np.load(d / "image.npy")
        assert acc.shape == (H, W, 4) and img.shape == (H, W, 4)
        assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32)), extra
        assert np.array_equal(img, want_img.astype(np.float32)), extra
