"""The waves-per-SIMD variants of the render kernel (4, 5 and, for path mode over flat scenes, 6) differ only in where values live,
not in the operations on them: the same frames must come out bit for bit, with the same ray counts.  RTGO_MAX_WPE caps the variant
per launch (read when the launch is planned), so one build compares them.  Needs a real MI355X."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def render(name, W, H, N, frames, max_wpe):
    from raytracingo_amd import capi, scene
    old = os.environ.get("RTGO_MAX_WPE")
    os.environ["RTGO_MAX_WPE"] = str(max_wpe)
    try:
        t = scene.tables(name, W, H)
        ctx = capi.Context(0)
        ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
        ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
        ctx.set_background(t["bg"])
        ctx.set_lights(t["lights"])
        ctx.resize(W * H)
        out = []
        for f in range(frames):
            ctx.reset_stats()
            ctx.launch(capi.make_frame(W, H, N, f, True))
            ctx.sync()
            out.append((ctx.read_accum(H, W).copy(), ctx.read_image(H, W).copy(), ctx.stats()["rays_total"]))
        return out
    finally:
        if old is None:
            os.environ.pop("RTGO_MAX_WPE", None)
        else:
            os.environ["RTGO_MAX_WPE"] = old


@pytest.mark.parametrize("name", ["cornell", "checkered"])
def test_six_and_five_waves_give_the_same_frames(name):
    W, H, N = 480, 270, 4
    five = render(name, W, H, N, 2, 5)
    six = render(name, W, H, N, 2, 6)
    for f, ((a5, i5, r5), (a6, i6, r6)) in enumerate(zip(five, six)):
        assert r5 == r6 > 0, (name, f, r5, r6)
        assert np.array_equal(a5.view(np.uint32), a6.view(np.uint32)), (name, f, "accumulation buffers differ")
        assert np.array_equal(i5, i6), (name, f, "images differ")
