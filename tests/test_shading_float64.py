"""The device's analytic shading through the C ABI, held to tests/analytic_shading_ref64.py -- the float64 statement of the rules -- with the
constants tests/test_oracle_shading_float64.py measured for the oracle: never to the oracle itself, and with no bounds of its own.  Whole
frames of the scenes built for this in the three modes, the direct term alone, detector scenes in which every pixel names the patch its
bounce ray met -- in path mode with the cosine it left under, in distributed mode about N and about Rr at three exponents -- also through the
launch paths that share the lobe sampler differently (the instrumented kernel, the batched frames, the large-scene walk), and the
degenerate frame.  Needs a real MI355X."""
import numpy as np
import pytest

import analytic_shading_ref64 as S
import shading_scenes as SC
import test_oracle_shading_float64 as T

pytestmark = pytest.mark.gpu
UNIT = S.UNIT
W, H = T.W48, T.H36


def device_frames(t, width, height, n, md, mode, frames, stats=False, large=False, batched=False, each=False, only=None):
    """the accumulation buffer, the bytes and rtgo_get_stats after progressive frames 0 .. frames - 1 of a fresh context.  each: the list of
    those three after every frame; only = f: frame_count f alone, on a zeroed buffer"""
    from raytracingo_amd import capi
    path, amb = T.MODES[mode]
    ctx = capi.Context(0)
    try:
        (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"])
        c = t["cam"]
        ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
        ctx.set_background(t["bg"])
        ctx.set_lights(t["lights"])
        ctx.resize(width * height)
        if only is not None:
            ctx.write_accum(np.zeros((height, width, 4), np.float32))
            ctx.launch(capi.make_frame(width, height, n, only, path, amb, bands=(1, 1, 0), max_depth=md, stats=stats))
            ctx.sync()
        elif each:
            out = []
            for f in range(frames):
                ctx.launch(capi.make_frame(width, height, n, f, path, amb, bands=(1, 1, 0), max_depth=md, stats=stats))
                ctx.sync()
                out.append((ctx.read_accum(height, width).copy(), ctx.read_image(height, width).copy(), ctx.stats()))
            return out
        elif batched:
            ctx.launch_frames(capi.make_frame(width, height, n, 0, path, amb, bands=(1, 1, 0), max_depth=md, stats=stats), frames)
            ctx.sync()
        else:
            for f in range(frames):
                ctx.launch(capi.make_frame(width, height, n, f, path, amb, bands=(1, 1, 0), max_depth=md, stats=stats))
                ctx.sync()
        return ctx.read_accum(height, width).copy(), ctx.read_image(height, width).copy(), ctx.stats()
    finally:
        ctx.close()


CASES = [(name, mode, md, n) for name in SC.SCENES for mode in T.MODES for md in T.DEPTHS[name] for n in (1, 2)]


@pytest.mark.parametrize("name,mode,md,n", CASES, ids=lambda v: str(v))
def test_whole_frames(name, mode, md, n):
    """frames 0 .. 2 accumulated: the checks, caps and floors of the CPU test, and rtgo_get_stats' ray counts within the reference's clear and
    unclear counts.  One sample per pixel: the third buffer against the reference's three steps, on the pixels clear in all three.  Four
    samples: every frame on its own clear pixels, through the recurrence from the buffer the device held before it, so that no pixel has
    to be clear in all twelve of its paths"""
    if n == 1:
        ref = T.reference(name, mode, md, n, frames=3)
        acc, img, st = device_frames(ref[0], W, H, n, md, mode, 3)
        T.check_frame(name, mode, md, n, ref, acc, img, rays_occlusion=st["rays_occlusion"], rays_total=st["rays_total"])
        return
    t = SC.SCENES[name](W / H)
    prev, before = None, {"rays_occlusion": 0, "rays_total": 0}
    for fc, (acc, img, st) in enumerate(device_frames(t, W, H, n, md, mode, 3, each=True)):
        ref = T.reference_frame(name, mode, md, n, fc, prev)
        T.check_frame(name, mode, md, n, ref, acc, img, rays_occlusion=st["rays_occlusion"] - before["rays_occlusion"],
                      rays_total=st["rays_total"] - before["rays_total"])
        prev, before = acc, st


@pytest.mark.parametrize("mode", ["distributed", "ambient"])
def test_direct_light_alone(mode):
    """two_lights at max_depth 0: every clear pixel is the reference's direct term -- |Lm . n_light| min(Le, 1) max(N . Lm, 0) kd / (1 + falloff
    lightDistance) of a light the index rule can draw -- and nothing else: no 0.1 kd under ambient light at depth == max_depth.  A shadowed
    pixel carries its blocker's min(Le, 1), which differs per channel and per blocker, so lit and shadowed cannot be confused within the bound."""
    t = SC.two_lights(W / H)
    r = S.render(t, T.frame_of(W, H, 1, 0, 0, mode))
    acc, img, st = device_frames(t, W, H, 1, 0, mode, 1)
    clear = r["clear"]
    hit = (r["hits"] > 0).any(-1)
    assert (~clear & hit).sum() <= T.UNCLEAR_CAP["two_lights"] * hit.sum()
    assert (clear & r["shadowed"]).mean() >= 0.10 and (clear & r["lit"]).mean() >= 0.30
    c64, c32 = r["accum"], acc[..., :3].astype(np.float64)
    dev = (np.abs(c32 - c64) / (r["kappa"][..., None] * np.maximum(np.abs(c64), 1e-3))).max(-1) / UNIT
    print("direct light alone,", mode, "largest dev %.2f units" % dev[clear].max())
    assert dev[clear].max() <= T.DEV_BOUND[("two_lights", mode)]
    assert (acc[clear & ~hit][:, :3] == t["bg"]).all() and (acc[..., 3] == 1.0).all()
    assert st["rays_total"] - st["rays_occlusion"] == W * H          # max_depth 0: the primaries are the only radiance rays
    lo = int(r["rays_occlusion"][0])
    assert lo <= st["rays_occlusion"] <= lo + int((~r["clear_paths"]).sum())


# ------------------------------------------------------------------------------------------------ the detector
@pytest.mark.parametrize("fc", T.DETECTOR_FRAMES)
@pytest.mark.parametrize("pose,spec", T.DETECTOR_CASES, ids=lambda v: str(v))
def test_detector(pose, spec, fc):
    """frame_count fc alone on a zeroed buffer, max_depth 1, one sample: path mode in three poses (kd (N . Ra) Le_patch: the patch and the
    cosine), distributed mode with a target of specularity 0, 1, 30 and 300 under an oblique camera (the patch the lobe's ray met: about N
    at 0, about Rr else, the exponents 30 and 300 through glossy_theta).  T.check_detector holds the oracle to the same"""
    t, weight, _ = T.detector_reference(pose, spec, fc)
    acc, _, _ = device_frames(t, W, H, 1, 1, T.detector_mode(spec), 1, only=fc)
    T.check_detector(pose, spec, fc, acc)


@pytest.mark.parametrize("variant", ["collect_stats", "launch_frames", "large_scene"])
@pytest.mark.parametrize("spec", [None, 30], ids=["path", "distributed-30"])
def test_detector_through_other_kernels(spec, variant):
    """the same through the kernels that share the lobe sampler differently: the canonical instrumented kernel, the large-scene walk, and
    the batched frames, whose final running average over 4 frames is held to the reference's four steps on the pixels clear in all four
    (each frame's own share of unclear pixels is capped in test_detector)"""
    pose, mode = "rotated", T.detector_mode(spec)
    t, weight, _ = T.detector_reference(pose, spec, 0)
    if variant == "launch_frames":
        acc, _, _ = device_frames(t, W, H, 1, 1, mode, 4, batched=True)
        c64, kappa, ok = T.detector_average(pose, spec, 4)
        dev = (np.abs(acc[..., :3].astype(np.float64) - c64) / (kappa[..., None] * np.maximum(np.abs(c64), 1e-3))).max(-1) / UNIT
        print("detector", mode, "4 batched frames: largest dev %.2f units" % dev[ok].max())
        assert ok.mean() >= 0.90 and dev[ok].max() <= T.DEV_BOUND[("detector", mode)]
    else:
        acc, _, _ = device_frames(t, W, H, 1, 1, mode, 1, stats=variant == "collect_stats", large=variant == "large_scene", only=0)
        T.check_detector(pose, spec, 0, acc)


# ------------------------------------------------------------------------------------------------ the degenerate frame
def test_degenerate_plane():
    """one rectangle tilted by exactly 45 degrees about x, path mode, 16 x 12: N = (0, a, a), the lobe's frame is 0 / 0 and the bounce ray NaN.
    That the launch ends was read off the code first (rtgo_device.h): the lobe's loop ends because NaN < 0 is false and is bounded by 1024
    draws besides; the tree walks visit every node at most once whatever the comparisons say (a stack over a finite tree; a NaN slab test
    only prunes); the grid walk drops a ray with a NaN component before its first step (`live &= tdx > 2 margin ...`: a comparison with
    NaN is false); the leaf tests accept nothing (closer() compares).  Held to what tests/test_oracle_shading_float64.py pins for the
    oracle: NaN in the accumulation buffer wherever the plane is hit, alpha 1, bytes 255 (clamp's fmaxf(0, fminf(NaN, 1)) = 1), the
    background elsewhere."""
    t = T.tilted_plane()
    acc, img, _ = device_frames(t, 16, 12, 1, 1, "path", 1)
    ref = S.render(t, T.frame_of(16, 12, 1, 1, 0, "path"))
    hit = (ref["hits"] > 0).all(-1)
    assert hit.mean() > 0.5
    assert np.isnan(acc[hit][:, :3]).all() and (acc[..., 3] == 1.0).all()
    assert (img[hit][:, :3] == 255).all() and (img[..., 3] == 255).all()
    assert (acc[~hit][:, :3] == t["bg"]).all()
