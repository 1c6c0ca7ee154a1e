"""render_unit16_kernel: render_slab7_kernel's body with what a launch of 16 samples per pixel in workgroups of 256 threads fixes compiled
in (UNIT16, rtgo_render_body.inc).  A unit is 4 pixels x 16 samples, so a pixel's samples are the 16 lanes of one DPP row
and the in-order sample sum is 16 row-broadcast additions per channel; the lane's pixel and sample are a shift and a mask; a level
record's three words sit at fixed offsets.  Every float operation that reaches a pixel is the same operation on the same values in the
same order, so everything a launch leaves -- every pixel of the accumulation buffer, the 8-bit image, the ray count -- must be what the
same launch leaves with RTGO_NO_UNIT16=1 (render_slab7_kernel) and what the canonical walk leaves (a collect_stats launch), byte for
byte; rtgo_stats.last_variant bit 11 says the new kernel ran.

RTGO_MAX_WPE=7 pins the seven-waves kernels on these small frames, RTGO_TREE=0 the first fast-walk structure.  Needs a real MI355X."""
import numpy as np
import pytest

from test_pair_walk import FULL, Env, seeded_scene, tables

pytestmark = pytest.mark.gpu

PAIR, PAIR7, SLAB, UNIT16, CANON = 256, 512, 1024, 2048, 4
W, H = 66, 8          # 16 units of 4 pixels and one of 2 in every row


def render(t, W, H, N, frames, cam=None, bg=None, max_depth=5, bands=FULL, window=None, stats=False, env=None):
    """accum and image of the launch's rows after `frames` progressive frames, rays_total, last_variant of every launch"""
    from raytracingo_amd import capi
    kv = {"RTGO_MAX_WPE": "7", "RTGO_TREE": "0", "RTGO_NO_UNIT16": None, "RTGO_NO_SLAB": None, "RTGO_NO_PAIR": None}
    kv.update(env or {})
    with Env(**kv):
        ctx = capi.Context(0)
        try:
            ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
            c = t["cam"] if cam is None else cam
            ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
            ctx.set_background(t["bg"] if bg is None else bg)
            ctx.set_lights(t["lights"])
            x0, y0, w, h = window if window else (0, 0, W, H)
            rows = capi.local_rows(h, *bands)
            ctx.resize(rows * w)
            variants = []
            for f in range(frames):
                ctx.launch(capi.make_frame(W, H, N, f, True, max_depth=max_depth, bands=bands, window=window, stats=stats))
                ctx.sync()
                variants.append(ctx.stats()["last_variant"])
            return ctx.read_accum(rows, w).copy(), ctx.read_image(rows, w).copy(), ctx.stats()["rays_total"], variants
        finally:
            ctx.close()


def three_kernels(t, W, H, N, frames, unit16=True, **kw):
    """the job as shipped, with RTGO_NO_UNIT16=1 and on the canonical walk: the same bytes in the accumulation buffer and in the image,
    the same rays.  unit16: whether the first is expected to take render_unit16_kernel; the slab kernel is expected either way.
    Returns the first job's accumulation buffer."""
    a_u, i_u, r_u, v_u = render(t, W, H, N, frames, **kw)
    a_s, i_s, r_s, v_s = render(t, W, H, N, frames, env={"RTGO_NO_UNIT16": "1"}, **kw)
    a_c, i_c, r_c, v_c = render(t, W, H, N, frames, stats=True, **kw)
    assert all(bool(v & UNIT16) == unit16 for v in v_u), v_u
    assert all(v & SLAB and v & PAIR7 and v & PAIR for v in v_u), v_u
    assert all(not v & UNIT16 and v & SLAB for v in v_s), v_s
    assert all(v & CANON and not v & (PAIR | SLAB | UNIT16) for v in v_c), v_c
    assert r_u == r_s == r_c, (r_u, r_s, r_c)
    for name, a, i in (("render_slab7_kernel", a_s, i_s), ("the canonical walk", a_c, i_c)):
        assert a_u.tobytes() == a.tobytes(), "render_unit16_kernel != %s: %d pixels" % (name, int(np.sum(np.any(a_u != a, axis=-1))))
        assert i_u.tobytes() == i.tobytes(), name
    return a_u


@pytest.mark.parametrize("max_depth", [0, 1, 5])
def test_cornell_frames_0_to_2(max_depth):
    # the last unit of a row holds 2 pixels: its lanes 32..63 are out of range and must add nothing to a row of the lanes 0..31
    three_kernels(tables("cornell", W, H), W, H, 4, 3, max_depth=max_depth)


BG = np.array([0.3, 0.5, 0.7], dtype=np.float32)


def wide_camera(t):
    """cornell's camera with the image plane 2.5 times as wide and as high: the room's outline crosses the frame, and the pixels on it
    have samples that miss beside samples that hit"""
    cam = t["cam"].copy()
    cam[3:9] *= np.float32(2.5)
    return cam


def pixels_partly_missed(acc, bg):
    """pixels of a frame-0, max_depth-0 render whose 16 payloads are k background colours, 0 < k < 16, and zeros (walls at the depth limit):
    the three channels are in the background's ratio and below its full sum"""
    full = np.zeros(3, np.float32)
    for _ in range(16):
        full = full + bg
    full = full * np.float32(0.0625)
    rgb = acc[..., 0:3].astype(np.float64)
    k = rgb / full.astype(np.float64)
    same = (np.abs(k[..., 1] - k[..., 0]) < 1e-5) & (np.abs(k[..., 2] - k[..., 0]) < 1e-5)
    return same & (k[..., 0] > 0.03) & (k[..., 0] < 0.97)


@pytest.mark.parametrize("max_depth", [0, 1, 5])
def test_background_not_black_and_samples_that_partly_miss(max_depth):
    # a missed sample's payload is the background colour: with hits among a pixel's 16 the order of the additions decides the bits
    t = tables("cornell", W, H)
    cam = wide_camera(t)
    if max_depth == 0:
        a0, *_ = render(t, W, H, 4, 1, cam=cam, bg=BG, max_depth=0)
        partly = pixels_partly_missed(a0, BG)
        units = {(y, x // 4) for y, x in zip(*np.nonzero(partly))}
        print("pixels with samples that partly miss: %d, in %d units" % (int(partly.sum()), len(units)))
        assert partly.sum() >= 4 and len(units) >= 2, "the camera shows no pixel on the room's outline"
    three_kernels(t, W, H, 4, 3, cam=cam, bg=BG, max_depth=max_depth)


def test_window_whose_x0_is_no_multiple_of_4():
    three_kernels(tables("cornell", 96, 16), 96, 16, 4, 3, window=(5, 3, 50, 9))
    three_kernels(tables("cornell", 96, 16), 96, 16, 4, 2, window=(5, 3, 50, 9), cam=wide_camera(tables("cornell", 96, 16)), bg=BG)


def test_one_of_three_band_shares():
    three_kernels(tables("cornell", W, 24), W, 24, 4, 3, bands=(4, 3, 1))


@pytest.mark.parametrize("sample", [2, 3])
def test_other_sample_counts_keep_the_slab_kernel(sample):
    # selection is unchanged: bit 11 clear, bit 10 set
    three_kernels(tables("cornell", W, H), W, H, sample, 3, unit16=False)


def test_a_two_box_room():
    t, cam = seeded_scene(1, W, H)       # both boxes in the air at random rotations and scales (tests/test_pair_walk.py)
    three_kernels(t, W, H, 4, 3, cam=cam)
    three_kernels(t, W, H, 4, 2, cam=cam, bg=BG, max_depth=1)


def test_debug_line_names_the_kernel(capfd):
    t = tables("cornell", W, H)
    capfd.readouterr()
    *_, v = render(t, W, H, 4, 1, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 1 and " kernel render_unit16_kernel," in lines[0] and "kernel render_slab7_kernel," in lines[0], err[-2000:]
    assert " x 256 threads" in lines[0], lines[0]
    assert all(x & UNIT16 for x in v), v
