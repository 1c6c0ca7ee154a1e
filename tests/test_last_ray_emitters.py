"""The last-ray certificate: in path mode, a path's last ray (depth == max_depth) can only add an emitter's Le, so when
the up-front list is a room followed by the scene's emitters, every emitter lies inside every wall by a margin and the background is +0,
that ray skips the room and only the lanes that hit an emitter walk the tree.  The accumulation buffers must be bit for bit those of the
usual walk (RTGO_NO_LAST_EMITTER), and the launches that must not take it -- an emitter on or beyond a wall plane, a nonzero or negative
zero background, scenes without a room -- must not (rtgo_stats.last_variant bit 6).  Needs a real MI355X."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOB = "RTGO_NO_LAST_EMITTER"
BIT = 64


def render(t, W, H, N, frames, off, max_depth=5, bands=(4, 1, 0), cam=None, bg=None):
    """accum of the launch's rows after `frames` progressive frames, rays_total, and last_variant of every launch"""
    from raytracingo_amd import capi
    old = os.environ.get(KNOB)
    if off:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)
    try:
        ctx = capi.Context(0)
        try:
            ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
            c = t["cam"] if cam is None else cam
            ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
            ctx.set_background(t["bg"] if bg is None else bg)
            ctx.set_lights(t["lights"])
            rows = capi.local_rows(H, bands[0], bands[1], bands[2])
            ctx.resize(rows * W)
            variants = []
            for f in range(frames):
                ctx.launch(capi.make_frame(W, H, N, f, True, max_depth=max_depth, bands=bands))
                ctx.sync()
                variants.append(ctx.stats()["last_variant"])
            return ctx.read_accum(rows, W).copy(), ctx.stats()["rays_total"], variants
        finally:
            ctx.close()
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def on_off(t, W, H, N, frames, **kw):
    """renders with the certificate allowed and with it off; asserts the same bits and rays; returns whether a launch of the first took it
    (the first launches of a job try both fast-walk structures, and each has a certificate of its own: the list differs between them)"""
    a_on, r_on, v_on = render(t, W, H, N, frames, False, **kw)
    a_off, r_off, v_off = render(t, W, H, N, frames, True, **kw)
    assert all(v & BIT == 0 for v in v_off), v_off
    assert r_on == r_off
    assert a_on.tobytes() == a_off.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a_on != a_off, axis=-1)))
    return any(v & BIT for v in v_on)


def tables(name, W, H):
    from raytracingo_amd import scene
    return scene.tables(name, W, H)


def emitter_rows(t):
    return np.nonzero(t["mat"][:, 7] > 0.01)[0]


@pytest.mark.parametrize("W,H,N,frames", [(320, 180, 4, 2), (640, 360, 2, 3), (257, 131, 5, 1), (1920, 1080, 4, 1)])
def test_cornell_same_bits_with_and_without(W, H, N, frames):
    assert on_off(tables("cornell", W, H), W, H, N, frames)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 3, 4, 5])
def test_cornell_every_max_depth(max_depth):
    W, H = 320, 180
    took = on_off(tables("cornell", W, H), W, H, 4, 2, max_depth=max_depth)
    assert took == (max_depth >= 1)   # (max_depth 0: the last ray is the primary ray; the launch does not take the certificate)


def test_cornell_random_cameras_and_band_shares():
    W, H = 384, 216
    t = tables("cornell", W, H)
    rng = np.random.default_rng(20261016)
    for k in range(6):
        cam = t["cam"].copy()
        cam[0:3] = rng.uniform([-3.5, -3.5, -3.5], [3.5, 3.5, 16.0]).astype(np.float32)   # inside the room and in front of it
        G = int(rng.choice([1, 2, 4, 8]))
        g = int(rng.integers(0, G))
        assert on_off(t, W, H, 4, 2, cam=cam, bands=(4, G, g))


def moved_light(t, y):
    """the cornell light at height y (the ceiling is at 4): its matrix and box move together"""
    t = {k: v.copy() for k, v in t.items()}
    e = emitter_rows(t)
    assert len(e) == 1
    dy = y - t["M"][e[0], 7]
    t["M"][e[0], 7] = y
    t["aabb"][e[0], 1] += dy
    t["aabb"][e[0], 4] += dy
    return t


@pytest.mark.parametrize("y,takes", [(3.95, True), (3.9999, False), (4.0, False), (4.5, False)])
def test_cornell_light_near_and_beyond_the_ceiling(y, takes):
    W, H = 320, 180
    assert on_off(moved_light(tables("cornell", W, H), y), W, H, 4, 2) == takes


@pytest.mark.parametrize("bg", [(0.25, 0.0, 0.0), (0.0, 0.0, 1e-30), (-0.0, 0.0, 0.0)])
def test_background_must_be_positive_zero(bg):
    W, H = 320, 180
    assert not on_off(tables("cornell", W, H), W, H, 4, 2, bg=np.array(bg, dtype=np.float32))


@pytest.mark.parametrize("name", ["checkered", "plateau", "balls", "slide", "window", "mirror_spheres", "soft_mirrors"])
def test_other_scenes_same_bits(name):
    W, H = 320, 180
    took = on_off(tables(name, W, H), W, H, 4, 3)
    if name in ("checkered", "plateau"):   # no room: the certificate has to refuse
        assert not took
