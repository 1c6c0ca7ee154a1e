"""The pair kernels fold a path's level records once, after the ray loop (FOLDLATE, rtgo_render_body.inc): in the loop a
path that ends keeps one word that says what its payload is -- the background, the emitter it hit, or zero at the depth limit -- and after
the loop every lane of the wave looks its payload up and runs `term = a_k * term` over its own records, innermost first.  The same
multiplications in the same order as the fold inside the loop, which the generic kernels keep, so everything a launch leaves -- the
accumulation buffer, the image, the ray count -- must be what RTGO_NO_PAIR=1 leaves, bit for bit.

The cases are the places where a deferred fold can go wrong: paths that end at every depth within one wave, records and the word carried
from pass to pass and from frame to frame, lanes of a unit that never start, primaries that end at depth 0 on the emitter or on the
background, a background that is not black.  Jobs are set up as tests/test_pair_walk.py sets them up (its render() and on_off() run them:
RTGO_TREE=0, RTGO_MAX_WPE to reach the kernel under test on a 96 x 64 frame).  Needs a real MI355X."""
import numpy as np
import pytest

from test_pair_walk import BIT as PAIR_BIT, on_off, render, tables

pytestmark = pytest.mark.gpu

BIT7 = 512
CERT = 64          # last_variant bit 6: the launch has the last-ray certificate
W, H = 96, 64


def check_variants(v, wpe):
    assert all(x & PAIR_BIT for x in v), v
    assert all(bool(x & BIT7) == (wpe == 7) for x in v), v


@pytest.mark.parametrize("wpe", [5, 6, 7])
@pytest.mark.parametrize("max_depth", [1, 2, 3, 4, 5])
def test_every_depth_at_every_wave_count(max_depth, wpe):
    _, v = on_off(tables("cornell", W, H), W, H, 4, 3, wpe=wpe, max_depth=max_depth)
    check_variants(v, wpe)


@pytest.mark.parametrize("sample,wpe", [(1, 7), (2, 5), (4, 6), (8, 7)])
def test_passes_and_pixels_per_unit(sample, wpe):
    # sample 8: four passes of a unit, each with fresh records and a fresh word; sample 1: 64 pixels per unit
    _, v = on_off(tables("cornell", W, H), W, H, sample, 2, wpe=wpe, env={"RTGO_STREAM": "0"})
    check_variants(v, wpe)


@pytest.mark.parametrize("width,wpe", [(95, 7), (97, 6)])
def test_lanes_that_never_start(width, wpe):
    # the row's last unit has pixels past the window: their lanes fold nothing and their payload stays zero
    _, v = on_off(tables("cornell", width, H), width, H, 4, 2, wpe=wpe)
    check_variants(v, wpe)


def emitter_camera(t):
    """the eye inside the room, looking at the centre of the emitter: U, V, W keep their lengths"""
    cam = t["cam"].copy()
    e = int(np.argmax(t["mat"][:, 7]))
    assert t["mat"][e, 7] > 0.01
    target = 0.5 * (t["aabb"][e, 0:3] + t["aabb"][e, 3:6]).astype(np.float64)
    eye = np.array([0.3, 0.5, 3.5])
    ulen, vlen, wlen = [float(np.linalg.norm(cam[3 + 3 * a:6 + 3 * a])) for a in range(3)]
    w = (target - eye) / np.linalg.norm(target - eye)
    u = np.cross(w, [0.0, 0.0, -1.0])
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    cam[0:3], cam[3:6], cam[6:9], cam[9:12] = eye, u * ulen, v * vlen, w * wlen
    return cam


@pytest.mark.parametrize("wpe", [6, 7])
def test_primaries_that_end_on_the_emitter(wpe):
    t = tables("cornell", W, H)
    a, v = on_off(t, W, H, 4, 2, wpe=wpe, cam=emitter_camera(t))
    check_variants(v, wpe)
    # the window's centre sees the emitter itself: Le, whatever the frame
    e = int(np.argmax(t["mat"][:, 7]))
    assert np.allclose(a[H // 2, W // 2, 0:3], t["mat"][e, 7:10], rtol=1e-6), a[H // 2, W // 2]


def test_stock_camera_primaries_that_miss():
    # the stock camera stands outside the room: hot strips hold primaries that pass it by and take the background at depth 0
    t = tables("cornell", W, H)
    a, v = on_off(t, W, H, 4, 2, wpe=7)
    check_variants(v, 7)
    assert all(x & CERT for x in v), v
    assert np.any(np.all(a[:, :, 0:3] == t["bg"], axis=-1)) and np.any(a[:, :, 0:3] != t["bg"])


@pytest.mark.parametrize("wpe", [5, 7])
def test_background_that_is_not_black(wpe):
    # ... and no last-ray certificate: every ray of the launch takes the full walk
    t = {k: x.copy() for k, x in tables("cornell", W, H).items()}
    t["bg"] = np.array([0.25, 0.5, 0.125], dtype=np.float32)
    a, v = on_off(t, W, H, 4, 3, wpe=wpe)
    check_variants(v, wpe)
    assert not any(x & CERT for x in v), v
    assert np.any(np.all(a[:, :, 0:3] == t["bg"], axis=-1))


def test_band_share():
    _, v = on_off(tables("cornell", W, H), W, H, 4, 3, wpe=5, bands=(4, 8, 5))
    check_variants(v, 5)


def test_against_the_canonical_launch():
    t = tables("cornell", W, H)
    a_on, v_on = on_off(t, W, H, 4, 1, wpe=7, max_depth=3)
    check_variants(v_on, 7)
    a_canon, _, _, v = render(t, W, H, 4, 1, False, wpe=7, max_depth=3, stats=True)
    assert v[0] & 4 and not v[0] & PAIR_BIT, v
    assert a_on.tobytes() == a_canon.tobytes(), "deferred fold != canonical launch: %d pixels" % int(np.sum(np.any(a_on != a_canon, axis=-1)))
