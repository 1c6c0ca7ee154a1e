"""The pair kernel at seven waves per SIMD (render_pair7_kernel): render_pair_kernel<6>'s body under a 72-VGPR budget,
on launches that reserve no traversal stack.  Waves per SIMD change where values live, not the operations on them, so everything a launch
leaves -- the accumulation buffer, the 8-bit image, the ray count -- must be what the six-waves kernel leaves (RTGO_MAX_WPE=6: the code
path of every launch before this kernel existed), bit for bit, and rtgo_stats.last_variant bit 9 says which one ran.

A launch takes seven waves by its own work only from kUnitsPerWave4For7 = 26 units per wave on (rtgo_capi.hip; a 1080p frame has 35), more
than a test should render: the cases force it with RTGO_MAX_WPE=7, and the 512 x 288 case (8 units per wave) checks that its own work
keeps it on render_pair_kernel<6>.
Jobs pin the first fast-walk structure (RTGO_TREE=0), as tests/test_pair_walk.py sets them up: its render() runs them.  Needs a real MI355X."""
import re

import numpy as np
import pytest

from test_pair_walk import BIT as PAIR_BIT, inside_camera, render, tables

pytestmark = pytest.mark.gpu

BIT7 = 512


def six_and_seven(t, W, H, N, frames, **kw):
    """the same job at RTGO_MAX_WPE=6 and =7: the same bits, image and rays; bit 9 clear in every launch of the first and set in every
    launch of the second that is not the launch-time trial's.  Returns the second job's variants."""
    a6, i6, r6, v6 = render(t, W, H, N, frames, False, wpe=6, **kw)
    a7, i7, r7, v7 = render(t, W, H, N, frames, False, wpe=7, **kw)
    assert all(v & BIT7 == 0 for v in v6), v6
    assert all(v & PAIR_BIT for v in v6), v6
    assert all(v & BIT7 and v & PAIR_BIT for v in v7 if not v & 8), v7
    assert any(not v & 8 for v in v7), v7
    assert r6 == r7 > 0, (r6, r7)
    assert a6.tobytes() == a7.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a6 != a7, axis=-1)))
    assert i6.tobytes() == i7.tobytes()
    return v7


# ---- 96 x 64, three progressive frames

@pytest.mark.parametrize("N,max_depth", [(4, 5), (2, 1)])
def test_small_frames(N, max_depth):
    # spp 16 at depth 5; spp 4 at depth 1, where the last-ray path is the first bounce
    W, H = 96, 64
    six_and_seven(tables("cornell", W, H), W, H, N, 3, max_depth=max_depth)


def test_band_share():
    W, H = 96, 64
    six_and_seven(tables("cornell", W, H), W, H, 4, 3, bands=(4, 8, 5))


def test_eye_inside_the_room():
    W, H = 96, 64
    t = tables("cornell", W, H)
    six_and_seven(t, W, H, 4, 3, cam=inside_camera(t))


# ---- 512 x 288, 16 spp, two frames, the eye inside the room: 8 units per wave

def test_small_job_keeps_six_waves_and_seven_hands_its_seeds_over(capfd):
    W, H = 512, 288
    t = tables("cornell", W, H)
    cam = inside_camera(t)   # (the launch of tests/test_pair_walk.py: from outside, the room covers too little of the window for 8 units per wave)
    capfd.readouterr()
    a0, i0, r0, v0 = render(t, W, H, 4, 2, False, wpe=None, cam=cam, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 2, err[-2000:]
    for l in lines:
        assert re.search(r"kernel render_pair_kernel<6>$", l), l
    assert all(v & PAIR_BIT and not v & BIT7 for v in v0), v0
    # the second frame reads the seeds the first one's seed pass left (seeds / seeds_next): at 7 against 6
    capfd.readouterr()
    a7, i7, r7, v7 = render(t, W, H, 4, 2, False, wpe=7, cam=cam, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 2, err[-2000:]
    for l in lines:
        assert re.search(r"7 waves/SIMD variant, 7 workgroups/CU.*kernel render_pair7_kernel$", l), l
    assert all(v & PAIR_BIT and v & BIT7 for v in v7), v7
    a6, i6, r6, v6 = render(t, W, H, 4, 2, False, wpe=6, cam=cam)
    assert all(v & PAIR_BIT and not v & BIT7 for v in v6), v6
    assert r0 == r6 == r7 > 0
    assert a0.tobytes() == a6.tobytes() == a7.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a6 != a7, axis=-1)))
    assert i0.tobytes() == i6.tobytes() == i7.tobytes()


# ---- the knob without the pair kernel: today's six-waves flat kernel

def test_no_pair_at_seven_takes_the_six_waves_flat_kernel(capfd):
    W, H = 96, 64
    t = tables("cornell", W, H)
    capfd.readouterr()
    a_off, i_off, r_off, v_off = render(t, W, H, 4, 1, True, wpe=7, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 1 and re.search(r"kernel render_kernel<6>$", lines[0]), err[-2000:]
    assert v_off[0] & (PAIR_BIT | BIT7) == 0, v_off
    a7, i7, r7, v7 = render(t, W, H, 4, 1, False, wpe=7)
    assert v7[0] & BIT7 and v7[0] & PAIR_BIT, v7
    assert r_off == r7 > 0
    assert a_off.tobytes() == a7.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a_off != a7, axis=-1)))
    assert i_off.tobytes() == i7.tobytes()
