"""render_roomw_kernel: render_unit16_kernel's body with the room's slab test steered in world axes (ROOMW, room_world in rtgo_device.h;
the certificate: csrc/rtgo_room_world.h).  The steering only picks which wall gets the reference's test, so everything a
launch leaves -- every pixel of the accumulation buffer, the 8-bit image, the ray count -- must be what the same launch leaves with
RTGO_NO_ROOMW=1 (render_unit16_kernel, or whatever kernel the launch gets) and what the canonical walk leaves (a collect_stats launch),
byte for byte, over three progressive frames; rtgo_stats.last_variant bit 12 says the new kernel ran, and must be clear in the other two.

Frames of 160 x 90 and smaller at sample=4; RTGO_MAX_WPE=7 pins the seven-waves kernels on them, RTGO_TREE=0 the first fast-walk
structure (tests/test_unit16_kernel_gpu.py, whose render() this uses).  Needs a real MI355X."""
import numpy as np
import pytest

import adversarial_cameras as AC
from test_pair_walk import tables
from test_unit16_kernel_gpu import BG, render, wide_camera

pytestmark = pytest.mark.gpu

PAIR, PAIR7, SLAB, UNIT16, ROOMW, CANON = 256, 512, 1024, 2048, 4096, 4
W, H = 160, 90
FRAMES = 3
ON, OFF, WITH_UNIT16 = "set", "clear", "set where bit 11 is"


def three_ways(t, W, H, expect=ON, frames=FRAMES, **kw):
    """the job as shipped, with RTGO_NO_ROOMW=1 and on the canonical walk: the same bytes and the same rays.  expect: bit 12 of the first
    job's launches -- ON, OFF, or WITH_UNIT16 (set exactly where the launch would take render_unit16_kernel; the test prints which)."""
    a_w, i_w, r_w, v_w = render(t, W, H, 4, frames, env={"RTGO_NO_ROOMW": None}, **kw)
    a_u, i_u, r_u, v_u = render(t, W, H, 4, frames, env={"RTGO_NO_ROOMW": "1"}, **kw)
    a_c, i_c, r_c, v_c = render(t, W, H, 4, frames, env={"RTGO_NO_ROOMW": None}, stats=True, **kw)
    print("last_variant as shipped %s, with RTGO_NO_ROOMW=1 %s" % (v_w, v_u))
    assert len(v_w) == frames
    if expect == ON:
        assert all(v & ROOMW and v & UNIT16 and v & SLAB and v & PAIR7 and v & PAIR for v in v_w), v_w
    elif expect == OFF:
        assert all(not v & ROOMW for v in v_w), v_w
    else:
        print("bit 12 is %s: the launch %s render_unit16_kernel" % (("set", "would take") if v_w[0] & ROOMW else ("clear", "does not get")))
        assert all(bool(v & ROOMW) == bool(v & UNIT16) for v in v_w), v_w
    assert all(not v & ROOMW for v in v_u), v_u
    assert [v & ~ROOMW for v in v_w] == v_u, "RTGO_NO_ROOMW=1 changes more than bit 12: %s, %s" % (v_w, v_u)
    assert all(v & CANON and not v & (PAIR | SLAB | UNIT16 | ROOMW) for v in v_c), v_c
    assert r_w == r_u == r_c, (r_w, r_u, r_c)
    for name, a, i in (("RTGO_NO_ROOMW=1", a_u, i_u), ("the canonical walk", a_c, i_c)):
        assert a_w.tobytes() == a.tobytes(), "as shipped != %s: %d pixels" % (name, int(np.sum(np.any(a_w != a, axis=-1))))
        assert i_w.tobytes() == i.tobytes(), name
    return a_w


def look_at(t, eye, target, up=(0.0, 1.0, 0.0)):
    """cornell's camera (the lengths of its U, V and W) moved to `eye` and turned towards `target`"""
    cam = t["cam"].copy()
    ulen, vlen, wlen = [float(np.linalg.norm(cam[3 + 3 * a:6 + 3 * a])) for a in range(3)]
    w = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    w /= np.linalg.norm(w)
    u = np.cross(w, np.asarray(up, np.float64))
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    cam[0:3], cam[3:6], cam[6:9], cam[9:12] = eye, u * ulen, v * vlen, w * wlen
    return cam


# ---- cornell as the bench sees it, a window and a band share

def test_cornell_as_the_bench_sees_it():
    a = three_ways(tables("cornell", W, H), W, H)
    assert np.isfinite(a).all() and float(a[..., 0:3].max()) > 0.0


@pytest.mark.parametrize("max_depth", [0, 1])
def test_cornell_shallow_paths(max_depth):
    # (max_depth 0: no last-ray certificate, every ray tests the room; 1: the second ray is the last and skips it)
    three_ways(tables("cornell", 66, 8), 66, 8, max_depth=max_depth)


def test_a_window_and_a_half_band_share():
    t = tables("cornell", W, H)
    three_ways(t, W, H, expect=WITH_UNIT16, window=(5, 3, 150, 80))
    three_ways(t, W, H, expect=WITH_UNIT16, bands=(4, 2, 1))


# ---- cameras

def grazing(tilt):
    """tests/adversarial_cameras.py's camera in a plane x = c, a thousandth inside the left wall: every primary ray runs along that wall,
    exactly parallel to it (tilt 0: d.x = 0, the six single tests) or within ten times the parallel threshold of it"""
    cam = AC.in_plane(0, -3.999, (0.7, 3.3))
    cam[9] = tilt
    return cam


@pytest.mark.parametrize("tilt", [0.0, -3e-4, 3e-4, -6e-5])
def test_looking_along_a_wall_at_grazing_incidence(tilt):
    three_ways(tables("cornell", 96, 54), 96, 54, cam=grazing(tilt))


def test_eye_on_a_wall_plane():
    # (CORNELL_PLANES: from these eyes the rays that run inside the wall's own plane hit that wall)
    for axis, c, eye_ab, w_ab, _ in AC.CORNELL_PLANES[5:7]:
        three_ways(tables("cornell", 48, 36), 48, 36, frames=2, cam=AC.in_plane(axis, c, eye_ab, w_ab))


def test_on_the_diagonal_looking_into_a_corner():
    t = tables("cornell", 96, 54)
    three_ways(t, 96, 54, cam=look_at(t, (-1.0, -1.0, 1.0), (4.0, 4.0, -4.0)))
    three_ways(t, 96, 54, frames=2, cam=look_at(t, (3.0, 3.0, -3.0), (4.0, 4.0, -4.0)))


def test_eye_outside_looking_in_through_a_back_facing_wall():
    t = tables("cornell", 96, 54)
    three_ways(t, 96, 54, cam=look_at(t, (13.0, 2.0, 3.0), (0.0, -1.0, 0.0)))        # through the right wall
    three_ways(t, 96, 54, frames=2, cam=look_at(t, (2.0, 15.0, 1.0), (0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0)))   # through the ceiling, past the lamp


def test_eye_outside_looking_past_the_room():
    t = tables("cornell", 96, 54)
    cam = look_at(t, (0.0, 0.0, 14.0), (7.0, 1.0, 0.0))
    a = three_ways(t, 96, 54, cam=cam, bg=BG)
    full = np.zeros(3, np.float32)
    for _ in range(16):
        full = full + BG
    missed = np.all(a[..., 0:3] == full * np.float32(0.0625), axis=-1)
    print("pixels whose samples all miss: %d of %d" % (int(missed.sum()), missed.size))
    assert 0 < missed.sum() < missed.size, "the frame does not miss the room in part"
    three_ways(t, 96, 54, frames=2, cam=wide_camera(t), bg=BG, max_depth=1)


# ---- scene variants, rebuilt through set_scene

def room_variant(W, H, order=None, turn=0.0):
    """cornell with the room's six walls in another insertion order and / or turned about the world's y axis, boxes as the host computes
    them (the unit cube's corners through the model matrix, 1e-3 of padding)"""
    t = {key: v.copy() for key, v in tables("cornell", W, H).items()}
    if order is not None:
        for key in ("type", "M", "mat", "aabb"):
            t[key][0:6] = t[key][list(order)]
    if turn != 0.0:
        c, s = np.cos(turn), np.sin(turn)
        R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)
        for i in range(6):
            M = (R @ t["M"][i].astype(np.float64).reshape(4, 4)).astype(np.float32)
            t["M"][i] = M.reshape(16)
            corners = np.array([[x, y, z, 1.0] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
            w = (corners @ M.T)[:, :3]
            t["aabb"][i, 0:3] = w.min(axis=0) - np.float32(1e-3)
            t["aabb"][i, 3:6] = w.max(axis=0) + np.float32(1e-3)
    return t


@pytest.mark.parametrize("order", [(5, 2, 0, 4, 1, 3), (3, 4, 5, 0, 1, 2)])
def test_walls_in_another_insertion_order(order):
    three_ways(room_variant(96, 54, order=order), 96, 54)


def test_room_turned_by_a_millionth_keeps_the_kernel():
    three_ways(room_variant(96, 54, turn=1e-6), 96, 54)


def test_room_turned_by_a_thousandth_does_not_take_it():
    three_ways(room_variant(96, 54, turn=1e-3), 96, 54, expect=OFF)


def test_debug_line_names_the_kernel_first(capfd):
    t = tables("cornell", 66, 8)
    capfd.readouterr()
    *_, v = render(t, 66, 8, 4, 1, env={"RTGO_DEBUG": "1", "RTGO_NO_ROOMW": None})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    tail = ("kernel render_roomw_kernel, the world-room form of kernel render_unit16_kernel, the 16 spp form of kernel render_slab7_kernel, "
            "the slab form of kernel render_pair7_kernel")
    assert len(lines) == 1 and lines[0].endswith(tail), err[-2000:]
    assert all(x & ROOMW for x in v), v
