"""The pair kernels' ray loop carries the walk's predicates as the wave's lane masks (Pred<true>, rtgo_device.h; MASKS,
rtgo_render_body.inc): compares made by the compare builtins, combined on the scalar unit, voted on with `!= 0`.  Only how
a condition is carried changes -- no float operation, nor the order of any -- so everything a launch leaves (the accumulation buffer, the
8-bit image, the ray count) must be what the same launch leaves under RTGO_NO_PAIR=1, whose kernels keep the bool and __ballot, bit for
bit; rtgo_stats.last_variant bit 8 says the pair kernel ran.

The cases are built so that every converted vote goes both ways: waves with lanes that never start (partial masks, and complements that
must not count those lanes), every depth limit with and without the last-ray certificate (the `last` votes of the list), rays inside a
box's face plane and inside a wall's plane (the `both` votes), a ray along a box edge and one into a room corner (second and third turns
of cuboid_range's finish loop), a camera no primary of which meets a box (the leaf and `far` votes all zero) and one every primary of
which does.  Jobs are set up as tests/test_pair_walk.py sets them up (render(), on_off(): RTGO_TREE=0, RTGO_MAX_WPE to reach the kernel
under test on a small frame).  Needs a real MI355X."""
import numpy as np
import pytest

import adversarial_cameras as A
from test_pair_walk import BIT as PAIR_BIT, BOX_A, on_off, tables

pytestmark = pytest.mark.gpu

BIT7 = 512
W, H = 64, 48
INSIDE = np.array([0.3, 0.5, 3.5], dtype=np.float32)   # an eye inside the room (it spans -4 .. 4)


def check_variants(v, wpe):
    assert all(x & PAIR_BIT for x in v), v
    assert all(bool(x & BIT7) == (wpe == 7) for x in v), v


@pytest.mark.parametrize("wpe", [5, 6, 7])
@pytest.mark.parametrize("sample", [2, 4])
def test_cornell_frames_0_to_2(sample, wpe):
    _, v = on_off(tables("cornell", W, H), W, H, sample, 3, wpe=wpe)
    check_variants(v, wpe)


@pytest.mark.parametrize("wpe", [6, 7])
def test_a_wave_with_lanes_that_never_start(wpe):
    # 65 pixels a row at 16 spp: the row's last unit has one pixel, 48 of its 64 lanes never start
    w, h = 65, 3
    _, v = on_off(tables("cornell", w, h), w, h, 4, 2, wpe=wpe)
    check_variants(v, wpe)


@pytest.mark.parametrize("certificate", [True, False])
@pytest.mark.parametrize("max_depth", [0, 1, 2, 3, 4, 5])
def test_every_depth_limit_with_and_without_the_last_ray_certificate(max_depth, certificate):
    env = None if certificate else {"RTGO_NO_LAST_EMITTER": "1"}
    _, v = on_off(tables("cornell", W, H), W, H, 2, 2, wpe=7, max_depth=max_depth, env=env)
    check_variants(v, 7)


@pytest.mark.parametrize("wpe", [5, 7])
def test_background_that_is_not_black(wpe):
    t = {k: x.copy() for k, x in tables("cornell", W, H).items()}
    t["bg"] = np.array([0.25, 0.5, 0.125], dtype=np.float32)
    a, v = on_off(t, W, H, 2, 2, wpe=wpe)
    check_variants(v, wpe)
    assert np.any(np.all(a[:, :, 0:3] == t["bg"], axis=-1))


# (axis, plane, the eye's other two coordinates): the short box's top, a wall
@pytest.mark.parametrize("axis,c,eye_ab", [(1, -2.0, (0.7, 3.3)), (0, -4.0, (-3.3, -0.7))], ids=["box_face_plane", "wall_plane"])
@pytest.mark.parametrize("wpe", [6, 7])
def test_camera_inside_a_plane_of_the_scene(axis, c, eye_ab, wpe):
    t = tables("cornell", W, H)
    cam = A.in_plane(axis, c, eye_ab)
    assert A.zero_axes(cam) == [axis]
    _, v = on_off(t, W, H, 2, 2, wpe=wpe, cam=cam)
    check_variants(v, wpe)


def face_frame(t, row):
    """centre, the two edge vectors and the normal of rectangle `row` in world space (the unit square |x|, |z| <= 1/2 at y = 0 through M)"""
    M = t["M"][row].astype(np.float64).reshape(4, 4)
    return M[:3, 3], M[:3, 0], M[:3, 2], M[:3, 1]


def in_room(p):
    return bool(np.all(np.abs(p) < 3.9))


@pytest.mark.parametrize("wpe", [6, 7])
def test_one_ray_along_a_box_edge(wpe):
    # every pixel shoots the ray that runs along an edge of the short box, where two of its faces are left after the margins
    t = tables("cornell", W, H)
    c, ex, ez, _ = face_frame(t, BOX_A.start)
    along = ex / np.linalg.norm(ex)
    # the edge's end from which one unit further along the edge is still inside the room (the other end may stand on the floor)
    eyes = [(c + s * 0.5 * ex + 0.5 * ez + s * along, -s * along) for s in (1.0, -1.0)]
    eye, d = next((e, d) for e, d in eyes if in_room(e))
    _, v = on_off(t, W, H, 2, 2, wpe=wpe, cam=A.one_ray(eye.astype(np.float32), d.astype(np.float32)))
    check_variants(v, wpe)


@pytest.mark.parametrize("wpe", [6, 7])
def test_one_ray_into_a_room_corner(wpe):
    # ... and the ray into the corner where three walls meet: all three faces of the room are left
    t = tables("cornell", W, H)
    d = np.array([-4.0, -4.0, -4.0]) - INSIDE.astype(np.float64)
    _, v = on_off(t, W, H, 2, 2, wpe=wpe, cam=A.one_ray(INSIDE, d.astype(np.float32)))
    check_variants(v, wpe)


def looking(eye, w, half=0.2):
    """cam[12]: the eye, a view direction w and a narrow square field around it"""
    w = np.asarray(w, np.float64) / np.linalg.norm(w)
    u = np.cross(w, [0.0, 0.0, 1.0] if abs(w[2]) < 0.9 else [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    cam = np.zeros(12, np.float32)
    cam[0:3], cam[3:6], cam[6:9], cam[9:12] = eye, half * u, half * v, w
    return cam


@pytest.mark.parametrize("wpe", [6, 7])
def test_no_primary_meets_a_box(wpe):
    # from above the boxes, looking up at the ceiling beside the lamp
    t = tables("cornell", W, H)
    _, v = on_off(t, W, H, 2, 2, wpe=wpe, cam=looking(np.array([-2.5, 2.0, 2.5]), [0.0, 1.0, 0.0]))
    check_variants(v, wpe)


@pytest.mark.parametrize("wpe", [6, 7])
def test_every_primary_meets_a_box(wpe):
    # half a unit in front of a face of the short box, looking straight at it
    t = tables("cornell", W, H)
    c, _, _, n = face_frame(t, BOX_A.start)
    n = n / np.linalg.norm(n)
    eye = c + 0.5 * n
    assert in_room(eye), eye
    _, v = on_off(t, W, H, 2, 2, wpe=wpe, cam=looking(eye, -n))
    check_variants(v, wpe)
