"""What a launch already decides, taken out of the pair kernels' ray loop: the kind of the list's cuboid as a template
parameter of cuboid_range (a room for the pair kernels, whose launches vouch for it; a box for every leaf), the last-ray predicate as one
word of the launch (LaunchParams::pair.last_depth), and the two-leaf scene's counts (kPairNodes, kPairSmall) as compile-time values, so that the
list's records sit at constant offsets.  None of it touches arithmetic that reaches a pixel, so everything a launch leaves -- the
accumulation buffer, the 8-bit image, the ray count -- must be, bit for bit, what the canonical walk leaves (a collect_stats launch,
which defines the closest hit) and what RTGO_NO_PAIR=1 leaves (the generic kernel, which still takes the cuboid's kind from the launch).

Cases: cornell at 64 x 48, 4 and 16 spp, max_depth 0 (no last ray: the certificate needs a bounce), 1 (the last ray is the first bounce)
and 5, through the pair kernels at 7, 6 and 5 waves per SIMD (RTGO_MAX_WPE: a frame this small takes 4 by its own work); the same with
RTGO_NO_LAST_EMITTER=1, where last_depth must say "no depth"; a scene whose list starts with a certified box (list_cub = 1: one big
cuboid, a small cube and the emitter), so that both kinds of cuboid and both kinds of margin run; two scenes with the pair kernels' tree
under a list that is no room (a certified box; a room with a wall missing), which must keep the generic kernel; and a frame 65 pixels
wide, whose strips end in a partial unit.  The references of a (spp, depth) are rendered once and shared.  Jobs pin the first fast-walk structure
(RTGO_TREE=0), as tests/test_pair_walk.py sets them up: its render() runs them.  Needs a real MI355X."""
import re

import numpy as np
import pytest

from test_pair_walk import BIT as PAIR_BIT, BOX_A, BOX_B, POSE_A, POSE_B, ROOM, render, reposed, tables, trs

pytestmark = pytest.mark.gpu

LAST_RAY_BIT = 64
CANON_BIT = 4
W, H, FRAMES = 64, 48, 2

_refs = {}


def references(name, t, w, h, N, max_depth):
    """(accum, image, rays) of the canonical walk and of the generic kernel (RTGO_NO_PAIR=1), which must agree; rendered once per key"""
    key = (name, w, h, N, max_depth)
    if key not in _refs:
        a_c, i_c, r_c, v_c = render(t, w, h, N, FRAMES, False, wpe=6, max_depth=max_depth, stats=True)
        assert all(v & CANON_BIT and not v & PAIR_BIT for v in v_c), v_c
        a_g, i_g, r_g, v_g = render(t, w, h, N, FRAMES, True, wpe=6, max_depth=max_depth)
        assert all(not v & PAIR_BIT and not v & CANON_BIT for v in v_g), v_g
        assert a_g.tobytes() == a_c.tobytes(), "generic kernel != canonical walk: %d pixels" % int(np.sum(np.any(a_g != a_c, axis=-1)))
        assert i_g.tobytes() == i_c.tobytes()
        _refs[key] = (a_c, i_c, r_g)
        assert float(a_c[..., :3].max()) > 0.0, "the frame is black: nothing would be compared"
    return _refs[key]


def same(got, ref, what):
    a, i, r, _ = got
    a_ref, i_ref, r_ref = ref
    assert a.tobytes() == a_ref.tobytes(), "%s: accumulation differs in %d pixels" % (what, int(np.sum(np.any(a != a_ref, axis=-1))))
    assert i.tobytes() == i_ref.tobytes(), what
    # (a collect_stats launch traces the pixels the timed kernels write without tracing: the ray count is held to the generic kernel's)
    assert r == r_ref > 0, (what, r, r_ref)


@pytest.mark.parametrize("max_depth", [0, 1, 5])
@pytest.mark.parametrize("N", [2, 4])
def test_cornell_pair_kernels_against_canonical_and_generic(N, max_depth):
    t = tables("cornell", W, H)
    ref = references("cornell", t, W, H, N, max_depth)
    for wpe in (7, 6, 5):
        got = render(t, W, H, N, FRAMES, False, wpe=wpe, max_depth=max_depth)
        v = got[3]
        assert all(x & PAIR_BIT for x in v), (wpe, v)
        assert all(bool(x & 512) == (wpe == 7) for x in v), (wpe, v)
        # the last-ray certificate is on exactly when there is a bounce to be last
        assert all(bool(x & LAST_RAY_BIT) == (max_depth >= 1) for x in v), (wpe, max_depth, v)
        same(got, ref, "cornell spp %d depth %d at %d waves" % (N * N, max_depth, wpe))


@pytest.mark.parametrize("max_depth", [0, 1, 5])
@pytest.mark.parametrize("N", [2, 4])
def test_cornell_without_the_last_ray_certificate(N, max_depth):
    t = tables("cornell", W, H)
    ref = references("cornell", t, W, H, N, max_depth)
    for wpe in (7, 6, 5):
        got = render(t, W, H, N, FRAMES, False, wpe=wpe, max_depth=max_depth, env={"RTGO_NO_LAST_EMITTER": "1"})
        v = got[3]
        assert all(x & PAIR_BIT and not x & LAST_RAY_BIT for x in v), (wpe, v)
        same(got, ref, "cornell spp %d depth %d at %d waves, RTGO_NO_LAST_EMITTER" % (N * N, max_depth, wpe))


def box_list_scene(w, h):
    """one big cuboid -- cornell's tall box, grown to most of the scene and tilted, so that its six faces are the up-front list and no
    face is antiparallel to the emitter -- with cornell's short box as a small cube on top of it, under cornell's emitter; no room"""
    t = {key: v.copy() for key, v in tables("cornell", w, h).items()}
    reposed(t, BOX_B, POSE_B, trs([0.0, -1.5, 0.0], [0.3, 1.0, 0.2], 0.4, [5.0, 4.0, 5.0]))
    reposed(t, BOX_A, POSE_A, trs([0.6, 1.6, 0.4], [0.0, 1.0, 0.0], 0.5, [1.0, 1.0, 1.0]))
    keep = np.r_[BOX_A, BOX_B, ROOM.stop + 12:len(t["type"])]
    return {key: (v[keep].copy() if key in ("type", "M", "mat", "aabb") else v) for key, v in t.items()}


def test_the_box_list_scene_has_a_certified_box_at_the_start_of_its_list():
    from raytracingo_amd import capi
    t = box_list_scene(W, H)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
        decoded = np.ascontiguousarray(ctx.read_build(False)["tree0.decoded"]).view(np.int32)
    finally:
        ctx.close()
    # {canonical depth, fast_depth, n_small, n_fnodes, n_big_pairs, list_cub, ...} (rtgo_capi.hip, build_spans)
    assert decoded[5] == 1 and decoded[4] == 3, decoded[:8]
    assert 0 < decoded[2] <= len(t["type"]) - 6, decoded[:8]   # (small primitives in the tree: the cube, and the emitter unless it is big)


@pytest.mark.parametrize("wpe", [None, 6])
@pytest.mark.parametrize("max_depth", [1, 5])
def test_box_list_scene(max_depth, wpe, capfd):
    t = box_list_scene(W, H)
    ref = references("box_list", t, W, H, 4, max_depth)
    capfd.readouterr()
    got = render(t, W, H, 4, FRAMES, False, wpe=wpe, max_depth=max_depth, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == FRAMES, err[-2000:]
    for l in lines:
        # the list's box is still certified at this launch's reach (a margin of -1: the launch dropped it), and the kernel is the generic one
        m = re.search(r"cuboid margin ([-+0-9.e]+),", l)
        assert m and 0.0 < float(m.group(1)) < 0.02, l
        assert re.search(r"kernel render_kernel<%s>$" % (wpe or r"\d"), l), l
    assert all(not x & PAIR_BIT and not x & LAST_RAY_BIT for x in got[3]), got[3]
    same(got, ref, "box-list scene depth %d" % max_depth)


# ---- two-leaf trees under a list that is no room: the pair kernels are compiled for a room (fast_list's KIND, kPairSmall), and the only
# thing that keeps them from such a launch is the host's `list_cub == 2`.  These scenes have the pair kernels' tree -- read back from the
# build -- and another list; a launch that took a pair kernel would test the list's first six records as a room.

EMITTER = slice(18, 19)   # (cornell's rows after the room and the two boxes)


def pair_tree_under_a_box_list(w, h):
    """list_cub = 1: one big tilted cuboid (cornell's tall box, grown), two small cubes above it -- apart on every axis, so that the
    tree's first split parts them whatever axis it takes -- and the emitter grown about its centre until it is big, so that it joins the
    list and the tree holds the two cubes alone.  The cubes are cornell's short box and a copy of its six faces in the room's rows."""
    t = {key: v.copy() for key, v in tables("cornell", w, h).items()}
    reposed(t, BOX_B, POSE_B, trs([0.0, -1.5, 0.0], [0.3, 1.0, 0.2], 0.4, [5.0, 4.0, 5.0]))
    for key in ("type", "M", "mat", "aabb"):
        t[key][ROOM] = t[key][BOX_A]
    reposed(t, ROOM, POSE_A, trs([1.7, 2.9, 1.7], [0.0, 1.0, 0.0], 0.5, [1.0, 1.0, 1.0]))
    reposed(t, BOX_A, POSE_A, trs([-1.7, 1.3, -1.7], [0.0, 1.0, 0.0], -0.3, [1.0, 1.0, 1.0]))
    centre = t["M"][EMITTER][0].astype(np.float64).reshape(4, 4)[:3, 3]
    grow = np.diag([3.0, 3.0, 3.0, 1.0])
    grow[:3, 3] = centre - 3.0 * centre
    reposed(t, EMITTER, np.eye(4), grow)
    return {key: (v[:19].copy() if key in ("type", "M", "mat", "aabb") else v) for key, v in t.items()}


def pair_tree_under_a_broken_room(w, h):
    """list_cub = 0: cornell without one wall -- five walls pair up twice, no cuboid; the two boxes and the emitter stay"""
    t = tables("cornell", w, h)
    keep = np.r_[0:5, 6:len(t["type"])]
    return {key: (v[keep].copy() if key in ("type", "M", "mat", "aabb") else v) for key, v in t.items()}


NOT_A_ROOM = {"box_list": (pair_tree_under_a_box_list, 1), "broken_room": (pair_tree_under_a_broken_room, 0)}


@pytest.mark.parametrize("which", sorted(NOT_A_ROOM))
def test_pair_tree_under_another_list_keeps_the_generic_kernel(which):
    from raytracingo_amd import capi
    make, list_cub = NOT_A_ROOM[which]
    t = make(W, H)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
        decoded = np.ascontiguousarray(ctx.read_build(False)["tree0.decoded"]).view(np.int32)
    finally:
        ctx.close()
    # {canonical depth, fast_depth, n_small, n_fnodes, n_big_pairs, list_cub, cuboid_groups, tree_spheres}: the pair kernels' tree ...
    assert decoded[2] == 12 and decoded[3] == 3, decoded[:8]
    assert decoded[6] == 2 + (1 if list_cub else 0), decoded[:8]      # (two certified leaves, and the list's cuboid if it has one)
    # ... under a list that is no room
    assert decoded[5] == list_cub, decoded[:8]
    ref = references("pair tree, " + which, t, W, H, 4, 5)   # (a key of its own: "box_list" is the one-cube scene's)
    for wpe in (7, 6, 5):
        got = render(t, W, H, 4, FRAMES, False, wpe=wpe)
        assert all(not x & PAIR_BIT and not x & 512 for x in got[3]), (which, wpe, got[3])
        same(got, ref, "%s at %d waves" % (which, wpe))


@pytest.mark.parametrize("wpe", [7, 6])
def test_a_frame_whose_strips_end_in_a_partial_unit(wpe):
    w = 65
    t = tables("cornell", w, H)
    ref = references("cornell", t, w, H, 4, 5)
    got = render(t, w, H, 4, FRAMES, False, wpe=wpe)
    assert all(x & PAIR_BIT for x in got[3]), got[3]
    same(got, ref, "cornell 65 pixels wide at %d waves" % wpe)
