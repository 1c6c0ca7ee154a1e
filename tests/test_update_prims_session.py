"""Pick, then drag, through the scripted session (rtgo_host_session_pick, rtgo_host_session_update_prims): cornell's short box is picked
through a pixel, its six faces are moved, the progressive accumulation restarts, the next frame is the edited scene's -- bit for bit what
a context given the edited array through rtgo_set_scene renders -- and a pick at the box's old place returns the room behind it."""
import numpy as np
import pytest

import test_large_scenes as TL

pytestmark = pytest.mark.gpu

W, H = 64, 48
ROOM, SHORT_BOX = range(0, 6), range(6, 12)   # cornell: 0-5 the room, 6-11 the short box, 12-17 the tall box, 18 the lamp


@pytest.fixture(scope="module")
def mods():
    from raytracingo_amd import capi, scene
    capi.load()
    scene.load()
    return capi, scene


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("mode", ["path", "distributed"])
def test_pick_then_drag(mods, oracle, mode):
    capi, scene = mods
    t = scene.tables("cornell", W, H)
    s = scene.Session("cornell", mode, W, H)
    s.frame()
    s.frame()
    assert s.read()[2] == 1
    # the lowest, then leftmost pixel that shows the short box (its nearest bottom corner, the floor behind it): the box is dragged to the right
    on_box = [(x, y) for y in range(0, H, 2) for x in range(0, W, 2) if s.pick(x, y)[0] in SHORT_BOX]
    assert on_box, "no pixel shows the short box"
    x, y = min(on_box, key=lambda p: (p[1], p[0]))
    picked = s.pick(x, y)[0]
    faces = np.arange(6 * (picked // 6), 6 * (picked // 6) + 6)   # the cube the picked face belongs to
    M = t["M"][faces].copy()
    M[:, 3] += np.float32(1.1)
    s.update_prims(faces, t["type"][faces], M, t["mat"][faces])
    assert s.read()[2] == 1   # (the count restarts with the next frame, as after move_camera)
    after = s.pick(x, y)[0]
    assert after in ROOM, "pixel (%d, %d) showed face %d of the short box and now shows %d" % (x, y, picked, after)
    s.frame()
    acc, img, count = s.read()
    assert count == 0
    s.frame()
    assert s.read()[2] == 1
    # the edited scene through the set call, rendered as Renderer::Initialize sets the frame up
    t_new = dict(t, M=t["M"].copy(), aabb=t["aabb"].copy())
    t_new["M"][faces] = M
    t_new["aabb"][faces] = TL.oracle_boxes(oracle, M)
    ctx = capi.Context(0)
    ctx.set_scene(t_new["type"], t_new["M"], t_new["mat"], t_new["aabb"])
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)
    ctx.launch(capi.make_frame(W, H, 1, 0, mode == "path", False))
    ctx.sync()
    assert np.array_equal(bits(acc), bits(ctx.read_accum(H, W))) and np.array_equal(img, ctx.read_image(H, W))
    # and a refused edit is an error that leaves the session's scene: the same pick, the same next frame as the context's
    bad = M.copy()
    bad[0] = 0.0
    with pytest.raises(capi.RtgoError):
        s.update_prims(faces, t["type"][faces], bad, t["mat"][faces])
    assert s.pick(x, y)[0] == after
    ctx.launch(capi.make_frame(W, H, 1, 1, mode == "path", False))
    ctx.launch(capi.make_frame(W, H, 1, 2, mode == "path", False))
    ctx.sync()
    s.frame()
    acc2, _, count2 = s.read()
    assert count2 == 2 and np.array_equal(bits(acc2), bits(ctx.read_accum(H, W)))
    ctx.close()
    s.close()
