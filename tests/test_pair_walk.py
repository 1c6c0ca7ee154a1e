"""The straight-line walk of a two-leaf tree (render_pair_kernel, fast_pair): a path-mode launch over a flat scene whose
fast-walk tree is a root over two certified cuboid leaves (cornell: the short and the tall box) takes a kernel that tests the two child
boxes and walks the nearer leaf, then the farther one under the stack word's cull, without root test, loop, stack or leaf dispatch.  It
makes the leaf tests fast_tree makes, on the same values, so everything a launch leaves -- the accumulation buffer, the image, the ray
count -- must be what RTGO_NO_PAIR=1 leaves (today's kernel), bit for bit, and rtgo_stats.last_variant bit 8 says which one ran.

The pair kernel exists at 5 and 6 waves per SIMD.  A 96 x 64 frame has too few units for more than 4 (pick_block), so the small cases set
RTGO_MAX_WPE, for the pair launch and for the one it is held to alike: without it they would not run the kernel under test.  The
512 x 288 cases reach 6 waves by their own work.  A job's first launches are the launch-time trial's: they time both fast-walk structures,
and cornell's second one (the 15 % tree) is no two-leaf tree, so its launches keep today's kernel; the cases pin the first structure
(RTGO_TREE=0) except the one that is about the trial.  Needs a real MI355X."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOB = "RTGO_NO_PAIR"
BIT = 256
FULL = (4, 1, 0)


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def render(t, W, H, N, frames, off, wpe=None, max_depth=5, bands=FULL, cam=None, path=True, stats=False, batched=0, env=None):
    """accum and image of the launch's rows after `frames` progressive frames, rays_total, and last_variant of every launch"""
    from raytracingo_amd import capi
    kv = {KNOB: "1" if off else None, "RTGO_MAX_WPE": wpe, "RTGO_TREE": "0"}
    kv.update(env or {})
    with Env(**kv):
        ctx = capi.Context(0)
        try:
            ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
            c = t["cam"] if cam is None else cam
            ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
            ctx.set_background(t["bg"])
            ctx.set_lights(t["lights"])
            rows = capi.local_rows(H, *bands)
            ctx.resize(rows * W)
            variants = []
            if batched:
                ctx.launch_frames(capi.make_frame(W, H, N, 0, path, max_depth=max_depth, bands=bands), batched)
                ctx.sync()
                variants.append(ctx.stats()["last_variant"])
            else:
                for f in range(frames):
                    ctx.launch(capi.make_frame(W, H, N, f, path, max_depth=max_depth, bands=bands, stats=stats))
                    ctx.sync()
                    variants.append(ctx.stats()["last_variant"])
            return ctx.read_accum(rows, W).copy(), ctx.read_image(rows, W).copy(), ctx.stats()["rays_total"], variants
        finally:
            ctx.close()


def on_off(t, W, H, N, frames, **kw):
    """the same job with the pair kernel allowed and with RTGO_NO_PAIR=1: the same bits, image and rays; bit 8 clear in every launch of the
    second.  Returns the first job's accumulation buffer and the last_variant of each of its launches."""
    a_on, i_on, r_on, v_on = render(t, W, H, N, frames, False, **kw)
    a_off, i_off, r_off, v_off = render(t, W, H, N, frames, True, **kw)
    assert all(v & BIT == 0 for v in v_off), v_off
    assert r_on == r_off
    assert a_on.tobytes() == a_off.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a_on != a_off, axis=-1)))
    assert i_on.tobytes() == i_off.tobytes()
    return a_on, v_on


def tables(name, W, H):
    from raytracingo_amd import scene
    return scene.tables(name, W, H)


# ---- cornell, small frames

@pytest.mark.parametrize("N,max_depth,wpe", [(4, 5, 6), (2, 5, 6), (4, 1, 6), (2, 1, 5), (4, 5, 5)])
def test_cornell_small_frames(N, max_depth, wpe):
    W, H = 96, 64
    _, v = on_off(tables("cornell", W, H), W, H, N, 3, wpe=wpe, max_depth=max_depth)
    assert all(x & BIT for x in v), v


def test_cornell_through_the_launch_time_trial():
    # unpinned: the job's first launches alternate between the two structures; the pair kernel goes with the first alone
    W, H = 96, 64
    _, v = on_off(tables("cornell", W, H), W, H, 4, 6, wpe=6, env={"RTGO_TREE": None})
    assert [bool(x & BIT) for x in v] == [not (x & 2) for x in v], v
    assert any(x & BIT for x in v) and any(x & 8 for x in v), v


@pytest.mark.parametrize("wpe", [5, 6])
def test_cornell_band_share(wpe):
    W, H = 96, 64
    _, v = on_off(tables("cornell", W, H), W, H, 4, 3, wpe=wpe, bands=(4, 8, 5))
    assert all(x & BIT for x in v), v


def inside_camera(t):
    cam = t["cam"].copy()
    cam[0:3] = np.array([0.3, 0.5, 3.5], dtype=np.float32)   # (the room spans -4 .. 4)
    return cam


@pytest.mark.parametrize("wpe", [None, 5])
def test_cornell_eye_inside_the_room_takes_the_pair_kernel_by_its_own_work(wpe, capfd):
    # 512 x 288 at 16 spp: the smallest frame with >= 8 units per wave, which is what takes a launch to 6 waves per SIMD
    W, H = 512, 288
    t = tables("cornell", W, H)
    capfd.readouterr()
    a_on, _, r_on, v_on = render(t, W, H, 4, 2, False, wpe=wpe, cam=inside_camera(t), env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    a_off, _, r_off, v_off = render(t, W, H, 4, 2, True, wpe=wpe, cam=inside_camera(t))
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 2, err[-2000:]
    for l in lines:
        assert re.search(r"kernel render_pair_kernel<%d>$" % (5 if wpe else 6), l), l
    assert all(v & BIT for v in v_on) and all(v & BIT == 0 for v in v_off), (v_on, v_off)
    assert r_on == r_off
    assert a_on.tobytes() == a_off.tobytes(), "accumulation differs: %d pixels" % int(np.sum(np.any(a_on != a_off, axis=-1)))


# ---- seeded scenes: cornell's room and emitter, its two boxes at other poses

ROOM, BOX_A, BOX_B = slice(0, 6), slice(6, 12), slice(12, 18)   # rows of scene.tables("cornell"): Scene::CreateCornellBox's order


def trs(center, axis, angle, scale):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    P = np.eye(4)
    P[:3, :3] = R @ np.diag(scale)
    P[:3, 3] = center
    return P


# the poses CreateCornellBox gives the two unit cubes (|x|, |y|, |z| <= 1/2)
POSE_A = trs([1.3, -3.0, 1.3], [0, 1, 0], -np.pi / 6.0, [2.0, 2.0, 2.0])
POSE_B = trs([-1.3, -2.0, -1.3], [0, 1, 0], np.pi / 8.0, [2.0, 4.0, 2.0])


def reposed(t, rows, old, new):
    """the six faces of one box carried from pose `old` to pose `new`, with boxes computed as the host computes them (the unit cube's
    corners through the model matrix, 1e-3 of padding)"""
    A = new @ np.linalg.inv(old)
    for i in range(rows.start, rows.stop):
        M = (A @ t["M"][i].astype(np.float64).reshape(4, 4)).astype(np.float32)
        t["M"][i] = M.reshape(16)
        corners = np.array([[x, y, z, 1.0] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
        w = (corners @ M.T)[:, :3]
        t["aabb"][i, 0:3] = w.min(axis=0) - np.float32(1e-3)
        t["aabb"][i, 3:6] = w.max(axis=0) + np.float32(1e-3)


def seeded_scene(k, W, H):
    """scene k of 8: (tables, camera).  Every one has the room, the emitter and two boxes; what each adds is in its comment."""
    t = {key: v.copy() for key, v in tables("cornell", W, H).items()}
    rng = np.random.default_rng(20261019 + k)
    cam = t["cam"].copy()

    def on_floor(cx, cz, angle, scale):   # a box standing on the floor (y = -4), turned about the vertical
        return trs([cx, -4.0 + 0.5 * scale[1], cz], [0, 1, 0], angle, scale)

    def afloat(c, scale):                 # a box in the air at a random rotation
        return trs(c, rng.normal(size=3), rng.uniform(0.0, np.pi), scale)

    if k == 0:     # both boxes touch the floor, random sizes and turns
        pa = on_floor(1.6, 1.0, rng.uniform(-1, 1), rng.uniform(1.0, 2.5, size=3))
        pb = on_floor(-1.6, -1.0, rng.uniform(-1, 1), rng.uniform(1.0, 2.5, size=3))
    elif k == 1:   # both in the air, any rotation
        pa, pb = afloat([1.5, 0.5, 0.5], rng.uniform(0.8, 2.0, size=3)), afloat([-1.5, -1.0, -0.5], rng.uniform(0.8, 2.0, size=3))
    elif k == 2:   # the boxes' axis-aligned boxes overlap (the turned boxes themselves do not meet)
        pa = on_floor(0.9, 0.9, np.pi / 4.0, [1.5, 2.0, 1.5])
        pb = on_floor(-0.9, -0.9, np.pi / 4.0, [1.5, 3.0, 1.5])
    elif k == 3:   # one in front of the other along the view: most rays that hit the near box's bounds hit the far one's too
        pa = on_floor(0.2, 2.0, rng.uniform(-0.5, 0.5), [1.5, 1.5, 1.5])
        pb = on_floor(-0.2, -1.5, rng.uniform(-0.5, 0.5), [2.5, 4.0, 1.5])
    elif k == 4:   # an axis-aligned camera and axis-aligned boxes: direction components and plane normals' components are exactly 0
        pa = on_floor(1.5, 0.5, 0.0, [2.0, 2.0, 2.0])
        pb = on_floor(-1.5, -0.5, 0.0, [2.0, 3.0, 2.0])
        cam[0:3] = [0.0, 0.0, 14.0]
        ulen, vlen, wlen = [float(np.linalg.norm(cam[3 + 3 * a:6 + 3 * a])) for a in range(3)]
        cam[3:6], cam[6:9], cam[9:12] = [ulen, 0.0, 0.0], [0.0, vlen, 0.0], [0.0, 0.0, -wlen]
    elif k == 5:   # the eye inside one leaf's box (its faces look outwards: seen from inside it is not there)
        pa = on_floor(1.5, 1.0, 0.3, [2.0, 2.0, 2.0])
        pb = on_floor(-0.5, 2.5, 0.2, [2.0, 5.0, 2.0])
        cam[0:3] = [-0.5, -1.0, 2.5]
    elif k == 6:   # a tall thin box on the floor beside a flat wide one in the air, tilted
        pa = on_floor(2.4, -1.0, rng.uniform(-1, 1), [1.0, 4.5, 1.0])
        pb = trs([-1.7, -1.0, 1.0], rng.normal(size=3), 0.3, [3.0, 1.0, 2.0])
    else:          # overlapping axis-aligned boxes in the air, any rotation
        pa, pb = afloat([0.8, 0.0, 0.0], [1.2, 1.2, 1.2]), afloat([-0.8, 0.3, 0.2], [1.2, 1.2, 1.2])
    reposed(t, BOX_A, POSE_A, pa)
    reposed(t, BOX_B, POSE_B, pb)
    return t, cam


@pytest.mark.parametrize("k", range(8))
def test_seeded_two_box_rooms(k):
    W, H = 96, 64
    t, cam = seeded_scene(k, W, H)
    a_on, v_on = on_off(t, W, H, 4, 1, wpe=6, cam=cam)
    assert all(x & BIT for x in v_on), v_on
    # ... and against the canonical walk, which defines the closest hit
    a_canon, _, _, v = render(t, W, H, 4, 1, False, wpe=6, cam=cam, stats=True)
    assert v[0] & 4 and not v[0] & BIT
    assert a_on.tobytes() == a_canon.tobytes(), "fast_pair != canonical walk: %d pixels" % int(np.sum(np.any(a_on != a_canon, axis=-1)))


# ---- launches that must not take it

def one_box_room(W, H):
    t = tables("cornell", W, H)
    keep = np.r_[0:12, 18:len(t["type"])]
    return {key: (v[keep].copy() if key in ("type", "M", "mat", "aabb") else v) for key, v in t.items()}


@pytest.mark.parametrize("what", ["checkered", "balls", "distributed", "no_cuboid", "launch_frames", "one_box"])
def test_launches_that_do_not_qualify(what):
    W, H = 96, 64
    kw = dict(wpe=6)
    if what in ("checkered", "balls"):
        t = tables(what, W, H)
    elif what == "one_box":
        t = one_box_room(W, H)
    else:
        t = tables("cornell", W, H)
    if what == "distributed":
        kw["path"] = False
    if what == "no_cuboid":
        kw["env"] = {"RTGO_NO_CUBOID": "1"}
    if what == "launch_frames":
        kw["batched"] = 3
    _, v = on_off(t, W, H, 4, 2, **kw)
    assert not any(x & BIT for x in v), v
