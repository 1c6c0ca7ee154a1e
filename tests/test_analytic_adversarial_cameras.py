"""The analytic fast walks on rays that lie in the planes of the scene and of the walks' own structures (tests/adversarial_cameras.py), on
the MI355X.  Needs a real MI355X.

A frame's camera is the only thing that drives a fast walk -- both trees, the up-front list with cuboid_range, cornell's pair kernels,
fast_grid -- so the cameras here put every primary ray of a frame into one plane: a wall, a box's face, a face of a node box of either
fast-walk tree or of the canonical LBVH, a bound or a cell plane of the uniform grid, with an exact zero (of either sign) in the
direction.  Per case:

1. rtgo_trace_rays over the launch's own rays (shade_rays_ref.raygen32) equals the brute force over the oracle's intersection programs on
   EVERY ray -- primitive, the bits of t, the bits of n -- through rtgo_set_scene with the scene in global memory and in LDS, and through
   rtgo_set_large_scene.  float64 is no yardstick here (analytic_ref64.closest calls every such ray unclear); no ray is set aside.
2. the instrumented canonical frame holds tests/parity.py against the oracle's render, in the three modes.
3. every pinned fast launch equals the canonical frame bit for bit -- accumulation buffer, image, rays_total, rays_occlusion -- and
   rtgo_stats.last_variant proves that the launch took the walk its pin names.
4. rtgo_shade_rays over the launch's own rays and seeds leaves the launch's buffers.

The conditions on the inputs (how many primaries hit, miss, hit a primitive whose tight box straddles the plane) are asserted, not
tolerated: the eyes and planes below were chosen so that the oracle meets them.  Counts per family: DESIGN.md section 4."""
import numpy as np
import pytest

import adversarial_cameras as A
import shade_rays_ref as R
from parity import assert_parity
from test_gpu_parity import _box_scene, _cuboid_scene, _random_scene
from test_trace_rays import Knob

pytestmark = pytest.mark.gpu

W, H = 48, 36            # in-plane cameras
W1, H1 = 8, 8            # one_ray cameras
TMIN, TMAX = R.T_MIN0, R.T_MAX0
MODES = {"path": (True, False), "distributed": (False, False), "ambient": (False, True)}
GRID_ENV = {"RTGO_GRID_MIN": 4, "RTGO_GRID_MAX_DUP": 8}      # as in test_uniform_grid_walk_on_random_scenes
CANON, SECOND_TREE, GRID, LARGE, BATCH, PAIR, PAIR7 = 4, 2, 16, 32, 128, 256, 512     # bits of rtgo_stats.last_variant
BOX_SCENES = {"boxes49": (49, 3), "boxes122": (122, 3)}       # (seed, boxes): every box and sphere stays inside the room, so the grid's bounds do too


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    assert m.HIT_DTYPE == A.HIT_DTYPE and m.HIT_MISS == A.HIT_MISS
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Bundle:
    """one scene: the oracle's Scene and tables, a context of rtgo_set_scene, one of rtgo_set_large_scene and one built under
    RTGO_NO_CUBOID=1, and what rtgo_set_scene built"""

    def __init__(self, capi, oracle, name):
        self.name, self.env, aabb = name, {}, False
        if name in ("cornell", "checkered", "balls"):
            self.sc, aabb = oracle.scene(name, W, H), True
            self.t = oracle.scene_tables(self.sc)
        elif name == "random1":
            self.sc, self.t = _random_scene(oracle, 1, W, H)
        elif name == "room":
            self.sc, self.t = _cuboid_scene(oracle, W, H, "good", turns=(0.0, 0.0))
        else:
            seed, n_boxes = BOX_SCENES[name]
            self.sc, self.t = _box_scene(oracle, seed, W, H, n_boxes, True, False)
            self.env = dict(GRID_ENV)
        t = self.t
        self.ctxs = []
        for large, knobs in ((False, {}), (True, {}), (False, {"RTGO_NO_CUBOID": 1})):
            with Knob(**dict(self.env, **knobs)):
                ctx = capi.Context(0)
                (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t["aabb"] if aabb else None)
            ctx.set_background(t["bg"])
            ctx.set_lights(t["lights"])
            ctx.resize(W * H)
            self.ctxs.append(ctx)
        self.ctx, self.big, self.nocub = self.ctxs
        assert self.nocub.stats()["cuboid_groups"] == 0
        self.build = self.ctx.read_build(False)
        self.tight = np.asarray(self.build["tight"], np.float32).reshape(-1, 6)
        info = np.ascontiguousarray(self.build["scene.info"]).view(np.int32)
        self.have_alt, self.has_grid = bool(info[2]), bool(info[3])

    def set_camera(self, cam):
        for k, name in enumerate(("eye", "U", "V", "W")):
            getattr(self.sc, name)[:] = [float(v) for v in cam[3 * k:3 * k + 3]]
        for ctx in self.ctxs:
            ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])

    def close(self):
        for ctx in self.ctxs:
            ctx.close()


@pytest.fixture(scope="module")
def bundles(capi, oracle):
    have = {}

    def get(name):
        if name not in have:
            have[name] = Bundle(capi, oracle, name)
        return have[name]

    yield get
    for b in have.values():
        b.close()


def launch(capi, B, ctx, w, h, n, mode, env, frames=(0,), stats=False, batched=0):
    """the launches of `frames` (progressive) or one rtgo_launch_frames call over `batched` frames, under the knobs `env`:
    (accum, image, rays_total, rays_occlusion, last_variant of the last launch)"""
    path, amb = MODES[mode]
    with Knob(**dict(B.env, **env)):
        s0 = ctx.stats()
        if batched:
            ctx.launch_frames(capi.make_frame(w, h, n, 0, path, amb, bands=(1, 1, 0)), batched)
        else:
            for f in frames:
                ctx.launch(capi.make_frame(w, h, n, f, path, amb, bands=(1, 1, 0), stats=stats))
        ctx.sync()
        s1 = ctx.stats()
    return (ctx.read_accum(h, w).copy(), ctx.read_image(h, w).copy(), s1["rays_total"] - s0["rays_total"],
            s1["rays_occlusion"] - s0["rays_occlusion"], s1["last_variant"])


def same_frame(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), "%s: accum differs at %d pixels" % (what, int((bits(got[0]) != bits(want[0])).any(-1).sum()))
    assert np.array_equal(got[1], want[1]), "%s: image" % what
    assert got[2:4] == want[2:4], "%s: (rays_total, rays_occlusion) %r against %r" % (what, got[2:4], want[2:4])


def pins_of(B):
    """(name, knobs, context, modes, the proof that the launch took the walk the pin names: last_variant -> bool)"""
    fast = lambda v: not v & CANON
    pins = [("RTGO_TREE=0", {"RTGO_TREE": 0}, B.ctx, MODES, lambda v: fast(v) and not v & (SECOND_TREE | GRID)),
            ("RTGO_MAX_WPE=4", {"RTGO_MAX_WPE": 4, "RTGO_TREE": 0}, B.ctx, MODES, lambda v: fast(v) and not v & PAIR),
            ("RTGO_MAX_WPE=5", {"RTGO_MAX_WPE": 5, "RTGO_TREE": 0}, B.ctx, MODES, fast),
            ("RTGO_NO_CUBOID=1", {"RTGO_NO_CUBOID": 1}, B.nocub, MODES, fast),
            ("RTGO_NO_PAIR=1", {"RTGO_NO_PAIR": 1, "RTGO_MAX_WPE": 6, "RTGO_TREE": 0}, B.ctx, ["path"], lambda v: fast(v) and not v & PAIR),
            ("rtgo_set_large_scene", {}, B.big, MODES, lambda v: bool(v & LARGE) and bool(v & CANON))]
    if B.have_alt:
        pins.append(("RTGO_TREE=1", {"RTGO_TREE": 1}, B.ctx, MODES, lambda v: fast(v) and bool(v & SECOND_TREE)))
    if B.has_grid:
        pins.append(("RTGO_TREE=2", {"RTGO_TREE": 2}, B.ctx, MODES, lambda v: fast(v) and bool(v & GRID)))
    if B.name == "cornell":
        pins.append(("pair kernel, 5 waves", {"RTGO_MAX_WPE": 5, "RTGO_TREE": 0}, B.ctx, ["path"], lambda v: fast(v) and bool(v & PAIR)))
        pins.append(("pair kernel, 6 waves", {"RTGO_MAX_WPE": 6, "RTGO_TREE": 0}, B.ctx, ["path"], lambda v: fast(v) and bool(v & PAIR) and not v & PAIR7))
        pins.append(("pair kernel, 7 waves", {"RTGO_MAX_WPE": 7, "RTGO_TREE": 0}, B.ctx, ["path"], lambda v: fast(v) and bool(v & PAIR) and bool(v & PAIR7)))
    return pins


def check_case(capi, oracle, B, cam, w, h, what, plane=None, need_hits=0, need_misses=0, need_straddling=0):
    """the four assertions of this file's docstring for one camera.  plane: (axis, c) of an in-plane camera.  Returns the counts."""
    cam = np.asarray(cam, np.float32)
    B.set_camera(cam)
    o, d, seed = A.rays(cam, w, h, 0)
    ref = A.brute_hits(oracle, B.sc, o, d, TMIN, TMAX)
    hit = ref["prim"] >= 0
    fig = {"rays": len(o), "hits": int(hit.sum()), "misses": int((~hit).sum()), "edge": int(A.edge_hits(B.t, o, d, ref).sum()),
           "prims": np.unique(ref["prim"][hit]).tolist()}
    if plane is not None:
        axis, c = plane
        assert cam[axis] == np.float32(c) and axis in A.zero_axes(cam)
        fig["straddling"] = int((hit & A.straddlers(B.tight, axis, c)[np.maximum(ref["prim"], 0)]).sum())
        fig["negative_zero"] = int(np.signbit(d[:, axis]).sum())
    print(what, fig)
    # ---- the conditions on the inputs
    assert fig["hits"] >= need_hits and fig["misses"] >= need_misses and fig.get("straddling", 0) >= need_straddling, (what, fig)
    # ---- 1. every ray against the brute force
    rays = capi.make_rays(o, d, TMIN, TMAX)
    for label, ctx, knobs in (("rtgo_set_scene", B.ctx, {"RTGO_TRACE_MODE": None}), ("RTGO_TRACE_MODE=0", B.ctx, {"RTGO_TRACE_MODE": 0}),
                              ("RTGO_TRACE_MODE=1", B.ctx, {"RTGO_TRACE_MODE": 1}), ("rtgo_set_large_scene", B.big, {"RTGO_TRACE_MODE": None})):
        with Knob(**dict(B.env, **knobs)):
            got = ctx.trace_rays(rays)
        bad = np.flatnonzero((bits(got).reshape(-1, 8) != bits(ref).reshape(-1, 8)).any(1))
        assert len(bad) == 0, "%s, %s: %d of %d rays differ from the brute force, first %r against %r" % (what, label, len(bad), len(o), got[bad[:3]], ref[bad[:3]])
    # ---- 2. the canonical frame against the oracle
    canon = {}
    for mode, (path, amb) in MODES.items():
        canon[mode] = launch(capi, B, B.ctx, w, h, 2, mode, {}, stats=True)
        assert canon[mode][4] & CANON
        racc, rimg, _ = oracle.render(B.sc, oracle.frame(w, h, 2, 0, path=path, ambient=amb, mode=1))
        assert_parity(canon[mode][0], racc, canon[mode][1], rimg, what="%s, canonical frame, %s" % (what, mode))
    # ---- 3. every pinned fast launch against the canonical frame
    for name, knobs, ctx, modes, proof in pins_of(B):
        took = []
        for mode in modes:
            got = launch(capi, B, ctx, w, h, 2, mode, knobs)
            same_frame(got, canon[mode], "%s, %s, %s" % (what, name, mode))
            took.append(got[4])
        assert all(proof(v) for v in took), "%s, %s: last_variant %s: the launch did not take the pinned walk" % (what, name, [hex(v) for v in took])
    for mode in ("path", "distributed"):
        three = launch(capi, B, B.ctx, w, h, 2, mode, {}, frames=(0, 1, 2), stats=True)
        got = launch(capi, B, B.ctx, w, h, 2, mode, {"RTGO_TREE": 0}, batched=3)
        same_frame(got, three, "%s, rtgo_launch_frames of 3 frames, %s" % (what, mode))
        assert got[4] & BATCH and not got[4] & CANON, "%s: rtgo_launch_frames took %s" % (what, hex(got[4]))
    # ---- 4. rtgo_shade_rays over the launch's own rays and seeds
    for mode, (path, amb) in MODES.items():
        want = launch(capi, B, B.ctx, w, h, 1, mode, {})
        s0 = B.ctx.stats()
        with Knob(**B.env):
            acc, img = B.ctx.shade_rays(rays, seed, path, amb, 5, 0)
        s1 = B.ctx.stats()
        got = (acc.reshape(h, w, 4), img.reshape(h, w, 4), s1["rays_total"] - s0["rays_total"], s1["rays_occlusion"] - s0["rays_occlusion"])
        same_frame(got, want, "%s, rtgo_shade_rays, %s" % (what, mode))
    return fig


# ---- cornell: the planes of its geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,c,eye_ab,w_ab,misses", A.CORNELL_PLANES, ids=lambda v: str(v))
def test_cornell_planes_of_its_geometry(capi, oracle, bundles, axis, c, eye_ab, w_ab, misses):
    B = bundles("cornell")
    assert B.ctx.stats()["cuboid_groups"] == 3
    check_case(capi, oracle, B, A.in_plane(axis, c, eye_ab, w_ab), W, H, "cornell, axis %d = %g" % (axis, c), plane=(axis, c),
               need_hits=100, need_misses=misses)


def test_cornell_one_ray_along_the_floor_and_left_wall_edge(capi, oracle, bundles):
    """into the back wall's corner, two direction components exactly zero (cornell's boxes are turned: none has an axis-parallel side)"""
    check_case(capi, oracle, bundles("cornell"), A.one_ray((-4.0, -4.0, 3.0), (0.0, 0.0, -1.0)), W1, H1, "cornell, one ray along the floor / left wall edge")


# ---- a room with two axis-aligned boxes: the six face planes of each ------------------------------------------------------------------------
# primitive (a face of box a: 7 .. 12, of box b: 13 .. 18) -> (eye_ab, w_ab): the eye beside the box, looking at it along the face's plane
ROOM_FACES = {7: ((0.3, 1.0), (-0.93, -0.17)), 8: ((-4.7, 1.0), (1.03, -0.17)), 9: ((-2.0, 3.0), (-0.15, -0.95)), 10: ((-2.0, 3.0), (-0.15, -0.95)),
              11: ((0.3, -2.0), (-0.93, -0.17)), 12: ((-4.7, -2.0), (1.03, -0.17)), 13: ((4.5, -0.5), (-0.93, -0.17)), 14: ((2.5, -3.5), (-0.15, 1.01)),
              15: ((-2.5, 1.5), (-0.15, -0.95)), 16: ((-2.5, 1.5), (-0.15, -0.95)), 17: ((4.5, -2.5), (-0.93, -0.17)), 18: ((4.5, -2.5), (-0.93, -0.17))}


@pytest.mark.parametrize("face", sorted(ROOM_FACES))
def test_room_with_two_axis_aligned_boxes(capi, oracle, bundles, face):
    B = bundles("room")
    assert B.ctx.stats()["cuboid_groups"] == 3       # the room and both boxes are certified
    M = B.t["M"][face].reshape(4, 4)
    axis = int(np.argmax(np.abs(M[:3, 1])))          # the face's normal is the image of the unit rectangle's y axis
    c = M[axis, 3]
    assert np.count_nonzero(np.abs(M[:3, 1]) > 1e-6) == 1, "the boxes are axis-aligned"
    eye_ab, w_ab = ROOM_FACES[face]
    check_case(capi, oracle, B, A.in_plane(axis, c, eye_ab, w_ab), W, H, "room, face %d: axis %d = %r" % (face, axis, float(c)), plane=(axis, c), need_hits=100)


def test_room_one_ray_down_a_box_s_vertical_edge(capi, oracle, bundles):
    """box b spans x 1 .. 3, z -2 .. 0: from under the ceiling straight down the edge x = 3, z = 0, onto the top face's corner"""
    B = bundles("room")
    x, z = B.t["M"][15].reshape(4, 4)[0, 3], B.t["M"][17].reshape(4, 4)[2, 3]
    assert (x, z) == (3.0, 0.0)
    check_case(capi, oracle, B, A.one_ray((x, 3.5, z), (0.0, -1.0, 0.0)), W1, H1, "room, one ray down box b's edge")


# ---- structure planes: faces of the boxes of tree 0, tree 1 and the canonical nodes ---------------------------------------------------------
# (scene, structure, axis) -> (c, eye_ab, w_ab): per structure and axis the plane of adversarial_cameras.planes() that the most tight boxes
# straddle among those on which the oracle can meet the conditions (PASSED_OVER: the planes with more that cannot, and why), and an eye
# from which it does.  cornell's second structure has no tree (everything is up front) and checkered's is its first: no tree-1 planes there.
STRUCTURE_PLANES = {
    ("cornell", "tree0", 0): (-0.06703925132751465, (0.4, 0.8), (0.35, 0.15)),
    ("cornell", "tree0", 1): (-1.9989899396896362, (0.7, 3.3), (0.35, 0.15)),
    ("cornell", "tree0", 2): (-0.06703925132751465, (0.4, 0.8), (0.35, 0.15)),
    ("cornell", "nodes", 0): (-1.9330509901046753, (0.4, 0.8), (0.35, 0.15)),
    ("cornell", "nodes", 1): (-2.999000072479248, (0.7, 3.3), (0.35, 0.15)),
    ("cornell", "nodes", 2): (-1.9330509901046753, (0.4, 0.8), (0.35, 0.15)),
    ("checkered", "tree0", 0): (-2.001009941101074, (-0.5, 1.6), (0.35, 0.15)),
    ("checkered", "tree0", 1): (-3.9936957359313965, (0.8, 1.6), (0.35, 0.15)),
    ("checkered", "tree0", 2): (-2.001009941101074, (0.8, 0.0), (0.35, 0.15)),
    ("checkered", "nodes", 0): (-0.0010000000474974513, (-0.5, 1.6), (0.35, 0.15)),
    ("checkered", "nodes", 1): (-3.9937055110931396, (0.8, 1.6), (0.35, 0.15)),
    ("checkered", "nodes", 2): (-0.0010000000474974513, (0.8, 0.0), (0.35, 0.15)),
    ("random1", "tree0", 0): (-0.3062397241592407, (0.23, 1.4), (-0.35, -0.15)),
    ("random1", "tree1", 0): (-0.3062397241592407, (0.23, 1.4), (-0.35, -0.15)),
    ("random1", "nodes", 0): (0.6087414622306824, (0.23, 1.4), (-0.35, -0.15)),
    ("random1", "tree0", 1): (1.5257302522659302, (0.7, 1.4), (0.35, 0.15)),
    ("random1", "tree1", 1): (1.5257302522659302, (0.7, 1.4), (0.35, 0.15)),
    ("random1", "nodes", 1): (1.5447590351104736, (0.7, 1.4), (0.35, 0.15)),
    ("random1", "tree0", 2): (0.33003443479537964, (0.7, 0.79), (-0.35, -0.15)),
    ("random1", "tree1", 2): (0.35923564434051514, (0.7, 0.79), (-0.35, -0.15)),
    ("random1", "nodes", 2): (0.34030407667160034, (0.7, 0.79), (-0.35, -0.15)),
}
# cornell, axis y: the plane with the most lies a millimetre BELOW the floor (the bottom of the floor's own padded box), outside the closed
# room: no ray in it hits anything
PASSED_OVER = {("cornell", "tree0", 1): (-4.001009941101074,), ("cornell", "nodes", 1): (-4.000999927520752,)}


@pytest.mark.parametrize("key", sorted(STRUCTURE_PLANES), ids=lambda v: "%s-%s-%d" % v)
def test_structure_planes(capi, oracle, bundles, key):
    scene, structure, axis = key
    c, eye_ab, w_ab = STRUCTURE_PLANES[key]
    B = bundles(scene)
    cand = A.planes(B.build, axis)[structure]
    c = np.float32(c)
    assert (bits(cand) == bits(c)).any(), "%r is no face of %s on axis %d" % (float(c), structure, axis)
    left = np.array([p for p in cand if float(p) not in PASSED_OVER.get(key, ())], np.float32)
    best, count = A.most_straddled(B.tight, axis, left)
    assert bits(best) == bits(c), "the plane that the most tight boxes straddle is %r (%d boxes)" % (float(best), count)
    check_case(capi, oracle, B, A.in_plane(axis, c, eye_ab, w_ab), W, H, "%s, %s, axis %d = %r (%d tight boxes straddle it)" % (scene, structure, axis, float(c), count),
               plane=(axis, c), need_hits=100, need_straddling=50)


# ---- grid planes: the grid's bounds and the cell plane that the most tight boxes straddle ---------------------------------------------------
# per scene and axis the eye within the plane (eye_ab, w_ab).  W carries -0.0 on the axis: the component is -0 where both pixel offsets
# are negative and +0 elsewhere, so every frame holds both signs (rcp(-0) steps the other way).
GRID_EYES = {"balls": {0: ((0.4, 1.6), (0.35, 0.15)), 1: ((0.8, 1.6), (0.35, 0.15)), 2: ((0.8, 0.8), (0.35, 0.15))},
             "boxes49": {0: ((0.4, 1.2), (-0.35, -0.15)), 1: ((0.6, 1.2), (-0.35, -0.15)), 2: ((0.6, 0.9), (0.35, 0.15))},
             "boxes122": {0: ((0.4, 1.2), (-0.35, -0.15)), 1: ((0.6, 1.2), (-0.35, -0.15)), 2: ((0.6, 0.9), (0.35, 0.15))}}


def grid_plane(B, axis, kind):
    g = A.planes(B.build, axis)["grid"]
    assert B.has_grid and len(g) >= 3, "%s has no grid" % B.name
    return {"lower": g[0], "upper": g[-1], "cell": A.most_straddled(B.tight, axis, g[1:-1])[0]}[kind]


@pytest.mark.parametrize("kind", ["lower", "upper", "cell"])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("scene", sorted(GRID_EYES))
def test_grid_planes(capi, oracle, bundles, scene, axis, kind):
    B = bundles(scene)
    c = grid_plane(B, axis, kind)
    eye_ab, w_ab = GRID_EYES[scene][axis]
    fig = check_case(capi, oracle, B, A.in_plane(axis, c, eye_ab, w_ab, zero=-0.0), W, H, "%s, grid %s plane, axis %d = %r" % (scene, kind, axis, float(c)),
                     plane=(axis, c), need_hits=100, need_straddling=50)
    assert 0 < fig["negative_zero"] < fig["rays"], "both signs of the zero component"


@pytest.mark.parametrize("scene", ["balls", "boxes49"])
def test_grid_one_ray_along_the_line_where_two_cell_planes_meet(capi, oracle, bundles, scene):
    """straight down the line x = a cell plane, z = a cell plane: both horizontal components are zero (of either sign, by the pixel) and
    the walk's parameters to the next x and z planes tie"""
    B = bundles(scene)
    x, z = grid_plane(B, 0, "cell"), grid_plane(B, 2, "cell")
    check_case(capi, oracle, B, A.one_ray((x, 3.5, z), (-0.0, -1.0, -0.0)), W1, H1, "%s, one ray down the line x = %r, z = %r" % (scene, float(x), float(z)))
