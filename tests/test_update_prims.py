"""rtgo_update_prims on the MI355X: some primitives of the analytic scene edited in place.

Every comparison is against a second context given the edited array through the set call.  A scene of rtgo_set_scene afterwards holds what
that context holds, digest for digest over the spans of rtgo_debug_build_digest, and so renders and answers rays the same, bit for bit.
A scene of rtgo_set_large_scene is refitted -- the old topology with boxes that close over the new leaves, checked node by node here,
since tests/accel_check.check_analytic knows the structures of rtgo_set_scene only -- or rebuilt to the arrays of a fresh build; either way
frames, ray queries and ray counts are the fresh context's.  Then continuity across an update, and the refusals, which leave digests,
frames and every field of rtgo_stats as they were.  (The refusal of a rebuilt tree deeper than the walk's stack has no input here, as the
set call's has none in tests/test_large_scenes.py.)"""
import ctypes as C

import numpy as np
import pytest

import accel_check
import shade_rays_ref as R
import shading_scenes as SC
import test_large_scenes as TL
import test_oracle_shading_float64 as T
from test_trace_rays import Knob

pytestmark = pytest.mark.gpu

RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE, RTGO_E_UNSUPPORTED = 0, 1, 3, 4
TMIN, TMAX = R.T_MIN0, R.T_MAX0
# what pins the walk the issue names for a scene (tests/test_shade_rays.py's knobs): cornell's two-leaf walk (last_variant bit 8), balls' grid (bit 4)
PIN = {"cornell": ({"RTGO_MAX_WPE": 6, "RTGO_TREE": 0}, 256), "balls": ({"RTGO_TREE": 2}, 16)}
CERT = 64   # last_variant bit 6: path mode under the last-ray certificate


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_tables = {}


def tables(oracle, name):
    """(tables, width, height): the shading scenes at 48 x 36 (set without boxes), cornell and balls at 64 x 48 (with the reference's boxes)"""
    if name not in _tables:
        if name in SC.SCENES:
            _tables[name] = (SC.SCENES[name](48 / 36), 48, 36)
        else:
            _tables[name] = (oracle.scene_tables(oracle.scene(name, 64, 48)), 64, 48)
    return _tables[name]


def edit(oracle, t, idx, types=None, M=None, mat=None, pad=None):
    """t with primitives idx replaced (None: kept); boxes, where t has them, by the CubeBox rule (+ pad [k, 6]) for the new matrices"""
    out = dict(t)
    idx = np.asarray(idx)
    for key, new in (("type", types), ("M", M), ("mat", mat)):
        out[key] = t[key].copy()
        if new is not None:
            out[key][idx] = np.asarray(new, out[key].dtype).reshape((len(idx),) + out[key].shape[1:])
    if t.get("aabb") is not None:
        out["aabb"] = t["aabb"].copy()
        if M is not None:
            out["aabb"][idx] = TL.oracle_boxes(oracle, out["M"][idx]) + (0 if pad is None else pad)
    return out


def moved(M, d):
    M = np.array(M, np.float32).reshape(-1, 16).copy()
    M[:, [3, 7, 11]] += np.asarray(d, np.float32)
    return M


def set_scene(ctx, t, large, pixels=None):
    (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t.get("aabb"))
    c = t["cam"]
    ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    if pixels:
        ctx.resize(pixels)
    return ctx


def update(ctx, t_new, idx, rebuild=False):
    """primitives idx of ctx's scene become t_new's"""
    idx = np.asarray(idx)
    ctx.update_prims(idx, t_new["type"][idx], t_new["M"][idx], t_new["mat"][idx], None if t_new.get("aabb") is None else t_new["aabb"][idx], rebuild)


def answers(capi, ctx, t, w, h, name=None, frames=(0, 1)):
    """what the contract names, over ctx: per mode the buffers and ray-count deltas after each frame; a window of bands with collect_stats 1
    and a frame with collect_stats 2; rtgo_trace_rays' hits and rtgo_shade_rays' buffers over frame 0's rays; the scene's stats"""
    out = {}
    knobs, bit = PIN.get(name, ({}, 0))
    with Knob(**knobs):
        for mode, (path, amb) in T.MODES.items():
            for f in frames:
                s0 = ctx.stats()
                ctx.launch(capi.make_frame(w, h, 1, f, path, amb, bands=(1, 1, 0)))
                ctx.sync()
                s1 = ctx.stats()
                out["%s frame %d" % (mode, f)] = (ctx.read_accum(h, w).copy(), ctx.read_image(h, w).copy(), s1["rays_total"] - s0["rays_total"],
                                                  s1["rays_occlusion"] - s0["rays_occlusion"])
                if bit:   # (pinned: the launch-time trial has no say in either)
                    out["%s frame %d walk" % (mode, f)] = s1["last_variant"] & bit
                    out["%s frame %d certificate" % (mode, f)] = s1["last_variant"] & CERT
        for stats, window, bands in ((1, (8, 4, w - 16, h - 8), (4, 2, 1)), (2, None, (1, 1, 0))):
            x0, y0, ww, hh = window or (0, 0, w, h)
            rows = capi.local_rows(hh, *bands)
            s0 = ctx.stats()
            ctx.launch(capi.make_frame(w, h, 1, 0, True, False, window, bands, stats=stats))
            ctx.sync()
            s1 = ctx.stats()
            out["collect_stats %d" % stats] = (ctx.read_accum(rows, ww).copy(), ctx.read_image(rows, ww).copy(), s1["rays_total"] - s0["rays_total"],
                                               s1["rays_occlusion"] - s0["rays_occlusion"])
    o, d, seed = R.raygen32(t["cam"], w, h, 0)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    out["trace_rays"] = (ctx.trace_rays(rays).view(np.uint32).copy(),)
    out["trace_rays any"] = (ctx.trace_rays(rays, capi.TRACE_ANY_HIT)["prim"].copy(),)
    out["shade_rays"] = ctx.shade_rays(rays, seed, True, False, 5, 0)
    s = ctx.stats()
    out["scene stats"] = (s["cuboid_groups"], s["lbvh_depth"], s["guard_reach"], s["guard_quadric"])
    return out


def assert_same_answers(got, want, what):
    assert list(got) == list(want)
    for key in want:
        g, x = got[key], want[key]
        if not isinstance(x, tuple):
            assert g == x, "%s, %s: %r against %r" % (what, key, g, x)
            continue
        for k, (a, b) in enumerate(zip(g, x)):
            if isinstance(b, np.ndarray):
                assert np.array_equal(bits(a), bits(b)), "%s, %s [%d]: differs at %d words" % (what, key, k, (bits(a) != bits(b)).sum())
            else:
                assert a == b, "%s, %s [%d]: %r against %r" % (what, key, k, a, b)


def same_digests(a, b, what):
    da, db = a.build_digest(False), b.build_digest(False)
    names = list(a.read_build(False))
    assert len(da) == len(db) == len(names)
    bad = [n for n, x, y in zip(names, da, db) if x != y]
    assert not bad, "%s: spans %s differ" % (what, bad)


# ---- 1. scenes of rtgo_set_scene ---------------------------------------------------------------------------------------------------------
def lds_edits(oracle, name, t):
    """[(what, [(indices, edited tables), ...])]: each entry one or more updates in turn, each checked"""
    n = len(t["type"])
    dark = lambda idx: np.concatenate([t["mat"][idx, :7], np.zeros((len(idx), 3), np.float32)], 1)
    recolour = lambda idx: t["mat"][idx] * np.array([0.5, 1, 0.25, 1, 1, 1, 1, 1, 1, 1], np.float32)
    emitters = np.flatnonzero(t["mat"][:, 7] > 0.01)
    every = np.arange(n)
    if name == "cornell":   # 0-5 the room, 6-11 the short box, 12-17 the tall box, 18 the lamp
        box = np.arange(6, 12)
        t_off = edit(oracle, t, emitters, mat=dark(emitters))
        return [("the short box moved", [(box, edit(oracle, t, box, M=moved(t["M"][box], (-0.6, 0.0, 0.9))))]),
                ("a wall's material", [([2], edit(oracle, t, [2], mat=recolour([2])))]),
                ("the emitter off and on", [(emitters, t_off), (emitters, t)]),
                ("a face becomes a disk", [([11], edit(oracle, t, [11], types=[SC.DISK]))]),
                ("every primitive", [(every, edit(oracle, t, every, M=moved(t["M"], (0.05, 0.0, -0.05)), mat=recolour(every)))])]
    if name == "balls":
        ball = int(np.flatnonzero(t["type"] == SC.SPHERE)[7])
        return [("one sphere moved", [([ball], edit(oracle, t, [ball], M=moved(t["M"][ball], (0.3, 0.4, -0.2))))]),
                ("every primitive", [(every, edit(oracle, t, every, mat=recolour(every)))])]
    if name == "room":      # 0-5 the room, 6 the emitter, 7-12 and 13-18 the boxes, 19 the disk
        box = np.arange(7, 13)
        return [("a box moved", [(box, edit(oracle, t, box, M=moved(t["M"][box], (0.5, 0.0, 0.7))))]),
                ("the emitter off and on", [(emitters, edit(oracle, t, emitters, mat=dark(emitters))), (emitters, t)]),
                ("the disk becomes a rectangle", [([19], edit(oracle, t, [19], types=[SC.RECTANGLE], mat=[SC.GLOSSY]))])]
    assert name == "quadrics"   # 0 the floor, 1 and 3 spheres, 2 a cylinder
    return [("a sphere moved", [([3], edit(oracle, t, [3], M=moved(t["M"][3], (-0.8, 0.4, 0.3))))]),
            ("a sphere becomes a cylinder, the cylinder a sphere", [([1, 2], edit(oracle, t, [1, 2], types=[SC.CYLINDER, SC.SPHERE]))]),
            ("every primitive", [(every, edit(oracle, t, every, mat=recolour(every)))])]


# (both flags take one path over a scene of rtgo_set_scene: the second flag goes through each scene's first edit)
LDS_CASES = [(name, k, False) for name, count in (("cornell", 5), ("balls", 2), ("room", 3), ("quadrics", 3)) for k in range(count)] + \
            [(name, 0, True) for name in ("cornell", "balls", "room", "quadrics")]


@pytest.mark.parametrize("name,case,rebuild", LDS_CASES, ids=lambda v: str(v))
def test_resident_scene_holds_what_a_fresh_set_holds(capi, oracle, name, case, rebuild):
    t, w, h = tables(oracle, name)
    what, steps = lds_edits(oracle, name, t)[case]
    ctx, fresh = set_scene(capi.Context(0), t, False, w * h), capi.Context(0)
    ctx.launch(capi.make_frame(w, h, 1, 0, True, False))   # (a mask, seeds and a trial to drop)
    ctx.launch(capi.make_frame(w, h, 1, 1, True, False))
    for k, (idx, t_new) in enumerate(steps):
        update(ctx, t_new, idx, rebuild)
        set_scene(fresh, t_new, False, w * h)
        label = "%s: %s, step %d" % (name, what, k)
        same_digests(ctx, fresh, label)
        got, want = answers(capi, ctx, t_new, w, h, name), answers(capi, fresh, t_new, w, h, name)
        assert_same_answers(got, want, label)
        if name in PIN and case < 2:   # (these edits keep what the walk needs: the comparison above covered a launch that took it)
            walks = {key: v for key, v in want.items() if key.endswith("walk")}
            print(label, "last_variant & %d:" % PIN[name][1], walks)
            assert any(walks.values()), "%s: no launch of the fresh context took the walk the knobs pin" % label
        v = accel_check.check_analytic(ctx.read_build(False), t_new["type"], t_new["M"], t_new.get("aabb"))
        assert not v, "%s: %s" % (label, list(v)[:5])
        if name == "cornell" and case == 2:   # the last-ray certificate follows the emitter: gone with it (step 0), back with it (step 1)
            assert [got["path frame %d certificate" % f] for f in (0, 1)] == [CERT * k] * 2, label
    ctx.close()
    fresh.close()


def test_resident_scene_without_boxes(capi, oracle):
    """cornell set without boxes: an update brings none either, and the device's CubeBox boxes follow the edit"""
    t, w, h = tables(oracle, "cornell")
    t = {k: v for k, v in t.items() if k != "aabb"}
    box = np.arange(12, 18)
    t_new = edit(oracle, t, box, M=moved(t["M"][box], (0.4, 0.0, 0.5)))
    ctx, fresh = set_scene(capi.Context(0), t, False, w * h), set_scene(capi.Context(0), t_new, False, w * h)
    update(ctx, t_new, box)
    same_digests(ctx, fresh, "cornell without boxes")
    assert_same_answers(answers(capi, ctx, t_new, w, h, "cornell"), answers(capi, fresh, t_new, w, h, "cornell"), "cornell without boxes")
    ctx.close()
    fresh.close()


# ---- 2. scenes of rtgo_set_large_scene ---------------------------------------------------------------------------------------------------
LW, LH = 48, 36


def large_scene(oracle, n, seed, with_aabbs):
    """n primitives of all four types in view of a camera, under one drawable light; n = 300: spheres at the centroids of accel_check.sphere300's
    triangles"""
    if n == 300:
        m = accel_check.sphere300()
        c = m["positions"][m["indices"].reshape(-1, 3)].mean(axis=1)
        c = (c - c.mean(axis=0)) * np.float32(3.0 / np.abs(c - c.mean(axis=0)).max())
        types = np.full(n, SC.SPHERE, np.uint32)
        M = np.stack([SC.model(c[i], np.eye(3), 0.18 + 0.001 * (i % 7)) for i in range(n)])
        mat = TL.random_scene(n, seed)[2]
    else:
        types, M, mat = TL.random_scene(n, seed, spread=3.0)
    L = SC.flat((0.5, 9.0, 2.0), (0, -1, 0), 2.0)
    t = {"type": types.astype(np.int32), "M": M.astype(np.float32), "mat": mat, "lights": np.array([SC.light_record(L, 0.05)] * 2, np.float32),
         "cam": SC.camera((0.5, 1.0, 13.0), (0, 0, 0), (0, 1, 0), 40.0, LW / LH), "bg": np.array((0.3, 0.4, 0.6), np.float32)}
    if with_aabbs:   # boxes of the caller's own, larger than the CubeBox rule's by a different pad per primitive
        t["aabb"] = TL.oracle_boxes(oracle, t["M"]) + box_pad(n, seed + 1)
    return t


def box_pad(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 0.25, size=(n, 6)).astype(np.float32) * np.array([-1, -1, -1, 1, 1, 1], np.float32)


def large_edit(oracle, t, idx, seed):
    """primitives idx replaced by others: type, matrix and material"""
    types, M, mat = TL.random_scene(len(idx), seed, spread=3.0)
    return edit(oracle, t, idx, types=types, M=M, mat=mat, pad=box_pad(len(idx), seed + 1) if t.get("aabb") is not None else None)


def closure_violations(boxes, links, aabb):
    """the refitted tree, node by node: a leaf's box is its primitive's, an internal node's the exact min / max of its children's; every
    primitive in one leaf"""
    out = []
    leaf = links[:, 1] < 0
    prim = links[leaf, 0]
    if sorted(prim.tolist()) != list(range(len(aabb))):
        out.append("the leaves do not hold every primitive once")
    if not np.array_equal(bits(boxes[leaf]), bits(aabb[prim])):
        out.append("a leaf's box is not its primitive's")
    inner = np.flatnonzero(~leaf)
    l, r = links[inner, 0], links[inner, 1]
    want = np.concatenate([np.minimum(boxes[l, :3], boxes[r, :3]), np.maximum(boxes[l, 3:], boxes[r, 3:])], 1)
    if not np.array_equal(bits(boxes[inner]), bits(want)):
        out.append("%d internal boxes are not the union of their children's" % (bits(boxes[inner]) != bits(want)).any(1).sum())
    return out


@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("n", [1, 2, 3, 257, 300, 513])
def test_large_scene_first_last_all(capi, oracle, n, rebuild, with_aabbs):
    t = large_scene(oracle, n, 100 + n, with_aabbs)
    ctx, fresh = capi.Context(0), capi.Context(0)
    for what, idx in (("the first", [0]), ("the last", [n - 1]), ("all", np.arange(n)[::-1])):
        set_scene(ctx, t, True, LW * LH)
        _, links0, _, _ = ctx.read_bvh()
        depth0 = ctx.stats()["lbvh_depth"]
        ctx.launch(capi.make_frame(LW, LH, 1, 0, True, False))   # (a mask and seeds over the old bounds)
        t_new = large_edit(oracle, t, idx, 7 * n + len(idx))
        update(ctx, t_new, idx, rebuild)
        set_scene(fresh, t_new, True, LW * LH)
        label = "n %d, %s, %s" % (n, what, "rebuild" if rebuild else "refit")
        boxes, links, inv, aabb = ctx.read_bvh()
        fboxes, flinks, finv, faabb = fresh.read_bvh()
        assert np.array_equal(bits(inv), bits(finv)) and np.array_equal(bits(aabb), bits(faabb)), label + ": records or boxes"
        if t_new.get("aabb") is not None:
            assert np.array_equal(bits(aabb), bits(t_new["aabb"])), label
        if rebuild:
            assert np.array_equal(links, flinks) and np.array_equal(bits(boxes), bits(fboxes)), label + ": nodes"
            assert ctx.stats()["lbvh_depth"] == fresh.stats()["lbvh_depth"]
            same_digests(ctx, fresh, label)
        else:
            assert np.array_equal(links, links0), label + ": the topology moved"
            assert not closure_violations(boxes, links, aabb), label
            assert np.array_equal(bits(boxes[0]), bits(fboxes[0])), label + ": root box"
            assert ctx.stats()["lbvh_depth"] == depth0
        got, want = answers(capi, ctx, t_new, LW, LH), answers(capi, fresh, t_new, LW, LH)
        if not rebuild:   # (the refitted tree keeps its depth; everything else of the scene's stats is the fresh context's)
            got["scene stats"] = (got["scene stats"][0], want["scene stats"][1]) + got["scene stats"][2:]
        assert_same_answers(got, want, label)
        assert (want["trace_rays any"][0] >= 0).any() or n < 4, label + ": the view sees nothing"
    ctx.close()
    fresh.close()


def compact_scene(oracle, n=257):
    """n small spheres in a ball of radius 1.5 about the origin, far smaller than the frame; boxes by the CubeBox rule on the device"""
    rng = np.random.default_rng(5)
    c = rng.normal(size=(n, 3))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * rng.uniform(0.2, 1.5, size=(n, 1))
    t = large_scene(oracle, n, 3, False)
    t["type"][:] = SC.SPHERE
    t["M"] = np.stack([SC.model(c[i], np.eye(3), 0.12) for i in range(n)])
    return t


def test_a_primitive_moved_outside_the_old_bounds_shows(capi, oracle):
    t = compact_scene(oracle)
    ctx = set_scene(capi.Context(0), t, True, LW * LH)
    f0 = capi.make_frame(LW, LH, 1, 0, True, False, bands=(1, 1, 0))
    ctx.reset_stats()
    ctx.launch(f0)
    ctx.sync()
    assert ctx.stats()["rays_culled"] > 0, "the old screen rectangle culls nothing: the case shows nothing"
    o, d, _ = R.raygen32(t["cam"], LW, LH, 0)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    before = ctx.trace_rays(rays)["prim"].reshape(LH, LW)
    t_new = edit(oracle, t, [0], M=[SC.model((3.0, 4.0, 0.0), np.eye(3), 0.7)])
    for rebuild in (False, True):
        set_scene(ctx, t, True, LW * LH)
        ctx.launch(f0)
        update(ctx, t_new, [0], rebuild)
        ctx.launch(f0)
        ctx.sync()
        acc = ctx.read_accum(LH, LW).copy()
        fresh = set_scene(capi.Context(0), t_new, True, LW * LH)
        fresh.launch(f0)
        fresh.sync()
        assert np.array_equal(bits(acc), bits(fresh.read_accum(LH, LW))), rebuild
        after = ctx.trace_rays(rays)["prim"].reshape(LH, LW)
        cols, rows = np.flatnonzero((before >= 0).any(axis=0)), np.flatnonzero((before >= 0).any(axis=1))
        y, x = np.mgrid[0:LH, 0:LW]
        new = (after == 0) & ((x > cols.max() + 3) | (y > rows.max() + 3))   # beyond the old rectangle and its pad
        assert new.sum() > 10, "the moved sphere does not reach beyond the old rectangle"
        bg = np.broadcast_to(t["bg"], (LH, LW, 3))
        assert (acc[new][:, :3] != bg[new]).any(axis=1).all(), "pixels of the moved sphere were answered as background"
        fresh.close()
    ctx.close()


@pytest.mark.parametrize("large", [False, True], ids=["resident", "large"])
def test_a_primitive_moved_inwards_shrinks_the_guard(capi, oracle, large):
    """(launches over a scene of rtgo_set_large_scene report no guard quantities: there the equality is of zeros, and of the pixels)"""
    t_in = compact_scene(oracle)
    t_out = edit(oracle, t_in, [5], M=[SC.model((40.0, -30.0, -60.0), np.eye(3), 0.5)])
    f0 = capi.make_frame(LW, LH, 1, 0, True, False)
    fresh = set_scene(capi.Context(0), t_in, large, LW * LH)
    fresh.launch(f0)
    want = fresh.stats()
    ctx = set_scene(capi.Context(0), t_out, large, LW * LH)
    ctx.launch(f0)
    far = ctx.stats()
    print("guard_reach / guard_quadric with the far sphere", far["guard_reach"], far["guard_quadric"], "and without", want["guard_reach"], want["guard_quadric"])
    assert large or (far["guard_reach"] > want["guard_reach"] and far["guard_quadric"] > want["guard_quadric"])
    update(ctx, t_in, [5])
    ctx.launch(f0)
    got = ctx.stats()
    assert got["guard_reach"] == want["guard_reach"] and got["guard_quadric"] == want["guard_quadric"]
    assert np.array_equal(bits(ctx.read_accum(LH, LW)), bits(fresh.read_accum(LH, LW)))
    ctx.close()
    fresh.close()


@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
def test_a_material_only_refit_leaves_the_nodes(capi, oracle, with_aabbs):
    t = large_scene(oracle, 257, 11, with_aabbs)
    ctx = set_scene(capi.Context(0), t, True, LW * LH)
    before = ctx.read_build(False)
    idx = np.array([0, 100, 256])
    t_new = edit(oracle, t, idx, mat=t["mat"][idx][:, ::-1].copy())
    update(ctx, t_new, idx)
    after = ctx.read_build(False)
    assert np.array_equal(bits(before["nodes"]), bits(after["nodes"])) and np.array_equal(bits(before["aabb"]), bits(after["aabb"]))
    assert not np.array_equal(bits(before["prims"]), bits(after["prims"]))
    fresh = set_scene(capi.Context(0), t_new, True, LW * LH)
    same_digests(ctx, fresh, "material-only refit")   # (nothing moved: the refit is the fresh build)
    assert_same_answers(answers(capi, ctx, t_new, LW, LH), answers(capi, fresh, t_new, LW, LH), "material-only refit")
    ctx.close()
    fresh.close()


# ---- 3. continuity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["resident", "refit", "rebuild"])
def test_accumulation_goes_on_across_an_update(capi, oracle, kind):
    if kind == "resident":
        t, w, h = tables(oracle, "cornell")
        idx = np.arange(6, 12)
        t_new = edit(oracle, t, idx, M=moved(t["M"][idx], (-0.6, 0.0, 0.9)))
    else:
        t, w, h = large_scene(oracle, 257, 21, True), LW, LH
        idx = np.arange(0, 257, 5)
        t_new = large_edit(oracle, t, idx, 22)
    large = kind != "resident"
    for mode, (path, amb) in T.MODES.items():
        ctx = set_scene(capi.Context(0), t, large, w * h)
        ctx.launch(capi.make_frame(w, h, 1, 0, path, amb))
        ctx.sync()
        first = ctx.read_accum(h, w).copy()
        update(ctx, t_new, idx, kind == "rebuild")
        ctx.launch(capi.make_frame(w, h, 1, 1, path, amb))
        ctx.sync()
        fresh = set_scene(capi.Context(0), t_new, large, w * h)
        fresh.write_accum(first)
        fresh.launch(capi.make_frame(w, h, 1, 1, path, amb))
        fresh.sync()
        assert np.array_equal(bits(ctx.read_accum(h, w)), bits(fresh.read_accum(h, w))), (kind, mode)
        assert np.array_equal(ctx.read_image(h, w), fresh.read_image(h, w)), (kind, mode)
        assert not np.array_equal(bits(first), bits(fresh.read_accum(h, w)))
        ctx.close()
        fresh.close()


@pytest.mark.parametrize("kind", ["resident", "refit", "rebuild"])
def test_three_updates_in_a_row_are_one_set_call(capi, oracle, kind):
    if kind == "resident":
        t, w, h = tables(oracle, "room")
        steps = [np.arange(7, 13), np.array([19, 6]), np.array([0, 8, 14])]
    else:
        t, w, h = large_scene(oracle, 513, 31, False), LW, LH
        steps = [np.array([0, 512]), np.arange(100, 300), np.array([512, 7, 150])]   # (overlapping: the later edit stands)
    large = kind != "resident"
    ctx = set_scene(capi.Context(0), t, large, w * h)
    t_new = t
    for k, idx in enumerate(steps):
        if large:
            t_new = large_edit(oracle, t_new, idx, 40 + k)
        else:
            t_new = edit(oracle, t_new, idx, M=moved(t_new["M"][idx], (0.1 * (k + 1), 0.0, -0.15)), mat=t_new["mat"][idx] * np.float32(0.75))
        update(ctx, t_new, idx, kind == "rebuild")
    fresh = set_scene(capi.Context(0), t_new, large, w * h)
    if kind != "refit":
        same_digests(ctx, fresh, kind)
    else:
        boxes, links, inv, aabb = ctx.read_bvh()
        assert not closure_violations(boxes, links, aabb)
        assert np.array_equal(bits(boxes[0]), bits(fresh.read_bvh()[0][0]))
    got, want = answers(capi, ctx, t_new, w, h), answers(capi, fresh, t_new, w, h)
    if kind == "refit":
        got["scene stats"] = (got["scene stats"][0], want["scene stats"][1]) + got["scene stats"][2:]
    assert_same_answers(got, want, kind)
    ctx.close()
    fresh.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def raw(capi, ctx, idx, prims, aabbs, n, flags=0):
    """the bare C call; idx / prims / aabbs: numpy arrays or None"""
    p = lambda a, ty: None if a is None else a.ctypes.data_as(C.POINTER(ty))
    return capi.load().rtgo_update_prims(ctx._h, p(idx, C.c_uint32), p(prims, capi.Prim), p(aabbs, capi.Aabb), n, flags)


def records(capi, t, idx):
    rec = np.zeros(len(idx), dtype=capi.PRIM_DTYPE)
    rec["type"], rec["model"] = t["type"][idx], t["M"][idx]
    m = t["mat"][idx]
    rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = m[:, 0:3], m[:, 3:6], m[:, 6], m[:, 7:10]
    return rec


@pytest.mark.parametrize("kind", ["resident", "resident without boxes", "large", "large without boxes"])
def test_refusals_leave_everything(capi, oracle, kind):
    large, boxed = kind.startswith("large"), "without" not in kind
    if large:
        t, w, h = large_scene(oracle, 257, 51, boxed), LW, LH
    else:
        t, w, h = tables(oracle, "cornell")
        t = t if boxed else {k: v for k, v in t.items() if k != "aabb"}
    n = len(t["type"])
    ctx = set_scene(capi.Context(0), t, large, w * h)
    f0 = capi.make_frame(w, h, 1, 0, True, False)
    ctx.launch(f0)
    ctx.sync()
    frame, digests, stats = ctx.read_accum(h, w).copy(), ctx.build_digest(False), ctx.stats()
    idx = np.array([1, 0], np.uint32)
    good = records(capi, t, idx)
    good["model"][:, 3] += 0.25
    box = np.ascontiguousarray(TL.oracle_boxes(oracle, good["model"]) + np.array([-1, -1, -1, 1, 1, 1], np.float32)) if boxed else None

    def bad(field, value):
        r = good.copy()
        r[field][1] = value
        return r

    empty = None if box is None else box.copy()
    if empty is not None:
        empty[1, 3] = empty[1, 0] - 1.0
    nan_box = None if box is None else box.copy()
    if nan_box is not None:
        nan_box[0, 4] = np.nan
    cases = [("unknown flag bits", (idx, good, box, 2, 2), RTGO_E_INVALID), ("a high flag bit", (idx, good, box, 2, 1 | 1 << 31), RTGO_E_INVALID),
             ("NULL indices", (None, good, box, 2), RTGO_E_INVALID), ("NULL prims", (idx, None, box, 2), RTGO_E_INVALID),
             ("boxes against the scene", (idx, good, None if boxed else np.zeros((2, 6), np.float32), 2), RTGO_E_INVALID),
             ("an index at the count", (np.array([1, n], np.uint32), good, box, 2), RTGO_E_INVALID),
             ("an index far beyond", (np.array([0xFFFFFFFF, 0], np.uint32), good, box, 2), RTGO_E_INVALID),
             ("an index named twice", (np.array([1, 1], np.uint32), good, box, 2), RTGO_E_INVALID),
             ("an unknown type", (idx, bad("type", 4), box, 2), RTGO_E_INVALID),
             ("a singular matrix", (idx, bad("model", np.zeros(16, np.float32)), box, 2), RTGO_E_INVALID),
             ("a matrix that is not finite", (idx, bad("model", np.full(16, np.inf, np.float32)), box, 2), RTGO_E_INVALID),
             ("a material that is not finite", (idx, bad("kd", np.array([np.nan, 0, 0], np.float32)), box, 2), RTGO_E_INVALID)]
    if boxed:
        cases += [("an empty box", (idx, good, empty, 2), RTGO_E_INVALID), ("a box that is not finite", (idx, good, nan_box, 2), RTGO_E_INVALID)]
    for flag in (0, 1):
        for what, args, code in cases:
            a = args if len(args) == 5 else args + (flag,)
            assert raw(capi, ctx, *a) == code, "%s: %s" % (kind, what)
            assert capi.load().rtgo_last_error(ctx._h), what
        assert raw(capi, ctx, None, None, None, 0, flag) == RTGO_OK   # no updates: nothing to check, nothing changes
        assert raw(capi, ctx, idx, good, box, 0, flag) == RTGO_OK
    assert ctx.build_digest(False) == digests, kind
    assert ctx.stats() == stats, kind
    ctx.launch(f0)
    ctx.sync()
    assert np.array_equal(bits(ctx.read_accum(h, w)), bits(frame)), kind
    # and the call as given is good: what was refused was the argument named
    assert raw(capi, ctx, idx, good, box, 2, 0) == RTGO_OK
    assert ctx.build_digest(False) != digests
    ctx.close()


def test_no_analytic_scene_is_a_state_error(capi):
    ctx = capi.Context(0)
    idx, rec = np.zeros(1, np.uint32), np.zeros(1, dtype=capi.PRIM_DTYPE)
    rec["model"][0] = np.eye(4, dtype=np.float32).reshape(16)
    assert raw(capi, ctx, idx, rec, None, 1) == RTGO_E_STATE
    assert raw(capi, ctx, None, None, None, 0) == RTGO_E_STATE
    m = accel_check.sphere300()   # a whitted scene alone does not count
    ctx.whitted_set_mesh(m["positions"], m["normals"], m["indices"], m["tri_material"], m["materials"])
    assert raw(capi, ctx, idx, rec, None, 1) == RTGO_E_STATE
    assert raw(capi, ctx, idx, rec, None, 1, 1) == RTGO_E_STATE
    ctx.close()
