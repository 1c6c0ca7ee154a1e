"""The whitted path over instanced meshes (rtgo_whitted_set_scene / rtgo_whitted_set_instances): sutil::Scene's two levels.
The references for an instanced scene: the instanced oracle (oracle_py.whitted_render_instanced, the kernel's arithmetic restated), and
the same scene flattened (tests/whitted_instances.py) and drawn by rtgo_whitted_set_mesh or by the flat oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import whitted_instances as WI
from parity import assert_parity, compare


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_instance_struct_layouts():
    from raytracingo_amd import capi
    assert C.sizeof(capi.WhittedInstance) == 56 and capi.WhittedInstance.mesh.offset == 48 and capi.WhittedInstance.material_offset.offset == 52
    assert C.sizeof(capi.WhittedMesh) == 56
    assert [getattr(capi.WhittedMesh, f).offset for f in ("positions", "normals", "texcoords", "n_vertices", "indices", "material_of_triangle", "n_triangles")] == \
        [0, 8, 16, 24, 32, 40, 48]
    assert capi.RTGO_WHITTED_MAX_MESHES == 256 and capi.RTGO_WHITTED_MAX_INSTANCES == 8192


def _unrotated_waterbottle():
    """the fixture's WaterBottle with make_fixture.py's half turn about y undone exactly (x and z negated): instanced under
    diag(-1, 1, -1) it is the fixture again"""
    import whitted_scene
    wb = whitted_scene.waterbottle()
    flip = np.array([-1, 1, -1], np.float32)
    obj = dict(wb, positions=wb["positions"] * flip, normals=wb["normals"] * flip)
    half_turn = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float32)
    return wb, obj, half_turn


def test_flattening_gives_back_the_fixture_bit_for_bit():
    wb, obj, half_turn = _unrotated_waterbottle()
    flat = WI.flatten([obj], [(half_turn, 0, 0)])
    assert np.array_equal(flat["positions"].view(np.uint32), wb["positions"].view(np.uint32))
    assert np.array_equal(flat["normals"].view(np.uint32), wb["normals"].view(np.uint32))
    assert np.array_equal(flat["indices"], wb["indices"]) and np.array_equal(flat["texcoords"], wb["texcoords"])


def test_split_scene_concatenates_to_the_original():
    import whitted_scene
    mesh = whitted_scene.build()
    meshes, inst = WI.split_scene(mesh)
    assert len(meshes) == 3
    flat = WI.flatten(meshes, inst)
    for k in ("positions", "normals", "indices", "tri_material"):
        assert np.array_equal(flat[k], mesh[k]), k


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _setup(ctx, mesh_like, cam, W, H):
    ctx.whitted_set_lights(mesh_like["lights"])
    ctx.whitted_set_miss_color(mesh_like["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)


def _mesh_ctx(capi, mesh, cam, W, H):
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
    if mesh.get("texcoords") is not None:
        ctx.whitted_set_texcoords(mesh["texcoords"])
    for mi, (bc, mr, nm) in (mesh.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    _setup(ctx, mesh, cam, W, H)
    return ctx


def _scene_ctx(capi, meshes, instances, materials, extra, cam, W, H, textures=None):
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, instances, materials)
    for mi, (bc, mr, nm) in (textures or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    _setup(ctx, extra, cam, W, H)
    return ctx


def _frames(ctx, W, H, n):
    ctx.reset_stats()
    for sf in range(n):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    st = ctx.stats()
    return ctx.read_accum(H, W), ctx.read_image(H, W), (st["rays_total"], st["rays_occlusion"])


def _same(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accumulation differs"
    assert np.array_equal(a[1], b[1]), what + ": image differs"
    assert a[2] == b[2], what + ": ray counts differ %r %r" % (a[2], b[2])


@pytest.mark.gpu
def test_identity_instances_are_bitwise_the_single_mesh(capi, oracle, monkeypatch):
    """whitted_scene.build()'s sphere, box and ground as three meshes under identity instances (materials by material_offset): the frame
    is bitwise rtgo_whitted_set_mesh's on the concatenated mesh, accumulation, image and ray counts, with the top level in LDS and in L2"""
    import whitted_scene
    W, H = 160, 100
    mesh = whitted_scene.build()
    cam = whitted_scene.camera(oracle, W, H)
    ref = _frames(_mesh_ctx(capi, mesh, cam, W, H), W, H, 3)
    meshes, inst = WI.split_scene(mesh)
    for mode in ("2", "0"):
        monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
        got = _frames(_scene_ctx(capi, meshes, inst, mesh["materials"], mesh, cam, W, H), W, H, 3)
        _same(got, ref, "identity instances, mode " + mode)
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
    assert ref[2][1] > 0


@pytest.mark.gpu
def test_half_turn_waterbottle_is_bitwise_the_fixture(capi, oracle):
    """the WaterBottle un-rotated exactly (x, z negated) under diag(-1, 1, -1), with its base-colour and metallic-roughness textures: Moeller-
    Trumbore and the shading arithmetic are exact under the sign flip, so the frame is bitwise the single-mesh frame.  (With the normal map
    it is not: dp/du, dp/dv stay in object space, LocalGeometry.h:118-134 -- that case is held to the instanced oracle instead,
    test_normal_mapped_waterbottle_under_a_scale_against_the_instanced_oracle.)"""
    import whitted_scene
    W, H = 160, 120
    wb, obj, half_turn = _unrotated_waterbottle()
    bc, mr, _ = wb["textures"][0]
    wb = dict(wb, textures={0: (bc, mr, None)})
    cam = whitted_scene.camera(oracle, W, H, eye=(0.12, 0.08, 0.42), lookat=(0.0, 0.0, 0.0), fov=40.0)
    ref = _frames(_mesh_ctx(capi, wb, cam, W, H), W, H, 2)
    got = _frames(_scene_ctx(capi, [obj], [(half_turn, 0, 0)], wb["materials"], wb, cam, W, H, textures=wb["textures"]), W, H, 2)
    _same(got, ref, "half-turn WaterBottle")
    on = (ref[0][..., :3] != np.float32(wb["miss"])).any(axis=-1)
    assert on.mean() > 0.1


_materials = WI.materials
_lights = WI.lights


def _against_instanced_oracle(capi, oracle, meshes, inst, mats, extra, cam, W, H, what, n=2, modes=False, monkeypatch=None):
    """the kernel against the instanced oracle: parity.assert_parity over n subframes; subframe 0 alone (no jitter): ray counts exactly
    equal and the pixels that see only the miss colour bitwise equal.  modes: the top level in LDS (RTGO_WHITTED_MODE=2) and in L2 (0)
    give bitwise one frame.  Returns the n-subframe frame."""
    textures = extra.get("textures")
    ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam, W, H, textures=textures)
    a0 = _frames(ctx, W, H, 1)
    r0 = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 1)
    assert a0[2] == (r0[2]["rays_total"], r0[2]["rays_occlusion"]), (what, "subframe 0 ray counts", a0[2], r0[2])
    miss_px = (r0[0][..., :3] == np.float32(extra["miss"])).all(axis=-1)
    assert np.array_equal(a0[0][miss_px], r0[0][miss_px]), (what, "miss pixels")
    got = _frames(ctx, W, H, n)
    ref = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, n)
    m = assert_parity(got[0], ref[0], got[1], ref[1], what=what)
    hit = (~miss_px).mean()
    print(what, "hit %.3f" % hit, m, "rays", got[2])
    if modes:
        frames = []
        for mode in ("2", "0"):
            monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
            frames.append(_frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H, textures=textures), W, H, n))
        monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
        _same(frames[0], frames[1], what + ": top level in LDS against L2")
        _same(frames[0], got, what + ": RTGO_WHITTED_MODE=2 against the default")
    return got, ref, hit


def _against_oracle(oracle, acc, img, racc, rimg, what):
    a, r = acc[..., :3].astype(np.float64), racc[..., :3].astype(np.float64)
    within = (np.abs(a - r) <= 1e-3 * np.maximum(1.0, np.abs(r))).all(axis=-1).mean()
    same8 = (img[..., :3] == rimg[..., :3]).all(axis=-1).mean()
    print(what, "within 1e-3: %.4f, 8-bit identical: %.4f" % (within, same8), compare(acc, racc))
    assert within >= 0.99 and same8 >= 0.99, (what, within, same8)
    return within, same8


@pytest.mark.gpu
def test_rigid_and_scaled_instances_against_the_flattened_oracle(capi, oracle, monkeypatch):
    """20 instances of a 900-triangle torus with vertex normals (18 002 triangles with the ground: past RTGO_MAX_TRIANGLES) under random
    rotations and translations, five of them uniformly and five non-uniformly scaled, above a ground they and each other shadow; against
    the oracle on the flattened scene at 96 x 64, two subframes.  Measured on an MI355X: 100 % of pixels within 1e-3 (99.95 % within
    1e-4), 99.98 % of the 8-bit image identical.  (Scales are applied only to meshes with vertex normals: without them the reference's N = W2O^T Ng is not
    unit length, LocalGeometry.h:103, 116, and has no flattened equivalent -- test_scaled_faceted_instances_against_the_instanced_oracle.)
    The same scene against the instanced oracle (measured on an MI355X: 100 % of pixels within 1e-4, 99.98 % bit-exact), top level in LDS
    and in L2 bitwise one frame."""
    import whitted_scene
    W, H = 96, 64
    meshes, inst = WI.tori_scene()
    assert len(meshes[0]["indices"]) == 900 and len(inst) == 21
    mats = _materials()
    extra = _lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5))
    acc, img, rays = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    flat = dict(WI.flatten(meshes, inst), materials=mats, **extra)
    racc, rimg, rc = oracle.whitted_render(flat, cam, W, H, 2)
    _against_oracle(oracle, acc, img, racc, rimg, "rigid and scaled")
    assert abs(rays[0] - rc["rays_total"]) <= 0.01 * rc["rays_total"]
    _against_instanced_oracle(capi, oracle, meshes, inst, mats, extra, cam, W, H, "rigid and scaled, instanced oracle", modes=True,
                              monkeypatch=monkeypatch)
    # the tori shadow the ground: against the ground alone, pixels darker by a common factor on all three channels (the ground's hue
    # kept -- a torus in front of the ground would change it: their materials are strongly coloured)
    g_acc, _, _ = _frames(_scene_ctx(capi, meshes, inst[:1], mats, extra, cam, W, H), W, H, 2)
    ratio = acc[..., :3] / np.maximum(g_acc[..., :3], 1e-6)
    shadow = (ratio.max(axis=-1) < 0.9) & (ratio.min(axis=-1) > 0.05) & (ratio.max(axis=-1) < 1.25 * ratio.min(axis=-1))
    assert shadow.sum() > 20, shadow.sum()


@pytest.mark.gpu
def test_four_thousand_instances_against_the_flattened_oracle(capi, oracle):
    """4096 instances of an 8-triangle octahedron (no vertex normals, rigid transforms) over a ground: against the flattened oracle at
    64 x 48 (measured on an MI355X: 100 % of pixels within 1e-3, 99.97 % of the 8-bit image identical), and at 1080p two contexts give
    bitwise one frame; against the instanced oracle 100 % of pixels within 1e-4 (99.93 % bit-exact)"""
    import whitted_scene
    W, H = 64, 48
    meshes, inst = WI.octahedra_scene()
    mats = _materials()
    extra = _lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.5, 5.0), lookat=(0.0, 0.2, -0.5))
    acc, img, rays = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    flat = dict(WI.flatten(meshes, inst), materials=mats, **extra)
    racc, rimg, rc = oracle.whitted_render(flat, cam, W, H, 2)
    _against_oracle(oracle, acc, img, racc, rimg, "4096 instances")
    _against_instanced_oracle(capi, oracle, meshes, inst, mats, extra, cam, W, H, "4096 instances, instanced oracle")
    W, H = 1920, 1080
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.5, 5.0), lookat=(0.0, 0.2, -0.5))
    a = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    b = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    _same(a, b, "4096 instances at 1080p, two contexts")


@pytest.mark.gpu
def test_updates_textures_and_refusals(capi, oracle):
    """rtgo_whitted_set_instances == a fresh rtgo_whitted_set_scene with those instances; rtgo_whitted_set_mesh after an instanced scene ==
    a fresh context; textures after set_scene; every refusal of rtgo_whitted_set_scene / set_instances raises"""
    import whitted_scene
    W, H = 96, 64
    mesh = whitted_scene.build()
    cam = whitted_scene.camera(oracle, W, H)
    meshes, inst = WI.split_scene(mesh)
    moved = [(WI.transform(WI.rotation(np.random.RandomState(k)), [0.3 * k, 0.1, -0.2 * k]), m, off) for k, (tr, m, off) in enumerate(inst)]
    moved.append((WI.transform(0.5 * np.eye(3), [0.0, 2.8, 0.5]), 0, 2))
    ctx = _scene_ctx(capi, meshes, inst, mesh["materials"], mesh, cam, W, H)
    _frames(ctx, W, H, 1)
    ctx.whitted_set_instances(moved)
    updated = _frames(ctx, W, H, 2)
    fresh = _frames(_scene_ctx(capi, meshes, moved, mesh["materials"], mesh, cam, W, H), W, H, 2)
    _same(updated, fresh, "set_instances against a fresh set_scene")
    # set_mesh replaces the instanced scene
    ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
    _same(_frames(ctx, W, H, 2), _frames(_mesh_ctx(capi, mesh, cam, W, H), W, H, 2), "set_mesh after set_scene")
    # ... and set_scene the single mesh
    ctx.whitted_set_scene(meshes, inst, mesh["materials"])
    _same(_frames(ctx, W, H, 2), _frames(_mesh_ctx(capi, mesh, cam, W, H), W, H, 2), "set_scene after set_mesh")
    # textures on an instanced scene: per-mesh texture coordinates, a texture on material 0 (the ground)
    quad = whitted_scene.textured_quad()
    qmeshes = [dict(quad, tri_material=quad["tri_material"])]
    tctx = _scene_ctx(capi, qmeshes, [(np.eye(3, 4, dtype=np.float32), 0, 0)], quad["materials"], quad, cam, W, H, textures=quad["textures"])
    tref = _mesh_ctx(capi, quad, cam, W, H)
    _same(_frames(tctx, W, H, 2), _frames(tref, W, H, 2), "textured quads, instanced")
    with pytest.raises(capi.RtgoError):
        tctx.whitted_set_texcoords(quad["texcoords"])          # per mesh in an instanced scene
    # refusals
    eye = np.eye(3, 4, dtype=np.float32)
    mats = mesh["materials"]
    bad = [
        (meshes, [(eye, 3, 0)], mats),                                        # mesh index beyond the array
        (meshes, [(eye, 0, 3)], mats),                                        # offset + material index reaches the table's end
        (meshes, [(np.full((3, 4), np.nan, np.float32), 0, 0)], mats),         # non-finite transform
        (meshes, [(np.zeros((3, 4), np.float32), 0, 0)], mats),                # singular transform
        (meshes, [(np.diag([1.0, 0.0, 1.0]).astype(np.float32) @ eye, 0, 0)], mats),
        (meshes, [(eye, 0, 0)] * 8193, mats),                                 # too many instances
        ([meshes[0]] * 257, [(eye, 0, 0)], mats),                             # too many meshes
        (meshes, [], mats),                                                   # no instances
        ([dict(meshes[0], indices=np.array([[0, 1, 100000]], np.uint32))], [(eye, 0, 0)], mats),   # index beyond the vertices
    ]
    c2 = capi.Context(0)
    with pytest.raises(capi.RtgoError):
        c2.whitted_launch(W, H, 0)                                            # no scene
    with pytest.raises(capi.RtgoError):
        c2.whitted_set_instances([(eye, 0, 0)])                               # no instanced scene
    for k, (ms, ins, mt) in enumerate(bad):
        with pytest.raises(capi.RtgoError):
            c2.whitted_set_scene(ms, ins, mt)
    ctx2 = _scene_ctx(capi, meshes, inst, mats, mesh, cam, W, H)
    for ms, ins, mt in bad[:6]:
        with pytest.raises(capi.RtgoError):
            ctx2.whitted_set_instances(ins)
    # a refused update leaves the scene as it was
    _same(_frames(ctx2, W, H, 2), _frames(_mesh_ctx(capi, mesh, cam, W, H), W, H, 2), "after refused updates")


# ---- GPU against the instanced oracle ----------------------------------------------------------------------------------------------
def _faceted_box():
    """a closed cube of 12 triangles, no vertex normals"""
    p = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, c, d in quads:
        tris += [(a, b, c), (a, c, d)]
    return {"positions": p, "normals": None, "indices": np.array(tris, np.uint32), "tri_material": None}


@pytest.mark.gpu
def test_scaled_faceted_instances_against_the_instanced_oracle(capi, oracle, monkeypatch):
    """octahedra and cubes without vertex normals under non-uniform scales: N = W2O^T Ng is not unit length (LocalGeometry.h:103, 116),
    which no flattened scene expresses"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(31)
    meshes = [WI.octahedron(0.4), _faceted_box(), WI.ground(6.0)]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 2, 0)]
    for k in range(12):
        S = np.diag([0.4 + 1.6 * rng.rand(), 0.3 + rng.rand(), 0.5 + 1.5 * rng.rand()])
        inst.append((WI.transform(WI.rotation(rng) @ S @ WI.rotation(rng), [-2.2 + 0.9 * (k % 6), 0.6 + 0.3 * (k // 6), -1.0 + 1.2 * (k // 6)]), k % 2, 1 + k % 3))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.0, 5.0), lookat=(0.0, 0.5, -0.3))
    _, _, hit = _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "scaled faceted", modes=True, monkeypatch=monkeypatch)
    assert hit > 0.5


@pytest.mark.gpu
def test_normal_mapped_waterbottle_under_a_scale_against_the_instanced_oracle(capi, oracle, monkeypatch):
    """the WaterBottle with all three textures, normal map included, under a rotation and a non-uniform scale: dp/du, dp/dv stay in object
    space beside the world N (LocalGeometry.h:118-134, whitted.cu:288-292)"""
    import whitted_scene
    W, H = 96, 80
    wb = whitted_scene.waterbottle()
    A = WI.rotation(np.random.RandomState(2)) @ np.diag([1.3, 0.8, 1.1])
    inst = [(WI.transform(A, [0.01, -0.02, 0.0]), 0, 0)]
    cam = whitted_scene.camera(oracle, W, H, eye=(0.12, 0.08, 0.45), lookat=(0.0, 0.0, 0.0), fov=40.0)
    extra = {"lights": wb["lights"], "miss": wb["miss"], "textures": wb["textures"]}
    _, _, hit = _against_instanced_oracle(capi, oracle, [wb], inst, wb["materials"], extra, cam, W, H, "normal-mapped WaterBottle", modes=True,
                                          monkeypatch=monkeypatch)
    assert hit > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [True, False], ids=["smooth", "faceted"])
def test_mirrored_instances_against_the_instanced_oracle(capi, oracle, monkeypatch, smooth):
    """rigid transforms with det < 0, tori with vertex normals and faceted octahedra (whose W2O^T Ng points opposite to the world
    triangle's own normal), and a scaled mirror"""
    import whitted_scene
    W, H = 96, 64
    meshes, inst = WI.mirrored_scene(smooth, n=10)
    _, inst2 = WI.mirrored_scene(smooth, n=5, scale=[1.3, 0.7, 0.9], seed=6)
    shift = np.array([[0, 0, 0, 0.3], [0, 0, 0, 0.4], [0, 0, 0, 1.7]], np.float32)
    inst = inst + [(tr + shift, m, o) for tr, m, o in inst2[1:]]
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.5, 5.5), lookat=(0.0, 0.5, -0.3))
    _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "mirrored " + ("smooth" if smooth else "faceted"),
                              modes=True, monkeypatch=monkeypatch)


@pytest.mark.gpu
def test_mixed_meshes_against_the_instanced_oracle(capi, oracle, monkeypatch):
    """one scene whose meshes differ: normals on some only (tori with, octahedra and a cube without), texture coordinates on some only
    (the textured quads with them, a cube without) with a base-colour texture on a material both use -- the cube's UV is then its
    barycentrics (LocalGeometry.h:97-102)"""
    import whitted_scene
    W, H = 96, 64
    quad = whitted_scene.textured_quad()
    qmesh = {k: quad[k] for k in ("positions", "normals", "texcoords", "indices", "tri_material")}
    meshes = [WI.torus(20, 10), WI.octahedron(0.35), _faceted_box(), qmesh, WI.ground(6.0, normals=True)]
    mats = np.concatenate([_materials(), quad["materials"]])
    extra = dict(_lights(), textures={4 + k: v for k, v in quad["textures"].items()})
    rng = np.random.RandomState(17)
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 4, 0), (WI.transform(0.7 * np.eye(3), [0.0, 0.2, -2.0]), 3, 4)]
    for k in range(12):
        mi = k % 3
        A = WI.rotation(rng) @ np.diag([1.0, 0.8 + 0.4 * rng.rand(), 1.2])
        off = 4 if mi == 2 else 1 + k % 2     # the cube shares material 4 (base-colour texture) with the quads
        inst.append((WI.transform(A, [-2.2 + 0.9 * (k % 6), 0.6, -0.5 + 1.1 * (k // 6)]), mi, off))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.0, 5.0), lookat=(0.0, 0.5, -0.8))
    _against_instanced_oracle(capi, oracle, meshes, inst, mats, extra, cam, W, H, "mixed meshes", modes=True, monkeypatch=monkeypatch)


@pytest.mark.gpu
def test_256_distinct_meshes_against_the_instanced_oracle(capi, oracle):
    """256 meshes (RTGO_WHITTED_MAX_MESHES), each its own shape -- perturbed octahedra and cubes, some with vertex normals -- one instance each"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(41)
    meshes, inst = [], []
    for k in range(256):
        m = WI.octahedron(0.12) if k % 2 else _faceted_box()
        pos = m["positions"] * (0.2 if k % 2 == 0 else 1.0) * (0.8 + 0.4 * rng.rand(*m["positions"].shape)).astype(np.float32)
        m = dict(m, positions=pos.astype(np.float32))
        if k % 4 == 1:
            m["normals"] = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(np.float32)
        if k == 0:
            m = WI.ground(5.0)
        meshes.append(m)
        t = [0, 0, 0] if k == 0 else [-3.0 + 0.4 * (k % 16), 0.2 + 0.3 * rng.rand(), -3.0 + 0.4 * (k // 16)]
        inst.append((WI.transform(np.eye(3) if k == 0 else WI.rotation(rng), t), k, 1 + k % 3 if k else 0))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.2, 3.5, 4.5), lookat=(0.0, 0.2, -0.5))
    _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "256 meshes")


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [1, 4, 5])
def test_instance_counts_at_the_top_level_edges(capi, oracle, monkeypatch, n_inst):
    """1 and 4 instances: the top level is one leaf code (no records); 5: the first count with records"""
    import whitted_scene
    W, H = 96, 64
    meshes = [WI.torus(), WI.ground(4.0, normals=True)]
    rng = np.random.RandomState(3)
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(n_inst - 1):
        inst.append((WI.transform(WI.rotation(rng) * (0.8 + 0.2 * k), [-1.5 + 1.0 * k, 0.5, -0.3 * k]), 0, 1 + k % 2))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.0, 4.5), lookat=(0.0, 0.3, -0.5))
    _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "%d instances" % n_inst, modes=True, monkeypatch=monkeypatch)


@pytest.mark.gpu
def test_meshes_of_one_four_and_five_triangles(capi, oracle, monkeypatch):
    """meshes whose root is a leaf code (1 and 4 triangles) and the smallest with a record (5), several instances of each"""
    import whitted_scene
    W, H = 96, 64
    fan = lambda n: {"positions": np.array([[0, 0, 0]] + [[np.cos(a), 0.3 * np.sin(3 * a), np.sin(a)] for a in np.linspace(0, 1.6 * np.pi, n + 1)], np.float32) * 0.5,
                     "normals": None, "indices": np.array([(0, k + 1, k + 2) for k in range(n)], np.uint32),
                     "tri_material": (np.arange(n) % 2).astype(np.uint32)}
    meshes = [fan(1), fan(4), fan(5), WI.ground(5.0)]
    assert [len(m["indices"]) for m in meshes[:3]] == [1, 4, 5]
    rng = np.random.RandomState(9)
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 3, 0)]
    for k in range(15):
        inst.append((WI.transform(WI.rotation(rng), [-2.0 + 1.0 * (k % 5), 0.7, -1.0 + 1.0 * (k // 5)]), k % 3, 1 + k % 2))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.2, 3.0, 4.5), lookat=(0.0, 0.4, -0.5))
    _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "1, 4, 5 triangles", modes=True, monkeypatch=monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["in_world_box", "in_closed_mesh"])
def test_camera_inside_an_instance(capi, oracle, monkeypatch, where):
    """the eye inside an instance's world box (the hole of a large torus) and inside a closed, non-uniformly scaled mesh (a faceted cube
    with a light inside it, wound so that its faces shade towards the inside)"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(13)
    extra = _lights()
    if where == "in_world_box":
        meshes = [WI.torus(), WI.ground(6.0, normals=True)]
        inst = [(WI.transform(np.eye(3), [0, 0, 0]), 1, 0), (WI.transform(4.0 * np.eye(3), [0.0, 1.0, 0.0]), 0, 1)]
        for k in range(8):
            inst.append((WI.transform(WI.rotation(rng) * 0.6, [-2.5 + 0.7 * k, 0.6, -3.0]), 0, 2))
        cam = whitted_scene.camera(oracle, W, H, eye=(0.0, 1.2, 0.2), lookat=(0.0, 0.8, -3.0), fov=70.0)
    else:
        meshes = [WI.swap_winding(_faceted_box()), WI.octahedron(0.3)]
        inst = [(WI.transform(WI.rotation(rng) @ np.diag([8.0, 3.0, 6.0]), [0.0, 1.0, 0.0]), 0, 0)]
        for k in range(6):
            inst.append((WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.6, 1.4]), [-1.5 + 0.6 * k, 0.8, -1.5]), 1, 1 + k % 3))
        extra["lights"] = extra["lights"].copy()
        extra["lights"][0, 4:7] = [0.5, 1.8, 0.5]
        cam = whitted_scene.camera(oracle, W, H, eye=(0.0, 1.0, 0.5), lookat=(0.0, 0.8, -1.5), fov=75.0)
    _, _, hit = _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), extra, cam, W, H, "camera " + where, modes=True,
                                          monkeypatch=monkeypatch)
    assert hit > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["far_from_origin", "scale_1e-3", "scale_1e3"])
def test_far_and_extreme_scales(capi, oracle, monkeypatch, case):
    """instances 1e4 from the origin with the camera and lights near them; the same scene under a uniform scale of 1e-3 and of 1e3 (the
    whole scene, camera and lights included, so the image is the same picture)"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(21)
    s, off = {"far_from_origin": (1.0, np.array([1.0e4, 20.0, -1.0e4])), "scale_1e-3": (1e-3, np.zeros(3)), "scale_1e3": (1e3, np.zeros(3))}[case]
    meshes = [WI.torus(), WI.octahedron(0.3), WI.ground(3.0, normals=True)]
    inst = [(WI.transform(s * np.eye(3), off), 2, 0)]
    for k in range(10):
        A = s * WI.rotation(rng)
        inst.append((WI.transform(A, off + s * np.array([-1.6 + 0.8 * (k % 5), 0.5, -0.6 + 0.9 * (k // 5)])), k % 2, 1 + k % 2))
    extra = _lights()
    extra["lights"] = extra["lights"].copy()
    extra["lights"][:, 4:7] = (off + s * (np.array([[1.0, 3.0, 2.0], [-2.0, 2.0, -1.0]]) - 0.0)).astype(np.float32)
    # whitted.cu has no falloff: the lights' intensities need no rescaling; tmin (0.01, 0.001) is absolute, so the 1e-3 scene is seen from
    # 2.5 units away through a narrow field of view
    far = 2.5e3 if case == "scale_1e-3" else 1.0
    eye = off + s * far * np.array([0.2, 1.6, 2.2])
    cam = whitted_scene.camera(oracle, W, H, eye=tuple(eye), lookat=tuple(off + s * np.array([0.0, 0.3, -0.2])), fov=45.0 / far if far > 1 else 45.0)
    _, _, hit = _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), extra, cam, W, H, case, modes=True, monkeypatch=monkeypatch)
    assert hit > 0.3


@pytest.mark.gpu
def test_exactly_zero_object_space_direction_components(capi, oracle, monkeypatch):
    """exact 90-degree rotations (signed permutation matrices: W2O is exact) and a camera whose U, V, W are exact multiples of the world
    axes: subframe 0's centre column and centre row (W, H even) have d.x = 0 or d.y = 0 exactly, and so an exact zero in d' in every
    instance (the safe_inv path of the mesh walk; test_rays_with_an_exactly_zero_direction_component is the analytic path's)"""
    import whitted_scene
    W, H = 96, 64
    meshes = [WI.torus(), WI.octahedron(0.35), _faceted_box(), WI.ground(4.0)]
    perms = [np.eye(3)[list(p)] * np.array(sg)[:, None] for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))
             for sg in ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 3, 0)]
    for k in range(20):
        P = perms[(5 * k) % len(perms)]
        t = [0.0 if k % 4 == 0 else -1.8 + 0.9 * (k % 5), 0.7 if k % 3 else 1.0, -2.0 + 0.8 * (k // 5)]
        inst.append((WI.transform(P @ np.diag([1.0, 0.7, 1.3]) if k % 2 else P, t), k % 3, 1 + k % 2))
    cam = whitted_scene.camera(oracle, W, H, eye=(0.0, 1.0, 5.0), lookat=(0.0, 1.0, 0.0), fov=50.0)
    U, V, Wv = cam[3:6], cam[6:9], cam[9:12]
    assert U[1] == 0 and U[2] == 0 and V[0] == 0 and V[2] == 0 and Wv[0] == 0 and Wv[1] == 0, cam
    for tr, _, _ in inst:
        M = WI.as34(tr)[:, :3]
        assert set(np.abs(M[M != 0]).round(6)) <= {1.0, 0.7, 1.3} and ((M != 0).sum(axis=0) == 1).all()
    # the centre column and row of subframe 0 meet instances (so their exact zeros reach the mesh walks)
    r0 = oracle.whitted_render_instanced(meshes, inst, _materials(), _lights(), cam, W, H, 1)[0]
    for line in (r0[:, W // 2], r0[H // 2, :]):
        assert (line[..., :3] != _lights()["miss"]).any(axis=-1).mean() > 0.5
    _against_instanced_oracle(capi, oracle, meshes, inst, _materials(), _lights(), cam, W, H, "zero direction components", modes=True,
                              monkeypatch=monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("x_first", [True, False], ids=["x_before_y", "y_before_x"])
def test_ties_between_instances(capi, oracle, x_first):
    """instance X draws mesh {T}, instance Y mesh {T} + S (S: far triangles behind the camera), under one transform with distinct material
    offsets, ~1000 filler instances between them in index and in space (so X and Y sit in different top-level leaves): every ray that
    meets T meets both copies at the same t, and the lower instance index must win.  The frame is bitwise that of the scene where the
    losing copy is replaced by S alone."""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(5)
    T = {"positions": np.array([[-0.8, 0.0, 0.0], [0.8, 0.0, 0.0], [0.0, 1.2, 0.0]], np.float32), "normals": None,
         "indices": np.array([[0, 1, 2]], np.uint32), "tri_material": None}
    Sp = np.array([[0, 0, 60], [1, 0, 60], [0, 1, 60], [5, 0, 60], [6, 0, 60], [5, 1, 60]], np.float32)
    S = {"positions": Sp, "normals": None, "indices": np.array([[0, 1, 2], [3, 4, 5]], np.uint32), "tri_material": None}
    TS = {"positions": np.concatenate([T["positions"], Sp]), "normals": None, "indices": np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.uint32),
          "tri_material": None}
    A = WI.rotation(rng) * 0.25 + np.diag([0.8, 0.8, 0.8])
    tr = WI.transform(A, [0.1, 0.3, 0.0])
    n_world = np.linalg.inv(A).T @ np.cross(T["positions"][1] - T["positions"][0], T["positions"][2] - T["positions"][0])
    if n_world @ (np.array([0.3, 1.0, 3.0]) - tr[:, 3]) < 0:      # T faces the camera (N = W2O^T Ng: otherwise it shades black)
        T["indices"] = T["indices"][:, [0, 2, 1]]
        TS["indices"][0] = TS["indices"][0, [0, 2, 1]]
    meshes = [T, TS, S, WI.octahedron(0.08), WI.ground(4.0)]
    fill = [(WI.transform(WI.rotation(rng), [-1.6 + 0.1 * (k % 32), 0.3, 5.0 + 1.6 * (k // 32)]), 3, 1) for k in range(1000)]   # behind the eye
    lo, hi = (0, 1) if x_first else (1, 0)     # mesh of the lower and the higher index: X = {T} or Y = {T} + S

    def scene(hi_mesh):
        return [(WI.transform(np.eye(3), [0, 0, 0]), 4, 0), (tr, lo, 2)] + fill + [(tr, hi_mesh, 3)]
    mats, extra = _materials(), _lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 1.0, 3.0), lookat=(0.2, 0.6, 0.0), fov=40.0)
    got = _frames(_scene_ctx(capi, meshes, scene(hi), mats, extra, cam, W, H), W, H, 2)
    ref = _frames(_scene_ctx(capi, meshes, scene(2), mats, extra, cam, W, H), W, H, 2)
    _same(got, ref, "ties, lower index wins")
    # the test has power: the other copy winning (the lower one replaced) gives another frame, and T covers many pixels
    lost = _frames(_scene_ctx(capi, meshes, [(WI.transform(np.eye(3), [0, 0, 0]), 4, 0), (tr, 2, 2)] + fill + [(tr, hi, 3)], mats, extra, cam, W, H), W, H, 2)
    differs = (got[0] != lost[0]).any(axis=-1).mean()
    assert differs > 0.05, differs
    racc, rimg, _ = oracle.whitted_render_instanced(meshes, scene(hi), mats, extra, cam, W, H, 2)
    assert_parity(got[0], racc, got[1], rimg, what="ties against the instanced oracle")
