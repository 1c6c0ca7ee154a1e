"""The whitted path over instanced meshes (rtgo_whitted_set_scene / rtgo_whitted_set_instances): sutil::Scene's two levels.
The reference for an instanced scene is the same scene flattened (tests/whitted_instances.py) and drawn by rtgo_whitted_set_mesh or
by the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import whitted_instances as WI
from parity import compare


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
    it is not: dp/du, dp/dv stay in object space, LocalGeometry.h:118-134 -- parity unpinned, nothing reference-held renders that case.)"""
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


def _materials():
    return np.array([[0.8, 0.8, 0.75, 1.0, 0.0, 0.9], [0.9, 0.25, 0.2, 1.0, 0.1, 0.35], [0.3, 0.5, 0.9, 1.0, 0.6, 0.3],
                     [0.95, 0.8, 0.3, 1.0, 1.0, 0.25]], np.float32)


def _lights():
    lights = np.zeros((2, 8), dtype=np.float32)
    lights[0] = [1.0, 0.95, 0.9, 2.5, 1.0, 6.0, 2.0, 0]
    lights[1] = [0.6, 0.7, 1.0, 1.0, -4.0, 3.0, -1.0, 0]
    return {"lights": lights, "miss": np.array([0.1, 0.15, 0.25], np.float32)}


def _against_oracle(oracle, acc, img, racc, rimg, what):
    a, r = acc[..., :3].astype(np.float64), racc[..., :3].astype(np.float64)
    within = (np.abs(a - r) <= 1e-3 * np.maximum(1.0, np.abs(r))).all(axis=-1).mean()
    same8 = (img[..., :3] == rimg[..., :3]).all(axis=-1).mean()
    print(what, "within 1e-3: %.4f, 8-bit identical: %.4f" % (within, same8), compare(acc, racc))
    assert within >= 0.99 and same8 >= 0.99, (what, within, same8)
    return within, same8


@pytest.mark.gpu
def test_rigid_and_scaled_instances_against_the_flattened_oracle(capi, oracle):
    """20 instances of a 900-triangle torus with vertex normals (18 002 triangles with the ground: past RTGO_MAX_TRIANGLES) under random
    rotations and translations, five of them uniformly and five non-uniformly scaled, above a ground they and each other shadow; against
    the oracle on the flattened scene at 96 x 64, two subframes.  Measured on an MI355X: 100 % of pixels within 1e-3 (99.95 % within
    1e-4), 99.98 % of the 8-bit image identical.  (Scales are applied only to meshes with vertex normals: without them the reference's N = W2O^T Ng is not
    unit length, LocalGeometry.h:103, 116, and has no flattened equivalent -- parity unpinned.)"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(7)
    tor = WI.torus()
    assert len(tor["indices"]) == 900
    meshes = [tor, WI.ground(normals=True)]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(20):
        A = WI.rotation(rng)
        if 5 <= k < 10:
            A = 0.7 * A
        elif 10 <= k < 15:
            A = A @ np.diag([1.4, 0.6, 1.0]) @ WI.rotation(rng)
        t = [-2.4 + 1.2 * (k % 5), 0.45 + 0.35 * (k // 10), -2.0 + 1.0 * (k // 5)]
        inst.append((WI.transform(A, t), 0, 1 + k % 2))
    mats = _materials()
    extra = _lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5))
    acc, img, rays = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    flat = dict(WI.flatten(meshes, inst), materials=mats, **extra)
    racc, rimg, rc = oracle.whitted_render(flat, cam, W, H, 2)
    _against_oracle(oracle, acc, img, racc, rimg, "rigid and scaled")
    assert abs(rays[0] - rc["rays_total"]) <= 0.01 * rc["rays_total"]
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
    bitwise one frame"""
    import whitted_scene
    W, H = 64, 48
    rng = np.random.RandomState(11)
    meshes = [WI.octahedron(0.09), WI.ground(8.0)]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(4095):
        t = [-3.2 + 0.1 * (k % 64), 0.15 + 0.4 * rng.rand(), -3.2 + 0.1 * (k // 64)]
        inst.append((WI.transform(WI.rotation(rng), t), 0, 1 + k % 3))
    mats = _materials()
    extra = _lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.5, 5.0), lookat=(0.0, 0.2, -0.5))
    acc, img, rays = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    flat = dict(WI.flatten(meshes, inst), materials=mats, **extra)
    racc, rimg, rc = oracle.whitted_render(flat, cam, W, H, 2)
    _against_oracle(oracle, acc, img, racc, rimg, "4096 instances")
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
