"""Clustered meshes on the whitted path: rtgo_whitted_set_scene / set_instances accept meshes beyond RTGO_MAX_TRIANGLES, up to
RTGO_WHITTED_MAX_MESH_TRIANGLES each and RTGO_WHITTED_MAX_SCENE_TRIANGLES together.  References: the oracle on the same mesh (brute force
over any number of triangles), the instanced oracle on the mesh cut into contiguous identity chunks, and -- bit for bit -- the same chunks
drawn by today's two-level path (a caller's cut into instances of at most RTGO_MAX_TRIANGLES triangles)."""
import os
import re

import numpy as np
import pytest

import whitted_big_meshes as BM
import whitted_instances as WI
from parity import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3, 4, dtype=np.float32)


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_limit_macros_match_the_binding():
    from raytracingo_amd import capi
    src = open(os.path.join(ROOT, "include", "rtgo.h")).read()
    per_mesh = re.search(r"#define RTGO_WHITTED_MAX_MESH_TRIANGLES \(1 << (\d+)\)", src)
    per_scene = re.search(r"#define RTGO_WHITTED_MAX_SCENE_TRIANGLES \(1 << (\d+)\)", src)
    assert per_mesh and per_scene
    assert capi.RTGO_WHITTED_MAX_MESH_TRIANGLES == 1 << int(per_mesh.group(1)) == 1 << 24
    assert capi.RTGO_WHITTED_MAX_SCENE_TRIANGLES == 1 << int(per_scene.group(1)) == 1 << 26
    assert re.search(r"#define RTGO_MAX_TRIANGLES 8192\b", src)   # rtgo_whitted_set_mesh keeps its cap


def _well_formed(mesh):
    p, ix = mesh["positions"], mesh["indices"]
    assert p.dtype == np.float32 and ix.dtype == np.uint32 and ix.shape[1] == 3
    assert np.isfinite(p).all() and int(ix.max()) < len(p)
    e1 = p[ix[:, 1]].astype(np.float64) - p[ix[:, 0]]
    e2 = p[ix[:, 2]].astype(np.float64) - p[ix[:, 0]]
    assert (np.linalg.norm(np.cross(e1, e2), axis=1) > 0).all()   # no degenerate triangle
    if mesh.get("normals") is not None:
        assert np.allclose(np.linalg.norm(mesh["normals"], axis=1), 1.0, atol=1e-5)
    if mesh.get("texcoords") is not None:
        assert mesh["texcoords"].shape == (len(p), 2) and np.isfinite(mesh["texcoords"]).all()


def test_procedural_meshes_are_well_formed():
    for n_u, n_v in ((200, 100), (600, 250)):
        m = BM.displaced_torus(n_u, n_v)
        assert len(m["indices"]) == 2 * n_u * n_v > 8192
        _well_formed(m)
        assert set(np.unique(m["tri_material"])) == {0, 1}
    s = BM.flat_sheet(100)
    assert len(s["indices"]) == 20000
    _well_formed(s)
    assert (s["positions"][:, 1] == 0).all()


def test_chunks_put_back_together_are_the_mesh():
    m = BM.displaced_torus(200, 100)
    parts = BM.chunks(m)
    assert [len(p["indices"]) for p, _ in parts] == [8192] * 4 + [40000 - 4 * 8192]
    idx, tm = BM.unchunk(parts)
    assert np.array_equal(idx, m["indices"]) and np.array_equal(tm, m["tri_material"])
    for p, v0 in parts:
        assert np.array_equal(p["positions"], m["positions"][v0:v0 + len(p["positions"])])
        assert np.array_equal(p["normals"], m["normals"][v0:v0 + len(p["positions"])])
        assert np.array_equal(p["texcoords"], m["texcoords"][v0:v0 + len(p["positions"])])
    meshes, inst = BM.chunked_scene([WI.ground(), m], [(EYE, 0, 0), (EYE, 1, 2), (EYE, 0, 1)], big={1})
    assert len(meshes) == 6 and [mi for _, mi, _ in inst] == [0, 1, 2, 3, 4, 5, 0]
    assert [off for _, _, off in inst] == [0] + [2] * 5 + [1]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _setup(ctx, extra, cam, W, H):
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)


def _scene_ctx(capi, meshes, instances, materials, extra, cam, W, H):
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, instances, materials)
    for mi, (bc, mr, nm) in (extra.get("textures") or {}).items():
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


def _torus_and_ground(n_u, n_v, normals=True):
    """the displaced torus and a ground quad below it as ONE mesh (the ground's two triangles last, material 2)"""
    t = BM.displaced_torus(n_u, n_v, texcoords=False)
    g = WI.ground(3.0, -0.35, normals=normals)
    nv = len(t["positions"])
    return {"positions": np.concatenate([t["positions"], g["positions"]]),
            "normals": np.concatenate([t["normals"], g["normals"]]) if normals else None,
            "indices": np.concatenate([t["indices"], g["indices"] + np.uint32(nv)]),
            "tri_material": np.concatenate([t["tri_material"], np.full(2, 2, np.uint32)])}


def _against_oracle(capi, oracle, mesh, cam, W, H, what, n=2):
    """one identity instance of `mesh` against oracle.whitted_render on the same mesh: ray counts of subframe 0 exactly, parity over n"""
    mats, extra = WI.materials(), WI.lights()
    ctx = _scene_ctx(capi, [mesh], [(EYE, 0, 0)], mats, extra, cam, W, H)
    flat = dict(mesh, materials=mats, **extra)
    a0 = _frames(ctx, W, H, 1)
    r0 = oracle.whitted_render(flat, cam, W, H, 1)
    assert a0[2] == (r0[2]["rays_total"], r0[2]["rays_occlusion"]), (what, "subframe 0 ray counts", a0[2], r0[2])
    got = _frames(ctx, W, H, n)
    ref = oracle.whitted_render(flat, cam, W, H, n)
    m = assert_parity(got[0], ref[0], got[1], ref[1], what=what)
    print(what, m, "rays", got[2])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("normals", [True, False])
def test_clustered_mesh_against_the_oracle(capi, oracle, normals):
    """a 40 002-triangle mesh (a displaced torus over a ground: ten clusters) as one instance, against the oracle on the same mesh"""
    import whitted_scene
    W, H = 96, 64
    mesh = _torus_and_ground(200, 100, normals)
    if not normals:
        mesh["normals"] = None
    cam = whitted_scene.camera(oracle, W, H, eye=(0.6, 1.5, 2.2), lookat=(0.0, -0.1, 0.0))
    got = _against_oracle(capi, oracle, mesh, cam, W, H, "clustered torus, normals %s" % normals)
    assert got[2][1] > 0


def _big_scene():
    """a 300 000-triangle displaced torus (mesh 1) under a rotation, a uniform scale and a non-uniform scale, over a ground (mesh 0)"""
    rng = np.random.RandomState(31)
    big = BM.displaced_torus(600, 250, texcoords=False)
    meshes = [WI.ground(4.0, -0.4, normals=True), big]
    inst = [(EYE, 0, 0),
            (WI.transform(WI.rotation(rng), [-1.3, 0.1, 0.0]), 1, 1),
            (WI.transform(0.7 * WI.rotation(rng), [0.2, 0.0, -0.6]), 1, 2),
            (WI.transform(WI.rotation(rng) @ np.diag([1.3, 0.6, 1.0]) @ WI.rotation(rng), [1.3, 0.2, 0.3]), 1, 0)]
    return meshes, inst


@pytest.mark.gpu
def test_big_mesh_under_transforms_against_the_instanced_oracle(capi, oracle):
    """the 300 000-triangle mesh (74 clusters) under rotated, uniformly and non-uniformly scaled instances: against the instanced oracle
    given the mesh as contiguous identity chunks composed with each instance's transform"""
    import whitted_scene
    W, H = 96, 64
    meshes, inst = _big_scene()
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 2.4, 3.6), lookat=(0.0, 0.0, -0.1))
    ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam, W, H)
    cmeshes, cinst = BM.chunked_scene(meshes, inst, big={1})
    a0 = _frames(ctx, W, H, 1)
    r0 = oracle.whitted_render_instanced(cmeshes, cinst, mats, extra, cam, W, H, 1)
    assert a0[2] == (r0[2]["rays_total"], r0[2]["rays_occlusion"]), ("subframe 0 ray counts", a0[2], r0[2])
    got = _frames(ctx, W, H, 2)
    ref = oracle.whitted_render_instanced(cmeshes, cinst, mats, extra, cam, W, H, 2)
    print("big mesh under transforms", assert_parity(got[0], ref[0], got[1], ref[1], what="big mesh under transforms"), got[2])
    # ... and bitwise the caller's cut drawn by today's path
    _same(got, _frames(_scene_ctx(capi, cmeshes, cinst, mats, extra, cam, W, H), W, H, 2), "transformed instances against the chunked scene")


@pytest.mark.gpu
def test_big_mesh_is_bitwise_the_callers_cut(capi, oracle, monkeypatch):
    """the 300 000-triangle mesh as one identity instance against the same mesh cut into contiguous 8192-triangle identity instances
    (today's path): accumulation, image and ray counts identical; the top level in LDS and in L2 bitwise; two contexts bitwise"""
    import whitted_scene
    W, H = 160, 120
    meshes, _ = _big_scene()
    mats, extra = WI.materials(), WI.lights()
    inst = [(EYE, 0, 0), (EYE, 1, 1)]
    cam = whitted_scene.camera(oracle, W, H, eye=(0.2, 1.2, 1.9), lookat=(0.0, -0.1, 0.0))
    cmeshes, cinst = BM.chunked_scene(meshes, inst, big={1})
    assert len(cinst) == 1 + 37
    ref = _frames(_scene_ctx(capi, cmeshes, cinst, mats, extra, cam, W, H), W, H, 3)
    frames = []
    for mode in ("2", "0"):
        monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
        frames.append(_frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 3))
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
    _same(frames[0], ref, "one clustered instance against the caller's cut")
    _same(frames[1], frames[0], "top level in L2 against LDS")
    _same(_frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 3), frames[0], "a second context")
    assert ref[2][1] > 0 and (ref[1][..., :3] != 0).any()


def _checker(n=8):
    t = np.zeros((n, n, 4), np.uint8)
    t[..., 3] = 255
    on = (np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0
    t[on] = [250, 240, 200, 255]
    t[~on] = [60, 120, 200, 255]
    return t


@pytest.mark.gpu
def test_mixed_scene_with_a_textured_clustered_mesh(capi, oracle):
    """small meshes of today's structure (a torus with normals, octahedra) and a 40 000-triangle clustered mesh with texture
    coordinates and a base-colour texture, in one scene: bitwise the chunked equivalent, and against the instanced oracle"""
    import whitted_scene
    W, H = 96, 64
    rng = np.random.RandomState(5)
    big = BM.displaced_torus(200, 100)
    meshes = [WI.ground(3.0, -0.4), WI.torus(), big, WI.octahedron(0.2)]
    mats = np.concatenate([WI.materials(), np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.5]], np.float32)])
    inst = [(EYE, 0, 0), (WI.transform(WI.rotation(rng), [-1.1, 0.1, 0.2]), 1, 1), (WI.transform(np.eye(3), [0.3, 0.0, -0.3]), 2, 3),
            (WI.transform(WI.rotation(rng), [1.1, 0.2, 0.4]), 3, 2), (WI.transform(0.8 * WI.rotation(rng), [-0.4, 0.5, 0.9]), 3, 1)]
    extra = dict(WI.lights(), textures={4: (_checker(), None, None)})
    cam = whitted_scene.camera(oracle, W, H, eye=(0.2, 2.0, 3.0), lookat=(0.0, 0.0, 0.0))
    ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam, W, H)
    got = _frames(ctx, W, H, 2)
    cmeshes, cinst = BM.chunked_scene(meshes, inst, big={2})
    _same(got, _frames(_scene_ctx(capi, cmeshes, cinst, mats, extra, cam, W, H), W, H, 2), "mixed scene against the chunked scene")
    ref = oracle.whitted_render_instanced(cmeshes, cinst, mats, extra, cam, W, H, 2)
    print("mixed", assert_parity(got[0], ref[0], got[1], ref[1], what="mixed scene"), got[2])


@pytest.mark.gpu
def test_instance_updates_and_refusals_with_clustered_meshes(capi, oracle):
    """set_instances on a scene with clustered meshes == a fresh set_scene with those instances; refused updates and a refused set_scene
    leave the scene as it was"""
    import whitted_scene
    W, H = 96, 64
    meshes, inst = _big_scene()
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 2.4, 3.6), lookat=(0.0, 0.0, -0.1))
    ctx = _scene_ctx(capi, meshes, inst[:2], mats, extra, cam, W, H)
    before = _frames(ctx, W, H, 2)
    ctx.whitted_set_instances(inst)
    updated = _frames(ctx, W, H, 2)
    _same(updated, _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2), "set_instances against a fresh set_scene")
    assert not np.array_equal(updated[1], before[1])
    for bad in ([(EYE, 2, 0)], [(EYE, 1, 0)] * 8193, [(EYE, 1, 3)]):
        with pytest.raises(capi.RtgoError):
            ctx.whitted_set_instances(bad)
    _same(_frames(ctx, W, H, 2), updated, "after refused updates")
    with pytest.raises(capi.RtgoError, match=r"\(4\)"):
        ctx.whitted_set_scene([dict(meshes[1], indices=np.zeros((capi.RTGO_WHITTED_MAX_MESH_TRIANGLES + 1, 3), np.uint32))], [(EYE, 0, 0)], mats)
    _same(_frames(ctx, W, H, 2), updated, "after a refused set_scene")


@pytest.mark.gpu
def test_coincident_copies_across_clusters(capi, oracle):
    """5000 coincident copies of a ground triangle appended to a 40 002-triangle mesh: their Morton keys differ only in the index, so the
    sort keeps them in index order over two clusters and more; the lowest index wins every tie, so the frame is bitwise the frame
    without the copies"""
    import whitted_scene
    W, H = 96, 64
    mesh = _torus_and_ground(200, 100)
    t = mesh["indices"][-1]
    dup = dict(mesh, indices=np.concatenate([mesh["indices"], np.tile(t, (5000, 1))]),
               tri_material=np.concatenate([mesh["tri_material"], np.full(5000, 3, np.uint32)]))   # (another material: a copy that won would show)
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.6, 1.5, 2.2), lookat=(0.0, -0.1, 0.0))
    a = _frames(_scene_ctx(capi, [mesh], [(EYE, 0, 0)], mats, extra, cam, W, H), W, H, 2)
    b = _frames(_scene_ctx(capi, [dup], [(EYE, 0, 0)], mats, extra, cam, W, H), W, H, 2)
    _same(b, a, "coincident copies")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["inside", "edge_on", "grazing"])
def test_camera_inside_the_box_and_a_flat_mesh_at_its_bounds(capi, oracle, case):
    """a camera inside the clustered mesh's box (in the torus's hole), and a flat 20 000-triangle sheet seen exactly edge-on and at a
    grazing angle (its box is the build pads alone in y): against the oracle"""
    import whitted_scene
    W, H = 96, 64
    if case == "inside":
        mesh = _torus_and_ground(200, 100)
        cam = whitted_scene.camera(oracle, W, H, eye=(0.0, 0.05, 0.0), lookat=(1.0, -0.05, 0.3), fov=70.0)
    else:
        mesh = BM.flat_sheet(100)
        eye = (0.0, 0.0, 2.5) if case == "edge_on" else (0.3, 0.02, 2.5)
        cam = whitted_scene.camera(oracle, W, H, eye=eye, lookat=(0.0, 0.0, 0.0))
    got = _against_oracle(capi, oracle, mesh, cam, W, H, "clustered, " + case)
    if case != "edge_on":
        assert got[2][1] > 0   # lit hits (the sheet faces +y)


@pytest.mark.gpu
def test_refusals_over_the_triangle_limits(capi, oracle):
    """one mesh over RTGO_WHITTED_MAX_MESH_TRIANGLES, and meshes over RTGO_WHITTED_MAX_SCENE_TRIANGLES together: RTGO_E_UNSUPPORTED (4),
    and nothing to render afterwards"""
    mats = WI.materials()
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ctx = capi.Context(0)
    over = np.zeros((capi.RTGO_WHITTED_MAX_MESH_TRIANGLES + 1, 3), np.uint32)
    with pytest.raises(capi.RtgoError, match=r"set_scene failed \(4\)"):
        ctx.whitted_set_scene([{"positions": pos, "indices": over}], [(EYE, 0, 0)], mats)
    full = over[:capi.RTGO_WHITTED_MAX_MESH_TRIANGLES]
    parts = [{"positions": pos, "indices": full}] * 4 + [{"positions": pos, "indices": np.array([[0, 1, 2]], np.uint32)}]
    with pytest.raises(capi.RtgoError, match=r"set_scene failed \(4\)"):
        ctx.whitted_set_scene(parts, [(EYE, 4, 0)], mats)
    ctx.set_camera([0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, -1])
    ctx.resize(16)
    with pytest.raises(capi.RtgoError, match=r"\(3\)"):
        ctx.whitted_launch(4, 4, 0)   # no scene was set


def _plus_one_triangle(mesh):
    """mesh with one more triangle below it, facing +y (vertex normals (0, 1, 0) when the mesh has normals)"""
    tri = np.array([[-1.5, -0.3, -1.5], [0.0, -0.3, 1.5], [1.5, -0.3, -1.5]], np.float32)
    nv = len(mesh["positions"])
    out = {"positions": np.concatenate([mesh["positions"], tri]),
           "normals": None if mesh.get("normals") is None else np.concatenate([mesh["normals"], np.tile(np.float32([0, 1, 0]), (3, 1))]),
           "indices": np.concatenate([mesh["indices"], np.array([[nv, nv + 1, nv + 2]], np.uint32)]),
           "tri_material": np.concatenate([mesh["tri_material"], np.array([2], np.uint32)])}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_tri", [8193, 16384, 16385])
def test_first_sizes_beyond_the_old_cap_are_bitwise_the_callers_cut(capi, oracle, monkeypatch, n_tri):
    """8193 and 16384 triangles: three and four clusters, a mid level that is one leaf without records; 16385: five clusters, the first
    size whose mid level has records.  Each as one identity instance is bitwise the caller's cut into contiguous 8192-triangle identity
    instances, with everything in LDS that fits and with the top level in L2"""
    import whitted_scene
    W, H = 96, 64
    n_u = 64 if n_tri < 16384 else 128
    mesh = BM.displaced_torus(n_u, 64, texcoords=False)
    if n_tri % 2:
        mesh = _plus_one_triangle(mesh)
    assert len(mesh["indices"]) == n_tri
    mats, extra = WI.materials(), WI.lights()
    inst = [(EYE, 0, 0)]
    cam = whitted_scene.camera(oracle, W, H, eye=(0.6, 1.5, 2.2), lookat=(0.0, -0.1, 0.0))
    cmeshes, cinst = BM.chunked_scene([mesh], inst, big={0})
    ref = _frames(_scene_ctx(capi, cmeshes, cinst, mats, extra, cam, W, H), W, H, 2)
    for mode in ("2", "0"):
        monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
        _same(_frames(_scene_ctx(capi, [mesh], inst, mats, extra, cam, W, H), W, H, 2), ref, "%d triangles, mode %s" % (n_tri, mode))
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
    assert ref[2][1] > 0


@pytest.mark.gpu
def test_clustered_mesh_among_instances_whose_top_level_stays_in_l2(capi, oracle, monkeypatch):
    """2400 instances of a small octahedron around one clustered 40 000-triangle instance, over a ground: the top level's InstWalk array
    alone (2402 x 64 B) and its records (at least 600 x 64 B) exceed the 160 KiB of LDS, so render_inst_kernel<false, true> runs without
    any knob.  Bitwise the caller's cut; RTGO_WHITTED_MODE=0 gives the same frame"""
    import whitted_scene
    W, H = 128, 96
    rng = np.random.RandomState(17)
    meshes = [WI.ground(4.0, -0.4), BM.displaced_torus(200, 100, texcoords=False), WI.octahedron(0.04)]
    inst = [(EYE, 0, 0), (EYE, 1, 1)]
    for k in range(2400):
        t = [-3.0 + 0.1 * (k % 60), -0.3 + 0.05 * rng.rand(), -2.0 + 0.1 * (k // 60)]
        inst.append((WI.transform(WI.rotation(rng), t), 2, 2 + k % 2))
    assert 64 * len(inst) + 64 * (len(inst) // 4 - 1) > 160 * 1024
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 2.6, 3.6), lookat=(0.0, -0.2, -0.2))
    cmeshes, cinst = BM.chunked_scene(meshes, inst, big={1})
    ref = _frames(_scene_ctx(capi, cmeshes, cinst, mats, extra, cam, W, H), W, H, 2)
    got = _frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2)
    _same(got, ref, "2400 instances and a clustered mesh against the caller's cut")
    monkeypatch.setenv("RTGO_WHITTED_MODE", "0")
    _same(_frames(_scene_ctx(capi, meshes, inst, mats, extra, cam, W, H), W, H, 2), got, "RTGO_WHITTED_MODE=0")
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
    assert ref[2][1] > 0


@pytest.mark.gpu
def test_replaced_textures_and_closed_contexts_release_their_memory(capi, oracle):
    """a material's base-colour texture set again 20 times (1024 x 1024 texels, 4 MB each) frees the texels it replaces; ten create /
    set_scene (a clustered mesh among instances) / launch / close cycles give back what they took"""
    import whitted_scene
    from test_large_scenes import hip, mem_free
    W, H = 32, 32
    meshes, inst = [WI.ground(3.0, -0.4), BM.displaced_torus(200, 100)], [(EYE, 0, 0), (EYE, 1, 1)]
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.6, 1.5, 2.2), lookat=(0.0, -0.1, 0.0))

    def rendered():
        ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam, W, H)
        ctx.whitted_launch(W, H, 0)
        ctx.sync()
        return ctx

    rendered().close()   # (the first launch of the process loads the code objects)
    Hp = hip()
    tex = np.random.RandomState(3).randint(0, 256, size=(1024, 1024, 4)).astype(np.uint8)
    ctx = rendered()
    ctx.whitted_set_material_textures(1, tex)
    free0 = mem_free(Hp)
    for _ in range(20):
        ctx.whitted_set_material_textures(1, tex)
    free1 = mem_free(Hp)
    ctx.close()
    assert free0 - free1 < 8 << 20, ("textures", free0, free1)
    free0 = mem_free(Hp)
    for _ in range(10):
        rendered().close()
    free1 = mem_free(Hp)
    assert free0 - free1 < 8 << 20, ("contexts", free0, free1)
