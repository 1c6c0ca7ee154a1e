"""rtgo_whitted_update_mesh on the MI355X: a mesh refitted to moved vertices against the same mesh set afresh.

Any tree over the same triangles returns the same closest hit (smallest t, then lowest index), so a refitted mesh renders bit for bit
like a freshly built one: every comparison here is an equality, none has a tolerance.  Over unchanged vertices the refit reproduces the
build's own arrays (every box either build writes is a fminf / fmaxf union of padded triangle bounds), so there the build digests are
equal span for span."""
import numpy as np
import pytest

import accel_check as A
import trace_rays_ref as R
import whitted_big_meshes as BM
import whitted_instances as WI
import whitted_scene
from test_trace_rays import Knob

pytestmark = pytest.mark.gpu

W, H = 96, 64
SHIFT = np.float32([37.0, -5.0, 11.0])
EYE, LOOKAT = np.float32([0.5, 3.0, 7.0]), np.float32([0.0, 1.0, 0.0])
TMIN, TMAX = np.float32(0.01), np.float32(1e16)
MODES = (0, 1, 2)
E_INVALID, E_STATE, E_UNSUPPORTED = r"\(1\)", r"\(3\)", r"\(4\)"


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


# ---- meshes --------------------------------------------------------------------------------------------------------------------
def grid_mesh(q=64):
    """2 q^2 triangles (8192: the limit of one build) of a wavy sheet over [-3, 3]^2 with vertex normals"""
    g = np.linspace(-3.0, 3.0, q + 1)
    X, Z = np.meshgrid(g, g, indexing="ij")
    Y = 0.8 + 0.3 * np.sin(1.7 * X) * np.cos(1.3 * Z)
    n = np.stack([-0.51 * np.cos(1.7 * X) * np.cos(1.3 * Z), np.ones_like(X), 0.39 * np.sin(1.7 * X) * np.sin(1.3 * Z)], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    i, j = np.arange(q)[:, None], np.arange(q)[None, :]
    a, b, c, d = i * (q + 1) + j, (i + 1) * (q + 1) + j, (i + 1) * (q + 1) + j + 1, i * (q + 1) + j + 1
    tris = np.stack([np.stack([a, d, c], -1), np.stack([a, c, b], -1)], axis=2).reshape(-1, 3)
    base = whitted_scene.build()
    return {"positions": np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(np.float32), "normals": n.reshape(-1, 3).astype(np.float32),
            "indices": tris.astype(np.uint32), "tri_material": (np.arange(len(tris)) // 2 % 3).astype(np.uint32), "materials": base["materials"]}


def leaf_quad():
    """textured_quad()'s first four triangles: one leaf, no records"""
    m = whitted_scene.textured_quad()
    return dict(m, indices=m["indices"][:4], tri_material=m["tri_material"][:4])


# name -> (mesh, RTGO_WHITTED_NO_SAH)
MESHES = {"sah": (whitted_scene.build, None), "morton": (whitted_scene.build, 1), "quad": (whitted_scene.textured_quad, None),
          "leaf": (leaf_quad, None), "grid8192": (grid_mesh, None)}


def make(name):
    fn, no_sah = MESHES[name]
    mesh = dict(fn())
    lights = whitted_scene.build()
    mesh["lights"], mesh["miss"] = lights["lights"], lights["miss"]   # two point lights for every mesh
    return mesh, Knob(RTGO_WHITTED_NO_SAH=no_sah)


def smooth(mesh):
    """a sine displacement along the normals (+y where the mesh has none) and a translation: bounds, pad and 16-bit grid all move"""
    p = mesh["positions"].astype(np.float64)
    n = mesh["normals"].astype(np.float64) if mesh.get("normals") is not None else np.tile([0.0, 1.0, 0.0], (len(p), 1))
    d = 0.15 * np.sin(3.0 * p[:, 0] + 2.0 * p[:, 2] + p[:, 1])
    return (p + d[:, None] * n + SHIFT).astype(np.float32)


def camera(oracle, shift=0.0):
    return whitted_scene.camera(oracle, W, H, eye=tuple(EYE + np.float32(shift)), lookat=tuple(LOOKAT + np.float32(shift)))


# ---- contexts and comparisons --------------------------------------------------------------------------------------------------
def mesh_ctx(capi, mesh, cam):
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
    if mesh.get("texcoords") is not None:
        ctx.whitted_set_texcoords(mesh["texcoords"])
    for mi, (bc, mr, nm) in (mesh.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    view(ctx, mesh, cam)
    return ctx


def view(ctx, extra, cam):
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)


def frames(ctx):
    """subframes 0 and 1: accumulation buffer, image, (rays_total, rays_occlusion)"""
    ctx.reset_stats()
    for sf in range(2):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    st = ctx.stats()
    return ctx.read_accum(H, W), ctx.read_image(H, W), (st["rays_total"], st["rays_occlusion"])


def same_frames(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accumulation differs"
    assert np.array_equal(a[1], b[1]), what + ": image differs"
    assert a[2] == b[2], what + ": ray counts differ %r %r" % (a[2], b[2])


def same_pixels(refit, fresh, miss, what, modes=MODES):
    for mode in modes:
        with Knob(RTGO_WHITTED_MODE=mode):
            a, b = frames(refit), frames(fresh)
        same_frames(a, b, "%s, RTGO_WHITTED_MODE=%d" % (what, mode))
        hit = (b[0][..., :3] != np.float32(miss)).any(axis=-1).mean()
        assert hit > 0.1 and b[2][1] > 0, (what, "the frame shows too little of the mesh", hit, b[2])


def same_rays(capi, refit, fresh, cam, what):
    o, d = R.primaries(cam, W, H)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    a, b = refit.whitted_trace_rays(rays), fresh.whitted_trace_rays(rays)
    for f in ("t", "prim", "u", "v"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (what, "closest hits differ in", f)
    assert (b["prim"] >= 0).mean() > 0.1, what
    x, y = refit.whitted_trace_rays(rays, capi.TRACE_ANY_HIT), fresh.whitted_trace_rays(rays, capi.TRACE_ANY_HIT)
    assert np.array_equal(x["prim"] >= 0, y["prim"] >= 0) and np.array_equal(x["prim"] >= 0, b["prim"] >= 0), (what, "any-hit mask")


def no_violations(v, what):
    assert len(v) == 0, "%s: %d violations, first: %s" % (what, len(v), list(v)[:5])


def refit_against_fresh(capi, oracle, name, new_positions, what, shift=0.0, new_normals=None, fresh_normals=None):
    """mesh `name` refitted to new_positions (new_normals: None keeps them) against a fresh context over them"""
    mesh, knob = make(name)
    cam = camera(oracle, shift)
    new = dict(mesh, positions=np.ascontiguousarray(new_positions, np.float32))
    if fresh_normals is not None:
        new["normals"] = fresh_normals
    with knob:
        refit = mesh_ctx(capi, mesh, cam)
        refit.whitted_update_mesh(0, new["positions"], new_normals)
        fresh = mesh_ctx(capi, new, cam)
    try:
        same_pixels(refit, fresh, mesh["miss"], what)
        same_rays(capi, refit, fresh, cam, what)
        no_violations(A.check_mesh(refit.read_build(True), new), what)
    finally:
        refit.close()
        fresh.close()


# ---- case 1: identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_unchanged_vertices_reproduce_the_build_bit_for_bit(capi, name):
    mesh, knob = make(name)
    ctx = capi.Context(0)
    try:
        with knob:
            ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
        before = ctx.build_digest(True)
        n_recs = A.whitted_meta(ctx.read_build(True)["meta"])["n_recs"]
        assert (n_recs == 0) == (name == "leaf")
        ctx.whitted_update_mesh(0, mesh["positions"])
        assert list(ctx.build_digest(True)) == list(before)
        if mesh.get("normals") is not None:
            ctx.whitted_update_mesh(0, mesh["positions"], mesh["normals"])
            assert list(ctx.build_digest(True)) == list(before)
    finally:
        ctx.close()


# ---- case 2: smooth deformation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_smooth_deformation_renders_like_a_fresh_build(capi, oracle, name):
    """("quad" carries its textures through the update: the fresh context sets the same ones)"""
    mesh, _ = make(name)
    refit_against_fresh(capi, oracle, name, smooth(mesh), name + ", smooth deformation", shift=SHIFT)


# ---- case 3: adversarial --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sah", "morton"])
def test_permuted_vertices_render_like_a_fresh_build(capi, oracle, name):
    """the vertex positions permuted at random: the kept order means nothing any more and the boxes overlap everywhere"""
    mesh, _ = make(name)
    perm = np.random.RandomState(11).permutation(len(mesh["positions"]))
    refit_against_fresh(capi, oracle, name, mesh["positions"][perm], name + ", permuted vertices")


# ---- case 4: flattened ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sah", "morton"])
def test_flattened_mesh_renders_like_a_fresh_build(capi, oracle, name):
    """all y = 0: no extent on an axis, coincident triangles -- the lowest index wins the ties in either tree"""
    mesh, _ = make(name)
    flat = mesh["positions"].copy()
    flat[:, 1] = 0.0
    refit_against_fresh(capi, oracle, name, flat, name + ", flattened")


# ---- case 5: there and back -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_there_and_back_gives_the_original_build(capi, name):
    mesh, knob = make(name)
    ctx = capi.Context(0)
    try:
        with knob:
            ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
        before = list(ctx.build_digest(True))
        ctx.whitted_update_mesh(0, smooth(mesh))
        assert list(ctx.build_digest(True)) != before
        ctx.whitted_update_mesh(0, mesh["positions"])
        assert list(ctx.build_digest(True)) == before
    finally:
        ctx.close()


# ---- case 6: normals and textures -----------------------------------------------------------------------------------------------
def test_new_normals_and_kept_normals(capi, oracle):
    mesh, _ = make("sah")
    pos = smooth(mesh)
    n = mesh["normals"].astype(np.float64) + 0.3 * np.sin(5.0 * mesh["positions"].astype(np.float64)[:, [1, 2, 0]])
    new_normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    assert not np.array_equal(new_normals, mesh["normals"])
    refit_against_fresh(capi, oracle, "sah", pos, "new normals", shift=SHIFT, new_normals=new_normals, fresh_normals=new_normals)
    refit_against_fresh(capi, oracle, "sah", pos, "kept normals", shift=SHIFT, new_normals=None, fresh_normals=mesh["normals"])


def test_textures_stay_through_an_update(capi, oracle):
    mesh, _ = make("quad")
    cam = camera(oracle, SHIFT)
    new = dict(mesh, positions=smooth(mesh))
    refit = mesh_ctx(capi, mesh, cam)
    refit.whitted_update_mesh(0, new["positions"])
    fresh, bare = mesh_ctx(capi, new, cam), mesh_ctx(capi, dict(new, textures=None), cam)
    try:
        same_pixels(refit, fresh, mesh["miss"], "textured quad")
        assert not np.array_equal(frames(fresh)[1], frames(bare)[1]), "the textures do not show in this frame"
    finally:
        for c in (refit, fresh, bare):
            c.close()


# ---- case 7: instanced ----------------------------------------------------------------------------------------------------------
def test_instanced_scene(capi, oracle):
    """two meshes, four instances, the torus drawn three times (twice under a rotation and a non-uniform scale); the torus updated"""
    rng = np.random.RandomState(9)
    torus = WI.torus(16, 8)
    meshes = [WI.ground(normals=True), torus]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 0, 0), (WI.transform(np.eye(3), [-1.5, 0.6, 0.5]), 1, 1),
            (WI.transform(WI.rotation(rng) @ np.diag([1.6, 0.5, 1.0]), [0.2, 1.0, -0.5]), 1, 2),
            (WI.transform(WI.rotation(rng) @ np.diag([0.7, 1.8, 1.2]), [1.8, 1.2, 0.8]), 1, 1)]
    moved = [(WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.6 + 0.4 * k, 1.0]), [k - 1.5, 0.8, 0.4 * k]), m, off) for k, (_, m, off) in enumerate(inst)]
    moved[0] = inst[0]
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 3.5, 6.0), lookat=(0.0, 0.6, 0.0))
    p = torus["positions"].astype(np.float64)
    bent = (p + 0.08 * np.sin(9.0 * p[:, [2, 0, 1]]) * torus["normals"] + [0.3, 0.1, -0.2]).astype(np.float32)
    new_meshes = [meshes[0], dict(torus, positions=bent)]

    def scene(ms, instances):
        ctx = capi.Context(0)
        ctx.whitted_set_scene(ms, instances, mats)
        view(ctx, extra, cam)
        return ctx

    refit, fresh = scene(meshes, inst), scene(new_meshes, inst)
    try:
        before = frames(refit)
        refit.whitted_update_mesh(1, bent)
        same_pixels(refit, fresh, extra["miss"], "instanced", modes=(0, 2))
        assert not np.array_equal(frames(refit)[1], before[1])
        same_rays(capi, refit, fresh, cam, "instanced")
        no_violations(A.check_instanced(refit.read_build(True), new_meshes, inst), "instanced, refitted")
        # the mesh's new box reached the host's tables: the next top level is built from it
        refit.whitted_set_instances(moved)
        fresh.whitted_set_instances(moved)
        same_pixels(refit, fresh, extra["miss"], "instanced, moved", modes=(0, 2))
        no_violations(A.check_instanced(refit.read_build(True), new_meshes, moved), "instanced, refitted and moved")
        # unchanged vertices: the scene's arrays as they are
        digest = list(refit.build_digest(True))
        refit.whitted_update_mesh(1, bent, torus["normals"])
        refit.whitted_update_mesh(0, meshes[0]["positions"])
        assert list(refit.build_digest(True)) == digest
    finally:
        refit.close()
        fresh.close()


# ---- case 8: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(capi, oracle):
    mesh, _ = make("sah")
    nv = len(mesh["positions"])
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.RtgoError, match=E_STATE):
            ctx.whitted_update_mesh(0, mesh["positions"])
        ctx.whitted_set_mesh(mesh["positions"], None, mesh["indices"], mesh["tri_material"], mesh["materials"])   # (set without normals)
        before = list(ctx.build_digest(True))
        bad = mesh["positions"].copy()
        bad[nv // 2, 1] = np.nan
        inf = mesh["positions"].copy()
        inf[3, 0] = np.inf
        for code, args in ((E_INVALID, (1, mesh["positions"])), (E_INVALID, (0, mesh["positions"][:-1])), (E_INVALID, (0, bad)), (E_INVALID, (0, inf)),
                           (E_INVALID, (0, mesh["positions"], mesh["normals"]))):
            with pytest.raises(capi.RtgoError, match=code):
                ctx.whitted_update_mesh(*args)
            assert list(ctx.build_digest(True)) == before
        assert ctx._lib.rtgo_whitted_update_mesh(ctx._h, 0, None, None, nv) == 1
        assert list(ctx.build_digest(True)) == before
        # a NaN among the normals of a mesh that has them
        ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
        before = list(ctx.build_digest(True))
        nn = mesh["normals"].copy()
        nn[0, 2] = np.nan
        with pytest.raises(capi.RtgoError, match=E_INVALID):
            ctx.whitted_update_mesh(0, mesh["positions"], nn)
        assert list(ctx.build_digest(True)) == before
    finally:
        ctx.close()


def test_refusals_in_an_instanced_scene(capi, oracle):
    """a clustered mesh (8320 triangles) is refused; so is an update that throws an instance's box out of the float range"""
    big = BM.displaced_torus(65, 64)
    assert len(big["indices"]) == 8320
    small = WI.octahedron(0.3)
    eye = WI.transform(np.eye(3), [0, 0, 0])
    inst = [(eye, 0, 0), (WI.transform(np.diag([1e30, 1.0, 1.0]), [0, 1, 0]), 1, 0)]
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene([big, small], inst, WI.materials())
        before = list(ctx.build_digest(True))
        with pytest.raises(capi.RtgoError, match=E_UNSUPPORTED):
            ctx.whitted_update_mesh(0, big["positions"])
        assert list(ctx.build_digest(True)) == before
        with pytest.raises(capi.RtgoError, match=E_INVALID):
            ctx.whitted_update_mesh(2, small["positions"])
        with pytest.raises(capi.RtgoError, match=E_INVALID):
            ctx.whitted_update_mesh(1, small["positions"], np.ones_like(small["positions"]))
        with pytest.raises(capi.RtgoError, match=E_INVALID):
            ctx.whitted_update_mesh(1, small["positions"] * np.float32(1e10))   # 1e30 x 3e9: beyond the float range
        assert list(ctx.build_digest(True)) == before
        ctx.whitted_update_mesh(1, small["positions"] * np.float32(2.0))
        assert list(ctx.build_digest(True)) != before
    finally:
        ctx.close()
